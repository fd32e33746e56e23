"""arith_dynamic encoding, what needs no GPU (include/rans4x16_hip.h part 2h): the symbols and their bindings, the clean
refusals, the drop-in header with all five reference names, the bound against the reference's recorded values, the
capacity rule against the model's streams, and the census of the lists test_gpu_arith_enc.py encodes."""
import collections
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import arith_cases as K
import arith_enc_model as E
import arith_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rans4x16_hip_arith_compress_bound", "rans4x16_hip_arith_compress_cap", "rans4x16_hip_arith_compress_dev",
         "rans4x16_hip_arith_compress_batch", "rans4x16_hip_arith_compress_to", "rans4x16_hip_arith_compress")
BOUND_SIZES = (0, 1, 19, 20, 21, 1 << 20, (1 << 31) - 1)
BOUND_ORDERS = (0, 1, 64, 65, 128, 129, 192, 193, 8, 9, 0x408)


def test_the_six_symbols_are_declared_exported_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    assert re.search(r"\bR4X16_ROUTE_ARITH_ENC\s*=\s*7\b", header)
    assert codec.ROUTE_WHICH["arith_enc"] == 7 and codec.ROUTE_KINDS["arith_enc"] == E.KINDS
    assert codec.ROUTE_WHICH["arith"] == 6 and codec.ROUTE_KINDS["arith"] == ("o0", "o1_lds", "o1_global", "rle")
    for fn in ("arith_compress", "arith_compress_batch", "arith_compress_bound", "arith_compress_cap"):
        assert callable(getattr(codec, fn)) and callable(getattr(htscodecs_amd, fn)), fn
    assert hasattr(codec.DeviceCodec, "arith_compress")
    for ref_name in ("arith_uncompress", "arith_uncompress_to", "arith_compress", "arith_compress_to", "arith_compress_bound"):
        assert not hasattr(L, ref_name), ref_name                    # nothing under a reference name
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "htscodecs_amd", "librans4x16_hip.so")],
                              stdout=subprocess.PIPE, text=True).stdout
    assert not re.search(r"\bT arith_", exported)
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, exported), name


def test_the_calls_refuse_cleanly_without_a_context_or_a_device():
    import htscodecs_amd
    from htscodecs_amd import codec
    L = htscodecs_amd.load()
    assert L.rans4x16_hip_arith_compress_dev(None, 0, None, None, None, None, None, None, None, None, 0, None, 0, 0, None) == -1
    assert L.rans4x16_hip_arith_compress_batch(None, 0, None, None, None, None, None, None) == -1
    n = C.c_uint(64)
    assert not L.rans4x16_hip_arith_compress(b"abc", 3, None, 0)
    assert not L.rans4x16_hip_arith_compress_to(b"abc", 3, None, None, 0)
    assert not L.rans4x16_hip_arith_compress(None, 3, C.byref(n), 0)
    # what the order word refuses is refused before any device is asked for: X_EXT, more than 255 planes; and a buffer
    # below the capacity rule
    data = M.text("q8")[:100]
    assert codec.arith_compress(data, M.X_EXT) is None and codec.arith_compress(data, M.X_EXT | 1 | M.X_PACK) is None
    assert codec.arith_compress(data, M.X_STRIPE | (256 << 8)) is None
    assert codec.arith_compress(data, 1, out_size=codec.arith_compress_cap(100, 1) - 1) is None


@pytest.mark.parametrize("lang,std", [("c", "-std=c99"), ("c++", "-std=c++11")])
def test_the_drop_in_header_gives_all_five_reference_names(lang, std, tmp_path):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    assert cc
    src = tmp_path / ("use." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "arith_dynamic_hip.h"\n'
                   "unsigned char *a(unsigned char *in, unsigned int n, unsigned int *o) { return arith_uncompress(in, n, o); }\n"
                   "unsigned char *b(unsigned char *in, unsigned int n, unsigned char *out, unsigned int *o)"
                   " { return arith_uncompress_to(in, n, out, o); }\n"
                   "unsigned int c(unsigned int n, int order) { return arith_compress_bound(n, order); }\n"
                   "unsigned char *d(unsigned char *in, unsigned int n, unsigned int *o, int order) { return arith_compress(in, n, o, order); }\n"
                   "unsigned char *e(unsigned char *in, unsigned int n, unsigned char *out, unsigned int *o, int order)"
                   " { return arith_compress_to(in, n, out, o, order); }\n")
    run = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "use.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    nm = subprocess.run(["nm", str(tmp_path / "use.o")], stdout=subprocess.PIPE, text=True).stdout
    for name in ("rans4x16_hip_arith_compress_bound", "rans4x16_hip_arith_compress_to", "rans4x16_hip_arith_compress",
                 "rans4x16_hip_arith_uncompress_to", "rans4x16_hip_arith_uncompress"):
        assert re.search(r"\bU %s\b" % name, nm), name
    assert not re.search(r"\bT arith_", nm)


def _bounds():
    rows = [tuple(int(v) for v in line.split()) for line in open(os.path.join(M.GOLDEN, "bound.txt"))]
    assert [(s, o) for s, o, _ in rows] == [(s, o) for s in BOUND_SIZES for o in BOUND_ORDERS]
    return rows


def test_the_bound_is_the_references():
    from htscodecs_amd import codec
    for size, order, bound in _bounds():
        assert codec.arith_compress_bound(size, order) == bound, (size, order)


def test_the_capacity_rule_lies_between_every_stream_and_the_bound():
    from htscodecs_amd import codec
    for size, order, bound in _bounds():
        cap = codec.arith_compress_cap(size, order)
        assert size < cap <= bound, (size, order, cap, bound)
    for what, data, order, stream in E.edge_cases() + E.fixture_cases():
        cap = codec.arith_compress_cap(len(data), order)
        assert len(stream) <= cap <= codec.arith_compress_bound(len(data), order), (what, order, len(stream), cap)
    # the rule's own arithmetic
    assert codec.arith_compress_cap(100, 1) == 128 and codec.arith_compress_cap(20, 9) == 48
    assert codec.arith_compress_cap(21, 9) == 21 + 7 + 6 * 4 and codec.arith_compress_cap(1000, 9 | (255 << 8)) == 1000 + 7 + 6 * 255
    # an even order skips method 1: a plane from the third on is tried with X_PACK alone, and a short plane of 16 symbols
    # then carries a map longer than the half it saves - six bytes a plane do not hold it, 28 do
    data = E.packed_planes()
    s = M.compress(data, 8 | (8 << 8))
    assert len(data) + 7 + 6 * 8 < len(s) <= codec.arith_compress_cap(len(data), 8 | (8 << 8)) == len(data) + 7 + 28 * 8
    assert len(M.compress(data, 9 | (8 << 8))) <= len(data) + 7 + 6 * 8


@pytest.fixture(scope="module")
def census():
    """the events, the routes and the coded bodies' lengths of every list the GPU tests encode; each stream is held to
    M.compress (and to the reference's own where the list has it) on the way"""
    ev, bodies = collections.Counter(), collections.defaultdict(set)
    for cases in (E.fixture_cases(), E.edge_cases(), E.step_cases(), K.tie_cases(), E.boundary_cases(), E.rare_cases(), E.trip_cases()):
        for c in cases:
            trace = []
            s = E.compress(c[1], c[2], trace, ev)
            assert s == (c[3] if len(c) > 3 else M.compress(c[1], c[2])), c[0]
            for cand in trace:
                if cand["coded"] and not cand["stored"]:
                    bodies[cand["home"]].add(cand["body"] % 16)
    return ev, bodies


def test_census_every_event_twice_in_each_home(census):
    ev, bodies = census
    print({h: {e: ev[h, e] for e in E.EVENTS} for h in ("o0", "o1_lds", "o1_global")})
    for home in ("o0", "o1_lds", "o1_global"):
        for e in E.EVENTS:
            assert ev[home, e] >= 2, (home, e, ev[home, e])
        assert bodies[home] == set(range(16)), (home, sorted(bodies[home]))      # the dword sink's flush at every residue


def test_census_the_decision_boundary_in_each_home():
    """coded size n - 1 (coded), n and n + 1 (stored): inputs found by the seeded search, in each home twice"""
    seen = collections.Counter()
    for what, data, order in E.boundary_cases():
        trace = []
        s = E.compress(data, order, trace)
        (c,) = trace
        assert c["coded"] and c["body"] - c["n"] in (-1, 0, 1) and c["stored"] == (c["body"] >= c["n"])
        assert bool(s[0] & M.X_CAT) == c["stored"]
        seen[c["home"], c["body"] - c["n"]] += 1
    assert all(seen[h, d] == 2 for h in ("o0", "o1_lds", "o1_global") for d in (-1, 0, 1)), seen


def test_census_the_model_events_by_decoding(census):
    """encoder and decoder walk the same model: the model's own events of the step list, counted by decoding the streams"""
    ev = collections.Counter()
    for what, data, order in E.step_cases() + K.tie_cases():
        if len(data) <= 50000:
            s = M.compress(data, order)
            st, out = M.uncompress_to(s, len(data) if s[0] & M.X_NOSZ else None, events=ev)
            assert st == 0 and out == data, what
    for home in ("o0", "o1_lds", "o1_global"):
        for e in ("halve", "swap", "swap_boundary", "halve_tie"):
            assert ev[home, e] >= 2, (home, e)
