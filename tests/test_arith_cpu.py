"""arith_dynamic decoding (include/rans4x16_hip.h part 2g), the half that needs no GPU: the Python model
(arith_model.py) against the reference's 28 streams and the reference-made vectors of tests/golden/arith/edge.bin, the
header walk (htscodecs_amd/csrc/r4x16_arith_parse.h) as a stand-alone program under the sanitizers against the model,
the drop-in header from C and C++, and the symbols."""
import ctypes as C
import hashlib
import os
import re
import shutil
import struct
import subprocess

import pytest

import arith_cases as K
import arith_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rans4x16_hip_arith_uncompress_dev", "rans4x16_hip_arith_peek_dev", "rans4x16_hip_arith_uncompress_batch",
         "rans4x16_hip_arith_uncompress_to", "rans4x16_hip_arith_uncompress")
NO_CAP = 0xffffffff


def test_the_model_decodes_and_regenerates_the_28_reference_streams():
    fx = M.fixtures()
    assert len(fx) == 28 and {o for _, _, o, _ in fx} == {0, 1, 64, 65, 128, 129, 192, 193, 8, 9}
    for fn, base, order, stream in fx:
        text = M.text(base)
        assert M.uncompress(stream) == (0, text), fn
        assert M.compress(text, order) == stream, fn


def test_the_model_regenerates_every_constructed_stream_of_edge_bin():
    inputs, _ = K.edge()
    assert len(inputs) >= 300
    for what, order, data, stream in inputs:
        assert M.compress(data, order) == stream, (what, order)
        cap = len(data) if stream and not stream[0] & M.X_STRIPE and stream[0] & M.X_NOSZ else None
        assert M.uncompress_to(stream, cap) == (0, data), (what, order)


def test_the_model_gives_the_reference_answer_to_every_damaged_stream_of_edge_bin():
    _, damaged = K.edge()
    assert len(damaged) >= 300
    accepted = 0
    for i, (stream, cap, answer) in enumerate(damaged):
        st, out = M.uncompress_to(stream, cap)
        if answer is None:
            assert st != 0, (i, "the reference refuses this stream")
        else:
            assert st == 0, (i, st, "the reference accepts this stream")
            assert (len(out), hashlib.sha256(out).hexdigest()) == answer, i
            accepted += 1
    assert 50 <= accepted <= len(damaged) - 50                       # both answers are well represented


@pytest.fixture(scope="module")
def parse_check(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/arith_parse_check.cpp"
    exe = str(tmp_path_factory.mktemp("arith") / "arith_parse_check")
    # (the sanitizer runtimes linked in: the program stands alone whatever the environment preloads)
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "htscodecs_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "arith_parse_check.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    return exe


def test_the_walk_as_a_program_under_sanitizers_gives_the_models_statuses(parse_check, tmp_path):
    """the fixtures, every edge.bin stream and the model-made damaged streams, under three stripe reservations"""
    inputs, damaged = K.edge()
    cases = [(s, None) for _, _, _, s in M.fixtures()]
    cases += [(s, len(d) if s and not s[0] & M.X_STRIPE and s[0] & M.X_NOSZ else None) for _, _, d, s in inputs]
    cases += [(s, cap) for s, cap, _ in damaged] + list(K.model_damaged())
    cases += [(b"", 10), (b"", None)]
    limits = ((255, NO_CAP), (4, 4096), (0, 0))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for planes, stripe_out in limits:
            for s, cap in cases:
                f.write(struct.pack("<IIII", len(s), NO_CAP if cap is None else cap, planes, stripe_out) + s)
    run = subprocess.run([parse_check, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == "arith_parse_check: ok %d" % (len(limits) * len(cases)), lines[-1]
    it = iter(lines)
    refused = 0
    for planes, stripe_out in limits:
        for i, (s, cap) in enumerate(cases):
            st, out_size = [int(v) for v in next(it).split()[:2]]
            want_st, want = M.uncompress_to(s, cap, max_planes=planes, max_stripe_out=None if stripe_out == NO_CAP else stripe_out)
            assert st == want_st, (planes, i, st, want_st, s[:12].hex(), cap)
            assert out_size == len(want), (planes, i)
            refused += st != 0
    assert refused > 300


@pytest.mark.parametrize("lang,std", [("c", "-std=c99"), ("c++", "-std=c++11")])
def test_the_drop_in_header_compiles_from_c_and_cxx(lang, std, tmp_path):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    assert cc
    src = tmp_path / ("use." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "arith_dynamic_hip.h"\n'
                   "unsigned char *a(unsigned char *in, unsigned int n, unsigned int *o) { return arith_uncompress(in, n, o); }\n"
                   "unsigned char *b(unsigned char *in, unsigned int n, unsigned char *out, unsigned int *o)"
                   " { return arith_uncompress_to(in, n, out, o); }\n")
    run = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "use.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    # nothing is exported under a reference name: the object only refers to the library's own symbols
    nm = subprocess.run(["nm", str(tmp_path / "use.o")], stdout=subprocess.PIPE, text=True).stdout
    assert "rans4x16_hip_arith_uncompress" in nm and not re.search(r"\bT arith_", nm)


def test_arith_symbols_are_declared_exported_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    assert re.search(r"\bR4X16_ROUTE_ARITH\s*=\s*6\b", header)
    assert codec.ROUTE_WHICH["arith"] == 6 and codec.ROUTE_KINDS["arith"] == ("o0", "o1_lds", "o1_global", "rle")
    assert callable(codec.arith_uncompress) and callable(codec.arith_uncompress_batch)
    for meth in ("arith_uncompress", "arith_peek"):
        assert hasattr(codec.DeviceCodec, meth), meth
    for ref_name in ("arith_uncompress", "arith_uncompress_to", "arith_compress", "arith_compress_to", "arith_compress_bound"):
        assert not hasattr(L, ref_name), ref_name                    # nothing under a reference name


def test_arith_calls_refuse_cleanly_without_a_context_or_a_stream():
    import htscodecs_amd
    from htscodecs_amd import codec
    L = htscodecs_amd.load()
    assert L.rans4x16_hip_arith_uncompress_dev(None, 0, None, None, None, None, None, None, None, None, 0, 0, 0, None) == -1
    assert L.rans4x16_hip_arith_peek_dev(None, 0, None, None, None, None, None, None, 0, None) == -1
    assert L.rans4x16_hip_arith_uncompress_batch(None, 0, None, None, None, None, None) == -1
    n = C.c_uint(0)
    assert not L.rans4x16_hip_arith_uncompress(None, 0, C.byref(n))
    assert not L.rans4x16_hip_arith_uncompress(b"\x00", 0, C.byref(n))
    # what the header walk refuses is refused before any device is asked for: X_EXT, a size beyond the capacity, a
    # truncated map, a bare X_NOSZ stream without a buffer
    assert codec.arith_uncompress(bytes([M.X_EXT, 5, 1, 2, 3, 4, 5, 6, 7, 8])) is None
    assert codec.arith_uncompress(bytes([0, 50, 3, 1, 2, 3]), out_size=49) is None
    assert codec.arith_uncompress(bytes([M.X_PACK, 9, 3, 65])) is None
    assert codec.arith_uncompress(bytes([M.X_NOSZ, 3, 1, 2, 3, 4, 5, 6, 7])) is None
