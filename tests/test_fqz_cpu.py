"""fqzcomp_qual decoding (include/rans4x16_hip.h part 2i), the half that needs no GPU: the Python model (fqz_model.py)
against the reference's 16 streams and the reference-made vectors of tests/golden/fqzcomp/edge.bin and records.bin, the header walk
(htscodecs_amd/csrc/r4x16_fqz_parse.h) through the C ABI and as a stand-alone program under the sanitizers against the
model, the census of what the GPU tests decode, the drop-in header from C and C++, and the symbols."""
import collections
import ctypes as C
import hashlib
import os
import re
import shutil
import struct
import subprocess

import pytest

import fqz_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rans4x16_hip_fqz_scan", "rans4x16_hip_set_fqz_limits", "rans4x16_hip_fqz_uncompress_dev", "rans4x16_hip_fqz_peek_dev",
         "rans4x16_hip_fqz_uncompress_batch", "rans4x16_hip_fqz_decompress")
NO_CAP = 0xffffffff
# the events every list of the GPU tests must hold twice at least: the model's census (fqz_model._symbol, decompress)
EVENTS = ("qual:halve", "qual:halve_tie", "qual:swap", "qual:swap_lane", "len:swap", "sel:swap", "row:first", "row:revisit",
          "clamp:p", "clamp:delta", "ctx:wrap", "len:carried", "param:switch", "dup:taken", "dup:other_length", "rev:odd", "rev:even",
          "coder:dry", "qmap:beyond",
          # the per-record models past their first halving (a total of 65,519: record 4,080 to 4,095), the two-entry models'
          # swaps and level entries, the end pass by lane, by wave and past its first trip of 64 records: records.bin
          "len:halve", "sel:halve", "rev:halve", "dup:halve", "rev:swap", "dup:swap", "len:swap_lane", "sel:swap_lane",
          "rev:level", "dup:level", "rev:lane", "rev:wave", "rev:later_trip", "dup:wave",
          "refuse:empty", "refuse:short", "refuse:version", "refuse:nparam", "refuse:param_short", "refuse:qmap",
          "refuse:param", "refuse:len_remainder", "refuse:len_zero", "refuse:dup_length",
          "undefined:read_array", "undefined:sel_model")

_decoded = {}


def decoded(stream):
    """the model's answer to a stream, with its census: computed once, shared by the tests of this file"""
    if stream not in _decoded:
        ev = []
        st, out, lens = M.decompress(stream, events=ev)
        _decoded[stream] = (st, out, lens, collections.Counter(ev))
    return _decoded[stream]


def all_streams():
    """every stream the GPU tests decode: the fixtures, the inputs and damaged streams of edge.bin and records.bin, the
    model-made ones"""
    inputs, damaged = M.edge()
    rec_inputs, rec_damaged = M.records()
    return ([f[2] for f in M.fixtures()] + [i[4] for i in inputs] + [s for s, _ in damaged] +
            [s for s, _ in M.model_refused()] + M.model_undefined() + [i[4] for i in rec_inputs] + [s for s, _ in rec_damaged])


def test_the_model_decodes_the_16_reference_streams():
    fx = M.fixtures()
    assert len(fx) == 16
    sizes = collections.Counter()
    for fn, base, stream, want, lens in fx:
        st, out, got_lens = M.decompress(stream)
        assert (st, out, got_lens) == (0, want, lens), fn
        sizes[(len(want), len(lens))] += 1
    assert sizes == {(151000, 1000): 4, (146383, 1000): 4, (100000, 1000): 4, (62341, 100): 4}


def test_the_model_decodes_every_input_of_edge_bin():
    inputs, _ = M.edge()
    names = [i[0] for i in inputs]
    for want in ("nparam2", "nparam3", "nparam9", "nparam9+stab", "rev", "rev_then_dup_other_len", "dup_shorter", "dup_chain", "qtab",
                 "width1", "width2", "width4", "width5", "width64", "width65", "width255", "width256", "halve", "halve_tie", "lens",
                 "delta", "do_len_carried", "do_len_both", "sloc15", "starts", "empty"):
        assert want in names, want
    for name, data, lens, flags, stream, size, digest in inputs:
        st, out, got_lens, _ = decoded(stream)
        assert st == 0 and got_lens == lens and len(out) == size == sum(lens), name
        assert out == data if data is not None else hashlib.sha256(out).digest() == digest, name
    # what the fixtures do not reach
    heads = {i[0]: M.parse(i[4])[1] for i in inputs}
    assert heads["nparam9"].nparam == 9 > M.LDS_PARAMS >= heads["nparam3"].nparam == 3
    assert heads["rev"].gflags & M.GFLAG_DO_REV and heads["qtab"].p[0].pflags & M.PFLAG_HAVE_QTAB
    assert [heads["width%d" % w].max_sym + 1 for w in (1, 2, 4, 5, 64, 65, 255, 256)] == [1, 2, 4, 5, 64, 65, 255, 256]
    assert heads["sloc15"].p[0].sloc == 15 and heads["empty"].out_size == 0
    lens = next(i[2] for i in inputs if i[0] == "lens")
    assert set(lens) >= {1, 255, 256, 1023, 1024, 1025, 70000}
    starts = next(i[2] for i in inputs if i[0] == "starts")
    assert {sum(starts[:k]) % 16 for k in range(len(starts))} == set(range(16))


def test_the_model_gives_the_reference_answer_to_every_damaged_stream_of_edge_bin():
    _, damaged = M.edge()
    assert len(damaged) >= 300
    accepted, sites = 0, collections.Counter()
    for i, (stream, answer) in enumerate(damaged):
        assert M.var_get(stream, 0, len(stream))[1] <= 1 << 20 and not M.undefined(stream), i
        st, out, lens, ev = decoded(stream)
        if answer is None:
            assert st != 0, (i, "the reference refuses this stream")
            sites.update(e for e in ev if e.startswith("refuse:"))
        else:
            assert st == 0, (i, st, "the reference accepts this stream")
            assert (len(out), len(lens), hashlib.sha256(out).hexdigest()) == answer, i
            accepted += 1
    assert accepted >= 100 and len(damaged) - accepted >= 100
    # the deaths inside the loop: x >= nparam, len against the remainder, a duplicate longer than what is decoded
    assert sites["refuse:param"] >= 10 and sites["refuse:len_remainder"] >= 10 and sites["refuse:dup_length"] >= 10, sites


def coder_order(data, lens, flags):
    """the input as the coder sees it under GFLAG_DO_REV (the reversed records flipped), a record a list entry"""
    recs, at = [], 0
    for ln, f in zip(lens, flags):
        recs.append(data[at:at + ln][::-1] if f & M.FREVERSE else data[at:at + ln])
        at += ln
    return recs


def test_the_model_reproduces_every_entry_of_records_bin():
    inputs, damaged = M.records()
    by_name = {i[0]: i for i in inputs}
    assert set(by_name) >= {"records", "rev_trips", "rev_edges", "bit_swap", "dup_long"}
    for name, data, lens, flags, stream, size, digest in inputs:
        st, out, got_lens, _ = decoded(stream)
        assert st == 0 and got_lens == lens and len(out) == size == sum(lens), name
        assert out == data if data is not None else hashlib.sha256(out).digest() == digest, name
        assert data is not None or size > 4096, name
    rev = lambda fl: [bool(f & M.FREVERSE) for f in fl]

    # records: a slice's worth of short records under GFLAG_DO_REV, two parameter blocks that both select and dedup
    name, data, lens, flags, stream, size, digest = by_name["records"]
    h, ev = M.parse(stream)[1], decoded(stream)[3]
    assert len(lens) >= 6600 and size <= 100000
    assert h.gflags & M.GFLAG_DO_REV and h.nparam == 2
    for pm in h.p:
        assert pm.pflags & (M.PFLAG_DO_SEL | M.PFLAG_DO_DEDUP | M.PFLAG_DO_LEN) == M.PFLAG_DO_SEL | M.PFLAG_DO_DEDUP
    sels = collections.Counter(f >> 16 for f in flags)
    assert set(sels) == {0, 1} and min(sels.values()) >= 1000 and ev["param:switch"] >= 1000
    assert set(lens) >= {1, 2, 3, 4, 5, 6, 31, 32, 33, 63, 64, 65} and sum(ln <= 6 for ln in lens) >= 0.9 * len(lens)
    assert 0.35 <= sum(rev(flags)) / len(lens) <= 0.45
    assert ev["dup:taken"] >= 50 and h.max_sym <= 4
    for what in ("len", "sel", "rev", "dup"):
        assert ev[what + ":halve"] >= (8 if what == "len" else 2), (what, ev[what + ":halve"])

    # rev_trips: a trip that is all the wave's, one that is all the lanes', a mixed remainder with a partial last trip
    name, data, lens, flags, stream, size, digest = by_name["rev_trips"]
    ev = decoded(stream)[3]
    assert M.parse(stream)[1].gflags & M.GFLAG_DO_REV and len(lens) > 192 and len(lens) % 64
    assert all(rev(flags)[:128]) and min(lens[:64]) > 32 and max(lens[64:128]) <= 32 and set(lens[64:128]) >= {1, 2, 31, 32}
    assert ev["rev:trip_all_wave"] == 1
    tail = [(ln, r) for ln, r in zip(lens[128:], rev(flags)[128:])]
    assert {ln for ln, r in tail if r} >= {33, 64, 65, 127, 128, 129} and {r for ln, r in tail} == {False, True}
    assert rev(flags)[63] and lens[63] > 32 and rev(flags)[128] and lens[128] > 32 and lens[64] == lens[127] == 32
    # rev_edges: both sides of the first two trip boundaries long and reversed
    name, data, lens, flags, stream, size, digest = by_name["rev_edges"]
    assert M.parse(stream)[1].gflags & M.GFLAG_DO_REV and len(lens) > 128 and len(lens) % 64
    assert all(rev(flags)[k] and lens[k] > 32 for k in (63, 64, 127, 128))

    # bit_swap: the step that first halves the revcomp model moves its entry up, and so with the dup model
    name, data, lens, flags, stream, size, digest = by_name["bit_swap"]
    h, ev = M.parse(stream)[1], decoded(stream)[3]
    assert h.nparam == 1 and h.gflags & M.GFLAG_DO_REV and h.p[0].pflags & M.PFLAG_DO_DEDUP
    assert len(lens) >= 4200 and set(lens) == {1, 2}
    assert ev["rev:halve_swap"] >= 1
    assert ev["dup:halve_swap"] >= 1
    assert ev["rev:halve_tie"] == ev["dup:halve_tie"] == 0           # (no tie at a halving of a two-entry model: the README)

    # dup_long: the copy by one lane, by a full wave, by a wave's second trip; behind a duplicate; behind a reversed record
    name, data, lens, flags, stream, size, digest = by_name["dup_long"]
    assert M.parse(stream)[1].gflags & M.GFLAG_DO_REV
    recs = coder_order(data, lens, flags)
    dup = [k > 0 and recs[k] == recs[k - 1] for k in range(len(recs))]
    assert sum(dup) == decoded(stream)[3]["dup:taken"]
    assert {lens[k] for k in range(len(recs)) if dup[k]} == {1, 63, 64, 65, 200, 1025}
    assert any(dup[k] and dup[k - 1] for k in range(1, len(recs)))
    after_rev = [k for k in range(1, len(recs)) if dup[k] and rev(flags)[k - 1] and not rev(flags)[k] and lens[k] > 1]
    assert after_rev and all(recs[k] != recs[k][::-1] for k in after_rev)     # the copy is of the bytes before the end pass

    # damaged variants of `records`, the reference's answer to each; the damage lies behind the first halvings
    good = by_name["records"][4]
    assert len(damaged) >= 12
    accepted, first = 0, len(good)
    for i, (stream, answer) in enumerate(damaged):
        assert M.var_get(stream, 0, len(stream))[1] <= 1 << 20 and not M.undefined(stream), i
        same = next((k for k in range(min(len(stream), len(good))) if stream[k] != good[k]), min(len(stream), len(good)))
        assert stream != good and same >= M.parse(good)[1].hdr, i
        first = min(first, same)
        st, out, lens, ev = decoded(stream)
        if answer is None:
            assert st != 0, (i, "the reference refuses this stream")
        else:
            assert st == 0, (i, st, "the reference accepts this stream")
            assert (len(out), len(lens), hashlib.sha256(out).hexdigest()) == answer, i
            accepted += 1
    assert accepted >= 4 and len(damaged) - accepted >= 4
    ev = []
    M.decompress(good[:first], events=ev)                            # what is decoded before the coder runs dry is the intact stream's
    intact = ev[:ev.index("coder:dry")]
    for what in ("len", "sel", "rev", "dup"):
        assert what + ":halve" in intact, (what, first)


def test_the_scan_through_the_c_abi_agrees_with_the_model_on_every_stream():
    from htscodecs_amd import codec
    refused = 0
    for s in all_streams() + [s[:k] for s in all_streams()[16:60] for k in range(0, 40, 3)]:
        st, info = codec.fqz_scan(s)
        want_st, h = M.parse(s)
        assert st == want_st, (st, want_st, s[:24].hex())
        assert info["stored_size"] == h.out_size
        if st == 0:
            assert info == {"stored_size": h.out_size, "header_bytes": h.hdr, "gflags": h.gflags, "nparam": h.nparam,
                            "max_sel": h.max_sel, "max_sym": h.max_sym}
        refused += st != 0
    assert refused > 100


@pytest.fixture(scope="module")
def parse_check(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fqz_parse_check.cpp"
    exe = str(tmp_path_factory.mktemp("fqz") / "fqz_parse_check")
    # (the sanitizer runtimes linked in: the program stands alone whatever the environment preloads)
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "htscodecs_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "fqz_parse_check.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    return exe


def test_the_walk_as_a_program_under_sanitizers_gives_the_models_answers(parse_check, tmp_path):
    """every stream, every truncation of every header (and a few bytes behind it), and each stream under a capacity one
    short of its stored size"""
    streams = all_streams()
    cases = [(s, NO_CAP) for s in streams]
    seen = set()
    for s in streams:
        st, h = M.parse(s)
        head = s[:h.hdr + 8] if st == 0 else s[:64]
        if head in seen:
            continue
        seen.add(head)
        cases += [(s[:k], NO_CAP) for k in range(len(head))]
        if st == 0 and h.out_size:
            cases += [(s, h.out_size - 1), (s, h.out_size)]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for s, cap in cases:
            f.write(struct.pack("<II", len(s), cap) + s)
    run = subprocess.run([parse_check, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == "fqz_parse_check: ok %d" % len(cases), lines[-1]
    refused = 0
    for i, ((s, cap), line) in enumerate(zip(cases, lines)):
        got = [int(v) for v in line.split()]
        st, h = M.parse(s)
        if st == 0 and cap != NO_CAP and cap < h.out_size:
            st = M.E_CAPACITY
        assert got[0] == st and got[1] == h.out_size, (i, got, st, s[:24].hex(), cap)
        if st == 0:
            assert got[2:7] == [h.hdr, h.gflags, h.nparam, h.max_sel, h.max_sym], (i, got)
            tabs, want = M.flat_tables(h), 0
            assert len(tabs) == 512 + 3344 * h.nparam
            for b in tabs:
                want = (want * 31 + b) & 0xffffffff
            assert got[7] == want, (i, "the flat tables differ", s[:24].hex())
        refused += st != 0
    assert refused > 1000


def test_every_event_occurs_twice_in_what_the_gpu_tests_decode():
    total = collections.Counter()
    for s in all_streams():
        if len(s) > 20000 and M.parse(s)[1].out_size > 100000:
            continue                                                 # the large fixtures: one of each text below
        total.update(decoded(s)[3])
    for fn, base, stream, want, lens in M.fixtures():
        if fn.endswith(".1"):
            total.update(decoded(stream)[3])
    for e in EVENTS:
        assert total[e] >= 2, (e, total[e])


@pytest.mark.parametrize("lang,std", [("c", "-std=c99"), ("c++", "-std=c++11")])
def test_the_drop_in_header_compiles_from_c_and_cxx(lang, std, tmp_path):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    assert cc
    src = tmp_path / ("use." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "fqzcomp_qual_hip.h"\n'
                   "char *a(char *in, size_t n, size_t *o, int *lengths, int nl) { return fqz_decompress(in, n, o, lengths, nl); }\n")
    run = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "use.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    nm = subprocess.run(["nm", str(tmp_path / "use.o")], stdout=subprocess.PIPE, text=True).stdout
    assert "rans4x16_hip_fqz_decompress" in nm and not re.search(r"\bT fqz_", nm)
    header = open(os.path.join(ROOT, "include", "fqzcomp_qual_hip.h")).read()
    assert not re.search(r"\bfqz_compress\s*\(", header)            # decoding only


def test_fqz_symbols_are_declared_exported_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    assert re.search(r"\bR4X16_ROUTE_FQZ\s*=\s*8\b", header)
    assert codec.ROUTE_WHICH["fqz"] == 8 and codec.ROUTE_KINDS["fqz"] == M.KINDS
    assert callable(codec.fqz_scan) and callable(codec.fqz_decompress) and callable(codec.fqz_uncompress_batch)
    for meth in ("fqz_uncompress", "fqz_peek", "set_fqz_limits"):
        assert hasattr(codec.DeviceCodec, meth), meth
    for ref_name in ("fqz_decompress", "fqz_compress", "fqz_qual_stats"):
        assert not hasattr(L, ref_name), ref_name                    # nothing under a reference name


def test_fqz_calls_refuse_cleanly_without_a_context_or_a_stream():
    import htscodecs_amd
    from htscodecs_amd import codec
    L = htscodecs_amd.load()
    assert L.rans4x16_hip_fqz_uncompress_dev(None, 0, None, None, None, None, None, None, None, None, None, None, None, None, 0, 0, 0, None) == -1
    assert L.rans4x16_hip_fqz_peek_dev(None, 0, None, None, None, None, None, 0, None) == -1
    assert L.rans4x16_hip_fqz_uncompress_batch(None, 0, None, None, None, None, None, None, None, None) == -1
    assert L.rans4x16_hip_set_fqz_limits(None, 0, 0) == -1
    n = C.c_size_t(7)
    assert not L.rans4x16_hip_fqz_decompress(None, 0, C.byref(n), None, 0)
    # what the header walk refuses is refused before any device is asked for, and the stored size is reported all the same
    for s, site in M.model_refused():
        if s:
            n = C.c_size_t(7)
            assert not L.rans4x16_hip_fqz_decompress(s, len(s), C.byref(n), None, 0), site
            assert n.value == M.parse(s)[1].out_size
    for s in M.model_undefined():
        assert codec.fqz_decompress(s) is None
        assert codec.fqz_scan(s)[0] == M.E_TABLE
