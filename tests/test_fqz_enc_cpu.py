"""fqzcomp_qual encoding without a GPU (include/rans4x16_hip.h part 2j): the host's parameter choice
(rans4x16_hip_fqz_pick_parameters, htscodecs_amd/csrc/r4x16_fqz_pick.h) against the reference's own streams, the Python
model of the encode loop under parameter bytes (fqz_enc_model.py) against the same streams and against fqz_model.py, the
census of what the GPU tests encode, and the interface.

The reference's answers are the 16 streams of tests/golden/fqzcomp (vers 4, strat = the file's suffix, READ2 flags for
q40+dir from q40+dir.r2) and the inputs of edge.bin / records.bin.  strat 4 and above (the reference's all-zero row) has
no reference stream: there the bytes are held to the model's reading of them only."""
import collections
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import pytest

import arith_model as A
import fqz_enc_model as E
import fqz_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rans4x16_hip_fqz_pick_parameters", "rans4x16_hip_fqz_compress_cap", "rans4x16_hip_fqz_compress_dev",
         "rans4x16_hip_fqz_compress_batch", "rans4x16_hip_fqz_compress")
EVENTS = ("carry", "ff_pending", "ff_flush_carry", "shift2", "halve:qual", "halve_tie:qual", "halve:len", "halve:sel", "halve:rev", "halve:dup",
          "dup:taken", "len:carried", "tab_global")

_picked = {}


def picked(k):
    """fixture k under the library's pick: (file name, status, parameter bytes, lens, flags, the reference's stream, data)"""
    if k not in _picked:
        from htscodecs_amd import codec
        fn, strat, stream, data, lens, flags = E.fixture_slices()[k]
        st, par, l2, f2 = codec.fqz_pick_parameters(data, lens, flags, 4, strat)
        _picked[k] = (fn, st, par, l2, f2, stream, data)
    return _picked[k]


_streams = {}


def model_stream(k):
    """the model's stream of fixture k under the picked parameters"""
    if k not in _streams:
        fn, st, par, lens, flags, stream, data = picked(k)
        _streams[k] = E.compress(data, lens, flags, par)
    return _streams[k]


# ---- the pick against the reference ----------------------------------------------------------------------------------
def test_r2_fixture_is_what_its_readme_says():
    r2 = E.r2_flags()
    assert len(r2) == 1000 and r2.count(0) == 516 and r2.count(128) == 484


@pytest.mark.parametrize("k", range(16))
def test_pick_gives_the_references_parameter_bytes_and_the_model_its_stream(k):
    fn, st, par, lens, flags, stream, data = picked(k)
    assert st == 0, fn
    assert par == E.params_of(stream), fn
    assert lens == E.fixture_slices()[k][4]                          # the lengths were exact: no fix-up
    assert all(f & 0xffff == g for f, g in zip(flags, E.fixture_slices()[k][5]))
    assert E.verdict(data, lens, flags, par) == 0
    assert model_stream(k) == stream, fn


def test_ten_of_the_16_carry_a_selector_table_with_max_sel_1_3_and_7():
    seen = collections.Counter()
    for k in range(16):
        fn, st, par, lens, flags, stream, data = picked(k)
        h = E.parse_params(par)[1]
        if h.gflags & M.GFLAG_HAVE_STAB:
            seen[h.max_sel] += 1
            assert max(f >> 16 for f in flags) == h.max_sel and h.p[0].pflags & M.PFLAG_DO_SEL
        else:
            assert all(f >> 16 == 0 for f in flags)
    assert sum(seen.values()) == 10 and set(seen) == {1, 3, 7}, seen


def test_the_models_loop_is_fqz_models_under_the_same_parameters():
    """fqz_enc_model.compress reads parameter bytes; fqz_model.compress takes the parameters as tables.  Same streams."""
    rng_data = bytes([3, 4, 5, 4, 3, 3, 7, 8] * 30)
    lens, flags = [60, 60, 60, 60], [16, 0 | (1 << 16), 16 | (1 << 16), 0]
    gps = [M.gparams([M.param(max_sym=8, qbits=4, qshift=2, pbits=3, pshift=2, dbits=2, do_dedup=True)]),
           M.gparams([M.param(max_sym=8, qbits=4, qshift=2, do_len=True, do_sel=True), M.param(qbits=3, qshift=3, do_sel=True, qmap_of=[3, 4, 5, 7, 8])],
                     gflags=M.GFLAG_DO_REV)]
    for gp in gps:
        want = M.compress(rng_data, lens, flags, gp)
        par = M.store_parameters(gp)
        assert E.verdict(rng_data, lens, flags, par) == 0
        assert E.compress(rng_data, lens, flags, par) == want
        assert M.decompress(want)[:2] == (0, rng_data)


def test_the_model_gives_the_references_stream_for_every_input_of_edge_and_records():
    kept, hashed = E.kept_vectors(), E.hashed_vectors()
    assert len(kept) >= 25 and len(hashed) == 7
    for name, data, lens, flags, stream in kept + hashed:
        par = E.params_of(stream)
        assert E.verdict(data, lens, flags, par) == 0, name
        assert E.compress(data, lens, flags, par) == stream, name


# ---- the pick's own rules --------------------------------------------------------------------------------------------
def test_length_fix_ups_oversized_undersized_and_exact():
    from htscodecs_amd import codec
    data = bytes([10, 20, 30, 20] * 25)                              # 100 bytes
    for lens, want in (([40, 40, 40], [40, 40, 20]), ([40, 70, 40, 5], [40, 60, 0, 0]), ([30, 30], [30, 70]), ([50, 50], [50, 50]),
                       ([1000], [100])):
        st, par, l2, f2 = codec.fqz_pick_parameters(data, lens, [0] * len(lens), 4, 0)
        assert st == 0 and l2 == want, (lens, l2)


def test_vers_3_sets_do_rev_and_nothing_else():
    from htscodecs_amd import codec
    fn, strat, stream, data, lens, flags = E.fixture_slices()[12]
    st3, par3, _, _ = codec.fqz_pick_parameters(data, lens, flags, 3, strat)
    st4, par4, _, _ = codec.fqz_pick_parameters(data, lens, flags, 4, strat)
    assert st3 == st4 == 0 and par3[1] == par4[1] | M.GFLAG_DO_REV and par3[:1] + par3[2:] == par4[:1] + par4[2:]


def test_strat_4_5_and_100_give_the_same_bytes():
    """row 4 of strat_opts: all zero.  No reference stream exists for it, so the bytes are checked against the model's
    reading of them only: a stream under them decodes back."""
    from htscodecs_amd import codec
    fn, strat, stream, data, lens, flags = E.fixture_slices()[12]
    res = [codec.fqz_pick_parameters(data, lens, flags, 4, s) for s in (4, 5, 100)]
    assert all(r[0] == 0 for r in res) and res[0][1:] == res[1][1:] == res[2][1:]
    st, par, l2, f2 = res[0]
    h = E.parse_params(par)[1]
    assert h.p[0].qmask == 0 and not h.p[0].pflags & (M.PFLAG_HAVE_PTAB | M.PFLAG_HAVE_DTAB)
    assert M.decompress(E.compress(data, l2, f2, par))[:2] == (0, data)
    assert codec.fqz_pick_parameters(data, lens, flags, 4, -1)[0] == M.E_UNSUPPORTED


def test_capacity_reports_the_size_and_leaves_the_slice_alone():
    from htscodecs_amd import codec
    fn, strat, stream, data, lens, flags = E.fixture_slices()[8]
    want = E.params_of(stream)
    for cap in (0, len(want) - 1):
        st, need, l2, f2 = codec.fqz_pick_parameters(data, lens, flags, 4, strat, params_cap=cap)
        assert st == M.E_CAPACITY and need == len(want) and l2 == lens and f2 == flags
    st, par, l2, f2 = codec.fqz_pick_parameters(data, lens, flags, 4, strat, params_cap=len(want))
    assert st == 0 and par == want


# ---- the pick as a program under sanitizers --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pick_check(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fqz_pick_check.cpp"
    exe = str(tmp_path_factory.mktemp("fqzp") / "fqz_pick_check")
    # (the sanitizer runtimes linked in: the program stands alone whatever the environment preloads)
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "htscodecs_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "fqz_pick_check.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    return exe


def test_the_pick_as_a_program_under_sanitizers(pick_check, tmp_path):
    NONE = 0xffffffff
    cases = []
    for k in (0, 5, 9, 12):                                          # the four texts: q4.0, q8.1, q40+dir.1, qvar.0
        fn, strat, stream, data, lens, flags = E.fixture_slices()[k]
        cases.append((4, strat, lens, flags, data, NONE, E.params_of(stream)))
    fn, strat, stream, data, lens, flags = E.fixture_slices()[12]
    small = data[:500]
    hostile = [(4, 0, [], [], b"", NONE), (4, 0, [], [], small, NONE), (3, 1, [500], [16], small, NONE), (4, 2, [1], [0], small, NONE),
               (4, 0, [0xffffffff, 0xfffffff0, 7], [0, 128, 0], small, NONE), (4, 3, [0x7fffffff] * 5, [0] * 5, small, NONE),
               (4, 0, [0, 0, 0], [0, 0, 0], small, NONE), (4, 1, [100] * 5, [128, 0, 128, 0, 128], small, 0), (4, 1, [100] * 5, [0] * 5, small, 8)]
    cases += [h + (None,) for h in hostile]
    fn, strat, stream, data, lens, flags = E.fixture_slices()[0]
    want = E.params_of(stream)
    cases.append((4, strat, lens, flags, data, len(want) - 1, None))
    cases.append((4, strat, lens, flags, data, len(want), want))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for vers, strat, lens, flags, data, cap, _ in cases:
            f.write(struct.pack("<5I", vers, strat, len(lens), len(data), cap) + struct.pack("<%dI" % len(lens), *lens) +
                    struct.pack("<%dI" % len(flags), *flags) + bytes(data))
    run = subprocess.run([pick_check, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:]                   # the sanitizers report nothing
    lines = run.stdout.rstrip("\n").split("\n")
    assert lines[-1] == "fqz_pick_check: ok %d" % len(cases), lines[-1]
    for (vers, strat, lens, flags, data, cap, want), line in zip(cases, lines):
        got = line.split(" ")
        if want is not None:
            assert got[0] == "0" and bytes.fromhex(got[2]) == want
        if cap not in (NONE,) and want is None:
            assert got[0] == "1" and int(got[1]) > cap
        if got[0] == "0" and lens:
            l2 = list(struct.unpack(">%dI" % len(lens), bytes.fromhex(got[3])))
            assert sum(l2) == len(data)                              # the fix-ups: the lengths cover the bytes exactly
            par = bytes.fromhex(got[2])
            assert E.parse_params(par)[0] == 0


# ---- the census ----------------------------------------------------------------------------------------------------
def test_every_event_occurs_twice_in_what_the_gpu_tests_encode():
    """over the very inputs test_gpu_fqz_enc.py encodes: the 16 fixtures under picked parameters, every input of edge.bin
    and records.bin (kept and hashed), the census slice and the drop-in case"""
    from htscodecs_amd import codec
    total = collections.Counter()                                    # from nothing: every input counted once
    for k in range(16):
        fn, st, par, lens, flags, stream, data = picked(k)
        assert E.compress(data, lens, flags, par, total) == stream
    for name, data, lens, flags, stream in E.kept_vectors() + E.hashed_vectors():
        assert E.compress(data, lens, flags, E.params_of(stream), total) == stream, name
    data, lens, flags, par = E.census_slice()
    assert E.verdict(data, lens, flags, par) == 0
    stream = E.compress(data, lens, flags, par, total)
    assert M.decompress(stream)[:2] == (0, data)
    data, lens, flags = E.drop_in_case()
    st, par, l2, f2 = codec.fqz_pick_parameters(data, lens, flags, 3, 0)
    assert st == 0
    E.compress(data, l2, f2, par, total)
    for e in EVENTS:
        assert total[e] >= 2, (e, total[e])


# ---- the interface -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lang,std", [("c", "-std=c99"), ("c++", "-std=c++11")])
def test_the_drop_in_header_declares_fqz_compress_for_c_and_cxx(lang, std, tmp_path):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    assert cc
    src = tmp_path / ("use." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "fqzcomp_qual_enc_hip.h"\n'
                   "char *d(char *in, size_t n, size_t *o) { return fqz_decompress(in, n, o, NULL, 0); }\n"
                   "char *a(fqz_slice *s, char *in, size_t n, size_t *o, fqz_gparams *gp) {\n"
                   "    s->flags[0] |= FQZ_FREVERSE | FQZ_FREAD2; s->len[0] = (uint32_t)n; s->num_records = 1;\n"
                   "    return fqz_compress(4, s, in, n, o, FQZ_MAX_STRAT, gp); }\n")
    run = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "use.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    nm = subprocess.run(["nm", str(tmp_path / "use.o")], stdout=subprocess.PIPE, text=True).stdout
    assert "rans4x16_hip_fqz_compress" in nm and not re.search(r"\bT fqz_", nm)
    header = open(os.path.join(ROOT, "include", "fqzcomp_qual_enc_hip.h")).read()
    assert "gp must be NULL" in header and '#include "fqzcomp_qual_hip.h"' in header        # the writer's header holds the reader's


def test_fqz_enc_symbols_are_declared_exported_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    assert re.search(r"\bR4X16_ROUTE_FQZ_ENC\s*=\s*10\b", header)
    assert codec.ROUTE_WHICH["fqz_enc"] == 10 and codec.ROUTE_KINDS["fqz_enc"] == E.KINDS
    for fn in ("fqz_pick_parameters", "fqz_compress", "fqz_compress_batch", "fqz_compress_cap"):
        assert callable(getattr(codec, fn)) and callable(getattr(htscodecs_amd, fn)), fn
    assert hasattr(codec.DeviceCodec, "fqz_compress")
    for args in ((0, 0, 9), (1, 1, 9), (151000, 1000, 300), (1 << 31, 1 << 20, 4096)):
        assert codec.fqz_compress_cap(*args) == E.cap(*args)


def test_fqz_enc_calls_refuse_cleanly_without_a_context():
    import htscodecs_amd
    L = htscodecs_amd.load()
    assert L.rans4x16_hip_fqz_compress_dev(None, 0, *([None] * 15), 0, 0, 0, None) == -1
    assert L.rans4x16_hip_fqz_compress_batch(None, 0, None, None, None, None, None, 4, 0, None, None, None, None, None) == -1
    n = C.c_size_t(7)
    assert not L.rans4x16_hip_fqz_compress(4, None, None, 0, C.byref(n), 0, None)        # no slice
    size = C.c_uint(7)
    assert L.rans4x16_hip_fqz_pick_parameters(4, 0, -1, None, None, None, 0, None, 0, C.byref(size)) == M.E_UNSUPPORTED and size.value == 0
    assert L.rans4x16_hip_fqz_pick_parameters(4, 0, 3, None, None, None, 0, None, 0, C.byref(size)) == M.E_UNSUPPORTED
    # no record and no byte: defined here (the reference reads len[0]), and the size comes back without a buffer
    assert L.rans4x16_hip_fqz_pick_parameters(4, 0, 0, None, None, None, 0, None, 0, C.byref(size)) == M.E_CAPACITY and size.value >= 9
