"""Best of several strategies for fqzcomp_qual encoding without a GPU (include/rans4x16_hip.h part 2l): the shared
statistics pass of htscodecs_amd/csrc/r4x16_fqz_best.hip as a stand-alone program under sanitizers against the host pick
of every strategy alone (tests/host/fqz_best_check.cpp); the winners' table from the reference's own streams; the
interface."""
import os
import re
import shutil
import struct
import subprocess

import pytest

import fqz_best_cases as B
import fqz_enc_model as E
import fqz_model as M
import fqz_pick_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rans4x16_hip_fqz_compress_best_dev", "rans4x16_hip_fqz_compress_best_packed_dev", "rans4x16_hip_fqz_best_chunk_blocks",
         "rans4x16_hip_fqz_compress_best_batch")


# ---- one statistics pass, several candidates: the arithmetic as a program under sanitizers -------------------------
@pytest.fixture(scope="module")
def best_check(tmp_path_factory):
    """the program's output lines over the 4 fixture slices and every small case of pick.bin"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fqz_best_check.cpp"
    tmp = tmp_path_factory.mktemp("fqzbest")
    exe = str(tmp / "fqz_best_check")
    # (the sanitizer runtimes linked in: the program stands alone whatever the environment preloads)
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "htscodecs_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "fqz_best_check.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    inputs = [(4, name) + B.fixture_slice(name) for name in B.SLICES] + [(c.vers, c.name, c.bytes(), c.lens, c.flags) for c in P.small_cases()]
    path = tmp / "cases.bin"
    with open(path, "wb") as f:
        for vers, name, data, lens, flags in inputs:
            f.write(struct.pack("<5I", vers, 0, len(lens), len(data), 1) + struct.pack("<%dI" % len(lens), *lens) +
                    struct.pack("<%dI" % len(flags), *flags) + bytes(data))
    run = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:]                   # no disagreement, and the sanitizers report nothing
    return run.stdout.rstrip("\n").split("\n"), inputs


def test_candidates_decided_from_shared_statistics_are_the_host_picks(best_check):
    """every candidate of [0,1,2,3], [2,0], [3,1] and [4,0] over the 4 fixture slices and the 41 small cases: status,
    parameter bytes, lengths and flags of the host pick of its strategy alone - the program exits 1 otherwise"""
    lines, inputs = best_check
    candidates = sum(len(l) for l in B.LISTS)
    assert lines[-1] == "fqz_best_check: ok %d %d" % (len(inputs), len(inputs) * candidates), lines[-1]
    assert len(inputs) == 4 + 41 and len(lines) == len(inputs) * len(B.LISTS) + 1
    rows = [l.split(" ") for l in lines[:-1]]
    for k, row in enumerate(rows):
        case, which = divmod(k, len(B.LISTS))
        assert row[:2] == [str(case), str(which)] and row[2:-2] == ["0"] * len(B.LISTS[which]), row
    # the bins are computed for a candidate that does not ask for them: [2,0] and [3,1] decide rows 2 and 3 from them
    assert all(r[-2] == "1" for r in rows) and {r[-1] for r in rows} == {"1"}


def test_the_bins_and_the_histogram_only_where_a_candidate_or_the_slice_asks():
    """what the program's `bins` and `need J` columns say under a list that asks nothing: rows 2 and 3 have do_qa = do_r2 =
    0 (fqzcomp_qual.c:199-206) - the histogram is counted for READ2 records alone"""
    rows = {0: (-1, 0), 1: (-1, 1), 2: (0, 0), 3: (0, 0), 4: (0, 0)}
    text = open(os.path.join(ROOT, "htscodecs_amd", "csrc", "r4x16_fqz_pick_dec.h")).read()
    opts = re.search(r"const int opts\[FQD_NSTRATS\]\[12\] = \{(.*?)\};", text, flags=re.S).group(1)
    got = [tuple(int(v) for v in row.split(",")) for row in re.findall(r"\{([^{}]*)\}", opts)]
    assert {k: (r[11], r[10]) for k, r in enumerate(got)} == rows


# ---- the expectation table, from the reference's streams --------------------------------------------------------------
def test_the_smallest_of_the_references_streams_per_slice():
    sizes = {name: [len(B.fixture_stream(name, s)) for s in range(4)] for name in B.SLICES}
    for name, (strat, size) in B.WINNERS.items():
        assert min(sizes[name]) == size and sizes[name].index(size) == strat and sizes[name].count(size) == 1, (name, sizes[name])
    assert B.WINNERS == {"q4": (0, 9307), "q40+dir": (1, 43803), "q8": (0, 30012), "qvar": (3, 32073)}
    assert len({s for s, size in B.WINNERS.values()}) == 3           # no row is best everywhere


def test_the_winner_is_what_the_host_pick_and_the_model_make():
    """for other inputs the expected winners come from the host pick plus the model: here on the smallest fixture slice,
    where the reference's streams say the same"""
    data, lens, flags = B.fixture_slice("qvar")
    cands = []
    for strat in range(4):
        st, par, hl, hf = P.host_pick(4, strat, data, lens, flags)
        assert st == 0 and E.verdict(data, hl, hf, par) == 0
        cands.append((0, E.compress(data, hl, hf, par)))
    assert [out for st, out in cands] == [B.fixture_stream("qvar", s) for s in range(4)]
    assert B.expect(cands) == (0, B.fixture_stream("qvar", 3), 3)


def test_the_pairs_of_pick_bin_share_one_slice():
    pairs = B.pairs()
    for a, b in pairs:
        assert (a.bytes(), a.lens, a.flags, a.vers) == (b.bytes(), b.lens, b.flags, b.vers) and (a.strat, b.strat) == (0, 1), a.name
    assert [len(a.stream) for a, b in pairs] == [1350, 1711, 1818, 2181]
    assert all(B.expect([(0, a.stream), (0, b.stream)]) == (0, a.stream, 0) for a, b in pairs)
    assert all(B.expect([(0, b.stream), (0, a.stream)]) == (0, a.stream, 1) for a, b in pairs)


def test_the_rule_that_makes_a_block_of_its_candidates():
    assert B.expect([(0, b"abc"), (0, b"ab"), (0, b"xy")]) == (0, b"ab", 1)              # the first of equals
    assert B.expect([(M.E_TABLE, None), (0, b"abc")]) == (0, b"abc", 1)                  # a refused candidate is out of the running
    assert B.expect([(M.E_TABLE, None), (M.E_SIZE, None)]) == (M.E_TABLE, None, -1)      # none left: the first one's status
    assert B.expect([(0, b"a"), (P.E_UNDECIDED, None)]) == (P.E_UNDECIDED, None, -1)
    assert B.expect([(0, b"a"), (M.E_UNSUPPORTED, None)]) == (M.E_UNSUPPORTED, None, -1)


# ---- the interface -------------------------------------------------------------------------------------------------
def test_fqz_best_symbols_are_declared_exported_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    assert re.search(r"\bR4X16_ROUTE_FQZ_BEST\s*=\s*12\b", header) and re.search(r"\bR4X16_FQZ_BEST_KINDS\s*=\s*5\b", header)
    for k, kind in enumerate(("BLOCKS", "CANDIDATES", "COUNTED", "UNDECIDED", "REFUSED")):
        assert re.search(r"\bR4X16_FQZ_BEST_%s\s*=\s*%d\b" % (kind, k), header), kind
    assert codec.ROUTE_WHICH["fqz_best"] == 12
    assert codec.ROUTE_KINDS["fqz_best"] == ("blocks", "candidates", "counted", "undecided", "refused")
    assert callable(codec.fqz_compress_best_batch) and callable(htscodecs_amd.fqz_compress_best_batch)
    for fn in ("fqz_compress_best", "fqz_compress_best_packed", "fqz_best_chunk_blocks"):
        assert hasattr(codec.DeviceCodec, fn), fn
    makefile = open(os.path.join(ROOT, "htscodecs_amd", "csrc", "Makefile")).read()
    assert "r4x16_fqz_best.hip" in makefile and "r4x16_fqz_best.h " in makefile


def test_fqz_best_calls_refuse_cleanly_without_a_context():
    import ctypes as C
    import htscodecs_amd
    L = htscodecs_amd.load()
    for strats, k in (((0, 1, 2, 3), 4), ((0,), 0), ((0,) * 17, 17), ((0, -1), 2)):
        arr = (C.c_int * len(strats))(*strats)
        assert L.rans4x16_hip_fqz_compress_best_dev(None, 0, *([None] * 7), 4, k, arr, *([None] * 7), 0, 0, None) == -1
        assert L.rans4x16_hip_fqz_compress_best_packed_dev(None, 0, *([None] * 7), 4, k, arr, None, 0, *([None] * 5), 0, 0, None) == -1
        assert L.rans4x16_hip_fqz_compress_best_batch(None, 0, *([None] * 5), 4, k, arr, *([None] * 4)) == -1
        assert L.rans4x16_hip_fqz_best_chunk_blocks(None, 4, k, 1000, 10) == -1
