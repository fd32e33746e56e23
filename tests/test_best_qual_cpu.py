"""Quality blocks: best of several methods across rANS 4x16, arith_dynamic and fqzcomp_qual (include/rans4x16_hip.h part
2n), the half that needs no GPU: what the calls refuse of a method list before they ask for a device - the list's check is
host C++ of its own (htscodecs_amd/csrc/r4x16_best_qual.h) and runs here as a stand-alone program under sanitizers
(tests/host/best_qual_check.cpp) -, the new symbols in the header, the library and the Python layer, the cross rule, and
the census of the family the GPU tests encode (best_qual_cases.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import best_any_cases as A
import best_qual_cases as Q
import fqz_best_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rans4x16_hip_compress_best_qual_packed_dev", "rans4x16_hip_best_qual_chunk_blocks", "rans4x16_hip_uncompress_qual_packed_dev",
       "rans4x16_hip_compress_best_qual_batch", "rans4x16_hip_uncompress_qual_batch")
# the lists the program offers and what the check must say of each
TAKEN = {
    "triple": "ok | rans 0 | arith 0 | fqz 0@2",
    "reversed": "ok | rans 0 | arith 0 | fqz 0@0",
    "eight": "ok | rans 1 65 | arith 1 65 | fqz 0@4 1@5 2@6 3@7",
    "one strategy": "ok | rans | arith | fqz 7@0",
    "no strategy": "ok | rans 193 | arith 193 | fqz",
    "stripes of 255 planes": "ok | rans %d | arith %d | fqz" % (8 | (255 << 8), 9 | (255 << 8)),
    "sixteen strategies among 32": "ok | rans" + " 1" * 16 + " | arith | fqz " + " ".join("%d@%d" % (j, 2 * j) for j in range(16)),
}
REFUSED = {
    "k = 0": "bad arguments",
    "k = 33": "bad arguments",
    "a NULL list": "bad arguments",
    "the rANS 4x8 tag's place": "unknown codec tag",                  # 2 << 24
    "the tag behind fqzcomp's": "unknown codec tag",                  # 4 << 24
    "the highest tag": "unknown codec tag",
    "bits above the tag": "unknown codec tag",
    "a negative word": "unknown codec tag",
    "a negative strategy": "unknown codec tag",
    "a rANS word with bit 16": "an order word above 16 bits",
    "an arith word with bit 23": "an order word above 16 bits",
    "a strategy with bit 16": "a strategy above 16 bits",
    "a strategy with bit 23": "a strategy above 16 bits",
    "a rANS stripe method of 256 planes": "more than 255 stripes",
    "an arith stripe method of 256 planes": "more than 255 stripes",
    "seventeen strategies": "more than 16 fqzcomp_qual strategies",
}
# the lists above that hold a CODEC_FQZ tag: part 2m's calls, which admit none, meet the tag before the word's own checks
WITH_FQZ = ("triple", "reversed", "eight", "one strategy", "sixteen strategies among 32", "the tag behind fqzcomp's", "bits above the tag",
            "a negative strategy", "a strategy with bit 16", "a strategy with bit 23", "seventeen strategies")


def test_the_method_lists_refusals_without_a_device(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/best_qual_check.cpp"
    exe = str(tmp_path / "best_qual_check")
    # (the sanitizer runtimes linked in: the program stands alone whatever the environment preloads)
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "htscodecs_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "best_qual_check.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    lines = run.stdout.rstrip("\n").split("\n")
    assert lines[-1] == "best_qual_check: ok", run.stdout
    got = dict(l.split(": ", 1) for l in lines[:-1])
    want = dict(TAKEN)
    want.update(REFUSED)
    # part 2m's flavour: a list without the tag gives the same line, every list with one is refused for the tag
    assert set(WITH_FQZ) <= set(want) and all(v.endswith("| fqz") for k, v in TAKEN.items() if k not in WITH_FQZ)
    for name, line in list(want.items()):
        want["2m " + name] = "unknown codec tag" if name in WITH_FQZ else line
    assert want["2m one strategy"] == want["2m seventeen strategies"] == want["2m a strategy with bit 16"] == "unknown codec tag"
    assert want["2m no strategy"] == TAKEN["no strategy"] and want["2m k = 33"] == "bad arguments" and len(want) == 2 * (len(TAKEN) + len(REFUSED))
    assert got == want


def test_the_unit_puts_the_refusal_in_front_of_the_device():
    """the calls of both parts hand their arguments to one routine under their flavour and touch nothing themselves; that
    routine's first step after the context is the list's check, and its reason goes into the error text under the call's
    name"""
    text = open(os.path.join(ROOT, "htscodecs_amd", "csrc", "r4x16_best_qual.hip")).read()
    assert 'if (const char *why = bq_split(k, methods, p, f.admit)) { c->err = std::string(who) + ": " + why; return -1; }' in text
    touches = ("hipSetDevice", "r4x16_packed_call_args", "hipLaunchKernelGGL", "r4x16_ensure", "hipMemcpy")
    for routine, who, calls in (("bq_compress_dev", "enc_dev", ("compress_best_%s_packed_dev",)), ("bq_chunk_blocks", "fit", ("best_%s_chunk_blocks",)),
                                ("bq_compress_batch", "enc_batch", ("compress_best_%s_batch",))):
        body = text[text.index("static int %s(" % routine):]
        body = body[:body.index("\n}\n")]
        check = body.index("bq_methods(c, f, f.who.%s, k, methods, &p)" % who)
        for touched in touches:
            assert touched not in body[:check], (routine, touched)
        for call in calls:
            for part, flavour in (("any", "BQ_ANY"), ("qual", "BQ_QUAL")):
                assert '"%s"' % (call % part) in text[text.index("static const BqFlavour %s = " % flavour):].split(";")[0]
                entry = text[text.index('extern "C" int rans4x16_hip_%s(' % (call % part)):]
                entry = entry[entry.index("\n{\n") + 3:entry.index("\n}\n")]
                assert entry.startswith("    return %s(c, %s, " % (routine, flavour)) and entry.count(";") == 1, (call % part, entry)


def test_the_new_symbols_are_declared_exported_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exports = open(os.path.join(ROOT, "htscodecs_amd", "csrc", "exports.map")).read()
    globs = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    so = os.path.join(ROOT, "htscodecs_amd", "librans4x16_hip.so")
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout if os.path.exists(so) else None
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert any(re.fullmatch(g.replace("*", r"\w*"), name) for g in globs), name
        assert dyn is None or re.search(r"\bT %s$" % name, dyn, flags=re.M), name
        assert hasattr(L, name) and name in hlib.SIGNATURES, name
    m = re.search(r"#define\s+R4X16_CODEC_FQZ\s+(.+)", header)
    assert m and eval(m.group(1)) == Q.CODEC_FQZ == 3 << 24 == htscodecs_amd.CODEC_FQZ
    assert Q.CODEC_FQZ & Q.CODEC_MASK == Q.CODEC_FQZ
    assert re.search(r"R4X16_ROUTE_BEST_QUAL\s*=\s*14\b", header) and re.search(r"R4X16_BEST_QUAL_KINDS\s*=\s*8\b", header)
    for k, kind in enumerate(Q.KINDS):
        assert re.search(r"\bR4X16_BEST_QUAL_%s\s*=\s*%d\b" % (kind.upper(), k), header), kind
    assert codec.ROUTE_WHICH["best_qual"] == 14 and codec.ROUTE_KINDS["best_qual"] == Q.KINDS
    assert callable(htscodecs_amd.compress_best_qual_batch) and callable(htscodecs_amd.uncompress_qual_batch)
    for meth in ("compress_best_qual_packed", "uncompress_qual_packed", "best_qual_chunk_blocks"):
        assert hasattr(codec.DeviceCodec, meth), meth
    makefile = open(os.path.join(ROOT, "htscodecs_amd", "csrc", "Makefile")).read()
    assert "r4x16_best_qual.hip" in makefile and "r4x16_best_qual.h " in makefile


def test_the_calls_refuse_a_null_context():
    import htscodecs_amd
    L = htscodecs_amd.load()
    meth = (C.c_int * 3)(*Q.TRIPLE)
    off = (C.c_uint64 * 1)()
    assert L.rans4x16_hip_compress_best_qual_packed_dev(None, 0, *([None] * 7), 4, 3, meth, None, 0, off, *([None] * 4), 0, 0, 0, None) == -1
    assert L.rans4x16_hip_best_qual_chunk_blocks(None, 4, 3, meth, 4096, 10, 0) == -1
    assert L.rans4x16_hip_uncompress_qual_packed_dev(None, 0, *([None] * 5), 0, off, *([None] * 7), 0, 0, None) == -1
    assert L.rans4x16_hip_compress_best_qual_batch(None, 0, *([None] * 5), 4, None, None, 3, meth, None, None) == -1
    assert L.rans4x16_hip_uncompress_qual_batch(None, 0, *([None] * 9)) == -1


# ---- the expectation maker ------------------------------------------------------------------------------------------------
def test_the_cross_rule():
    r0, a0, f0 = Q.TRIPLE
    both = [r0, a0, f0]
    ok = lambda out, pos: (Q.OK, out, pos)
    # the smaller stream; on equal sizes the one whose winning method stands earlier
    assert Q.cross(both, dict(rans=ok(b"aaaa", 0), arith=ok(b"bbb", 1), fqz=ok(b"cc", 2))) == (f0, b"cc", Q.OK, False)
    assert Q.cross(both, dict(rans=ok(b"aaa", 0), arith=ok(b"bbb", 1), fqz=ok(b"ccc", 2))) == (r0, b"aaa", Q.OK, True)
    assert Q.cross(both[::-1], dict(rans=ok(b"aaa", 2), arith=ok(b"bbb", 1), fqz=ok(b"ccc", 0))) == (f0, b"ccc", Q.OK, True)
    assert Q.cross(both, dict(rans=ok(b"aaaa", 0), arith=ok(b"bbb", 1), fqz=ok(b"ccc", 2))) == (a0, b"bbb", Q.OK, True)
    assert Q.cross(both, dict(rans=ok(b"aaa", 0), arith=ok(b"bbbb", 1), fqz=ok(b"cccc", 2))) == (r0, b"aaa", Q.OK, False)   # a tie among losers is none
    # an undecided fqzcomp sub-list leaves the block undecided, any other failure takes only that codec out
    assert Q.cross(both, dict(rans=ok(b"a", 0), arith=ok(b"b", 1), fqz=(Q.UNDECIDED, None, -1))) == (-1, None, Q.UNDECIDED, False)
    for st in (Q.SIZE, Q.UNSUPPORTED, 3, 7):
        assert Q.cross(both, dict(rans=ok(b"aa", 0), arith=ok(b"b", 1), fqz=(st, None, -1))) == (a0, b"b", Q.OK, False)
    # nothing left: the status of the sub-list whose first method stands first
    failed = dict(rans=(Q.UNSUPPORTED, None, -1), arith=(Q.CAPACITY, None, -1), fqz=(Q.SIZE, None, -1))
    assert Q.cross(both, failed) == (-1, None, Q.UNSUPPORTED, False)
    assert Q.cross([a0, r0, f0], failed) == (-1, None, Q.CAPACITY, False)
    assert Q.cross(both[::-1], failed) == (-1, None, Q.SIZE, False)
    # a list of one codec
    assert Q.cross([f0], dict(fqz=ok(b"cc", 0))) == (f0, b"cc", Q.OK, False)
    assert Q.cross([f0], dict(fqz=(Q.SIZE, None, -1))) == (-1, None, Q.SIZE, False)


def test_the_expectation_of_a_list_without_fqzcomp_is_part_2ms():
    for b in Q.small_blocks()[::7]:
        for methods in ([A.rans(1), A.arith(1)], [A.arith(65), A.rans(65), A.rans(0)]):
            assert Q.expect(b, methods)[:4] == A.expect(b[0], methods)


def test_the_four_fixture_slices_under_the_writers_list():
    """[rans 1, arith 1, FQZ|0..3]: fqzcomp_qual wins q4, q40+dir and q8 with the reference's own smallest stream, and
    arith_dynamic order 1 wins qvar by 153 bytes"""
    methods = [A.rans(1), A.arith(1)] + [Q.fqz(s) for s in range(4)]
    got = {}
    for name in B.SLICES:
        strat, size = B.WINNERS[name]
        block = B.fixture_slice(name)
        f = (0, B.fixture_stream(name, strat), strat, list(block[1]))
        chosen, out, st, tie, lens = Q.expect(block, methods, fqz_result=f)
        assert st == Q.OK and not tie
        got[name] = (Q.who_of(chosen), len(out))
        if Q.who_of(chosen) == "fqz":
            assert chosen == Q.fqz(strat) and out == B.fixture_stream(name, strat) and lens == list(block[1])
    assert got == {"q4": ("fqz", 9307), "q40+dir": ("fqz", 43803), "q8": ("fqz", 30012), "qvar": ("arith", 31920)}


def test_the_small_family_holds_every_outcome():
    blocks = Q.small_blocks()
    assert len(blocks) == 105
    sizes = sorted({len(b[1]) for b in blocks})
    assert sizes == [1, 2, 5, 40, 300]
    assert all(1 <= v <= 65 for b in blocks if len(b[1]) in Q.RECORDS and len(b[1]) > 1 for v in b[1])
    r, a, f, fqz_ties, ra_ties = Q.small_census()
    assert (r, a, f, fqz_ties, ra_ties) == (23, 174, 37, 46, 35)
    assert r + a + f + fqz_ties + ra_ties == 3 * len(blocks)
    assert min(r, a, f) >= 10 and fqz_ties >= 5 and ra_ties >= 5
    # the tie rule is seen from both sides: the reversed list gives the tied blocks to the other codec
    fwd = [Q.expect(b, Q.LISTS[0]) for b in blocks]
    rev = [Q.expect(b, Q.LISTS[1]) for b in blocks]
    flipped = [(x[0], y[0]) for x, y in zip(fwd, rev) if x[3]]
    assert len(flipped) >= 10 and all(y[3] == x[3] for x, y in zip(fwd, rev))
    assert all(x != y for x, y in flipped)
    assert all(x[0] == y[0] and x[1] == y[1] for x, y in zip(fwd, rev) if not x[3])
