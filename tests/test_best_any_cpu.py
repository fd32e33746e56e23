"""Best of several methods across codecs (include/rans4x16_hip.h part 2m), the half that needs no GPU: the calls' refusal
of a NULL context, the new symbols in the header, the export map, the library and the Python layer, and the expectation maker of the
GPU tests (best_any_cases.py) against the committed reference streams.  The refusals of bad method lists and the planner's
arithmetic are asked of a context, which only a device gives: their checks are written here (check_bad_list,
check_planner) and run by test_gpu_best_any.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

import best_any_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rans4x16_hip_compress_best_any_packed_dev", "rans4x16_hip_best_any_chunk_blocks", "rans4x16_hip_uncompress_any_packed_dev",
       "rans4x16_hip_compress_best_any_batch", "rans4x16_hip_uncompress_any_batch")
# a list the calls must refuse, and the words of the refusal
BAD_LISTS = [
    ("k = 0", 0, [0], "bad arguments"),
    ("k = 33", 33, [0] * 33, "bad arguments"),
    ("a NULL list", 2, None, "bad arguments"),
    ("the rANS 4x8 tag's place", 2, [0, (2 << 24) | 1], "unknown codec tag"),
    ("the highest tag", 1, [0x0F000000], "unknown codec tag"),
    ("bits above the tag", 1, [1 << 28], "unknown codec tag"),
    ("a negative word", 1, [-1], "unknown codec tag"),
    ("a rANS word with bit 16", 2, [1, 1 | (1 << 16)], "above 16 bits"),
    ("an arith word with bit 23", 2, [1, B.arith(65 | (1 << 23))], "above 16 bits"),
    ("a rANS stripe method of 256 planes", 2, [1, 8 | (256 << 8)], "255 stripes"),
    ("an arith stripe method of 256 planes", 2, [1, B.arith(9 | (256 << 8))], "255 stripes"),
]


def _calls(L, h, k, meth, off=None):
    """every call that takes a method list, with arguments that are otherwise acceptable for an empty batch (off: the one
    entry of d_out_off such a batch has - device memory where there is a context)"""
    off = (C.c_uint64 * 1)() if off is None else off
    return [L.rans4x16_hip_compress_best_any_packed_dev(h, 0, None, None, None, None, 0, off, None, None, k, meth, None, 0, 0, None),
            L.rans4x16_hip_best_any_chunk_blocks(h, 4, k, meth, 4096, 0),
            L.rans4x16_hip_compress_best_any_batch(h, 0, None, None, None, None, k, meth, None, None)]


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
    for macro, value in (("R4X16_CODEC_RANS4X16", B.CODEC_RANS), ("R4X16_CODEC_ARITH", B.CODEC_ARITH), ("R4X16_CODEC_MASK", B.CODEC_MASK)):
        m = re.search(r"#define\s+%s\s+(.+)" % macro, header)
        assert m and eval(m.group(1)) == value, macro
    assert (htscodecs_amd.CODEC_RANS4X16, htscodecs_amd.CODEC_ARITH, htscodecs_amd.CODEC_MASK) == (B.CODEC_RANS, B.CODEC_ARITH, B.CODEC_MASK)
    assert re.search(r"R4X16_ROUTE_BEST_ANY\s*=\s*13\b", header) and re.search(r"R4X16_BEST_ANY_KINDS\s*=\s*5\b", header)
    assert codec.ROUTE_WHICH["best_any"] == 13 and codec.ROUTE_KINDS["best_any"] == ("rans", "arith", "tie", "failed", "chunks")
    assert callable(htscodecs_amd.compress_best_any_batch) and callable(htscodecs_amd.uncompress_any_batch)
    for meth in ("compress_best_any_packed", "uncompress_any_packed", "best_any_chunk_blocks"):
        assert hasattr(codec.DeviceCodec, meth), meth


def test_the_calls_refuse_a_null_context():
    import htscodecs_amd
    L = htscodecs_amd.load()
    meth = (C.c_int * 2)(1, B.arith(1))
    assert _calls(L, None, 2, meth) == [-1, -1, -1]
    off = (C.c_uint64 * 1)()
    assert L.rans4x16_hip_uncompress_any_packed_dev(None, 0, None, None, None, None, None, 0, off, None, None, None, 0, 0, None) == -1
    assert L.rans4x16_hip_uncompress_any_batch(None, 0, None, None, None, None, None, None) == -1


def _c_list(methods):
    return (C.c_int * max(len(methods), 1))(*methods) if methods is not None else None


def check_bad_list(ctx, what, k, methods, words):
    """On a context: the refusal names its reason, writes nothing and takes no memory, and an acceptable list on the same
    arguments (an empty batch) is taken - the list alone was refused."""
    import torch
    L = ctx.L
    d_off = torch.full((1,), -7, dtype=torch.int64, device="cuda:0")
    assert _calls(L, ctx.h, 2, _c_list([1, B.arith(1)]), d_off.data_ptr()) == [0, 4, 0] and d_off.item() == 0
    held = L.rans4x16_hip_workspace_bytes(ctx.h)
    d_off.fill_(-7)
    for rc in _calls(L, ctx.h, k, _c_list(methods), d_off.data_ptr()):
        assert rc == -1 and words in ctx.error(), (what, rc, ctx.error())
    torch.cuda.synchronize()
    assert d_off.item() == -7                                          # nothing was enqueued
    assert L.rans4x16_hip_workspace_bytes(ctx.h) == held


def check_planner(dc):
    """The planner never returns more than n, and does not grow when max_workspace_mb shrinks.  Host arithmetic, but on a
    context: test_gpu_best_any.py runs it."""
    keep = dc.get_option("max_workspace_mb")
    lists = ([1, B.arith(1)], [0, 1, 65, 193, B.arith(0), B.arith(1), B.arith(65), B.arith(193)], [B.arith(9), 9], [1], [B.arith(65)])
    try:
        for methods in lists:
            for n, max_in in ((0, 4096), (1, 1), (64, 4096), (1000, 65536)):
                last = None
                for mb in (keep, 4096, 64, 8, 1):
                    dc.set_option("max_workspace_mb", mb)
                    got = dc.best_any_chunk_blocks(n, methods, max_in, n * max_in)
                    assert 0 <= got <= n and (got >= 1 or n == 0), (methods, n, mb, got)
                    assert last is None or got <= last, (methods, n, mb, got, last)
                    last = got
    finally:
        dc.set_option("max_workspace_mb", keep)


# the table of the part's introduction: the reference's own streams for the same text and order word go either way
ROWS = [("q4", 64, 12878, 13360, "rans"), ("q8", 64, 33458, 35211, "rans"), ("q8", 192, 32024, 32267, "rans"),
        ("q4", 193, 10825, 10283, "arith"), ("q8", 65, 31025, 30907, "arith")]


@pytest.mark.parametrize("name,order,r_bytes,a_bytes,smaller", ROWS, ids=["%s.%d" % r[:2] for r in ROWS])
def test_the_expectation_maker_reproduces_the_fixture_rows(name, order, r_bytes, a_bytes, smaller):
    assert len(B.fixture_stream(name, B.rans(order))) == r_bytes and len(B.fixture_stream(name, B.arith(order))) == a_bytes
    for methods in ((B.rans(order), B.arith(order)), (B.arith(order), B.rans(order))):
        chosen, stream, status, tie = B.expect_fixture(name, methods)
        want = B.rans(order) if smaller == "rans" else B.arith(order)
        assert (chosen, status, tie) == (want, B.OK, False) and stream == B.fixture_stream(name, want)


def test_the_pick_rule_on_ties_skips_and_single_codecs():
    streams = {B.rans(0): b"aaaa", B.rans(1): b"bbb", B.arith(0): b"ccc", B.arith(1): b"dddd", B.rans(9): b"e", B.arith(9): b"f"}
    pick = lambda size, methods: B.pick(size, methods, streams.__getitem__)
    assert pick(8, [B.rans(0), B.rans(1), B.arith(0), B.arith(1)]) == (B.rans(1), b"bbb", B.OK, True)
    assert pick(8, [B.rans(0), B.arith(0), B.rans(1), B.arith(1)]) == (B.arith(0), b"ccc", B.OK, True)
    assert pick(8, [B.arith(1), B.rans(0)]) == (B.arith(1), b"dddd", B.OK, True)
    assert pick(8, [B.rans(0), B.arith(0)]) == (B.arith(0), b"ccc", B.OK, False)
    assert pick(7, [B.rans(9), B.arith(0)]) == (B.arith(0), b"ccc", B.OK, False)      # the stripe method is not tried
    assert pick(8, [B.rans(9), B.arith(0)]) == (B.rans(9), b"e", B.OK, False)
    assert pick(7, [B.rans(9), B.arith(9)]) == (-1, None, B.UNSUPPORTED, False)
    assert pick(8, [B.rans(0), B.rans(1)]) == (B.rans(1), b"bbb", B.OK, False)


def test_the_small_family_holds_every_outcome():
    assert len(B.small_blocks()) == len(B.SIZES) * len(B.ALPHABETS) and len(B.small_family()) == 1008
    ties, a_wins, r_wins = B.small_census()
    assert ties + a_wins + r_wins == 1008 and min(ties, a_wins, r_wins) >= 20
