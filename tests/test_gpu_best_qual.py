"""Quality blocks: best of several methods across rANS 4x16, arith_dynamic and fqzcomp_qual on the device
(htscodecs_amd/csrc/r4x16_best_qual.hip, include/rans4x16_hip.h part 2n) against the CPU expectation of best_qual_cases.py:
the small family under the three lists with the route's counts, the four fixture slices with the reference's own fqzcomp
streams, single-codec lists against the codecs' own calls, a batch that mixes an empty block, a slice without records, an
undecided block and ordinary ones, the dense arena's rules, a run in chunks, the decode of the mixed arena and the
host-buffer calls.  Everything is exact.  Every device call runs in the confinement layout of test_gpu_confinement.py, as
test_gpu_fqz_best.run does: the inputs a few bytes apart in an arena of their own, the output arena filled with a pattern
and every byte outside the results compared afterwards, the inputs and the records compared afterwards too."""
import numpy as np
import pytest

import best_any_cases as A
import best_qual_cases as Q
import fqz_best_cases as B
import fqz_gpu as G
import fqz_pick_cases as P
import test_best_qual_cpu as CPU
from test_gpu_confinement import pattern

pytestmark = pytest.mark.gpu
SENTINEL = 0x5a5a5a5a
GUARD = 4096
WRITER = (A.rans(1), A.arith(1), Q.fqz(0), Q.fqz(1), Q.fqz(2), Q.fqz(3))
ROUTES = ("best_qual", "fqz_best", "fqz_pick", "best_any")


@pytest.fixture(scope="module")
def dc():
    import htscodecs_amd as H
    return H.DeviceCodec(0)


class _Res:
    pass


def as_i32(a):
    return np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)


def run(dc, blocks, methods, vers=4, capacity=None, sizing=False, max_in=None, max_rec=None, call="qual", records=True):
    """blocks: [(data, lens, flags)].  One packed encode call into a patterned arena of `capacity` bytes (default: ample).
    call: "qual", or a codec's own best-packed call ("rans", "arith", "any" with `methods` as that call takes them, "fqz"
    with strategies).  records False: the four record tensors are None.  Asserts that nothing outside the results was
    written, that the length entries of a block fqzcomp did not win stay untouched, and that the inputs are as they were."""
    import torch as t
    n = len(blocks)
    in_off, rec_off, pos, rpos = [], [], 3, 2
    for i, (data, lens, flags) in enumerate(blocks):
        in_off.append(pos); rec_off.append(rpos)
        pos += len(data) + 1 + i % 7
        rpos += len(lens) + i % 3
    arena_in = np.full(pos + 64, 0xee, dtype=np.uint8)
    a_len = np.full(rpos + 8, SENTINEL, dtype=np.int64)
    a_fl = np.full(rpos + 8, SENTINEL, dtype=np.int64)
    for (data, lens, flags), o, ro in zip(blocks, in_off, rec_off):
        arena_in[o:o + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
        a_len[ro:ro + len(lens)] = lens
        a_fl[ro:ro + len(flags)] = flags
    dev = dc.dev
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(dev)
    i64 = lambda v: up(np.array(v, dtype=np.int64))
    r = _Res()
    r.alloc = sum(2 * len(b[0]) + 14 * len(b[1]) + 256 for b in blocks) + GUARD
    r.cap = 0 if sizing else (r.alloc - GUARD if capacity is None else capacity)
    r.pat = pattern(r.alloc)
    d_in, d_len, d_fl = up(arena_in), up(as_i32(a_len)), up(as_i32(a_fl))
    d_out = None if sizing else up(r.pat.copy())
    d_lo = t.full_like(d_len, SENTINEL)
    d_osz, d_st, d_ch = (t.full((n,), -7, dtype=t.int32, device=dev) for _ in range(3))
    d_off = t.full((n + 1,), -7, dtype=t.int64, device=dev)
    d_ioff, sizes, d_roff = i64(in_off), up(as_i32([len(b[0]) for b in blocks])), i64(rec_off)
    nrec = up(as_i32([len(b[1]) for b in blocks]))
    max_in = max_in if max_in is not None else max([len(b[0]) for b in blocks] + [1])
    max_rec = max_rec if max_rec is not None else max([len(b[1]) for b in blocks] + [1])
    total = sum(len(b[0]) for b in blocks)
    dc.set_option("route_count", 1)
    dc.set_fqz_limits(0, B.max_sym(blocks))                          # the model slots: no wider than the batch needs
    try:
        for w in ROUTES:
            dc.route_read(w)
        if call == "qual":
            recs = (d_len, d_fl, d_roff, nrec) if records else (None, None, None, None)
            dc.compress_best_qual_packed(d_in, d_ioff, sizes, *recs, d_out, d_off, d_osz, d_st, list(methods), max_in, max_rec, vers=vers,
                                         chosen=d_ch, d_len_out=d_lo, total_in_size=total, out_capacity=r.cap)
        elif call == "fqz":
            dc.fqz_compress_best_packed(d_in, d_ioff, sizes, d_len, d_fl, d_roff, nrec, d_out, d_off, d_osz, d_st, list(methods), max_in, max_rec,
                                        vers=vers, chosen=d_ch, d_len_out=d_lo, out_capacity=r.cap)
        else:
            fn = {"any": dc.compress_best_any_packed, "rans": dc.compress_best_packed, "arith": dc.arith_compress_best_packed}[call]
            if sizing and call == "rans":
                d_out = t.zeros(1, dtype=t.uint8, device=dev)
            fn(d_in, d_ioff, sizes, d_out, d_off, d_osz, d_st, list(methods), max_in, chosen=d_ch, total_in_size=total, out_capacity=r.cap)
        t.cuda.synchronize(dev)
        r.routes = {w: dc.route_read(w) for w in ROUTES}
    finally:
        dc.set_option("route_count", 0)
        dc.set_fqz_limits(0, 0)
    r.route = r.routes["best_qual"]
    r.d_out, r.d_off, r.d_osz, r.d_chosen = d_out, d_off, d_osz, d_ch
    r.arena = None if sizing else d_out.cpu().numpy()
    r.off, r.osz, r.st, r.chosen = d_off.tolist(), d_osz.tolist(), d_st.tolist(), d_ch.tolist()
    assert (d_in.cpu().numpy() == arena_in).all(), "the call changed its input"
    assert (d_len.cpu().numpy() == as_i32(a_len)).all() and (d_fl.cpu().numpy() == as_i32(a_fl)).all(), "the call changed the records"
    assert r.off[0] == 0 and all(b >= a for a, b in zip(r.off, r.off[1:])), r.off[:8]
    written = np.zeros(r.alloc, dtype=bool)
    r.outs = []
    for i in range(n):
        assert r.osz[i] >= 0 and (r.osz[i] == 0 or r.st[i] == 0), (i, r.st[i], r.osz[i])
        if r.st[i] == 0 and not sizing:
            assert r.off[i + 1] - r.off[i] == r.osz[i] and r.off[i + 1] <= r.cap, (i, r.off[i], r.off[i + 1], r.osz[i])
            written[r.off[i]:r.off[i + 1]] = True
            r.outs.append(r.arena[r.off[i]:r.off[i + 1]].tobytes())
        else:
            r.outs.append(None)
    if not sizing:
        bad = np.nonzero((r.arena != r.pat) & ~written)[0]
        assert not len(bad), ("bytes written outside the results", bad[:8].tolist(), len(bad))
    lo = d_lo.cpu().numpy().view(np.uint32)
    touched = np.zeros(len(lo), dtype=bool)
    r.lens_out = []
    fqz_won = lambda i: r.chosen[i] >= 0 and (call == "fqz" or r.chosen[i] & Q.CODEC_MASK == Q.CODEC_FQZ) and call in ("qual", "fqz")
    for i, (b, ro) in enumerate(zip(blocks, rec_off)):
        nr = len(b[1])
        if fqz_won(i):
            touched[ro:ro + nr] = True
            r.lens_out.append(lo[ro:ro + nr].tolist())
        else:
            r.lens_out.append(None)
    assert (lo[~touched] == SENTINEL).all(), "length entries of a block fqzcomp did not win were written"
    return r


def check(r, want, what):
    """Everything the call reports against the expectation [(chosen, stream or None, status, tie, lengths or None)]: the
    offsets are the scan of the winners' sizes, whatever the capacity refuses"""
    need = [0] + np.cumsum([len(w[1]) if w[1] is not None else 0 for w in want]).tolist()
    assert r.off == need, (what, r.off[:8], need[:8])
    for i, (m, s, status, _, lens) in enumerate(want):
        tag = (what, i, r.st[i], r.osz[i], r.chosen[i], m, status, s and len(s))
        assert r.chosen[i] == m, tag
        if s is None:
            assert r.st[i] == status and r.osz[i] == 0 and r.outs[i] is None, tag
        elif need[i + 1] > r.cap:
            assert r.st[i] == Q.CAPACITY and r.osz[i] == 0, tag
        else:
            assert r.st[i] == 0 and r.osz[i] == len(s) and r.outs[i] == s, tag
        assert r.lens_out[i] == lens, (tag, "lengths")


def census(want, chunks=1):
    out = dict.fromkeys(Q.KINDS, 0)
    out["chunks"] = chunks
    for m, s, status, tie, _ in want:
        out["blocks"] += 1
        out["undecided" if status == Q.UNDECIDED else Q.who_of(m)] += 1
        out["tie"] += tie
    return out


# ---- the small family ---------------------------------------------------------------------------------------------------
_family = {}


def family(dc, which):
    """(expectation, result) of the small family under LISTS[which], run once"""
    if which not in _family:
        blocks = list(Q.small_blocks())
        want = [Q.expect(b, Q.LISTS[which]) for b in blocks]
        _family[which] = (want, run(dc, blocks, Q.LISTS[which]))
    return _family[which]


@pytest.mark.parametrize("which", range(3))
def test_the_small_family_in_one_batch(dc, which):
    want, r = family(dc, which)
    check(r, want, Q.LISTS[which])
    assert r.route == census(want), (r.route, census(want))
    # the per-codec routes count their own candidates as before
    nf = sum(1 for m in Q.LISTS[which] if m & Q.CODEC_MASK == Q.CODEC_FQZ)
    assert r.routes["fqz_best"]["candidates"] == nf * len(want) and r.routes["fqz_best"]["blocks"] == r.route["fqz"]
    assert r.routes["fqz_pick"]["blocks"] == nf * len(want) and r.routes["best_any"] == dict.fromkeys(r.routes["best_any"], 0)


def test_the_routes_counts_over_the_family_are_the_census(dc):
    tot = dict.fromkeys(Q.KINDS, 0)
    for which in range(3):
        for k, v in family(dc, which)[1].route.items():
            tot[k] += v
    rans, arith, fqz, fqz_ties, ra_ties = Q.small_census()
    assert tot["tie"] == fqz_ties + ra_ties and tot["rans"] + tot["arith"] + tot["fqz"] == 3 * len(Q.small_blocks())
    assert tot["rans"] >= rans and tot["arith"] >= arith and tot["fqz"] >= fqz and tot["failed"] == tot["undecided"] == 0 and tot["chunks"] == 3


def test_the_tie_rule_is_seen_from_both_sides(dc):
    (w0, r0), (w1, r1) = family(dc, 0), family(dc, 1)
    ties = 0
    for i in range(len(w0)):
        if w0[i][3]:
            ties += 1
            assert r0.chosen[i] != r1.chosen[i] and r0.osz[i] == r1.osz[i], (i, r0.chosen[i], r1.chosen[i])
        else:
            assert r0.chosen[i] == r1.chosen[i] and r0.outs[i] == r1.outs[i], i
    assert ties >= 10


# ---- the reference's streams ----------------------------------------------------------------------------------------------
def fixtures():
    return [B.fixture_slice(name) for name in B.SLICES]


def fixture_want(methods=WRITER):
    want = []
    for name in B.SLICES:
        strat, size = B.WINNERS[name]
        block = B.fixture_slice(name)
        want.append(Q.expect(block, methods, fqz_result=(0, B.fixture_stream(name, strat), strat, list(block[1]))))
    return want


def test_the_four_fixture_slices_under_the_writers_list(dc):
    want = fixture_want()
    assert [Q.who_of(w[0]) for w in want] == ["fqz", "fqz", "fqz", "arith"]
    r = run(dc, fixtures(), WRITER)
    check(r, want, "fixtures")
    for i, name in enumerate(B.SLICES[:3]):                          # where fqzcomp wins: the committed reference stream
        assert r.outs[i] == B.fixture_stream(name, B.WINNERS[name][0]) and r.osz[i] == B.WINNERS[name][1]
    assert r.route == dict(blocks=4, chunks=1, rans=0, arith=1, fqz=3, tie=0, failed=0, undecided=0)
    assert r.routes["fqz_best"]["blocks"] == 3 and r.routes["fqz_best"]["candidates"] == 16


# ---- single-codec lists ---------------------------------------------------------------------------------------------------
def some_blocks():
    return list(Q.small_blocks())[::3] + fixtures()[3:]


@pytest.mark.parametrize("codec,words", [("rans", (0, 1, 65)), ("arith", (0, 1, 65)), ("fqz", (0, 1, 2, 3)), ("fqz", (3, 0))])
def test_a_list_of_one_codec_gives_what_that_codecs_call_gives(dc, codec, words):
    blocks = some_blocks()
    tag = {"rans": 0, "arith": Q.CODEC_ARITH, "fqz": Q.CODEC_FQZ}[codec]
    own = run(dc, blocks, words, call=codec)
    r = run(dc, blocks, [tag | w for w in words])
    assert r.off == own.off and r.osz == own.osz and r.st == own.st and r.lens_out == own.lens_out
    if codec == "fqz":
        assert r.chosen == [c if c < 0 else tag | words[c] for c in own.chosen]
    else:
        assert r.chosen == [c if c < 0 else tag | c for c in own.chosen]
    assert np.array_equal(r.arena, own.arena)
    assert r.route[codec] == sum(s == 0 for s in own.st) and r.route["tie"] == 0
    if codec == "fqz":
        assert r.routes["fqz_best"] == own.routes["fqz_best"] and r.routes["fqz_pick"] == own.routes["fqz_pick"]


def test_a_list_without_fqzcomp_and_without_records_is_part_2ms_call(dc):
    blocks = some_blocks()
    methods = [A.rans(1), A.arith(1), A.arith(65), A.rans(65)]
    own = run(dc, blocks, methods, call="any")
    r = run(dc, blocks, methods, records=False)
    assert r.off == own.off and r.osz == own.osz and r.st == own.st and r.chosen == own.chosen and np.array_equal(r.arena, own.arena)
    assert {k: r.route[k] for k in ("rans", "arith", "tie", "failed", "chunks")} == own.routes["best_any"]
    check(r, [Q.expect(b, methods) for b in blocks], "no fqzcomp")


# ---- failures, and what stays of the block ----------------------------------------------------------------------------------
MIXED = (A.rans(0), A.arith(0), Q.fqz(2), Q.fqz(3))


def mixed():
    """ordinary slices, an empty block, a slice of ten bytes without a record - its record sum is wrong and no fix-up can
    mend it -, one whose sum is short (the fix-ups mend it), and one with READ2 records"""
    some = list(Q.small_blocks())
    d, l, f = some[39]
    r2 = (d, l, tuple(x | (128 if k % 2 else 0) for k, x in enumerate(f)))
    return [some[27], (b"", (), ()), some[33], (bytes([7, 9] * 5), (), ()), (bytes([3, 4, 4, 5] * 5), (8, 8), (0, 16)), r2, some[36], some[12]]


def test_a_batch_of_an_empty_block_a_slice_without_records_an_undecided_block_and_ordinary_ones(dc):
    blocks = mixed()
    methods = list(MIXED)
    plain = [Q.expect(b, methods) for b in blocks]
    assert Q.fqz_sub(blocks[3], [2, 3])[0] == Q.SIZE and Q.who_of(plain[3][0]) in ("rans", "arith")       # fqzcomp out, the others stand
    assert [Q.who_of(w[0]) for w in plain].count("fqz") >= 3 and Q.who_of(plain[5][0]) == "fqz" and plain[4][2] == 0
    r = run(dc, blocks, methods)
    check(r, plain, "decided")
    assert r.route == census(plain)
    # guard_bits: strategies 2 and 3 compare something only where there is a READ2 record - that block alone is undecided
    dc.set_fqz_pick(0, 64)
    try:
        r = run(dc, blocks, methods)
    finally:
        dc.set_fqz_pick(0, 0)
    want = list(plain)
    want[5] = (-1, None, Q.UNDECIDED, False, None)
    check(r, want, "undecided")
    assert r.st[5] == Q.UNDECIDED and r.osz[5] == 0 and r.chosen[5] == -1 and r.off[6] == r.off[5]
    assert r.route == census(want) and r.route["undecided"] == 1 and r.routes["fqz_best"]["undecided"] == 1
    # the records' own refusal first in the list: with fqzcomp alone the block has that status
    r = run(dc, blocks[3:4], [Q.fqz(0), Q.fqz(3)])
    assert r.st == [Q.SIZE] and r.chosen == [-1] and r.osz == [0] and r.route["failed"] == 1


def test_blocks_above_the_maxima_lose_the_codec_that_has_the_limit(dc):
    blocks = [(bytes(100), (50, 50), (0, 0)), (bytes(range(30)) * 2, (10,) * 6, (0,) * 6), (bytes(101), (101,), (0,))]
    methods = list(Q.TRIPLE)
    want = [Q.expect(b, methods) for b in blocks]
    r = run(dc, blocks, methods, max_rec=2)                          # max_records is fqzcomp's alone
    want[1] = Q.expect(blocks[1], methods, fqz_result=(Q.UNSUPPORTED, None, -1, None))
    check(r, want, "max_records")
    r = run(dc, blocks, methods, max_in=100)                         # max_in_size is every codec's
    want = [Q.expect(b, methods) for b in blocks[:2]] + [(-1, None, Q.UNSUPPORTED, False, None)]
    check(r, want, "max_in_size")
    assert r.route["failed"] == 1


# ---- the dense arena's rules -----------------------------------------------------------------------------------------------
def test_an_arena_one_byte_short_a_cut_in_the_middle_and_the_sizing_pass(dc):
    want, whole = family(dc, 0)
    blocks = list(Q.small_blocks())
    total = whole.off[-1]
    assert total == sum(len(w[1]) for w in want)
    last_f = max(i for i, w in enumerate(want) if Q.who_of(w[0]) == "fqz")
    last_a = max(i for i, w in enumerate(want) if Q.who_of(w[0]) == "arith")
    for cap in (total - 1, whole.off[last_f + 1] - 1, whole.off[last_a + 1] - 1):
        r = run(dc, blocks, Q.LISTS[0], capacity=cap)
        check(r, want, ("capacity", cap))
        fits = [whole.off[i + 1] <= cap or whole.osz[i] == 0 for i in range(len(blocks))]
        assert [s == 0 for s in r.st] == fits and not all(fits)
    s = run(dc, blocks, Q.LISTS[0], sizing=True)
    assert s.off == whole.off and s.chosen == whole.chosen and not any(s.osz)
    assert all(st == (Q.CAPACITY if len(w[1]) else 0) for st, w in zip(s.st, want))


# ---- chunks -----------------------------------------------------------------------------------------------------------------
def test_twelve_blocks_in_at_least_three_chunks(dc):
    blocks = list(Q.small_blocks())[18:27] + list(Q.small_blocks())[36:39]
    assert len(blocks) == 12
    methods = list(Q.EIGHT)
    want = [Q.expect(b, methods) for b in blocks]
    whole = run(dc, blocks, methods)
    check(whole, want, "whole")
    assert whole.route["chunks"] == 1
    keep = dc.get_option("max_workspace_mb")
    n, max_in, max_rec, total = 12, max(len(b[0]) for b in blocks), max(len(b[1]) for b in blocks), sum(len(b[0]) for b in blocks)
    try:
        dc.set_fqz_limits(0, B.max_sym(blocks))
        assert dc.best_qual_chunk_blocks(n, methods, max_in, max_rec, total) == n
        last = n
        for mb in (1024, 512, 256, 128, 64, 32, 16, 8, 4, 2, 1):
            dc.set_option("max_workspace_mb", mb)
            per = dc.best_qual_chunk_blocks(n, methods, max_in, max_rec, total)
            assert 1 <= per <= last                                  # the plan does not grow when the ceiling shrinks
            last = per
            if per <= 4:
                break
        assert 1 <= per <= 4, per
        dc.set_fqz_limits(0, 0)
        r = run(dc, blocks, methods)
    finally:
        dc.set_option("max_workspace_mb", keep)
        dc.set_fqz_limits(0, 0)
    chunks = -(-n // per)
    assert chunks >= 3 and r.route["chunks"] == chunks, (per, chunks, r.route)
    check(r, want, "chunks")
    assert np.array_equal(r.arena, whole.arena) and r.off == whole.off and r.chosen == whole.chosen and r.lens_out == whole.lens_out
    assert {k: v for k, v in r.route.items() if k != "chunks"} == {k: v for k, v in whole.route.items() if k != "chunks"}


def test_the_planner_answers_a_bad_list_and_an_empty_batch(dc):
    assert dc.best_qual_chunk_blocks(0, list(Q.TRIPLE), 4096, 10) == 0
    for methods, words in (([0, (2 << 24) | 1], "unknown codec tag"), ([Q.fqz(0)] * 17, "more than 16"), ([Q.fqz(1 << 16)], "above 16 bits")):
        with pytest.raises(RuntimeError, match=words):
            dc.best_qual_chunk_blocks(4, methods, 4096, 10)


@pytest.mark.parametrize("name", ["the rANS 4x8 tag's place", "the tag behind fqzcomp's", "seventeen strategies", "k = 33", "a negative strategy"])
def test_a_bad_method_list_is_refused_before_anything_is_enqueued(dc, name):
    import torch
    lists = {"the rANS 4x8 tag's place": [0, (2 << 24) | 1], "the tag behind fqzcomp's": [Q.fqz(0), (4 << 24) | 1],
             "seventeen strategies": [1] * 3 + [Q.fqz(j & 3) for j in range(17)] + [1] * 12, "k = 33": [0] * 33, "a negative strategy": [Q.fqz(0), -2]}
    d_off = torch.full((1,), -7, dtype=torch.int64, device=dc.dev)
    empty = torch.zeros(0, dtype=torch.int32, device=dc.dev)
    d_in = torch.zeros(8, dtype=torch.uint8, device=dc.dev)
    args = lambda: (d_in, torch.zeros(0, dtype=torch.int64, device=dc.dev), empty, None, None, None, None, d_in, d_off, empty, empty)
    dc.compress_best_qual_packed(*args(), list(Q.TRIPLE), 0, 0)
    torch.cuda.synchronize()
    assert d_off.item() == 0                                         # an empty batch under an acceptable list is taken
    d_off.fill_(-7)
    held = dc.L.rans4x16_hip_workspace_bytes(dc.ctx.h)
    with pytest.raises(RuntimeError, match=CPU.REFUSED[name]):
        dc.compress_best_qual_packed(*args(), lists[name], 0, 0)
    torch.cuda.synchronize()
    assert d_off.item() == -7 and dc.L.rans4x16_hip_workspace_bytes(dc.ctx.h) == held


# ---- decode -------------------------------------------------------------------------------------------------------------------
def decode(dc, d_in, in_off, in_size, method, sizes, len_caps, max_out=None, capacity=None, max_sym=255):
    """uncompress_qual_packed into a patterned arena, the lengths into a patterned array with a slot per block"""
    import torch as t
    dev, n = dc.dev, in_size.numel()
    r = _Res()
    r.alloc = sum(sizes) + GUARD
    r.pat = pattern(r.alloc)
    d_out = t.from_numpy(r.pat.copy()).to(dev)
    off = t.full((n + 1,), -7, dtype=t.int64, device=dev)
    osz, st, nrec = (t.full((n,), -3, dtype=t.int32, device=dev) for _ in range(3))
    len_off, at = [], 5
    for i, c in enumerate(len_caps):
        len_off.append(at)
        at += c + 1 + i % 3
    len_fill = (G.LEN_FILL + np.arange(at + 8)).astype(np.int32)
    d_len = t.from_numpy(len_fill.copy()).to(dev)
    dc.set_fqz_limits(0, max_sym)
    try:
        dc.uncompress_qual_packed(d_in, in_off, in_size, method, d_out, off, osz, st, int(in_size.max().item()) if n else 0,
                                  max(sizes) if max_out is None else max_out, out_capacity=r.alloc - GUARD if capacity is None else capacity,
                                  d_len=d_len, len_off=t.tensor(len_off, dtype=t.int64, device=dev),
                                  len_cap=t.tensor(len_caps, dtype=t.int32, device=dev), nrec=nrec)
        t.cuda.synchronize()
    finally:
        dc.set_fqz_limits(0, 0)
    r.arena, r.off, r.osz, r.st, r.nrec = d_out.cpu().numpy(), off.tolist(), osz.tolist(), st.tolist(), nrec.tolist()
    got, meth = d_len.cpu().numpy(), method.tolist()
    mask = np.zeros(len(got), dtype=bool)
    r.lens = []
    for i, (o, c) in enumerate(zip(len_off, len_caps)):
        k = min(r.nrec[i], c) if r.st[i] == 0 else 0
        mask[o:o + k] = True
        r.lens.append(got[o:o + k].tolist())
        if r.st[i] != 0 and meth[i] >= 0 and meth[i] & Q.CODEC_MASK == Q.CODEC_FQZ:
            mask[o:o + c] = True                                     # a refused fqzcomp stream's slot may hold anything
    bad = np.nonzero((got != len_fill) & ~mask)[0]
    assert not len(bad), ("lengths written outside their slots", bad[:8].tolist())
    return r


def check_decoded(r, blocks, status, what):
    """status[i]: what block i must report; 0: its bytes.  The offsets are the scan of the sizes that were claimed."""
    mask = np.zeros(r.alloc, dtype=bool)
    for i, b in enumerate(blocks):
        tag = (what, i, r.st[i], r.osz[i], status[i])
        assert r.st[i] == status[i], tag
        if status[i] == 0:
            assert r.osz[i] == len(b) == r.off[i + 1] - r.off[i] and r.arena[r.off[i]:r.off[i + 1]].tobytes() == b, tag
            mask[r.off[i]:r.off[i + 1]] = True
        else:
            assert r.osz[i] == 0 and r.nrec[i] == 0, tag
    assert np.array_equal(r.arena[~mask], r.pat[~mask]), (what, "a byte outside the blocks' ranges changed")


def test_the_mixed_arena_goes_straight_into_the_decoder(dc):
    import torch as t
    want, enc = family(dc, 2)
    blocks = list(Q.small_blocks())
    datas = [bytes(b[0]) for b in blocks]
    sizes = [len(d) for d in datas]
    assert {Q.who_of(w[0]) for w in want} == {"rans", "arith", "fqz"}
    nrecs = [len(b[1]) for b in blocks]
    sym = B.max_sym(blocks)
    r = decode(dc, enc.d_out, enc.d_off, enc.d_osz, enc.d_chosen, sizes, nrecs, max_sym=sym)
    assert r.off == [0] + np.cumsum(sizes).tolist()
    check_decoded(r, datas, [0] * len(blocks), "round trip")
    for i, (w, b) in enumerate(zip(want, blocks)):
        if Q.who_of(w[0]) == "fqz":
            k = P.reached(w[4], len(b[0]))
            assert r.nrec[i] == k and r.lens[i] == w[4][:k], i
        else:
            assert r.nrec[i] == 0 and r.lens[i] == [], i
    # a claim above max_out_size refuses that block alone, whichever codec it is
    limit = 40
    over = [n > limit for n in sizes]
    assert len({Q.who_of(w[0]) for w, o in zip(want, over) if o}) == 3 and over.count(False) >= 20
    r = decode(dc, enc.d_out, enc.d_off, enc.d_osz, enc.d_chosen, sizes, nrecs, max_out=limit, max_sym=sym)
    check_decoded(r, datas, [Q.UNSUPPORTED if o else 0 for o in over], "max_out_size")
    # a capacity that cuts the output: the blocks behind the cut are CAPACITY, the offsets stand
    cap = sum(sizes[:50]) + 1
    r = decode(dc, enc.d_out, enc.d_off, enc.d_osz, enc.d_chosen, sizes, nrecs, capacity=cap, max_sym=sym)
    assert r.off == [0] + np.cumsum(sizes).tolist()
    check_decoded(r, datas, [0 if sum(sizes[:i + 1]) <= cap else Q.CAPACITY for i in range(len(blocks))], "capacity")
    # a block that was never written, and a tag that is no candidate's
    method = enc.d_chosen.clone()
    method[3], method[4], method[5] = -1, (2 << 24) | 1, 4 << 24
    r = decode(dc, enc.d_out, enc.d_off, enc.d_osz, method, sizes, nrecs, max_sym=sym)
    check_decoded(r, datas, [Q.EMPTY if i == 3 else Q.UNSUPPORTED if i in (4, 5) else 0 for i in range(len(blocks))], "no stream, no codec")
    assert all(r.off[i + 1] == r.off[i] for i in (3, 4, 5))


def test_a_stream_under_the_wrong_tag_gets_that_decoders_own_status(dc):
    import torch as t
    want, enc = family(dc, 2)
    blocks = list(Q.small_blocks())
    pick = {}
    for i, w in enumerate(want):
        if len(blocks[i][0]) >= 200 or Q.who_of(w[0]) == "rans":
            pick.setdefault(Q.who_of(w[0]), i)
    f, a, rr = pick["fqz"], pick["arith"], pick["rans"]
    streams = [want[f][1], want[a][1], want[rr][1], want[a][1], want[f][1]]
    raw, offs = bytearray(b"\xee" * 7), []
    for s in streams:
        offs.append(len(raw))
        raw += s + b"\xee" * 7
    d_in = t.from_numpy(np.frombuffer(bytes(raw) + b"\0" * 64, dtype=np.uint8).copy()).to(dc.dev)
    in_off = t.tensor(offs, dtype=t.int64, device=dc.dev)
    in_size = t.tensor([len(s) for s in streams], dtype=t.int32, device=dc.dev)
    wrong = [A.arith(1), Q.fqz(0), Q.fqz(0), A.rans(1), A.rans(1)]
    method = t.tensor(wrong, dtype=t.int32, device=dc.dev)
    sizes = [4096] * len(streams)
    r = decode(dc, d_in, in_off, in_size, method, sizes, [64] * len(streams))           # (decode: nothing outside the slots)
    assert r.st[1] != 0 and r.st[2] != 0 and r.osz[1] == r.osz[2] == 0, r.st             # no fqzcomp header: never the version byte
    # the decoders' own words for the same streams: part 2m's call for rANS and arith, the fqzcomp decoder's for the rest
    off = t.full((len(streams) + 1,), -7, dtype=t.int64, device=dc.dev)
    osz, st = (t.full((len(streams),), -3, dtype=t.int32, device=dc.dev) for _ in range(2))
    d_out = t.zeros(sum(sizes), dtype=t.uint8, device=dc.dev)
    only = t.tensor([m if m & Q.CODEC_MASK != Q.CODEC_FQZ else -1 for m in wrong], dtype=t.int32, device=dc.dev)
    dc.uncompress_any_packed(d_in, in_off, in_size, only, d_out, off, osz, st, max(len(s) for s in streams), 4096)
    t.cuda.synchronize()
    own, own_size = st.tolist(), osz.tolist()
    assert [r.osz[i] for i in (0, 3, 4)] == [own_size[i] for i in (0, 3, 4)]
    for i in (1, 2):
        claim = streams[i][0] if streams[i][0] < 128 else None
        assert claim is not None and claim <= 4096
        own[i] = G.run_dev(dc, [streams[i]], [claim])[1][0]
    assert r.st == own, (r.st, own)


# ---- host buffers -----------------------------------------------------------------------------------------------------------------
def test_the_host_batches(dc):
    import htscodecs_amd as H
    blocks = list(Q.small_blocks())
    methods = list(Q.EIGHT)
    want = [Q.expect(b, methods) for b in blocks]
    datas, lens, flags = [b[0] for b in blocks], [list(b[1]) for b in blocks], [list(b[2]) for b in blocks]
    outs, chosen, status, lens2, flags2 = H.compress_best_qual_batch(datas, lens, flags, methods, ctx=dc.ctx)   # out[i] == NULL: the library allocates
    assert status == [0] * len(blocks) and chosen == [w[0] for w in want] and outs == [w[1] for w in want]
    for i, w in enumerate(want):
        assert lens2[i] == (w[4] if Q.who_of(w[0]) == "fqz" else lens[i]) and flags2[i] == [f & 0xffff for f in flags[i]], i
    caps = [len(w[1]) + (i % 3) for i, w in enumerate(want)]
    short = [i for i, w in enumerate(want) if Q.who_of(w[0]) == "fqz"][0]
    caps[short] = len(want[short][1]) - 1
    outs2, chosen2, status2, _, _ = H.compress_best_qual_batch(datas, lens, flags, methods, caps=caps, ctx=dc.ctx)
    assert status2 == [Q.CAPACITY if i == short else 0 for i in range(len(blocks))] and chosen2 == chosen
    assert outs2 == [None if i == short else w[1] for i, w in enumerate(want)]
    # the way back, with the record lengths of the blocks fqzcomp won
    back, st, blens, nrec = H.uncompress_qual_batch(outs, chosen, [len(d) for d in datas], nlengths=[len(l) for l in lens], ctx=dc.ctx)
    assert st == [0] * len(blocks) and back == [bytes(d) for d in datas]
    for i, (w, b) in enumerate(zip(want, blocks)):
        k = P.reached(w[4], len(b[0])) if Q.who_of(w[0]) == "fqz" else 0
        assert nrec[i] == k and blens[i] == (w[4][:k] if k else []), i
    caps = [len(d) for d in datas]
    caps[short] -= 1
    caps[0] -= 1
    back, st, _, _ = H.uncompress_qual_batch(outs, chosen, caps, ctx=dc.ctx)
    assert st == [Q.CAPACITY if i in (0, short) else 0 for i in range(len(blocks))], st
    back, st, _, nrec = H.uncompress_qual_batch([b""] + outs[:3], [-1] + chosen[:3], [8] + [len(d) for d in datas[:3]], ctx=dc.ctx)
    assert st == [Q.EMPTY, 0, 0, 0] and back[1:] == [bytes(d) for d in datas[:3]]
    # a list without an fqzcomp method, and no records: part 2m's batch
    eight, pair = datas[20:28], [A.rans(1), A.arith(1), A.arith(65), A.rans(65)]
    own = H.compress_best_any_batch(eight, pair, ctx=dc.ctx)
    got = H.compress_best_qual_batch(eight, [[]] * 8, [[]] * 8, pair, ctx=dc.ctx)
    assert own[2] == [0] * 8 and got[:3] == own and got[3:] == ([[]] * 8, [[]] * 8)


def test_the_host_batch_picks_an_undecided_block_on_the_host(dc):
    import htscodecs_amd as H
    blocks = mixed()
    methods = list(MIXED)
    want = [Q.expect(b, methods) for b in blocks]
    datas, lens, flags = [b[0] for b in blocks], [list(b[1]) for b in blocks], [list(b[2]) for b in blocks]
    for guard, host in ((0, 0), (64, 1)):
        dc.set_fqz_pick(0, guard)
        dc.set_option("route_count", 1)
        try:
            dc.route_read("fqz_pick"); dc.route_read("best_qual")
            outs, chosen, status, lens2, flags2 = H.compress_best_qual_batch(datas, lens, flags, methods, ctx=dc.ctx)
            pick, route = dc.route_read("fqz_pick"), dc.route_read("best_qual")
        finally:
            dc.set_option("route_count", 0)
            dc.set_fqz_pick(0, 0)
        assert status == [w[2] for w in want] and chosen == [w[0] for w in want] and outs == [w[1] for w in want], (guard, status, chosen)
        assert pick["host"] == host and route["undecided"] == host and route["blocks"] == len(blocks)
        for i, w in enumerate(want):
            assert lens2[i] == (w[4] if Q.who_of(w[0]) == "fqz" else lens[i]), (guard, i)
    assert Q.who_of(want[5][0]) == "fqz"                             # the block the host decided: fqzcomp's, with its lengths
