"""Best of several strategies for fqzcomp_qual encoding on the device (htscodecs_amd/csrc/r4x16_fqz_best.hip,
include/rans4x16_hip.h part 2l).

The expected streams are the reference's own where it made them: the 16 streams of tests/golden/fqzcomp, whose smallest
per slice are q4.0, q40+dir.1, q8.0 and qvar.3 (test_fqz_best_cpu.py), and the `_s0` / `_s1` pairs of
tests/golden/fqzcomp/pick.bin that share one slice.  Everywhere else the answer is the smallest of the existing one-call's
results (fqz_compress_pick, which test_gpu_fqz_pick.py holds to the reference), the first on a tie.  Everything is exact.
Every device call runs in the confinement layout of test_gpu_confinement.py: the slots a few bytes apart in an arena filled
with a pattern, every byte outside the results compared afterwards, the inputs and the records compared afterwards too."""
import itertools

import numpy as np
import pytest

import fqz_best_cases as B
import fqz_enc_model as E
import fqz_gpu as G
import fqz_model as M
import fqz_pick_cases as P
from test_gpu_confinement import Layout, pattern
from test_gpu_fqz_pick import run as pick_run

pytestmark = pytest.mark.gpu
SENTINEL = 0x5a5a5a5a
BEST_KINDS = ("blocks", "candidates", "counted", "undecided", "refused")


@pytest.fixture(scope="module")
def dc():
    import htscodecs_amd as H
    return H.DeviceCodec(0)


def ample(blocks):
    from htscodecs_amd import codec
    return [E.cap(len(d), len(l), codec.fqz_pick_cap()) for d, l, f in blocks]


def run(dc, blocks, strats, vers=4, packed=False, caps=None, capacity=None, max_in=None, max_rec=None):
    """blocks: [(data, lens, flags)].  One call of fqz_compress_best (or _best_packed, into an arena of `capacity` bytes).
    -> (bytes or None, sizes, statuses, chosen, lengths out or None, {route name: counts}).  Asserts that nothing outside
    the results was written, that a block without a result left no length behind, and that the inputs are as they were."""
    import torch as t
    n = len(blocks)
    caps = ample(blocks) if caps is None else caps
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
    as_i32 = lambda a: np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)
    dev = dc.dev
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(dev)
    i64 = lambda v: up(np.array(v, dtype=np.int64))
    if packed:
        capacity = sum(caps) if capacity is None else capacity
        fill = pattern(capacity + 4096)
    else:
        lay = Layout(caps, what=[len(b[0]) for b in blocks])
        fill = lay.pattern
    d_in, d_out, d_len, d_fl = up(arena_in), up(fill.copy()), up(as_i32(a_len)), up(as_i32(a_fl))
    d_lo = t.full_like(d_len, SENTINEL)
    d_osz, d_st, d_ch = (t.full((n,), -7, dtype=t.int32, device=dev) for _ in range(3))
    d_off = t.full((n + 1,), -7, dtype=t.int64, device=dev)
    sizes = up(as_i32([len(b[0]) for b in blocks]))
    nrec = up(as_i32([len(b[1]) for b in blocks]))
    max_in = max_in if max_in is not None else max([len(b[0]) for b in blocks] + [1])
    max_rec = max_rec if max_rec is not None else max([len(b[1]) for b in blocks] + [1])
    names = ("fqz_best", "fqz_pick", "fqz_enc", "launch")
    dc.set_option("route_count", 1)
    dc.set_fqz_limits(0, B.max_sym(blocks))                          # the model slots: no wider than the batch needs
    try:
        for w in names:
            dc.route_read(w)
        if packed:
            dc.fqz_compress_best_packed(d_in, i64(in_off), sizes, d_len, d_fl, i64(rec_off), nrec, d_out, d_off, d_osz, d_st, strats,
                                        max_in, max_rec, vers=vers, chosen=d_ch, d_len_out=d_lo, out_capacity=capacity)
        else:
            dc.fqz_compress_best(d_in, i64(in_off), sizes, d_len, d_fl, i64(rec_off), nrec, d_out, up(lay.offs.copy()), up(as_i32(caps)),
                                 d_osz, d_st, strats, max_in, max_rec, vers=vers, chosen=d_ch, d_len_out=d_lo)
        t.cuda.synchronize(dev)
        route = {w: dc.route_read(w) for w in names}
    finally:
        dc.set_option("route_count", 0)
        dc.set_fqz_limits(0, 0)
    assert route["launch"]["side_by_side"] == 0 and route["launch"]["in_order"] >= 1
    arena = d_out.cpu().numpy()
    st, osz, chosen = d_st.tolist(), d_osz.tolist(), d_ch.tolist()
    assert (d_in.cpu().numpy() == arena_in).all(), "the call changed its input"
    assert (d_len.cpu().numpy() == as_i32(a_len)).all() and (d_fl.cpu().numpy() == as_i32(a_fl)).all(), "the call changed the records"
    for i in range(n):
        assert osz[i] >= 0 and (osz[i] == 0 or st[i] == 0), (i, st[i], osz[i])
        assert -1 <= chosen[i] < len(strats) and (chosen[i] >= 0 if st[i] == 0 else st[i] == M.E_CAPACITY or chosen[i] == -1), (i, st[i], chosen[i])
    written = np.zeros(len(arena), dtype=bool)
    if packed:
        off = d_off.tolist()
        assert off[0] == 0 and all(b >= a for a, b in zip(off, off[1:])), off
        for i in range(n):
            if st[i] == 0:
                assert off[i + 1] - off[i] == osz[i] and off[i + 1] <= capacity, (i, off[i], off[i + 1], osz[i])
                written[off[i]:off[i + 1]] = True
        outs = [arena[off[i]:off[i] + osz[i]].tobytes() if st[i] == 0 else None for i in range(n)]
        assert not written[min(off[n], len(arena)):].any()
    else:
        for i in range(n):
            if st[i] == 0:
                assert osz[i] <= caps[i], (i, osz[i], caps[i])
                written[int(lay.offs[i]):int(lay.offs[i]) + osz[i]] = True
        outs = [x if s == 0 else None for x, s in zip(lay.take(arena, osz), st)]
    bad = np.nonzero((arena != fill) & ~written)[0]                  # outside every result: other slots, refused slots, the gaps
    assert not len(bad), ("bytes written outside the results", bad[:8].tolist(), len(bad))
    lo = d_lo.cpu().numpy().view(np.uint32)
    touched = np.zeros(len(lo), dtype=bool)
    lens_out = []
    for i, (b, ro) in enumerate(zip(blocks, rec_off)):
        nr = len(b[1])
        if chosen[i] >= 0:
            touched[ro:ro + nr] = True
            lens_out.append(lo[ro:ro + nr].tolist())
        else:
            lens_out.append(None)
    assert (lo[~touched] == SENTINEL).all(), "length entries of another block, or of one without a winner, were written"
    return outs, osz, st, chosen, lens_out, route


# ---- the existing one-call, computed once per (version, strategy, slice) --------------------------------------------
_one = {}


def one_calls(dc, blocks, strats, vers=4):
    """[[(status, bytes or None) of fqz_compress_pick under strats[j]] per block], every missing answer from one batch"""
    key = lambda b, s: (vers, min(s, 4), bytes(b[0]), tuple(b[1]), tuple(b[2]))
    todo = {}
    for b in blocks:
        for s in set(strats):
            if key(b, s) not in _one:
                todo[key(b, s)] = (s, b[0], b[1], b[2])
    if todo:
        keys = list(todo)
        outs, osz, st, _, _, _ = pick_run(dc, [todo[k] for k in keys], vers=vers, compress=True)
        for k, o, s in zip(keys, outs, st):
            _one[k] = (s, o)
    return [[_one[key(b, s)] for s in strats] for b in blocks]


def check_against_one_calls(dc, blocks, strats, vers=4, **kw):
    outs, osz, st, chosen, lens_out, route = run(dc, blocks, strats, vers=vers, **kw)
    for i, cands in enumerate(one_calls(dc, blocks, strats, vers)):
        wst, wout, wj = B.expect(cands)
        assert (st[i], chosen[i]) == (wst, wj), (i, strats, st[i], chosen[i], wst, wj, [(s, o and len(o)) for s, o in cands])
        assert outs[i] == wout, (i, strats, "differs from the one-call's stream")
        if wj >= 0:
            assert lens_out[i] == P.host_pick(vers, strats[wj], *blocks[i])[2], (i, "lengths")
    return outs, st, chosen, route


def fixtures():
    """the four slices in the order of the issue's table: q4, q40+dir, q8, qvar"""
    return [B.fixture_slice(name) for name in B.SLICES]


def winners():
    return [B.fixture_stream(name, s) for name, (s, size) in B.WINNERS.items()]


# ---- 1, 2: the reference's streams --------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", (False, True))
def test_the_four_slices_in_one_batch_give_the_references_smallest_streams(dc, packed):
    outs, osz, st, chosen, lens_out, route = run(dc, fixtures(), [0, 1, 2, 3], packed=packed)
    assert st == [0] * 4 and chosen == [0, 1, 0, 3]
    assert outs == winners() and osz == [9307, 43803, 30012, 32073]
    assert lens_out == [b[1] for b in fixtures()]
    r = route["fqz_best"]
    assert r == dict(blocks=4, candidates=16, counted=4, undecided=0, refused=0), r
    assert route["fqz_pick"]["blocks"] == 16 and route["fqz_enc"]["streams"] == 16


@pytest.mark.parametrize("k", range(4))
def test_each_slice_alone(dc, k):
    for packed in (False, True):
        outs, osz, st, chosen, _, _ = run(dc, fixtures()[k:k + 1], [0, 1, 2, 3], packed=packed)
        assert st == [0] and chosen == [[0, 1, 0, 3][k]] and outs == winners()[k:k + 1]


def test_the_list_order_decides_the_index_and_the_first_of_equals_wins(dc):
    outs, osz, st, chosen, _, _ = run(dc, fixtures(), [3, 2, 1, 0])
    assert st == [0] * 4 and chosen == [3, 2, 3, 0] and outs == winners()
    outs, osz, st, chosen, _, _ = run(dc, fixtures(), [1, 1])
    assert st == [0] * 4 and chosen == [0] * 4
    assert outs == [B.fixture_stream(name, 1) for name in B.SLICES]
    outs, st, chosen, _ = check_against_one_calls(dc, fixtures(), [7, 4])        # 4 and above: the all-zero row, twice
    assert st == [0] * 4 and chosen == [0] * 4


# ---- 3: the pairs of pick.bin that share one slice ---------------------------------------------------------------------
def test_pairs_of_pick_bin_give_the_references_s0_stream(dc):
    pairs = B.pairs()
    blocks = [(a.bytes(), a.lens, a.flags) for a, b in pairs]
    for a, b in pairs:
        assert (a.bytes(), a.lens, a.flags, a.vers) == (b.bytes(), b.lens, b.flags, b.vers) and (a.strat, b.strat) == (0, 1)
    assert [len(a.stream) for a, b in pairs] == [1350, 1711, 1818, 2181]
    assert all(len(a.stream) < len(b.stream) for a, b in pairs)
    outs, osz, st, chosen, _, _ = run(dc, blocks, [0, 1])
    assert st == [0] * 4 and chosen == [0] * 4 and outs == [a.stream for a, b in pairs]
    outs, osz, st, chosen, _, _ = run(dc, blocks, [1, 0], packed=True)
    assert st == [0] * 4 and chosen == [1] * 4 and outs == [a.stream for a, b in pairs]


# ---- 4: equivalence with the one-call ------------------------------------------------------------------------------------
def small(vers):
    return [(c.bytes(), c.lens, c.flags) for c in P.small_cases() if c.vers == vers]


@pytest.mark.parametrize("vers", (4, 3))
def test_one_strategy_is_the_one_call_status_included(dc, vers):
    cs = [c for c in P.small_cases() if c.vers == vers]
    by_strat = {}
    for c in cs:
        by_strat.setdefault(c.strat, []).append(c)
    for strat, group in sorted(by_strat.items()):
        blocks = [(c.bytes(), c.lens, c.flags) for c in group]
        outs, st, chosen, route = check_against_one_calls(dc, blocks, [strat], vers=vers)
        for c, o, s in zip(group, outs, st):
            if c.stream is not None:
                assert (s, o) == (0, c.stream), c.name
            else:
                assert (s, o) == (M.E_SIZE if c.name == "nrec0_bytes" else M.E_TABLE, None), c.name


@pytest.mark.parametrize("pair", list(itertools.permutations(range(4), 2)))
def test_every_ordered_pair_is_the_smaller_of_two_one_calls(dc, pair):
    """the four fixtures and the small cases: every strategy decided from statistics another candidate shaped"""
    check_against_one_calls(dc, fixtures() + small(4), list(pair))


# ---- 5: a refused candidate ----------------------------------------------------------------------------------------------
def test_a_refused_candidate_is_out_of_the_running(dc):
    c = [c for c in P.small_cases() if c.name == "first_len725"][0]
    block = (c.bytes(), c.lens, c.flags)
    two = one_calls(dc, [block], [0, 2], c.vers)[0]
    assert two[0] == (M.E_TABLE, None) and two[1][0] == 0
    outs, osz, st, chosen, _, route = run(dc, [block], [0, 2], vers=c.vers)
    assert st == [0] and chosen == [1] and outs == [two[1][1]]
    assert route["fqz_best"] == dict(blocks=1, candidates=1, counted=1, undecided=0, refused=1)
    outs, osz, st, chosen, _, route = run(dc, [block], [0], vers=c.vers)
    assert st == [M.E_TABLE] and chosen == [-1] and outs == [None] and osz == [0]
    assert route["fqz_best"] == dict(blocks=0, candidates=0, counted=1, undecided=0, refused=1)


# ---- 6: undecided ---------------------------------------------------------------------------------------------------------
def test_a_candidate_the_pick_cannot_decide_leaves_the_block_undecided(dc):
    dc.set_fqz_pick(0, 64)
    try:
        outs, osz, st, chosen, _, route = run(dc, fixtures(), [0, 1, 2, 3])
        assert st == [P.E_UNDECIDED] * 4 and chosen == [-1] * 4 and osz == [0] * 4      # (run: nothing was written)
        assert route["fqz_best"] == dict(blocks=0, candidates=0, counted=4, undecided=4, refused=0)
        # strategies 2 and 3 ask the average-quality question of nobody: without a READ2 record nothing is compared
        outs, osz, st, chosen, _, route = run(dc, fixtures(), [2, 3], packed=True)
        r2 = [any(f & 128 for f in b[2]) for b in fixtures()]
        assert r2 == [False, True, False, False]
        assert st == [P.E_UNDECIDED if x else 0 for x in r2]
        two = [min((B.fixture_stream(name, s) for s in (2, 3)), key=len) for name in B.SLICES]
        assert outs == [None if x else w for x, w in zip(r2, two)]
        assert route["fqz_best"] == dict(blocks=3, candidates=6, counted=1, undecided=1, refused=0)
    finally:
        dc.set_fqz_pick(0, 0)


def host_batch(dc, strats, want_host):
    import htscodecs_amd as H
    blocks = fixtures()
    dc.set_option("route_count", 1)
    try:
        dc.route_read("fqz_pick"); dc.route_read("fqz_best")
        outs, st, chosen, lens, flags = H.fqz_compress_best_batch([b[0] for b in blocks], [b[1] for b in blocks], [b[2] for b in blocks],
                                                                  strats, ctx=dc.ctx)
        pick, best = dc.route_read("fqz_pick"), dc.route_read("fqz_best")
    finally:
        dc.set_option("route_count", 0)
    assert st == [0] * 4 and outs == winners() and [strats[j] for j in chosen] == [0, 1, 0, 3]
    assert lens == [b[1] for b in blocks] and flags == [[f & 0xffff for f in b[2]] for b in blocks]
    assert pick["host"] == want_host and best["undecided"] == want_host and best["blocks"] == 4
    return best


def test_the_host_batch_gives_the_same_and_picks_the_undecided_blocks_on_the_host(dc):
    best = host_batch(dc, [0, 1, 2, 3], 0)
    assert best["counted"] == 4 and best["candidates"] == 16
    dc.set_fqz_pick(0, 64)
    try:
        best = host_batch(dc, [3, 2, 1, 0], 4)
        assert best["counted"] == 4 and best["candidates"] == 16       # the second trip counts no histogram
    finally:
        dc.set_fqz_pick(0, 0)


# ---- 7: confinement and capacity ------------------------------------------------------------------------------------------
def mixed():
    """twelve small slices and a fixture: several winners, sizes at every alignment"""
    return small(4)[:12] + fixtures()[3:]


def test_a_slot_one_byte_short_of_the_winner_is_a_capacity_error_and_writes_nothing(dc):
    blocks = mixed()
    strats = [0, 1, 2, 3]
    outs, st, chosen, _ = check_against_one_calls(dc, blocks, strats)
    assert st.count(0) >= 10
    caps = [len(o) - (1 if i % 2 else 0) if o is not None else 64 for i, o in enumerate(outs)]
    outs2, osz2, st2, chosen2, _, route = run(dc, blocks, strats, caps=caps)
    for i, o in enumerate(outs):
        if o is None:
            assert st2[i] == st[i]
        elif i % 2:
            # a loser may well fit: the test is the winner's
            assert st2[i] == M.E_CAPACITY and osz2[i] == 0 and outs2[i] is None and chosen2[i] == chosen[i], i
        else:
            assert st2[i] == 0 and outs2[i] == o, i
    assert route["fqz_best"]["blocks"] == st2.count(0)


def test_a_packed_arena_that_ends_inside_a_block_refuses_it_and_what_does_not_fit_behind(dc):
    blocks = mixed()
    strats = [0, 1, 2, 3]
    outs, osz, st, chosen, _, _ = run(dc, blocks, strats, packed=True)
    assert outs == check_against_one_calls(dc, blocks, strats)[0]
    ends = np.cumsum(osz)
    k = 7
    capacity = int(ends[k]) - 1                                      # ends inside block k
    outs2, osz2, st2, chosen2, _, route = run(dc, blocks, strats, packed=True, capacity=capacity)
    for i in range(len(blocks)):
        if st[i] != 0:
            assert st2[i] == st[i]
        elif ends[i] <= capacity:
            assert st2[i] == 0 and outs2[i] == outs[i], i
        else:
            assert st2[i] == M.E_CAPACITY and osz2[i] == 0 and chosen2[i] == chosen[i], i
    assert st2[k] == M.E_CAPACITY and st2[:k] == st[:k]
    # the sizing pass: no arena at all
    outs3, osz3, st3, _, _, _ = run(dc, blocks[:3], strats, packed=True, capacity=0)
    assert all(s != 0 for s in st3) and osz3 == [0] * 3


# ---- 8: chunks ------------------------------------------------------------------------------------------------------------
def test_the_same_batch_in_several_chunks(dc):
    blocks = (small(4) + small(3))[:24]
    strats = [0, 1, 2, 3]
    whole = run(dc, blocks, strats)
    keep = dc.get_option("max_workspace_mb")
    n, max_in, max_rec = len(blocks), max(len(b[0]) for b in blocks), max(len(b[1]) for b in blocks)
    try:
        dc.set_fqz_limits(0, B.max_sym(blocks))
        assert dc.fqz_best_chunk_blocks(n, 4, max_in, max_rec) == n
        for mb in (512, 256, 128, 64, 32, 16, 8):
            dc.set_option("max_workspace_mb", mb)
            chunk = dc.fqz_best_chunk_blocks(n, 4, max_in, max_rec)
            if chunk < n:
                break
        assert 1 <= chunk < n, chunk
        dc.set_fqz_limits(0, 0)
        parts = run(dc, blocks, strats)
        packed = run(dc, blocks, strats, packed=True)
    finally:
        dc.set_option("max_workspace_mb", keep)
        dc.set_fqz_limits(0, 0)
    assert parts[:5] == whole[:5] and packed[0] == whole[0] and packed[2:4] == whole[2:4]
    rounds = -(-n // chunk)
    assert parts[5]["launch"]["in_order"] == 3 * rounds, (parts[5]["launch"], chunk)       # a chunk: its pick, its encoder, its winners
    assert parts[5]["fqz_best"] == whole[5]["fqz_best"]


# ---- 9: the route ---------------------------------------------------------------------------------------------------------
def test_the_histogram_is_counted_once_a_slice_that_needs_it(dc):
    blocks = fixtures() + small(4)
    for strats in ([0, 1, 2, 3], [2, 3], [3], [1, 3, 3]):
        outs, osz, st, chosen, _, route = run(dc, blocks, strats)
        cands = one_calls(dc, blocks, strats)
        r, k = route["fqz_best"], len(strats)
        asks = any(s in (0, 1) for s in strats)                      # do_qa of rows 0 and 1, do_r2 of row 1
        slices = [b for b, c in zip(blocks, cands) if c[0][0] != M.E_UNSUPPORTED]
        assert r["counted"] == sum(1 for d, l, f in slices if asks or any(x & 128 for x in f)), (strats, r)
        refused = sum(1 for c in cands for s, o in c if s != 0)
        assert r["undecided"] == 0 and r["refused"] == refused and r["candidates"] == k * len(slices) - refused, (strats, r)
        assert r["blocks"] == st.count(0)
        assert route["fqz_enc"]["streams"] == sum(1 for (d, l, f), c in zip(blocks, cands) for s, o in c if s == 0 and len(d))
        assert route["fqz_pick"]["blocks"] == k * len(slices) and route["fqz_pick"]["undecided"] == 0


# ---- 10: the round trip ---------------------------------------------------------------------------------------------------
def test_every_winner_decodes_to_its_input_and_its_record_lengths(dc):
    blocks = fixtures() + small(4)
    outs, osz, st, chosen, lens_out, _ = run(dc, blocks, [0, 1, 2, 3])
    some = [(o, b, l) for o, b, l in zip(outs, blocks, lens_out) if o is not None and len(b[0])]
    assert len(some) >= 30
    streams = [o for o, b, l in some]
    back, st2, lens, nrec, _ = G.run_dev(dc, streams, [len(b[0]) for o, b, l in some], [len(l) for o, b, l in some])
    assert st2 == [0] * len(some)
    for i, (o, b, l) in enumerate(some):
        k = P.reached(l, len(b[0]))                                  # the records the encode loop reaches are the stream's
        assert back[i] == bytes(b[0]) and nrec[i] == k and lens[i] == l[:k], i


# ---- the calls' own refusals ------------------------------------------------------------------------------------------------
def test_a_bad_k_or_a_negative_strategy_refuses_the_call(dc):
    blocks = fixtures()[3:]
    for strats in ([], list(range(17)), [0, -1]):
        with pytest.raises(RuntimeError, match="strategies"):
            run(dc, blocks, strats)
        with pytest.raises(RuntimeError, match="strategies"):
            run(dc, blocks, strats, packed=True)
    outs, osz, st, chosen, _, _ = run(dc, blocks, [3] * 16)
    assert st == [0] and chosen == [0] and outs == [B.fixture_stream("qvar", 3)]


def test_blocks_above_the_maxima_are_not_read(dc):
    blocks = [(bytes(100), [50, 50], [0, 0]), (bytes(101), [101], [0]), (bytes(30), [10] * 3, [0] * 3)]
    outs, osz, st, chosen, _, route = run(dc, blocks, [0, 3], max_in=100, max_rec=2)
    assert st == [0, M.E_UNSUPPORTED, M.E_UNSUPPORTED] and chosen[1:] == [-1, -1]
    assert route["fqz_best"] == dict(blocks=1, candidates=2, counted=1, undecided=0, refused=0)
