"""The parameter choice of fqzcomp_qual encoding on the device (htscodecs_amd/csrc/r4x16_fqz_pick.hip,
include/rans4x16_hip.h part 2k).

The expected parameter bytes and streams are the reference's own: the 16 streams of tests/golden/fqzcomp and the cases of
tests/golden/fqzcomp/pick.bin whose bytes are kept (README.pick.md).  Everywhere else the answer is the host pick's
(rans4x16_hip_fqz_pick_parameters), which test_fqz_enc_cpu.py and test_fqz_pick_dev_cpu.py hold to the reference.
Everything is exact.  Every device call runs in the confinement layout of test_gpu_confinement.py: the slots a few bytes
apart at every alignment in an arena filled with a pattern, every byte outside them compared afterwards, the inputs at
odd places of their arenas and compared afterwards too."""
import numpy as np
import pytest

import fqz_enc_model as E
import fqz_model as M
import fqz_pick_cases as P
from test_gpu_confinement import Layout

pytestmark = pytest.mark.gpu
SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def dc():
    import htscodecs_amd as H
    return H.DeviceCodec(0)


def run(dc, blocks, vers=4, caps=None, compress=False, alias=False, max_in=None, max_rec=None, in_shift=0):
    """blocks: [(strat, data, lens, flags)].  One call of fqz_pick (or fqz_compress_pick) with per-block strategies.
    -> (slot bytes or None, sizes, statuses, lens out, flags out, route).  Asserts that nothing outside the slots and the
    blocks' record entries was written and that the inputs are as they were."""
    import torch as t
    from htscodecs_amd import codec
    n = len(blocks)
    if caps is None:
        caps = [E.cap(len(b[1]), len(b[2]), codec.fqz_pick_cap()) if compress else codec.fqz_pick_cap() for b in blocks]
    lay = Layout(caps, what=[len(b[1]) for b in blocks])
    in_off, rec_off, pos, rpos = [], [], 3 + in_shift, 2
    for i, (strat, data, lens, flags) in enumerate(blocks):
        in_off.append(pos); rec_off.append(rpos)
        pos += len(data) + 1 + i % 7
        rpos += len(lens) + i % 3
    arena_in = np.full(pos + 64, 0xee, dtype=np.uint8)
    a_len = np.full(rpos + 8, SENTINEL, dtype=np.int64)
    a_fl = np.full(rpos + 8, SENTINEL, dtype=np.int64)
    for (strat, data, lens, flags), o, ro in zip(blocks, in_off, rec_off):
        arena_in[o:o + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
        a_len[ro:ro + len(lens)] = lens
        a_fl[ro:ro + len(flags)] = flags
    as_i32 = lambda a: np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)
    dev = dc.dev
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(dev)
    i64 = lambda v: up(np.array(v, dtype=np.int64))
    d_in, d_out, d_len, d_fl = up(arena_in), up(lay.pattern.copy()), up(as_i32(a_len)), up(as_i32(a_fl))
    d_lo = d_len if alias else t.full_like(d_len, SENTINEL)
    d_fo = d_fl if alias else t.full_like(d_fl, SENTINEL)
    d_osz = t.full((n,), -7, dtype=t.int32, device=dev)
    d_st = t.full((n,), -7, dtype=t.int32, device=dev)
    sizes = up(as_i32([len(b[1]) for b in blocks]))
    nrec = up(as_i32([len(b[2]) for b in blocks]))
    d_strat = up(as_i32([b[0] for b in blocks]))
    max_in = max_in if max_in is not None else max([len(b[1]) for b in blocks] + [1])
    max_rec = max_rec if max_rec is not None else max([len(b[2]) for b in blocks] + [1])
    dc.set_option("route_count", 1)
    dc.set_fqz_limits(0, max([max(bytes(b[1])) for b in blocks if len(b[1])] + [1]))      # the model slots: no wider than the batch needs
    try:
        dc.route_read("fqz_pick"); dc.route_read("launch"); dc.route_read("fqz_enc")
        if compress:
            dc.fqz_compress_pick(d_in, i64(in_off), sizes, d_len, d_fl, i64(rec_off), nrec, d_out, up(lay.offs.copy()), up(as_i32(caps)),
                                 d_osz, d_st, max_in, max_rec, vers=vers, strat=99, d_strat=d_strat)
        else:
            dc.fqz_pick(d_in, i64(in_off), sizes, d_len, d_fl, i64(rec_off), nrec, d_out, up(lay.offs.copy()), up(as_i32(caps)), d_osz,
                        d_lo, d_fo, d_st, max_in, max_rec, vers=vers, strat=99, d_strat=d_strat)
        t.cuda.synchronize(dev)
        route, launch = dc.route_read("fqz_pick"), dc.route_read("launch")
    finally:
        dc.set_option("route_count", 0)
        dc.set_fqz_limits(0, 0)
    assert launch["side_by_side"] == 0 and launch["in_order"] >= 1
    arena = d_out.cpu().numpy()
    stray = lay.stray_writes(arena)
    assert stray is None, stray
    assert (d_in.cpu().numpy() == arena_in).all(), "the call changed its input"
    st, osz = d_st.tolist(), d_osz.tolist()
    lo, fo = d_lo.cpu().numpy().view(np.uint32), d_fo.cpu().numpy().view(np.uint32)
    if compress or not alias:                                        # the caller's records are only read
        assert (d_len.cpu().numpy() == as_i32(a_len)).all() and (d_fl.cpu().numpy() == as_i32(a_fl)).all()
    touched = np.zeros(len(lo), dtype=bool)
    lens_out, flags_out = [], []
    for i, (b, ro) in enumerate(zip(blocks, rec_off)):
        nr = len(b[2])
        if st[i] == 0 and not compress:
            touched[ro:ro + nr] = True
            lens_out.append(lo[ro:ro + nr].tolist()); flags_out.append(fo[ro:ro + nr].tolist())
        else:
            lens_out.append(None); flags_out.append(None)
    if not compress:
        before_l, before_f = (as_i32(a_len).view(np.uint32), as_i32(a_fl).view(np.uint32)) if alias else (None, None)
        for arr, before in ((lo, before_l), (fo, before_f)):
            want = before if alias else np.full(len(arr), SENTINEL, dtype=np.uint32)
            assert (arr[~touched] == want[~touched]).all(), "record entries of another block, or of a refused one, were written"
    outs = [x if s == 0 else None for x, s in zip(lay.take(arena, [max(z, 0) for z in osz]), st)]
    for i in range(n):
        if st[i] != 0:                                               # a refused block's slot is untouched
            o = int(lay.offs[i])
            assert (arena[o:o + caps[i]] == lay.pattern[o:o + caps[i]]).all(), i
            assert osz[i] == 0 or st[i] == M.E_CAPACITY
    return outs, osz, st, lens_out, flags_out, route


def check_against_host(dc, blocks, vers=4, **kw):
    """fqz_pick against rans4x16_hip_fqz_pick_parameters: bytes, lengths, flags, and the route against the host's census"""
    outs, osz, st, lens_out, flags_out, route = run(dc, blocks, vers=vers, **kw)
    for i, (strat, data, lens, flags) in enumerate(blocks):
        hst, par, hl, hf = P.host_pick(vers, strat, data, lens, flags)
        assert st[i] == hst == 0, (i, st[i], hst)
        assert outs[i] == par and lens_out[i] == hl and flags_out[i] == hf, (i, "differs from the host pick")
    want = P.census(vers, blocks)
    assert route == want, (route, want)
    return outs, route


# ---- the reference's answers ---------------------------------------------------------------------------------------
def fixture_blocks():
    return [(strat, data, lens, flags) for fn, vers, strat, data, lens, flags, stream in P.fixture_inputs()]


def test_the_16_fixtures_get_the_references_parameter_bytes(dc):
    outs, route = check_against_host(dc, fixture_blocks())
    assert outs == [E.params_of(x[6]) for x in P.fixture_inputs()]
    assert route["blocks"] == 16 and route["undecided"] == 0 and route["sel"] == 10 and route["dedup"] == 4


def test_the_16_fixtures_in_one_call_are_the_references_streams(dc):
    outs, osz, st, _, _, route = run(dc, fixture_blocks(), compress=True)
    assert st == [0] * 16 and route["blocks"] == 16 and route["undecided"] == 0
    assert outs == [x[6] for x in P.fixture_inputs()]


def kept(vers):
    return [c for c in P.small_cases() if c.vers == vers]


@pytest.mark.parametrize("vers", (4, 3))
def test_pick_bin_cases_get_the_references_parameter_bytes(dc, vers):
    cs = kept(vers)
    outs, route = check_against_host(dc, [(c.strat, c.bytes(), c.lens, c.flags) for c in cs], vers=vers)
    assert outs == [c.params for c in cs]
    assert route["undecided"] == 0 and route["blocks"] == len(cs)


_streams = {}


def pick_bin_streams(dc):
    """fqz_compress_pick over the kept cases, one batch a version, run once: {name: (status, bytes)}"""
    if not _streams:
        for vers in (4, 3):
            cs = kept(vers)
            outs, osz, st, _, _, route = run(dc, [(c.strat, c.bytes(), c.lens, c.flags) for c in cs], vers=vers, compress=True)
            assert route["undecided"] == 0 and route["blocks"] == len(cs)
            for c, o, s in zip(cs, outs, st):
                _streams[c.name] = (s, o)
    return _streams


@pytest.mark.parametrize("k", range(38))
def test_pick_bin_cases_in_one_call_are_the_references_streams(dc, k):
    """every case whose stream is kept - decoded back by the reference (README.pick.md); `overrun` among them: the encoder
    gets the records the encode loop reaches"""
    c = P.kept_cases()[k]
    st, out = pick_bin_streams(dc)[c.name]
    assert st == 0 and out == c.stream, (c.name, st)


def test_what_the_reference_did_not_decode_back_the_one_call_refuses(dc):
    """parameter bytes the header walk refuses (ptab = i >> 7: README.pick.md) and bytes without a record: the front end's
    statuses, as in part 2j; the pick alone gives the reference's bytes for all three (above)"""
    got = {c.name: pick_bin_streams(dc)[c.name] for c in P.small_cases() if c.stream is None}
    assert got == {"first_len725": (M.E_TABLE, None), "first_len1448": (M.E_TABLE, None), "nrec0_bytes": (M.E_SIZE, None)}


# ---- the kernels' edges, against the host pick -----------------------------------------------------------------------
def edge_blocks():
    rs = np.random.RandomState(5)
    q = lambda n, k=12: rs.randint(0, k, n).astype(np.uint8).tobytes()
    r2 = lambda n: [128 * int(v) for v in rs.randint(0, 2, n)]
    blocks = []
    for nrec in (1, 63, 64, 65, 129):
        lens = [int(v) for v in rs.randint(1, 40, nrec)]
        blocks.append((nrec % 4, q(sum(lens)), lens, r2(nrec)))
    for rl in (1, 127, 128, 129, 255, 256, 257):
        blocks.append((rl % 2, q(3 * rl), [rl] * 3, [0, 128, 0]))
    big = [x for x in E.hashed_vectors() if max(x[2]) == 70000][0]
    blocks.append((0, big[1], big[2], [f & 0xffff for f in big[3]]))
    blocks.append((0, b"\x07", [1], [0]))
    blocks.append((0, q(300), [], []))                               # no record, bytes: one record of direction 0
    blocks.append((1, b"", [], []))
    blocks.append((2, b"", [0, 0], [0, 128]))
    blocks.append((0, q(200), [50, 0, 0, 50, 0, 100], [0, 128, 0, 0, 128, 0]))           # zero-length records in the middle
    blocks.append((1, q(120), [50, 50, 50, 50, 7], [0, 128, 0, 128, 0]))                 # the list over-runs
    blocks.append((0, q(130), [0xffffffff, 0xfffffff0, 7], [0, 0, 0]))
    blocks.append((0, q(500), [100, 100], [128, 0]))                                     # the list under-runs
    blocks.append((0, bytes(400), [100] * 4, [0] * 4))                                   # max_sym 0
    blocks.append((1, bytes([255, 0, 255, 3] * 100), [100] * 4, [0, 128, 0, 128]))       # max_sym 255
    blocks.append((1, q(1000), [100] * 10, [128] * 10))                                  # all records READ2
    d = q(40)
    blocks.append((0, d * 25, [40] * 25, [0] * 25))                                      # every record a duplicate: dedup
    blocks.append((3, q(600, 60), [200] * 3, [(2 << 16) | 128, 1 << 16, 0]))             # a caller's selectors
    return blocks


def test_kernel_edges_in_one_heterogeneous_batch(dc):
    blocks = edge_blocks()
    outs, route = check_against_host(dc, blocks)
    assert route["blocks"] == len(blocks) and route["dedup"] >= 1 and route["split"] >= 1


def test_the_same_batch_in_several_chunks(dc):
    """a block takes 1 MiB of counters and more: under max_workspace_mb = 8 the batch runs in chunks of a few blocks"""
    keep = dc.get_option("max_workspace_mb")
    dc.set_option("max_workspace_mb", 8)
    try:
        blocks = [b for b in edge_blocks() if len(b[1]) < 4096]
        outs, osz, st, lens_out, flags_out, route = run(dc, blocks)
        outs2, _, st2, _, _, _ = run(dc, blocks, compress=True)
    finally:
        dc.set_option("max_workspace_mb", keep)
    for i, (strat, data, lens, flags) in enumerate(blocks):
        hst, par, hl, hf = P.host_pick(4, strat, data, lens, flags)
        assert st[i] == 0 and outs[i] == par and lens_out[i] == hl and flags_out[i] == hf, i
        k = P.reached(hl, len(data))                                # the encoder gets the records the encode loop reaches
        if st2[i] == 0:
            assert outs2[i] == E.compress(data, hl[:k], hf[:k], par), i
        else:
            assert st2[i] == E.verdict(data, hl[:k], hf[:k], par), i
    assert route["blocks"] == len(blocks)


@pytest.mark.parametrize("shift", range(16))
def test_blocks_starting_at_every_address_mod_16(dc, shift):
    rs = np.random.RandomState(shift)
    blocks = [(shift % 4, rs.randint(0, 9, 333).astype(np.uint8).tobytes(), [111] * 3, [0, 128, 0])]
    check_against_host(dc, blocks, in_shift=shift)


def test_one_slice_under_five_strategies_in_one_call_equals_five_calls(dc):
    fn, vers, strat, data, lens, flags, stream = P.fixture_inputs()[8]
    together, _ = check_against_host(dc, [(s, data, lens, flags) for s in range(5)])
    apart = [check_against_host(dc, [(s, data, lens, flags)])[0][0] for s in range(5)]
    assert together == apart and len(set(together)) >= 4


def test_len_out_and_flags_out_may_be_the_inputs(dc):
    check_against_host(dc, fixture_blocks()[8:12] + edge_blocks()[:5], alias=True)


def test_a_slot_one_byte_short_reports_the_size_and_writes_nothing(dc):
    blocks = fixture_blocks()[8:10]
    sizes = [len(P.host_pick(4, *b)[1]) for b in blocks]
    outs, osz, st, lens_out, flags_out, route = run(dc, blocks, caps=[sizes[0] - 1, sizes[1]])
    assert st == [M.E_CAPACITY, 0] and osz == sizes and outs[0] is None and outs[1] == P.host_pick(4, *blocks[1])[1]
    assert route["blocks"] == 1


def test_blocks_above_the_maxima_and_negative_strategies_are_not_read(dc):
    blocks = [(0, bytes(100), [50, 50], [0, 0]), (-1, bytes(100), [50, 50], [0, 0]), (0, bytes(101), [101], [0]), (0, bytes(30), [10] * 3, [0] * 3)]
    outs, osz, st, _, _, route = run(dc, blocks, max_in=100, max_rec=2)
    assert st == [0, M.E_UNSUPPORTED, M.E_UNSUPPORTED, M.E_UNSUPPORTED] and route["blocks"] == 1


# ---- the guard -------------------------------------------------------------------------------------------------------
def test_guard_bits_40_leaves_every_non_zero_comparison_undecided(dc):
    """q4 under strategies 2 and 3 compares nothing (do_qa = 0, no READ2 record): still decided.  Every other fixture has a
    non-zero entropy comparison: undecided, nothing written (run() compares the slots and the record entries)."""
    dc.set_fqz_pick(0, 40)
    try:
        blocks = fixture_blocks()
        outs, osz, st, _, _, route = run(dc, blocks)
        outs2, _, st2, _, _, _ = run(dc, blocks, compress=True)
    finally:
        dc.set_fqz_pick(0, 0)
    names = [x[0] for x in P.fixture_inputs()]
    decided = [n for n, s in zip(names, st) if s == 0]
    assert set(st) == {0, P.E_UNDECIDED} and st2 == st
    assert {"q4.2", "q4.3"} <= set(decided)
    for n, s, o, x in zip(names, st, outs, P.fixture_inputs()):
        strat, r2 = x[2], any(f & 128 for f in x[5])
        assert (s == 0) == (strat >= 2 and not r2), n                # strategies 0 and 1 ask the average-quality question, READ2 the other
        if s == 0:
            assert o == E.params_of(x[6]), n
    assert route["undecided"] == st.count(P.E_UNDECIDED) and route["blocks"] == st.count(0)


# ---- the host batch --------------------------------------------------------------------------------------------------
def host_batch(dc, strat):
    import htscodecs_amd as H
    some = [x for x in P.fixture_inputs() if x[2] == strat]
    outs, st, lens, flags = H.fqz_compress_batch([x[3] for x in some], [x[4] for x in some], [x[5] for x in some], 4, strat, ctx=dc.ctx)
    assert st == [0] * len(some) and outs == [x[6] for x in some]
    assert lens == [x[4] for x in some] and flags == [[f & 0xffff for f in x[5]] for x in some]
    return len(some)


def test_the_host_batch_picks_on_the_device_and_falls_back(dc):
    dc.set_option("route_count", 1)
    try:
        dc.route_read("fqz_pick")
        for strat in range(4):                                       # mode 0: the pick's route stays empty
            host_batch(dc, strat)
        assert not any(dc.route_read("fqz_pick").values())
        dc.set_fqz_pick(1, 0)
        n = sum(host_batch(dc, strat) for strat in range(4))
        route = dc.route_read("fqz_pick")
        assert route["blocks"] == n == 16 and route["undecided"] == 0 and route["host"] == 0
        dc.set_fqz_pick(1, 40)
        n = sum(host_batch(dc, strat) for strat in range(4))
        route = dc.route_read("fqz_pick")
        assert route["undecided"] == route["host"] == 10 and route["blocks"] == 6          # strategies 2 and 3 without READ2 compare nothing
    finally:
        dc.set_fqz_pick(0, 0)
        dc.set_option("route_count", 0)
