"""rANS 4x8's packed and best-of-two device-resident calls (include/rans4x8_hip.h part 2a):
rans4x8_hip_compress_packed_dev, rans4x8_hip_compress_best_dev, rans4x8_hip_compress_best_packed_dev,
rans4x8_hip_peek_dev, rans4x8_hip_uncompress_packed_dev.

Expected bytes come from the 4x8 oracle (orc8_rans_compress, tests/cpu_libs.py) and from the slot calls
(rans4x8_hip_compress_dev / rans4x8_hip_uncompress_dev); best-of-two from the reference's caller loop over the oracle:
the smallest candidate, the first on a tie.  Every dense arena is a window at an odd offset of a larger allocation filled
with the position-dependent pattern of test_gpu_confinement.py, and every byte outside [0, min(total, capacity)) is
compared after each packed call - so a stray write, or a range that landed shifted, is seen in every test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import datagen
from test_gpu_confinement import pattern
from test_oracle4x8 import Codec8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(datagen.GOLDEN, "r4x8")
FIXTURES = sorted(os.listdir(GOLD))
NAMES = ("rans4x8_hip_compress_packed_dev", "rans4x8_hip_compress_best_dev", "rans4x8_hip_compress_best_packed_dev",
         "rans4x8_hip_peek_dev", "rans4x8_hip_uncompress_packed_dev")
OK, CAPACITY, TRUNCATED, UNSUPPORTED, EMPTY = 0, 1, 2, 6, 9
NONE = 0xFFFFFFFF
LEAD, GUARD = 4097, 4096                       # the dense arena starts at an odd offset of its allocation
SIZES = [1, 2, 3, 4, 5, 26, 27, 0, 63, 64, 65, 4095, 4096, 65537, 262145]      # one zero-length block in the middle
TEXTS = ("q4", "q8", "q40+dir", "qvar")
gpu = pytest.mark.gpu


def _blocks(sizes=SIZES):
    return [datagen.tile(TEXTS[i % 4], s, i).tobytes() for i, s in enumerate(sizes)]


# ---- CPU half ------------------------------------------------------------------------------------------------
def test_4x8_packed_symbols_are_declared_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x8_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    for meth in ("compress_packed_4x8", "compress_best_4x8", "peek_4x8", "uncompress_packed_4x8"):
        assert hasattr(codec.DeviceCodec, meth), meth


def test_4x8_packed_calls_refuse_a_null_context():
    import htscodecs_amd
    L = htscodecs_amd.load()
    meth = (C.c_int * 2)(0, 1)
    off = (C.c_uint64 * 1)()
    assert L.rans4x8_hip_compress_packed_dev(None, 0, None, None, None, None, 0, off, None, None, 0, None, 0, None) == -1
    assert L.rans4x8_hip_compress_best_dev(None, 0, None, None, None, None, None, None, None, None, 2, meth, None, 0, None) == -1
    assert L.rans4x8_hip_compress_best_packed_dev(None, 0, None, None, None, None, 0, off, None, None, 2, meth, None, 0, None) == -1
    assert L.rans4x8_hip_peek_dev(None, 0, None, None, None, None, None, None, 0, None) == -1
    assert L.rans4x8_hip_uncompress_packed_dev(None, 0, None, None, None, None, 0, off, None, None, 0, 0, None) == -1


# ---- GPU half ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


@pytest.fixture(scope="module")
def dc(H):
    return H.DeviceCodec(0)


@pytest.fixture(scope="module")
def orc8():
    import cpu_libs
    return Codec8(cpu_libs.oracle().lib, "orc8_")


@pytest.fixture(scope="module")
def ref(orc8):
    """The blocks of tests 1, 3, 4 and 8 and the oracle's streams for both orders (None for the empty block): computed
    once, never changed."""
    blocks = _blocks()
    return blocks, [[orc8.compress(b, o) if len(b) else None for b in blocks] for o in (0, 1)]


class _In:
    """Blocks back to back (unaligned) in one device arena, 64 readable bytes behind the last."""

    def __init__(self, dc, blocks):
        import torch
        self.torch, self.dc, self.blocks, self.n = torch, dc, blocks, len(blocks)
        sizes = np.array([len(b) for b in blocks], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)])
        arena = np.zeros(int(off[-1]) + 64, dtype=np.uint8)
        for b, o in zip(blocks, off):
            arena[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        self.d_in = torch.from_numpy(arena).to(dc.dev)
        self.d_off = torch.from_numpy(off[:-1].copy()).to(dc.dev)
        self.d_size = torch.from_numpy(sizes.astype(np.int32)).to(dc.dev)
        self.max_in = max(1, int(sizes.max()))


class _Dense:
    """A dense output arena of `alloc` bytes: a window at an odd offset of an allocation that holds the pattern."""

    def __init__(self, dc, n, alloc):
        import torch
        self.torch, self.dc, self.n, self.alloc = torch, dc, n, alloc
        self.pat = pattern(LEAD + alloc + GUARD)
        self.arena = torch.from_numpy(self.pat.copy()).to(dc.dev)
        self.d_out = self.arena[LEAD:LEAD + alloc]
        assert self.d_out.data_ptr() % 2 == 1
        self.d_off = torch.full((n + 1,), -7, dtype=torch.int64, device=dc.dev)
        self.d_osz = torch.full((n,), -3, dtype=torch.int32, device=dc.dev)
        self.d_st = torch.full((n,), -3, dtype=torch.int32, device=dc.dev)
        self.d_chosen = torch.full((n,), -3, dtype=torch.int32, device=dc.dev)

    def read(self, capacity=None):
        """(offsets, sizes, statuses, chosen, window) after the call; asserts that nothing outside
        [0, min(total, capacity)) of the window - lead and guard included - was written."""
        self.torch.cuda.synchronize()
        off = self.d_off.cpu().numpy()
        got = self.arena.cpu().numpy()
        upto = min(int(off[-1]), self.alloc if capacity is None else capacity)
        outside = np.ones(len(got), dtype=bool)
        outside[LEAD:LEAD + upto] = False
        bad = np.nonzero((got != self.pat) & outside)[0]
        assert not len(bad), ("bytes written outside the results", bad[:8] - LEAD, upto)
        return off, self.d_osz.cpu().numpy(), self.d_st.cpu().numpy(), self.d_chosen.cpu().numpy(), got[LEAD:LEAD + self.alloc]


def _slot_encode(dc, L, b, order, d_order=None):
    """rans4x8_hip_compress_dev with slots of exactly the bound: (streams or None, statuses)."""
    import torch
    caps = np.array([L.rans4x8_hip_compress_bound(len(x)) for x in b.blocks], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum((caps + 255) // 256 * 256)])
    d_out = torch.zeros(int(off[-1]), dtype=torch.uint8, device=dc.dev)
    d_off = torch.from_numpy(off[:-1].copy()).to(dc.dev)
    d_cap = torch.from_numpy(caps.astype(np.int32)).to(dc.dev)
    d_osz = torch.full((b.n,), -3, dtype=torch.int32, device=dc.dev)
    d_st = torch.full((b.n,), -3, dtype=torch.int32, device=dc.dev)
    dc.compress_4x8(b.d_in, b.d_off, b.d_size, d_out, d_off, d_cap, d_osz, d_st, order, b.max_in, d_order=d_order)
    torch.cuda.synchronize()
    out, osz, st = d_out.cpu().numpy(), d_osz.cpu().numpy(), d_st.cpu().numpy()
    return [out[off[i]:off[i] + osz[i]].tobytes() if st[i] == 0 else None for i in range(b.n)], st


MODES = {"order0": (0, None), "order1": (1, None), "alternating": (0, [i & 1 for i in range(len(SIZES))])}


def _mode_args(dc, mode):
    import torch
    order, per = MODES[mode]
    return order, (torch.tensor(per, dtype=torch.int32, device=dc.dev) if per is not None else None), \
        [order if per is None else per[i] for i in range(len(SIZES))]


def _check_dense(blocks, want, off, osz, st, win, capacity=None):
    """Block by block against `want` (stream or None): bytes, size, status; offsets as the running sum of the
    uncut sizes; blocks that end beyond the capacity report CAPACITY with size 0."""
    assert off[0] == 0
    at = 0
    for i, w in enumerate(want):
        assert off[i] == at, i
        if w is None:
            assert len(blocks[i]) == 0 and (osz[i], st[i]) == (0, EMPTY), (i, osz[i], st[i])    # a failed block counts 0
            continue
        at += len(w)
        if capacity is not None and at > capacity:
            assert (osz[i], st[i]) == (0, CAPACITY), (i, osz[i], st[i])
        else:
            assert (osz[i], st[i]) == (len(w), OK), (i, osz[i], st[i])
            assert win[off[i]:off[i] + len(w)].tobytes() == w, i
    assert off[len(want)] == at
    return at


@gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_packed_encode_against_the_oracle_and_the_slot_call(H, dc, ref, mode):
    """1. Sizes 1 .. 262,145 with a zero-length block in the middle, order 0 / order 1 / d_order alternating: bytes, sizes
    and statuses per block against the oracle and against rans4x8_hip_compress_dev with bound-sized slots (blocks under 4
    bytes fall to order 0 in both); d_out_off is the running sum, d_out_off[n] the total."""
    blocks, streams = ref
    L = H.load()
    b = _In(dc, blocks)
    order, d_order, per = _mode_args(dc, mode)
    want = [streams[per[i]][i] for i in range(b.n)]
    total = sum(len(w) for w in want if w)
    o = _Dense(dc, b.n, total + 100)
    dc.compress_packed_4x8(b.d_in, b.d_off, b.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, order, b.max_in, d_order=d_order)
    off, osz, st, _, win = o.read()
    assert _check_dense(blocks, want, off, osz, st, win) == total
    assert st[SIZES.index(0)] == EMPTY
    for i in (0, 1, 2):
        assert win[off[i]] == 0                                     # order byte: in_size < 4 is coded with order 0
    slot, slot_st = _slot_encode(dc, L, b, order, d_order)
    assert list(slot_st) == list(st)
    for i in range(b.n):
        assert slot[i] == want[i], i


@gpu
def test_reference_fixtures_through_packed_decode_and_encode(dc):
    """2. The reference's eight fixtures as one batch: the packed decode gives the stripped inputs, the packed encode of
    those gives the fixtures' streams laid back to back, byte for byte."""
    import torch
    comps, plains, orders = [], [], []
    for fn in FIXTURES:
        name, order = fn.rsplit(".", 1)
        with open(os.path.join(GOLD, fn), "rb") as f:
            comps.append(f.read())
        plains.append(datagen.base_text(name).tobytes())
        orders.append(int(order))
    assert len(comps) == 8
    c = _In(dc, comps)
    raw_total = sum(len(p) for p in plains)
    o = _Dense(dc, c.n, raw_total)
    dc.uncompress_packed_4x8(c.d_in, c.d_off, c.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, c.max_in, max(len(p) for p in plains))
    off, osz, st, _, win = o.read()
    assert list(st) == [OK] * 8 and list(osz) == [len(p) for p in plains]
    assert list(off) == list(np.concatenate([[0], np.cumsum([len(p) for p in plains])]))
    assert win[:raw_total].tobytes() == b"".join(plains)
    p = _In(dc, plains)
    e = _Dense(dc, p.n, sum(len(x) for x in comps))
    dc.compress_packed_4x8(p.d_in, p.d_off, p.d_size, e.d_out, e.d_off, e.d_osz, e.d_st, 0, p.max_in,
                           d_order=torch.tensor(orders, dtype=torch.int32, device=dc.dev))
    off, osz, st, _, win = e.read()
    assert list(st) == [OK] * 8 and list(osz) == [len(x) for x in comps]
    assert off[8] == e.alloc and win.tobytes() == b"".join(comps)


def _cut_middle(want):
    """A capacity that ends inside block 12 (4,096 bytes of input): blocks 0 .. 11 fit, 12 is cut, the larger 13 and 14
    behind it are cut too."""
    return sum(len(w) for w in want[:12] if w) + len(want[12]) // 2


@gpu
@pytest.mark.parametrize("which", ["zero", "exact", "minus1", "middle"])
def test_capacity_rule(dc, ref, which):
    """3. out_capacity 0, the exact total, the total minus 1 and a value that cuts a middle block: blocks that fit are what
    the full run gives, cut blocks report CAPACITY with size 0, d_out_off is the same in all runs, and no byte at or
    beyond the capacity is written."""
    blocks, streams = ref
    b = _In(dc, blocks)
    order, d_order, per = _mode_args(dc, "alternating")
    want = [streams[per[i]][i] for i in range(b.n)]
    total = sum(len(w) for w in want if w)
    capacity = {"zero": 0, "exact": total, "minus1": total - 1, "middle": _cut_middle(want)}[which]
    o = _Dense(dc, b.n, total + 100)
    dc.compress_packed_4x8(b.d_in, b.d_off, b.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, order, b.max_in, d_order=d_order,
                           out_capacity=capacity)
    off, osz, st, _, win = o.read(capacity)
    assert _check_dense(blocks, want, off, osz, st, win, capacity) == total
    cut = [i for i in range(b.n) if st[i] == CAPACITY]
    assert cut == {"zero": [i for i in range(b.n) if want[i]], "exact": [], "minus1": [b.n - 1], "middle": [12, 13, 14]}[which]


@gpu
def test_confinement_of_encode_best_and_decode(dc, ref):
    """4. d_out at an odd offset inside a larger arena that holds the pattern; after the packed encode, the packed
    best-of-two and the packed decode - each with room to spare and with a capacity that cuts the last block - every
    byte outside [0, min(total, capacity)) still holds it (_Dense.read asserts that).  The best-of-two's d_chosen is -1 for
    the blocks the capacity cuts."""
    blocks, streams = ref
    b = _In(dc, blocks)
    want = [streams[1][i] for i in range(b.n)]
    total = sum(len(w) for w in want if w)
    for capacity in (None, total - 1000):
        o = _Dense(dc, b.n, total + 4096)
        dc.compress_packed_4x8(b.d_in, b.d_off, b.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, 1, b.max_in, out_capacity=capacity)
        off, osz, st, _, win = o.read(capacity)
        assert _check_dense(blocks, want, off, osz, st, win, capacity) == total
    best = [min((streams[m][i] for m in (1, 0)), key=len) if len(blocks[i]) else None for i in range(b.n)]
    btotal = sum(len(w) for w in best if w)
    for capacity in (None, btotal - 1000):
        o = _Dense(dc, b.n, btotal + 4096)
        dc.compress_best_4x8(b.d_in, b.d_off, b.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, [1, 0], b.max_in, chosen=o.d_chosen,
                             packed=True, out_capacity=capacity)
        off, osz, st, chosen, win = o.read(capacity)
        assert _check_dense(blocks, best, off, osz, st, win, capacity) == btotal
        assert (CAPACITY in st) == (capacity is not None)
        for i in range(b.n):                                        # a cut block has no winner, like a failed one
            fits = best[i] is not None and st[i] != CAPACITY
            assert chosen[i] == ((0 if len(streams[1][i]) <= len(streams[0][i]) else 1) if fits else -1), (i, chosen[i], st[i])
    comps = [w for w in want if w]
    plains = [x for x in blocks if len(x)]
    c = _In(dc, comps)
    raw_total = sum(len(x) for x in plains)
    for capacity in (None, raw_total - 1000):
        o = _Dense(dc, c.n, raw_total + 4096)
        dc.uncompress_packed_4x8(c.d_in, c.d_off, c.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, c.max_in, max(SIZES), out_capacity=capacity)
        off, osz, st, _, win = o.read(capacity)
        assert _check_dense(plains, plains, off, osz, st, win, capacity) == raw_total


BEST_SIZES = SIZES + [1000, 70001]             # two blocks of constant bytes behind the sizes of test 1


def _best_blocks():
    return _blocks() + [datagen.const(1000, 65).tobytes(), datagen.const(70001, 33).tobytes()]


@pytest.fixture(scope="module")
def best_ref(orc8, ref):
    blocks = _best_blocks()
    streams = [ref[1][o] + [orc8.compress(b, o) for b in blocks[len(SIZES):]] for o in (0, 1)]
    return blocks, streams


def _reference_loop(streams, methods, i):
    """The caller's loop of a CRAM 3.0 writer over the oracle: every method in turn, a result kept when it is smaller
    than the best so far.  (winner's index into methods, its bytes)."""
    best, idx = None, -1
    for j, m in enumerate(methods):
        s = streams[m][i]
        if s is not None and (best is None or len(s) < len(best)):
            best, idx = s, j
    return idx, best


@gpu
@pytest.mark.parametrize("methods", [[0, 1], [1, 0], [1, 1], [0]], ids=lambda m: "m" + "".join(map(str, m)))
def test_best_of_two_slot_and_packed(H, dc, best_ref, methods):
    """5. Winner's bytes and d_chosen against the reference loop over the oracle, in the slot form (one block's slot 1 byte
    short of its winner: CAPACITY) and the packed form (offsets, `dense` route count); blocks under 4 bytes tie and choose
    index 0 whatever the order of the methods."""
    import torch
    blocks, streams = best_ref
    L = H.load()
    b = _In(dc, blocks)
    want = [_reference_loop(streams, methods, i) for i in range(b.n)]
    for i, s in enumerate(BEST_SIZES):
        if 0 < s < 4:
            assert streams[0][i] == streams[1][i] and want[i][0] == 0, i
    dc.set_option("route_count", 1)
    try:
        dc.route_read("result")
        # packed form
        total = sum(len(w) for _, w in want if w)
        o = _Dense(dc, b.n, total + 64)
        dc.compress_best_4x8(b.d_in, b.d_off, b.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, methods, b.max_in, chosen=o.d_chosen,
                             packed=True)
        off, osz, st, chosen, win = o.read()
        assert _check_dense(blocks, [w for _, w in want], off, osz, st, win) == total
        assert list(chosen) == [j for j, _ in want]
        assert dc.route_read("result") == {"in_slot": 0, "dense": b.n, "gathered": 0}
        # slot form: tight slots (the winner's size, not the bound), one of them 1 byte short
        short = BEST_SIZES.index(4096)
        caps = np.array([len(w) if w else 16 for _, w in want], dtype=np.int64)
        caps[short] -= 1
        soff = np.concatenate([[0], np.cumsum(caps)])
        pat = pattern(LEAD + int(soff[-1]) + GUARD)
        arena = torch.from_numpy(pat.copy()).to(dc.dev)
        d_off = torch.from_numpy(soff[:-1].copy()).to(dc.dev)
        d_cap = torch.from_numpy(caps.astype(np.int32)).to(dc.dev)
        d_osz, d_st, d_chosen = (torch.full((b.n,), -3, dtype=torch.int32, device=dc.dev) for _ in range(3))
        dc.compress_best_4x8(b.d_in, b.d_off, b.d_size, arena[LEAD:], d_off, d_osz, d_st, methods, b.max_in, chosen=d_chosen,
                             out_cap=d_cap)
        torch.cuda.synchronize()
        assert dc.route_read("result") == {"in_slot": b.n, "dense": 0, "gathered": 0}
    finally:
        dc.set_option("route_count", 0)
    got, osz, st, chosen = arena.cpu().numpy(), d_osz.cpu().numpy(), d_st.cpu().numpy(), d_chosen.cpu().numpy()
    expect = pat.copy()
    for i, (j, w) in enumerate(want):
        if w is None:
            assert (osz[i], st[i], chosen[i]) == (0, EMPTY, -1), i
        elif i == short:
            assert (osz[i], st[i], chosen[i]) == (0, CAPACITY, -1), i
        else:
            assert (osz[i], st[i], chosen[i]) == (len(w), OK, j), i
            expect[LEAD + soff[i]:LEAD + soff[i] + len(w)] = np.frombuffer(w, dtype=np.uint8)
    assert np.array_equal(got, expect)                              # the winners in their slots, nothing else written


@gpu
def test_best_of_two_refuses_bad_methods_and_enqueues_nothing(H, dc, best_ref):
    """5 (end). k = 0, k = 3 and method 2 return -1; no output array is touched."""
    import torch
    blocks, _ = best_ref
    L = H.load()
    b = _In(dc, blocks[:4])
    o = _Dense(dc, b.n, 4096)
    d_cap = torch.full((b.n,), 1024, dtype=torch.int32, device=dc.dev)
    d_soff = torch.arange(b.n, dtype=torch.int64, device=dc.dev) * 1024
    stream = C.c_void_p(torch.cuda.current_stream(dc.dev).cuda_stream)
    for methods, k in (([0, 1], 0), ([0, 1, 0], 3), ([0, 2], 2), ([2], 1), ([-1, 0], 2)):
        meth = (C.c_int * len(methods))(*methods)
        assert L.rans4x8_hip_compress_best_packed_dev(dc.ctx.h, b.n, b.d_in.data_ptr(), b.d_off.data_ptr(), b.d_size.data_ptr(),
                                                      o.d_out.data_ptr(), 4096, o.d_off.data_ptr(), o.d_osz.data_ptr(),
                                                      o.d_st.data_ptr(), k, meth, o.d_chosen.data_ptr(), b.max_in, stream) == -1
        assert L.rans4x8_hip_compress_best_dev(dc.ctx.h, b.n, b.d_in.data_ptr(), b.d_off.data_ptr(), b.d_size.data_ptr(),
                                               o.d_out.data_ptr(), d_soff.data_ptr(), d_cap.data_ptr(), o.d_osz.data_ptr(),
                                               o.d_st.data_ptr(), k, meth, o.d_chosen.data_ptr(), b.max_in, stream) == -1
    torch.cuda.synchronize()
    assert np.array_equal(o.arena.cpu().numpy(), o.pat)
    assert o.d_off.tolist() == [-7] * (b.n + 1)
    assert o.d_osz.tolist() == o.d_st.tolist() == o.d_chosen.tolist() == [-3] * b.n


@gpu
def test_chunked_calls_and_two_streams(H, orc8):
    """6. 600 blocks of 4 .. 16 KiB on a context whose max_workspace_mb is 40: an encode item takes 598,272 bytes of
    workspace (image 137,472 + table 198,656 + scratch 262,144) and a decode block 214,272, so the unchunked packed
    encode, best-of-two and packed decode take 359, 718 and 129 MB - asserted from the workspace of a second context
    without the cap being at least three times the cap, and the capped context's workspace staying under it: three
    chunks or more each.  Results equal the unchunked ones, and the same batch issued on two streams one after the
    other gives identical results."""
    import torch
    cap_mb = 40
    rs = np.random.RandomState(600)
    sizes = [int(s) for s in rs.randint(4096, 16385, size=600)]
    blocks = _blocks(sizes)
    small, big = H.DeviceCodec(0), H.DeviceCodec(0)
    small.set_option("max_workspace_mb", cap_mb)
    want1 = [orc8.compress(x, 1) for x in blocks[:40]]

    def run(dc, what, b, alloc):
        o = _Dense(dc, b.n, alloc)
        if what == "encode":
            dc.compress_packed_4x8(b.d_in, b.d_off, b.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, 1, b.max_in)
        elif what == "best":
            dc.compress_best_4x8(b.d_in, b.d_off, b.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, [0, 1], b.max_in, chosen=o.d_chosen,
                                 packed=True)
        else:
            dc.uncompress_packed_4x8(b.d_in, b.d_off, b.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, b.max_in, 16384)
        return o

    def same(x, y):
        return all(np.array_equal(p, q) for p, q in zip(x, y))

    raw_total = sum(sizes)
    comps = None
    for what in ("decode", "encode", "best"):                       # (the unchunked workspace only grows: smallest first)
        if what == "decode":
            b = _In(small, blocks)
            o = run(small, "encode", b, raw_total)
            off, osz, st, _, win = o.read()
            assert not st.any()
            comps = [win[off[i]:off[i + 1]].tobytes() for i in range(600)]
            assert comps[:40] == want1
            small = H.DeviceCodec(0)                                 # (a fresh capped context: its workspace starts at 0)
            small.set_option("max_workspace_mb", cap_mb)
            src = [_In(small, comps), _In(big, comps)]
        else:
            src = [_In(small, blocks), _In(big, blocks)]
        full = run(big, what, src[1], raw_total).read()
        assert big.workspace_bytes() >= 3 * (cap_mb << 20), (what, big.workspace_bytes())
        first = run(small, what, src[0], raw_total).read()
        assert 0 < small.workspace_bytes() <= cap_mb << 20, (what, small.workspace_bytes())
        assert not full[2].any() and same(full, first), what
        torch.cuda.synchronize()
        outs = []
        for _ in range(2):                                          # two streams, one after the other, no host wait between
            with torch.cuda.stream(torch.cuda.Stream(device=small.dev)):
                outs.append(run(small, what, src[0], raw_total))
        for o in outs:
            assert same(o.read(), first), what
        if what == "decode":
            assert first[4][:raw_total].tobytes() == b"".join(blocks)
        if what == "best":
            assert set(first[3].tolist()) <= {0, 1}


def _slot_decode(dc, b, caps):
    import torch
    off = np.concatenate([[0], np.cumsum(np.maximum(np.array(caps, dtype=np.int64), 1) + 64)])
    d_out = torch.zeros(int(off[-1]), dtype=torch.uint8, device=dc.dev)
    d_off = torch.from_numpy(off[:-1].copy()).to(dc.dev)
    d_cap = torch.tensor(caps, dtype=torch.int32, device=dc.dev)
    d_osz = torch.full((b.n,), -3, dtype=torch.int32, device=dc.dev)
    d_st = torch.full((b.n,), -3, dtype=torch.int32, device=dc.dev)
    dc.uncompress_4x8(b.d_in, b.d_off, b.d_size, d_out, d_off, d_cap, d_osz, d_st)
    torch.cuda.synchronize()
    out, osz, st = d_out.cpu().numpy(), d_osz.cpu().numpy(), d_st.cpu().numpy()
    return [out[off[i]:off[i] + osz[i]].tobytes() for i in range(b.n)], osz, st


@gpu
def test_peek_and_packed_decode_on_hostile_input(dc, orc8):
    """7. Streams of 0, 1, 8 and 9 bytes; a valid stream whose size field says max_out_size + 1, 0xFFFFFFFF and the true
    size + 1 / - 1 (those two: whatever rans4x8_hip_uncompress_dev reports at that capacity); one block above
    max_in_size.  The neighbours of every refused block decode intact and the offsets follow the claims."""
    import torch
    max_in, max_out = 60000, 70000
    plain = [datagen.tile(TEXTS[i % 4], 5000 + 37 * i, i).tobytes() for i in range(8)]
    valid = [orc8.compress(p, i & 1) for i, p in enumerate(plain)]

    def sized(s, v):
        return s[:5] + int(v).to_bytes(4, "little") + s[9:]

    large = orc8.compress(datagen.rand(64000, 7).tobytes(), 0)
    assert len(large) > max_in and all(len(v) <= max_in for v in valid)
    nine = bytes([0, 0, 0, 0, 0, 100, 0, 0, 0])
    streams = [valid[0], b"", valid[1], b"\x01", bytes(range(8)), valid[2], nine, valid[3], sized(valid[4], max_out + 1),
               valid[5], sized(valid[4], NONE), sized(valid[6], len(plain[6]) + 1), valid[7], sized(valid[6], len(plain[6]) - 1),
               large, valid[0]]
    kind = ["ok", EMPTY, "ok", TRUNCATED, TRUNCATED, "ok", "decoder", "ok", UNSUPPORTED, "ok", UNSUPPORTED, "decoder", "ok",
            "decoder", UNSUPPORTED, "ok"]
    b = _In(dc, streams)
    n = b.n
    # peek
    d_fmt, d_raw, d_pst = (torch.full((n,), -5, dtype=torch.int32, device=dc.dev) for _ in range(3))
    dc.peek_4x8(b.d_in, b.d_off, b.d_size, d_fmt, d_raw, d_pst, max_in)
    torch.cuda.synchronize()
    fmt, raw, pst = d_fmt.tolist(), [r & NONE for r in d_raw.tolist()], d_pst.tolist()
    claims = []
    for i, s in enumerate(streams):
        if len(s) == 0:
            assert (fmt[i], raw[i], pst[i]) == (-1, NONE, EMPTY), i
        elif len(s) > max_in:
            assert (fmt[i], raw[i], pst[i]) == (-1, NONE, UNSUPPORTED), i
        elif len(s) < 9:
            assert (fmt[i], raw[i], pst[i]) == (s[0], NONE, TRUNCATED), i
        else:
            assert (fmt[i], raw[i], pst[i]) == (s[0], int.from_bytes(s[5:9], "little"), OK), i
        claims.append(raw[i] if pst[i] == OK and raw[i] <= max_out else 0)
    # the slot call's verdict on every block at capacity = claim
    ref_out, ref_osz, ref_st = _slot_decode(dc, b, claims)
    # packed decode
    total = sum(claims)
    o = _Dense(dc, n, total + 64)
    dc.uncompress_packed_4x8(b.d_in, b.d_off, b.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, max_in, max_out)
    off, osz, st, _, win = o.read()
    assert list(off) == list(np.concatenate([[0], np.cumsum(claims)]))
    it = iter(plain[:4] + [plain[5], plain[7], plain[0]])
    for i, k in enumerate(kind):
        if k == "ok":
            p = next(it)
            assert (osz[i], st[i]) == (len(p), OK) and win[off[i]:off[i + 1]].tobytes() == p, i
        elif k == "decoder":
            assert st[i] == ref_st[i] and osz[i] == ref_osz[i], (i, st[i], ref_st[i])
            assert win[off[i]:off[i] + osz[i]].tobytes() == ref_out[i], i
            assert off[i + 1] - off[i] == claims[i]                 # a block that fails while decoding keeps its range
        else:
            assert (osz[i], st[i]) == (0, k) and off[i + 1] == off[i], (i, osz[i], st[i])
    assert st[6] == TRUNCATED and osz[6] == 0                       # nine bytes: peek lets it through, the decoder refuses it


@gpu
def test_round_trip_without_a_read_back(dc, ref):
    """8. The packed encode's d_out / d_out_off / d_out_size go straight into the packed decode (the offsets as d_in_off);
    the host touches only the final comparison."""
    blocks, _ = ref
    b = _In(dc, blocks)
    bound = dc.L.rans4x8_hip_compress_bound(b.max_in)
    e = _Dense(dc, b.n, sum(SIZES) + 64 * len(SIZES) + 4096)
    order, d_order, _ = _mode_args(dc, "alternating")
    dc.compress_packed_4x8(b.d_in, b.d_off, b.d_size, e.d_out, e.d_off, e.d_osz, e.d_st, order, b.max_in, d_order=d_order)
    o = _Dense(dc, b.n, sum(SIZES) + 64)
    dc.uncompress_packed_4x8(e.d_out, e.d_off, e.d_osz, o.d_out, o.d_off, o.d_osz, o.d_st, bound, b.max_in)
    off, osz, st, _, win = o.read()
    assert list(osz) == SIZES and list(off) == list(np.concatenate([[0], np.cumsum(SIZES)]))
    assert [s for s in st if s] == [EMPTY] and st[SIZES.index(0)] == EMPTY
    assert win[:sum(SIZES)].tobytes() == b"".join(blocks)


@gpu
def test_sizing_pass_without_an_arena(H, dc, ref):
    """d_out == NULL with out_capacity == 0 in the three packed calls: the call is enqueued, every block that needs room
    reports CAPACITY with size 0 (d_chosen -1), a refused block keeps its status, d_out_off is what the full run gives -
    and the context takes the next call as usual."""
    import torch
    blocks, streams = ref
    L = H.load()
    b = _In(dc, blocks)
    stream = C.c_void_p(torch.cuda.current_stream(dc.dev).cuda_stream)
    empty = SIZES.index(0)

    def check(o, sizes, refused):
        torch.cuda.synchronize()
        assert o.d_off.tolist() == [0] + list(np.cumsum(sizes))
        assert o.d_osz.tolist() == [0] * len(sizes)
        assert o.d_st.tolist() == [refused if s == 0 else CAPACITY for s in sizes]

    want = [streams[1][i] for i in range(b.n)]
    o = _Dense(dc, b.n, 64)
    assert L.rans4x8_hip_compress_packed_dev(dc.ctx.h, b.n, b.d_in.data_ptr(), b.d_off.data_ptr(), b.d_size.data_ptr(), None, 0,
                                             o.d_off.data_ptr(), o.d_osz.data_ptr(), o.d_st.data_ptr(), 1, None, b.max_in,
                                             stream) == 0
    check(o, [len(w) if w else 0 for w in want], EMPTY)
    best = [min((streams[m][i] for m in (0, 1)), key=len) if len(blocks[i]) else None for i in range(b.n)]
    o = _Dense(dc, b.n, 64)
    meth = (C.c_int * 2)(0, 1)
    assert L.rans4x8_hip_compress_best_packed_dev(dc.ctx.h, b.n, b.d_in.data_ptr(), b.d_off.data_ptr(), b.d_size.data_ptr(), None, 0,
                                                  o.d_off.data_ptr(), o.d_osz.data_ptr(), o.d_st.data_ptr(), 2, meth,
                                                  o.d_chosen.data_ptr(), b.max_in, stream) == 0
    check(o, [len(w) if w else 0 for w in best], EMPTY)
    assert o.d_chosen.tolist() == [-1] * b.n
    comps = [w if w else b"" for w in want]                         # (the empty block's place: a stream of no bytes)
    c = _In(dc, comps)
    o = _Dense(dc, c.n, 64)
    assert L.rans4x8_hip_uncompress_packed_dev(dc.ctx.h, c.n, c.d_in.data_ptr(), c.d_off.data_ptr(), c.d_size.data_ptr(), None, 0,
                                               o.d_off.data_ptr(), o.d_osz.data_ptr(), o.d_st.data_ptr(), c.max_in, max(SIZES),
                                               stream) == 0
    check(o, SIZES, EMPTY)
    assert np.array_equal(o.arena.cpu().numpy(), o.pat)
    # the same context, the full run
    total = sum(SIZES)
    o = _Dense(dc, c.n, total)
    dc.uncompress_packed_4x8(c.d_in, c.d_off, c.d_size, o.d_out, o.d_off, o.d_osz, o.d_st, c.max_in, max(SIZES))
    off, osz, st, _, win = o.read()
    assert list(osz) == SIZES and st[empty] == EMPTY and win[:total].tobytes() == b"".join(blocks)
