"""The packed device-resident calls (include/rans4x16_hip.h part 2a): rans4x16_hip_compress_packed_dev,
rans4x16_hip_compress_best_packed_dev, rans4x16_hip_peek_dev, rans4x16_hip_uncompress_packed_dev.

Expected bytes always come from the oracle; best-of-k from the reference loop of test_gpu_best_dev.py.  The output arena
is filled with the position-dependent pattern of test_gpu_confinement.py, so that a byte written outside the blocks'
ranges - or a range that landed shifted - is seen.

What the input set (inputs() of test_gpu_best_dev.py: 53 blocks of 0 .. 200,000 bytes) holds, found by running the oracle
alone over it on the CPU (test_inputs_reach_both_branches_of_the_size_arithmetic asserts it): under every order of
DEVICE_ORDERS and STRIPE_ORDERS that does not ask for X_CAT itself (32 and 33 do: the explicit-CAT branch) at least one
block is entropy-coded (first byte without X_CAT) and at least one block is a CAT fall-back (plen >= dlen, rANS_static4x16pr.c:1332-1337: the uniformly random
blocks and the blocks of at most a few bytes) - the branch of the size kernel that no header flag announces."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_gpu_best_dev as B
from test_gpu_best_dev import DEVICE_ORDERS, NINE, STRIPE_ORDERS, inputs
from test_gpu_confinement import pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rans4x16_hip_compress_packed_dev", "rans4x16_hip_compress_best_packed_dev", "rans4x16_hip_peek_dev",
         "rans4x16_hip_uncompress_packed_dev")
TABLE3 = [0, (2 << 8) | 9, (7 << 8) | 0xc9]
GUARD = 4096
NONE = 0xFFFFFFFF


def _stream(oracle, i, data, order):
    return B._oracle_bytes(oracle, "in", i, data, order)


def _mixed(orders, n):
    return [orders[(5 * i) % len(orders)] for i in range(n)]


# ---- CPU half ------------------------------------------------------------------------------------------------
def test_packed_symbols_are_declared_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    for meth in ("compress_packed", "compress_best_packed", "peek", "uncompress_packed"):
        assert hasattr(codec.DeviceCodec, meth), meth
    assert re.search(r"\bR4X16_ROUTE_RESULT\s*=\s*4\b", header)


def test_packed_calls_refuse_a_null_context():
    import htscodecs_amd
    L = htscodecs_amd.load()
    meth = (C.c_int * 2)(0, 1)
    off = (C.c_uint64 * 1)()
    assert L.rans4x16_hip_compress_packed_dev(None, 0, None, None, None, None, 0, off, None, None, 0, None, 0, 0, None) == -1
    assert L.rans4x16_hip_compress_best_packed_dev(None, 0, None, None, None, None, 0, off, None, None, 2, meth, None, 0, 0, None) == -1
    assert L.rans4x16_hip_peek_dev(None, 0, None, None, None, None, None, None, 0, None) == -1
    assert L.rans4x16_hip_uncompress_packed_dev(None, 0, None, None, None, None, 0, off, None, None, None, 0, 0, None) == -1


def test_result_route_list_is_known():
    from htscodecs_amd import codec
    assert codec.ROUTE_WHICH["result"] == 4
    assert codec.ROUTE_KINDS["result"] == ("in_slot", "dense", "gathered")


def test_inputs_reach_both_branches_of_the_size_arithmetic(oracle):
    blocks = inputs()
    for order in DEVICE_ORDERS + STRIPE_ORDERS:
        first = [_stream(oracle, i, d, order)[0] for i, d in enumerate(blocks) if len(d)]
        if not order & 0x20:                        # (32 and 33 ask for X_CAT themselves: every block is stored, none falls back)
            assert any(not f & 0x20 for f in first), order
            assert any(f & 0x20 for f in first), order


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


@pytest.fixture
def routes(dc):
    dc.set_option("route_count", 1)
    dc.route_read("result")
    dc.route_read("launch")
    yield dc
    dc.set_option("route_count", 0)


class _Packed:
    """The blocks of a B._Batch (device input arena) and a dense output arena filled with the pattern."""

    def __init__(self, dc, blocks, alloc):
        import torch
        self.torch, self.dc, self.blocks, self.n = torch, dc, blocks, len(blocks)
        self.b = B._Batch(dc, blocks, [0] * len(blocks))
        self.alloc = alloc + GUARD
        self.pat = pattern(self.alloc)
        self.fresh()

    def fresh(self):
        torch, dev = self.torch, self.dc.dev
        self.d_out = torch.from_numpy(self.pat.copy()).to(dev)
        self.d_off = torch.full((self.n + 1,), -7, dtype=torch.int64, device=dev)
        self.d_osz = torch.full((self.n,), -3, dtype=torch.int32, device=dev)
        self.d_st = torch.full((self.n,), -3, dtype=torch.int32, device=dev)
        self.d_chosen = torch.full((self.n,), -3, dtype=torch.int32, device=dev)

    def compress(self, order=0, orders=None, capacity=None):
        b = self.b
        d_order = self.torch.tensor(orders, dtype=self.torch.int32, device=self.dc.dev) if orders is not None else None
        self.dc.compress_packed(b.d_in, b.d_in_off, b.d_in_size, self.d_out, self.d_off, self.d_osz, self.d_st, order, b.max_in,
                                d_order=d_order, total_in_size=b.total_in,
                                out_capacity=self.alloc - GUARD if capacity is None else capacity)

    def best(self, methods, capacity=None):
        b = self.b
        self.dc.compress_best_packed(b.d_in, b.d_in_off, b.d_in_size, self.d_out, self.d_off, self.d_osz, self.d_st, methods,
                                     b.max_in, chosen=self.d_chosen, total_in_size=b.total_in,
                                     out_capacity=self.alloc - GUARD if capacity is None else capacity)

    def read(self):
        self.torch.cuda.synchronize()
        return (self.d_out.cpu().numpy(), self.d_off.cpu().numpy().tolist(), self.d_osz.cpu().numpy().tolist(),
                self.d_st.cpu().numpy().tolist(), self.d_chosen.cpu().numpy().tolist())


def _prefix(sizes):
    return [0] + np.cumsum(sizes).tolist()


def _check_dense(p, want, what, capacity=None):
    """want[i]: the bytes of block i.  Without a capacity everything fits; with one, blocks that end beyond it are refused."""
    arena, off, osz, st, _ = p.read()
    need = _prefix([len(w) for w in want])
    assert off == need, (what, off[:5], need[:5])
    cap = p.alloc - GUARD if capacity is None else capacity
    first_refused = next((i for i in range(p.n) if need[i + 1] > cap), p.n)
    for i, w in enumerate(want):
        if need[i + 1] > cap:
            assert st[i] == 1 and osz[i] == 0, (what, i, st[i], osz[i])
        else:
            assert st[i] == 0 and osz[i] == len(w), (what, i, st[i], osz[i], len(w))
            assert arena[need[i]:need[i + 1]].tobytes() == w, (what, i, len(p.blocks[i]))
    # later blocks all end beyond the capacity too (every stream has at least one byte): nothing from the first refused
    # block's start on is written - in particular nothing from min(off[n], capacity) to the end of the allocation
    keep = need[first_refused] if first_refused < p.n else need[-1]
    assert keep <= min(need[-1], cap) or first_refused == p.n
    assert np.array_equal(arena[keep:], p.pat[keep:]), (what, "bytes behind the last written block changed")
    return arena, off, osz, st


def _slot_call(H, dc, blocks, order=0, orders=None):
    import torch
    per = orders if orders is not None else [order] * len(blocks)
    batch = B._Batch(dc, blocks, [H.rans_compress_bound_4x16(len(b), o) for b, o in zip(blocks, per)])
    d_order = torch.tensor(orders, dtype=torch.int32, device=dc.dev) if orders is not None else None
    dc.compress(batch.d_in, batch.d_in_off, batch.d_in_size, batch.d_out, batch.d_out_off, batch.d_cap, batch.d_osz, batch.d_st,
                order, batch.max_in, d_order=d_order)
    _, _, st, osz = batch.read()
    return st, osz


def _alloc_for(want):
    return sum(len(w) for w in want)


@pytest.mark.gpu
@pytest.mark.parametrize("order", DEVICE_ORDERS)
def test_dense_equals_the_concatenation(H, routes, oracle, order):
    dc, blocks = routes, inputs()
    assert {0, 1, 3, 4, 20, 21, 200000} <= {len(b) for b in blocks}
    want = [_stream(oracle, i, d, order) for i, d in enumerate(blocks)]
    p = _Packed(dc, blocks, _alloc_for(want))
    p.compress(order=order)
    arena, off, osz, st = _check_dense(p, want, order)
    assert arena[:off[-1]].tobytes() == b"".join(want)
    r = dc.route_read("result")
    assert r["dense"] == len(blocks) and r["gathered"] == 0 and r["in_slot"] == 0, r
    assert (st, osz) == _slot_call(H, dc, blocks, order=order)
    assert dc.route_read("result")["in_slot"] == len(blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("enc_direct", [1, 0])
def test_dense_with_per_block_orders_and_without_the_short_step_routes(H, routes, oracle, enc_direct):
    dc, blocks = routes, inputs()
    keep = dc.get_option("enc_direct")
    try:
        dc.set_option("enc_direct", enc_direct)
        orders = _mixed(DEVICE_ORDERS, len(blocks))
        assert set(orders) == set(DEVICE_ORDERS)
        want = [_stream(oracle, i, d, o) for i, (d, o) in enumerate(zip(blocks, orders))]
        p = _Packed(dc, blocks, _alloc_for(want))
        p.compress(orders=orders)
        _, _, osz, st = _check_dense(p, want, ("mixed", enc_direct))
        r = dc.route_read("result")
        assert r["dense"] == len(blocks) and r["gathered"] == 0, r
        assert (st, osz) == _slot_call(H, dc, blocks, orders=orders)
        want1 = [_stream(oracle, i, d, 1) for i, d in enumerate(blocks)]
        p = _Packed(dc, blocks, _alloc_for(want1))
        p.compress(order=1)
        _check_dense(p, want1, ("order 1", enc_direct))
    finally:
        dc.set_option("enc_direct", keep)


@pytest.mark.gpu
@pytest.mark.parametrize("order", STRIPE_ORDERS + ["mixed"])
def test_gathered_route(H, routes, oracle, order):
    dc, blocks = routes, inputs()
    assert any(len(b) % 4 for b in blocks) and any(len(b) <= 20 for b in blocks)
    try:
        if order == "mixed":
            dc.set_stripe_encode(7)
            orders = _mixed(STRIPE_ORDERS + DEVICE_ORDERS, len(blocks))
            assert set(orders) == set(STRIPE_ORDERS + DEVICE_ORDERS)
            want = [_stream(oracle, i, d, o) for i, (d, o) in enumerate(zip(blocks, orders))]
            p = _Packed(dc, blocks, _alloc_for(want))
            p.compress(orders=orders)
        else:
            want = [_stream(oracle, i, d, order) for i, d in enumerate(blocks)]
            p = _Packed(dc, blocks, _alloc_for(want))
            p.compress(order=order)
        arena, off, osz, st = _check_dense(p, want, order)
        assert arena[:off[-1]].tobytes() == b"".join(want)
        r = dc.route_read("result")
        assert r["gathered"] == len(blocks) and r["dense"] == 0 and r["in_slot"] == 0, r
    finally:
        dc.set_stripe_encode(0)


def _check_best(p, ref, what, capacity=None):
    want = [c for c, _, _ in ref]
    _check_dense(p, want, what, capacity)
    _, off, _, st, chosen = p.read()
    for i, (_, m, _) in enumerate(ref):
        if st[i] == 0:
            assert chosen[i] == m, (what, i, chosen[i], m)       # the first of equal sizes wins: the loop's own choice


@pytest.mark.gpu
@pytest.mark.parametrize("methods", [NINE, TABLE3], ids=["nine", "planes-2-7"])
def test_best_of_k_packed(H, routes, oracle, methods):
    dc, blocks = routes, inputs()
    ref = B.reference_loop(oracle, "in", blocks, methods)
    assert all(c is not None for c, _, _ in ref)
    p = _Packed(dc, blocks, _alloc_for([c for c, _, _ in ref]))
    p.best(methods)
    _check_best(p, ref, methods)
    r = dc.route_read("result")
    assert r["gathered"] == len(blocks) and r["dense"] == 0 and r["in_slot"] == 0, r


@pytest.mark.gpu
def test_a_small_ceiling_walks_the_packed_calls_in_chunks(H, routes, oracle):
    """Dense: workspace and slot of a 200,000-byte order-1 block take more than 600 KB (r4x16_api.hip: enc_ws_layout's
    fixed records alone), so 53 blocks under 8 MiB are at least three chunks.  Best-of-k: as in
    test_gpu_best_dev.py, 100 MiB."""
    dc, blocks = routes, inputs()
    keep = dc.get_option("max_workspace_mb")
    want = [_stream(oracle, i, d, 1) for i, d in enumerate(blocks)]
    ref = B.reference_loop(oracle, "in", blocks, NINE)
    p = _Packed(dc, blocks, _alloc_for(want))
    q = _Packed(dc, blocks, _alloc_for([c for c, _, _ in ref]))
    p.compress(order=1)
    one_chunk = p.read()[0].copy()
    assert sum(dc.route_read("launch").values()) == 1
    assert dc.route_read("result")["dense"] == len(blocks)
    try:
        dc.set_option("max_workspace_mb", 8)
        assert len(blocks) * 600 * 1024 >= 3 * (8 << 20)
        p.fresh()
        p.compress(order=1)
        _check_dense(p, want, "dense chunks")
        assert sum(dc.route_read("launch").values()) >= 3
        assert dc.route_read("result")["dense"] == len(blocks)
        assert np.array_equal(p.read()[0], one_chunk)
        dc.set_option("max_workspace_mb", 100)
        q.best(NINE)
        _check_best(q, ref, "best chunks")
        assert sum(dc.route_read("launch").values()) >= 3
    finally:
        dc.set_option("max_workspace_mb", keep)


def _slot_stride(H, orders, max_in):
    """Bytes of one internal slot of the gathered route (r4x16_packed.hip: r4x16_packed_stride): the largest bound of the
    orders at the largest block, + 64, rounded up to 256."""
    return (max(H.rans_compress_bound_4x16(max_in, o) for o in orders) + 64 + 255) // 256 * 256


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["best", "stripe"])
def test_the_gathered_route_walks_its_own_chunks(H, routes, oracle, what):
    """The gathered route gives its slot arena at most a quarter of the ceiling (r4x16_packed.hip: gathered), so at 40 MiB
    at most 10 MiB / 410 KB = 25 of the 53 blocks share a round: three rounds of the packed call's own loop - offsets,
    sizes, statuses and winners written from a base, the running offset carried on, the slots reused."""
    dc, blocks = routes, inputs()
    ceiling_mb = 40
    methods = NINE if what == "best" else [0xc9]
    if what == "best":
        ref = B.reference_loop(oracle, "in", blocks, NINE)
        want = [c for c, _, _ in ref]
    else:
        want = [_stream(oracle, i, d, 0xc9) for i, d in enumerate(blocks)]
    p = _Packed(dc, blocks, _alloc_for(want))
    per_round = ((ceiling_mb << 20) // 4) // _slot_stride(H, methods, p.b.max_in)
    least_rounds = -(-len(blocks) // per_round)
    assert least_rounds >= 3, (per_round, least_rounds)
    run = (lambda: p.best(NINE)) if what == "best" else (lambda: p.compress(order=0xc9))
    check = (lambda w: _check_best(p, ref, w)) if what == "best" else (lambda w: _check_dense(p, want, w))
    run()
    check((what, "one chunk"))
    one = [x.copy() if isinstance(x, np.ndarray) else x for x in p.read()]
    keep = dc.get_option("max_workspace_mb")
    try:
        dc.set_option("max_workspace_mb", ceiling_mb)
        dc.route_read("launch")
        dc.route_read("result")
        p.fresh()
        run()
        check((what, "chunks"))
        assert sum(dc.route_read("launch").values()) >= least_rounds         # at least one chain launch per round
        assert dc.route_read("result")["gathered"] == len(blocks)
    finally:
        dc.set_option("max_workspace_mb", keep)
    got = p.read()
    assert np.array_equal(got[0], one[0]) and list(got[1:4]) == one[1:4]
    if what == "best":
        assert got[4] == one[4]


@pytest.mark.gpu
def test_the_slot_arena_grows_and_is_reused(H, oracle):
    """A fresh context, the dense route (its slots lie in the packed arena) over 3 blocks of 4 KiB, then 13, then 3 again:
    the first call allocates the arena, the second finds it too small and grows it - synchronize, free, allocate - and
    the third lays its slots out in an arena larger than it asked for."""
    import datagen
    dc = H.DeviceCodec(0)
    blocks = [datagen.tile(datagen.BASE_NAMES[j % len(datagen.BASE_NAMES)], 4096, j + 1).tobytes() for j in range(13)]
    want = [oracle.compress(b, 1) for b in blocks]
    for n in (3, 13, 3):
        p = _Packed(dc, blocks[:n], _alloc_for(want[:n]))
        p.compress(order=1)
        _check_dense(p, want[:n], ("regrow", n))


@pytest.mark.gpu
def test_two_streams_of_one_context_share_the_slot_arena_in_order(H, dc, oracle):
    import torch
    blocks = inputs()
    sets = [(blocks, 1), (blocks[::-1], 193)]
    wants = [[B._oracle_bytes(oracle, ("in", o < 2), i, d, o) for i, d in enumerate(bl)] for bl, o in sets]
    ps = [_Packed(dc, bl, _alloc_for(w)) for (bl, _), w in zip(sets, wants)]
    streams = [torch.cuda.Stream(device=dc.dev), torch.cuda.Stream(device=dc.dev)]
    torch.cuda.synchronize()
    for _ in range(2):
        for p, (_, o), s in zip(ps, sets, streams):
            with torch.cuda.stream(s):
                p.compress(order=o)
    for p, w, (_, o) in zip(ps, wants, sets):
        _check_dense(p, w, ("streams", o))


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["dense", "gathered", "best"])
def test_capacity_cuts_and_confinement(H, dc, oracle, route):
    blocks = inputs()
    if route == "best":
        ref = B.reference_loop(oracle, "in", blocks, NINE)
        want = [c for c, _, _ in ref]
    else:
        order = 1 if route == "dense" else 9
        want = [_stream(oracle, i, d, order) for i, d in enumerate(blocks)]
    need = _prefix([len(w) for w in want])
    k = len(blocks) // 2
    p = _Packed(dc, blocks, need[-1])
    for cap in (need[k] + len(want[k]) // 2, need[k + 1], 0):           # inside a block, exactly at a block's end, nothing
        p.fresh()
        if route == "best":
            p.best(NINE, capacity=cap)
            _check_best(p, ref, (route, cap), capacity=cap)
        else:
            p.compress(order=order, capacity=cap)
            _check_dense(p, want, (route, cap), capacity=cap)
        _, off, _, st, _ = p.read()
        assert off[-1] == need[-1]
        assert [s for s in st[:k]] == ([0] * k if cap else [1] * k) and all(s == 1 for s in st[k + 1:])
        assert st[k] == (0 if cap == need[k + 1] else 1)


# ---- peek ----------------------------------------------------------------------------------------------------
def _arena_of(dc, items):
    import torch
    sizes = [len(x) for x in items]
    off = np.cumsum([0] + sizes)[:-1].astype(np.int64)
    arena = np.frombuffer(b"".join(items) + bytes(64), dtype=np.uint8).copy()
    t = lambda a: torch.from_numpy(a).to(dc.dev)
    return t(arena), t(off), t(np.array(sizes, dtype=np.int32))


def _varint_len(v):
    n = 1
    while v >= 128:
        v >>= 7
        n += 1
    return n


@pytest.mark.gpu
def test_peek(H, dc, oracle):
    import torch
    blocks = inputs()
    items, expect = [], []          # (first byte | -1, raw size, status)
    for order in DEVICE_ORDERS + STRIPE_ORDERS:
        for i, d in enumerate(blocks):
            s = _stream(oracle, i, d, order)
            sized = bool(s[0] & 8) or not s[0] & 0x10
            items.append(s)
            expect.append((s[0], len(d) if sized else NONE, 0))
            if sized and i % 3 == 0:
                items.append(s[:1])
                expect.append((s[0], NONE, 2))
                if _varint_len(len(d)) >= 2:
                    items.append(s[:_varint_len(len(d))])       # the flag byte and all but the last byte of the varint
                    expect.append((s[0], NONE, 2))
    items.append(b"")
    expect.append((-1, NONE, 9))
    assert any(e[1] == NONE and e[2] == 0 for e in expect) and any(e[1] == 200000 for e in expect)
    d_in, d_off, d_size = _arena_of(dc, items)
    n = len(items)
    fmt, raw, st = (torch.full((n,), -5, dtype=torch.int32, device=dc.dev) for _ in range(3))
    dc.peek(d_in, d_off, d_size, fmt, raw, st, max(len(x) for x in items))
    torch.cuda.synchronize()
    got = list(zip(fmt.tolist(), [r & 0xFFFFFFFF for r in raw.tolist()], st.tolist()))
    bad = [(i, g, e) for i, (g, e) in enumerate(zip(got, expect)) if g != e]
    assert not bad, bad[:5]


# ---- packed decode -------------------------------------------------------------------------------------------
class _Unpacked:
    def __init__(self, dc, streams, alloc):
        import torch
        self.torch, self.dc, self.n = torch, dc, len(streams)
        self.d_in, self.d_in_off, self.d_in_size = _arena_of(dc, streams)
        self.max_in = max(len(s) for s in streams)
        self.alloc = alloc + GUARD
        self.pat = pattern(self.alloc)

    def run(self, max_out, nosz=None, capacity=None):
        torch, dev = self.torch, self.dc.dev
        self.d_out = torch.from_numpy(self.pat.copy()).to(dev)
        self.d_off = torch.full((self.n + 1,), -7, dtype=torch.int64, device=dev)
        self.d_osz = torch.full((self.n,), -3, dtype=torch.int32, device=dev)
        self.d_st = torch.full((self.n,), -3, dtype=torch.int32, device=dev)
        d_nosz = torch.tensor(nosz, dtype=torch.int32, device=dev) if nosz is not None else None
        self.dc.uncompress_packed(self.d_in, self.d_in_off, self.d_in_size, self.d_out, self.d_off, self.d_osz, self.d_st,
                                  self.max_in, max_out, nosz_size=d_nosz,
                                  out_capacity=self.alloc - GUARD if capacity is None else capacity)
        torch.cuda.synchronize()
        return self.d_out.cpu().numpy(), self.d_off.tolist(), self.d_osz.tolist(), self.d_st.tolist()


def _check_decoded(u, res, claims, expect, what, capacity=None):
    """claims[i]: bytes block i reserves; expect[i]: its bytes, or a status (int) / a set of statuses, or None (any failure)."""
    arena, off, osz, st = res
    need = _prefix(claims)
    assert off == need, (what, off[:6], need[:6])
    cap = u.alloc - GUARD if capacity is None else capacity
    mask = np.zeros(u.alloc, dtype=bool)
    for i, e in enumerate(expect):
        if isinstance(e, bytes) and need[i + 1] > cap:     # (an empty block behind the cut too: its range ends beyond it)
            e = 1
        if isinstance(e, bytes):
            assert st[i] == 0 and osz[i] == len(e), (what, i, st[i], osz[i])
            assert arena[need[i]:need[i + 1]].tobytes() == e, (what, i)
        else:
            assert osz[i] == 0 and st[i] != 0 and (e is None or st[i] == e), (what, i, st[i], osz[i], e)
            if e is None:
                mask[need[i]:need[i + 1]] = True              # failed while decoding: its own range is unspecified
        if isinstance(e, bytes):
            mask[need[i]:need[i + 1]] = True
    assert np.array_equal(arena[~mask], u.pat[~mask]), (what, "bytes outside the decoded blocks' ranges changed")


def _decode_set(oracle):
    blocks = inputs()
    orders = _mixed(DEVICE_ORDERS + STRIPE_ORDERS, len(blocks))
    assert set(orders) == set(DEVICE_ORDERS + STRIPE_ORDERS)
    streams = [_stream(oracle, i, d, o) for i, (d, o) in enumerate(zip(blocks, orders))]
    nosz = [bool(s) and not s[0] & 8 and bool(s[0] & 0x10) for s in streams]
    return blocks, streams, nosz


@pytest.fixture
def planes(dc):
    assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 7, 200000) == 0
    yield
    assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 0, 0) == 0


@pytest.mark.gpu
def test_packed_decode(H, dc, oracle, planes):
    blocks, streams, nosz = _decode_set(oracle)
    assert any(nosz) and any(s[0] & 8 for s in streams if s)
    sizes = [len(b) for b in blocks]
    u = _Unpacked(dc, streams, sum(sizes))
    # every block, the sizes of the X_NOSZ blocks given
    _check_decoded(u, u.run(200000, nosz=sizes), sizes, blocks, "all")
    arena, off, _, _ = u.run(200000, nosz=sizes)
    assert arena[:off[-1]].tobytes() == b"".join(blocks)
    # without them: SIZE and no bytes for those blocks
    claims = [0 if z else s for s, z in zip(sizes, nosz)]
    _check_decoded(u, u.run(200000), claims, [5 if z else b for b, z in zip(blocks, nosz)], "no nosz sizes")
    # blocks larger than max_out_size: UNSUPPORTED, no bytes, the others decode
    claims = [0 if s > 65536 else s for s in sizes]
    assert 0 < sum(s > 65536 for s in sizes) < len(sizes)
    _check_decoded(u, u.run(65536, nosz=sizes), claims, [6 if s > 65536 else b for b, s in zip(blocks, sizes)], "max_out_size")
    # capacity: inside a block, at a block's end, nothing
    need = _prefix(sizes)
    k = len(blocks) // 2
    assert sizes[k] > 1
    for cap in (need[k] + sizes[k] // 2, need[k + 1], 0):
        _check_decoded(u, u.run(200000, nosz=sizes, capacity=cap), sizes, blocks, ("capacity", cap), capacity=cap)


@pytest.mark.gpu
def test_packed_decode_of_hostile_and_damaged_blocks(H, dc, oracle, planes):
    blocks, streams, nosz = _decode_set(oracle)
    blocks, streams, sizes = list(blocks), list(streams), [len(b) for b in blocks]
    # a header that claims 0xFFFFFFF0 bytes
    at = 3
    streams.insert(at, bytes([0x00, 0x8f, 0xff, 0xff, 0xff, 0x70]) + bytes(40))
    blocks.insert(at, 6)
    sizes.insert(at, 0)
    # a valid header and table-less rest with every byte flipped: the reference refuses it (checked here), whatever the
    # decoder makes of it - it keeps the range its header claims
    j = next(i for i, (b, s) in enumerate(zip(blocks, streams)) if isinstance(b, bytes) and len(b) == 40000 and s[0] == 1)
    hdr = 1 + _varint_len(len(blocks[j]))
    streams[j] = streams[j][:hdr] + bytes(x ^ 0xff for x in streams[j][hdr:])
    assert oracle.uncompress(streams[j], capacity=len(blocks[j])) is None
    blocks[j] = None
    u = _Unpacked(dc, streams, sum(sizes))
    nz = [s for s in sizes]
    _check_decoded(u, u.run(200000, nosz=nz), sizes, blocks, "hostile")


@pytest.mark.gpu
def test_round_trip_without_the_host(H, dc, oracle):
    import torch
    blocks = inputs()
    orders = _mixed(DEVICE_ORDERS, len(blocks))
    want = [_stream(oracle, i, d, o) for i, (d, o) in enumerate(zip(blocks, orders))]
    p = _Packed(dc, blocks, _alloc_for(want))
    p.compress(orders=orders)
    total = sum(len(b) for b in blocks)
    pat = pattern(total + GUARD)
    d_back = torch.from_numpy(pat.copy()).to(dc.dev)
    d_off = torch.full((len(blocks) + 1,), -7, dtype=torch.int64, device=dc.dev)
    d_osz, d_st = (torch.full((len(blocks),), -3, dtype=torch.int32, device=dc.dev) for _ in range(2))
    # no host copy in between: the compressed arena, its offsets and sizes go straight in (the sizes of X_NOSZ blocks are
    # the input sizes the caller has on the device anyway)
    dc.uncompress_packed(p.d_out, p.d_off, p.d_osz, d_back, d_off, d_osz, d_st, int(p.alloc), p.b.max_in,
                         nosz_size=p.b.d_in_size, out_capacity=total)
    torch.cuda.synchronize()
    assert d_st.tolist() == [0] * len(blocks)
    assert d_off.tolist() == _prefix([len(b) for b in blocks])
    back = d_back.cpu().numpy()
    assert back[:total].tobytes() == b"".join(blocks)
    assert np.array_equal(back[total:], pat[total:])
