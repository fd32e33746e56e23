"""Device-resident "try k methods, keep the smallest" (rans4x16_hip_compress_best_dev) and X_STRIPE under per-block
orders (rans4x16_hip_set_dev_stripe_encode).  The expected bytes and the expected method always come from the oracle
run through the reference's caller loop (tokenise_name3.c:1246-1300): methods in order, a later one must be strictly
smaller, X_STRIPE methods skipped when the size is no multiple of four."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import datagen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = [0, 1, 128, 129, 64, 65, 192, 193, 201]
# the reference's five tables (tokenise_name3.c:1254-1260), one method alone, and two tables with other plane counts -
# the last holds two stripe methods of different N
TABLES = [[0, 128], [0, 200], [0, 128, 201], [0, 1, 129, 65, 193, 201], NINE, [1],
          [0, (2 << 8) | 9, (7 << 8) | 0xc9], [(3 << 8) | 8, 8]]
DEVICE_ORDERS = [0, 1, 16, 17, 32, 33, 64, 65, 128, 129, 192, 193, 0xd1]
STRIPE_ORDERS = [8, 9, 0x48, 0xc9, (2 << 8) | 9, (3 << 8) | 0xc9, (5 << 8) | 8, (7 << 8) | 8]


def _inputs():
    blocks = []
    for size in (24, 100, 1000, 4096, 40000, 65536, 200000):
        for name in datagen.BASE_NAMES:
            blocks.append(datagen.tile(name, size, 1).tobytes())
    for size in (4000, 40000):
        blocks += [datagen.rand(size).tobytes(), datagen.rand(size, nsym=16).tobytes(), datagen.runs(size)[:size].tobytes(),
                   datagen.markov(size)[:size].tobytes(), datagen.const(size).tobytes()]
    for size in (0, 1, 3, 4, 8, 20, 21, 22, 23):
        blocks.append(datagen.tile("q40+dir", size, 3).tobytes())
    rs = np.random.RandomState(5)
    for size in (4000, 40000):                     # little-endian uint32 columns: what the stripe methods are for
        blocks.append(rs.randint(0, 300, size // 4).astype("<u4").tobytes())
        blocks.append(rs.randint(0, 70000, size // 4).astype("<u4").tobytes())
        blocks.append((1000 + 3 * np.arange(size // 4)).astype("<u4").tobytes())
    return blocks


_INPUTS = None
_ORACLE_CACHE = {}


def inputs():
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = _inputs()
    return _INPUTS


def _oracle_bytes(oracle, tag, i, data, method):
    key = (tag, i, method)
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = oracle.compress(data, method)
    return _ORACLE_CACHE[key]


def reference_loop(oracle, tag, blocks, methods, caps=None):
    """[(bytes | None, method | -1, tie at the minimum)] of the reference's loop; a candidate whose bound exceeds the
    block's capacity is not there."""
    res = []
    for i, d in enumerate(blocks):
        best, best_m, sizes = None, -1, []
        for m in methods:
            if len(d) % 4 != 0 and (m & 8):
                continue
            if caps is not None and oracle.bound(len(d), m) > caps[i]:
                continue
            c = _oracle_bytes(oracle, tag, i, d, m)
            sizes.append(len(c))
            if best is None or len(c) < len(best):
                best, best_m = c, m
        res.append((best, best_m, len(sizes) > 1 and sizes.count(min(sizes)) > 1))
    return res


# ---- CPU half ------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    import htscodecs_amd
    from htscodecs_amd import lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("rans4x16_hip_compress_best_dev", "rans4x16_hip_set_dev_stripe_encode"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    from htscodecs_amd import codec
    assert hasattr(codec.DeviceCodec, "compress_best") and hasattr(codec.DeviceCodec, "set_stripe_encode")


def test_null_context_is_refused():
    import htscodecs_amd
    L = htscodecs_amd.load()
    meth = (C.c_int * 2)(0, 1)
    assert L.rans4x16_hip_compress_best_dev(None, 0, None, None, None, None, None, None, None, None, 2, meth, None, 0, 0, None) == -1
    assert L.rans4x16_hip_set_dev_stripe_encode(None, 4) == -1


def test_inputs_hold_what_they_claim(oracle):
    """The input set must exercise the choice: several methods win, the stripe method among them, and many blocks tie at
    the minimum (first wins).  Reference behaviour alone, no GPU."""
    blocks = inputs()
    res = reference_loop(oracle, "in", blocks, NINE)
    winners = {}
    for _, m, _ in res:
        winners[m] = winners.get(m, 0) + 1
    print("winners:", winners, "ties:", sum(t for _, _, t in res), "of", len(blocks))
    assert len(winners) >= 5 and 201 in winners, winners
    assert sum(t for _, _, t in res) >= 10
    for (c, m, _), d in zip(res, blocks):
        assert oracle.uncompress(c, capacity=len(d), out_size_hint=len(d)) == d


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


class _Batch:
    """Blocks in a device arena, with output slots of the given capacities."""

    def __init__(self, dc, blocks, caps):
        import torch
        self.torch, self.dc, self.blocks, self.n = torch, dc, blocks, len(blocks)
        sizes = [len(b) for b in blocks]
        self.max_in, self.total_in = max(sizes), sum(sizes)
        in_off = np.cumsum([0] + [(s + 255) // 256 * 256 + 256 for s in sizes])[:-1].astype(np.int64)
        arena = np.zeros(int(in_off[-1]) + sizes[-1] + 512, dtype=np.uint8)
        for b, off in zip(blocks, in_off):
            arena[off:off + len(b)] = np.frombuffer(b, dtype=np.uint8)
        self.out_off = np.cumsum([0] + [(int(c) + 255) // 256 * 256 + 256 for c in caps])[:-1].astype(np.int64)
        t = lambda a: torch.from_numpy(a).to(dc.dev)
        self.d_in, self.d_in_off, self.d_in_size = t(arena), t(in_off), t(np.array(sizes, dtype=np.int32))
        self.d_out_off, self.d_cap = t(self.out_off), t(np.array(caps, dtype=np.int32))
        self.out_bytes = int(self.out_off[-1]) + int(caps[-1]) + 512
        torch.cuda.synchronize()
        self.fresh()

    def fresh(self):
        torch, dev = self.torch, self.dc.dev
        self.d_out = torch.full((self.out_bytes,), 0xee, dtype=torch.uint8, device=dev)
        self.d_osz = torch.full((self.n,), -3, dtype=torch.int32, device=dev)
        self.d_st = torch.full((self.n,), -3, dtype=torch.int32, device=dev)
        self.d_chosen = torch.full((self.n,), -3, dtype=torch.int32, device=dev)

    def best(self, methods, total=True):
        self.dc.compress_best(self.d_in, self.d_in_off, self.d_in_size, self.d_out, self.d_out_off, self.d_cap, self.d_osz,
                              self.d_st, methods, self.max_in, chosen=self.d_chosen, total_in_size=self.total_in if total else 0)

    def orders(self, d_order):
        self.dc.compress(self.d_in, self.d_in_off, self.d_in_size, self.d_out, self.d_out_off, self.d_cap, self.d_osz,
                         self.d_st, 0, self.max_in, d_order=d_order)

    def read(self):
        self.torch.cuda.synchronize()
        st, osz, chosen, comp = (x.cpu().numpy() for x in (self.d_st, self.d_osz, self.d_chosen, self.d_out))
        got = [comp[self.out_off[i]:self.out_off[i] + max(int(osz[i]), 0)].tobytes() for i in range(self.n)]
        return got, chosen.tolist(), st.tolist(), osz.tolist()


def _check(batch, want, what):
    got, chosen, st, osz = batch.read()
    for i, (c, m, _) in enumerate(want):
        where = (what, i, len(batch.blocks[i]))
        if c is None:
            assert st[i] != 0 and osz[i] == 0 and chosen[i] == -1, (where, st[i], osz[i], chosen[i])
        else:
            assert st[i] == 0, (where, st[i])
            assert chosen[i] == m, (where, chosen[i], m)
            assert got[i] == c, where
    return got


def _full_caps(H, blocks, methods):
    return [max(H.rans_compress_bound_4x16(len(b), m) for m in methods) for b in blocks]


@pytest.mark.gpu
@pytest.mark.parametrize("methods", TABLES, ids=lambda m: "-".join(str(x) for x in m))
def test_best_of_k_keeps_what_the_reference_loop_keeps(H, dc, oracle, methods):
    blocks = inputs()
    batch = _Batch(dc, blocks, _full_caps(H, blocks, methods))
    batch.best(methods)
    want = reference_loop(oracle, "in", blocks, methods)
    got = _check(batch, want, methods)
    if all(m & 8 for m in methods):                # no candidate is tried on a size that is no multiple of four
        assert [i for i, w in enumerate(want) if w[0] is None] == [i for i, d in enumerate(blocks) if len(d) % 4]
        assert all(batch.read()[2][i] == 6 for i, d in enumerate(blocks) if len(d) % 4)
    else:
        assert all(w[0] is not None for w in want)
    for g, d, w in zip(got, blocks, want):         # every winner decodes back to its input
        if w[0] is not None:
            assert H.rans_uncompress_4x16(g, len(d)) == d


@pytest.mark.gpu
def test_failing_candidates_are_skipped_and_a_block_without_any_fails_alone(H, dc, oracle):
    blocks = inputs()
    caps = _full_caps(H, blocks, NINE)
    ref = reference_loop(oracle, "in", blocks, NINE)
    some = [i for i, (_, m, _) in enumerate(ref) if m == 201][0]          # the stripe method would win here ...
    caps[some] = H.rans_compress_bound_4x16(len(blocks[some]), 193)        # ... and is the one candidate that no longer fits
    none = [i for i, b in enumerate(blocks) if len(b) == 40000][0]
    caps[none] = H.rans_compress_bound_4x16(len(blocks[none]), 0) - 1      # below every bound
    assert min(oracle.bound(len(blocks[some]), m) for m in NINE) <= caps[some] < max(oracle.bound(len(blocks[some]), m) for m in NINE)
    want = reference_loop(oracle, "in", blocks, NINE, caps)
    assert want[some][1] not in (-1, 201) and want[none][0] is None
    batch = _Batch(dc, blocks, caps)
    batch.best(NINE)
    _check(batch, want, "capacity")
    assert batch.read()[2][none] == 1                                       # the first tried candidate's status: CAPACITY


def _candidate_bytes_per_block(H, methods, max_in):
    """The candidate slots one block takes in the arena (r4x16_best.hip: best_run): a bound-sized slot per plain method,
    N x K slots of the largest plane's bound per stripe method; every slot + 64, rounded up to 256."""
    slot = lambda size, order: (H.rans_compress_bound_4x16(size, order) + 64 + 255) // 256 * 256
    total = 0
    for m in methods:
        if m & 8:
            N = (m >> 8) or 4
            K = sum(1 for s in (1, 64, 128, 0) if (m & s) == s)
            total += N * K * slot(max((max_in + N - 1) // N, 20), 0xc1)
        else:
            total += slot(max_in, m)
    return total


@pytest.mark.gpu
def test_a_small_workspace_ceiling_walks_the_batch_in_chunks(H, dc, oracle):
    blocks = inputs()
    batch = _Batch(dc, blocks, _full_caps(H, blocks, NINE))
    ceiling_mb = 100
    # the candidate slots of a chunk alone must fit under the ceiling: that bounds the blocks per chunk of the outer walk
    per_block = _candidate_bytes_per_block(H, NINE, batch.max_in)
    per_chunk = max((ceiling_mb << 20) // per_block, 1)
    least_chunks = -(-len(blocks) // per_chunk)
    assert least_chunks >= 3, (per_block, per_chunk)
    keep = dc.get_option("max_workspace_mb")
    dc.set_option("route_count", 1)
    try:
        dc.set_option("max_workspace_mb", ceiling_mb)
        dc.route_read("launch")
        batch.best(NINE, total=False)
        _check(batch, reference_loop(oracle, "in", blocks, NINE), "chunks")
        launches = sum(dc.route_read("launch").values())                     # at least one chain launch per chunk
        assert launches >= least_chunks, (launches, least_chunks)
    finally:
        dc.set_option("max_workspace_mb", keep)
        dc.set_option("route_count", 0)
    batch.fresh()
    batch.best(NINE)
    _check(batch, reference_loop(oracle, "in", blocks, NINE), "one chunk again")


@pytest.mark.gpu
def test_bad_method_tables_are_refused(H, dc, oracle):
    """k outside 1..32, no table, and a stripe method with more than 255 planes make the call return -1 (the Python
    mirror raises), and nothing is enqueued; 255 planes and 32 methods are accepted."""
    blocks = [datagen.tile("q8", 1024, 1).tobytes(), b"abcd" * 8]
    batch = _Batch(dc, blocks, _full_caps(H, blocks, [193, (255 << 8) | 9]))
    for bad in ([], [0] * 33, [0, (256 << 8) | 8], [(1000 << 8) | 0xc9]):
        with pytest.raises(RuntimeError):
            batch.best(bad)
    L, h = H.load(), dc.ctx.h
    assert L.rans4x16_hip_compress_best_dev(h, 0, None, None, None, None, None, None, None, None, 1, None, None, 0, 0, None) == -1
    assert batch.read()[2] == [-3, -3]                                      # untouched
    batch.best([0] * 31 + [1])
    got, chosen, st, _ = batch.read()
    assert st == [0, 0] and all(c in (0, 1) for c in chosen)
    batch.fresh()
    batch.best([0, (255 << 8) | 9])
    _check(batch, reference_loop(oracle, "bad", blocks, [0, (255 << 8) | 9]), "255 planes")


@pytest.mark.gpu
def test_two_streams_of_one_context_share_the_arena_in_order(H, dc, oracle):
    import torch
    blocks = inputs()
    tables = (NINE, TABLES[6])
    batches = [_Batch(dc, blocks, _full_caps(H, blocks, m)) for m in tables]
    streams = [torch.cuda.Stream(device=dc.dev), torch.cuda.Stream(device=dc.dev)]
    torch.cuda.synchronize()
    for _ in range(2):
        for b, m, s in zip(batches, tables, streams):
            with torch.cuda.stream(s):
                b.best(m)
    for b, m in zip(batches, tables):
        _check(b, reference_loop(oracle, "in", blocks, m), ("streams", m))


def _order_blocks():
    names = ["q4", "q8", "q40+dir", "qvar"]
    rs = np.random.RandomState(89)
    blocks = [datagen.base_text("q4").tobytes(), datagen.base_text("q40+dir").tobytes(), b"", b"a", b"abcdefghij" * 2, b"x" * 21,
              datagen.tile("q8", 1000, 1).tobytes(), datagen.tile("qvar", 65537, 2).tobytes(), datagen.tile("q40+dir", 300003, 5).tobytes()]
    blocks += [datagen.tile(names[k % 4], int(rs.randint(22, 5000)), k).tobytes() for k in range(30)]
    every = STRIPE_ORDERS + DEVICE_ORDERS
    orders = [every[(5 * i) % len(every)] for i in range(len(blocks))]
    orders[2:6] = [8, 9, 0xc9, (7 << 8) | 8]                               # 0, 1, 20 and 21 bytes under stripe orders
    orders[8] = (3 << 8) | 0xc9
    assert set(orders) == set(every)
    return blocks, orders


@pytest.mark.gpu
def test_per_block_orders_with_stripe_blocks(H, dc, oracle):
    import torch
    blocks, orders = _order_blocks()
    want = [_oracle_bytes(oracle, "ord", i, b, o) for i, (b, o) in enumerate(zip(blocks, orders))]
    batch = _Batch(dc, blocks, [H.rans_compress_bound_4x16(len(b), o) for b, o in zip(blocks, orders)])
    d_order = torch.tensor(orders, dtype=torch.int32, device=dc.dev)
    planes = lambda o: (o >> 8) or 4
    try:
        for max_planes in (7, 2, 0):
            dc.set_stripe_encode(max_planes)
            batch.fresh()
            batch.orders(d_order)
            got, _, st, osz = batch.read()
            for i, (b, o) in enumerate(zip(blocks, orders)):
                refused = (o & 8) and len(b) > 20 and planes(o) > max_planes
                if refused:
                    assert st[i] == 6 and osz[i] == 0, (max_planes, i, o, st[i], osz[i])
                else:
                    assert st[i] == 0, (max_planes, i, o, st[i])
                    assert got[i] == want[i], (max_planes, i, o, len(b))
        # one `order` for all blocks is not affected by the setting: the stripe route of the uniform call, whose own
        # internal items carry per-item orders, with the setting on
        dc.set_stripe_encode(7)
        for order in (8, 0xc9, (3 << 8) | 0xc9):
            ubatch = _Batch(dc, blocks, [H.rans_compress_bound_4x16(len(b), order) for b in blocks])
            dc.compress(ubatch.d_in, ubatch.d_in_off, ubatch.d_in_size, ubatch.d_out, ubatch.d_out_off, ubatch.d_cap,
                        ubatch.d_osz, ubatch.d_st, order, ubatch.max_in)
            got, _, st, _ = ubatch.read()
            for i, b in enumerate(blocks):
                assert st[i] == 0, (order, i, st[i])
                assert got[i] == _oracle_bytes(oracle, "ord", i, b, order), (order, i, len(b))
    finally:
        dc.set_stripe_encode(0)
    with pytest.raises(ValueError):
        dc.set_stripe_encode(256)
