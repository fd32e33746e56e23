"""The staging arena of the host-buffer calls (htscodecs_amd/csrc/r4x16_stage.h, r4x16_stage_begin / r4x16_stage_verdicts in
r4x16_host.hip) at the shapes where a slip in its layout would show: item counts around 32, where the per-item arrays of
eight bytes cross a 256-byte step; block sizes around the 256-byte slot step, the empty block among them; one and
several slots per block; with planes, with an order array, with gather descriptors.  Every call site of the layout is
driven - the single pass, the pipeline, the rANS 4x8 pair, both stripe routes, best-of-k and the arith batch - and
every output buffer ends in a canary that must come back untouched.  tests/host/stage_check.cpp checks the layout's
own arithmetic on the CPU; here the kernels and the copies run over it."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

COUNTS = (1, 31, 32, 33)
SIZES = (0, 1, 255, 256, 257, 4096)
CANARY = 64
STRIPE = 8                                   # X_STRIPE of the order byte; the plane count rides in order >> 8 (0: four)


@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


@pytest.fixture(scope="module")
def orc8():
    import cpu_libs
    from test_oracle4x8 import Codec8
    return Codec8(cpu_libs.oracle().lib, "orc8_")


@functools.lru_cache(maxsize=None)
def _blocks(count):
    """`count` blocks whose sizes walk SIZES from a start that differs per count, and an order 0 / 1 for each"""
    rs = np.random.RandomState(1000 + count)
    sizes = [SIZES[(i + count) % len(SIZES)] for i in range(count)]
    blocks = tuple(datagen.tile("q40+dir", s, i).tobytes() if s else b"" for i, s in enumerate(sizes))
    return blocks, tuple(int(o) for o in rs.randint(0, 2, size=count))


def _call(H, name, blocks, caps, *extra):
    """One host-buffer batch call of the library on the calling thread's context: blocks in, buffers of caps[i] bytes with
    a canary behind each out.  extra: the arguments between out_size and status.  -> ([bytes or None], statuses, rc)"""
    from htscodecs_amd import codec
    ctx = codec._thread_ctx()
    n = len(blocks)
    srcs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in blocks]
    outs = [np.full(int(c) + CANARY, 0xA5, dtype=np.uint8) for c in caps]
    dummy = np.zeros(1, dtype=np.uint8)
    in_p = (C.c_void_p * n)(*[(s.ctypes.data if len(s) else dummy.ctypes.data) for s in srcs])
    out_p = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    in_sz = (C.c_uint * n)(*[len(s) for s in srcs])
    out_sz = (C.c_uint * n)(*[int(c) for c in caps])
    status = (C.c_int * n)()
    rc = getattr(ctx.L, name)(ctx.h, n, in_p, in_sz, out_p, out_sz, *extra, status)
    assert rc >= 0, ctx.error()
    for i, (o, c) in enumerate(zip(outs, caps)):
        assert (o[int(c):] == 0xA5).all(), (name, i, "the canary behind the buffer was written")
        assert out_sz[i] <= c, (name, i, out_sz[i], c)
    return [outs[i][:out_sz[i]].tobytes() if status[i] == 0 else None for i in range(n)], list(status), rc


def _ints(v):
    return (C.c_int * len(v))(*v)


def _both_ways(H, oracle, blocks, orders):
    L = H.load()
    want = [oracle.compress(b, o) for b, o in zip(blocks, orders)]
    enc, st, _ = _call(H, "rans4x16_hip_compress_batch", blocks, [L.rans_compress_bound_4x16(len(b), o) for b, o in zip(blocks, orders)],
                       _ints(orders))
    assert st == [0] * len(blocks), st
    bad = [(i, len(b), o) for i, (b, o, e, w) in enumerate(zip(blocks, orders, enc, want)) if e != w]
    assert not bad, bad
    dec, st, _ = _call(H, "rans4x16_hip_uncompress_batch", want, [len(b) for b in blocks])
    assert st == [0] * len(blocks), st
    bad = [(i, len(b), o) for i, (b, o, d) in enumerate(zip(blocks, orders, dec)) if d != b]
    assert not bad, bad


@pytest.mark.parametrize("pipe_mb", [0, 1])
@pytest.mark.parametrize("count", COUNTS)
def test_rans4x16_batches_single_pass_and_pipelined(H, oracle, opts, count, pipe_mb):
    """host_pipe_mb 0: the single pass.  1: the pipeline (one slot per block) for batches of 32 blocks and more, and for
    those whose input and capacities come to 1 MiB - the 31-block encode with its bound-sized slots; the others stay."""
    opts.set("host_pipe_mb", pipe_mb)
    blocks, orders = _blocks(count)
    _both_ways(H, oracle, blocks, orders)


@pytest.mark.parametrize("count", COUNTS)
def test_rans4x8_batches(H, orc8, count):
    """The same grid through the 4x8 pair.  The empty block is refused both ways (the reference's encoder divides by its
    size, its decoder wants nine bytes of header: rANS_static.c:937) and keeps its place in the batch."""
    blocks, orders = _blocks(count)
    L = H.load()
    want = [orc8.compress(b, o) if b else None for b, o in zip(blocks, orders)]
    enc, st, rc = _call(H, "rans4x8_hip_compress_batch", blocks, [L.rans4x8_hip_compress_bound(len(b)) for b in blocks], _ints(orders))
    assert [s == 0 for s in st] == [bool(b) for b in blocks], st
    assert rc == sum(1 for b in blocks if not b)
    assert enc == want
    dec, st, rc = _call(H, "rans4x8_hip_uncompress_batch", [w or b"" for w in want], [len(b) for b in blocks])
    assert [s == 0 for s in st] == [bool(b) for b in blocks], st
    assert dec == [b if b else None for b in blocks]


@pytest.mark.parametrize("stripe_dev", [1, 0])
def test_stripe_and_plain_blocks_in_one_batch(H, oracle, opts, stripe_dev):
    """33 blocks: plain ones of the grid's sizes between X_STRIPE blocks of four and of three planes, 24 and 4,096 bytes,
    through the device-resident stripe route (1) and the host-orchestrated one (0)."""
    opts.set("host_stripe_dev", stripe_dev)
    opts.set("host_pipe_mb", 0)
    plain, porders = _blocks(33)
    blocks, orders = [], []
    striped = [(24, STRIPE), (4096, STRIPE | 1), (24, (3 << 8) | STRIPE | 1), (4096, (3 << 8) | STRIPE)]
    for i in range(33):
        if i % 3 == 1:
            size, order = striped[(i // 3) % 4]
            blocks.append(datagen.tile("q4", size, i).tobytes())
            orders.append(order)
        else:
            blocks.append(plain[i])
            orders.append(porders[i])
    assert sum(1 for o in orders if o & STRIPE) == 11
    _both_ways(H, oracle, blocks, orders)


def test_best_of_three_with_a_stripe_method(H, oracle):
    """rans4x16_hip_compress_best_batch: two plain methods share a block's input and own a slot each (K = 2 slots per
    block in the pipeline's arena), the stripe method goes through the stripe route; the smallest wins, the first on ties,
    and blocks whose size is no multiple of four skip the stripe method (tokenise_name3.c:1246-1300)."""
    methods = [0, 1, STRIPE | 1]
    blocks, _ = _blocks(33)
    L = H.load()
    chosen = (C.c_int * len(blocks))()
    got, st, _ = _call(H, "rans4x16_hip_compress_best_batch", blocks,
                       [max(L.rans_compress_bound_4x16(len(b), m) for m in methods) for b in blocks], len(methods), _ints(methods), chosen)
    assert st == [0] * len(blocks), st
    for i, b in enumerate(blocks):
        best, best_m = None, None
        for m in methods:
            if len(b) % 4 != 0 and (m & STRIPE):
                continue
            c = oracle.compress(b, m)
            if best is None or len(c) < len(best):
                best, best_m = c, m
        assert (chosen[i], got[i]) == (best_m, best), (i, len(b), chosen[i], best_m)


def test_arith_batch_with_a_refused_block_between(H):
    """rans4x16_hip_arith_uncompress_batch: three of the committed streams and, between them, a stripe stream cut in half,
    which the host walk refuses before anything is uploaded - it takes no bytes of the arena, the offsets of the blocks
    behind it do not advance for it."""
    import arith_model as M
    def stream(name):
        with open(os.path.join(datagen.GOLDEN, "arith", name), "rb") as f:
            return f.read()
    names = ["q4.1", "q4.9", "q4.65", "q4.8"]
    streams = [stream(n) for n in names]
    streams[1] = streams[1][:len(streams[1]) // 2]
    raw = M.text("q4")
    caps = [len(raw)] * 4
    wst, _ = M.uncompress_to(streams[1], caps[1])
    assert wst == M.E_TRUNCATED
    outs, st, rc = _call(H, "rans4x16_hip_arith_uncompress_batch", streams, caps)
    assert st == [0, wst, 0, 0] and rc == 1
    assert outs == [raw, None, raw, raw]
