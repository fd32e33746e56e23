"""The host-buffer batch calls of the adaptive coders (rans4x16_hip_arith_uncompress_batch, _arith_compress_batch,
_fqz_uncompress_batch) on mixed batches: blocks the host walk refuses beside blocks it takes, blocks the device refuses,
empty blocks, stripe blocks, and batches of which nothing is taken.

For every block: status, size, bytes (record count and lengths for fqzcomp_qual), that a refused block's buffers are
byte for byte what they were before the call, and the call's return value - the count of blocks that failed.  A batch
of which nothing is taken must not reach the device: no launch is counted.

Expected answers are the reference's own streams and inputs of tests/golden/arith/edge.bin and
tests/golden/fqzcomp/edge.bin, and the Python models (arith_model.py, arith_enc_model.py, fqz_model.py) that the CPU
tests pin to them.  The calls are made through the library handle: codec.py's wrappers give neither the return value nor
the buffers back."""
import ctypes as C

import numpy as np
import pytest

import arith_cases as K
import arith_enc_model as E
import arith_model as M
import fqz_model as F

pytestmark = pytest.mark.gpu
FILL = 0xA5
LEN_FILL = -77


@pytest.fixture(scope="module")
def ctx():
    from htscodecs_amd import codec
    return codec._thread_ctx()


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data if a is not None else None for a in arrays])


def _launches(ctx, call):
    """call() with the route read-out on -> (its return value, the chunks of device calls it made)"""
    ctx.set_option("route_count", 1)
    try:
        ctx.route_read("launch")
        rc = call()
        launch = ctx.route_read("launch")
    finally:
        ctx.set_option("route_count", 0)
    assert rc >= 0, ctx.error()
    return rc, launch["in_order"] + launch["side_by_side"]


def _batch(ctx, name, blocks, caps, orders=None, lengths=None, nlengths=None, want_nrec=False):
    """One call of rans4x16_hip_<name>_batch -> (return value, launches, statuses, sizes, output buffers, lengths buffers,
    record counts).  Output buffers hold FILL beforehand and one byte more than their capacity; lengths: None, or per
    block None or the entries of the caller's array (LEN_FILL beforehand), of which nlengths are announced."""
    n = len(blocks)
    srcs = [np.frombuffer(bytes(b) or b"\0", dtype=np.uint8).copy() for b in blocks]
    outs = [np.full(int(c) + 1, FILL, dtype=np.uint8) for c in caps]
    in_sz = (C.c_uint * n)(*[len(b) for b in blocks])
    out_sz = (C.c_uint * n)(*[int(c) for c in caps])
    status = (C.c_int * n)(*([-7] * n))
    args = [ctx.h, n, _ptrs(srcs), in_sz, _ptrs(outs), out_sz]
    lens, nrec = None, None
    if orders is not None:
        args.append((C.c_int * n)(*[int(o) for o in orders]))
    args.append(status)
    if name == "fqz_uncompress":
        lens = None if lengths is None else [None if v is None else np.full(v, LEN_FILL, dtype=np.int32) for v in lengths]
        nrec = (C.c_uint * n)(*([77] * n)) if want_nrec else None
        args += [None if lens is None else _ptrs(lens), None if nlengths is None else (C.c_int * n)(*nlengths), nrec]
    fn = getattr(ctx.L, "rans4x16_hip_%s_batch" % name)
    rc, launches = _launches(ctx, lambda: fn(*args))
    return rc, launches, list(status), list(out_sz), outs, lens, None if nrec is None else list(nrec)


def _check_outputs(want, st, osz, outs):
    """want: [(status, bytes)].  A block that failed has size 0 and an untouched buffer; one that did not, its bytes and
    nothing behind them"""
    for i, (wst, wout) in enumerate(want):
        assert st[i] == wst, (i, st[i], wst)
        if wst:
            assert osz[i] == 0 and (outs[i] == FILL).all(), (i, "a refused block's buffer was written")
        else:
            assert osz[i] == len(wout) and outs[i][:osz[i]].tobytes() == wout, (i, "bytes differ")
            assert (outs[i][osz[i]:] == FILL).all(), (i, "bytes behind the result were written")


def _arith_edge(what, order, size):
    (hit,) = [c for c in K.edge()[0] if c[0] == what and c[1] == order and len(c[2]) == size]
    return hit[2], hit[3]                                            # (data, the reference's stream)


# ---- arith_dynamic decode -------------------------------------------------------------------------------------------
def _arith_dec_cases():
    a_raw, a = _arith_edge("m=5", 0x41, 91)
    b_raw, b = _arith_edge("run 29", 0x41, 34)
    c_raw, c = _arith_edge("m=63", 0x1, 91)
    _, empty = _arith_edge("q8[:0]", 0x0, 0)
    s_raw, stripe = _arith_edge("stripe N=4", 0x409, 130)
    _, packed = _arith_edge("pack 3", 0x80, 64)
    cut = packed[:4]                                                 # ends inside the pack map
    assert stripe[0] & M.X_STRIPE and M.uncompress_to(cut, 64)[0] == M.E_TRUNCATED
    return dict(a=(a, a_raw), b=(b, b_raw), c=(c, c_raw), empty=empty, stripe=(stripe, s_raw), cut=cut)


def test_arith_decode_a_mixed_batch(ctx):
    k = _arith_dec_cases()
    blocks = [k["a"][0], k["cut"], k["b"][0], k["c"][0], k["empty"], k["stripe"][0]]
    caps = [len(k["a"][1]) + 5, 64, len(k["b"][1]), len(k["c"][1]) - 1, 0, len(k["stripe"][1])]
    want = [M.uncompress_to(s, cap) for s, cap in zip(blocks, caps)]
    assert [w[0] for w in want] == [0, M.E_TRUNCATED, 0, M.E_CAPACITY, 0, 0]
    assert [w[1] for w in want] == [k["a"][1], b"", k["b"][1], b"", b"", k["stripe"][1]]
    rc, launches, st, osz, outs, _, _ = _batch(ctx, "arith_uncompress", blocks, caps)
    _check_outputs(want, st, osz, outs)
    assert rc == 2 and launches == 1


def test_arith_decode_a_batch_of_which_every_stream_is_refused(ctx):
    k = _arith_dec_cases()
    blocks = [b"", k["cut"], k["c"][0]]
    caps = [10, 64, len(k["c"][1]) - 1]
    want = [M.uncompress_to(s, cap) for s, cap in zip(blocks, caps)]
    assert [w[0] for w in want] == [M.E_EMPTY, M.E_TRUNCATED, M.E_CAPACITY]
    rc, launches, st, osz, outs, _, _ = _batch(ctx, "arith_uncompress", blocks, caps)
    _check_outputs(want, st, osz, outs)
    assert rc == 3 and launches == 0


# ---- arith_dynamic encode -------------------------------------------------------------------------------------------
def _cap(data, order):
    from htscodecs_amd import codec
    return codec.arith_compress_cap(len(data), order)


def _enc_want(datas, orders, caps):
    want = []
    for d, o, cap in zip(datas, orders, caps):
        st = E.refused(len(d), o)
        if st == 0 and cap < _cap(d, o):
            st = M.E_CAPACITY
        want.append((st, b"" if st else E.compress(d, o)))
    return want


def test_arith_encode_a_mixed_batch(ctx):
    good, good_s = _arith_edge("m=5", 0x41, 91)
    other, _ = _arith_edge("m=63", 0x1, 91)
    striped, striped_s = _arith_edge("stripe N=4", 0x409, 130)
    datas = [good, b"", other, other, striped]
    orders = [0x41, 0, 1, 1 | M.X_EXT, 0x409]
    caps = [_cap(good, 0x41) + 3, _cap(b"", 0), _cap(other, 1) - 1, _cap(other, 1) + 40, _cap(striped, 0x409)]
    want = _enc_want(datas, orders, caps)
    assert [w[0] for w in want] == [0, 0, M.E_CAPACITY, M.E_UNSUPPORTED, 0]
    assert want[0][1] == good_s and want[4][1] == striped_s and want[1][1] == M.compress(b"", 0)      # the reference's streams
    rc, launches, st, osz, outs, _, _ = _batch(ctx, "arith_compress", datas, caps, orders=orders)
    _check_outputs(want, st, osz, outs)
    assert rc == 2 and launches == 1


def test_arith_encode_a_batch_of_empty_blocks_goes_to_the_device(ctx):
    datas, orders = [b"", b"", b""], [0, 0x41, 0xc1]
    caps = [_cap(d, o) for d, o in zip(datas, orders)]
    want = _enc_want(datas, orders, caps)
    assert all(w[0] == 0 and len(w[1]) >= 1 for w in want)
    rc, launches, st, osz, outs, _, _ = _batch(ctx, "arith_compress", datas, caps, orders=orders)
    _check_outputs(want, st, osz, outs)
    assert rc == 0 and launches == 1


def test_arith_encode_a_batch_of_which_every_block_is_refused(ctx):
    other, _ = _arith_edge("m=63", 0x1, 91)
    datas, orders = [other, other, b"", other], [M.X_EXT, 0x41, M.X_EXT | 1, 8 | (256 << 8)]
    caps = [_cap(other, 0) + 9, _cap(other, 0x41) - 1, 50, 4000]
    want = _enc_want(datas, orders, caps)
    assert [w[0] for w in want] == [M.E_UNSUPPORTED, M.E_CAPACITY, M.E_UNSUPPORTED, M.E_UNSUPPORTED]
    rc, launches, st, osz, outs, _, _ = _batch(ctx, "arith_compress", datas, caps, orders=orders)
    _check_outputs(want, st, osz, outs)
    assert rc == 4 and launches == 0


# ---- fqzcomp_qual decode --------------------------------------------------------------------------------------------
def _fqz_answers(blocks, caps):
    """[(status, bytes, lengths)] of the model under these capacities"""
    return [F.decompress(s, cap=cap) for s, cap in zip(blocks, caps)]


def _check_lengths(want, st, lens, room, announced, nrec):
    for i, (wst, _, wlens) in enumerate(want):
        assert nrec[i] == (0 if wst else len(wlens)), (i, nrec[i])
        if lens is None or lens[i] is None:
            continue
        k = 0 if wst else min(len(wlens), announced[i])
        assert lens[i][:k].tolist() == wlens[:k], (i, "lengths differ")
        assert (lens[i][k:] == LEN_FILL).all(), (i, "entries behind the last record or the announced count were written")


def test_fqz_decode_a_mixed_batch(ctx):
    by_name = {i[0]: i for i in F.edge()[0]}
    names = ("nparam2", "rev", "dup_chain", "starts", "sloc15", "do_len_both")
    good = [by_name[k][4] for k in names]
    nrecs = [len(by_name[k][2]) for k in names]
    assert nrecs == [12, 9, 9, 40, 8, 5] and all(len(s) <= 400 for s in good)
    short = [s for s, site in F.model_refused() if site == "short"][0]
    damaged = [s for s, ans in F.edge()[1] if ans is None and len(s) <= 400 and F.parse(s)[0] == 0][0]
    blocks = good[:3] + [short] + good[3:5] + [damaged] + good[5:]
    sizes = [F.parse(s)[1].out_size if F.parse(s)[0] == 0 else 30 for s in blocks]
    caps = [n + (i % 3) for i, n in enumerate(sizes)]
    want = _fqz_answers(blocks, caps)
    assert [w[0] != 0 for w in want] == [False, False, False, True, False, False, True, False]
    assert want[3][0] == F.parse(short)[0] and F.parse(damaged)[0] == 0              # the host walk refuses one, the device the other
    for k, name in zip((0, 1, 2, 4, 5, 7), names):                                   # the reference's own inputs and lengths
        data, ref_lens = by_name[name][1], by_name[name][2]
        assert want[k][2] == ref_lens and (data is None or want[k][1] == data), name
    #          exact  none  fewer  refused  more  none announced  refused  no array
    room = [12, None, 9, 6, 45, 8, 20, None]
    announced = [12, 0, 4, 6, 45, 0, 20, 3]
    rc, launches, st, osz, outs, lens, nrec = _batch(ctx, "fqz_uncompress", blocks, caps, lengths=room, nlengths=announced,
                                                      want_nrec=True)
    _check_outputs([w[:2] for w in want], st, osz, outs)
    _check_lengths(want, st, lens, room, announced, nrec)
    assert rc == 2 and launches == 1
    # without any lengths and without record counts: the same bytes
    rc, launches, st, osz, outs, _, _ = _batch(ctx, "fqz_uncompress", blocks, caps)
    _check_outputs([w[:2] for w in want], st, osz, outs)
    assert rc == 2 and launches == 1


def test_fqz_decode_a_batch_of_which_every_stream_is_refused(ctx):
    by_name = {i[0]: i for i in F.edge()[0]}
    refused = [s for s, _ in F.model_refused()][:4]
    blocks = refused + [by_name["rev"][4]]
    caps = [30] * 4 + [by_name["rev"][5] - 1]
    want = _fqz_answers(blocks, caps)
    assert all(w[0] != 0 for w in want) and want[4][0] == F.E_CAPACITY
    rc, launches, st, osz, outs, lens, nrec = _batch(ctx, "fqz_uncompress", blocks, caps, lengths=[4] * 5, nlengths=[4] * 5,
                                                      want_nrec=True)
    _check_outputs([w[:2] for w in want], st, osz, outs)
    _check_lengths(want, st, lens, [4] * 5, [4] * 5, nrec)
    assert rc == 5 and launches == 0
