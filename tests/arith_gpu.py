"""What the GPU tests of arith_dynamic decoding share (test_gpu_arith.py, test_gpu_arith_hostile.py,
test_gpu_arith_trips.py): one run of
rans4x16_hip_arith_uncompress_dev over a list of streams with the confinement pattern of test_gpu_confinement.py - the
output slots a few bytes apart at every alignment in an arena filled with a pattern, every byte outside them compared
afterwards - and the route the model expects."""
import collections

import numpy as np

import arith_model as M
from test_gpu_confinement import Layout

KINDS = ("o0", "o1_lds", "o1_global", "rle")


def expect(streams, caps, planes=0, stripe_out=0):
    """[(status, bytes)] of the model, and the route count: entropy-coded pieces of the accepted blocks"""
    res, route = [], collections.Counter({k: 0 for k in KINDS})
    for s, cap in zip(streams, caps):
        t = []
        res.append(M.uncompress_to(s, cap, max_planes=planes, max_stripe_out=stripe_out, trace=t))
        route.update(t)
    return res, dict(route)


def run_dev(dc, streams, caps, planes=0, stripe_out=0, stream=None, total=0, max_in=None, max_out=None, in_off=None):
    """-> ([bytes or None], statuses, route).  Asserts that nothing outside the slots was written.  max_in / max_out /
    total: what the call announces (default: the largest stream, the largest capacity, n x the largest capacity).
    in_off: where each stream lies in the input arena, whose start is 256-byte aligned (default: a few bytes apart,
    from byte 3)."""
    import torch
    t = dc.torch if hasattr(dc, "torch") else torch
    n = len(streams)
    lay = Layout(caps, what=[s[:8].hex() for s in streams])
    if in_off is None:
        in_off, pos = [], 3
        for i, s in enumerate(streams):
            in_off.append(pos)
            pos += len(s) + 1 + i % 7
    else:
        spans = sorted((o, o + len(s)) for o, s in zip(in_off, streams))
        assert len(in_off) == n and spans[0][0] >= 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        pos = spans[-1][1]
    arena_in = np.zeros(pos + 64, dtype=np.uint8)
    for o, s in zip(in_off, streams):
        arena_in[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    dev = dc.dev
    up = lambda a: t.from_numpy(a).to(dev)
    d_in, d_out = up(arena_in), up(lay.pattern.copy())
    assert d_in.data_ptr() % 256 == 0
    d_ioff, d_ooff = up(np.array(in_off, dtype=np.int64)), up(lay.offs.copy())
    d_isz = up(np.array([len(s) for s in streams], dtype=np.int32))
    d_cap = up(np.array(caps, dtype=np.int64).astype(np.uint32).view(np.int32))
    d_osz = t.full((n,), -7, dtype=t.int32, device=dev)
    d_st = t.full((n,), -7, dtype=t.int32, device=dev)
    assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, planes, stripe_out) == 0
    dc.set_option("route_count", 1)
    try:
        dc.route_read("arith")
        args = (d_in, d_ioff, d_isz, d_out, d_ooff, d_cap, d_osz, d_st, max_in or max([len(s) for s in streams] + [1]),
                max_out or max(list(caps) + [1]), total)
        if stream is None:
            dc.arith_uncompress(*args)
        else:
            stream.wait_stream(t.cuda.current_stream(dev))
            with t.cuda.stream(stream):
                dc.arith_uncompress(*args)
            stream.synchronize()
        t.cuda.synchronize(dev)
        route = dc.route_read("arith")
    finally:
        dc.set_option("route_count", 0)
        assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 0, 0) == 0
    arena = d_out.cpu().numpy()
    stray = lay.stray_writes(arena)
    assert stray is None, stray
    st, osz = d_st.tolist(), d_osz.tolist()
    outs = [b if s == 0 else None for b, s in zip(lay.take(arena, [max(z, 0) for z in osz]), st)]
    for i in range(n):
        assert st[i] >= 0 and (osz[i] == 0 if st[i] else 0 <= osz[i] <= caps[i]), (i, st[i], osz[i])
    return outs, st, route


def check(dc, streams, caps, planes=0, stripe_out=0, want=None, **kw):
    """run_dev against the model: statuses, bytes (`want`: the raw inputs, where the blocks must all decode to them) and
    route"""
    res, route = expect(streams, caps, planes, stripe_out)
    outs, st, got_route = run_dev(dc, streams, caps, planes, stripe_out, **kw)
    for i, ((wst, wout), out) in enumerate(zip(res, outs)):
        assert st[i] == wst, (i, st[i], wst, streams[i][:12].hex(), caps[i])
        if wst == 0:
            assert out == wout, (i, "bytes differ", streams[i][:12].hex(), len(wout))
            if want is not None:
                assert wout == want[i], (i, "the model does not give the raw input")
    if want is not None:
        assert all(s == 0 for s in st)
    assert got_route == route, (got_route, route)
    return outs, st, got_route
