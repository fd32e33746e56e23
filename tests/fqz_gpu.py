"""What the GPU tests of fqzcomp_qual decoding share (test_gpu_fqz.py, test_gpu_fqz_records.py): one run of rans4x16_hip_fqz_uncompress_dev over a
list of streams with the confinement pattern of test_gpu_confinement.py - the output slots a few bytes apart at every
alignment in an arena filled with a pattern, every byte outside them compared afterwards; the lengths slots a few
entries apart in an arena of their own, every entry the call may not write compared - and the answers and the route of
the Python model (fqz_model.py), computed once per stream."""
import collections

import numpy as np

import fqz_model as M
from test_gpu_confinement import Layout

KINDS = M.KINDS
LEN_FILL = 0x5a5a0000

_answers = {}


def answer(stream):
    """(status, bytes, lengths, route) of the model, computed once"""
    if stream not in _answers:
        route = collections.Counter()
        st, out, lens = M.decompress(stream, route=route)
        _answers[stream] = (st, out, lens, dict(route))
    return _answers[stream]


def expect(streams, caps):
    """[(status, bytes, lengths)] of the model under these capacities, and the route count of the accepted streams"""
    res, route = [], collections.Counter({k: 0 for k in KINDS})
    for s, cap in zip(streams, caps):
        st, out, lens, r = answer(s)
        pst, h = M.parse(s)
        if pst == 0 and cap < h.out_size:                            # the walk's last test, before a symbol is decoded
            st, out, lens, r = M.E_CAPACITY, b"", [], {}
        if st == 0 and len(out) == 0:
            r = {}                                                   # nothing is decoded: no wave takes the stream
        res.append((st, out, lens))
        route.update(r)
    return res, dict(route)


def run_dev(dc, streams, caps, len_caps=None, total=0, max_in=None, max_out=None, want_chunks=None):
    """-> ([bytes or None], statuses, [lengths], nrec, route).  Asserts that nothing outside the slots was written, in the
    output arena and in the lengths arena (inside a lengths slot: nothing behind entry min(nrec, cap)).  len_caps: entries
    of each lengths slot (default: none are asked for).  want_chunks: the chunks the call must walk in."""
    import torch as t
    n = len(streams)
    lay = Layout(caps, what=[s[:8].hex() for s in streams])
    in_off, pos = [], 3
    for i, s in enumerate(streams):
        in_off.append(pos)
        pos += len(s) + 1 + i % 7
    arena_in = np.zeros(pos + 64, dtype=np.uint8)
    for o, s in zip(in_off, streams):
        arena_in[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    dev = dc.dev
    up = lambda a: t.from_numpy(a).to(dev)
    d_in, d_out = up(arena_in), up(lay.pattern.copy())
    d_ioff, d_ooff = up(np.array(in_off, dtype=np.int64)), up(lay.offs.copy())
    d_isz = up(np.array([len(s) for s in streams], dtype=np.int32))
    d_cap = up(np.array(caps, dtype=np.int64).astype(np.uint32).view(np.int32))
    d_osz = t.full((n,), -7, dtype=t.int32, device=dev)
    d_st = t.full((n,), -7, dtype=t.int32, device=dev)
    d_nrec = t.full((n,), -7, dtype=t.int32, device=dev)
    kw = {}
    if len_caps is not None:
        len_off, at = [], 5
        for i, c in enumerate(len_caps):
            len_off.append(at)
            at += c + 1 + i % 3
        len_fill = (LEN_FILL + np.arange(at + 8)).astype(np.int32)
        kw = dict(d_len=up(len_fill.copy()), len_off=up(np.array(len_off, dtype=np.int64)), len_cap=up(np.array(len_caps, dtype=np.int32)))
    dc.set_option("route_count", 1)
    try:
        dc.route_read("fqz")
        dc.route_read("launch")
        dc.fqz_uncompress(d_in, d_ioff, d_isz, d_out, d_ooff, d_cap, d_osz, d_st, max_in or max([len(s) for s in streams] + [1]),
                          max_out or max(list(caps) + [1]), total, nrec=d_nrec, **kw)
        t.cuda.synchronize(dev)
        route, launch = dc.route_read("fqz"), dc.route_read("launch")
    finally:
        dc.set_option("route_count", 0)
    assert launch["side_by_side"] == 0 and launch["in_order"] >= 1
    if want_chunks is not None:
        assert launch["in_order"] == want_chunks, launch
    arena = d_out.cpu().numpy()
    stray = lay.stray_writes(arena)
    assert stray is None, stray
    st, osz, nrec = d_st.tolist(), d_osz.tolist(), d_nrec.tolist()
    outs = [b if s == 0 else None for b, s in zip(lay.take(arena, [max(z, 0) for z in osz]), st)]
    for i in range(n):
        assert st[i] >= 0 and (osz[i] == 0 and nrec[i] == 0 if st[i] else 0 <= osz[i] <= caps[i] and nrec[i] >= 0), (i, st[i], osz[i], nrec[i])
    lens = [None] * n
    if len_caps is not None:
        got = kw["d_len"].cpu().numpy()
        mask = np.zeros(len(got), dtype=bool)
        for i, (o, c) in enumerate(zip(len_off, len_caps)):
            k = min(nrec[i], c) if st[i] == 0 else 0
            mask[o:o + k] = True
            lens[i] = got[o:o + k].tolist()
            if st[i] != 0:
                mask[o:o + c] = True                                 # a refused stream's slot may hold anything
        bad = np.nonzero((got != len_fill) & ~mask)[0]
        assert not len(bad), ("lengths written outside their slots", bad[:8].tolist())
    return outs, st, lens, nrec, route


def check(dc, streams, caps=None, want=None, len_caps="exact", **kw):
    """run_dev against the model: statuses, bytes, lengths, record counts and route.  caps: default the stored sizes (1
    for a stream that stores none).  len_caps "exact": as many entries as the model counts records.  want: the raw inputs,
    where every stream must decode to them."""
    if caps is None:
        caps = [max(M.parse(s)[1].out_size, 1) if M.var_get(s, 0, len(s))[1] <= 1 << 24 else 1 for s in streams]
    res, route = expect(streams, caps)
    if len_caps == "exact":
        len_caps = [len(r[2]) for r in res]
    outs, st, lens, nrec, got_route = run_dev(dc, streams, caps, len_caps, **kw)
    for i, ((wst, wout, wlens), out) in enumerate(zip(res, outs)):
        assert st[i] == wst, (i, st[i], wst, streams[i][:16].hex(), caps[i])
        if wst == 0:
            assert out == wout, (i, "bytes differ", streams[i][:16].hex(), len(wout))
            assert nrec[i] == len(wlens), (i, nrec[i], len(wlens))
            if len_caps is not None:
                assert lens[i] == wlens[:len_caps[i]], (i, "lengths differ")
            if want is not None:
                assert wout == want[i], (i, "the model does not give the raw input")
    if want is not None:
        assert all(s == 0 for s in st)
    assert got_route == route, (got_route, route)
    return outs, st, lens, nrec, got_route
