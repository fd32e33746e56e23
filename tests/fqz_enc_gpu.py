"""What the GPU tests of fqzcomp_qual encoding share (test_gpu_fqz_enc.py): one run of rans4x16_hip_fqz_compress_dev over
a list of blocks with the confinement pattern of test_gpu_confinement.py - the output slots a few bytes apart at every
alignment in an arena filled with a pattern, every byte outside them compared afterwards; inputs, parameter bytes and
records at odd places of their arenas - and the answers of the Python model (fqz_enc_model.py), computed once per block.

A block is (data, lens, flags, params): the slice as the parameter choice leaves it, and the parameter bytes."""
import collections

import numpy as np

import fqz_enc_model as E
import fqz_model as M
from test_gpu_confinement import Layout

KINDS = E.KINDS
_answers = {}


def answer(block, max_sym_limit=255):
    """(status, the stream or None, route) of the model, capacity aside, computed once"""
    data, lens, flags, params = block
    key = (bytes(data), tuple(lens), tuple(flags), bytes(params), max_sym_limit)
    if key not in _answers:
        st = E.verdict(data, lens, flags, params, max_sym_limit)
        route = collections.Counter()
        out = E.compress(data, lens, flags, params, route=route) if st == 0 else None
        _answers[key] = (st, out, dict(route))
    return _answers[key]


def expect(blocks, caps, max_sym_limit=255):
    res, route = [], collections.Counter({k: 0 for k in KINDS})
    for b, cap in zip(blocks, caps):
        st, out, r = answer(b, max_sym_limit)
        if st == 0 and len(out) > cap:
            st, out = M.E_CAPACITY, None
            r = {k: v for k, v in r.items() if k != "dup"}           # the stream reached a wave; it did not finish
        res.append((st, out))
        route.update(r)
    return res, dict(route)


def run_dev(dc, blocks, caps, max_in=None, max_par=None, max_rec=None):
    """-> ([bytes or None], statuses, route).  Asserts that nothing outside the slots was written and that the inputs are
    as they were."""
    import torch as t
    n = len(blocks)
    lay = Layout(caps, what=[len(b[0]) for b in blocks])
    in_off, par_off, rec_off, pos, ppos, rpos = [], [], [], 3, 1, 2
    for i, (data, lens, flags, params) in enumerate(blocks):
        in_off.append(pos); par_off.append(ppos); rec_off.append(rpos)
        pos += len(data) + 1 + i % 7
        ppos += len(params) + i % 5
        rpos += len(lens) + i % 3
    arena_in = np.full(pos + 64, 0xee, dtype=np.uint8)
    arena_par = np.full(ppos + 64, 0xee, dtype=np.uint8)
    a_len = np.full(rpos + 8, 0x7fffffff, dtype=np.int64)
    a_fl = np.full(rpos + 8, 0x7fffffff, dtype=np.int64)
    for (data, lens, flags, params), o, po, ro in zip(blocks, in_off, par_off, rec_off):
        arena_in[o:o + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
        arena_par[po:po + len(params)] = np.frombuffer(bytes(params), dtype=np.uint8)
        a_len[ro:ro + len(lens)] = lens
        a_fl[ro:ro + len(flags)] = flags
    as_i32 = lambda a: np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)
    dev = dc.dev
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_in, d_par, d_out = up(arena_in), up(arena_par), up(lay.pattern.copy())
    d_len, d_fl = up(as_i32(a_len)), up(as_i32(a_fl))
    i64 = lambda v: up(np.array(v, dtype=np.int64))
    d_osz = t.full((n,), -7, dtype=t.int32, device=dev)
    d_st = t.full((n,), -7, dtype=t.int32, device=dev)
    dc.set_option("route_count", 1)
    try:
        dc.route_read("fqz_enc")
        dc.route_read("launch")
        dc.fqz_compress(d_in, i64(in_off), up(as_i32([len(b[0]) for b in blocks])),
                        d_par, i64(par_off), up(as_i32([len(b[3]) for b in blocks])),
                        d_len, d_fl, i64(rec_off), up(as_i32([len(b[1]) for b in blocks])),
                        d_out, up(lay.offs.copy()), up(as_i32(caps)), d_osz, d_st,
                        max_in if max_in is not None else max([len(b[0]) for b in blocks] + [1]),
                        max_par if max_par is not None else max([len(b[3]) for b in blocks] + [1]),
                        max_rec if max_rec is not None else max([len(b[1]) for b in blocks] + [1]))
        t.cuda.synchronize(dev)
        route, launch = dc.route_read("fqz_enc"), dc.route_read("launch")
    finally:
        dc.set_option("route_count", 0)
    assert launch["side_by_side"] == 0 and launch["in_order"] >= 1
    arena = d_out.cpu().numpy()
    stray = lay.stray_writes(arena)
    assert stray is None, stray
    assert (d_in.cpu().numpy() == arena_in).all(), "the call changed its input"
    st, osz = d_st.tolist(), d_osz.tolist()
    for i in range(n):
        assert st[i] >= 0 and (osz[i] == 0 if st[i] else 0 < osz[i] <= caps[i]), (i, st[i], osz[i])
    outs = [b if s == 0 else None for b, s in zip(lay.take(arena, [max(z, 0) for z in osz]), st)]
    return outs, st, route


def check(dc, blocks, caps=None, max_sym_limit=None, **kw):
    """run_dev against the model: statuses, bytes and route.  caps: default rans4x16_hip_fqz_compress_cap.  The slots are
    sized (set_fqz_limits) for the batch's largest max_sym unless max_sym_limit says otherwise."""
    if caps is None:
        caps = [E.cap(len(b[0]), len(b[1]), len(b[3])) for b in blocks]
    limit = max_sym_limit
    if limit is None:
        syms = [E.parse_params(b[3]) for b in blocks]
        limit = max([h.max_sym for st, h in syms if st == 0] + [1])
    res, route = expect(blocks, caps, limit)
    dc.set_fqz_limits(kw.pop("max_slots", 0), limit)
    try:
        outs, st, got_route = run_dev(dc, blocks, caps, **kw)
    finally:
        dc.set_fqz_limits(0, 0)
    for i, ((wst, wout), out) in enumerate(zip(res, outs)):
        assert st[i] == wst, (i, st[i], wst, len(blocks[i][0]), caps[i])
        if wst == 0:
            assert out == wout, (i, "bytes differ", len(out), len(wout))
    assert got_route == route, (got_route, route)
    return outs, st, got_route


def decode_back(dc, streams, blocks):
    """every stream through DeviceCodec.fqz_uncompress: the block's bytes and its record lengths"""
    import fqz_gpu
    caps = [max(len(b[0]), 1) for b in blocks]
    limit = max([M.parse(s)[1].max_sym for s in streams] + [1])
    dc.set_fqz_limits(0, limit)
    try:
        outs, st, lens, nrec, route = fqz_gpu.run_dev(dc, streams, caps, [len(b[1]) for b in blocks])
    finally:
        dc.set_fqz_limits(0, 0)
    for i, b in enumerate(blocks):
        assert st[i] == 0 and outs[i] == bytes(b[0]), (i, st[i])
        if len(b[0]):
            assert lens[i] == list(b[1]), (i, "lengths differ")
