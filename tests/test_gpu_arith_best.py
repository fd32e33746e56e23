"""rans4x16_hip_arith_compress_best_packed_dev (include/rans4x16_hip.h part 2h) against the model: tok3_model.best over
arith_enc_model.compress - bytes, sizes, offsets, d_chosen and statuses -, the sizing pass, a capacity that cuts the
batch, confinement in a patterned arena, the route's candidate count and a run in chunks."""
import numpy as np
import pytest

import arith_enc_model as AE
import tok3_arith_model as TA
import tok3_model as M
from test_gpu_confinement import pattern

pytestmark = pytest.mark.gpu

GUARD = 4096
UNSUPPORTED, CAPACITY = 6, 1
# tokenise_name3.c:1255-1259, then stripe methods only, then one method
LISTS = [TA.ROWS[1], TA.ROWS[3], TA.ROWS[5], TA.ROWS[7], TA.ROWS[9], [200, 201, 8], [65]]


@pytest.fixture(scope="module")
def dc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd.DeviceCodec(0)


def _text(n, seed):
    rng = np.random.default_rng(seed)
    return bytes(rng.choice(np.frombuffer(b"ACGT0123:.", dtype=np.uint8), size=n, p=[.3, .2, .2, .1, .04, .04, .04, .04, .02, .02]).tolist())


@pytest.fixture(scope="module")
def blocks():
    """The described columns of two reference containers (sizes 1 to 4,000) and the constructed sizes."""
    fx = dict(TA.fixtures())
    out = []
    for name in ("nv2.names.19", "01.names.19"):
        w = M.walk(TA.cleared(fx[name]))
        cols = TA.columns(fx[name], w)
        out += [cols[i] for _, i in M.described(w) if 1 <= len(cols[i]) <= 4000]
    assert min(map(len, out)) >= 1 and max(map(len, out)) > 2000 and len(out) > 40
    out += [_text(n, n) for n in (0, 1, 3, 4, 20, 21, 24, 4001)]
    return out


_memo = {}


def _compress(data, method):
    """arith_enc_model.compress with its candidate streams' route, made once per (column, method)"""
    key = (data, method)
    if key not in _memo:
        trace = []
        s = AE.compress(data, method, trace=trace)
        _memo[key] = (s, AE.route_of(trace))
    return _memo[key]


def _expect(blocks, methods):
    """Per block (method or -1, stream or None), and the route of every candidate that was tried."""
    want, route = [], dict.fromkeys(AE.KINDS, 0)
    for data in blocks:
        win = M.best(lambda d, m: _compress(d, m)[0], data, methods)
        want.append(win if win is not None else (-1, None))
        for m in methods:
            if len(data) % 4 != 0 and (m & 8):
                continue
            for k, v in _compress(data, m)[1].items():
                route[k] += v
    return want, route


class _Res:
    pass


def _run(dc, blocks, methods, capacity=None, sizing=False, alloc=None, gap=7, total=None):
    import torch
    dev = dc.dev
    n = len(blocks)
    raw, offs = bytearray(b"\xee" * gap), []
    for b in blocks:
        offs.append(len(raw))
        raw += b + b"\xee" * gap
    d_in = torch.from_numpy(np.frombuffer(bytes(raw) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    in_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    in_size = torch.tensor([len(b) for b in blocks], dtype=torch.int32, device=dev)
    r = _Res()
    r.alloc = (sum(len(b) + 160 for b in blocks) if alloc is None else alloc) + GUARD
    r.pat = pattern(r.alloc)
    d_out = None if sizing else torch.from_numpy(r.pat.copy()).to(dev)
    r.cap = 0 if sizing else (r.alloc - GUARD if capacity is None else capacity)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    osz = torch.full((n,), -3, dtype=torch.int32, device=dev)
    st = torch.full((n,), -3, dtype=torch.int32, device=dev)
    chosen = torch.full((n,), -3, dtype=torch.int32, device=dev)
    dc.set_option("route_count", 1)
    try:
        dc.route_read("arith_enc")
        dc.route_read("launch")
        dc.arith_compress_best_packed(d_in, in_off, in_size, d_out, off, osz, st, methods, max(len(b) for b in blocks), chosen=chosen,
                                      total_in_size=sum(len(b) for b in blocks) if total is None else total, out_capacity=r.cap)
        torch.cuda.synchronize()
        r.route = dc.route_read("arith_enc")
        r.launches = dc.route_read("launch")["in_order"]
    finally:
        dc.set_option("route_count", 0)
    r.arena = None if sizing else d_out.cpu().numpy()
    r.off, r.osz, r.st, r.chosen = off.cpu().numpy().tolist(), osz.cpu().numpy().tolist(), st.cpu().numpy().tolist(), chosen.cpu().numpy().tolist()
    return r


def _check(r, want, what):
    """Everything the call reports against the model; every byte outside the blocks' ranges keeps the pattern."""
    need = [0] + np.cumsum([len(s) if s is not None else 0 for _, s in want]).tolist()
    assert r.off == need, (what, r.off[:8], need[:8])
    mask = np.zeros(r.alloc, dtype=bool)
    for i, (m, s) in enumerate(want):
        tag = (what, i, r.st[i], r.osz[i], r.chosen[i], m)
        assert r.chosen[i] == m, tag
        if s is None:
            assert r.st[i] == UNSUPPORTED and r.osz[i] == 0, tag
        elif need[i + 1] > r.cap:
            assert r.st[i] == CAPACITY and r.osz[i] == 0, tag
        else:
            assert r.st[i] == 0 and r.osz[i] == len(s), tag
            mask[need[i]:need[i + 1]] = True
            assert r.arena[need[i]:need[i + 1]].tobytes() == s, tag
    if r.arena is not None:
        assert np.array_equal(r.arena[~mask], r.pat[~mask]), (what, "a byte outside the blocks' ranges changed")


@pytest.mark.parametrize("methods", LISTS, ids=lambda m: "-".join(map(str, m)))
def test_best_of_k_equals_the_model(dc, blocks, methods):
    want, route = _expect(blocks, methods)
    r = _run(dc, blocks, methods)
    _check(r, want, methods)
    assert r.route == route, (r.route, route)
    # the sizing pass: the same offsets, nothing written, every block that has bytes reports CAPACITY
    s = _run(dc, blocks, methods, sizing=True)
    assert s.off == r.off and s.chosen == r.chosen and not any(s.osz)
    assert all(st == (UNSUPPORTED if w is None else CAPACITY) for st, (_, w) in zip(s.st, want))
    # a capacity that ends inside the block in the middle
    mid = len(blocks) // 2
    cut = _run(dc, blocks, methods, capacity=r.off[mid] + 1)
    _check(cut, want, (methods, "cut"))
    assert CAPACITY in cut.st


def test_the_batch_holds_ties_skipped_methods_and_a_block_without_a_method(blocks):
    ties = skipped = 0
    for data in blocks:
        tried = [m for m in TA.ROWS[9] if not (len(data) % 4 and (m & 8))]
        sizes = [len(_compress(data, m)[0]) for m in tried]
        ties += sizes.count(min(sizes)) > 1
        skipped += len(tried) < len(TA.ROWS[9])
    assert ties >= 1 and skipped >= 1
    want, _ = _expect(blocks, LISTS[5])
    assert any(s is None for _, s in want) and any(s is not None for _, s in want)


def test_a_run_in_chunks_gives_the_same_bytes(dc, blocks):
    methods = TA.ROWS[9]
    want, route = _expect(blocks, methods)
    whole = _run(dc, blocks, methods)
    keep = dc.get_option("max_workspace_mb")
    plan = lambda: dc.arith_best_chunk_blocks(len(blocks), methods, max(len(b) for b in blocks), sum(len(b) for b in blocks))
    assert plan() == len(blocks)                                       # one chunk
    try:
        dc.set_option("max_workspace_mb", 1)
        r = _run(dc, blocks, methods)
        per = plan()                                                   # (the arenas are as the run left them)
    finally:
        dc.set_option("max_workspace_mb", keep)
    # the call's own chunks, from its plan: offsets carried on, pick and gather at a base, the slot arena used again
    chunks = -(-len(blocks) // per)
    assert chunks >= 3 and whole.launches == 1 and r.launches >= chunks, (per, chunks, whole.launches, r.launches)
    _check(r, want, "chunks")
    assert r.route == route and np.array_equal(r.arena, whole.arena)


def test_a_batch_that_holds_more_than_it_announced(dc, blocks):
    """Candidates that find no room fail their block as a whole: a block comes out with the model's winner or not at all,
    never with the smallest of the candidates that happened to find room."""
    methods = TA.ROWS[9]
    want, _ = _expect(blocks, methods)
    r = _run(dc, blocks, methods, total=sum(len(b) for b in blocks) // 3)
    ok = [i for i, st in enumerate(r.st) if st == 0]
    assert ok and len(ok) < len(blocks) and all(st in (0, UNSUPPORTED) for st in r.st), r.st
    assert r.off == [0] + np.cumsum(r.osz).tolist()
    mask = np.zeros(r.alloc, dtype=bool)
    for i, (m, s) in enumerate(want):
        if r.st[i] == 0:
            assert r.chosen[i] == m and r.arena[r.off[i]:r.off[i + 1]].tobytes() == s, i
            mask[r.off[i]:r.off[i + 1]] = True
        else:
            assert r.osz[i] == 0 and r.chosen[i] == -1, i
    assert np.array_equal(r.arena[~mask], r.pat[~mask])


def test_bad_arguments(dc, blocks):
    import torch
    with pytest.raises(RuntimeError, match="255 stripes"):
        _run(dc, blocks[:2], [0, (256 << 8) | 8])
    L, n = dc.L, 1
    z = torch.zeros(4, dtype=torch.int64, device=dc.dev)
    import ctypes as C
    meth = (C.c_int * 33)()
    for k in (0, 33):
        assert L.rans4x16_hip_arith_compress_best_packed_dev(dc.ctx.h, n, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 8,
                                                             z.data_ptr(), z.data_ptr(), z.data_ptr(), k, meth, None, 8, 0, None) == -1
