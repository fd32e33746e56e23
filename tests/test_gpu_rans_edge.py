"""rANS 4x16 and 4x8 on the GPU against reference-made edge and damaged vectors (tests/golden/rans/edge.bin, made by
oracle/make_rans_edge.py from the REFERENCE's answers; README.edge.md beside it; tests/test_rans_edge_cpu.py holds the
oracle to the same file).  Nothing here reads a reference tree, and the oracle is not asked.

Every entry family goes through an entry point in one batch call: the host batches, the drop-in symbols (the stripe
host entry among them), the slot calls on device memory, the packed calls, the best-of calls, and the 4x8 surface.
  - encode vectors come out byte for byte (the large ones by length and SHA-256);
  - reference streams decode to their inputs;
  - a damaged stream whose answer from the reference is stable and accepted decodes to the reference's length and
    SHA-256 - or one of rans_edge_cases.DEVIATIONS holds for its bytes and the status is that entry's own;
  - a stable refused stream is refused;
  - an unstable stream may get any status; like every other it is decoded into a slot between guard bytes, and nothing
    outside the slots is written.
The device gets no allowance of its own: only the predicates."""
import time

import numpy as np
import pytest

import rans_edge_cases as X
from test_gpu_confinement import _Guarded, caps_of

pytestmark = pytest.mark.gpu
PLAIN = [0, 1, 128, 129, 64, 65, 192, 193]              # a best-of list every size_* case has a vector for, in the order tried
STRIPE_PLANES, MAX_BLOCK = 32, 70000


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
def vectors():
    """{16: [(case, vector, input)], 8: ...}: the inputs are made once and shared."""
    out = {16: [], 8: []}
    for c in X.load().cases:
        data = X.case_input(c)
        out[c.codec] += [(c, v, data) for v in c.vectors]
    return out


def held(v, got):
    """got is the vector's stream (the large ones: its length and SHA-256)."""
    return got is not None and (got == v.stream if isinstance(v.stream, bytes) else X.digest(got) == v.stream)


def check_encoded(label, picked, got, status):
    bad = [(c.name, hex(v.order), int(s)) for (c, v, _), g, s in zip(picked, got, status) if s != 0 or not held(v, g)]
    assert not bad, (label, len(bad), bad[:10])


def check_decoded(label, picked, got, status):
    bad = [(c.name, hex(v.order), int(s)) for (c, v, d), g, s in zip(picked, got, status) if s != 0 or g != d]
    assert not bad, (label, len(bad), bad[:10])


def timed(label, t0):
    import torch
    torch.cuda.synchronize()
    print("%s: %.2f s" % (label, time.time() - t0))


def judge(label, codec, entries, got, status, named=True):
    """entries: [(Damaged, stream, capacity)]; got: bytes or None per entry.  named=False: the call gives no status, so a
    refusal inside a deviation is not held to the entry's own."""
    bad, used = [], {}
    for (d, stream, cap), g, s in zip(entries, got, status):
        if d.answer is None:
            continue
        if d.answer == X.REFUSED:
            if g is not None or s == 0:
                bad.append(("the reference refuses", stream[:16].hex(), int(s)))
        elif g is not None:
            if s != 0 or X.digest(g) != d.answer:
                bad.append(("other bytes", stream[:16].hex(), int(s), len(g), d.answer[0]))
        else:
            own = {x.status: x.name for x in X.deviation(codec, stream, cap)}
            if named and s not in own or not own:
                bad.append(("refused outside the named classes", stream[:16].hex(), int(s), sorted(own.values())))
            else:
                name = own[s] if named else sorted(own.values())[0]
                used[name] = used.get(name, 0) + 1
    print(label, "deviations used:", used)
    assert not bad, (label, len(bad), bad[:10])
    return used


# ---- rANS 4x16: encode vectors and reference streams ---------------------------------------------------------------------
def test_host_batches_4x16(H, vectors):
    t0 = time.time()
    picked = vectors[16]
    enc, st = H.compress_batch([d for _, _, d in picked], [v.order for _, v, _ in picked])
    check_encoded("compress_batch", picked, enc, st)
    dec, st = H.uncompress_batch(enc, [len(d) for _, _, d in picked])
    check_decoded("uncompress_batch", picked, dec, st)
    timed("host batches 4x16, %d vectors" % len(picked), t0)


def test_drop_in_symbols_and_the_stripe_host_entry(H, vectors):
    """rans_compress_to_4x16 / rans_uncompress_to_4x16 / rans_uncompress_4x16 of the library, one call a vector: every
    stripe vector, and every case's first."""
    t0 = time.time()
    picked = [p for k, p in enumerate(vectors[16]) if p[1].order & X.X_STRIPE or p[1] is p[0].vectors[0]]
    assert sum(bool(v.order & X.X_STRIPE) for _, v, _ in picked) >= 60
    for c, v, data in picked:
        got = H.rans_compress_4x16(data, v.order)
        assert held(v, got), (c.name, hex(v.order))
        assert H.rans_uncompress_4x16(got, len(data)) == data, (c.name, hex(v.order))
        if not got[0] & X.X_NOSZ or got[0] & X.X_STRIPE:
            assert H.rans_uncompress_4x16(got) == data, (c.name, hex(v.order))
    timed("drop-in symbols, %d vectors" % len(picked), t0)


def test_slot_calls_4x16(H, dc, vectors):
    """rans4x16_hip_compress_dev under per-block orders (every vector without X_STRIPE in one call) and under one order
    (a call per stripe order), rans4x16_hip_uncompress_dev over every reference stream in one call; slots of exactly
    the bound / the stored size between guard bytes."""
    import torch
    t0 = time.time()
    plain = [p for p in vectors[16] if not p[1].order & X.X_STRIPE]
    what = lambda picked: [(c.name, hex(v.order)) for c, v, _ in picked]
    G = _Guarded(dc.dev, [d for _, _, d in plain], caps_of([H.rans_compress_bound_4x16(len(d), v.order) for _, v, d in plain]), what(plain))
    dc.compress(*G.args(), 0, G.max_in, d_order=torch.tensor([v.order for _, v, _ in plain], dtype=torch.int32, device=dc.dev), total_in_size=G.total_in)
    st, osz, got = G.results("compress_dev")
    check_encoded("compress_dev", plain, got, st)
    streams = {(c.name, v.order): g for (c, v, _), g in zip(plain, got)}
    stripes = [p for p in vectors[16] if p[1].order & X.X_STRIPE]
    for order in sorted({v.order for _, v, _ in stripes}):
        picked = [p for p in stripes if p[1].order == order]
        G = _Guarded(dc.dev, [d for _, _, d in picked], caps_of([H.rans_compress_bound_4x16(len(d), order) for _, _, d in picked]), what(picked))
        dc.compress(*G.args(), order, G.max_in)
        st, osz, got = G.results(("compress_dev", hex(order)))
        check_encoded(("compress_dev", hex(order)), picked, got, st)
        streams.update({(c.name, v.order): g for (c, v, _), g in zip(picked, got)})
    timed("slot calls 4x16, encode", t0)
    # decode: the capacity of a stream without a size field and of a stripe stream IS its size (:1379, :1447)
    t0 = time.time()
    picked = vectors[16]
    comps = [streams[(c.name, v.order)] for c, v, _ in picked]
    caps = [len(d) + (37 if k % 3 == 2 and not s[0] & 0x18 else 0) for k, ((_, _, d), s) in enumerate(zip(picked, comps))]
    assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, STRIPE_PLANES, MAX_BLOCK) == 0
    try:
        G = _Guarded(dc.dev, comps, caps, what(picked))
        dc.uncompress(*G.args(), G.max_in, G.max_cap)
        st, osz, got = G.results("uncompress_dev")
        check_decoded("uncompress_dev", picked, got, st)
    finally:
        assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 0, 0) == 0
    timed("slot calls 4x16, decode of %d streams" % len(picked), t0)


def test_packed_calls_4x16(H, dc, vectors):
    """rans4x16_hip_compress_packed_dev under per-block orders and rans4x16_hip_uncompress_packed_dev on its output, the
    sizes of the streams without a size field handed over."""
    import torch
    t0 = time.time()
    picked = [p for p in vectors[16] if not p[1].order & X.X_STRIPE]
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).to(dc.dev)
    sizes = [len(d) for _, _, d in picked]
    n = len(picked)
    d_in = t(np.frombuffer(b"".join(d for _, _, d in picked) + b"\0", dtype=np.uint8).copy(), np.uint8)
    in_off = t(np.concatenate([[0], np.cumsum(sizes)[:-1]]), np.int64)
    in_size = t(sizes, np.int32)
    room = sum(H.rans_compress_bound_4x16(len(d), v.order) for _, v, d in picked)
    d_out = torch.zeros(room, dtype=torch.uint8, device=dc.dev)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dc.dev)
    out_size = torch.zeros(n, dtype=torch.int32, device=dc.dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dc.dev)
    dc.compress_packed(d_in, in_off, in_size, d_out, out_off, out_size, status, 0, max(sizes), d_order=t([v.order for _, v, _ in picked], np.int32),
                       total_in_size=sum(sizes))
    torch.cuda.synchronize()
    off, osz, st, out = out_off.cpu().numpy(), out_size.cpu().numpy(), status.cpu().numpy(), d_out.cpu().numpy()
    assert (off[1:] - off[:-1] == osz).all() and off[0] == 0
    check_encoded("compress_packed_dev", picked, [out[o:o + k].tobytes() for o, k in zip(off, osz)], st)
    back = torch.zeros(sum(sizes) + 1, dtype=torch.uint8, device=dc.dev)
    back_off = torch.zeros(n + 1, dtype=torch.int64, device=dc.dev)
    back_size = torch.zeros(n, dtype=torch.int32, device=dc.dev)
    st2 = torch.full((n,), -1, dtype=torch.int32, device=dc.dev)
    dc.uncompress_packed(d_out, out_off, out_size, back, back_off, back_size, st2, int(osz.max()), max(sizes), nosz_size=in_size)
    torch.cuda.synchronize()
    boff, bsz, host = back_off.cpu().numpy(), back_size.cpu().numpy(), back.cpu().numpy()
    check_decoded("uncompress_packed_dev", picked, [host[o:o + k].tobytes() for o, k in zip(boff, bsz)], st2.cpu().numpy())
    timed("packed calls 4x16, %d vectors" % n, t0)


def test_best_of_calls_keep_the_first_smallest_reference_stream(H, dc, vectors):
    """rans4x16_hip_compress_best_batch and rans4x16_hip_compress_best_dev under a list every size_* case holds a
    reference stream for: the smallest of them stands, the first tried on a tie (:1199, tokenise_name3.c:1246-1300)."""
    import torch
    t0 = time.time()
    cases = [c for c in X.load().cases if c.name.startswith("size_")]
    assert len(cases) == 34
    want = []
    for c in cases:
        by = {v.order: v.stream for v in c.vectors}
        best = min(PLAIN, key=lambda m: (len(by[m]), PLAIN.index(m)))
        want.append((by[best], best))
    assert sum(sum(len(dict((v.order, v.stream) for v in c.vectors)[m]) == len(w) for m in PLAIN) > 1 for c, (w, _) in zip(cases, want)) >= 10   # ties
    datas = [c.data for c in cases]
    enc, chosen, st = H.compress_best_batch(datas, PLAIN)
    assert [(e, m, s) for e, m, s in zip(enc, chosen, st)] == [(w, m, 0) for w, m in want]
    G = _Guarded(dc.dev, datas, caps_of([max(H.rans_compress_bound_4x16(len(d), m) for m in PLAIN) for d in datas]), [c.name for c in cases])
    dc.compress_best(*G.args(), PLAIN, G.max_in, chosen=G.chosen)
    st, osz, got = G.results("compress_best_dev")
    assert [(g, int(m), int(s)) for g, m, s in zip(got, G.chosen.cpu().numpy(), st)] == [(w, m, 0) for w, m in want]
    timed("best-of calls, %d blocks" % len(cases), t0)


# ---- rANS 4x16: damaged streams ----------------------------------------------------------------------------------------
def test_damaged_streams_4x16(H, dc):
    t0 = time.time()
    ds = X.damaged_streams(16)
    # handed over with a capacity: rans4x16_hip_uncompress_batch, and rans4x16_hip_uncompress_dev between guard bytes
    to = [(d, s, d.capacity) for d, s in ds if d.op == X.OP_U16_TO]
    dec, st = H.uncompress_batch([s for _, s, _ in to], [c for _, _, c in to])
    judge("uncompress_batch", 16, to, dec, st)
    timed("damaged 4x16, host batch of %d" % len(to), t0)
    t0 = time.time()
    assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 255, MAX_BLOCK) == 0
    try:
        G = _Guarded(dc.dev, [s for _, s, _ in to], [c for _, _, c in to], [s[:8].hex() for _, s, _ in to])
        dc.uncompress(*G.args(), G.max_in, G.max_cap)
        st, osz, got = G.results("uncompress_dev, damaged")
        judge("uncompress_dev", 16, to, [g if s == 0 else None for g, s in zip(got, st)], st)
    finally:
        assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 0, 0) == 0
    timed("damaged 4x16, slot call of %d" % len(to), t0)
    # handed over without a buffer: rans_uncompress_4x16, the callee sizes the result
    t0 = time.time()
    free = [(d, s, 0) for d, s in ds if d.op == X.OP_U16]
    got = [H.rans_uncompress_4x16(s) for _, s, _ in free]
    judge("rans_uncompress_4x16", 16, free, got, [0 if g is not None else -1 for g in got], named=False)
    timed("damaged 4x16, %d drop-in calls" % len(free), t0)


def test_the_drop_in_symbol_refuses_within_the_named_classes(H):
    """The drop-in symbol gives no status, so the test above cannot hold its refusals to an entry's own: here every
    stable accepted stream it refuses goes through the batch call, which names the status, with the capacity the symbol
    allocates: the stream's size field."""
    ds = [(d, s) for d, s in X.damaged_streams(16) if d.op == X.OP_U16 and d.answer not in (None, X.REFUSED)]
    refused = [(d, s, X.size_field(s)) for d, s in ds if H.rans_uncompress_4x16(s) is None]
    print(len(refused), "of", len(ds), "refused")
    assert refused
    if refused:
        dec, st = H.uncompress_batch([s for _, s, _ in refused], [c for _, _, c in refused])
        assert all(x is None for x in dec)
        used = judge("uncompress_batch of what the drop-in symbol refused", 16, refused, dec, st)
        # every 4x16 entry has a member here: a stream the reference accepts stably and the device refuses with its status
        assert set(used) == {x.name for x in X.DEVIATIONS if x.codec == 16 and x.what == "decode"}, used


# ---- rANS 4x8 --------------------------------------------------------------------------------------------------------
def test_host_batches_and_slot_calls_4x8(H, dc, vectors):
    t0 = time.time()
    picked = vectors[8]
    datas, orders = [d for _, _, d in picked], [v.order for _, v, _ in picked]
    enc, st = H.compress_batch_4x8(datas, orders)
    check_encoded("compress_batch_4x8", picked, enc, st)
    dec, st = H.uncompress_batch_4x8(enc, [len(d) for d in datas])
    check_decoded("uncompress_batch_4x8", picked, dec, st)
    for (c, v, d), e in zip(picked[:6], enc):
        assert H.rans_compress(d, v.order) == e and H.rans_uncompress(e) == d, c.name
    enc0, st0 = H.compress_batch_4x8([b""], [0])                           # DEVIATIONS: x8_encode_nothing
    assert enc0 == [None] and st0[0] != 0 and [x.name for x in X.deviation(8, b"", what="encode")] == ["x8_encode_nothing"]
    import torch
    what = [(c.name, v.order) for c, v, _ in picked]
    G = _Guarded(dc.dev, datas, caps_of([dc.L.rans4x8_hip_compress_bound(len(d)) for d in datas]), what)
    dc.compress_4x8(*G.args(), 0, G.max_in, d_order=torch.tensor(orders, dtype=torch.int32, device=dc.dev))
    st, osz, got = G.results("rans4x8_hip_compress_dev")
    check_encoded("rans4x8_hip_compress_dev", picked, got, st)
    G = _Guarded(dc.dev, got, caps_of([len(d) for d in datas]), what)
    dc.uncompress_4x8(*G.args())
    st, osz, back = G.results("rans4x8_hip_uncompress_dev")
    check_decoded("rans4x8_hip_uncompress_dev", picked, back, st)
    timed("4x8, %d vectors" % len(picked), t0)


def test_damaged_streams_4x8(H, dc):
    """The reference allocates what bytes 5 to 8 claim; so does this test, for every claim a stable accepted stream makes."""
    t0 = time.time()
    ds = X.damaged_streams(8)
    claim = lambda s: int.from_bytes(s[5:9], "little") if len(s) >= 9 else 0
    entries = [(d, s, claim(s)) for d, s in ds]
    assert all(c < 1 << 20 for _, _, c in entries)
    dec, st = H.uncompress_batch_4x8([s for _, s, _ in entries], [c for _, _, c in entries])
    names = {x.name for x in X.DEVIATIONS if x.codec == 8 and x.what == "decode"}
    assert set(judge("uncompress_batch_4x8", 8, entries, dec, st)) == names            # every 4x8 entry has a member
    small = entries
    G = _Guarded(dc.dev, [s for _, s, _ in small], [c for _, _, c in small], [s[:12].hex() for _, s, _ in small])
    dc.uncompress_4x8(*G.args())
    st, osz, got = G.results("rans4x8_hip_uncompress_dev, damaged")
    assert set(judge("rans4x8_hip_uncompress_dev", 8, small, [g if s == 0 else None for g, s in zip(got, st)], st)) == names
    timed("damaged 4x8, %d streams" % len(entries), t0)
