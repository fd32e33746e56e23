"""Device calls write only inside their callers' slots (include/rans4x16_hip.h part 2: block i owns
d_out + d_out_off[i] for d_out_cap[i] bytes and nothing else).  Every other GPU test reads back out[off : off + size] of a
zero-filled arena with roomy slots; here the output arena is filled with a position-dependent pattern, the slots lie a few
bytes apart at every alignment with capacities of exactly what the interface asks for, and after the call EVERY byte outside
the slots must still hold the pattern - next to the usual assertions inside them (status 0, the oracle's bytes).  The bytes
between a block's produced size and its capacity are the callee's to clobber and are not looked at.

Shapes: the sizes on either side of the 16- and 32-byte trips of the unpacking loops and of the point where their four-deep
pipeline runs out (4 x 64 and 4 x 256 lanes of 16 / 32 bytes), alphabets for every X_PACK width, run-heavy data for X_RLE,
quality data for the ordinary rows, every flag set the device calls take; the CPU test below pins that the oracle's streams
of this corpus really hold those shapes."""
import ctypes as C

import numpy as np
import pytest

import datagen

SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 16383, 16385,
         65535, 65537,
         127, 129, 191, 193, 639, 641,            # 64 k +- 1
         8191, 8193, 32767, 32769]                # 4 x 64 x 32 +- 1, 4 x 256 x 32 +- 1 (4 x 64 x 16 and 4 x 256 x 16 +- 1 are above)
ORDERS = [0, 1, 64, 65, 128, 129, 192, 193, 32, 33, 17, 0xd1]
PACK_ORDERS = [128, 129, 192, 193, 0xd1]
# rand alphabets of 1 .. 17 symbols (X_PACK: none, 8, 4, 2 codes per byte; 17: the flag is dropped), runs, quality tiles
ALPHABETS = [("rand", 1), ("rand", 2), ("rand", 3), ("rand", 4), ("rand", 5), ("rand", 16), ("rand", 17),
             ("runs",), ("q4",), ("q40+dir",)]
STRIPE_METHODS = [8, 9, 0xc9, (2 << 8) | 9, (3 << 8) | 0xc9, (7 << 8) | 8]
GAPS = (1, 3, 16, 64, 512)
GUARD = 512


def pattern(n):
    """p[i] = (i * 167 + 13) & 0xff (of period 256)."""
    return np.resize(((np.arange(256) * 167 + 13) & 0xff).astype(np.uint8), n)


def _data(alph, n, seed):
    if alph[0] == "rand":
        return datagen.rand(n, seed, alph[1], 33 + seed % 50)
    if alph[0] == "runs":
        return datagen.runs(n, 5, 9, seed, 40)
    return datagen.tile(alph[0], n, seed)


_CORPUS = None
_STREAMS = {}


def corpus():
    """[(bytes, order)]: every size with every alphabet.  The small alphabets take the X_PACK flag sets in turn (that is
    where the unpacking loops run), the others walk through all twelve flag sets."""
    global _CORPUS
    if _CORPUS is None:
        out = []
        for si, n in enumerate(SIZES):
            for ai, alph in enumerate(ALPHABETS):
                packs = alph[0] == "rand" and alph[1] <= 16
                order = PACK_ORDERS[(si + ai) % len(PACK_ORDERS)] if packs else ORDERS[(si + 5 * ai) % len(ORDERS)]
                out.append((np.ascontiguousarray(_data(alph, n, 7 * si + ai + 1)).tobytes(), order))
        _CORPUS = out
    return _CORPUS


def streams(oracle, tag, blocks, orders):
    """The oracle's streams, computed once per (tag) and shared by the tests."""
    if tag not in _STREAMS:
        _STREAMS[tag] = [oracle.compress(b, o) for b, o in zip(blocks, orders)]
    return _STREAMS[tag]


def stripe_blocks():
    rs = np.random.RandomState(31)
    blocks = [datagen.tile("q40+dir", n, n).tobytes() for n in (20, 21, 22, 23, 24, 25, 26, 27, 63, 65, 255, 257, 1001, 4097)]
    blocks += [rs.randint(0, 300, 1024).astype("<u4").tobytes(), rs.randint(0, 70000, 4096).astype("<u4").tobytes()[:16383],
               (1000 + 3 * np.arange(16384)).astype("<u4").tobytes()[:65535], datagen.tile("q8", 65537, 3).tobytes(),
               datagen.runs(30001, 5, 9, 4, 40).tobytes(), datagen.rand(12289, 5, 4, 65).tobytes()]
    return blocks


# ---- layout and the guard check (numpy only) -------------------------------------------------------------------
class Layout:
    """Slots in one arena: slot i starts at an offset that is i mod 16 modulo 16, behind a gap of at least GAPS[i mod 5]
    bytes after its predecessor (the smallest such offset: the two rules together leave up to 15 bytes of choice), with
    GUARD bytes before the first slot and after the last.  `what` describes block i in a failure message."""

    def __init__(self, caps, what=None):
        self.caps = np.asarray(caps, dtype=np.int64)
        offs, pos = [], GUARD
        for i, c in enumerate(self.caps):
            pos += GAPS[i % len(GAPS)] if i else 0
            pos += (i % 16 - pos) % 16
            offs.append(pos)
            pos += int(c)
        self.offs = np.array(offs, dtype=np.int64)
        self.size = pos + GUARD
        self.what = what or [None] * len(self.caps)
        mask = np.zeros(self.size, dtype=bool)
        for o, c in zip(self.offs, self.caps):
            mask[o:o + c] = True
        self.mask = mask
        self.pattern = pattern(self.size)

    def stray_writes(self, arena):
        """None, or the report of the bytes outside every slot that no longer hold the pattern."""
        arena = np.asarray(arena)
        assert arena.shape == self.pattern.shape
        bad = np.nonzero((arena != self.pattern) & ~self.mask)[0]
        if not len(bad):
            return None
        first, last = int(bad[0]), int(bad[-1])
        ends = self.offs + self.caps
        # the nearest slot to the first offender; distance < 0: so many bytes before its start, > 0: past its last byte
        dist = np.where(first < self.offs, first - self.offs, first - ends + 1)
        k = int(np.argmin(np.abs(dist)))
        return ("%d bytes written outside every slot: first at %d, last at %d; nearest block %d %r (slot [%d, %d)), "
                "signed distance %+d" % (len(bad), first, last, k, self.what[k], self.offs[k], ends[k], int(dist[k])))

    def take(self, arena, sizes):
        return [np.asarray(arena[o:o + max(int(n), 0)]).tobytes() for o, n in zip(self.offs, sizes)]


def caps_of(exact):
    """Exactly what the interface asks for, for two blocks in three; 37 bytes more for the third."""
    return [int(c) + (37 if i % 3 == 2 else 0) for i, c in enumerate(exact)]


def dec_caps(plains, comps):
    """caps_of for decode: the stored size, or 37 bytes more - except where the capacity IS the size: streams without a
    size field (X_NOSZ) and stripe streams (rANS_static4x16pr.c:1379)."""
    return [len(p) + (37 if i % 3 == 2 and not c[0] & 0x18 else 0) for i, (p, c) in enumerate(zip(plains, comps))]


def pack_width(stream):
    """Codes per byte of a stream's X_PACK header (0: one symbol, 1: the copy case), None without the flag."""
    if not stream or not stream[0] & 0x80 or stream[0] & 0x08:
        return None
    pos = 1
    if not stream[0] & 0x10:
        while stream[pos] & 0x80:
            pos += 1
        pos += 1
    n = stream[pos] or 256
    return 0 if n <= 1 else 8 if n <= 2 else 4 if n <= 4 else 2 if n <= 16 else 1


def _varint(stream, pos):
    v = 0
    while True:
        v = (v << 7) | (stream[pos] & 0x7f)
        pos += 1
        if not stream[pos - 1] & 0x80:
            return v, pos


def rle_meta_len(stream):
    """Bytes of run-length meta data of a stream with X_RLE (0 without the flag)."""
    if not stream or not stream[0] & 0x40 or stream[0] & 0x08:
        return 0
    pos = 1
    if not stream[0] & 0x10:
        _, pos = _varint(stream, pos)
    if stream[0] & 0x80:                                   # the X_PACK header: symbol count, map, packed length
        n = stream[pos] or 256
        pos += 1 + (n if n <= 16 else 0)
        _, pos = _varint(stream, pos)
    mlen, pos = _varint(stream, pos)
    return mlen // 2


# ---- CPU: the corpus holds what it claims, the guard check sees what it must ----------------------------------
def test_inputs_hold_what_they_claim(oracle):
    blocks, orders = zip(*corpus())
    want = streams(oracle, "corpus", blocks, orders)
    assert len(blocks) <= 400 and max(len(b) for b in blocks) <= 70000
    assert set(orders) == set(ORDERS)
    for b, w in zip(blocks, want):
        assert oracle.uncompress(w, capacity=len(b), out_size_hint=len(b)) == b
    by_width = {}
    for b, w in zip(blocks, want):
        by_width.setdefault(pack_width(w), set()).add(len(b))
    print("pack widths:", {k: len(v) for k, v in by_width.items()})
    # every X_PACK width, the one-symbol and the copy case; streams that asked for X_PACK and lost the flag
    for width, trip in ((8, 32), (4, 16), (2, 16)):
        sizes = by_width[width]
        assert {0, 1, trip - 1} <= {n % trip for n in sizes}, (width, sorted(sizes))
        for lanes in (64, 256):                                # the four-deep pipeline of the trips runs out here
            assert {4 * lanes * trip - 1, 4 * lanes * trip + 1} <= sizes, (width, lanes)
    assert by_width.get(0), "no one-symbol X_PACK stream"
    dropped = [w for w, o in zip(want, orders) if o & 0x80 and not w[0] & 0x80]
    assert len(dropped) >= 10, len(dropped)
    # X_RLE streams whose run-length payload is there, with X_PACK in front of it and without; X_CAT streams
    rle = [w for w in want if w[0] & 0x40]
    assert len(rle) >= 20 and sum(1 for w in rle if w[0] & 0x80) >= 5, len(rle)
    assert sum(1 for w in rle if rle_meta_len(w) > 1) >= 10
    assert sum(1 for w in want if w[0] & 0x20) >= 10
    # every decoded size class modulo the 16- and 32-byte trips, over the whole corpus
    assert {n % 16 for n in SIZES} >= {0, 1, 2, 3, 4, 5, 15} and {n % 32 for n in SIZES} >= {0, 1, 15, 16, 17, 31}
    # the stripe blocks: sizes on either side of where the flag is dropped, sizes that are no multiple of N
    for m in STRIPE_METHODS:
        N = (m >> 8) or 4
        sb = stripe_blocks()
        ws = streams(oracle, ("stripe", m), sb, [m] * len(sb))
        assert [bool(w[0] & 8) for w, b in zip(ws, sb) if len(b) in (20, 21)] == [False, True]
        assert sum(1 for b in sb if len(b) % N) >= 5 and sum(1 for b in sb if len(b) % N == 0) >= 2, N


def test_guard_check_reports_one_byte_either_side_of_a_slot():
    caps = caps_of([5, 300, 1, 4096, 77, 64, 33])
    lay = Layout(caps, what=[("size", c) for c in caps])
    assert [int(o) % 16 for o in lay.offs] == [i % 16 for i in range(len(caps))]
    gaps = lay.offs[1:] - (lay.offs[:-1] + lay.caps[:-1])
    assert all(GAPS[(i + 1) % 5] <= g < GAPS[(i + 1) % 5] + 16 for i, g in enumerate(gaps)), gaps
    assert lay.offs[0] >= GUARD and lay.size - (lay.offs[-1] + lay.caps[-1]) >= GUARD
    arena = lay.pattern.copy()
    assert lay.stray_writes(arena) is None
    for k in range(len(caps)):
        inside = arena.copy()
        inside[lay.offs[k]:lay.offs[k] + caps[k]] ^= 0xff                    # a slot is its owner's, all of it
        assert lay.stray_writes(inside) is None
        before = arena.copy()
        before[lay.offs[k] - 1] ^= 0x01
        msg = lay.stray_writes(before)
        assert msg and "first at %d," % (lay.offs[k] - 1) in msg and "signed distance -1" in msg and "nearest block %d " % k in msg, msg
        after = arena.copy()
        after[lay.offs[k] + caps[k]] = 0 if after[lay.offs[k] + caps[k]] else 1   # a zero store is a store
        msg = lay.stray_writes(after)
        assert msg and "first at %d," % (lay.offs[k] + caps[k]) in msg and "signed distance +1" in msg, msg
    # a copy of the pattern itself that landed shifted is seen too: the pattern depends on the position
    shifted = arena.copy()
    shifted[40:80] = arena[140:180]
    assert lay.stray_writes(shifted)


# ---- GPU ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


class _Guarded:
    """Blocks in a device arena the way a caller of the *_dev entry points holds them, the output slots laid out by
    Layout in an arena filled with the pattern; both arenas are checked as a whole after a call."""

    def __init__(self, dev, blocks, caps, what):
        import torch
        self.torch, self.dev, self.n = torch, dev, len(blocks)
        self.blocks = [bytes(b) for b in blocks]
        sizes = [len(b) for b in self.blocks]
        self.inl = Layout(sizes)                                            # the inputs lie as awkwardly as the outputs
        arena = self.inl.pattern.copy()
        for b, off in zip(self.blocks, self.inl.offs):
            arena[off:off + len(b)] = np.frombuffer(b, dtype=np.uint8)
        self.in_host = arena
        self.lay = Layout(caps, what)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.d_in, self.in_off, self.in_size = t(arena), t(self.inl.offs), t(np.array(sizes, dtype=np.int32))
        self.out_off, self.out_cap = t(self.lay.offs), t(self.lay.caps.astype(np.int32))
        self.max_in, self.total_in = max(sizes), sum(sizes)
        self.max_cap, self.total_cap = int(self.lay.caps.max()), int(self.lay.caps.sum())
        self.fresh()

    def fresh(self):
        torch = self.torch
        self.d_out = torch.from_numpy(self.lay.pattern).to(self.dev)
        self.out_size = torch.full((self.n,), -3, dtype=torch.int32, device=self.dev)
        self.status = torch.full((self.n,), -3, dtype=torch.int32, device=self.dev)
        self.chosen = torch.full((self.n,), -3, dtype=torch.int32, device=self.dev)

    def args(self):
        return (self.d_in, self.in_off, self.in_size, self.d_out, self.out_off, self.out_cap, self.out_size, self.status)

    def ptrs(self):
        return tuple(x.data_ptr() for x in self.args())

    def results(self, label):
        """(statuses, sizes, bytes per slot) once nothing was written outside the slots and the inputs are intact."""
        self.torch.cuda.synchronize()
        out = self.d_out.cpu().numpy()
        stray = self.lay.stray_writes(out)
        assert stray is None, "%s: %s" % (label, stray)
        assert np.array_equal(self.d_in.cpu().numpy(), self.in_host), "%s: the input arena was written to" % (label,)
        st, osz = self.status.cpu().numpy(), self.out_size.cpu().numpy()
        assert (osz >= 0).all() and (osz <= self.lay.caps).all(), (label, osz.tolist())
        return st, osz, self.lay.take(out, osz)


def _expect(label, G, st, osz, got, want, failing=()):
    bad = []
    for i in range(G.n):
        if i in failing:
            if st[i] != 1 or osz[i] != 0:
                bad.append((i, G.lay.what[i], "expected CAPACITY", int(st[i]), int(osz[i])))
        elif st[i] != 0 or got[i] != want[i]:
            bad.append((i, G.lay.what[i], int(st[i]), int(osz[i]), len(want[i])))
    assert not bad, (label, bad[:10])


def _what(blocks, orders):
    return [("order", o, "size", len(b)) for b, o in zip(blocks, orders)]


@pytest.mark.gpu
@pytest.mark.parametrize("back", [0, 99999], ids=["one-wave", "workgroup"])
@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "rows"])
def test_uncompress_dev_writes_only_inside_its_slots(H, oracle, opts, direct, back):
    """rans4x16_hip_uncompress_dev and _dev_sized over the oracle's streams of the corpus, capacities of exactly the
    stored size: both expansion kernels, with the short-step rows and without."""
    opts.set("dec_direct", direct)
    opts.set("back_wg_per_cu", back)
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    blocks, orders = zip(*corpus())
    comps = streams(oracle, "corpus", blocks, orders)
    G = _Guarded(dc.dev, comps, dec_caps(blocks, comps), _what(blocks, orders))
    for sized in (True, False):
        G.fresh()
        dc.route_read("expand"), dc.route_read("decode")
        if sized:
            dc.uncompress(*G.args(), G.max_in, G.max_cap, total_out_cap=G.total_cap)
        else:
            rc = dc.L.rans4x16_hip_uncompress_dev(dc.ctx.h, G.n, *G.ptrs(), G.max_in, G.max_cap, dc._stream())
            assert rc == 0, dc.ctx.error()
        st, osz, got = G.results(("decode", "sized" if sized else "plain", direct, back))
        _expect(("decode", sized), G, st, osz, got, blocks)
        exp, rows = dc.route_read("expand"), dc.route_read("decode")
        assert (exp["wave"] > 0 and exp["workgroup"] == 0) if back == 0 else (exp["workgroup"] > 0 and exp["wave"] == 0), exp
        assert (rows["direct"] > 0) if direct else (rows["direct"] == 0 and sum(rows.values()) > 0), rows


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [1, 0], ids=["records", "rows"])
def test_compress_dev_writes_only_inside_its_slots(H, oracle, opts, direct):
    """rans4x16_hip_compress_dev and _dev_sized, per-block orders and one order for all, capacities of exactly the bound;
    one block in seven has a third of it, reports CAPACITY with size 0 and leaves its surroundings alone too."""
    import torch
    opts.set("enc_direct", direct)
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    blocks, orders = (list(x) for x in zip(*corpus()))
    for k, o in enumerate(ORDERS):                                          # empty blocks: a header and nothing else
        blocks.append(b""); orders.append(o)
    small = set(range(3, len(blocks), 7))

    def run(label, order_of, d_order, order, sized):
        bounds = [H.rans_compress_bound_4x16(len(b), order_of(i)) for i, b in enumerate(blocks)]
        caps = caps_of(bounds)
        for i in small:
            caps[i] = bounds[i] // 3
        G = _Guarded(dc.dev, blocks, caps, _what(blocks, [order_of(i) for i in range(len(blocks))]))
        dc.route_read("encode")
        if sized:
            dc.compress(*G.args(), order, G.max_in, d_order=d_order, total_in_size=G.total_in)
        else:
            rc = dc.L.rans4x16_hip_compress_dev(dc.ctx.h, G.n, *G.ptrs(), order, d_order.data_ptr() if d_order is not None else None,
                                                G.max_in, dc._stream())
            assert rc == 0, dc.ctx.error()
        st, osz, got = G.results(label)
        want = streams(oracle, label[:2], blocks, [order_of(i) for i in range(len(blocks))])
        _expect(label, G, st, osz, got, want, failing=small)
        enc = dc.route_read("encode")
        assert (enc["records"] > 0) if direct else (enc["records"] == 0 and enc["u16"] + enc["packed"] > 0), (label, enc)

    d_order = torch.tensor(orders, dtype=torch.int32, device=dc.dev)
    run(("encode", "per-block", "sized"), lambda i: orders[i], d_order, 0, True)
    run(("encode", "per-block", "plain"), lambda i: orders[i], d_order, 0, False)
    for one in (1, 193, 0xd1):
        run(("encode", one, "sized"), lambda i: one, None, one, True)
    run(("encode", 64, "plain"), lambda i: 64, None, 64, False)


@pytest.mark.gpu
@pytest.mark.parametrize("method", STRIPE_METHODS, ids=lambda m: "%#x" % m)
def test_stripe_dev_calls_write_only_inside_their_slots(H, oracle, method):
    """X_STRIPE device-resident: encode with one order, encode under per-block orders (rans4x16_hip_set_dev_stripe_encode),
    decode (rans4x16_hip_set_dev_stripe_planes) with two ordinary blocks in the batch; sizes that are no multiple of N and
    the sizes on either side of where the flag is dropped."""
    import torch
    dc = H.DeviceCodec(0)
    blocks = stripe_blocks()
    N = (method >> 8) or 4
    want = streams(oracle, ("stripe", method), blocks, [method] * len(blocks))
    try:
        G = _Guarded(dc.dev, blocks, caps_of([H.rans_compress_bound_4x16(len(b), method) for b in blocks]), _what(blocks, [method] * len(blocks)))
        dc.compress(*G.args(), method, G.max_in)
        st, osz, got = G.results(("stripe encode", method))
        _expect(("stripe encode", method), G, st, osz, got, want)
        # per-block orders: the stripe method on two blocks in three, plain flag sets on the others
        orders = [method if i % 3 else (1, 193, 64)[(i // 3) % 3] for i in range(len(blocks))]
        wanto = streams(oracle, ("stripe orders", method), blocks, orders)
        dc.set_stripe_encode(7)
        G = _Guarded(dc.dev, blocks, caps_of([H.rans_compress_bound_4x16(len(b), o) for b, o in zip(blocks, orders)]), _what(blocks, orders))
        dc.compress(*G.args(), 0, G.max_in, d_order=torch.tensor(orders, dtype=torch.int32, device=dc.dev), total_in_size=G.total_in)
        st, osz, got = G.results(("stripe encode under d_order", method))
        _expect(("stripe encode under d_order", method), G, st, osz, got, wanto)
        # decode: a stripe block's capacity is its stored size (:1379); the ordinary ones get 37 bytes more now and then
        plains = list(blocks) + [blocks[12], blocks[18]]
        comps = list(want) + [oracle.compress(blocks[12], 1), oracle.compress(blocks[18], 193)]
        caps = dec_caps(plains, comps)
        assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, N, max(len(p) for p in plains)) == 0
        G = _Guarded(dc.dev, comps, caps, _what(plains, [c[0] for c in comps]))
        dc.uncompress(*G.args(), G.max_in, G.max_cap)
        st, osz, got = G.results(("stripe decode", method))
        _expect(("stripe decode", method), G, st, osz, got, plains)
    finally:
        dc.set_stripe_encode(0)
        assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 0, 0) == 0


def _best_blocks():
    blocks = stripe_blocks() + [b for b, _ in corpus()[::5]]
    return blocks


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["nine", "stripes"])
def test_compress_best_dev_writes_only_inside_its_slots(H, oracle, table):
    from test_gpu_best_dev import NINE, reference_loop
    methods = NINE if table == "nine" else [(3 << 8) | 8, 8]
    dc = H.DeviceCodec(0)
    blocks = _best_blocks()
    caps = caps_of([max(H.rans_compress_bound_4x16(len(b), m) for m in methods) for b in blocks])
    want = reference_loop(oracle, "confinement", blocks, methods)
    G = _Guarded(dc.dev, blocks, caps, [("size", len(b)) for b in blocks])
    dc.compress_best(*G.args(), methods, G.max_in, chosen=G.chosen, total_in_size=G.total_in)
    st, osz, got = G.results(("best", table))
    chosen = G.chosen.cpu().numpy()
    bad = []
    for i, (c, m, _) in enumerate(want):
        if c is None:                                                       # only stripe methods, and a size that is no multiple of four
            ok = st[i] != 0 and osz[i] == 0 and chosen[i] == -1
        else:
            ok = st[i] == 0 and chosen[i] == m and got[i] == c
        if not ok:
            bad.append((i, len(blocks[i]), int(st[i]), int(chosen[i]), m))
    assert not bad, bad[:10]
    assert (table == "nine") == all(w[0] is not None for w in want)


@pytest.mark.gpu
def test_device_resident_4x8_writes_only_inside_its_slots(H, oracle):
    """The sibling of test_device_resident_4x8 (test_gpu_4x8.py): rans4x8_hip_{compress,uncompress}_dev with edge sizes,
    slots at every alignment a few bytes apart, capacities of exactly the bound / the stored size, orders 0 and 1 per
    block, and one undersized slot each way (CAPACITY, size 0)."""
    import torch
    from test_oracle4x8 import Codec8
    orc8 = Codec8(oracle.lib, "orc8_")
    dc = H.DeviceCodec(0)
    L = dc.L
    blocks, orders = [], []
    for si, n in enumerate(SIZES):
        for ai, alph in enumerate((("rand", 4), ("runs",), ("q40+dir",))):
            blocks.append(np.ascontiguousarray(_data(alph, n, 3 * si + ai + 1)).tobytes())
            orders.append((si + ai) & 1)
    want = [orc8.compress(b, o) for b, o in zip(blocks, orders)]
    d_order = torch.tensor(orders, dtype=torch.int32, device=dc.dev)
    small = len(blocks) // 2
    caps = caps_of([L.rans4x8_hip_compress_bound(len(b)) for b in blocks])
    caps[small] //= 3
    G = _Guarded(dc.dev, blocks, caps, _what(blocks, orders))
    rc = L.rans4x8_hip_compress_dev(dc.ctx.h, G.n, *G.ptrs(), 0, d_order.data_ptr(), G.max_in, dc._stream())
    assert rc == 0, dc.ctx.error()
    st, osz, got = G.results("4x8 encode")
    _expect("4x8 encode", G, st, osz, got, want, failing={small})
    caps = caps_of([len(b) for b in blocks])
    caps[small] = len(blocks[small]) - 1
    G = _Guarded(dc.dev, want, caps, _what(blocks, orders))
    rc = L.rans4x8_hip_uncompress_dev(dc.ctx.h, G.n, *G.ptrs(), dc._stream())
    assert rc == 0, dc.ctx.error()
    st, osz, got = G.results("4x8 decode")
    _expect("4x8 decode", G, st, osz, got, blocks, failing={small})


def _host_call(H, fn_name, srcs, lay, arena, orders=None):
    """rans4x16_hip_{compress,uncompress}_batch through ctypes with every output buffer cut from `arena` at lay.offs."""
    from htscodecs_amd import codec
    L = H.load()
    ctx = codec._thread_ctx()
    n = len(srcs)
    keep = [np.frombuffer(s, dtype=np.uint8) for s in srcs]
    dummy = np.zeros(1, dtype=np.uint8)
    in_p = (C.c_void_p * n)(*[(s.ctypes.data if len(s) else dummy.ctypes.data) for s in keep])
    out_p = (C.c_void_p * n)(*[arena.ctypes.data + int(o) for o in lay.offs])
    in_sz = (C.c_uint * n)(*[len(s) for s in keep])
    out_sz = (C.c_uint * n)(*[int(c) for c in lay.caps])
    status = (C.c_int * n)()
    if orders is None:
        rc = getattr(L, fn_name)(ctx.h, n, in_p, in_sz, out_p, out_sz, status)
    else:
        rc = getattr(L, fn_name)(ctx.h, n, in_p, in_sz, out_p, out_sz, (C.c_int * n)(*orders), status)
    assert rc >= 0, ctx.error()
    return rc, np.array(status[:]), np.array(out_sz[:])


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [1, 0], ids=["packed", "slot-by-slot"])
@pytest.mark.parametrize("route", ["single-pass", "pipelined"])
def test_host_batches_write_only_inside_the_callers_buffers(H, oracle, opts, route, pack):
    """rans4x16_hip_{compress,uncompress}_batch with every output buffer cut from one host array filled with the pattern:
    single-pass and through the pipeline (slabs on three lanes), results gathered on the device or copied slot by slot;
    stripe blocks among them; undersized slots on encode."""
    if route == "pipelined":
        opts.set("host_pipe_mb", 1); opts.set("host_slab_min_mb", 1); opts.set("host_lanes", 3)
    else:
        opts.set("host_pipe_mb", 0)
    opts.set("host_pack", pack)
    blocks, orders = (list(x) for x in zip(*corpus()))
    for k, b in enumerate(stripe_blocks()):
        blocks.append(b); orders.append(STRIPE_METHODS[k % len(STRIPE_METHODS)])
    want = streams(oracle, "host", blocks, orders)
    small = set(range(3, len(blocks), 7))
    bounds = [H.rans_compress_bound_4x16(len(b), o) for b, o in zip(blocks, orders)]
    caps = caps_of(bounds)
    for i in small:
        caps[i] = max(bounds[i] // 3, 1)
    lay = Layout(caps, _what(blocks, orders))
    arena = lay.pattern.copy()
    rc, st, osz = _host_call(H, "rans4x16_hip_compress_batch", blocks, lay, arena, orders)
    stray = lay.stray_writes(arena)
    assert stray is None, ("host encode", route, pack, stray)
    got = lay.take(arena, osz)
    bad = [(i, lay.what[i], int(st[i]), int(osz[i])) for i in range(len(blocks))
           if ((st[i] == 0 or osz[i] != 0) if i in small else (st[i] != 0 or got[i] != want[i]))]
    assert not bad and rc == len(small), (rc, bad[:10])
    # decode: capacities of exactly the stored size (a stripe block's must be that, :1379)
    caps = dec_caps(blocks, want)
    lay = Layout(caps, _what(blocks, orders))
    arena = lay.pattern.copy()
    rc, st, osz = _host_call(H, "rans4x16_hip_uncompress_batch", want, lay, arena)
    stray = lay.stray_writes(arena)
    assert stray is None, ("host decode", route, pack, stray)
    got = lay.take(arena, osz)
    bad = [(i, lay.what[i], int(st[i]), int(osz[i])) for i in range(len(blocks)) if st[i] != 0 or got[i] != blocks[i]]
    assert not bad and rc == 0, (rc, bad[:10])


@pytest.mark.gpu
def test_drop_in_symbols_write_only_inside_the_callers_buffer(H, oracle):
    """rans_compress_to_4x16 / rans_uncompress_to_4x16 with a caller buffer of exactly the bound / the stored size, cut
    from a guarded array at an odd offset."""
    L = H.load()
    picks = corpus()[3::17] + [(b, STRIPE_METHODS[k % len(STRIPE_METHODS)]) for k, b in enumerate(stripe_blocks())][::3]
    for k, (b, o) in enumerate(picks):
        want = oracle.compress(b, o)
        src = np.frombuffer(b, dtype=np.uint8)
        lay = Layout([0] * (k % 16) + [H.rans_compress_bound_4x16(len(b), o)], None)
        arena = lay.pattern.copy()
        n = C.c_uint(int(lay.caps[-1]))
        r = L.rans_compress_to_4x16(src.ctypes.data, len(src), arena.ctypes.data + int(lay.offs[-1]), C.byref(n), o)
        assert r == arena.ctypes.data + int(lay.offs[-1]), (k, o, len(b))
        assert lay.stray_writes(arena) is None, ("rans_compress_to_4x16", o, len(b), lay.stray_writes(arena))
        assert arena[lay.offs[-1]:lay.offs[-1] + n.value].tobytes() == want, (k, o, len(b))
        comp = np.frombuffer(want, dtype=np.uint8)
        lay = Layout([0] * (k % 16) + [len(b)], None)
        arena = lay.pattern.copy()
        n = C.c_uint(len(b))
        r = L.rans_uncompress_to_4x16(comp.ctypes.data, len(comp), arena.ctypes.data + int(lay.offs[-1]), C.byref(n))
        assert r == arena.ctypes.data + int(lay.offs[-1]) and n.value == len(b), (k, o, len(b))
        assert lay.stray_writes(arena) is None, ("rans_uncompress_to_4x16", o, len(b), lay.stray_writes(arena))
        assert arena[lay.offs[-1]:lay.offs[-1] + len(b)].tobytes() == b, (k, o, len(b))
