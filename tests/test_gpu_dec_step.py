"""The step of the decode chain (htscodecs_amd/csrc/r4x16_decode.hip: chain_decode_lds, chain_decode_dir, chain_decode_mid and
the global-memory chain_decode behind k_dec_chain) by row kind, length, ring alignment and wave mix:
rans4x16_hip_uncompress_dev_sized over streams that the CPU oracle made, compared byte for byte with the RAW INPUT - the
oracle only produces the streams, expected bytes never come from the code under test.  The sibling of
test_gpu_enc_step.py for the other direction.

What decides a decoded block's last bytes:
  * the per-chain count.  Order 1: q = n >> 2 per chain, chain 3 takes n & 3 more; order 0: (n + 3 - k) >> 2.  Order 1
    queues a dword every 4 steps and stores 16 bytes every 16 steps; the epilogue writes nd = (min(count, t - 4) >> 2) & 3
    queued dwords and rem = count - 4 * pushed (0 .. 4) bytes, with a case of its own for count == t.  The lengths
    BASE + 0 .. 63 hold every q mod 16 with every n & 3;
  * FAST against slow trips: a trip is FAST only if every stream of the wave has a whole trip of steps and of words
    left, so the lengths run side by side in one wave (shortest first, unsorted; sorted; with a last wave that has
    quads without a stream), alone (every other lane idle), and beside long streams;
  * the word ring: off0 = words & 15 shifts every ring read and every quarter crossing - the same stream is laid at 16
    consecutive byte offsets of the input arena;
  * the row kind: every route kind of the read-out (l1 .. l5, direct, mid, short_ring), orders 0 and 1, the all-affine
    body of the direct rows, and option dec_short_ring = 1 (k_dec_chain<true, 1, 4>: four-step trips over a ring of
    two quarters);
  * rANS 4x8, which runs on the same loop (BYTE = true) with its own end-of-stream arithmetic.

Every case asserts the route it took (option route_count, rans4x16_hip_route_read).  The route cannot tell whether an
image was decoded from LDS or from global memory: the order-1 image of 256 symbols has 256 rows of at least 256 bytes
and so exceeds the largest LDS class of its depth (DEC_CLASSES: {163840, 1, 4}) - it goes to the catch-all
k_dec_chain<false, 4> and is counted as l4; the order-1 images of 151 symbols and all order-0 images fit a class.

Every decode goes into an output arena filled with the pattern of test_gpu_confinement.py, the slots at odd offsets 1 to 3
bytes apart with capacities of exactly the block sizes: the order-1 loops write unaligned 16-byte vectors at
out + k * q, and an overshoot into the neighbour or a quarter that starts a dword late is reported by (case, n, offset).

The CPU test at the end pins that the cases are what they claim: entropy-coded with the order asked for (a stored block
never reaches the chain and would pass silently), the alphabet size and the table precision the case names, the
lengths' coverage of the epilogue, all 16 ring alignments, nwords < 16 at the short end."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_confinement import GUARD, Layout, _varint, pattern
from test_gpu_enc_step import table_bits, takes_packed

RANS_LOW = 1 << 15
ST_CONTEXT = 7                              # include/rans4x16_hip.h
ROUTES = ("l1", "l2", "l3", "l4", "l5", "direct", "mid", "short_ring")
ALONE = (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 63)
LONG = (20000, 33333, 65539)
CUTS = (2, 4, 30, 32)


# ---- generators --------------------------------------------------------------------------------------------------
def alphabet(nsym, order, shape="lo"):
    """The byte values of an alphabet that the decoder counts as `nsym` symbols: every order-1 alphabet lists byte 0,
    so an order-1 case has nsym - 1 byte values without byte 0.  shape "lo": contiguous from a byte above 0 (affine,
    byte = index + c with c > 0); "c0": contiguous from byte 0 or 1 (affine, c = 0); "gaps": not affine."""
    k = nsym - 1 if order else nsym
    if shape == "c0":
        return np.arange(k, dtype=np.uint8) + (1 if order else 0)
    lo = min(33, 256 - k)
    if shape == "lo":
        return (np.arange(k) + lo).astype(np.uint8)
    lo = min(33, 256 - k - 5)
    return (np.arange(k) + lo + np.where(np.arange(k) >= (k + 1) // 2, 5, 0)).astype(np.uint8)


def skewed(n, a, seed, p=0.9):
    """One dominant symbol at about p, the rest uniform, every symbol once at the front."""
    rng = np.random.default_rng(seed)
    w = np.full(len(a), (1 - p) / max(len(a) - 1, 1))
    w[0] = p if len(a) > 1 else 1.0
    out = a[rng.choice(len(a), size=n, p=w)]
    m = min(n, len(a))
    out[:m] = a[:m]
    return out.tobytes()


def uniform(n, a, seed):
    """Uniform draws, every symbol once at the front: nearly every step renormalises."""
    rng = np.random.default_rng(seed)
    out = a[rng.integers(0, len(a), size=n)]
    m = min(n, len(a))
    out[:m] = a[:m]
    return out.tobytes()


def cyclic(n, a):
    """Each symbol followed by the same next one: order-1 contexts of a single symbol, (next to) no words."""
    return np.resize(a, n).tobytes()


def rare(n, a):
    """One symbol, and at every 20th place the others in turn: what makes compute_shift take 12 bits at a few KB - many
    symbols of a context at 1.86 / 1024 of its total, which 10 bits round down to 1 / 1024."""
    out = np.full(n, a[0], dtype=np.uint8)
    at = np.arange(0, n, 20)
    out[at] = a[1 + np.arange(len(at)) % (len(a) - 1)]
    return out.tobytes()



Case = collections.namedtuple("Case", "route order nsym gen bits shape base p")


# image sizes as r4x16_common.h has them (img_alpha_bytes, dir_img_bytes, mid_img_bytes, pk_img_bytes up to 48 symbols)
def _alpha_bytes(n):
    return (2 * n + 15) & ~15


def dir_img_bytes(n, rows, look):
    return _alpha_bytes(n) + rows * (4 * (n + 1) + (1 << (look - 1)))


def mid_img_bytes(n):
    return _alpha_bytes(n) + n * (64 + 2 * ((n + 10) & ~1))


def pk_img_bytes(n):
    return ((8 * n + 15) & ~15) + n * (16 * ((n + 11) // 12) + (0 if n % 12 else 16))


RING_BYTES, RING_BYTES_SHORT = 272, 136                  # r4x16_decode.hip


def short_step_min_len(route, order, nsym, bits):
    """The shortest block that the front end gives direct rows (order-0 tables are 12-bit, one row) or mid rows."""
    if route == "direct":
        return dir_img_bytes(nsym, nsym if order else 1, bits if order else 12) // 4
    return mid_img_bytes(nsym) // 4 if route == "mid" else 0


def takes_short_ring(nsym):
    """k_dec_classify: the image needs more than the class of sixteen with the long ring and fits it with the short one."""
    return pk_img_bytes(nsym) + RING_BYTES > 3344 and pk_img_bytes(nsym) + RING_BYTES_SHORT <= 3360


def case(route, order, nsym, gen="skewed", bits=None, shape="lo", base=None, p=0.9):
    """bits: the table precision of an order-1 stream (10 unless the case says 12).  BASE: the smallest power of two from
    which the oracle alone entropy-codes the case - skewed data 2,048 up to 151 symbols and 4,096 at 256, uniform data
    4,096; a 12-bit table needs a context of more than 4,096 symbols (compute_shift halves its total twice): 8,192."""
    bits = bits or (10 if order else None)
    if base is None:
        base = 8192 if bits == 12 else 4096 if (gen == "uniform" or nsym > 151) else 2048
        # the front end gives the direct and the mid rows only to streams of a step per 16 bytes of image at least
        # (o1_tables, o0_front): the next power of two from which all 64 lengths have one
        while base < short_step_min_len(route, order, nsym, bits):
            base *= 2
    return Case(route, order, nsym, gen, bits, shape, base, p)


def cid(c):
    return "%s-o%d-%dsym-%s-%s%s" % (c.route, c.order, c.nsym, c.gen, c.shape, "-12bit" if c.bits == 12 else "")


@functools.lru_cache(maxsize=None)
def raw_of(c, n):
    a = alphabet(c.nsym, c.order, c.shape)
    if c.gen == "skewed":               # (long blocks: less skew, or the dominant context's total takes the table to 12 bits)
        return skewed(n, a, 100003 * c.nsym + 17 * n, c.p if n < 16384 else min(c.p, 0.7))
    if c.gen == "uniform":
        return uniform(n, a, 100003 * c.nsym + 17 * n)
    return {"cyclic": cyclic, "rare": rare}[c.gen](n, a)


@functools.lru_cache(maxsize=None)
def comp_of(c, n):
    import cpu_libs
    return cpu_libs.oracle().compress(raw_of(c, n), c.order)


def lengths(c):
    return [c.base + r for r in range(64)]


# The kinds and how each is reached.  Packed kinds (l1, l5, mid, short_ring) need 10-bit tables.
OPTS = {"l1": {"dec_direct": 0, "dec_mid": 0, "dec_short_ring": 0}, "short_ring": {"dec_direct": 0, "dec_mid": 0, "dec_short_ring": 1},
        "l5": {"dec_direct": 0, "dec_mid": 0}, "l2": {"dec_direct": 0, "dec_mid": 0}, "l3": {"dec_direct": 0, "dec_mid": 0},
        "l4": {"dec_direct": 0, "dec_mid": 0}, "direct": {"dec_direct": 1}, "mid": {"dec_direct": 0, "dec_mid": 1}}
TWELVE = dict(gen="rare", bits=12)            # a 12-bit order-1 table
KINDS = {
    "l1": [case("l1", 1, ns) for ns in (13, 36, 37, 46, 48)] + [case("l1", 1, 46, "uniform"), case("l1", 1, 46, "cyclic")],
    # dec_short_ring = 1: 43 and 44 symbols take the short ring (images of 3,104 and 3,168 bytes); 42 (3,024 + 272 <= 3,344:
    # the class of sixteen holds it with the long ring anyway) and 45, 46, 47 (3,248 bytes and more: image + 136 > 3,360 since
    # the 8-byte head entries of the packed rows) keep l1 and say so (k_dec_classify, takes_short_ring)
    "short_ring": [case("short_ring", 1, 43), case("short_ring", 1, 44), case("short_ring", 1, 44, "uniform"),
                   case("short_ring", 1, 44, "cyclic")] + [case("l1", 1, ns) for ns in (42, 45, 46, 47)],
    "l5": [case("l5", 1, 49), case("l5", 1, 96), case("l5", 1, 64, "uniform")],
    "l2": [case("l2", 0, ns) for ns in (3, 12, 50)] + [case("l2", 1, 3), case("l2", 1, 12), case("l2", 0, 50, "uniform"),
           case("l2", 1, 12, "cyclic"), case("l2", 1, 30, **TWELVE)],
    # (order 1 of 51 symbols with a 10-bit table has wide packed rows: l5; the u16 rows of depth 3 start at 97 there)
    "l3": [case("l3", 0, ns) for ns in (51, 97, 150)] + [case("l3", 1, ns) for ns in (97, 150)] + [case("l3", 0, 64, "uniform")],
    "l4": [case("l4", o, ns) for o in (0, 1) for ns in (151, 256)],
    "direct": [case("direct", o, ns, shape=sh) for o in (0, 1) for ns in (3, 46, 128) for sh in ("lo", "gaps")] +
              [case("direct", 1, 46, "uniform"), case("direct", 1, 46, "cyclic"), case("direct", 0, 46, "uniform"),
               case("direct", 1, 30, **TWELVE)],
    "mid": [case("mid", 1, 13), case("mid", 1, 47), case("mid", 1, 46, "uniform"), case("mid", 1, 46, "cyclic")],
}
SHORT = [case("l2", o, 3, gen, base=0) for o in (0, 1) for gen in ("skewed", "cyclic")]      # the short end: see short_lengths


def expected_route(c, o, n):
    """The route of an n-byte stream of case `c` under the options `o`: _expected_level of test_gpu_routes.py for 10-bit
    order-1 tables; order-0 streams and 12-bit tables have u16 rows (never packed, never mid), by the depth of the
    alphabet.  A stream too short for the direct or the mid rows (short_step_min_len) takes what it takes without them."""
    direct = o.get("dec_direct", 1) and n >= short_step_min_len("direct", c.order, c.nsym, c.bits)
    mid, short = o.get("dec_mid", 0) and n >= short_step_min_len("mid", c.order, c.nsym, c.bits), o.get("dec_short_ring", 0)
    if c.order == 1 and c.bits == 10:
        from test_gpu_routes import _expected_level
        lv = _expected_level(c.nsym, direct, mid)
        return "short_ring" if lv == "l1" and short and takes_short_ring(c.nsym) else lv
    if direct and c.nsym <= 128:
        return "direct"
    return "l2" if c.nsym <= 50 else "l3" if c.nsym <= 150 else "l4"


# ---- what a stream holds (numpy and the oracle only) -------------------------------------------------------------
def _alphabet_of(s, pos):
    """The alphabet of a table (rANS_static4x16pr.c:208-255, well-formed streams): (symbols, position behind it)."""
    syms, implicit = [], 0
    j = s[pos]
    pos += 1
    while True:
        syms.append(j)
        if not implicit and j + 1 == s[pos]:
            j, implicit = s[pos], s[pos + 1]
            pos += 2
        elif implicit:
            implicit -= 1
            j += 1
        else:
            j = s[pos]
            pos += 1
        if j == 0:
            return syms, pos


def _o1_table(s, pos):
    syms, pos = _alphabet_of(s, pos)
    for _ in syms:                                          # a row per context: a varint per symbol, a zero is a run
        zeros = 0
        for _ in syms:
            if zeros:
                zeros -= 1
                continue
            f, pos = _varint(s, pos)
            if f == 0:
                zeros = s[pos]
                pos += 1
    return syms, pos


Info = collections.namedtuple("Info", "coded order nsym bits nested words nwords")


@functools.lru_cache(maxsize=None)
def stream_info(s):
    """coded: no X_CAT and no transform; order; the decoder's nsym; table bits (order 1); nested: the order-1 table is itself
    an order-0 stream (a chain item of its own); words: offset of the first renormalisation word; nwords."""
    import cpu_libs
    flags = s[0]
    if flags & 0xfc:                                        # X_CAT, X_PACK, X_RLE, X_NOSZ, X_STRIPE
        return Info(False, flags & 1, 0, None, False, 0, 0)
    _, pos = _varint(s, 1)
    bits, nested = None, False
    if flags & 1:
        bits, nested = s[pos] >> 4, bool(s[pos] & 1)
        pos += 1
        if nested:
            usz, pos = _varint(s, pos)
            csz, pos = _varint(s, pos)
            src = np.frombuffer(s[pos:pos + csz], dtype=np.uint8)
            tab = np.zeros(usz + 16, dtype=np.uint8)
            lib = cpu_libs.oracle().lib
            lib.orc_o0_decode.restype = C.c_int
            lib.orc_o0_decode.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
            assert lib.orc_o0_decode(src.ctypes.data, csz, tab.ctypes.data, usz) == 0
            syms, used = _o1_table(tab.tobytes(), 0)
            assert used == usz, (used, usz)
            pos += csz
        else:
            syms, pos = _o1_table(s, pos)
    else:
        syms, pos = _alphabet_of(s, pos)
        for _ in syms:
            _, pos = _varint(s, pos)
    states = np.frombuffer(s[pos:pos + 16], dtype="<u4")
    assert len(states) == 4 and (states >= RANS_LOW).all(), "the table parse lost its place"
    return Info(True, flags & 1, len(syms), bits, nested, pos + 16, (len(s) - pos - 16) >> 1)


def epilogue(n, k, order, trip, t=None):
    """(count, nd, rem, count == t) of chain k of an n-byte stream, t: the steps its wave ran (alone: its own)."""
    q = n >> 2
    counts = [q, q, q, q + (n & 3)] if order else [(n + 3 - j) >> 2 for j in range(4)]
    if t is None:
        t = (max(counts) + trip - 1) // trip * trip
    count = counts[k]
    pushed = min(count, t - 4) >> 2 if t >= 4 else 0
    return count, pushed & 3, count - 4 * pushed, count == t


@functools.lru_cache(maxsize=None)
def short_lengths(c):
    """The short end of a 3-symbol case: every n from the smallest length the oracle entropy-codes with the order asked
    for, to that length plus 64 (counts below one trip, where t - 4 meets count; nwords below 16: every trip slow)."""
    for n0 in range(4, 257):
        i = stream_info(comp_of(c, n0))
        if i.coded and i.order == c.order:
            return list(range(n0, n0 + 65))
    raise AssertionError("the oracle never entropy-codes %s below 257 bytes" % cid(c))


# ---- the arenas ---------------------------------------------------------------------------------------------------
class Slots(Layout):
    """Output slots of exactly the block sizes at odd offsets, 1 to 3 bytes behind their predecessors, GUARD bytes around."""

    def __init__(self, caps, what):
        self.caps = np.asarray(caps, dtype=np.int64)
        offs, pos = [], GUARD + 1
        for i, c in enumerate(self.caps):
            if i:
                pos += 2 if pos & 1 else (1, 3)[i & 1]
            offs.append(pos)
            pos += int(c)
        self.offs = np.array(offs, dtype=np.int64)
        self.size = pos + GUARD
        self.what = what
        mask = np.zeros(self.size, dtype=bool)
        for o, c in zip(self.offs, self.caps):
            mask[o:o + c] = True
        self.mask = mask
        self.pattern = pattern(self.size)


def in_layout(comps, shifts=None):
    """Input offsets: stream i starts `shifts[i]` bytes (default 5 i mod 16) behind a 256-byte boundary."""
    offs, pos = [], 256
    for i, c in enumerate(comps):
        offs.append(pos + (5 * i % 16 if shifts is None else shifts[i]))
        pos = (offs[-1] + len(c) + 511) // 256 * 256
    return np.array(offs, dtype=np.int64), pos + 256


@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


def device(H, opts, options):
    for k, v in options.items():
        opts.set(k, v)
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    return dc


def decode(dc, comps, sizes, what, shifts=None, codec8=False):
    """One device-resident call: (statuses, sizes, bytes per slot, route read-out, address of the input arena) once no
    byte outside the slots has changed."""
    import torch
    in_off, total = in_layout(comps, shifts)
    arena = pattern(total)
    for c, off in zip(comps, in_off):
        arena[off:off + len(c)] = np.frombuffer(c, dtype=np.uint8)
    lay = Slots(sizes, what)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dc.dev)
    d_in, d_in_off, d_csz = t(arena), t(in_off), t(np.array([len(c) for c in comps], dtype=np.int32))
    d_out, d_out_off, d_cap = t(lay.pattern), t(lay.offs), t(lay.caps.astype(np.int32))
    d_osz, d_st = (torch.full((len(comps),), -3, dtype=torch.int32, device=dc.dev) for _ in range(2))
    assert d_in.data_ptr() % 16 == 0
    if codec8:
        rc = dc.L.rans4x8_hip_uncompress_dev(dc.ctx.h, len(comps), d_in.data_ptr(), d_in_off.data_ptr(), d_csz.data_ptr(),
                                             d_out.data_ptr(), d_out_off.data_ptr(), d_cap.data_ptr(), d_osz.data_ptr(),
                                             d_st.data_ptr(), dc._stream())
        assert rc == 0, dc.ctx.error()
        route = None
    else:
        dc.route_read("decode")
        dc.uncompress(d_in, d_in_off, d_csz, d_out, d_out_off, d_cap, d_osz, d_st, max(len(c) for c in comps), max(sizes),
                      total_out_cap=sum(sizes))
    torch.cuda.synchronize()
    if not codec8:
        route = dc.route_read("decode")
    out = d_out.cpu().numpy()
    stray = lay.stray_writes(out)
    assert stray is None, stray
    assert np.array_equal(d_in.cpu().numpy(), arena), "the input arena was written to"
    st, osz = d_st.tolist(), d_osz.tolist()
    return st, osz, lay.take(out, lay.caps), route, in_off


def mismatches(what, st, osz, got, want, may_refuse=False):
    """[(what, n, status, size, first differing offset, differing bytes)] of the blocks that are not their raw input."""
    bad = []
    for w, s, z, g, r in zip(what, st, osz, got, want):
        if may_refuse and s == ST_CONTEXT:
            continue
        if s != 0 or z != len(r) or g != r:
            d = np.nonzero(np.frombuffer(g, dtype=np.uint8) != np.frombuffer(r, dtype=np.uint8))[0]
            bad.append((w, len(r), s, z, int(d[0]) if len(d) else None, len(d)))
    return bad


def check_route(route, want):
    """want: {kind: payload streams}, and no stream on any other kind.  The read-out is of the payload launch alone: an
    order-1 table that travels as an order-0 stream is decoded by a launch of the front end, which is not counted."""
    assert {k: route[k] for k in ROUTES} == {k: want.get(k, 0) for k in ROUTES}, (route, dict(want))


def run(dc, cases, ns, o, shifts=None, order=None):
    """The blocks (case, n) for every case and n, in one call; every block must come out as its raw input, on the route
    of its case.  order: a permutation of the blocks."""
    items = [(c, n) for c in cases for n in ns(c)] if callable(ns) else [(c, n) for c in cases for n in ns]
    if order is not None:
        items = [items[i] for i in order(len(items))]
    what = [(cid(c), n) for c, n in items]
    raws = [raw_of(c, n) for c, n in items]
    comps = [comp_of(c, n) for c, n in items]
    st, osz, got, route, _ = decode(dc, comps, [len(r) for r in raws], what, shifts)
    bad = mismatches(what, st, osz, got, raws)
    assert not bad, bad[:10]
    want = collections.Counter(expected_route(c, o, n) for c, n in items)
    check_route(route, want)
    return route


# ---- GPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_length_in_one_batch(H, opts, kind):
    """Per case of the kind, the 64 lengths in one call: shortest first and unsorted (sched_sort = 0: neighbouring lengths
    share a wave), with the default sort, and - unsorted again - 61 of them, which is no multiple of any class's streams
    per wave (16, 15, .. 2): the last wave has quads without a stream."""
    o = OPTS[kind]
    for sort in (0, 1):
        dc = device(H, opts, dict(o, sched_sort=sort))
        for c in KINDS[kind]:
            run(dc, [c], lengths, o)
            if sort == 0:
                run(dc, [c], lambda c: lengths(c)[:61], o)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["l2", "direct"])
def test_short_end_in_one_batch(H, opts, kind):
    """3 symbols, every n from the smallest the oracle entropy-codes to 64 more: counts below one trip, nwords below 16.
    Three symbols are l2 rows; blocks this short stay on them in a batch that is given direct rows too (a direct image of 3
    symbols wants 400 bytes of order-1 and 520 of order-0 data: short_step_min_len), so the second run is of the l2 loop
    beside the direct classes' launches, and its route is asserted as l2."""
    o = OPTS[kind]
    for sort in (0, 1):
        dc = device(H, opts, dict(o, sched_sort=sort))
        for c in SHORT:
            run(dc, [c], short_lengths, o)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_lengths_alone(H, opts, kind):
    """One block per call: one quad works and every other lane is idle."""
    o = OPTS[kind]
    dc = device(H, opts, o)
    for c in KINDS[kind]:
        for r in ALONE:
            run(dc, [c], [c.base + r], o)
    if kind in ("l2", "direct"):
        for c in SHORT:
            ns = short_lengths(c)
            for n in (ns[0], ns[1], ns[3], ns[4], ns[17], ns[64]):
                run(dc, [c], [n], o)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_short_stream_beside_long_ones(H, opts, kind):
    """A BASE-length block and a 3-symbol short block with blocks of 20,000, 33,333 and 65,539 bytes of the same case: lanes
    past their end beside lanes in FAST trips; the long blocks must come out whole.  The 3-symbol block sits in the same
    wave where the kind holds 3 symbols (l2, direct) and in a launch of its own otherwise.  Where the class holds one
    stream per wave (order 1 of l3 and l4, and the direct rows of 128 symbols) the mix tests the persistent walk instead:
    one workgroup after the other takes a stream of another length."""
    o = OPTS[kind]
    for sort in (0, 1):
        dc = device(H, opts, dict(o, sched_sort=sort))
        for c in cut_cases(kind):                          # (cyclic data: no words, no FAST trip)
            short = SHORT[2 * c.order]
            items = [(c, c.base), (short, short_lengths(short)[5])] + [(c, n) for n in LONG]
            what = [(cid(x), n) for x, n in items]
            raws = [raw_of(x, n) for x, n in items]
            comps = [comp_of(x, n) for x, n in items]
            assert all(stream_info(s).coded for s in comps), what
            st, osz, got, route, _ = decode(dc, comps, [len(r) for r in raws], what)
            bad = mismatches(what, st, osz, got, raws)
            assert not bad, bad
            want = collections.Counter(expected_route(x, o, n) for x, n in items)
            check_route(route, want)


def align_streams(kind):
    """[(case, n)] of the alignment test.  BASE + 37 bytes: the kind's first (skewed) case, its first uniform case (uniform
    data: up to 64 symbols; l4 has none) and, where the kind has both orders and starts with order 0, its first order-1
    case - for l4 both of them: 151 symbols decode from LDS, 256 from global memory (chain_decode, a ring and a mirror of
    its own).  65,539 bytes: the uniform case (the skewed one where there is none) and the same order-1 cases."""
    cs = KINDS[kind]
    un = [c for c in cs if c.gen == "uniform"][:1]
    o1 = [c for c in cs if c.order == 1 and c.gen == "skewed" and c.bits == 10]
    o1 = [] if cs[0].order == 1 else o1 if kind == "l4" else o1[:1]
    return [(c, c.base + 37) for c in [cs[0]] + un + o1] + [(c, 65539) for c in (un or [cs[0]]) + o1]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_ring_alignment(H, opts, kind):
    """Streams of BASE + 37 bytes, and of 65,539 (uniform where the kind has uniform data, order 1 where it has both
    orders: align_streams; their words cross a hundred quarters and more and wrap the ring: the slot == 0 mirror is
    written many times), each at 16 consecutive byte offsets as 16 blocks of one call: every off0 = 0 .. 15, whatever
    the header length."""
    o = OPTS[kind]
    dc = device(H, opts, o)
    for c, n in align_streams(kind):
        comp, raw = comp_of(c, n), raw_of(c, n)
        what = [(cid(c), n, "shift", j) for j in range(16)]
        st, osz, got, route, in_off = decode(dc, [comp] * 16, [n] * 16, what, shifts=list(range(16)))
        starts = {int(off + stream_info(comp).words) % 16 for off in in_off}
        assert starts == set(range(16)), starts
        bad = mismatches(what, st, osz, got, [raw] * 16)
        assert not bad, bad
        check_route(route, {expected_route(c, o, n): 16})


@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("nsym", [3, 46, 128])
def test_direct_rows_affine_bodies(H, opts, order, nsym):
    """The lengths of one batch three ways.  Affine streams only (byte = index + c: contiguous alphabets, with byte 0
    unused and c > 0, and from byte 0 with c = 0), so that every wave takes the all-affine body chain_decode_dir<*, true>;
    non-affine streams only; and the two alternating block by block, where every wave takes the other body while it
    holds affine streams.  Which body ran follows from the alphabets (k_dec_chain: a wave takes the affine body only if
    all its streams are affine); the route says direct either way."""
    o = OPTS["direct"]
    aff = [case("direct", order, nsym, shape="lo"), case("direct", order, nsym, shape="c0")]
    non = case("direct", order, nsym, shape="gaps")
    for sort in (0, 1):
        dc = device(H, opts, dict(o, sched_sort=sort))
        for c in aff + [non]:
            run(dc, [c], lengths, o)
        # alternating: blocks 2 i and 2 i + 1 are the same length, one of each alphabet
        run(dc, [aff[0], non], lengths, o, order=lambda m: [i // 2 + (i & 1) * (m // 2) for i in range(m)])
        run(dc, [non, aff[1]], lengths, o, order=lambda m: [i // 2 + (i & 1) * (m // 2) for i in range(m)])


def cut_cases(kind):
    """(cyclic data has no words to cut)"""
    return [c for c in KINDS[kind] if c.gen != "cyclic"]


def truncated(c):
    """[(cut, stream without its last `cut` bytes)] of the case's stream of BASE + 37 bytes."""
    comp = comp_of(c, c.base + 37)
    return [(cut, comp[:len(comp) - cut]) for cut in CUTS]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_truncated_word_streams(H, oracle, opts, kind):
    """A stream without its last 2, 4, 30 and 32 bytes, decoded at its full claimed size.  Order 0: the bytes are the
    oracle's for the same truncated stream (it accepts these: a state that finds no word goes on without).  Order 1:
    the same bytes, or status 7 - a garbage symbol may open an empty context, which the device refuses by design.
    Never anything else, and never a byte outside the slot."""
    o = OPTS[kind]
    dc = device(H, opts, o)
    for c in cut_cases(kind):
        n = c.base + 37
        cuts = truncated(c)
        comps = [s for _, s in cuts]
        want = [oracle.uncompress(s, capacity=n) for s in comps]
        assert all(w is not None and len(w) == n for w in want), cid(c)
        what = [(cid(c), n, "cut", cut) for cut, _ in cuts]
        st, osz, got, route, _ = decode(dc, comps, [n] * len(cuts), what)
        bad = mismatches(what, st, osz, got, want, may_refuse=c.order == 1)
        assert not bad, bad
        check_route(route, {expected_route(c, o, n): len(cuts)})


# ---- rANS 4x8 -----------------------------------------------------------------------------------------------------
C8 = [case("x8", o, 46) for o in (0, 1)]
C8_SHORT = [case("x8", o, 3, base=0) for o in (0, 1)]
SHORT8 = list(range(4, 4 + 65))         # (rANS 4x8 has no stored fall-back: every length is entropy-coded)


@functools.lru_cache(maxsize=None)
def comp8_of(c, n):
    import cpu_libs
    from test_oracle4x8 import Codec8
    return Codec8(cpu_libs.oracle().lib, "orc8_").compress(raw_of(c, n), c.order)


def lengths8(c):
    return SHORT8 if c.nsym == 3 else lengths(c)


@pytest.mark.gpu
def test_4x8_every_length_in_one_batch_and_alone(H, opts):
    """rans4x8_hip_uncompress_dev (chain_decode_lds<.., BYTE = true>: images of up to 50 symbols decode from LDS,
    k8_classify; the 4x8 calls have no route read-out): BASE + 0 .. 63 over 46 symbols and the 3-symbol short end, orders 0
    and 1, in one batch each and alone."""
    dc = device(H, opts, {})
    for c in C8 + C8_SHORT:
        ns = lengths8(c)
        for pick in (ns, ns[:61]) + tuple([ns[r]] for r in ALONE):
            what = [(cid(c), n) for n in pick]
            raws = [raw_of(c, n) for n in pick]
            st, osz, got, _, _ = decode(dc, [comp8_of(c, n) for n in pick], pick, what, codec8=True)
            bad = mismatches(what, st, osz, got, raws)
            assert not bad, bad[:10]


# ---- CPU: the cases are what they claim ----------------------------------------------------------------------------
def all_cases():
    seen = []
    for kind, cs in KINDS.items():
        for c in cs:
            seen.append((kind, c))
    for nsym in (3, 46, 128):
        for order in (0, 1):
            for sh in ("lo", "c0", "gaps"):
                seen.append(("direct", case("direct", order, nsym, shape=sh)))
    return seen


def test_cases_are_what_they_claim(oracle):
    """No GPU.  Every stream of every GPU case: entropy-coded by the oracle alone with the order asked for, nsym and table
    bits as the case names them, round-trips to its input; the route every case expects is the kind it is listed under."""
    routes = set()
    for kind, c in all_cases():
        o = OPTS[kind]
        assert {expected_route(c, o, n) for n in lengths(c)} == {c.route}, (kind, cid(c))
        routes.add(c.route)
        a = alphabet(c.nsym, c.order, c.shape)
        assert len(set(a.tolist()) | ({0} if c.order else set())) == c.nsym, cid(c)
        d = np.diff(a.astype(int))
        assert (d == 1).all() == (c.shape != "gaps") and (c.route != "direct" or c.shape != "lo" or a[0] > 1), cid(c)
        ns = lengths(c) + (list(LONG) if c.gen != "cyclic" else [])
        for n in ns:
            raw, comp = raw_of(c, n), comp_of(c, n)
            i = stream_info(comp)
            assert i.coded and i.order == c.order and i.nsym == c.nsym and i.bits == c.bits, (cid(c), n, i, comp[0])
            assert oracle.uncompress(comp, capacity=n) == raw, (cid(c), n)
            if c.order and n - c.base in (0, 37, 63):
                assert table_bits(raw) == c.bits, (cid(c), n)
                assert takes_packed(raw) == (c.bits == 10 and 20 <= c.nsym <= 64), (cid(c), n)
        assert c.gen != "uniform" or (c.nsym <= 64 and c.base >= 4096), cid(c)
        if c.gen == "cyclic":                              # (next to) no words: no trip is ever FAST
            assert all(stream_info(comp_of(c, n)).nwords < 32 for n in lengths(c)), cid(c)
    assert routes == set(ROUTES), routes


def test_lengths_cover_the_epilogue(oracle):
    """No GPU.  BASE + 0 .. 63: every q mod 16 with every n & 3; alone, the epilogue of chains 0 to 2 and of chain 3 sees
    every nd, every rem and both count == t and count != t, with trips of 8 and of 4 steps; the short end holds counts
    below one trip and nwords below 16."""
    bases = sorted({c.base for _, c in all_cases()})
    assert bases[0] == 2048 and all(b & (b - 1) == 0 for b in bases), bases
    for base in bases:
        ns = [base + r for r in range(64)]
        assert {((n >> 2) & 15, n & 3) for n in ns} == {(a, b) for a in range(16) for b in range(4)}
        for trip in (8, 4):
            for k in (0, 3):
                seen = [epilogue(n, k, 1, trip) for n in ns]
                assert {s[1] for s in seen} == {0, 1, 2, 3}, (base, trip, k)
                # (alone with four-step trips the longest chain, chain 3, ends inside its last trip or with it: rem 1 .. 4)
                assert {s[2] for s in seen} == ({1, 2, 3, 4} if (trip, k) == (4, 3) else {0, 1, 2, 3, 4}), (base, trip, k)
                assert {s[3] for s in seen} == {False, True}, (base, trip, k)
                # side by side in one wave t is the longest stream's: count != t with every nd and rem 0 .. 3
                t = (max(epilogue(n, 3, 1, trip)[0] for n in ns) + trip - 1) // trip * trip
                seen = [epilogue(n, k, 1, trip, t) for n in ns]
                assert {(s[1], s[2]) for s in seen} >= {(a, b) for a in range(4) for b in range(4)}, (base, trip, k)
        assert {n - base for n in ns if n - base in ALONE} == set(ALONE)
    assert {((c.base + r) >> 2) & 15 for c in (KINDS["l1"][0],) for r in ALONE} >= {0, 3, 4, 7, 8, 15}
    for c in SHORT:
        ns = short_lengths(c)
        assert ns[0] <= 64, (cid(c), ns[0])
        infos = [stream_info(comp_of(c, n)) for n in ns]
        assert all(i.coded and i.order == c.order and i.nsym == 3 for i in infos), cid(c)
        assert all(oracle.uncompress(comp_of(c, n), capacity=n) == raw_of(c, n) for n in ns), cid(c)
        assert any(i.nwords < 16 for i in infos), cid(c)
        counts = {epilogue(n, k, c.order, 8)[0] for n in ns for k in range(4)}
        assert counts >= set(range(max(1, ns[0] >> 2), 8)) and max(counts) >= 16, (cid(c), sorted(counts))
        assert {n & 3 for n in ns} == {0, 1, 2, 3}


def test_alignment_case_reaches_every_off0():
    """No GPU.  A stream at 16 consecutive byte offsets of an arena that starts on a 16-byte boundary: the 16 addresses of
    its first word are all different modulo 16, for every stream of the alignment test."""
    for kind in KINDS:
        streams = align_streams(kind)
        assert streams[0][0].gen == "skewed" and all(n in (c.base + 37, 65539) for c, n in streams), kind
        orders = {c.order for c in KINDS[kind]}
        assert {c.order for c, n in streams if n == 65539} >= orders - {0} and {c.order for c, n in streams if n != 65539} == orders, kind
        assert kind == "l4" or any(c.gen == "uniform" for c, n in streams if n == 65539), kind
        assert kind != "l4" or {c.nsym for c, n in streams if c.order == 1} == {151, 256}
        for c, n in streams:
            comp = comp_of(c, n)
            i = stream_info(comp)
            assert i.coded and i.order == c.order, (cid(c), n)
            in_off, _ = in_layout([comp] * 16, list(range(16)))
            assert {int(off + i.words) % 16 for off in in_off} == set(range(16)), (cid(c), n)
            if n == 65539:
                # the 256-byte ring wraps 16 times at the least (3 skewed symbols: 1.18 bits each), uniform data a hundred and more
                assert 2 * i.nwords > (100 if c.gen == "uniform" else 16) * 256, (cid(c), i.nwords)


def test_truncated_streams_are_what_they_claim(oracle):
    """No GPU.  The truncated streams still hold their states and some words; the oracle accepts every order-0 one."""
    for kind, cs in KINDS.items():
        for c in cut_cases(kind):
            n = c.base + 37
            i = stream_info(comp_of(c, n))
            assert 2 * i.nwords > max(CUTS), (cid(c), i.nwords)
            for cut, s in truncated(c):
                assert len(s) == i.words + 2 * i.nwords - cut
                got = oracle.uncompress(s, capacity=n)
                if c.order == 0:
                    assert got is not None and len(got) == n, (cid(c), cut)
                    assert got != raw_of(c, n) or cut == 0, (cid(c), cut)      # (the cut is felt: the last bytes differ)


def test_4x8_cases_are_what_they_claim(oracle):
    """No GPU.  The 4x8 streams carry the order asked for and round-trip; 46 and 3 symbols: images that decode from LDS."""
    from test_oracle4x8 import Codec8
    orc8 = Codec8(oracle.lib, "orc8_")
    for c in C8 + C8_SHORT:
        assert len(set(alphabet(c.nsym, c.order).tolist()) | ({0} if c.order else set())) == c.nsym <= 50
        for n in lengths8(c):
            comp = comp8_of(c, n)
            assert comp[0] == c.order and orc8.uncompress(comp) == raw_of(c, n), (cid(c), n)
    assert {n & 3 for n in SHORT8} == {0, 1, 2, 3} and min(SHORT8) >> 2 < 8
