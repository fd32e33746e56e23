"""arith_dynamic decoding on the device (include/rans4x16_hip.h part 2g; htscodecs_amd/csrc/r4x16_arith.hip).

Expected bytes are the raw inputs or the Python model's (arith_model.py, pinned by the reference-made files of
tests/golden/arith in test_arith_cpu.py), never the library's.  Every device case asserts its route (R4X16_ROUTE_ARITH)
against the model's count of entropy-coded pieces, and runs in the confinement layout of arith_gpu.run_dev: slots a few
bytes apart in a patterned arena, every byte outside them compared.  Streams are made once a module and shared."""
import functools

import pytest

import arith_cases as K
import arith_model as M
from arith_gpu import check, expect, run_dev

pytestmark = pytest.mark.gpu
ORDERS = (0, 1, 64, 65)                                              # order 0 / 1, without and with X_RLE


@pytest.fixture(scope="module")
def dc():
    import htscodecs_amd as H
    return H.DeviceCodec(0)


@functools.lru_cache(maxsize=None)
def fixtures():
    fx = M.fixtures()
    return [s for _, _, _, s in fx], [M.text(b) for _, b, _, _ in fx]


def _caps(streams, raws):
    """the stored size, 37 bytes more for one block in three - except where the capacity IS the size (X_NOSZ, X_STRIPE)"""
    return [len(r) + (37 if i % 3 == 2 and not s[0] & 0x18 else 0) for i, (s, r) in enumerate(zip(streams, raws))]


# ---- the 28 reference streams through every entry point -------------------------------------------------------------
def test_fixtures_as_one_batch_through_the_device_call(dc):
    streams, raws = fixtures()
    _, _, route = check(dc, streams, _caps(streams, raws), planes=4, stripe_out=max(map(len, raws)), want=raws)
    # the model's count is asserted by check(); here: what the count is made of.  The texts' own alphabets (m <= 84) keep
    # their order-1 rows in LDS; the four packed order-1 streams (q4 / q8 under 129 and 193) code packed bytes up to
    # 255 and take the global home
    assert route["o0"] > 12 and route["o1_lds"] > 12 and route["o1_global"] == 4 and route["rle"] >= 12


def test_fixtures_singly_through_the_device_call(dc):
    streams, raws = fixtures()
    for s, r in zip(streams, raws):
        check(dc, [s], [len(r)], planes=4, stripe_out=len(r), want=[r])


def test_fixtures_through_the_host_batch(dc):
    from htscodecs_amd import codec
    streams, raws = fixtures()
    codec.set_option("route_count", 1)
    try:
        codec.route_read("arith")
        outs, st = codec.arith_uncompress_batch(streams, _caps(streams, raws))
        route = codec.route_read("arith")
    finally:
        codec.set_option("route_count", 0)
    assert st == [0] * len(streams) and outs == raws
    assert route == expect(streams, _caps(streams, raws), 255, None)[1]


def test_fixtures_through_the_single_calls(dc):
    from htscodecs_amd import codec
    streams, raws = fixtures()
    for i, (s, r) in enumerate(zip(streams, raws)):
        assert codec.arith_uncompress(s) == r, i                     # arith_uncompress: the size from the stream
        if i % 4 == 0:                                               # arith_uncompress_to: a buffer of the caller's
            cap = len(r) + (0 if s[0] & 0x18 else 11)
            assert codec.arith_uncompress(s, out_size=cap) == r, i
    assert codec.arith_uncompress(streams[0], out_size=len(raws[0]) - 1) is None
    assert codec.arith_uncompress(b"") is None


def test_peek_gives_flag_byte_and_stored_size(dc):
    import numpy as np
    t = dc.torch
    streams, raws = fixtures()
    streams = list(streams[:6]) + [b"", M.compress(raws[0][:40], 16)]
    sizes = [len(r) for r in raws[:6]] + [None, None]
    off = np.cumsum([0] + [len(s) + 5 for s in streams])[:-1]
    arena = np.zeros(int(off[-1]) + len(streams[-1]) + 64, dtype=np.uint8)
    for o, s in zip(off, streams):
        arena[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    up = lambda a: t.from_numpy(a).to(dc.dev)
    fmt, raw, st = (t.full((len(streams),), -5, dtype=t.int32, device=dc.dev) for _ in range(3))
    dc.arith_peek(up(arena), up(off.astype(np.int64)), up(np.array([len(s) for s in streams], dtype=np.int32)), fmt, raw, st, 1 << 20)
    t.cuda.synchronize()
    assert st.tolist() == [0] * 6 + [M.E_EMPTY, 0]
    assert fmt.tolist() == [s[0] for s in streams[:6]] + [-1, streams[-1][0]]
    assert raw.tolist() == sizes[:6] + [-1, -1]


# ---- the step ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_cases():
    """[(what, raw, order)]"""
    q8 = M.text("q8")
    out = [("q8[:%d]" % n, q8[:n], o) for n in range(0, 71) for o in ORDERS]
    # the first halving of a model: (65,519 - m) / 16 symbols of one context, whatever m - one symbol repeated behind a
    # first byte that sets the alphabet, the alphabet walking through 1 .. 256 with the length
    for k, n in enumerate(range(4060, 4111)):
        m = (1, 2, 3, 64, 65, 128, 255, 256)[k % 8]
        out += [("halving n=%d m=%d" % (n, m), bytes([m - 1]) + bytes(n - 1), o) for o in ORDERS]
    for m in (1, 2, 3, 4, 5, 63, 64, 65, 128, 255, 256):
        out += [("m=%d" % m, K.with_alphabet(m, 300, m), o) for o in ORDERS]
    for m in (5, 64, 65, 256):                                       # across every lane boundary of the list
        out += [("climber m=%d" % m, K.climber(m, 2 * m + 20), o) for o in ORDERS]
    out += [("ties", K.ties(200), o) for o in ORDERS]
    # order-1 alphabets on both sides of the LDS budget (84 | 85), byte 255 included
    for m in (83, 84, 85, 86, 200, 256):
        out += [("order-1 home m=%d" % m, K.with_alphabet(m, 1500, 1000 + m), o) for o in (1, 65)]
    # one order-1 context, and one run context, used more than 4,100 times
    out += [("one row", bytes([83]) + b"A" * 4300, 1), ("one row, global", bytes([200]) + b"A" * 4300, 1),
            ("one run context", b"AAB" * 4200, 64), ("one run context", b"AAB" * 4200, 65)]
    return out


@functools.lru_cache(maxsize=None)
def step_streams():
    return [M.compress(raw, o) for _, raw, o in step_cases()]


def test_the_step_at_every_length_alphabet_and_home(dc):
    cases, streams = step_cases(), step_streams()
    raws = [r for _, r, _ in cases]
    _, _, route = check(dc, streams, _caps(streams, raws), want=raws)
    assert route["o1_lds"] > 50 and route["o1_global"] >= 10 and route["o0"] > 50 and route["rle"] > 50
    # the streams really are what their names say: the coder drops order 1 below 8 bytes, and the long ones kept their coder
    for (what, raw, o), s in zip(cases, streams):
        if len(raw) >= 100:
            assert s[0] == o, (what, s[0], o)
        if len(raw) < 8:
            assert s[0] & 3 == 0, what


def test_each_named_order_1_case_takes_its_own_home(dc):
    """singly, so that the route count is the case's own: rows in LDS up to m = 84, in global memory above"""
    for (what, raw, o), s in zip(step_cases(), step_streams()):
        if what.startswith(("order-1 home", "one row")):
            m = max(raw) + 1
            _, _, route = check(dc, [s], [len(raw)], want=[raw])
            assert route == {"o0": 0, "o1_lds": int(m <= 84), "o1_global": int(m > 84), "rle": int(bool(o & 64))}, (what, m, route)


def test_what_the_call_announces_is_enforced_beside_good_neighbours(dc):
    q = M.text("q8")
    good, raw = M.compress(q[:1000], 1), q[:1000]
    long_in, long_out = M.compress(q[:3000], 0), M.compress(bytes(4000), 64)
    assert len(long_in) > len(good) >= len(long_out)
    U = M.E_UNSUPPORTED
    # a block above max_in_size is not read; a stored size above max_out_size is refused (its slot would hold it)
    outs, st, _ = run_dev(dc, [good, long_in, good, long_out, good], [1000, 3000, 1000, 4000, 1037], max_in=len(good), max_out=1037)
    assert st == [0, U, 0, U, 0] and outs[0] == outs[2] == outs[4] == raw
    # a batch that decodes to more than total_out_size: the total holds two of these four blocks (1,000 bytes each of
    # 2,000); which two is not determined
    outs, st, _ = run_dev(dc, [good] * 4, [1000] * 4, total=2000)
    assert sorted(st) == [0, 0, U, U] and all(o == raw for o, x in zip(outs, st) if x == 0)


# ---- runs -------------------------------------------------------------------------------------------------------
def test_runs_of_every_length_and_place(dc):
    lengths = list(range(0, 11)) + [x for k in range(4, 12) for x in (3 * k - 1, 3 * k, 3 * k + 1)] + [299, 300, 301]
    raws = []
    for r in lengths:
        raws += [b"xyz" * 4 + b"q" * (r + 1) + b"zyx" * 4,           # inside
                 b"xyz" * 4 + b"q" * (r + 1),                        # a run that ends exactly at the block's end
                 b"q" * (r + 1) + b"xyzxyzxyz"]                      # a run right after the first byte
    orders = [64 + (i & 1) for i in range(len(raws))] + [65 - (i & 1) for i in range(len(raws))]
    raws = raws + raws
    streams = [M.compress(r, o) for r, o in zip(raws, orders)]
    assert sum(bool(s[0] & M.X_RLE) and not s[0] & M.X_CAT for s in streams) > len(streams) // 2
    check(dc, streams, _caps(streams, raws), want=raws)


# ---- containers ---------------------------------------------------------------------------------------------------
def _pack_raw(k, n, seed):
    import random
    rng = random.Random(seed)
    return bytes(rng.randrange(k) * 9 + 2 for _ in range(n - k)) + bytes(j * 9 + 2 for j in range(k)) if k else b""


def test_pack_cat_and_nosz(dc):
    raws, orders = [], []
    for k in (0, 1, 2, 3, 4, 5, 16, 17):
        for n in (k + 1, 37, 203, 1001):                             # not divisible by 8, 4 or 2
            for o in (128, 129, 192, 193):
                raws.append(_pack_raw(k, max(n, k), 31 * k + n))
                orders.append(o)
    q = M.text("qvar")
    import random
    noise = bytes(random.Random(5).sample(range(256), 256))            # every byte once: no coder beats a copy
    raws += [q[:100], q[:100], q[:9], noise, noise, q[:500], q[:500], q[:77]]
    orders += [32, 33 | 128, 32, 0, 65, 16, 17 | 64, 16 | 128]       # X_CAT explicit, as fall-back; bare X_NOSZ streams
    streams = [M.compress(r, o) for r, o in zip(raws, orders)]
    assert streams[-5][0] & M.X_CAT and streams[-4][0] & M.X_CAT and not streams[-3][0] & M.X_CAT
    check(dc, streams, _caps(streams, raws), want=raws)


def _plane_flags(s):
    """the flag byte of every plane of a stripe stream"""
    pos = 1 + M.var_get(s, 1, len(s))[0]
    n, pos = s[pos], pos + 1
    lens = []
    for _ in range(n):
        nb, v = M.var_get(s, pos, len(s))
        lens.append(v)
        pos += nb
    out = []
    for v in lens:
        out.append(s[pos])
        pos += v
    return out


def test_stripe_blocks_and_what_the_device_call_refuses(dc):
    q, q4 = M.text("q40+dir"), M.text("q4")
    raws, orders = [], []
    for N in (1, 2, 3, 4, 5, 8, 32):
        for n in (max(21, N + 1), N + 1 if N + 1 > 20 else 22, 10 * N + 23, 1201):   # (20 bytes and fewer are not striped)
            raws += [q[:n], q4[:n] if n % 2 else bytes(range(n % 251)) * 2 + q4[:n]]
            orders += [8 | (N << 8), 9 | (N << 8)]
    streams = [M.compress(r, o) for r, o in zip(raws, orders)]
    assert all(s[0] & M.X_STRIPE for s in streams)
    caps = [len(r) for r in raws]
    check(dc, streams, caps, planes=32, stripe_out=max(caps), want=raws)
    # planes of different methods inside one block
    assert any(len(set(_plane_flags(s))) > 1 for s in streams)
    # refusals, each beside blocks that decode: a nested stripe, more planes than reserved, a larger block than reserved,
    # a capacity that is not the stored size, X_EXT, no reservation at all
    good = M.compress(q[:400], 1)
    inner = M.compress(q[:100], 8 | (2 << 8))
    nested = bytes([8]) + M.var_put(100) + bytes([1]) + M.var_put(len(inner)) + inner
    five = M.compress(q[:300], 9 | (5 << 8))
    four = M.compress(q[:300], 9 | (4 << 8))
    ext = bytes([M.X_EXT]) + M.var_put(40) + bytes(range(30))
    batch = [good, nested, good, five, four, four, ext, good, M.compress(q[:5000], 8)]
    bcaps = [400, 100, 437, 300, 300, 301, 40, 400, 5000]
    _, st, _ = check(dc, batch, bcaps, planes=4, stripe_out=4096)
    assert st == [0, M.E_UNSUPPORTED, 0, M.E_UNSUPPORTED, 0, M.E_CAPACITY, M.E_UNSUPPORTED, 0, M.E_UNSUPPORTED]
    _, st, _ = check(dc, batch, bcaps, planes=0)
    U = M.E_UNSUPPORTED                                             # (the capacity test comes before the reservation's)
    assert st == [0, U, 0, U, U, M.E_CAPACITY, U, 0, U]


# ---- one mixed batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_stream", [False, True])
def test_one_mixed_batch_short_and_long_waves_together(dc, own_stream):
    cases, streams = step_cases(), step_streams()
    fx, fraw = fixtures()
    long_ones = [(fx[i], fraw[i]) for i in (1, 7, 12, 15)]            # q4.1, q4.65, q40+dir.0, q40+dir.8
    pick = list(range(0, len(cases), 3))
    q = M.text("qvar")
    more = [(_pack_raw(k, 150 + k, k), 128 + (k & 1) + 64 * (k & 2 > 0)) for k in (1, 2, 3, 4, 5, 16, 17)]
    more += [(q[:n], o | (N << 8)) for N, n in ((1, 21), (2, 33), (3, 100), (4, 1001)) for o in (8, 9)]
    more += [(q[:60], 32), (q[:60], 16), (q[:333], 17 | 64)]         # X_CAT, bare X_NOSZ streams
    batch = [streams[i] for i in pick] + [M.compress(r, o) for r, o in more] + [s for s, _ in long_ones]
    raws = [cases[i][1] for i in pick] + [r for r, _ in more] + [r for _, r in long_ones]
    order = sorted(range(len(batch)), key=lambda i: (i * 7919) % len(batch))          # the long ones among the short
    batch, raws = [batch[i] for i in order], [raws[i] for i in order]
    stream = dc.torch.cuda.Stream(dc.dev) if own_stream else None
    check(dc, batch, _caps(batch, raws), planes=4, stripe_out=max(map(len, raws)), want=raws, stream=stream)
