"""arith_dynamic encoding on the device (include/rans4x16_hip.h part 2h; htscodecs_amd/csrc/r4x16_arith_enc.hip).

Expected bytes are the reference's own streams (the 28 fixtures and the inputs of tests/golden/arith/edge.bin) first and
the Python model's second (arith_model.py, pinned to those streams by test_arith_cpu.py), never the library's.  Every
device case runs in the confinement layout of test_gpu_confinement.py - slots of exactly arith_compress_cap bytes, a few
bytes apart at every alignment in a patterned arena, every byte outside them compared afterwards - and asserts its route
(R4X16_ROUTE_ARITH_ENC) against the candidates the model's trace lists.  The lists of inputs are arith_enc_model.py's,
whose census test_arith_enc_cpu.py takes."""
import functools
import random

import numpy as np
import pytest

import arith_cases as K
import arith_enc_model as E
import arith_model as M
from test_gpu_confinement import Layout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dc():
    import htscodecs_amd as H
    return H.DeviceCodec(0)


def cap_of(data, order):
    from htscodecs_amd import codec
    return codec.arith_compress_cap(len(data), order)


@functools.lru_cache(maxsize=None)
def model(data, order):
    """(the model's stream, its route, its candidates) - None where the order word is refused"""
    if E.refused(len(data), order):
        return None, dict.fromkeys(E.KINDS, 0), ()
    trace = []
    s = E.compress(data, order, trace)
    return s, E.route_of(trace), tuple(trace)


def expect(datas, orders, statuses=None):
    want, route = [], dict.fromkeys(E.KINDS, 0)
    for i, (d, o) in enumerate(zip(datas, orders)):
        s, r, _ = model(d, o)
        if statuses is not None and statuses[i]:
            s, r = None, {}
        want.append(s)
        for k, v in r.items():
            route[k] += v
    return want, route


def run_enc(dc, datas, orders, caps=None, one_order=False, planes=0, max_in=None, total=0, stream=None):
    """-> ([bytes or None], statuses, route, the slots as they were left).  Slots of `caps` (default: exactly
    arith_compress_cap); asserts that nothing outside them was written.  one_order: the call's `order` serves all blocks
    (they must agree); otherwise d_order, after set_stripe_encode(planes)."""
    t = dc.torch
    n = len(datas)
    caps = [cap_of(d, o) for d, o in zip(datas, orders)] if caps is None else list(caps)
    lay = Layout(caps, what=["%d bytes, order %#x" % (len(d), o) for d, o in zip(datas, orders)])
    in_off, pos = [], 3
    for i, d in enumerate(datas):
        in_off.append(pos)
        pos += len(d) + 1 + i % 7
    arena_in = np.zeros(pos + 64, dtype=np.uint8)
    for o, d in zip(in_off, datas):
        arena_in[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    up = lambda a: t.from_numpy(a).to(dc.dev)
    d_in, d_out = up(arena_in), up(lay.pattern.copy())
    d_ioff, d_ooff = up(np.array(in_off, dtype=np.int64)), up(lay.offs.copy())
    d_isz = up(np.array([len(d) for d in datas], dtype=np.int32))
    d_cap = up(np.array(caps, dtype=np.int64).astype(np.uint32).view(np.int32))
    d_osz = t.full((n,), -7, dtype=t.int32, device=dc.dev)
    d_st = t.full((n,), -7, dtype=t.int32, device=dc.dev)
    d_ord = None
    if one_order:
        assert len(set(orders)) == 1
    else:
        d_ord = up(np.array(orders, dtype=np.int64).astype(np.uint32).view(np.int32))
    dc.set_stripe_encode(planes)
    dc.set_option("route_count", 1)
    try:
        dc.route_read("arith_enc")
        args = (d_in, d_ioff, d_isz, d_out, d_ooff, d_cap, d_osz, d_st, orders[0] if one_order else 0,
                max_in or max([len(d) for d in datas] + [1]))
        if stream is None:
            dc.arith_compress(*args, d_order=d_ord, total_in_size=total)
        else:
            stream.wait_stream(t.cuda.current_stream(dc.dev))
            with t.cuda.stream(stream):
                dc.arith_compress(*args, d_order=d_ord, total_in_size=total)
            stream.synchronize()
        t.cuda.synchronize(dc.dev)
        route = dc.route_read("arith_enc")
    finally:
        dc.set_option("route_count", 0)
        dc.set_stripe_encode(0)
    arena = d_out.cpu().numpy()
    stray = lay.stray_writes(arena)
    assert stray is None, stray
    st, osz = d_st.tolist(), d_osz.tolist()
    for i in range(n):
        assert st[i] >= 0 and (osz[i] == 0 if st[i] else 0 < osz[i] <= caps[i]), (i, st[i], osz[i])
    outs = [b if s == 0 else None for b, s in zip(lay.take(arena, osz), st)]
    return outs, st, route, (lay, arena)


def check(dc, datas, orders, want=None, **kw):
    """run_enc against the model (and `want`, the reference's streams, where there are any): bytes, statuses, route"""
    statuses = [E.refused(len(d), o) for d, o in zip(datas, orders)]
    mod, route = expect(datas, orders)
    outs, st, got_route, _ = run_enc(dc, datas, orders, **kw)
    assert st == statuses, [(i, a, b) for i, (a, b) in enumerate(zip(st, statuses)) if a != b][:5]
    for i, out in enumerate(outs):
        if want is not None:
            assert out == want[i], (i, "not the reference's bytes", len(datas[i]), hex(orders[i]), len(out or b""), len(want[i]))
        assert out == mod[i], (i, "not the model's bytes", len(datas[i]), hex(orders[i]), len(out or b""), len(mod[i] or b""))
    assert got_route == route, (got_route, route)
    return outs, got_route


def split(cases):
    return [c[1] for c in cases], [c[2] for c in cases]


# ---- the 28 fixtures through every entry point --------------------------------------------------------------------
def test_fixtures_in_one_batch_with_per_block_orders(dc):
    datas, orders = split(E.fixture_cases())
    _, route = check(dc, datas, orders, want=[c[3] for c in E.fixture_cases()], planes=4)
    assert route["o0"] >= 8 and route["o1_lds"] >= 8 and route["o1_global"] >= 2 and route["rle"] >= 8


def test_fixtures_with_one_order_a_call(dc):
    """one order for all blocks: stripe blocks are encoded without rans4x16_hip_set_dev_stripe_encode"""
    by_order = {}
    for _, text, order, s in E.fixture_cases():
        by_order.setdefault(order, []).append((text, s))
    assert 8 in by_order and 9 in by_order
    for order, lst in sorted(by_order.items()):
        check(dc, [t for t, _ in lst], [order] * len(lst), want=[s for _, s in lst], one_order=True)


def test_fixtures_through_the_host_batch(dc):
    from htscodecs_amd import codec
    datas, orders = split(E.fixture_cases())
    codec.set_option("route_count", 1)
    try:
        codec.route_read("arith_enc")
        outs, st = codec.arith_compress_batch(datas, orders)
        route = codec.route_read("arith_enc")
    finally:
        codec.set_option("route_count", 0)
    assert st == [0] * len(datas)
    assert outs == [c[3] for c in E.fixture_cases()]
    assert route == expect(datas, orders)[1]


def test_fixtures_through_the_single_calls(dc):
    from htscodecs_amd import codec
    for i, (fn, text, order, s) in enumerate(E.fixture_cases()):
        assert codec.arith_compress(text, order) == s, fn                               # arith_compress: a buffer of the bound
        if i % 4 == 0:                                                                  # arith_compress_to: the caller's buffer
            for cap in (codec.arith_compress_cap(len(text), order), codec.arith_compress_bound(len(text), order)):
                assert codec.arith_compress(text, order, out_size=cap) == s, (fn, cap)
    text, order = E.fixture_cases()[0][1:3]
    assert codec.arith_compress(text, order, out_size=codec.arith_compress_cap(len(text), order) - 1) is None
    assert codec.arith_compress(text, M.X_EXT) is None and codec.arith_compress(text, 8 | (256 << 8)) is None
    assert codec.arith_compress(b"", 0) == M.compress(b"", 0)


# ---- every input of edge.bin ----------------------------------------------------------------------------------------
def test_every_edge_input_gives_the_references_stream(dc):
    cases = E.edge_cases()
    datas, orders = split(cases)
    assert all(((o >> 8) or 4) <= 32 for o in orders if o & M.X_STRIPE)
    check(dc, datas, orders, want=[c[3] for c in cases], planes=32)


# ---- capacity -------------------------------------------------------------------------------------------------------
def test_the_exact_capacity_is_accepted_and_one_byte_less_is_not(dc):
    q = M.text("q8")
    datas = [q[:500], q[:500], q[:501], q[:3000], q[:3000], q[:40], q[:40], b"", b""]
    orders = [1, 1, 193, 9 | (5 << 8), 9 | (5 << 8), 65, 65, 0, 0]
    caps = [cap_of(d, o) - (i % 2) for i, (d, o) in enumerate(zip(datas, orders))]
    outs, st, _, (lay, arena) = run_enc(dc, datas, orders, caps=caps, planes=5)
    for i, (d, o) in enumerate(zip(datas, orders)):
        if i % 2:
            assert st[i] == M.E_CAPACITY and outs[i] is None
            slot = arena[lay.offs[i]:lay.offs[i] + caps[i]]
            assert (slot == lay.pattern[lay.offs[i]:lay.offs[i] + caps[i]]).all(), (i, "a refused block's slot was written")
        else:
            assert st[i] == 0 and outs[i] == M.compress(d, o), i


# ---- the step ---------------------------------------------------------------------------------------------------
def test_the_step_in_every_home_against_the_model(dc):
    cases = E.step_cases() + E.boundary_cases() + E.rare_cases()
    datas, orders = split(cases)
    outs, route = check(dc, datas, orders)
    assert route["o0"] > 50 and route["o1_lds"] > 50 and route["o1_global"] > 50 and route["rle"] > 50 and route["stored"] > 10
    # the dword sink's flush: bodies of every length mod 16 (and so mod 4) came out coded, in every home
    for home in ("o0", "o1_lds", "o1_global"):
        res = set()
        for d, o in zip(datas, orders):
            res |= {c["body"] % 16 for c in model(d, o)[2] if c["coded"] and not c["stored"] and c["home"] == home}
        assert res == set(range(16)), (home, sorted(res))


def test_the_halving_ties_in_every_home_against_the_model(dc):
    datas, orders = split(K.tie_cases())
    outs, route = check(dc, datas, orders)
    assert route["stored"] == 0 and route["o0"] >= 6 and route["o1_lds"] >= 12 and route["o1_global"] >= 12 and route["rle"] >= 14


def test_the_decision_between_coded_and_stored_at_its_boundary(dc):
    """coded size n - 1: coded; n and n + 1: stored (arith_dynamic.c:850 compares with >=)"""
    cases = E.boundary_cases()
    datas, orders = split(cases)
    outs, _ = check(dc, datas, orders)
    for (what, d, o), out in zip(cases, outs):
        assert bool(out[0] & M.X_CAT) == (not what.endswith("n-1")), what


# ---- second trips ---------------------------------------------------------------------------------------------------
def test_more_items_of_the_global_home_than_it_has_slots(dc):
    datas, orders = split(E.trip_cases())
    _, route = check(dc, datas, orders, one_order=True)
    assert route["o1_global"] == 1100


def test_a_small_ceiling_walks_the_call_in_chunks(dc):
    import htscodecs_amd as H
    small = H.DeviceCodec(0)                                          # (fresh: its arena starts at nothing)
    small.set_option("max_workspace_mb", 8)
    datas, orders = split(E.trip_cases()[:300])
    least = -(-300 * (256 * 256 * 4 + 256 * 4) // (8 << 20))          # a row slot an item
    assert least >= 3
    small.route_read("launch")
    outs, _ = check(small, datas, orders)
    launches = small.route_read("launch")
    assert launches["in_order"] >= least and launches["side_by_side"] == 0, (launches, least)
    dc.route_read("launch")
    outs_one, _ = check(dc, datas, orders)
    assert dc.route_read("launch") == {"in_order": 1, "side_by_side": 0}
    assert outs == outs_one


def test_stripe_blocks_up_to_255_planes_and_what_the_call_refuses(dc):
    q = M.text("q40+dir")
    check(dc, [q[:4000]], [9 | (255 << 8)], planes=255)
    check(dc, [q[:4000], q[:300]], [8 | (255 << 8)] * 2, one_order=True)
    check(dc, [E.packed_planes()] * 2, [8 | (8 << 8), 9 | (8 << 8)], planes=8)           # (what the capacity of an even order is for)
    # under d_order: without the setting, and with more planes than it reserved, beside blocks that are encoded
    datas = [q[:400], q[:400], q[:400], q[:400], q[:20]]
    orders = [1, 9 | (5 << 8), 9 | (4 << 8), 8, 9 | (5 << 8)]
    U = M.E_UNSUPPORTED
    outs, st, _, _ = run_enc(dc, datas, orders, planes=0)
    assert st == [0, U, U, U, 0] and outs[0] == M.compress(datas[0], 1) and outs[4] == M.compress(datas[4], 9)
    outs, st, _, _ = run_enc(dc, datas, orders, planes=4)
    assert st == [0, U, 0, 0, 0] and [outs[i] for i in (2, 3)] == [M.compress(datas[i], orders[i]) for i in (2, 3)]
    # the order word's own refusals: X_EXT, more than 255 planes
    outs, st, _, _ = run_enc(dc, datas[:3], [M.X_EXT | 1, 8 | (256 << 8), 65], planes=4)
    assert st == [U, U, 0] and outs[2] == M.compress(datas[2], 65)


def test_sizes_at_the_thresholds_of_the_flag_rules(dc):
    q = M.text("q4")
    datas, orders = [], []
    for n in (0, 1, 7, 8, 20, 21):
        for o in (0, 1, 64, 65, 128, 129, 192, 193, 8, 9, 9 | (2 << 8), 16, 17, 32, 33 | 128, 2, 3):
            datas.append(q[100:100 + n])
            orders.append(o)
    check(dc, datas, orders, planes=4)


# ---- stripe ties ------------------------------------------------------------------------------------------------------
def test_the_first_smallest_candidate_wins_a_tie(dc):
    """plane 0 cannot be coded smaller than it is: candidates 1, 64 and 0 all store it and tie; the reference keeps the
    first (flag 0x30: X_CAT | X_NOSZ), not the second (0x70, which keeps X_RLE)"""
    rng = random.Random(12)
    noise = bytes(rng.randrange(256) for _ in range(512))
    text = M.text("q4")[:512]
    data = bytes(b for pair in zip(noise, text) for b in pair)
    outs, _ = check(dc, [data], [9 | (2 << 8)], one_order=True)
    s = outs[0]
    pos = 1 + M.var_get(s, 1, len(s))[0] + 1
    for _ in range(2):
        pos += M.var_get(s, pos, len(s))[0]
    assert s[pos] == 0x30, hex(s[pos])


# ---- round trip -------------------------------------------------------------------------------------------------------
def test_round_trip_through_both_device_calls(dc):
    from arith_gpu import run_dev
    rng = random.Random(77)
    datas, orders = [], []
    for i in range(120):
        k = rng.choice((1, 2, 3, 5, 16, 17, 60, 120, 256))
        syms = rng.sample(range(256), k)
        n = rng.choice((0, 1, 5, 30, 200, 1500, 5000))
        datas.append(K.skewed(tuple(syms), max(n, k), i, runs=rng.choice((0, 0, 3, 9))) if n else b"")
        orders.append(rng.choice((0, 1, 64, 65, 128, 129, 192, 193, 8 | (3 << 8), 9 | (4 << 8), 9, 16, 33)))
    outs, st, _, _ = run_enc(dc, datas, orders, planes=4)
    assert st == [0] * len(datas)
    back, st, _ = run_dev(dc, outs, [len(d) for d in datas], planes=4, stripe_out=max(map(len, datas)))
    keep = [i for i, o in enumerate(outs) if o]
    assert [st[i] for i in keep] == [0] * len(keep) and [back[i] for i in keep] == [datas[i] for i in keep]
