"""arith_dynamic decoding on the device where a loop takes its second trip (include/rans4x16_hip.h part 2g;
htscodecs_amd/csrc/r4x16_arith.hip): the coder's input window at every refill and alignment, a workgroup of the global
home at its second item, the call's walk over chunks, stripe blocks of up to 255 planes, and a total_out_size that is
exactly what the batch decodes to.  The step's own second looks - halving and the comparison in one step - are inputs of
arith_cases.py and run here in one batch.

Everything is compared byte for byte with the Python model (arith_model.py) and with the raw input where the stream is
valid, in the confinement layout of arith_gpu.run_dev, with the route count of the model.  The batches are built once
and shared with test_arith_inputs_cpu.py, which holds them to the events they are here for."""
import functools

import pytest

import arith_cases as K
import arith_model as M
from arith_gpu import check, run_dev
from test_gpu_arith import _caps, _pack_raw, _plane_flags, step_cases, step_streams

pytestmark = pytest.mark.gpu
ROW_SLOT = 256 * 256 * 4 + 256 * 4                # bytes of one workgroup's rows in the global home (r4x16_arith.hip)
U = M.E_UNSUPPORTED


@pytest.fixture(scope="module")
def dc():
    import htscodecs_amd as H
    return H.DeviceCodec(0)


# ---- the step: halving and the comparison --------------------------------------------------------------------------
def test_halving_before_the_comparison_ties_and_their_twins(dc):
    cases, streams = K.tie_cases(), K.tie_streams()
    raws = [r for _, r, _ in cases]
    check(dc, streams, _caps(streams, raws), want=raws)


# ---- the input window ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def window_batch():
    """(streams, caps, raws - None for a truncated stream, in_off, [(home, payload bytes, payload address mod 16)]).
    The valid streams of window_residues lie so that a home's payloads start at all 16 addresses mod 16 (stream k of a
    home at 7 k + 5); the others a few bytes apart."""
    rows = [(home, s, len(raw), raw, size, None) for home, raw, s, size in K.window_bases()]
    rows += [(home, s, len(raw), raw, size, (7 * k + 5) % 16) for k, (home, raw, s, size) in enumerate(K.window_residues())]
    rows += [(home, s, cap, None, size, None) for home, s, cap, size in K.window_truncations()]
    in_off, facts, pos = [], [], 3
    for i, (home, s, _, _, size, want_at) in enumerate(rows):
        head = len(s) - size
        while want_at is not None and (pos + head) % 16 != want_at:
            pos += 1
        in_off.append(pos)
        facts.append((home, size, (pos + head) % 16))
        pos += len(s) + 1 + i % 7
    return [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], in_off, facts


def test_the_input_window_at_every_size_and_alignment(dc):
    streams, caps, raws, in_off, facts = window_batch()
    for home in ("o0", "o1_lds", "o1_global"):
        assert {at for h, size, at in facts if h == home and size > 1024} == set(range(16)), home
    outs, st, _ = check(dc, streams, caps, in_off=in_off)
    assert st == [0] * len(streams)                                   # (a truncated payload is a starved coder, not an error)
    for i, raw in enumerate(raws):
        if raw is not None:
            assert outs[i] == raw, (i, facts[i])


# ---- a workgroup's second item -------------------------------------------------------------------------------------
def _tiny(i):
    return bytes((i * 7 + k * k) % 3 for k in range(12))


@functools.lru_cache(maxsize=None)
def many_blocks():
    """(streams, raws): 1,040 blocks for planes = 0, an item each.  The global home runs 1,024 workgroups, so workgroup i
    decodes item i and then item i + 1,024: for twelve i both are order-1 streams of the global home - m = 256 with
    X_RLE and then m = 85 without, or the other way round - and the second meets the rows, totals and run models the
    first left.  The rest are order-0 streams of a few bytes."""
    raws = [_tiny(i) for i in range(1040)]
    orders = [0] * 1040
    for i in range(12):
        wide, narrow = K.with_alphabet(256, 700, 5000 + i), K.with_alphabet(85, 700, 6000 + i)
        a, b = (i, i + 1024) if i % 2 == 0 else (i + 1024, i)
        raws[a], orders[a] = wide, 65
        raws[b], orders[b] = narrow, 1
    streams = [M.compress(r, o) for r, o in zip(raws, orders)]
    assert all(s[0] == o for s, o in zip(streams, orders))            # (none fell back to a copy)
    return streams, raws


def _stripe_of(symbols, n, seed, chain):
    """n bytes whose four planes are chains of their own over `symbols`"""
    planes = [K.skewed(symbols, (n + 3) // 4, seed + j, chain=chain) for j in range(4)]
    return bytes(planes[x % 4][x // 4] for x in range(n))


def _stripe_high(n, seed):
    """eight symbols from 200 up: every plane's best method is order 1, and its rows take the global home"""
    return _stripe_of(tuple(range(200, 208)), n, seed, 8)


@functools.lru_cache(maxsize=None)
def many_planes():
    """(streams, raws): 300 blocks for planes = 4, four items each.  Blocks b and b + 256 share their four workgroups of
    the global home: for ten b both are stripe blocks with global-home planes, so items above 1,024 are of that home."""
    raws = [_tiny(i) for i in range(300)]
    orders = [0] * 300
    q = M.text("qvar")
    for b in range(10):
        for at in (b, b + 256):
            raws[at], orders[at] = _stripe_high(1600 + 4 * b + (at > 255), at), 9 | (4 << 8)
        raws[20 + b], orders[20 + b] = q[100 * b:100 * b + 400 + b], (8, 9)[b & 1] | (4 << 8)
    streams = [M.compress(r, o) for r, o in zip(raws, orders)]
    for b in list(range(10)) + list(range(256, 266)):
        t = []
        assert M.uncompress_to(streams[b], len(raws[b]), trace=t)[0] == 0 and t.count("o1_global") >= 3, (b, t)
    return streams, raws


def test_more_items_than_workgroups_of_the_global_home(dc):
    streams, raws = many_blocks()
    _, _, route = check(dc, streams, [len(r) for r in raws], want=raws)
    assert route == {"o0": 1040 - 24, "o1_lds": 0, "o1_global": 24, "rle": 12}
    streams, raws = many_planes()
    _, _, route = check(dc, streams, [len(r) for r in raws], planes=4, stripe_out=max(map(len, raws)), want=raws)
    assert route["o1_global"] >= 60 and route["o0"] >= 270


# ---- chunks -------------------------------------------------------------------------------------------------------
CEILING_MB = 8


@functools.lru_cache(maxsize=None)
def chunk_batches():
    """[(streams, raws, planes)]: 100 blocks for planes = 0 and 60 for planes = 4 - stripe blocks, both order-1 homes,
    X_PACK and X_CAT"""
    cases, streams = step_cases(), step_streams()
    pick = list(range(0, len(cases), 6))[:95]
    one = [streams[i] for i in pick] + list(K.tie_streams()[:5]), [cases[i][1] for i in pick] + [r for _, r, _ in K.tie_cases()[:5]]
    q = M.text("qvar")
    more = [(_stripe_high(900 + b, 70 + b), 9 | (4 << 8)) for b in range(10)]
    more += [(q[50 * b:50 * b + 300 + b], (8, 9)[b & 1] | (4 << 8)) for b in range(10)]
    more += [(_pack_raw(k, 150 + k, k), 128 + (k & 1) + 64 * (k & 2 > 0)) for k in (1, 2, 3, 4, 5, 7, 9, 12, 16, 17)]
    more += [(q[:60 + b], 32 + (b & 1)) for b in range(5)]
    more += [(q[b:b + 500], 1 + 64 * (b & 1)) for b in range(10)]
    more += [(K.with_alphabet(200, 400 + b, 300 + b), 65 - 64 * (b & 1)) for b in range(10)]
    more += [(q[:90 + b], 0) for b in range(5)]
    order = sorted(range(60), key=lambda i: (i * 37) % 60)
    two = [M.compress(*more[i]) for i in order], [more[i][0] for i in order]
    assert len(one[0]) == 100 and len(two[0]) == 60
    return [one + (0,), two + (4,)]


def test_a_small_ceiling_walks_the_arith_call_in_chunks(dc):
    """Every item of a chunk of up to 1,024 items has a row slot of 263,168 bytes in the call's arena, so a chunk under a
    ceiling holds at most ceiling / 263,168 items: the call counts its chunks under the launch route."""
    import htscodecs_amd as H
    small = H.DeviceCodec(0)                                          # (fresh: its arena starts at nothing)
    small.set_option("max_workspace_mb", CEILING_MB)
    for streams, raws, planes in chunk_batches():
        caps = _caps(streams, raws)
        least = -(-len(streams) * max(planes, 1) * ROW_SLOT // (CEILING_MB << 20))
        assert least >= 3
        small.route_read("launch")
        outs, st, _ = check(small, streams, caps, planes=planes, stripe_out=max(caps), want=raws)
        launches = small.route_read("launch")
        print("arith chunks: %d blocks, planes %d: %r (at least %d)" % (len(streams), planes, launches, least))
        assert launches["in_order"] >= least and launches["side_by_side"] == 0, (launches, least)
        dc.route_read("launch")
        outs_one, st_one, _ = check(dc, streams, caps, planes=planes, stripe_out=max(caps), want=raws)
        assert dc.route_read("launch") == {"in_order": 1, "side_by_side": 0}
        assert outs == outs_one and st == st_one


# ---- planes -------------------------------------------------------------------------------------------------------
MANY = (33, 63, 64, 65, 128, 254, 255)


@functools.lru_cache(maxsize=None)
def wide_stripes():
    """(streams, raws): stripe blocks of 33 .. 255 planes - one byte a plane and one plane with two, three bytes a plane
    and a few with four, and about 4,000 bytes that N does not divide - beside N = 1 and unstriped blocks"""
    q = M.text("q40+dir")
    raws, orders = [], []
    for k, N in enumerate(MANY):
        big = 4001 if 4001 % N else 4003
        assert big % N
        for j, n in enumerate((N + 1, 3 * N + 7, big)):
            raws.append(q[17 * k:17 * k + n])
            orders.append((8, 9)[(k + j) & 1] | (N << 8))
    raws += [q[:300], q[:301], q[:700], q[:40], q[:1000]]
    orders += [8 | (1 << 8), 9 | (1 << 8), 1, 0, 65]
    streams = [M.compress(r, o) for r, o in zip(raws, orders)]
    assert all(bool(s[0] & M.X_STRIPE) == bool(o & 8) for s, o in zip(streams, orders))
    return streams, raws


def test_stripe_blocks_of_up_to_255_planes(dc):
    streams, raws = wide_stripes()
    caps = [len(r) for r in raws]
    check(dc, streams, caps, planes=255, stripe_out=max(caps), want=raws)


# ---- total_out_size, exactly ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_total_blocks():
    """(streams, raws): 40 blocks whose decoded pieces all have a size of 1 mod 16, so that each takes 15 bytes more of
    the stage arena than it decodes to: ten stripe blocks of four planes (64 a + 4 bytes), ten X_PACK blocks (the packed
    bytes 16 a + 1), ten X_CAT blocks and ten plain ones"""
    q, qv = M.text("q40+dir"), M.text("qvar")
    raws, orders = [], []
    for a in range(10):
        raws.append(_stripe_of(tuple(range(40, 72)), 64 * (a + 2) + 4, 900 + a, 3))     # (32 symbols a plane: none is packed)
        orders.append((8, 9)[a & 1] | (4 << 8))
        k = (2, 3, 4, 5, 9, 16, 2, 4, 12, 7)[a]
        per = 8 if k <= 2 else 4 if k <= 4 else 2
        raws.append(K.skewed(tuple(range(3, 3 + 9 * k, 9)), per * (16 * (a + 6) + 1), 40 + a, chain=6))
        orders.append(128 + (a & 1) + 64 * (a & 2 > 0))
        raws.append(qv[7 * a:7 * a + 16 * (a + 1) + 1])
        orders.append(32)
        raws.append(q[13 * a:13 * a + 16 * (3 * a + 4) + 1])
        orders.append((0, 1, 64, 65)[a & 3])
    streams = [M.compress(r, o) for r, o in zip(raws, orders)]
    for s, r, o in zip(streams, raws, orders):
        if o & 8:
            assert s[0] & M.X_STRIPE and len(r) % 64 == 4 and not any(f & M.X_PACK for f in _plane_flags(s))
        elif o & 128:
            assert s[0] & M.X_PACK and not s[0] & M.X_CAT, o
        else:
            assert bool(s[0] & M.X_CAT) == (o == 32) and len(r) % 16 == 1
    return streams, raws


def test_a_total_out_size_of_exactly_what_the_batch_decodes_to(dc):
    streams, raws = exact_total_blocks()
    caps = [len(r) for r in raws]
    check(dc, streams, caps, planes=4, stripe_out=max(caps), want=raws, total=sum(caps))
    # one byte short: the batch decodes to more than it announced, and the blocks that find the total spent are refused
    outs, st, _ = run_dev(dc, streams, caps, planes=4, stripe_out=max(caps), total=sum(caps) - 1)
    assert set(st) == {0, U}, st
    assert all(o == r for o, r, x in zip(outs, raws, st) if x == 0)
