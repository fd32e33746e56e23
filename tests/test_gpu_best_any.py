"""rans4x16_hip_compress_best_any_packed_dev, rans4x16_hip_uncompress_any_packed_dev and the two host-buffer calls
(include/rans4x16_hip.h part 2m) against the CPU expectation of best_any_cases.py: the reference's own fixtures, the small
family under both list orders with the route's counts, single-codec lists against the codecs' own calls, the dense arena's
rules in a patterned arena, a run in chunks, failures that stay local, the round trip and the host batches."""
import numpy as np
import pytest

import best_any_cases as B
import test_best_any_cpu as CPU
from test_gpu_confinement import pattern

pytestmark = pytest.mark.gpu

GUARD = 4096
PAIR_ORDERS = (0, 1, 64, 65, 128, 129, 192, 193, 8, 9)


@pytest.fixture(scope="module")
def dc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd.DeviceCodec(0)


class _Res:
    pass


def _inputs(dc, blocks, gap=7):
    import torch
    raw, offs = bytearray(b"\xee" * gap), []
    for b in blocks:
        offs.append(len(raw))
        raw += b + b"\xee" * gap
    d_in = torch.from_numpy(np.frombuffer(bytes(raw) + b"\0" * 64, dtype=np.uint8).copy()).to(dc.dev)
    return d_in, torch.tensor(offs, dtype=torch.int64, device=dc.dev), torch.tensor([len(b) for b in blocks], dtype=torch.int32, device=dc.dev)


def _run(dc, blocks, methods, capacity=None, sizing=False, max_in=None, call="any"):
    """One encode call on a patterned arena; call: "any", or the single-codec call "rans" / "arith" with untagged words."""
    import torch
    dev, n = dc.dev, len(blocks)
    d_in, in_off, in_size = _inputs(dc, blocks)
    r = _Res()
    r.alloc = sum(len(b) + 160 for b in blocks) + GUARD
    r.pat = pattern(r.alloc)
    d_out = None if sizing else torch.from_numpy(r.pat.copy()).to(dev)
    r.cap = 0 if sizing else (r.alloc - GUARD if capacity is None else capacity)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    osz, st, chosen = (torch.full((n,), -3, dtype=torch.int32, device=dev) for _ in range(3))
    fn = {"any": dc.compress_best_any_packed, "rans": dc.compress_best_packed, "arith": dc.arith_compress_best_packed}[call]
    if sizing and call == "rans":
        d_out = torch.zeros(1, dtype=torch.uint8, device=dev)
    dc.set_option("route_count", 1)
    try:
        dc.route_read("best_any")
        fn(d_in, in_off, in_size, d_out, off, osz, st, list(methods), max(map(len, blocks)) if max_in is None else max_in, chosen=chosen,
           total_in_size=sum(map(len, blocks)), out_capacity=r.cap)
        torch.cuda.synchronize()
        r.route = dc.route_read("best_any")
    finally:
        dc.set_option("route_count", 0)
    r.d_out, r.d_off, r.d_osz, r.d_chosen = d_out, off, osz, chosen
    r.arena = None if sizing else d_out.cpu().numpy()
    r.off, r.osz, r.st, r.chosen = off.cpu().tolist(), osz.cpu().tolist(), st.cpu().tolist(), chosen.cpu().tolist()
    return r


def _check(r, want, what):
    """Everything the call reports against the expectation [(chosen, stream or None, status, tie)]; every byte outside the
    blocks' ranges keeps the pattern."""
    need = [0] + np.cumsum([len(s) if s is not None else 0 for _, s, _, _ in want]).tolist()
    assert r.off == need, (what, r.off[:8], need[:8])
    mask = np.zeros(r.alloc, dtype=bool)
    for i, (m, s, status, _) in enumerate(want):
        tag = (what, i, r.st[i], r.osz[i], r.chosen[i], m, status)
        assert r.chosen[i] == m, tag
        if s is None:
            assert r.st[i] == status and r.osz[i] == 0, tag
        elif need[i + 1] > r.cap:
            assert r.st[i] == B.CAPACITY and r.osz[i] == 0, tag
        else:
            assert r.st[i] == 0 and r.osz[i] == len(s), tag
            mask[need[i]:need[i + 1]] = True
            assert r.arena[need[i]:need[i + 1]].tobytes() == s, tag
    if r.arena is not None:
        assert np.array_equal(r.arena[~mask], r.pat[~mask]), (what, "a byte outside the blocks' ranges changed")


def _census(want):
    """what R4X16_ROUTE_BEST_ANY counts of a one-chunk call with this expectation"""
    is_arith = lambda m: m >= 0 and m & B.CODEC_MASK == B.CODEC_ARITH
    return {"rans": sum(m >= 0 and not is_arith(m) for m, _, _, _ in want), "arith": sum(is_arith(m) for m, _, _, _ in want),
            "tie": sum(t for _, _, _, t in want), "failed": sum(m < 0 for m, _, _, _ in want), "chunks": 1}


# ---- the reference's fixtures -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,winner", [("q4", B.arith(193)), ("q8", B.arith(65)), ("q40+dir", B.arith(1)), ("qvar", B.arith(1))])
def test_every_fixture_order_of_both_codecs_gives_the_smallest_committed_file(dc, name, winner):
    orders = B.fixture_orders(name)
    methods = [B.rans(o) for o in orders] + [B.arith(o) for o in orders]
    want = B.expect_fixture(name, methods)
    assert want[0] == winner and want[1] == B.fixture_stream(name, winner)
    _check(_run(dc, [B.text(name)], methods), [want], name)


@pytest.mark.parametrize("name,order,codec", [("q4", 64, B.rans), ("q8", 64, B.rans), ("q8", 192, B.rans), ("q4", 1, B.arith), ("q8", 1, B.arith),
                                              ("q40+dir", 1, B.arith), ("qvar", 1, B.arith)])
def test_a_pair_list_gives_the_smaller_fixture_in_either_list_order(dc, name, order, codec):
    for methods in ([B.rans(order), B.arith(order)], [B.arith(order), B.rans(order)]):
        want = B.expect_fixture(name, methods)
        assert want[0] == codec(order) and not want[3]
        _check(_run(dc, [B.text(name)], methods), [want], (name, methods))


# ---- the small family ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", PAIR_ORDERS)
def test_the_small_family_in_one_batch_under_both_list_orders(dc, order):
    blocks = list(B.small_blocks())
    res = []
    for methods in ([B.rans(order), B.arith(order)], [B.arith(order), B.rans(order)]):
        want = [B.expect(b, methods) for b in blocks]
        r = _run(dc, blocks, methods)
        _check(r, want, methods)
        assert r.route == _census(want), (methods, r.route, _census(want))
        res.append((want, r))
    # on a tie the chosen tag flips with the list order; without one it does not
    (w0, r0), (w1, r1) = res
    ties = 0
    for i, b in enumerate(blocks):
        if w0[i][0] < 0:
            assert order & 8 and len(b) % 4 and r0.chosen[i] == r1.chosen[i] == -1 and r0.st[i] == r1.st[i] == B.UNSUPPORTED
        elif w0[i][3]:
            ties += 1
            assert r0.chosen[i] == B.rans(order) and r1.chosen[i] == B.arith(order), (i, r0.chosen[i], r1.chosen[i])
        else:
            assert r0.chosen[i] == r1.chosen[i], i
    assert ties >= 20


def test_the_routes_counts_over_the_family_are_the_helpers(dc):
    """every (block, order) of the family under its pair list, a call an order: the sums are best_any_cases.small_census's"""
    blocks = list(B.small_blocks())
    tot = dict.fromkeys(("rans", "arith", "tie", "failed", "chunks"), 0)
    for order in B.ORDERS:
        for k, v in _run(dc, blocks, [B.rans(order), B.arith(order)]).route.items():
            tot[k] += v
    ties, a_wins, r_wins = B.small_census()
    tied_to_rans = ties                                                # rANS stands first in every list: it takes every tie
    skipped = len(blocks) * len(B.ORDERS) - len(B.small_family())
    assert tot == {"rans": r_wins + tied_to_rans, "arith": a_wins, "tie": ties, "failed": skipped, "chunks": len(B.ORDERS)}, tot


# ---- single-codec lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec,orders", [("rans", (0, 1, 65, 193, 9)), ("arith", (0, 1, 65, 193, 9)), ("rans", (8, 9)), ("arith", (9,))])
def test_a_list_of_one_codec_gives_what_that_codecs_call_gives(dc, codec, orders):
    blocks = list(B.small_blocks()) + [B.text("q4")[:5000], B.text("q40+dir")[:3000]]
    tag = B.CODEC_ARITH if codec == "arith" else 0
    own = _run(dc, blocks, orders, call=codec)
    r = _run(dc, blocks, [tag | o for o in orders])
    assert r.off == own.off and r.osz == own.osz and r.st == own.st
    assert r.chosen == [c if c < 0 else tag | c for c in own.chosen]
    assert np.array_equal(r.arena, own.arena)
    assert r.route[codec] == sum(s == 0 for s in own.st) and r.route["failed"] == sum(s != 0 for s in own.st) and r.route["tie"] == 0


# ---- the dense arena's rules -----------------------------------------------------------------------------------------------
def test_the_sizing_pass_and_a_capacity_that_cuts_the_batch(dc):
    blocks = list(B.small_blocks())
    methods = [B.rans(1), B.arith(1), B.rans(64), B.arith(65)]
    want = [B.expect(b, methods) for b in blocks]
    r = _run(dc, blocks, methods)
    _check(r, want, "whole")
    s = _run(dc, blocks, methods, sizing=True)
    assert s.off == r.off and s.chosen == r.chosen and not any(s.osz)
    assert all(st == (B.CAPACITY if len(w[1]) else 0) for st, w in zip(s.st, want))
    mid = len(blocks) // 2
    assert r.osz[mid] > 1
    cut = _run(dc, blocks, methods, capacity=r.off[mid] + 1)
    _check(cut, want, "cut")
    assert cut.off == r.off and all(st == B.CAPACITY and sz == 0 for st, sz in zip(cut.st[mid:], cut.osz[mid:]))
    assert cut.st[:mid] == r.st[:mid] and cut.osz[:mid] == r.osz[:mid]


# ---- chunks -----------------------------------------------------------------------------------------------------------------
def test_a_run_in_chunks_gives_the_same_result(dc):
    rs = np.random.RandomState(11)
    texts = [B.text(n) for n in ("q4", "q8", "q40+dir")]
    blocks = []
    for i in range(64):
        t, n = texts[i % 3], int(rs.randint(1, 4097))
        at = int(rs.randint(0, len(t) - n))
        blocks.append(t[at:at + n])
    methods = [B.rans(0), B.arith(1), B.rans(65), B.arith(193), B.rans(9), B.arith(9)]
    want = [B.expect(b, methods) for b in blocks]
    whole = _run(dc, blocks, methods)
    _check(whole, want, "whole")
    assert whole.route["chunks"] == 1
    keep = dc.get_option("max_workspace_mb")
    plan = lambda: dc.best_any_chunk_blocks(len(blocks), methods, max(map(len, blocks)), sum(map(len, blocks)))
    assert plan() == len(blocks)
    try:
        dc.set_option("max_workspace_mb", 4)
        r = _run(dc, blocks, methods)
        per = plan()                                                   # (the arenas are as the run left them)
    finally:
        dc.set_option("max_workspace_mb", keep)
    chunks = -(-len(blocks) // per)
    assert chunks >= 2 and r.route["chunks"] == chunks, (per, chunks, r.route)
    _check(r, want, "chunks")
    assert np.array_equal(r.arena, whole.arena) and r.off == whole.off and r.chosen == whole.chosen
    assert {k: v for k, v in r.route.items() if k != "chunks"} == {k: v for k, v in whole.route.items() if k != "chunks"}


def test_the_planner_stays_within_the_batch_and_follows_the_ceiling(dc):
    CPU.check_planner(dc)


@pytest.mark.parametrize("what,k,methods,words", CPU.BAD_LISTS, ids=[b[0] for b in CPU.BAD_LISTS])
def test_a_bad_method_list_is_refused_before_anything_is_enqueued(dc, what, k, methods, words):
    CPU.check_bad_list(dc.ctx, what, k, methods, words)


# ---- failures stay local ----------------------------------------------------------------------------------------------------
def test_a_block_above_max_in_size_fails_alone(dc):
    blocks = list(B.small_blocks())[40:70]
    methods = [B.arith(1), B.rans(1), B.rans(64)]
    big = B.text("q8")[:3000]
    limit = max(map(len, blocks))
    assert limit < len(big)
    want = [B.expect(b, methods) for b in blocks]
    at = 11
    r = _run(dc, blocks[:at] + [big] + blocks[at:], methods, max_in=limit)
    _check(r, want[:at] + [(-1, None, B.UNSUPPORTED, False)] + want[at:], "above max_in_size")
    clean = _run(dc, blocks, methods, max_in=limit)
    assert r.osz[:at] + r.osz[at + 1:] == clean.osz and r.chosen[:at] + r.chosen[at + 1:] == clean.chosen
    assert r.arena[:r.off[-1]].tobytes() == clean.arena[:clean.off[-1]].tobytes()
    assert r.route["failed"] == 1


def test_stripe_methods_alone_on_a_size_that_is_no_multiple_of_four(dc):
    blocks = list(B.small_blocks())[60:96]
    odd = B.text("q4")[:1001]
    for methods in ([B.rans(9), B.arith(9)], [B.arith(8), B.rans(9 | (2 << 8))]):
        ok = [b for b in blocks if len(b) % 4 == 0]
        want = [B.expect(b, methods) for b in ok]
        at = 5
        r = _run(dc, ok[:at] + [odd] + ok[at:], methods)
        _check(r, want[:at] + [(-1, None, B.UNSUPPORTED, False)] + want[at:], methods)
        clean = _run(dc, ok, methods)
        assert r.arena[:r.off[-1]].tobytes() == clean.arena[:clean.off[-1]].tobytes() and r.route["failed"] == 1


# ---- round trip ---------------------------------------------------------------------------------------------------------------
def _decode(dc, d_in, in_off, in_size, method, sizes, max_out=None, nosz=None, capacity=None):
    import torch
    dev, n = dc.dev, in_size.numel()
    r = _Res()
    r.alloc = sum(sizes) + GUARD
    r.pat = pattern(r.alloc)
    d_out = torch.from_numpy(r.pat.copy()).to(dev)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    osz, st = (torch.full((n,), -3, dtype=torch.int32, device=dev) for _ in range(2))
    dc.ctx.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 4, 8192)
    try:
        dc.uncompress_any_packed(d_in, in_off, in_size, method, d_out, off, osz, st, int(in_size.max().item()) if n else 0,
                                 max(sizes) if max_out is None else max_out, nosz_size=nosz,
                                 out_capacity=r.alloc - GUARD if capacity is None else capacity)
        torch.cuda.synchronize()
    finally:
        dc.ctx.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 0, 0)
    r.arena, r.off, r.osz, r.st = d_out.cpu().numpy(), off.cpu().tolist(), osz.cpu().tolist(), st.cpu().tolist()
    return r


def _check_decoded(r, blocks, status, what):
    """status[i]: what block i must report; 0: its bytes.  The offsets are the scan of the sizes that were claimed."""
    mask = np.zeros(r.alloc, dtype=bool)
    for i, b in enumerate(blocks):
        tag = (what, i, r.st[i], r.osz[i], status[i])
        assert r.st[i] == status[i], tag
        if status[i] == 0:
            assert r.osz[i] == len(b) == r.off[i + 1] - r.off[i] and r.arena[r.off[i]:r.off[i + 1]].tobytes() == b, tag
            mask[r.off[i]:r.off[i + 1]] = True
        else:
            assert r.osz[i] == 0, tag
    assert np.array_equal(r.arena[~mask], r.pat[~mask]), (what, "a byte outside the blocks' ranges changed")


def test_the_mixed_arena_goes_straight_into_the_decoder(dc):
    blocks = list(B.small_blocks()) + [B.text("q4")[:4000], B.text("q8")[:4000]]
    methods = [B.rans(9), B.arith(9), B.rans(193), B.arith(65)]
    want = [B.expect(b, methods) for b in blocks]
    enc = _run(dc, blocks, methods)
    _check(enc, want, "encode")
    won = {m & B.CODEC_MASK for m, _, _, _ in want if m >= 0}
    assert won == {B.CODEC_RANS, B.CODEC_ARITH}
    # an empty block's stream decodes to nothing; a block without a stream (none here by the list: made below) is EMPTY
    sizes = [len(b) for b in blocks]
    r = _decode(dc, enc.d_out, enc.d_off, enc.d_osz, enc.d_chosen, sizes)
    assert r.off == [0] + np.cumsum(sizes).tolist()
    _check_decoded(r, blocks, [0] * len(blocks), "round trip")
    # max_out_size below the largest block's size refuses that block alone
    assert 0 < sum(n > 3999 for n in sizes) < len(sizes)
    r = _decode(dc, enc.d_out, enc.d_off, enc.d_osz, enc.d_chosen, sizes, max_out=3999)
    _check_decoded(r, blocks, [B.UNSUPPORTED if n > 3999 else 0 for n in sizes], "max_out_size")
    # a capacity that cuts the output: the blocks behind the cut are CAPACITY, the offsets stand
    cut = _decode(dc, enc.d_out, enc.d_off, enc.d_osz, enc.d_chosen, sizes, capacity=sum(sizes[:50]) + 1)
    assert cut.off == [0] + np.cumsum(sizes).tolist()
    _check_decoded(cut, blocks, [0 if sum(sizes[:i + 1]) <= sum(sizes[:50]) + 1 else B.CAPACITY for i in range(len(blocks))], "capacity")


def test_failed_blocks_decode_as_empty(dc):
    blocks = [b for b in B.small_blocks()][30:66]
    methods = [B.arith(9), B.rans(8)]
    want = [B.expect(b, methods) for b in blocks]
    failed = [i for i, w in enumerate(want) if w[0] < 0]
    assert failed and len(failed) < len(blocks)
    enc = _run(dc, blocks, methods)
    _check(enc, want, "encode")
    r = _decode(dc, enc.d_out, enc.d_off, enc.d_osz, enc.d_chosen, [len(b) for b in blocks])
    _check_decoded(r, blocks, [B.EMPTY if i in failed else 0 for i in range(len(blocks))], "failed blocks")
    assert all(r.off[i + 1] == r.off[i] for i in failed)


def test_an_x_nosz_stream_of_each_codec(dc):
    import torch
    data = B.text("q4")[:2000]
    streams = [B._rans_stream(data, 1 | 16), B._arith_stream(data, 1 | 16), B._rans_stream(data, 1), B._arith_stream(data, 0)]
    assert all(s[0] & 16 for s in streams[:2]) and not any(s[0] & 16 for s in streams[2:])
    d_in, in_off, in_size = _inputs(dc, streams)
    method = torch.tensor([B.rans(1 | 16), B.arith(1 | 16), B.rans(1), B.arith(0)], dtype=torch.int32, device=dc.dev)
    nosz = torch.tensor([2000, 2000, 7, 7], dtype=torch.int32, device=dc.dev)
    r = _decode(dc, d_in, in_off, in_size, method, [2000] * 4, nosz=nosz)
    _check_decoded(r, [data] * 4, [0] * 4, "with d_nosz_size")
    r = _decode(dc, d_in, in_off, in_size, method, [2000] * 4)
    _check_decoded(r, [data] * 4, [B.SIZE, B.SIZE, 0, 0], "without d_nosz_size")
    # a tag that is no candidate's
    method[2] = (2 << 24) | 1
    r = _decode(dc, d_in, in_off, in_size, method, [2000] * 4, nosz=nosz)
    _check_decoded(r, [data] * 4, [0, 0, B.UNSUPPORTED, 0], "an unknown tag")


def test_an_fqzcomp_tagged_block_is_no_candidate_of_these_calls(dc):
    """CODEC_FQZ is the quality calls' tag (part 2n): here the device says UNSUPPORTED at the claim, the block takes no room,
    its neighbours decode and the fqzcomp decoder is not run; the host batch says the same, not its own CAPACITY"""
    import torch
    import htscodecs_amd as H
    data = B.text("q4")[:2000]
    quals = bytes((7 * i + i // 9) % 41 for i in range(300))
    fqz_stream = H.fqz_compress(quals, [100] * 3, [0] * 3, 4, 0)[0]
    # the premise of the host half: byte 1, read as a size field (the second byte of varint(300)), claims no more than 300
    assert fqz_stream[:2] == bytes([0x80 | (300 >> 7), 300 & 0x7f]) and fqz_stream[1] == 44 <= 300
    streams = [B._rans_stream(data, 1), fqz_stream, B._arith_stream(data, 0), b""]
    methods = [B.rans(1), H.CODEC_FQZ | 0, B.arith(0), -1]
    blocks, want = [data, quals, data, b""], [0, B.UNSUPPORTED, 0, B.EMPTY]
    d_in, in_off, in_size = _inputs(dc, streams)
    method = torch.tensor(methods, dtype=torch.int32, device=dc.dev)
    dc.set_option("route_count", 1)
    try:
        dc.route_read("fqz")
        r = _decode(dc, d_in, in_off, in_size, method, [2000, 300, 2000, 8])
        route = dc.route_read("fqz")
    finally:
        dc.set_option("route_count", 0)
    _check_decoded(r, blocks, want, "an fqzcomp tag")
    assert r.off == [0, 2000, 2000, 4000, 4000] and r.off[2] == r.off[1]
    assert route == dict.fromkeys(route, 0), route
    back, st = H.uncompress_any_batch(streams, methods, [2000, 300, 2000, 8], ctx=dc.ctx)
    assert st == want and back == [data, None, data, None]


# ---- host buffers ---------------------------------------------------------------------------------------------------------------
def test_the_host_batches(dc):
    import htscodecs_amd as H
    blocks = list(B.small_blocks())[76:108]
    assert len(blocks) == 32
    methods = [B.rans(1), B.arith(1), B.arith(9), B.rans(192)]
    want = [B.expect(b, methods) for b in blocks]
    outs, chosen, status = H.compress_best_any_batch(blocks, methods, ctx=dc.ctx)           # out[i] == NULL: the library allocates
    assert outs == [w[1] for w in want] and chosen == [w[0] for w in want] and status == [0] * 32
    caps = [len(w[1]) + (i % 3) for i, w in enumerate(want)]
    short = 17
    caps[short] = len(want[short][1]) - 1
    outs2, chosen2, status2 = H.compress_best_any_batch(blocks, methods, caps=caps, ctx=dc.ctx)
    assert status2 == [B.CAPACITY if i == short else 0 for i in range(32)] and chosen2 == chosen
    assert outs2 == [None if i == short else w[1] for i, w in enumerate(want)]
    back, st = H.uncompress_any_batch(outs, chosen, [len(b) for b in blocks], ctx=dc.ctx)
    assert st == [0] * 32 and back == blocks
    caps = [len(b) + (i % 2) for i, b in enumerate(blocks)]
    small = max(range(32), key=lambda i: len(blocks[i]))
    caps[small] = len(blocks[small]) - 1
    back, st = H.uncompress_any_batch(outs, chosen, caps, ctx=dc.ctx)
    assert [s != 0 for s in st] == [i == small for i in range(32)] and all(b == blocks[i] for i, b in enumerate(back) if i != small)
    # exact capacities and one buffer a byte short in the middle: that block alone fails, the last ones included decode
    caps = [len(b) for b in blocks]
    caps[13] -= 1
    back, st = H.uncompress_any_batch(outs, chosen, caps, ctx=dc.ctx)
    assert st == [B.CAPACITY if i == 13 else 0 for i in range(32)], st
    assert back == [None if i == 13 else b for i, b in enumerate(blocks)]
    # a block that was never written
    back, st = H.uncompress_any_batch([b""] + outs[:3], [-1] + chosen[:3], [8] + [len(b) for b in blocks[:3]], ctx=dc.ctx)
    assert st == [B.EMPTY, 0, 0, 0] and back[1:] == blocks[:3]
