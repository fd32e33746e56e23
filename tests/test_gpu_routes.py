"""Which route a call took (include/rans4x16_hip.h: option route_count, rans4x16_hip_route_read), asserted next to the
bytes.  A row kind or an expansion route that is bit-wrong only at shapes nobody routes through it stays hidden from a
suite that checks bytes alone, so every case here checks the oracle's bytes both ways AND the read-out of the kinds the
call ran on: option toggles on one context on every path (device-resident, single-pass host batch, pipelined host
batch on lane contexts), the block counts at which the budgets switch row kinds, and alphabets at the kinds' edges."""
import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

RES_SHORT, RES_MID = 2, 4            # include/rans4x16_hip.h R4X16_RES_*


@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


def _nsym(a):
    """The decoder's compact alphabet of an order-1 stream: the bytes used, and byte 0 by rule."""
    return len(set(np.unique(a).tolist()) | {0})


def _dev_encode(dc, blocks, order):
    """Blocks through rans4x16_hip_compress_dev_sized; returns the compressed blocks."""
    import torch
    dev = dc.dev
    sizes = np.array([len(b) for b in blocks], dtype=np.int64)
    in_off = np.concatenate([[0], np.cumsum((sizes + 255) // 256 * 256)]).astype(np.int64)
    arena = np.zeros(int(in_off[-1]) + 256, dtype=np.uint8)
    for b, off in zip(blocks, in_off):
        arena[off:off + len(b)] = b
    caps = np.array([dc.L.rans_compress_bound_4x16(int(s), order) for s in sizes], dtype=np.int64)
    out_off = np.concatenate([[0], np.cumsum((caps + 255) // 256 * 256)]).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_out = torch.zeros(int(out_off[-1]) + 256, dtype=torch.uint8, device=dev)
    osz = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
    st = torch.full((len(blocks),), -1, dtype=torch.int32, device=dev)
    dc.compress(t(arena), t(in_off[:-1]), t(sizes.astype(np.int32)), d_out, t(out_off[:-1]), t(caps.astype(np.int32)), osz, st,
                order, int(sizes.max()), total_in_size=int(sizes.sum()))
    torch.cuda.synchronize()
    st, osz, out = st.cpu().numpy(), osz.cpu().numpy(), d_out.cpu().numpy()
    assert (st == 0).all(), st[st != 0][:10]
    return [out[o:o + n].tobytes() for o, n in zip(out_off[:-1], osz)]


def _dev_decode(dc, comps, sizes):
    """Compressed blocks through rans4x16_hip_uncompress_dev_sized; returns the decoded blocks."""
    import torch
    dev = dc.dev
    csz = np.array([len(c) for c in comps], dtype=np.int64)
    in_off = np.concatenate([[0], np.cumsum((csz + 255) // 256 * 256)]).astype(np.int64)
    arena = np.zeros(int(in_off[-1]) + 256, dtype=np.uint8)
    for c, off in zip(comps, in_off):
        arena[off:off + len(c)] = np.frombuffer(c, dtype=np.uint8)
    sizes = np.array(sizes, dtype=np.int64)
    out_off = np.concatenate([[0], np.cumsum((sizes + 255) // 256 * 256)]).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_out = torch.zeros(int(out_off[-1]) + 256, dtype=torch.uint8, device=dev)
    osz = torch.zeros(len(comps), dtype=torch.int32, device=dev)
    st = torch.full((len(comps),), -1, dtype=torch.int32, device=dev)
    dc.uncompress(t(arena), t(in_off[:-1]), t(csz.astype(np.int32)), d_out, t(out_off[:-1]), t(sizes.astype(np.int32)), osz, st,
                  int(csz.max()), int(sizes.max()), total_out_cap=int(sizes.sum()))
    torch.cuda.synchronize()
    st, osz, out = st.cpu().numpy(), osz.cpu().numpy(), d_out.cpu().numpy()
    assert (st == 0).all(), st[st != 0][:10]
    return [out[o:o + n].tobytes() for o, n in zip(out_off[:-1], osz)]


# ---- option toggles on ONE context, on every path ----------------------------------------------------------------------
# Each option is set A, B, A on the same context; every call's read-out must show the route its setting selects.  The
# pipelined host batch runs on lane contexts that the first pipelined call of the context creates: they have to follow
# their parent's options at every call, not keep those of that first call.

def _toggle_data(option):
    """(blocks, order, fixed options) for a toggle: few blocks of 64 KiB - a batch far below one round of resident
    streams, which the budgets give the short-step kinds by default."""
    if option == "back_wg_per_cu":
        return [datagen.tile("q8", 65536, b) for b in range(40)], 65, {}
    if option == "dec_mid":
        return [datagen.tile("q40+dir", 65536, b) for b in range(40)], 1, {"dec_direct": 0}
    if option == "dec_short_ring":                         # 44 symbols with byte 0, 10-bit tables: an image of 3,168 bytes, which
        # fits the class of sixteen streams per wave with the short ring only (k_dec_classify; 45 and more fit neither way)
        return [datagen.rand(65536, 1 + b, 43, 33) for b in range(40)], 1, {"dec_direct": 0}
    return [datagen.tile("q40+dir", 65536, b) for b in range(40)], 1, {}


TOGGLES = {"dec_direct": (1, 0), "enc_direct": (1, 0), "back_wg_per_cu": (0, 99999), "dec_mid": (0, 8), "sched_concurrent": (1, 0),
           "dec_short_ring": (0, 1)}


def _check_route(option, value, path, enc, dec, exp, launch, nblk):
    compressed_dec = dec["l1"] + dec["l2"] + dec["l3"] + dec["l4"] + dec["l5"]
    if option == "dec_direct":
        if value:
            assert dec["direct"] == nblk and compressed_dec == 0, dec
        else:
            assert dec["direct"] == 0 and compressed_dec == nblk, dec
    elif option == "enc_direct":
        if value:
            assert enc["records"] >= nblk and enc["packed"] == 0, enc
        else:
            assert enc["records"] == 0 and enc["packed"] + enc["u16"] >= nblk, enc
    elif option == "back_wg_per_cu":
        if value:
            assert exp == {"wave": 0, "workgroup": nblk}, exp
        else:
            assert exp == {"wave": nblk, "workgroup": 0}, exp
    elif option == "dec_mid":
        assert dec["direct"] == 0, dec
        if value:
            assert dec["mid"] == nblk and compressed_dec == 0, dec
        else:
            assert dec["mid"] == 0 and compressed_dec == nblk, dec
    elif option == "dec_short_ring":
        # every payload stream (the launch that decodes nested order-1 tables is not counted)
        assert dec["direct"] == 0 and dec["mid"] == 0, dec
        if value:
            assert dec["short_ring"] == nblk and dec["l1"] == 0, dec
        else:
            assert dec["l1"] == nblk and dec["short_ring"] == 0, dec
    elif option == "sched_concurrent":
        # the classes of a call side by side on the context's side streams; a pipeline lane has none (its lanes are the
        # pipeline's concurrency), so a pipelined batch is in stream order either way
        assert launch["in_order"] + launch["side_by_side"] >= 2, launch
        if value and path != "pipelined":
            assert launch["side_by_side"] >= 2 and launch["in_order"] == 0, launch
        else:
            assert launch["side_by_side"] == 0, launch
    if option != "back_wg_per_cu":
        assert sum(exp.values()) == nblk, exp


@pytest.mark.parametrize("path", ["device", "single-pass", "pipelined"])
@pytest.mark.parametrize("option", list(TOGGLES))
def test_option_toggles_follow_on_every_path(H, oracle, opts, option, path):
    from htscodecs_amd import codec
    blocks, order, fixed = _toggle_data(option)
    want = [oracle.compress(b.tobytes(), order) for b in blocks]
    nblk = len(blocks)
    if path == "device":
        dc = H.DeviceCodec(0)
        setopt, read = dc.set_option, dc.route_read
        setopt("route_count", 1)
    else:
        setopt, read = opts.set, codec.route_read
        setopt("route_count", 1)
        if path == "pipelined":                            # every host batch of this test through the lanes
            setopt("host_pipe_mb", 1)
            setopt("host_lanes", 3)
        else:                                              # never pipelined (40 blocks would be: 32 or more)
            setopt("host_pipe_mb", 0)
    for k, v in fixed.items():
        setopt(k, v)
    a, b = TOGGLES[option]
    for value in (a, b, a):
        setopt(option, value)
        for w in ("encode", "decode", "expand", "launch"):
            read(w)                                       # start afresh
        if path == "device":
            enc = _dev_encode(dc, blocks, order)
            dec = _dev_decode(dc, want, [len(x) for x in blocks])
        else:
            enc, st = H.compress_batch([x.tobytes() for x in blocks], [order] * nblk)
            assert all(s == 0 for s in st), st
            dec, st = H.uncompress_batch(want, [len(x) for x in blocks])
            assert all(s == 0 for s in st), st
        bad = [i for i in range(nblk) if enc[i] != want[i] or dec[i] != blocks[i].tobytes()]
        assert not bad, (option, value, path, bad[:10])
        _check_route(option, value, path, read("encode"), read("decode"), read("expand"), read("launch"), nblk)


def test_lanes_follow_a_smaller_workspace_ceiling(H, oracle, opts):
    """max_workspace_mb set small AFTER a pipelined batch: the next pipelined batch is walked in chunks on the lanes (more
    chain launches than slabs), and is still the oracle's bytes both ways."""
    from htscodecs_amd import codec
    opts.set("route_count", 1)
    opts.set("host_pipe_mb", 1)
    opts.set("host_lanes", 3)
    blocks = [datagen.tile("q40+dir", 65536, b) for b in range(40)]
    want = [oracle.compress(b.tobytes(), 1) for b in blocks]
    for ceiling in (None, 1):
        if ceiling:
            opts.set("max_workspace_mb", ceiling)
        codec.route_read("launch")
        enc, st = H.compress_batch([b.tobytes() for b in blocks], [1] * len(blocks))
        assert all(s == 0 for s in st) and enc == want
        dec, st = H.uncompress_batch(want, [len(b) for b in blocks])
        assert all(s == 0 for s in st) and dec == [b.tobytes() for b in blocks]
        launches = sum(codec.route_read("launch").values())
        if ceiling:
            assert launches >= 8, launches                  # several chunks per slab and direction
        else:
            assert launches <= 2 * 3, launches               # one launch per slab and direction


# ---- the block counts at which the budgets switch row kinds --------------------------------------------------------------
# r4x16_dec_direct_budget / r4x16_dec_mid_budget / r4x16_enc_direct_budget give a batch of n blocks the short-step kind while
# ceil(n / (CUs x rounds)) <= the kind's class residency (rans4x16_hip_residency with R4X16_RES_SHORT / _MID).  Exactly the
# largest such count, and one block more, through the device-resident calls (one chunk: one budget); the kind must flip
# exactly there and both sides must be the oracle's bytes.

def _boundary_case(name):
    if name == "q40-o1":
        return datagen.tile("q40+dir", 16384, 0), 10
    if name == "q8-o1":
        return datagen.tile("q8", 4096, 0), 10
    if name == "q4-o1":
        return datagen.tile("q4", 4096, 0), 10
    return datagen.weighted(1 << 18, [100000, 50000] + [1] * 28, 3), 12      # a 12-bit order-1 table


@pytest.mark.parametrize("knob", [("dec_direct", 1), ("dec_direct", 2), ("enc_direct", 1), ("enc_direct", 2), ("dec_mid", 1)],
                         ids=lambda k: f"{k[0]}={k[1]}")
@pytest.mark.parametrize("case", ["q40-o1", "q8-o1", "q4-o1", "12bit-o1"])
def test_budget_boundaries_flip_the_row_kind(H, oracle, case, knob):
    block, shift = _boundary_case(case)
    comp = oracle.compress(block.tobytes(), 1)
    i = 1
    while comp[i] & 0x80:
        i += 1
    assert comp[i + 1] >> 4 == shift, "the case's table precision is not the one it stands for"
    option, rounds = knob
    decode = option != "enc_direct"
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    dc.set_option(option, rounds)
    if option == "dec_mid":
        dc.set_option("dec_direct", 0)
    kind, flag = {"dec_direct": ("direct", RES_SHORT), "enc_direct": ("records", RES_SHORT), "dec_mid": ("mid", RES_MID)}[option]
    which = "decode" if decode else "encode"
    try:
        spc, _, cus = dc.residency(decode, _nsym(block), 1, shift, kind=flag)
        counts = [rounds * cus * spc, rounds * cus * spc + 1]
    except RuntimeError:
        spc, counts = None, [64]                          # the stream can never take this kind
    seen = []
    for n in counts:
        dc.route_read(which)
        if decode:
            got = _dev_decode(dc, [comp] * n, [len(block)] * n)
            bad = [j for j in range(n) if got[j] != block.tobytes()]
        else:
            got = _dev_encode(dc, [block] * n, 1)
            bad = [j for j in range(n) if got[j] != comp]
        assert not bad, (case, knob, n, bad[:10])
        seen.append(dc.route_read(which)[kind])
    if spc is None:
        assert seen == [0], (case, knob, seen)
        return
    n0 = counts[0]
    # at n0 every block's payload stream has the kind; one block more and every payload stream has left it (other streams
    # of a block - an order-1 table that travels as an order-0 stream - keep theirs: at most the new block's one more)
    assert seen[0] >= n0, (case, knob, n0, seen)
    assert seen[0] - n0 <= seen[1] <= seen[0] - n0 + 1, (case, knob, n0, seen)


# ---- alphabets at the edges of the row kinds --------------------------------------------------------------------------
# One order-1 block per call, 10-bit tables; the decoder's level from the alphabet size and the options.  The mid rows are
# defined for 13 .. 64 symbols (MID_MAX_NSYM), but their one LDS class holds 8,976 bytes per stream: 47 symbols take
# 8,640 with the word ring, 48 already 9,008 - so 48 .. 64 symbols keep the packed rows.

def _expected_level(nsym, direct, mid):
    if direct and nsym <= 128:
        return "direct"
    if mid and 13 <= nsym <= 47:
        return "mid"
    if 13 <= nsym <= 48:
        return "l1"
    if 49 <= nsym <= 96:
        return "l5"
    return "l2" if nsym <= 50 else "l3" if nsym <= 150 else "l4"


def test_mid_rows_class_holds_47_symbols(H):
    dc = H.DeviceCodec(0)
    assert dc.residency(True, 13, 1, 10, kind=RES_MID)[0] == 16
    assert dc.residency(True, 47, 1, 10, kind=RES_MID)[0] == 16
    for ns in (12, 48, 64, 65):
        with pytest.raises(RuntimeError):
            dc.residency(True, ns, 1, 10, kind=RES_MID)
    with pytest.raises(RuntimeError):
        dc.residency(True, 30, 1, 12, kind=RES_MID)        # 12-bit tables: never the mid rows


@pytest.mark.parametrize("ns", [12, 13, 47, 48, 49, 50, 51, 64, 65, 128, 129])
def test_alphabet_edges_land_on_their_level(H, oracle, opts, ns):
    from htscodecs_amd import codec
    a = datagen.rand(70000, ns, ns, 0)
    assert _nsym(a) == ns
    comp = oracle.compress(a.tobytes(), 1)
    opts.set("route_count", 1)
    for direct, mid in ((1, 0), (0, 0), (0, 1)):
        opts.set("dec_direct", direct)
        opts.set("dec_mid", mid)
        codec.route_read("decode")
        dec, st = H.uncompress_batch([comp], [len(a)])
        assert st == [0] and dec[0] == a.tobytes()
        enc, st = H.compress_batch([a.tobytes()], [1])
        assert st == [0] and enc[0] == comp
        got = {k: v for k, v in codec.route_read("decode").items() if v}
        assert got == {_expected_level(ns, direct, mid): 1}, (ns, direct, mid, got)
