"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle and the
committed golden vectors.  Everything here is bit-exact (integer/byte work)."""
import base64
import json
import os

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

GOLD = datagen.GOLDEN
FIXTURES = sorted(os.listdir(os.path.join(GOLD, "r4x16")))
# every order byte of the reference interface; X_STRIPE (8, 9, N<<8) goes through the host entry
# points, which expand a stripe block into a device batch of its planes
DEVICE_ORDERS = {0, 1, 16, 17, 32, 33, 64, 65, 128, 129, 192, 193, 0xd1}
STRIPE_ORDERS = [8, 9, 0x48, 0xc9, (2 << 8) | 9, (3 << 8) | 0xc9, (5 << 8) | 8]


# Every test of this module runs twice: with the short-step ("direct") rows that small batches take by default, and with
# them switched off, so that the compressed rows (u16 search trees, packed 10/11-bit rows) stay covered by the same cases.
@pytest.fixture(scope="module", params=["short-step", "compressed-rows"])
def H(request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    from conftest import _Options
    from htscodecs_amd import codec
    o = _Options()
    for k in ("dec_direct", "enc_direct"):
        o.set(k, 1 if request.param == "short-step" else 0)
    codec.set_option("route_count", 1)                     # the thread context's read-out: checked at the end of the pass
    for w in ("encode", "decode"):
        codec.route_read(w)
    yield htscodecs_amd
    o.restore()
    try:
        _route_pass_check(request.param, codec)
    finally:
        codec.set_option("route_count", 0)


def _route_pass_check(param, codec):
    """What the thread context's host batches of the module ran on (option route_count): the "compressed-rows" pass must
    not have touched the short-step kinds, and must have run the compressed rows; the "short-step" pass must have run the
    short-step rows."""
    dec, enc = codec.route_read("decode"), codec.route_read("encode")
    compressed_dec = dec["l1"] + dec["l2"] + dec["l3"] + dec["l4"] + dec["l5"]
    if param == "compressed-rows":
        assert dec["direct"] == 0 and enc["records"] == 0, (dec, enc)
        assert compressed_dec > 0 and enc["u16"] + enc["packed"] > 0, (dec, enc)
    else:
        assert dec["direct"] > 0, dec


def _fixture(fn):
    name, order = fn.rsplit(".", 1)
    with open(os.path.join(GOLD, "r4x16", fn), "rb") as f:
        comp = f.read()
    return name, int(order), comp, datagen.base_text(name).tobytes()


def _supported(order):
    return True


SUPPORTED_FIXTURES = [f for f in FIXTURES if _supported(int(f.rsplit(".", 1)[1]))]


@pytest.mark.parametrize("fn", SUPPORTED_FIXTURES)
def test_fixture_decode(H, fn):
    name, order, comp, plain = _fixture(fn)
    got = H.rans_uncompress_4x16(comp)
    assert got is not None
    assert got == plain


@pytest.mark.parametrize("fn", SUPPORTED_FIXTURES)
def test_fixture_encode_bit_exact(H, fn):
    name, order, comp, plain = _fixture(fn)
    got = H.rans_compress_4x16(plain, order)
    assert got is not None
    assert got == comp


def test_edge_vectors(H, oracle):
    with open(os.path.join(GOLD, "edge.json")) as f:
        cases = [c for c in json.load(f)["cases"] if _supported(c["order"]) and c["n"] <= 1 << 20]
    datas = [datagen.make(c["in"]).tobytes() for c in cases]
    enc, st = H.compress_batch(datas, [c["order"] for c in cases])
    bad = []
    for c, d, e, s in zip(cases, datas, enc, st):
        want = base64.b64decode(c["out"]) if "out" in c else oracle.compress(d, c["order"])
        if e != want:
            bad.append((c["in"], c["order"], s, None if e is None else len(e), len(want)))
    assert not bad, bad[:10]
    # decode what the reference produced
    comps = [base64.b64decode(c["out"]) if "out" in c else oracle.compress(d, c["order"])
             for c, d in zip(cases, datas)]
    dec, st = H.uncompress_batch(comps, [len(d) for d in datas])
    bad = [(c["in"], c["order"], s) for c, d, x, s in zip(cases, datas, dec, st) if x != d]
    assert not bad, bad[:10]


def _random_inputs(rs, count, max_n=70000):
    out = []
    for _ in range(count):
        kind = rs.randint(0, 6)
        n = int(rs.choice([rs.randint(0, 64), rs.randint(64, 3000), rs.randint(3000, max_n)]))
        seed = int(rs.randint(1, 1 << 30))
        if kind == 0:
            a = datagen.rand(n, seed, int(rs.randint(1, 257)), 0)
        elif kind == 1:
            a = datagen.runs(n, int(rs.randint(1, 40)), int(rs.randint(2, 60)), seed, 30)
        elif kind == 2:
            w = rs.random_sample(int(rs.randint(2, 256))) ** int(rs.randint(1, 12))
            a = datagen.weighted(n, w + 1e-9, seed)
        elif kind == 3:
            a = datagen.tile(str(rs.choice(["q4", "q8", "q40+dir", "qvar"])), n, 0, seed)
        elif kind == 4:
            a = datagen.markov(min(n, 20000), int(rs.randint(2, 200)), seed, 0, float(rs.random_sample()))
        else:
            a = datagen.const(n, int(rs.randint(0, 256)))
        out.append(a.tobytes())
    return out


def test_random_differential_vs_oracle(H, oracle):
    rs = np.random.RandomState(4242)
    datas = _random_inputs(rs, 300)
    orders = [int(rs.choice(sorted(DEVICE_ORDERS) + STRIPE_ORDERS)) for _ in datas]
    enc, st = H.compress_batch(datas, orders)
    bad = []
    for d, o, e, s in zip(datas, orders, enc, st):
        want = oracle.compress(d, o)
        if e != want:
            bad.append((len(d), o, s, None if e is None else len(e), len(want)))
    assert not bad, bad[:10]
    comps = [oracle.compress(d, o) for d, o in zip(datas, orders)]
    dec, st = H.uncompress_batch(comps, [len(d) for d in datas])
    bad = [(len(d), o, s) for d, o, x, s in zip(datas, orders, dec, st) if x != d]
    assert not bad, bad[:10]


def test_device_resident_batch(H, oracle):
    """*_dev entry points on torch tensors: 96 blocks, mixed q4/q8/q40 tiles, ragged sizes."""
    import torch
    dc = H.DeviceCodec(0)
    names = ["q4", "q8", "q40+dir"]
    sizes = [65536, 40000, 65536 + 3, 1 << 17]
    blocks = [datagen.tile(names[b % 3], sizes[b % 4], b) for b in range(96)]
    for order in (1, 0):
        in_off = np.cumsum([0] + [(len(b) + 255) // 256 * 256 for b in blocks])[:-1].astype(np.int64)
        in_size = np.array([len(b) for b in blocks], dtype=np.int32)
        arena = np.zeros(int(in_off[-1]) + ((len(blocks[-1]) + 255) // 256 * 256), dtype=np.uint8)
        for b, off in zip(blocks, in_off):
            arena[off:off + len(b)] = b
        caps = np.array([H.rans_compress_bound_4x16(len(b), order) for b in blocks], dtype=np.int32)
        out_off = np.cumsum([0] + [(int(c) + 255) // 256 * 256 for c in caps])[:-1].astype(np.int64)
        dev = dc.dev
        d_in = torch.from_numpy(arena).to(dev)
        d_out = torch.zeros(int(out_off[-1]) + int(caps[-1]) + 256, dtype=torch.uint8, device=dev)
        t = lambda a: torch.from_numpy(a).to(dev)
        d_in_off, d_in_size, d_out_off, d_caps = t(in_off), t(in_size), t(out_off), t(caps)
        d_osz = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
        d_st = torch.full((len(blocks),), -1, dtype=torch.int32, device=dev)
        dc.compress(d_in, d_in_off, d_in_size, d_out, d_out_off, d_caps, d_osz, d_st, order, int(in_size.max()))
        torch.cuda.synchronize()
        assert (d_st == 0).all(), d_st.tolist()
        osz = d_osz.cpu().numpy()
        comp = d_out.cpu().numpy()
        for i, b in enumerate(blocks):
            want = oracle.compress(b.tobytes(), order)
            got = comp[out_off[i]:out_off[i] + osz[i]].tobytes()
            assert got == want, (i, order, len(got), len(want))
        # decode in place on the device: compressed slots -> new arena
        d_dec = torch.zeros_like(d_in)
        d_dcap = t(in_size.copy())
        d_dsz = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
        d_dst = torch.full((len(blocks),), -1, dtype=torch.int32, device=dev)
        dc.uncompress(d_out, d_out_off, d_osz, d_dec, d_in_off, d_dcap, d_dsz, d_dst,
                      int(osz.max()), int(in_size.max()))
        torch.cuda.synchronize()
        assert (d_dst == 0).all(), d_dst.tolist()
        assert (d_dsz.cpu().numpy() == in_size).all()
        dec = d_dec.cpu().numpy()
        for b, off in zip(blocks, in_off):
            assert (dec[off:off + len(b)] == b).all()


def test_full_size_blocks_roundtrip(H, oracle):
    """1 MiB blocks (BASELINE.json size): sizes must equal the reference's published sizes (order 193 =
    O1|PACK|RLE: 67,051 / 216,606 for q4 / q8), block 0 must match the md5 the real reference produced
    (tests/golden/edge.json), EVERY block is compared byte-for-byte with the oracle, and the round trip must be
    the identity."""
    import hashlib
    want = {("q4", 0): 80768, ("q8", 0): 236614, ("q40+dir", 0): 526965,
            ("q4", 1): 74990, ("q8", 1): 224009, ("q40+dir", 1): 507704,
            ("q4", 193): 67051, ("q8", 193): 216606, ("q40+dir", 193): 507704}
    with open(os.path.join(GOLD, "edge.json")) as f:
        md5 = {(c["in"][1], c["order"]): (c["md5"], c["len"]) for c in json.load(f)["cases"]
               if c["in"][0] == "tile" and c["n"] == 1 << 20 and c["in"][3:] == [0, 0]}
    datas, orders = [], []
    for (name, order) in want:
        for blk in range(4):
            datas.append(datagen.tile(name, 1 << 20, blk).tobytes())
            orders.append(order)
    enc, st = H.compress_batch(datas, orders)
    assert all(s == 0 for s in st), st
    for k, (name, order) in enumerate(want):
        assert len(enc[4 * k]) == want[(name, order)], (name, order, len(enc[4 * k]))
        assert (hashlib.md5(enc[4 * k]).hexdigest(), len(enc[4 * k])) == md5[(name, order)], (name, order)
        for blk in range(4):
            assert enc[4 * k + blk] == oracle.compress(datas[4 * k + blk], order), (name, order, blk)
    dec, st = H.uncompress_batch(enc, [len(d) for d in datas])
    assert all(s == 0 for s in st), st
    assert all(a == b for a, b in zip(dec, datas))


def test_damaged_streams_do_not_crash(H, oracle):
    rs = np.random.RandomState(99)
    datas = _random_inputs(rs, 60, max_n=20000)
    bads, caps, refs = [], [], []
    for d in datas:
        order = int(rs.choice([0, 1, 65, 129, 193]))
        comp = bytearray(oracle.compress(d, order))
        for _ in range(5):
            bad = bytearray(comp)
            mode = rs.randint(0, 3)
            if mode == 0 and len(bad) > 3:
                p = int(rs.randint(min(6, len(bad) - 1), len(bad)))
                bad[p] ^= int(rs.randint(1, 256))
            elif mode == 1:
                bad = bad[:int(rs.randint(1, len(bad) + 1))]
            else:
                p = int(rs.randint(0, len(bad)))
                bad[p] ^= 1 << int(rs.randint(0, 8))
            if bad[0] & 0x08:
                continue                      # flipped into STRIPE: handled by the host entry points
            cap = len(d) + 64
            bads.append(bytes(bad))
            caps.append(cap)
            refs.append(oracle.uncompress(bytes(bad), capacity=cap, out_size_hint=cap))
    dec, st = H.uncompress_batch(bads, caps)
    agree = 0
    for x, s, r in zip(dec, st, refs):
        if r is None:
            assert x is None and s != 0        # whatever the oracle rejects, the device rejects
        elif x is not None:
            assert x == r                      # accepted by both: identical bytes
            agree += 1
        else:
            assert s in (6, 7, 8)              # documented stricter cases (UNSUPPORTED, CONTEXT, RLE varint > 64 B)
    assert agree > 20


def test_cli_mirrors_reference_test_script(H, tmp_path):
    """tests/rans4x16.test:8-30 with the rebuilt CLI: round trip + decode of every committed
    fixture, and (stronger than the reference script) the encoder output equals the fixture."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "tools", "rans4x16pr_hip")
    if not os.path.exists(cli):
        pytest.skip("tools/rans4x16pr_hip not built")
    for fn in FIXTURES:
        name, order = fn.rsplit(".", 1)
        src = os.path.join(GOLD, "dat", name + ".nl")
        comp, back = str(tmp_path / "c"), str(tmp_path / "u")
        subprocess.run([cli, "-r", "-o" + order, src, comp], check=True)
        with open(comp, "rb") as f, open(os.path.join(GOLD, "r4x16", fn), "rb") as g:
            assert f.read() == g.read(), fn
        subprocess.run([cli, "-r", "-d", os.path.join(GOLD, "r4x16", fn), back], check=True)
        with open(back, "rb") as f, open(src, "rb") as g:
            assert f.read() == g.read(), fn
    # framed (non -r) mode round trip on one file
    subprocess.run([cli, "-o193", os.path.join(GOLD, "dat", "q8.nl"), str(tmp_path / "f")], check=True)
    subprocess.run([cli, "-d", str(tmp_path / "f"), str(tmp_path / "g")], check=True)
    with open(tmp_path / "g", "rb") as f, open(os.path.join(GOLD, "dat", "q8.nl"), "rb") as g:
        assert f.read() == g.read()


def test_device_batch_unaligned_offsets_and_edge_sizes(H, oracle):
    """*_dev with blocks at odd byte offsets, zero-length and tiny blocks, a 5 MiB block, per-block
    orders, and one slot whose capacity is too small (must fail alone with CAPACITY)."""
    import torch
    dc = H.DeviceCodec(0)
    dev = dc.dev
    sizes = [0, 1, 7, 8, 9, 63, 64, 65, 4097, 65537, 5 * (1 << 20) + 3, 1000, 12345]
    names = ["q4", "q8", "q40+dir", "qvar"]
    orders = [1, 0, 193, 65, 1, 129, 0, 1, 193, 1, 1, 64, 1]
    blocks = [datagen.tile(names[i % 4], s, i) for i, s in enumerate(sizes)]
    in_off, pos = [], 1                                   # odd offsets on purpose
    for b in blocks:
        in_off.append(pos)
        pos += len(b) + 3 + (len(b) & 1)
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for b, off in zip(blocks, in_off):
        arena[off:off + len(b)] = b
    caps = [H.rans_compress_bound_4x16(len(b), o) for b, o in zip(blocks, orders)]
    caps[3] -= 100                                        # too small on purpose
    out_off, pos = [], 3
    for c in caps:
        out_off.append(pos)
        pos += c + 5
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).to(dev)
    d_in = torch.from_numpy(arena).to(dev)
    d_out = torch.zeros(pos + 64, dtype=torch.uint8, device=dev)
    d_in_off, d_in_size = t(in_off, np.int64), t(sizes, np.int32)
    d_out_off, d_caps, d_ord = t(out_off, np.int64), t(caps, np.int32), t(orders, np.int32)
    d_osz = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
    d_st = torch.full((len(blocks),), -1, dtype=torch.int32, device=dev)
    dc.compress(d_in, d_in_off, d_in_size, d_out, d_out_off, d_caps, d_osz, d_st, 0, max(sizes), d_order=d_ord)
    torch.cuda.synchronize()
    st, osz, comp = d_st.cpu().numpy(), d_osz.cpu().numpy(), d_out.cpu().numpy()
    assert st[3] == 1 and osz[3] == 0
    for i, (b, o) in enumerate(zip(blocks, orders)):
        if i == 3:
            continue
        assert st[i] == 0, (i, st[i])
        assert comp[out_off[i]:out_off[i] + osz[i]].tobytes() == oracle.compress(b.tobytes(), o), (i, o)
    # decode the good ones back to odd offsets
    keep = [i for i in range(len(blocks)) if i != 3]
    d_dec = torch.zeros_like(d_in)
    dsz = torch.zeros(len(keep), dtype=torch.int32, device=dev)
    dst = torch.full((len(keep),), -1, dtype=torch.int32, device=dev)
    dc.uncompress(d_out, t([out_off[i] for i in keep], np.int64), t([int(osz[i]) for i in keep], np.int32),
                  d_dec, t([in_off[i] for i in keep], np.int64), t([sizes[i] for i in keep], np.int32),
                  dsz, dst, int(osz.max()), max(sizes))
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all(), dst.tolist()
    dec = d_dec.cpu().numpy()
    for i in keep:
        assert (dec[in_off[i]:in_off[i] + sizes[i]] == blocks[i]).all(), i


def test_host_api_from_threads(H, oracle):
    """The five entry points are re-entrant: four host threads, each with its own lazily
    created context, must all produce reference bytes."""
    from concurrent.futures import ThreadPoolExecutor
    datas = [datagen.tile("q8", 30000 + 1000 * i, i).tobytes() for i in range(16)]

    def work(i):
        c = H.rans_compress_4x16(datas[i], i % 2)
        return c == oracle.compress(datas[i], i % 2) and H.rans_uncompress_4x16(c) == datas[i]

    with ThreadPoolExecutor(4) as ex:
        assert all(ex.map(work, range(16)))


@pytest.mark.gpu
def test_many_small_blocks_span_several_shares(H, oracle):
    """The chain kernels are persistent: a grid of as many workgroups as are resident walks the batch in
    shares.  70,000 small blocks of three alphabets (three LDS size classes) and per-block orders 0/1
    make every class take more than one share for the small classes; all outputs are compared with the
    oracle, and the round trip must be the identity."""
    rs = np.random.RandomState(99)
    names = ["q4", "q8", "q40+dir"]
    n = 70000
    datas, orders = [], []
    for b in range(n):
        size = int(rs.randint(60, 420))
        datas.append(datagen.tile(names[b % 3], size, b % 97).tobytes())
        orders.append(int(rs.randint(0, 2)))
    enc, st = H.compress_batch(datas, orders)
    assert all(s == 0 for s in st)
    bad = [(i, len(datas[i]), orders[i]) for i in range(n) if enc[i] != oracle.compress(datas[i], orders[i])]
    assert not bad, bad[:10]
    dec, st = H.uncompress_batch(enc, [len(d) for d in datas])
    assert all(s == 0 for s in st)
    assert all(a == b for a, b in zip(dec, datas))


def test_alphabet_sizes_at_the_tree_depth_boundaries(H, oracle):
    """The decoder's lookup tree has 2, 3 or 4 levels (<= 50, <= 150, <= 256 symbols) and two-level rows
    lose their last dword unless the alphabet is a multiple of ten: alphabets around every boundary, both
    orders, uniform and skewed, must round-trip bit-exactly."""
    rs = np.random.RandomState(5150)
    datas, orders = [], []
    # (round 2: plus the packed-row boundaries - decode rows of 1..4 groups of twelve for 13..48 symbols, encode bit
    #  streams for 20..64 symbols; order-1 alphabets gain byte 0, hence the neighbours on both sides)
    for nsym in (1, 2, 9, 10, 11, 12, 13, 14, 19, 20, 21, 23, 24, 25, 35, 36, 37, 39, 40, 41, 46, 47, 48, 49, 50, 51, 52, 62, 63, 64, 65,
                 89, 90, 91, 119, 120, 121, 149, 150, 151, 152, 200, 255, 256):
        for order in (0, 1):
            n = 30000 + int(rs.randint(0, 7))
            datas.append(datagen.rand(n, int(rs.randint(1, 1 << 30)), nsym, int(rs.randint(0, 257 - nsym))).tobytes())
            orders.append(order)
            w = [int(rs.randint(1, 3000)) for _ in range(nsym)]
            datas.append(datagen.weighted(n, w, int(rs.randint(1, 1 << 30))).tobytes())
            orders.append(order)
    enc, st = H.compress_batch(datas, orders)
    assert all(s == 0 for s in st), st
    bad = [(len(set(d)), o) for d, o, e in zip(datas, orders, enc) if e != oracle.compress(d, o)]
    assert not bad, bad
    dec, st = H.uncompress_batch(enc, [len(d) for d in datas])
    assert all(s == 0 for s in st), st
    bad = [(len(set(d)), o) for d, o, x in zip(datas, orders, dec) if x != d]
    assert not bad, bad


def test_host_batch_pipeline_matches_single_pass(H, oracle, opts):
    """Large host batches go through the staged pipeline (pinned bounce buffers, copier threads, slabs on
    several lanes: r4x16_host.hip run_pipelined).  Force that route on a small batch with everything awkward
    in it: empty and tiny blocks, a block larger than a bounce buffer, per-block orders, blocks that must
    fail on decode - and require reference bytes and the same statuses as the single-pass route."""
    opts.set("host_pipe_mb", 1)
    opts.set("host_slab_min_mb", 1)
    opts.set("host_threads", 5)
    opts.set("host_lanes", 3)
    rs = np.random.RandomState(4242)
    datas = _random_inputs(rs, 120, max_n=300000)
    datas += [b"", b"x", datagen.tile("q40+dir", 9 * (1 << 20) + 13, 3).tobytes(), b"", datagen.tile("q4", 1 << 20, 1).tobytes()]
    datas += _random_inputs(rs, 60, max_n=100000)
    orders = [int(rs.choice(sorted(DEVICE_ORDERS))) for _ in datas]
    want = [oracle.compress(d, o) for d, o in zip(datas, orders)]
    for pack in (1, 0):                     # results gathered on the device / copied from their slots one by one
        opts.set("host_pack", pack)
        enc, st = H.compress_batch(datas, orders)
        bad = [(i, len(d), o) for i, (d, o, e, w) in enumerate(zip(datas, orders, enc, want)) if e != w]
        assert not bad, (pack, bad[:10])
        got, chosen, st = H.compress_best_batch(datas[:60], [0, 1, 65, 193])
        for d, g in zip(datas[:60], got):
            assert g == min((oracle.compress(d, m) for m in [0, 1, 65, 193]), key=len)
    # decode, with some streams damaged so that statuses differ per block
    comps = list(want)
    damaged = set(int(i) for i in rs.choice(len(comps), 25, replace=False) if len(comps[i]) > 40)
    for i in damaged:
        b = bytearray(comps[i]); b[1] ^= 0x55; b = b[:len(b) // 2]; comps[i] = bytes(b)
    caps = [len(d) for d in datas]
    dec, st = H.uncompress_batch(comps, caps)
    opts.set("host_pipe_mb", 0)
    dec1, st1 = H.uncompress_batch(comps, caps)
    assert list(st) == list(st1)
    assert dec == dec1
    for i, (d, x) in enumerate(zip(datas, dec)):
        if i not in damaged:
            assert x == d, i


def test_compress_best_keeps_what_the_reference_loop_keeps(H, oracle):
    """tokenise_name3.c:1246-1300 compress(): methods tried in order, a later one must be strictly smaller
    to replace the best so far, X_STRIPE methods skipped when the size is not a multiple of 4.  The one-call
    form must deliver the same bytes and the same method, for the reference's own method tables."""
    rs = np.random.RandomState(77)
    datas = _random_inputs(rs, 90, max_n=40000) + [b"", b"abc", b"A" * 24, datagen.tile("q4", 200000, 2).tobytes()]
    for methods in ([0, 128], [0, 192 + 8], [0, 1, 129, 65, 193, 193 + 8], [0, 1, 128, 129, 64, 65, 192, 193, 193 + 8], [1]):
        got, chosen, st = H.compress_best_batch(datas, methods)
        for i, d in enumerate(datas):
            best, best_m = None, None
            for m in methods:
                if len(d) % 4 != 0 and (m & 8):
                    continue
                c = oracle.compress(d, m)
                if best is None or len(c) < len(best):
                    best, best_m = c, m
            assert st[i] == 0, (i, len(d), methods)
            assert chosen[i] == best_m, (i, len(d), methods, chosen[i], best_m)
            assert got[i] == best, (i, len(d), methods)
            assert H.rans_uncompress_4x16(got[i], len(d)) == d


def test_pack_codes_outside_the_listed_symbols_decode_to_zero(H, oracle):
    """rANS_static4x16pr.c:1524: `uint8_t map[16] = {0}` - a damaged X_PACK stream whose nibbles exceed the
    symbol count decodes those positions to byte 0 (found by tests/soak/fuzz_damaged_gpu.py, seed 909)."""
    bad = bytes.fromhex("a0150800010203040506070b7150338022737671141307")
    want = oracle.uncompress(bad, capacity=64, out_size_hint=64)
    assert want == bytes.fromhex("010700050303000002020307060701070401030107")
    # run a valid PACK block with a different, larger map through the same context first: stale entries must not leak
    first = oracle.compress(bytes(range(65, 81)) * 40, 128)
    dec, st = H.uncompress_batch([first, bad, bad], [640, 64, 64])
    assert st == [0, 0, 0] and dec[0] == bytes(range(65, 81)) * 40
    assert dec[1] == want and dec[2] == want


def test_batch_calls_from_several_threads(H, oracle):
    """A thread pool of callers, each with its own context (SURVEY §8b threading): three threads run pipelined
    host batches (>= 32 blocks each, so copier threads, lanes and packing are all in play) at the same time."""
    from concurrent.futures import ThreadPoolExecutor
    rs = np.random.RandomState(31337)
    jobs = []
    for t in range(3):
        datas = _random_inputs(rs, 150, max_n=60000)
        orders = [int(rs.choice(sorted(DEVICE_ORDERS) + STRIPE_ORDERS)) for _ in datas]
        jobs.append((datas, orders))

    def work(job):
        datas, orders = job
        ok = True
        for _ in range(2):
            enc, st = H.compress_batch(datas, orders)
            ok &= all(e == oracle.compress(d, o) for d, o, e in zip(datas, orders, enc))
            dec, st = H.uncompress_batch(enc, [len(d) for d in datas])
            ok &= dec == datas
        return ok

    with ThreadPoolExecutor(3) as ex:
        assert all(ex.map(work, jobs))


def test_batch_with_undersized_output_slots(H, oracle):
    """Caller-provided capacities below rans_compress_bound_4x16 fail those blocks (status 1, size 0) and nothing
    else - on the pipelined route too, where failed blocks take part in the device-side packing with length 0."""
    import ctypes as C
    from htscodecs_amd import codec
    L = H.load()
    ctx = codec._thread_ctx()
    rs = np.random.RandomState(808)
    datas = _random_inputs(rs, 80, max_n=30000)
    orders = [int(rs.choice([0, 1, 65, 193])) for _ in datas]
    n = len(datas)
    srcs = [np.frombuffer(d, dtype=np.uint8) for d in datas]
    caps = [L.rans_compress_bound_4x16(len(d), o) for d, o in zip(datas, orders)]
    small = set(range(3, n, 7))
    for i in small:
        caps[i] = max(1, caps[i] // 3)
    outs = [np.empty(max(c, 1), dtype=np.uint8) for c in caps]
    dummy = np.zeros(1, dtype=np.uint8)
    in_p = (C.c_void_p * n)(*[(s.ctypes.data if len(s) else dummy.ctypes.data) for s in srcs])
    out_p = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    in_sz = (C.c_uint * n)(*[len(s) for s in srcs])
    out_sz = (C.c_uint * n)(*caps)
    ords = (C.c_int * n)(*orders)
    status = (C.c_int * n)()
    rc = L.rans4x16_hip_compress_batch(ctx.h, n, in_p, in_sz, out_p, out_sz, ords, status)
    assert rc == len(small)
    for i in range(n):
        if i in small:
            assert status[i] == 1 and out_sz[i] == 0
        else:
            assert status[i] == 0 and outs[i][:out_sz[i]].tobytes() == oracle.compress(datas[i], orders[i]), i
