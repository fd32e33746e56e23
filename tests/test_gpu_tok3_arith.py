"""tok3 containers of the arith flavour (use_arith = 1) on the device, after rans4x16_hip_set_tok3_arith: the reference's 55
arith containers become their names through every decode entry point, one batch mixes both flavours, mode 0 keeps to
the rANS path; names become the reference's containers (levels 7 and 9, byte for byte) or the model's (levels 1, 3, 5)
through every encode entry point and decode back; damaged containers beside intact ones; the names tool."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import arith_enc_model as AE
import tok3_arith_model as TA
import tok3_model as M
import tok3_names_model as N
import test_gpu_tok3 as T3
import test_gpu_tok3_enc as TE
import test_gpu_tok3_host as TH
import test_gpu_tok3_names as TN
from test_gpu_confinement import pattern
from test_tok3_cpu import _descriptor_bytes

pytestmark = pytest.mark.gpu

DECODE, ENCODE = 1, 2
LEVELS = (1, 3, 5, 7, 9)


@pytest.fixture(scope="module")
def files():
    """[(key, block)]: the reference's 11 names files, in name order."""
    return sorted(N.names_files().items())


def _ref_of(fixtures, columns):
    files = N.names_files()
    out = []
    for name, buf in fixtures:
        w = M.walk(TA.cleared(buf))
        assert w.status == 0, name
        want = files[name.split(".")[0]].replace(b"\n", b"\0")
        starts = [0] + [i + 1 for i, ch in enumerate(want[:-1]) if ch == 0]
        out.append((name, buf, w, columns(buf, w), want, starts))
    return out


@pytest.fixture(scope="module")
def aref():
    """Per arith fixture what test_gpu_tok3_names.ref holds per rANS fixture: (name, container, walk, [bytes of every
    column], the names file with every line end a NUL, name starts)."""
    out = _ref_of(TA.fixtures(), TA.columns)
    assert len(out) == 55 and all(c is not None for _, _, _, c, _, _ in out)
    return out


@pytest.fixture(scope="module")
def dc(aref):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    d = htscodecs_amd.DeviceCodec(0)
    assert d.L.rans4x16_hip_set_dev_stripe_planes(d.ctx.h, 4, 2 * max(w.largest_col for _, _, w, _, _, _ in aref)) == 0
    assert d.set_tok3_arith(0) == 0                                     # the default
    yield d
    d.set_tok3_arith(0)
    assert d.L.rans4x16_hip_set_dev_stripe_planes(d.ctx.h, 0, 0) == 0


@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    from htscodecs_amd import codec
    htscodecs_amd.load()
    ctx = codec._Ctx()
    ctx.set_option("route_count", 1)
    return ctx


class _mode:
    """the mode of a context for a with-block; the setter's return values are checked on the way"""

    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        from htscodecs_amd import codec
        self.was = codec.set_tok3_arith(self.mode, self.ctx)

    def __exit__(self, *exc):
        from htscodecs_amd import codec
        assert codec.set_tok3_arith(self.was, self.ctx) == self.mode


def _routes(dc):
    return dc.route_read("arith"), dc.route_read("decode"), dc.route_read("arith_enc"), dc.route_read("encode")


# ---- decode -------------------------------------------------------------------------------------------------------
def test_the_setter(dc):
    assert dc.set_tok3_arith(3) == 0 and dc.set_tok3_arith(1) == 3 and dc.set_tok3_arith(0) == 1
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            dc.set_tok3_arith(bad)
    assert dc.set_tok3_arith(0) == 0


def test_unpack_then_names_of_all_arith_fixtures(dc, aref):
    import torch
    containers = [buf for _, buf, _, _, _, _ in aref]
    expect = [(w, cols) for _, _, w, cols, _, _ in aref]
    max_col = max(w.largest_col for w, _ in expect)
    dc.set_option("route_count", 1)
    try:
        _routes(dc)
        with _mode(dc.ctx, DECODE):
            u = T3._unpack(dc, containers, 64, max_col, sum(w.total for w, _ in expect))
        arith, rans, _, _ = _routes(dc)
    finally:
        dc.set_option("route_count", 0)
    assert T3._check_unpack(u, containers, expect, 64, "all arith") == 55
    plain = sum(c["kind"] == M.PLAIN for w, _ in expect for c in w.cols)
    assert plain > 1000 and sum(arith.values()) > 500 and not any(rans.values()), (arith, rans)     # (stored columns count nowhere)
    # the names of the columns the unpack left
    dev = dc.dev
    n = len(containers)
    d_cols = torch.from_numpy(u.arena.copy()).to(dev)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).astype(dt)).to(dev)
    total = sum(len(want) for _, _, _, _, want, _ in aref)
    r = TN._outputs(dev, n, total, 1000, None, False)
    dc.tok3_names(d_cols, up(u.cid, np.int32), up(u.coff, np.int64), up(u.csz.view(np.int32), np.int32), up(T3._i32(u.ncol), np.int32),
                  up(T3._i32(u.ls), np.int32), up(T3._i32(u.nr), np.int32), r.d_out, r.d_off, r.d_per[0], r.d_per[1], r.d_per[2],
                  64, 1000, 32, blk_status=up(T3._i32(u.st), np.int32), name_start=r.d_ns)
    TN._collect(r)
    assert TN._check(r, TN._expect_fixtures(aref, total), "unpack + names") == 55


def test_decode_names_dev_of_all_arith_fixtures(dc, aref):
    total = sum(len(want) for _, _, _, _, want, _ in aref)
    with _mode(dc.ctx, DECODE):
        r = TN._decode_names(dc, aref)
        assert TN._check(r, TN._expect_fixtures(aref, total), "all arith") == 55
        cut = r.off[20] + 100
        short = TN._decode_names(dc, aref, capacity=cut)
        assert TN._check(short, TN._expect_fixtures(aref, cut), "cut") == 20
        sizing = TN._decode_names(dc, aref, sizing=True)
    assert sizing.off == r.off and all(s == N.CAPACITY for s in sizing.st) and not any(sizing.osz)


def test_a_batch_of_both_flavours_and_the_same_batch_in_mode_0(dc, aref):
    rans = [f for f in M.fixtures() if f[0].endswith(".7")]
    rref = _ref_of(rans, lambda buf, w: None)
    mixed = [x for pair in zip(rref, [a for a in aref if a[0].endswith(".17")]) for x in pair]
    assert len(mixed) == 22 and [TA.is_arith(m[1]) for m in mixed] == [False, True] * 11
    total = sum(len(want) for _, _, _, _, want, _ in mixed)
    dc.set_option("route_count", 1)
    try:
        _routes(dc)
        with _mode(dc.ctx, DECODE):
            r = TN._decode_names(dc, mixed)
        arith, dec, _, _ = _routes(dc)
        assert TN._check(r, TN._expect_fixtures(mixed, total), "mixed") == 22
        assert sum(arith.values()) > 0 and sum(dec.values()) > 0
        # mode 0: today's path - the arith blocks are refused by the walk and claim nothing, no arith kernel counts a stream
        z = TN._decode_names(dc, mixed)
        arith, dec, _, _ = _routes(dc)
    finally:
        dc.set_option("route_count", 0)
    expect, off = [], 0
    for _, buf, _, _, want, starts in mixed:
        if TA.is_arith(buf):
            expect.append((off, 0, M.UNSUPPORTED, b"", [], False))
        else:
            expect.append((off, len(want), 0, want, starts, True))
            off += len(want)
    assert TN._check(z, expect, "mode 0") == 11
    assert not any(arith.values()) and sum(dec.values()) > 0, (arith, dec)
    for i in range(0, 22, 2):                                           # the rANS blocks: the same bytes in either mode
        assert z.arena[z.off[i]:z.off[i + 1]].tobytes() == r.arena[r.off[i]:r.off[i + 1]].tobytes()


def test_decode_names_batch_and_the_single_block_symbols(H, aref, files):
    from htscodecs_amd import codec
    by = dict(files)
    bufs = [buf for _, buf, _, _, _, _ in aref]
    H.route_read("arith"), H.route_read("decode")
    with _mode(H, DECODE):
        r = TH._call(H, bufs, False)
    assert r.status == [0] * 55
    for (name, buf, _, _, want, _), got, nn in zip(aref, r.data, r.a):
        assert got == want and nn == 1000, name
    assert sum(H.route_read("arith").values()) > 500 and not any(H.route_read("decode").values())
    # mode 0, and the batch wrapper's argument that sets and restores the mode
    z = TH._call(H, bufs[:3], False)
    assert z.status == [M.UNSUPPORTED] * 3 and z.null == [True] * 3
    assert not any(H.route_read("arith").values())
    names, st = codec.tok3_decode_names_batch(bufs[:3], ctx=H, tok3_arith=1)
    assert st == [0] * 3 and names == [a[4] for a in aref[:3]]
    assert codec.set_tok3_arith(0, H) == 0                              # put back
    # the two symbols, and codec.decode_names dispatching on byte 8 as the drop-in header does
    L = H.L
    for name, buf, _, _, want, _ in aref:
        n = C.c_uint32(0)
        p = L.rans4x16_hip_tok3_arith_decode_names(buf, len(buf), C.byref(n))
        assert p, name
        got = C.string_at(p, n.value)
        codec._free(p)
        assert got == want, name
        assert not L.rans4x16_hip_tok3_decode_names(buf, len(buf), C.byref(n)), name      # the rANS symbol still refuses
    for name, buf, _, _, want, _ in aref:
        assert codec.decode_names(buf) == want, name
    # the mode a caller set on the thread's own context is what it was after each of the single-block calls: the
    # setter's return value says so
    blk = by["nv2"]
    for mine in (3, 1, 2, 0):
        codec.thread_tok3_arith(mine)
        name, buf = aref[0][0], aref[0][1]
        n = C.c_uint32(0)
        p = L.rans4x16_hip_tok3_arith_decode_names(buf, len(buf), C.byref(n))
        assert p and codec.thread_tok3_arith(mine) == mine
        codec._free(p)
        assert not L.rans4x16_hip_tok3_decode_names(buf, len(buf), C.byref(n))           # mode 0 for its call, whatever was set
        assert codec.thread_tok3_arith(mine) == mine
        assert codec.encode_names(blk, 7, use_arith=1) is not None and codec.thread_tok3_arith(mine) == mine
        assert codec.encode_names(blk, 7)[0][8] == 0 and codec.thread_tok3_arith(mine) == mine
    assert codec.thread_tok3_arith(0) == 0
    rans = dict(M.fixtures())["03.names.7"]
    assert codec.decode_names(rans) == by["03"].replace(b"\n", b"\0")


# ---- encode -------------------------------------------------------------------------------------------------------
_memo = {}


def _compress(data, method):
    key = (data, method)
    if key not in _memo:
        _memo[key] = AE.compress(data, method)
    return _memo[key]


@pytest.fixture(scope="module")
def framed(aref):
    """{level: [(container, [method per described column], (last_start, nreads, [(id, bytes)]))] per names file}: the
    model's frames over the columns of the level-19 fixtures (the tokeniser's columns: test_tok3_arith_cpu.py reframes them
    to the reference's bytes).  Every candidate stream is made once for all levels."""
    fx = dict(TA.fixtures())
    out = {}
    for level in LEVELS:
        per = []
        for name, buf, w, cols, _, _ in aref:
            if not name.endswith(".19"):
                continue
            block = (w.last_start, w.nreads, [(cid, cols[i]) for cid, i in M.described(w)])
            frame, chosen = M.frame(_compress, block[2], TA.ROWS[level], w.last_start, w.nreads)
            frame = frame[:8] + b"\1" + frame[9:]
            if level >= 7:
                assert frame == fx[name.replace(".19", ".%d" % (10 + level))], (name, level)
            per.append((frame, chosen, block))
        assert len(per) == 11
        out[level] = per
    return out


def _names_back(ctx, containers, files):
    from htscodecs_amd import codec
    names, st = codec.tok3_decode_names_batch(containers, ctx=ctx, tok3_arith=1)
    assert st == [0] * len(containers), st
    assert names == [b.replace(b"\n", b"\0") for _, b in files]


@pytest.mark.parametrize("level", LEVELS)
def test_encode_names_dev_writes_the_reference_containers(dc, files, framed, level):
    blocks = [b for _, b in files]
    want = [f for f, _, _ in framed[level]]
    dc.set_option("route_count", 1)
    try:
        _routes(dc)
        with _mode(dc.ctx, ENCODE):
            r = TE._encode_names(dc, blocks, TA.ROWS[level], dict(TE.LIMITS, max_columns=64))
        _, _, enc, rans = _routes(dc)
    finally:
        dc.set_option("route_count", 0)
    got = TE._containers(r, level)
    assert r.st == [0] * 11
    for (key, _), mine, w in zip(files, got, want):
        assert mine == w, (key, level)
    assert sum(enc.values()) > 0 and not any(rans.values()), (enc, rans)
    _names_back(dc.ctx, got, files)


@pytest.mark.parametrize("level", LEVELS)
def test_pack_dev_over_the_fixtures_own_columns(dc, framed, level):
    blocks = [b for _, _, b in framed[level]]
    want = [f for f, _, _ in framed[level]]
    max_col = max(len(d) for b in blocks for _, d in b[2])
    with _mode(dc.ctx, ENCODE):
        p = T3._pack(dc, blocks, TA.ROWS[level], max_col, sum(len(w) for w in want))
        T3._check_pack(p, want, level)
        assert p.chosen == [m for _, chosen, _ in framed[level] for m in chosen]
        s = T3._pack(dc, blocks, TA.ROWS[level], max_col, 0, sizing=True)
        assert s.off == p.off and not any(s.osz)
        cut = T3._pack(dc, blocks, TA.ROWS[level], max_col, sum(len(w) for w in want), capacity=p.off[5] + 9)
        T3._check_pack(cut, want, (level, "cut"))
    # mode 0 writes the rANS flavour
    z = T3._pack(dc, blocks[:1], TA.ROWS[level], max_col, 4 * len(want[0]) + 4096)
    assert z.st == [0] and z.arena[8] == 0


@pytest.mark.parametrize("level", LEVELS)
def test_encode_names_batch_and_the_single_block_symbols(H, files, framed, level):
    from htscodecs_amd import codec
    blocks = [b for _, b in files]
    want = [f for f, _, _ in framed[level]]
    H.route_read("arith_enc"), H.route_read("encode")
    with _mode(H, ENCODE):
        r = TH._call(H, blocks, True, methods=TA.ROWS[level])
    assert r.status == [0] * 11 and r.data == want
    assert (r.a, r.b) == ([len(b) for b in blocks], [1000] * 11)
    assert sum(H.route_read("arith_enc").values()) > 0 and not any(H.route_read("encode").values())
    res, ls, st = codec.tok3_encode_names_batch(blocks[:2], methods=TA.ROWS[level], ctx=H, tok3_arith=1)
    assert st == [0, 0] and res == want[:2] and codec.set_tok3_arith(0, H) == 0
    res, _, st = codec.tok3_encode_names_batch(blocks[:1], methods=TA.ROWS[level], ctx=H)     # mode 0: the rANS flavour
    assert st == [0] and res[0][8] == 0
    assert codec.tok3_level_methods(level) == TA.ROWS[level]
    L = H.L
    for (key, block), w in zip(files, want):
        buf = C.create_string_buffer(block + b"tail", len(block) + 4)
        out_len, ls = C.c_int(-1), C.c_int(-1)
        p = L.rans4x16_hip_tok3_arith_encode_names(buf, len(block) + 4, level, C.byref(out_len), C.byref(ls))
        assert p, key
        got = C.string_at(p, out_len.value)
        codec._free(p)
        assert got == w and ls.value == len(block), key
        assert buf.raw == TH._nul(block, len(block)) + b"tail", key
    for block, w in zip(blocks, want):
        assert codec.encode_names(block, level, use_arith=1) == (w, len(block))
    assert codec.encode_names(blocks[2], level)[0][8] == 0
    # the rANS symbol keeps its refusal, the caller's buffer untouched
    buf = C.create_string_buffer(blocks[2], len(blocks[2]))
    assert not L.rans4x16_hip_tok3_encode_names(buf, len(blocks[2]), level, 1, C.byref(out_len), None) and buf.raw == blocks[2]
    _names_back(H, r.data, files)


# ---- hostile ------------------------------------------------------------------------------------------------------
def damaged_variants():
    """200 variants of the two smallest arith fixtures of two names files, every header and descriptor byte edited in
    turn (the generator of tests/test_gpu_tok3_host.py's test_damaged_containers_in_one_decode_batch)."""
    by = dict(TA.fixtures())
    variants = []
    for name in ("nv2.names.17", "20.names.17"):
        buf = by[name]
        edits = [(p, x) for p in _descriptor_bytes(TA.cleared(buf)) for x in (0x01, 0x40, 0x80, 0xFF)]
        step = max(len(edits) // 100, 1)
        for p, x in edits[::step][:100]:
            b = bytearray(buf)
            b[p] ^= x
            variants.append(bytes(b))
    assert len(variants) == 200
    return variants


def hostile_expectation(variants):
    """Per variant (scan_any's status, the composed model's (status, names) where the scan accepts)."""
    from htscodecs_amd import codec
    out = []
    for v in variants:
        st = codec.tok3_scan_any(v)[0]
        if st != 0:
            out.append((st, None))
            continue
        assert TA.is_arith(v)                                          # (no edit of this set clears byte 8 and still scans)
        out.append((0, TA.names(v)))
    return out


def test_damaged_arith_containers_beside_intact_ones(H):
    by = dict(TA.fixtures())
    files = N.names_files()
    variants = damaged_variants()
    expect = hostile_expectation(variants)
    accepted = [i for i, (st, m) in enumerate(expect) if st == 0 and m[0] == 0]
    statuses = {st if st else m[0] for st, m in expect}
    assert len(accepted) >= 20 and len(statuses) >= 3, (len(accepted), statuses)
    intact = ["nv2.names.17", "20.names.17"]
    batch = [by[intact[0]]] + variants + [by[intact[1]]]
    # the caller's buffers in one patterned arena: a slot of each container's last_start, where that is sane
    caps = [min(int.from_bytes(b[0:4], "little"), 1 << 16) if len(b) >= 4 else 0 for b in batch]
    offs = (np.cumsum([0] + [c + 64 for c in caps])[:-1] + 64).tolist()
    arena = pattern(offs[-1] + caps[-1] + 4096).copy()
    pat = arena.copy()
    with _mode(H, DECODE):
        r = TH._call(H, batch, False, place=(arena, offs, caps))
    mask = np.zeros(len(arena), dtype=bool)
    for i, b in enumerate(batch):
        if r.status[i] == 0:
            mask[offs[i]:offs[i] + r.size[i]] = True
    assert np.array_equal(arena[~mask], pat[~mask]), "a byte outside the results changed"
    for k, name in ((0, intact[0]), (len(batch) - 1, intact[1])):
        assert r.status[k] == 0 and r.data[k] == files[name.split(".")[0]].replace(b"\n", b"\0"), name
    for i, (st, m) in enumerate(expect):
        got = r.status[1 + i]
        if st != 0:
            assert got == st, (i, got, st)                              # the scan's status, unchanged
        else:
            assert got == m[0], (i, got, m[0])
            if got == 0:
                assert r.data[1 + i] == m[1], i


# ---- the tool -----------------------------------------------------------------------------------------------------
def test_the_names_tool_writes_and_reads_the_arith_flavour(H, files, tmp_path):
    tool = os.path.join(M.ROOT, "tools", "tok3_hip")
    assert os.path.exists(tool), "tools/tok3_hip is built by build()"
    key, block = files[2]
    fx = dict(TA.fixtures())
    src, packed, back = tmp_path / "names", tmp_path / "packed", tmp_path / "back"
    src.write_bytes(block)
    run = lambda *a: subprocess.run([tool] + [str(x) for x in a], capture_output=True, text=True, timeout=120)
    r = run("-a", "-7", "-r", src, packed)
    assert r.returncode == 0, r.stderr
    assert packed.read_bytes() == fx["%s.names.17" % key]
    r = run("-d", "-r", packed, back)
    assert r.returncode == 0 and back.read_bytes() == block, r.stderr
    # in blocks: -a writes arith containers, -d takes the flavour from the data
    r = run("-a", "-9", src, packed)
    assert r.returncode == 0, r.stderr
    data = packed.read_bytes()
    assert int.from_bytes(data[:4], "little") == len(data) - 4 and data[4:] == fx["%s.names.19" % key]
    r = run("-d", packed, back)
    assert r.returncode == 0 and back.read_bytes() == block, r.stderr
    r = run("-11", src, packed)
    assert r.returncode == 1 and "arithmetic" in r.stderr and "-a" in r.stderr
