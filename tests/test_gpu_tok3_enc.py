"""tok3 name encoding on the device (include/rans4x16_hip.h part 2e): rans4x16_hip_tok3_tokenise_dev against the Python
model of the tokeniser (tok3_enc_model.py, pinned by the reference's own files in test_tok3_enc_cpu.py), byte for byte:
the 11 names files of tests/golden/names as one batch, the blocks built for what those files lack, the exact search
forced, the limits, the sizing pass and the capacity rule; then the columns packed by rans4x16_hip_tok3_pack_dev against
the 55 reference-made containers, and decoded again by rans4x16_hip_tok3_decode_names_dev.

Output arenas carry the position pattern of test_gpu_confinement.py and every byte outside the blocks' ranges is
compared.  The model's results are computed once per module and not changed."""
import numpy as np
import pytest

import tok3_enc_model as E
import tok3_model as M
import tok3_names_model as N
from test_gpu_confinement import pattern

pytestmark = pytest.mark.gpu

GUARD = 4096
LIMITS = dict(max_in_size=1 << 17, max_names=1000, max_name_len=256, max_tokens=128, max_columns=160)


@pytest.fixture(scope="module")
def dc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    d = htscodecs_amd.DeviceCodec(0)
    assert d.L.rans4x16_hip_set_dev_stripe_planes(d.ctx.h, 4, 8 * LIMITS["max_in_size"]) == 0      # (for the decodes below)
    yield d
    assert d.L.rans4x16_hip_set_dev_stripe_planes(d.ctx.h, 0, 0) == 0


@pytest.fixture(scope="module")
def files():
    """[(name, block)]: the reference's input files, in name order."""
    return sorted(N.names_files().items())


@pytest.fixture(scope="module")
def built():
    """[(what, block)]: the constructed blocks, the refused ones between the good ones."""
    return [(what, block) for what, block, _ in E.constructed()]


_memo = {}


def _model(block, lim):
    key = (block, tuple(sorted(lim.items())))
    if key not in _memo:
        _memo[key] = E.tokenise(block, **lim)
    return _memo[key]


def _prefix(sizes):
    return [0] + np.cumsum(np.asarray(sizes, dtype=np.int64)).tolist()


class _Result:
    pass


def _tokenise(dc, blocks, lim, capacity=None, sizing=False, search_slots=0, total_in_size=None, gap=3):
    """blocks: [bytes].  They lie `gap` bytes apart in the input, so that d_in_off is not a sum of sizes."""
    import torch
    dev = dc.dev
    nblk = len(blocks)
    raw, offs = bytearray(b"\xee" * gap), []
    for blk in blocks:
        offs.append(len(raw))
        raw += blk + b"\xee" * gap
    d_in = torch.from_numpy(np.frombuffer(bytes(raw) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    in_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    in_size = torch.tensor([len(b) for b in blocks], dtype=torch.int32, device=dev)
    r = _Result()
    alloc = sum(E.bound(len(b)) for b in blocks)
    r.alloc = alloc + GUARD
    r.pat = pattern(r.alloc)
    r.d_cols = None if sizing else torch.from_numpy(r.pat.copy()).to(dev)
    r.cap = 0 if sizing else (alloc if capacity is None else capacity)
    r.maxc = lim["max_columns"]
    r.d_off = torch.full((nblk + 1,), -7, dtype=torch.int64, device=dev)
    r.d_first = torch.full((nblk + 1,), -9, dtype=torch.int32, device=dev)
    r.d_per = [torch.full((nblk,), -3, dtype=torch.int32, device=dev) for _ in range(4)]      # size, status, last_start, nreads
    r.d_id = torch.full((nblk * r.maxc,), -5, dtype=torch.int32, device=dev)
    r.d_coff = torch.full((nblk * r.maxc,), -5, dtype=torch.int64, device=dev)
    r.d_csz = torch.full((nblk * r.maxc,), -5, dtype=torch.int32, device=dev)
    total = sum(len(b) for b in blocks if len(b) <= lim["max_in_size"]) if total_in_size is None else total_in_size
    dc.tok3_tokenise(d_in, in_off, in_size, r.d_cols, r.d_off, r.d_per[0], r.d_per[1], r.d_first, r.d_id, r.d_coff, r.d_csz,
                     r.d_per[2], r.d_per[3], lim["max_in_size"], lim["max_names"], lim["max_name_len"], lim["max_columns"],
                     max_tokens=lim["max_tokens"], total_in_size=total, search_slots=search_slots, col_capacity=r.cap)
    torch.cuda.synchronize()
    r.arena = None if sizing else r.d_cols.cpu().numpy()
    r.off = r.d_off.cpu().numpy().tolist()
    r.first = r.d_first.cpu().numpy().tolist()
    r.size, r.st, r.ls, r.nr = [x.cpu().numpy().view(np.uint32).tolist() for x in r.d_per]
    r.id, r.coff, r.csz = r.d_id.cpu().numpy(), r.d_coff.cpu().numpy(), r.d_csz.cpu().numpy()
    return r


def _expected(blocks, lim, cap, slots=None):
    """Per block (start, claim, status, [(id, bytes)], last_start, nreads); slots: total_in_size, where it is short."""
    out, off, used = [], 0, 0
    for blk in blocks:
        st, cols, ls, nr = _model(blk, lim)
        if len(blk) <= lim["max_in_size"]:
            used += len(blk)
            if slots is not None and used > slots:
                st, cols, ls, nr = E.UNSUPPORTED, [], 0, 0
        claim = sum(len(d) for _, d in cols)
        start, off = off, off + claim
        if st == 0 and off > cap:
            st, cols = E.CAPACITY, []
        out.append((start, claim, st, cols, ls, nr))
    return out


def _check(r, expect, what):
    """Returns the number of blocks that came out whole."""
    assert r.off == _prefix([e[1] for e in expect]), (what, r.off[:8])
    assert r.first == _prefix([len(e[3]) for e in expect]), (what, r.first[:8])
    mask = np.zeros(r.alloc, dtype=bool)
    whole = at = 0
    for i, (start, claim, st, cols, ls, nr) in enumerate(expect):
        tag = (what, i, r.st[i], st)
        assert r.st[i] == st, tag
        assert (r.ls[i], r.nr[i]) == (ls, nr), tag
        if st != 0:
            assert r.size[i] == 0, tag
            continue
        whole += 1
        assert r.size[i] == claim, tag
        mask[start:start + claim] = True
        o = start
        for cid, data in cols:
            ctag = tag + (hex(cid),)
            assert (int(r.id[at]), int(r.coff[at]), int(r.csz[at])) == (cid, o, len(data)), ctag
            assert r.arena[o:o + len(data)].tobytes() == data, ctag
            o += len(data)
            at += 1
    assert (r.id[at:] == -5).all() and (r.coff[at:] == -5).all() and (r.csz[at:] == -5).all(), (what, "directory behind the last column")
    if r.arena is not None:
        assert np.array_equal(r.arena[~mask], r.pat[~mask]), (what, "a byte outside the blocks' ranges changed")
    return whole


def test_the_names_files_as_one_batch(dc, files):
    blocks = [b for _, b in files]
    lim = dict(LIMITS)
    alloc = sum(E.bound(len(b)) for b in blocks)
    assert _check(_tokenise(dc, blocks, lim), _expected(blocks, lim, alloc), "names files") == 11


def test_the_constructed_blocks(dc, built):
    blocks = [b for _, b in built]
    lim = dict(LIMITS)
    alloc = sum(E.bound(len(b)) for b in blocks)
    expect = _expected(blocks, lim, alloc)
    assert {e[2] for e in expect} == {0, E.SIZE, E.UNSUPPORTED}
    whole = _check(_tokenise(dc, blocks, lim), expect, "constructed")
    assert whole == sum(e[2] == 0 for e in expect) >= 40


@pytest.mark.parametrize("slots", [1, 64])
def test_the_exact_search_gives_the_same_bytes(dc, files, built, slots):
    """search_slots 1: no table at all; 64: the table of a names file fills up inside the block."""
    blocks = [b for _, b in built] + [files[2][1], files[10][1]]
    lim = dict(LIMITS)
    alloc = sum(E.bound(len(b)) for b in blocks)
    _check(_tokenise(dc, blocks, lim, search_slots=slots), _expected(blocks, lim, alloc), "search_slots %d" % slots)


def test_sizing_pass_and_a_capacity_one_byte_short(dc, files, built):
    blocks = [files[0][1], built[0][1], b"no end", files[5][1], built[5][1]]
    lim = dict(LIMITS)
    full = _expected(blocks, lim, 1 << 40)
    total = full[-1][0] + full[-1][1]
    r = _tokenise(dc, blocks, lim, sizing=True)
    assert r.off[-1] == total
    assert _check(r, _expected(blocks, lim, 0), "sizing") == 0
    assert _check(_tokenise(dc, blocks, lim, capacity=total), _expected(blocks, lim, total), "exact capacity") == 4
    short = _expected(blocks, lim, total - 1)
    assert [e[2] for e in short] == [0, 0, E.SIZE, 0, E.CAPACITY]
    assert _check(_tokenise(dc, blocks, lim, capacity=total - 1), short, "one byte short") == 3
    first = full[0][1]
    assert _check(_tokenise(dc, blocks, lim, capacity=first), _expected(blocks, lim, first), "room for one") == 1


@pytest.mark.parametrize("which,value,refused", [("max_names", 64, 1), ("max_names", 65, 0), ("max_name_len", 128, 1),
                                                 ("max_name_len", 129, 0), ("max_in_size", 400, 2), ("max_columns", 12, None),
                                                 ("max_tokens", 64, 1), ("max_tokens", 65, 0)])
def test_limits_refuse_a_block_whole(dc, built, which, value, refused):
    by = dict(built)
    blocks = [by["64 names"], by["65 names"], (b"Qx:z-" * 26)[:129] + b"\nab\n", by["N_END at 63"], by["N_END at 64"], by["digit runs"],
              by["Illumina plain"], by["2 names"]]
    lim = dict(LIMITS)
    lim[which] = value
    alloc = sum(E.bound(len(b)) for b in blocks)
    expect = _expected(blocks, lim, alloc)
    sts = [e[2] for e in expect]
    assert sts[-1] == 0 and (sts.count(E.UNSUPPORTED) == refused if refused is not None else 0 < sts.count(E.UNSUPPORTED) < len(sts))
    _check(_tokenise(dc, blocks, lim), expect, "%s %d" % (which, value))


def test_a_block_beyond_the_announced_total_is_refused(dc, built):
    by = dict(built)
    blocks = [by["2 names"], by["digit runs"], by["64 names"], by["1 names"]]
    lim = dict(LIMITS)
    alloc = sum(E.bound(len(b)) for b in blocks)
    slots = len(blocks[0]) + len(blocks[1]) + len(blocks[2]) - 1
    expect = _expected(blocks, lim, alloc, slots=slots)
    assert [e[2] for e in expect] == [0, 0, E.UNSUPPORTED, E.UNSUPPORTED]
    _check(_tokenise(dc, blocks, lim, total_in_size=slots), expect, "short total")


# ---- names in, containers out ------------------------------------------------------------------------------------
def _encode_names(dc, blocks, methods, lim, capacity=None, sizing=False, search_slots=0, alloc=None):
    import torch
    dev = dc.dev
    nblk = len(blocks)
    raw, offs = bytearray(b"\xee" * 5), []
    for blk in blocks:
        offs.append(len(raw))
        raw += blk + b"\xee" * 5
    d_in = torch.from_numpy(np.frombuffer(bytes(raw) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    in_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    in_size = torch.tensor([len(b) for b in blocks], dtype=torch.int32, device=dev)
    r = _Result()
    alloc = sum(len(b) + 1024 for b in blocks) if alloc is None else alloc
    r.alloc = alloc + GUARD
    r.pat = pattern(r.alloc)
    r.d_out = None if sizing else torch.from_numpy(r.pat.copy()).to(dev)
    r.cap = 0 if sizing else (alloc if capacity is None else capacity)
    r.d_off = torch.full((nblk + 1,), -7, dtype=torch.int64, device=dev)
    r.d_first = torch.full((nblk + 1,), -9, dtype=torch.int32, device=dev)
    r.d_size = torch.full((nblk,), -3, dtype=torch.int32, device=dev)
    r.d_st = torch.full((nblk,), -3, dtype=torch.int32, device=dev)
    dc.tok3_encode_names(d_in, in_off, in_size, r.d_out, r.d_off, r.d_size, r.d_st, methods, lim["max_in_size"], lim["max_names"],
                         lim["max_name_len"], lim["max_columns"], max_tokens=lim["max_tokens"],
                         total_in_size=sum(len(b) for b in blocks), search_slots=search_slots, blk_first=r.d_first, out_capacity=r.cap)
    torch.cuda.synchronize()
    r.arena = None if sizing else r.d_out.cpu().numpy()
    r.off = r.d_off.cpu().numpy().tolist()
    r.first = r.d_first.cpu().numpy().tolist()
    r.size = r.d_size.cpu().numpy().view(np.uint32).tolist()
    r.st = r.d_st.cpu().numpy().tolist()
    return r


def _containers(r, what):
    """The containers of the blocks that came out whole (None for the others), after the checks every result must pass."""
    assert r.off == _prefix(r.size), (what, r.off[:8])
    mask = np.zeros(r.alloc, dtype=bool)
    out = []
    for i, (st, size) in enumerate(zip(r.st, r.size)):
        assert (st == 0) == (size != 0), (what, i, st, size)
        mask[r.off[i]:r.off[i] + size] = True
        out.append(r.arena[r.off[i]:r.off[i] + size].tobytes() if st == 0 else None)
    assert np.array_equal(r.arena[~mask], r.pat[~mask]), (what, "a byte outside the blocks' ranges changed")
    return out


def _decode_back(dc, containers, blocks, max_columns, what):
    """rans4x16_hip_tok3_decode_names_dev over the containers: every block's names, each line end a NUL."""
    import torch
    dev = dc.dev
    n = len(containers)
    want = [bytes(0 if ch <= 10 else ch for ch in blk[:E.frame(blk)[1]]) for blk in blocks]
    d_in = torch.from_numpy(np.frombuffer(b"".join(containers) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    in_off = torch.tensor(_prefix([len(c) for c in containers])[:-1], dtype=torch.int64, device=dev)
    in_size = torch.tensor([len(c) for c in containers], dtype=torch.int32, device=dev)
    d_out = torch.zeros(sum(len(x) for x in want) + 64, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    per = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3)]
    nreads = [E.frame(blk)[0] for blk in blocks]
    dc.tok3_decode_names(d_in, in_off, in_size, d_out, off, per[0], per[1], per[2], max_columns, max(len(c) for c in containers),
                         max(4 * len(b) for b in blocks), max(nreads), 128,
                         total_col_size=sum(6 * len(b) + 128 * nr for b, nr in zip(blocks, nreads)))
    torch.cuda.synchronize()
    o, got = off.cpu().numpy().tolist(), d_out.cpu().numpy()
    assert per[2].cpu().numpy().tolist() == [0] * n, (what, per[2].cpu().numpy().tolist())
    assert per[1].cpu().numpy().tolist() == nreads, what
    for i, w in enumerate(want):
        assert got[o[i]:o[i + 1]].tobytes() == w, (what, i)


@pytest.mark.parametrize("level", [1, 3, 5, 7, 9])
def test_encode_names_writes_the_reference_containers(dc, files, level):
    """Byte for byte the 51 fixtures outside tok3_model.EXCEPTIONS; every container decodes to its names file."""
    fx = dict(M.fixtures())
    blocks = [b for _, b in files]
    lim = dict(LIMITS, max_columns=64)
    r = _encode_names(dc, blocks, M.LISTS[level], lim)
    got = _containers(r, level)
    assert r.st == [0] * 11
    assert r.first == _prefix([len(_model(b, LIMITS)[1]) for b in blocks])
    same = 0
    for (key, _), mine in zip(files, got):
        name = "%s.names.%d" % (key, level)
        if name not in M.EXCEPTIONS:
            assert mine == fx[name], name
            same += 1
    assert same == (11 if level in (1, 7, 9) else 9)
    _decode_back(dc, got, blocks, 64, level)


def test_encode_names_of_the_constructed_blocks_decode_to_their_names(dc, built):
    blocks = [b for _, b in built]
    lim = dict(LIMITS)
    r = _encode_names(dc, blocks, M.LISTS[7], lim)
    got = _containers(r, "constructed")
    want = [_model(b, lim) for b in blocks]
    assert r.st == [w[0] for w in want]
    assert r.first == _prefix([len(w[1]) for w in want])
    whole = [i for i, c in enumerate(got) if c is not None]
    assert len(whole) >= 40
    for i in whole:
        assert got[i][:9] == want[i][2].to_bytes(4, "little") + want[i][3].to_bytes(4, "little") + b"\0", i
    _decode_back(dc, [got[i] for i in whole], [blocks[i] for i in whole], lim["max_columns"], "constructed")


def test_encode_names_sizing_pass_and_a_capacity_one_byte_short(dc, files, built):
    blocks = [files[3][1], b"no end", built[1][1], files[8][1]]
    lim = dict(LIMITS, max_columns=64)
    full = _encode_names(dc, blocks, M.LISTS[3], lim)
    assert full.st == [0, E.SIZE, 0, 0]
    total = full.off[-1]
    sizing = _encode_names(dc, blocks, M.LISTS[3], lim, sizing=True)
    assert sizing.off == full.off and sizing.st == [E.CAPACITY, E.SIZE, E.CAPACITY, E.CAPACITY] and sizing.size == [0] * 4
    exact = _encode_names(dc, blocks, M.LISTS[3], lim, capacity=total, alloc=total)
    assert _containers(exact, "exact") == _containers(full, "full")
    short = _encode_names(dc, blocks, M.LISTS[3], lim, capacity=total - 1, alloc=total)
    assert short.st == [0, E.SIZE, 0, E.CAPACITY] and short.off == full.off and short.size == full.size[:3] + [0]
    mask = np.zeros(short.alloc, dtype=bool)
    mask[:full.off[3]] = True
    assert np.array_equal(short.arena[:full.off[3]], full.arena[:full.off[3]])
    assert np.array_equal(short.arena[~mask], short.pat[~mask])
