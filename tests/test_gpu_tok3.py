"""tok3 column containers on the device (include/rans4x16_hip.h part 2c): rans4x16_hip_tok3_pack_dev and
rans4x16_hip_tok3_unpack_dev against the Python model of the container (tok3_model.py) over the oracle's rANS streams,
on the 55 reference-made containers of tests/golden/tok3 and on constructed and damaged ones.

Output arenas carry the position pattern of test_gpu_confinement.py and every byte outside the blocks' ranges is compared.
The expected results of the fixtures (walk, decoded columns) are computed once per module and not changed.

The fixtures' .3 / .5 / .7 / .9 levels hold X_STRIPE columns: the context decodes them after
rans4x16_hip_set_dev_stripe_planes, as rans4x16_hip_uncompress_packed_dev does."""
import numpy as np
import pytest

import tok3_model as M
from test_gpu_confinement import pattern
from test_tok3_cpu import WALK_CASES

pytestmark = pytest.mark.gpu

GUARD = 4096
TYPE_COLUMN = 0x10000
NINE = M.LISTS[9]


@pytest.fixture(scope="module")
def ref(oracle):
    """Per fixture: (name, container, walk, [bytes of every column, type columns included])."""
    out = []
    for name, buf in M.fixtures():
        w = M.walk(buf)
        assert w.status == 0, name
        cols = M.columns(buf, w, _decoder(oracle))
        assert cols is not None, name
        out.append((name, buf, w, cols))
    assert len(out) == 55
    return out


@pytest.fixture(scope="module")
def max_col(ref):
    return max(w.largest_col for _, _, w, _ in ref)


@pytest.fixture(scope="module")
def dc(ref, max_col):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    d = htscodecs_amd.DeviceCodec(0)
    assert d.L.rans4x16_hip_set_dev_stripe_planes(d.ctx.h, 4, 2 * max_col) == 0
    yield d
    assert d.L.rans4x16_hip_set_dev_stripe_planes(d.ctx.h, 0, 0) == 0


def _decoder(oracle):
    return lambda stream, size: oracle.uncompress(stream, capacity=size, out_size_hint=size)


def _prefix(sizes):
    return [0] + np.cumsum(np.asarray(sizes, dtype=np.int64)).tolist()


def _i32(values):
    return np.asarray(values, dtype=np.uint32).view(np.int32) if len(values) else np.zeros(0, dtype=np.int32)


# ---- unpack ----------------------------------------------------------------------------------------------------
class _Unpacked:
    pass


def _unpack(dc, containers, max_columns, max_col_size, alloc, capacity=None, sizing=False):
    import torch
    dev = dc.dev
    n = len(containers)
    d_in = torch.from_numpy(np.frombuffer(b"".join(containers) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    in_off = torch.tensor(_prefix([len(c) for c in containers])[:-1], dtype=torch.int64, device=dev)
    in_size = torch.from_numpy(_i32([len(c) for c in containers])).to(dev)
    u = _Unpacked()
    u.alloc = alloc + GUARD
    u.pat = pattern(u.alloc)
    d_out = None if sizing else torch.from_numpy(u.pat.copy()).to(dev)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    per_blk = [torch.full((n,), -3, dtype=torch.int32, device=dev) for _ in range(5)]
    cid = torch.full((n * max_columns,), -3, dtype=torch.int32, device=dev)
    coff = torch.full((n * max_columns,), -3, dtype=torch.int64, device=dev)
    csz = torch.full((n * max_columns,), -3, dtype=torch.int32, device=dev)
    u.cap = 0 if sizing else (alloc if capacity is None else capacity)
    dc.tok3_unpack(d_in, in_off, in_size, d_out, off, per_blk[0], per_blk[1], per_blk[2], per_blk[3], per_blk[4], cid, coff, csz,
                   max_columns, max(len(c) for c in containers), max_col_size, out_capacity=u.cap)
    torch.cuda.synchronize()
    u.arena = None if sizing else d_out.cpu().numpy()
    u.off = off.cpu().numpy().tolist()
    u.osz, u.st, u.ncol, u.ls, u.nr = [x.cpu().numpy().view(np.uint32).tolist() for x in per_blk]
    u.cid = cid.cpu().numpy().reshape(n, max_columns)
    u.coff = coff.cpu().numpy().reshape(n, max_columns)
    u.csz = csz.cpu().numpy().view(np.uint32).reshape(n, max_columns)
    return u


def _directory(w, start):
    """What the directory of a walked container holds: [(id with its flag, offset, size)] per descriptor."""
    out, at, lead = [], start, False
    for c in w.cols:
        if c["kind"] == M.SYNTH:
            lead = True
        else:
            out.append((c["id"] | (TYPE_COLUMN if lead else 0), at, c["size"]))
            lead = False
        at += c["size"]
    return out


def _check_unpack(u, containers, expect, max_columns, what):
    """expect[i] = (walk, columns or None where the oracle refuses a stream).  Returns the blocks that came out whole."""
    need = _prefix([w.total if w.status == 0 else 0 for w, _ in expect])
    assert u.off == need, (what, u.off[:6], need[:6])
    mask = np.zeros(u.alloc, dtype=bool)                       # bytes some block may have written
    whole = 0
    for i, (w, cols) in enumerate(expect):
        tag = (what, i, u.st[i], w.status)
        assert (u.ls[i], u.nr[i]) == (w.last_start, w.nreads) or len(containers[i]) < 9, tag
        if w.status != 0:
            assert u.st[i] == w.status and u.osz[i] == 0 and u.ncol[i] == 0, tag
            continue
        if need[i + 1] > u.cap:
            assert u.st[i] == M.CAPACITY and u.osz[i] == 0 and u.ncol[i] == 0, tag
            continue
        mask[need[i]:need[i + 1]] = True
        if cols is None:                                       # whatever the oracle rejects, the device rejects
            assert u.st[i] != 0 and u.osz[i] == 0 and u.ncol[i] == 0, tag
            continue
        if u.st[i] != 0:                                       # the documented stricter cases of the decoder
            assert u.st[i] in (6, 7, 8) and u.osz[i] == 0 and u.ncol[i] == 0, tag
            continue
        whole += 1
        assert u.osz[i] == w.total and u.ncol[i] == w.ndesc, tag
        assert u.arena[need[i]:need[i + 1]].tobytes() == b"".join(cols), tag
        want = _directory(w, need[i])
        got = list(zip(u.cid[i].tolist(), u.coff[i].tolist(), u.csz[i].tolist()))
        assert got[:len(want)] == want, tag
        assert all(g[0] == -1 and g[2] == 0 for g in got[len(want):]), tag
    if u.arena is not None:
        assert np.array_equal(u.arena[~mask], u.pat[~mask]), (what, "a byte outside the blocks' ranges changed")
    return whole


def test_unpack_all_fixtures_in_one_call(dc, ref, max_col):
    containers = [buf for _, buf, _, _ in ref]
    expect = [(w, cols) for _, _, w, cols in ref]
    u = _unpack(dc, containers, 64, max_col, sum(w.total for w, _ in expect))
    assert _check_unpack(u, containers, expect, 64, "all") == 55
    assert any(c["kind"] == M.SYNTH for w, _ in expect for c in w.cols)
    assert sum(c["kind"] == M.DUP for w, _ in expect for c in w.cols) == 160


def test_unpack_each_fixture_alone_with_its_own_count_and_one_less(dc, ref, max_col):
    for name, buf, w, cols in ref:
        u = _unpack(dc, [buf], w.ndesc, w.largest_col, w.total)
        assert _check_unpack(u, [buf], [(w, cols)], w.ndesc, name) == 1
        if w.ndesc > 1:
            short = M.walk(buf, max_columns=w.ndesc - 1)
            assert short.status == M.UNSUPPORTED
            u = _unpack(dc, [buf], w.ndesc - 1, max_col, w.total)
            assert _check_unpack(u, [buf], [(short, None)], w.ndesc - 1, name + " one less") == 0
            assert u.st[0] == M.UNSUPPORTED


# ---- pack ------------------------------------------------------------------------------------------------------
class _Packed:
    pass


def _pack(dc, blocks, methods, max_col_size, alloc, capacity=None, sizing=False, blk_first=None, total=True):
    """blocks: [(last_start, nreads, [(id, bytes)])]; blk_first overrides the blocks' own layout of the flat column list."""
    import torch
    dev = dc.dev
    flat = [c for _, _, cols in blocks for c in cols]
    n, nblk = len(flat), len(blocks)
    d_in = torch.from_numpy(np.frombuffer(b"".join(d for _, d in flat) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    col_off = torch.tensor(_prefix([len(d) for _, d in flat])[:-1], dtype=torch.int64, device=dev)
    col_size = torch.from_numpy(_i32([len(d) for _, d in flat])).to(dev)
    col_id = torch.from_numpy(_i32([i for i, _ in flat])).to(dev)
    first = blk_first if blk_first is not None else _prefix([len(cols) for _, _, cols in blocks])
    d_first = torch.from_numpy(_i32(first)).to(dev)
    ls = torch.from_numpy(_i32([b[0] for b in blocks])).to(dev)
    nr = torch.from_numpy(_i32([b[1] for b in blocks])).to(dev)
    p = _Packed()
    p.alloc = alloc + GUARD
    p.pat = pattern(p.alloc)
    d_out = None if sizing else torch.from_numpy(p.pat.copy()).to(dev)
    off = torch.full((nblk + 1,), -7, dtype=torch.int64, device=dev)
    osz = torch.full((nblk,), -3, dtype=torch.int32, device=dev)
    st = torch.full((nblk,), -3, dtype=torch.int32, device=dev)
    chosen = torch.full((n,), -3, dtype=torch.int32, device=dev)
    p.cap = 0 if sizing else (alloc if capacity is None else capacity)
    dc.tok3_pack(d_first, d_in, col_off, col_size, col_id, ls, nr, d_out, off, osz, st, methods, max_col_size, chosen=chosen,
                 total_col_size=sum(len(d) for _, d in flat) if total else 0, out_capacity=p.cap)
    torch.cuda.synchronize()
    p.arena = None if sizing else d_out.cpu().numpy()
    p.off, p.osz, p.st, p.chosen = off.cpu().numpy().tolist(), osz.cpu().numpy().tolist(), st.cpu().numpy().tolist(), chosen.cpu().numpy().tolist()
    return p


def _check_pack(p, want, what):
    """want[i]: the container of block i, or a status for a block that must fail.  Everything else keeps the pattern."""
    need = _prefix([len(w) if isinstance(w, bytes) else 0 for w in want])
    assert p.off == need, (what, p.off[:6], need[:6])
    mask = np.zeros(p.alloc, dtype=bool)
    for i, w in enumerate(want):
        tag = (what, i, p.st[i], p.osz[i])
        if not isinstance(w, bytes):
            assert p.st[i] == w and p.osz[i] == 0, tag
        elif need[i + 1] > p.cap:
            assert p.st[i] == M.CAPACITY and p.osz[i] == 0, tag
        else:
            assert p.st[i] == 0 and p.osz[i] == len(w), tag
            mask[need[i]:need[i + 1]] = True
            got = p.arena[need[i]:need[i + 1]].tobytes()
            assert got == w, tag + (next(k for k in range(len(w)) if got[k] != w[k]),)
    if p.arena is not None:
        assert np.array_equal(p.arena[~mask], p.pat[~mask]), (what, "a byte outside the blocks' ranges changed")


def _block_of(w, cols):
    return (w.last_start, w.nreads, [(cid, cols[i]) for cid, i in M.described(w)])


@pytest.mark.parametrize("level", [1, 3, 5, 7, 9])
def test_pack_reproduces_the_fixtures_byte_for_byte(dc, ref, oracle, max_col, level):
    mine = [(name, buf, w, cols) for name, buf, w, cols in ref if M.level_of(name) == level and name not in M.EXCEPTIONS]
    assert len(mine) == (11 if level in (1, 7, 9) else 9)
    blocks = [_block_of(w, cols) for _, _, w, cols in mine]
    want = [buf for _, buf, _, _ in mine]
    p = _pack(dc, blocks, M.LISTS[level], max_col, sum(len(b) for b in want))
    _check_pack(p, want, level)
    chosen = [m for b in blocks for m in M.frame(oracle.compress, b[2], M.LISTS[level], b[0], b[1])[1]]
    assert p.chosen == chosen


def test_the_four_exceptions_round_trip(dc, ref, oracle, max_col):
    mine = [(name, buf, w, cols) for name, buf, w, cols in ref if name in M.EXCEPTIONS]
    assert len(mine) == 4
    for level in (3, 5):
        part = [x for x in mine if M.level_of(x[0]) == level]
        blocks = [_block_of(w, cols) for _, _, w, cols in part]
        want = [M.frame(oracle.compress, b[2], M.LISTS[level], b[0], b[1])[0] for b in blocks]
        assert all(x != buf for x, (_, buf, _, _) in zip(want, part))              # (they are the exceptions)
        p = _pack(dc, blocks, M.LISTS[level], max_col, sum(len(b) for b in want))
        _check_pack(p, want, ("exceptions", level))
        expect = [(M.walk(x), cols) for x, (_, _, _, cols) in zip(want, part)]
        u = _unpack(dc, want, 64, max_col, sum(w.total for w, _ in expect))
        assert _check_unpack(u, want, expect, 64, ("exceptions", level)) == len(part)


# ---- constructed blocks ------------------------------------------------------------------------------------------
def _text(n, seed):
    rng = np.random.default_rng(seed)
    return bytes(rng.choice(np.frombuffer(b"ACGT01:/x", dtype=np.uint8), size=n, p=[.3, .2, .1, .1, .1, .05, .05, .05, .05]).tolist())


def _constructed(oracle, max_col_size):
    """Blocks that reach every branch of the framing, with the method list [0, 1] unless said otherwise."""
    def framed(data, methods=(0, 1)):
        s = M.best(oracle.compress, data, list(methods))[1]
        return len(M.var_put(len(s)) + s)

    sizes = [1, 2, 3, 4, 5, 20, 21, 4000, max_col_size]
    a = (7, 11, [((k // 3) << 4 | (k % 3 + 1), _text(n, n)) for k, n in enumerate(sizes)])
    short, long_ = b"A", b"AB"
    assert framed(short) == 4 and framed(long_) == 5                              # not a duplicate / a duplicate
    b = (0, 2, [(0x00, _text(30, 1)), (0x01, short), (0x02, short), (0x03, long_), (0x04, long_), (0x10, _text(9, 2))])
    x = _text(50, 3)
    c = (1, 3, [(0x01, x), (0x02, x), (0x03, x), (0x11, _text(8, 4))])              # the third equals a duplicate: written as one of the first
    zero = _text(40, 5)
    d = (2, 4, [(0x00, zero), (0x05, _text(12, 6)), (0x16, zero), (0x17, _text(7, 7))])      # equal to column id 0: written in full
    e = (3, 5, [(0x02, x), (0x13, x)])                                              # a duplicate as the last descriptor
    f = (4, 6, [(0x07, _text(100, 8))])                                             # one column
    return [a, b, c, d, e, f]


def _columns_of(block):
    """What unpacking the container of a block gives: the type columns of positions opened by another type included."""
    out, last = [], -1
    for cid, data in block[2]:
        if cid >> 4 != last and cid & 15:
            out.append(bytes([cid & 15]) + bytes([M.N_MATCH]) * (block[1] - 1))
        last = cid >> 4
        out.append(data)
    return out


@pytest.mark.parametrize("nblk", [1, 300])
def test_constructed_blocks_round_trip(dc, oracle, nblk):
    max_col_size = 5000
    kinds = _constructed(oracle, max_col_size)
    framed = [M.frame(oracle.compress, b[2], [0, 1], b[0], b[1])[0] for b in kinds]
    # the model wrote what the cases are about
    kinds_of = lambda i: [(c["kind"], c.get("src")) for c in M.walk(framed[i] + b"\0").cols]      # (+ a byte: a duplicate may end it)
    assert kinds_of(1) == [(M.PLAIN, None)] * 4 + [(M.DUP, 3), (M.PLAIN, None)]
    assert kinds_of(2)[:4] == [(M.SYNTH, None), (M.PLAIN, None), (M.DUP, 1), (M.DUP, 1)]
    assert all(k != M.DUP for k, _ in kinds_of(3))
    assert framed[4].endswith(bytes([0x80 | 0x43, 0, 2]))
    pick = [0] if nblk == 1 else [i % len(kinds) for i in range(nblk)]
    blocks = [kinds[i] for i in pick]
    want = [framed[i] for i in pick]
    for total in (True, False):
        p = _pack(dc, blocks, [0, 1], max_col_size, sum(len(w) for w in want), total=total)
        _check_pack(p, want, ("constructed", nblk, total))
    expect = []
    for i, cont in zip(pick, want):
        w = M.walk(cont)
        assert w.status == (M.TRUNCATED if i == 4 else 0)                          # unpack refuses a duplicate at the very end, as the reference does
        expect.append((w, _columns_of(kinds[i]) if w.status == 0 else None))
    u = _unpack(dc, want, 16, max_col_size, sum(w.total for w, _ in expect if w.status == 0))
    assert _check_unpack(u, want, expect, 16, ("constructed", nblk)) == sum(i != 4 for i in pick)


def test_the_tok3_arena_grows_and_is_reused(dc, oracle):
    """A fresh context, pack and unpack of 3 blocks of one 4 KiB column each, then of 13, then of 3 again: the first
    calls allocate the tok3 arena, the pack of 13 finds it too small and grows it - synchronize, free, allocate - and
    the last calls lay their arrays out in an arena larger than they asked for."""
    import htscodecs_amd
    fresh = htscodecs_amd.DeviceCodec(0)
    blocks = [(4 + j, 6, [(0x07, _text(4096, 100 + j))]) for j in range(13)]
    framed = [M.frame(oracle.compress, b[2], [0, 1], b[0], b[1])[0] for b in blocks]
    expect = [(M.walk(c), _columns_of(b)) for c, b in zip(framed, blocks)]
    assert all(w.status == 0 for w, _ in expect)
    for n in (3, 13, 3):
        p = _pack(fresh, blocks[:n], [0, 1], 5000, sum(len(c) for c in framed[:n]))
        _check_pack(p, framed[:n], ("regrow", n))
        u = _unpack(fresh, framed[:n], 16, 5000, sum(w.total for w, _ in expect[:n]))
        assert _check_unpack(u, framed[:n], expect[:n], 16, ("regrow", n)) == n


def test_a_column_equal_to_column_id_0_is_written_in_full(oracle):
    d = _constructed(oracle, 5000)[3]
    cont = M.frame(oracle.compress, d[2], [0, 1], d[0], d[1])[0]
    w = M.walk(cont)
    assert w.status == 0 and [c["kind"] for c in w.cols] == [M.PLAIN, M.PLAIN, M.SYNTH, M.PLAIN, M.PLAIN]


def test_unpack_of_a_duplicate_of_a_duplicate_and_of_a_type_column(dc, oracle):
    s = oracle.compress(_text(33, 9), 0)
    plain = lambda t, stream: bytes([t]) + M.var_put(len(stream)) + stream
    tail = plain(0x05, oracle.compress(b"z", 0))
    cont = (b"\x01\0\0\0\x06\0\0\0\0" + plain(0x80, s) + bytes([0x41, 0, 0]) + bytes([0x43, 0, 1]) + bytes([0x44, 0, 2])
            + bytes([0x80 | 0x42, 1, 0]) + bytes([0x43, 1, 0]) + tail)
    w = M.walk(cont)
    assert w.status == 0 and w.ndesc == 7 and w.ncol == 8
    cols = M.columns(cont, w, _decoder(oracle))
    assert cols[1] == cols[2] == cols[0] and cols[3] == b"" and cols[4] == cols[5] == cols[6] == bytes([2]) + bytes([10]) * 5
    u = _unpack(dc, [cont], 8, 64, w.total)
    assert _check_unpack(u, [cont], [(w, cols)], 8, "copies") == 1


# ---- failures, capacity ------------------------------------------------------------------------------------------
def test_pack_failures_leave_their_neighbours_alone(dc, oracle):
    good = lambda k: (k, 3, [(0x00, _text(30 + k, k)), (0x11, _text(20, 50 + k))])
    frame = lambda b: M.frame(oracle.compress, b[2], NINE, b[0], b[1])[0]
    blocks = [good(0),
              (1, 3, [(0x00, _text(10, 1)), (0x01, b"")]),                           # a zero-length column
              good(2),
              (3, 3, [(0x05, _text(10, 2)), (0x04, _text(10, 3))]),                  # ids out of order
              (4, 3, [(0x05, _text(10, 2)), (0x05, _text(10, 3))]),                  # .. or equal
              good(5),
              (6, 3, [(0x7f0, _text(10, 4)), (0x800, _text(10, 5))]),                # tnum 128
              (7, 3, [(0x00, _text(10, 6)), (0x01, _text(301, 7))]),                 # above max_col_size
              good(8)]
    want = [frame(b) if i in (0, 2, 5, 8) else (M.UNSUPPORTED if i == 7 else M.SIZE) for i, b in enumerate(blocks)]
    p = _pack(dc, blocks, NINE, 300, sum(len(w) for w in want if isinstance(w, bytes)))
    _check_pack(p, want, "failures")


def test_pack_with_an_inconsistent_block_table(dc, oracle):
    cols = [(0x00, _text(30, 1)), (0x10, _text(31, 2)), (0x00, _text(32, 3)), (0x10, _text(33, 4)), (0x20, _text(34, 5)), (0x30, _text(35, 6))]
    frame = lambda cs, k: M.frame(oracle.compress, cs, NINE, k, 3)[0]

    def run(first, want):
        blocks = [(k, 3, []) for k in range(len(first) - 1)]      # the headers; the columns are one flat list, laid out by `first`
        blocks[0] = (0, 3, cols)
        p = _pack(dc, blocks, NINE, 300, sum(len(w) for w in want if isinstance(w, bytes)), blk_first=first)
        _check_pack(p, want, first)

    run([0, 2, 4, 3, 6], [frame(cols[0:2], 0), frame(cols[2:4], 1), M.SIZE, M.SIZE])                    # first > next; a start inside an earlier block
    run([1, 2, 4, 6], [M.SIZE, frame(cols[2:4], 1), frame(cols[4:6], 2)])                             # does not start at 0
    run([0, 2, 4, 5], [frame(cols[0:2], 0), frame(cols[2:4], 1), M.SIZE])                             # does not end at n
    run([0, 2, 7, 6], [frame(cols[0:2], 0), M.SIZE, M.SIZE])                                          # beyond n


def test_pack_capacity(dc, ref, oracle, max_col):
    mine = [(name, buf, w, cols) for name, buf, w, cols in ref if M.level_of(name) == 9][:6]
    blocks = [_block_of(w, cols) for _, _, w, cols in mine]
    want = [buf for _, buf, _, _ in mine]
    total = sum(len(b) for b in want)
    p = _pack(dc, blocks, NINE, max_col, total, sizing=True)
    assert p.off == _prefix([len(b) for b in want]) and p.off[-1] == total
    assert all(s == M.CAPACITY for s in p.st) and not any(p.osz)
    p = _pack(dc, blocks, NINE, max_col, total, capacity=total - 1)
    _check_pack(p, want, "one byte short")
    assert p.st == [0] * 5 + [M.CAPACITY]


def test_unpack_capacity(dc, ref, max_col):
    mine = ref[20:26]
    containers = [buf for _, buf, _, _ in mine]
    expect = [(w, cols) for _, _, w, cols in mine]
    total = sum(w.total for w, _ in expect)
    u = _unpack(dc, containers, 64, max_col, total, sizing=True)
    assert u.off == _prefix([w.total for w, _ in expect])
    assert all(s == M.CAPACITY for s in u.st) and not any(u.osz) and not any(u.ncol)
    u = _unpack(dc, containers, 64, max_col, total, capacity=total - 1)
    assert _check_unpack(u, containers, expect, 64, "one byte short") == 5
    assert u.st == [0] * 5 + [M.CAPACITY]


# ---- hostile containers ------------------------------------------------------------------------------------------
def _expect_hostile(oracle, containers, max_columns, max_col_size):
    out = []
    for buf in containers:
        w = M.walk(buf, max_columns=max_columns, max_col_size=max_col_size)
        out.append((w, M.columns(buf, w, _decoder(oracle)) if w.status == 0 else None))
    return out


def test_every_walk_rule_on_the_device(dc, oracle):
    containers = [buf for _, buf, _ in WALK_CASES]
    expect = _expect_hostile(oracle, containers, 132, 64)
    assert [w.status for w, _ in expect] == [st for _, _, st in WALK_CASES]
    u = _unpack(dc, containers, 132, 64, sum(w.total for w, _ in expect if w.status == 0))
    _check_unpack(u, containers, expect, 132, "rules")
    assert u.st[:len(WALK_CASES)] == [st for _, _, st in WALK_CASES]              # (their streams are all sound)
    # the limits of the call
    buf = containers[[w for w, _, _ in WALK_CASES].index("128 positions")]
    for mc, ms in ((127, 64), (128, 0)):
        w = M.walk(buf, max_columns=mc, max_col_size=ms)
        assert w.status == M.UNSUPPORTED
        u = _unpack(dc, [buf], mc, ms, 0)
        _check_unpack(u, [buf], [(w, None)], mc, ("limits", mc, ms))


def test_damaged_fixtures_in_one_batch(dc, ref, oracle, max_col):
    rng = np.random.default_rng(77)
    containers = []
    for r in range(300):
        buf = bytearray(ref[int(rng.integers(len(ref)))][1])
        mode = r % 3
        if mode == 0:                                                               # anywhere
            for _ in range(int(rng.integers(1, 3))):
                buf[int(rng.integers(len(buf)))] ^= 1 << int(rng.integers(8))
        elif mode == 1:                                                             # a descriptor's neighbourhood
            w = M.walk(bytes(buf))
            c = w.cols[int(rng.integers(len(w.cols)))]
            at = c.get("stream_off", 9)
            buf[max(0, at - int(rng.integers(0, 3)))] = int(rng.integers(256))
        else:
            del buf[int(rng.integers(1, len(buf))):]
        containers.append(bytes(buf))
    expect = _expect_hostile(oracle, containers, 64, max_col)
    verdicts = {w.status for w, _ in expect}
    assert {0, M.TRUNCATED, M.UNSUPPORTED} <= verdicts, verdicts
    assert any(w.status == 0 and cols is None for w, cols in expect)                # a sound walk over a damaged stream
    u = _unpack(dc, containers, 64, max_col, sum(w.total for w, _ in expect if w.status == 0))
    assert _check_unpack(u, containers, expect, 64, "damaged") > 20
