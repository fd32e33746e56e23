"""tok3 name decoding on the device (include/rans4x16_hip.h part 2d): rans4x16_hip_tok3_names_dev and
rans4x16_hip_tok3_decode_names_dev against the Python model of the decoder (tok3_names_model.py, pinned by the
reference's own input files in test_tok3_names_cpu.py), on the 55 reference-made containers of tests/golden/tok3, on
column sets built token by token, on one block per rule that refuses, and on damaged columns.

Output arenas carry the position pattern of test_gpu_confinement.py and every byte outside the blocks' ranges is compared.
The expected results of the fixtures are computed once per module and not changed."""
import numpy as np
import pytest

import tok3_model as M
import tok3_names_model as N
from test_gpu_confinement import pattern
from test_tok3_names_cpu import block_columns

pytestmark = pytest.mark.gpu

GUARD = 4096
TYPE_COLUMN = 0x10000


class Block:
    """The columns of one name block as the stage is given them.  synth: ids whose descriptor carries
    R4X16_TOK3_TYPE_COLUMN - the type column of their position lies right in front of them and has no descriptor."""

    def __init__(self, cols, last_start, nreads, skip=0, synth=()):
        self.cols, self.last_start, self.nreads, self.skip, self.synth = sorted(cols), last_start, nreads, skip, set(synth)

    @property
    def ndesc(self):
        return len(self.cols) - len(self.synth)


@pytest.fixture(scope="module")
def ref(oracle):
    """Per fixture: (name, container, walk, [(id, bytes)], the names file with every line end a NUL, name starts)."""
    files = N.names_files()
    out = []
    for name, buf in M.fixtures():
        w = M.walk(buf)
        want = files[name.split(".")[0]].replace(b"\n", b"\0")
        starts = [0] + [i + 1 for i, ch in enumerate(want[:-1]) if ch == 0]
        out.append((name, buf, w, block_columns(buf, w, oracle), want, starts))
    assert len(out) == 55
    return out


@pytest.fixture(scope="module")
def dc(ref):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    d = htscodecs_amd.DeviceCodec(0)
    assert d.L.rans4x16_hip_set_dev_stripe_planes(d.ctx.h, 4, 2 * max(w.largest_col for _, _, w, _, _, _ in ref)) == 0
    yield d
    assert d.L.rans4x16_hip_set_dev_stripe_planes(d.ctx.h, 0, 0) == 0


def _prefix(sizes):
    return [0] + np.cumsum(np.asarray(sizes, dtype=np.int64)).tolist()


def _i32(values):
    return np.asarray(values, dtype=np.uint32).view(np.int32) if len(values) else np.zeros(0, dtype=np.int32)


class _Result:
    pass


def _outputs(dev, nblk, alloc, max_names, capacity, sizing):
    import torch
    r = _Result()
    r.alloc = alloc + GUARD
    r.pat = pattern(r.alloc)
    r.d_out = None if sizing else torch.from_numpy(r.pat.copy()).to(dev)
    r.d_off = torch.full((nblk + 1,), -7, dtype=torch.int64, device=dev)
    r.d_per = [torch.full((nblk,), -3, dtype=torch.int32, device=dev) for _ in range(3)]
    r.d_ns = torch.full((nblk * max_names,), -5, dtype=torch.int32, device=dev)
    r.max_names = max_names
    r.cap = 0 if sizing else (alloc if capacity is None else capacity)
    return r


def _collect(r):
    import torch
    torch.cuda.synchronize()
    r.arena = None if r.d_out is None else r.d_out.cpu().numpy()
    r.off = r.d_off.cpu().numpy().tolist()
    r.osz, r.nn, r.st = [x.cpu().numpy().view(np.uint32).tolist() for x in r.d_per]
    r.ns = r.d_ns.cpu().numpy().reshape(len(r.st), r.max_names)
    return r


def _lay_out(blocks, max_columns):
    """The column arena and the directory of `blocks`, as rans4x16_hip_tok3_unpack_dev leaves them."""
    arena = bytearray()
    n = len(blocks)
    cid = np.full((n, max_columns), -1, dtype=np.int32)
    coff = np.zeros((n, max_columns), dtype=np.int64)
    csz = np.zeros((n, max_columns), dtype=np.int32)
    ncol = []
    for b, blk in enumerate(blocks):
        d = 0
        lead = False
        for i, data in blk.cols:
            if (i & 15) == 0 and any((j >> 4) == (i >> 4) for j in blk.synth):
                assert len(data) == blk.nreads
                arena += data                                      # its descriptor is the next column's flag
                lead = True
                continue
            cid[b, d] = i | (TYPE_COLUMN if lead else 0)
            coff[b, d] = len(arena)
            csz[b, d] = len(data)
            arena += data
            lead = False
            d += 1
        assert d == blk.ndesc <= max_columns
        ncol.append(d)
    return bytes(arena), cid, coff, csz, ncol


def _names(dc, blocks, max_names, max_tokens=128, max_columns=None, capacity=None, sizing=False, with_status=True):
    import torch
    dev = dc.dev
    max_columns = max_columns or max(1, max(blk.ndesc for blk in blocks))
    arena, cid, coff, csz, ncol = _lay_out(blocks, max_columns)
    d_cols = torch.from_numpy(np.frombuffer(arena + b"\0" * 64, dtype=np.uint8).copy()).to(dev)[:max(len(arena), 1)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)
    r = _outputs(dev, len(blocks), sum(blk.last_start for blk in blocks if not blk.skip), max_names, capacity, sizing)
    dc.tok3_names(d_cols, up(cid), up(coff), up(csz), up(_i32(ncol)), up(_i32([blk.last_start for blk in blocks])),
                  up(_i32([blk.nreads for blk in blocks])), r.d_out, r.d_off, r.d_per[0], r.d_per[1], r.d_per[2],
                  max_columns, max_names, max_tokens, blk_status=up(_i32([blk.skip for blk in blocks])) if with_status else None,
                  name_start=r.d_ns, out_capacity=r.cap)
    return _collect(r)


def _expected(blocks, max_names, max_tokens, cap, hist_cap=None):
    """Per block (start, claim, status, bytes, name starts, may have written): the statuses in the order the call gives
    them - skipped, framing, history, capacity, then the decoder's."""
    out, off, hoff = [], 0, 0
    for blk in blocks:
        claim = 0 if blk.skip else blk.last_start
        start, off = off, off + claim
        data, starts, wrote = b"", [], False
        st = blk.skip or N.framing(blk.cols, blk.last_start, blk.nreads, max_names, max_tokens)
        if st == 0:
            hoff += N.history_units(blk.cols)
            if hist_cap is not None and hoff * 16 > hist_cap:
                st = N.UNSUPPORTED
            elif off > cap:
                st = N.CAPACITY
            else:
                st, data, starts = N.decode(blk.cols, blk.last_start, blk.nreads, max_names, max_tokens)
                wrote = True
        out.append((start, claim, st, data, starts, wrote))
    return out


def _check(r, expect, what):
    """Returns the number of blocks that came out whole."""
    assert r.off == _prefix([e[1] for e in expect]), (what, r.off[:8])
    mask = np.zeros(r.alloc, dtype=bool)
    whole = 0
    for i, (start, claim, st, data, starts, wrote) in enumerate(expect):
        tag = (what, i, r.st[i], st)
        assert r.st[i] == st, tag
        if wrote:
            mask[start:start + claim] = True                       # (a block that fails while it is decoded: unspecified bytes)
        if st != 0:
            assert r.osz[i] == 0 and r.nn[i] == 0, tag
            continue
        whole += 1
        assert r.osz[i] == len(data) == claim and r.nn[i] == len(starts), tag
        assert r.arena[start:start + claim].tobytes() == data, tag
        assert r.ns[i, :len(starts)].tolist() == starts, tag
        assert (r.ns[i, len(starts):] == -5).all(), tag
    if r.arena is not None:
        assert np.array_equal(r.arena[~mask], r.pat[~mask]), (what, "a byte outside the blocks' ranges changed")
    return whole


# ---- the fixtures ------------------------------------------------------------------------------------------------
def _decode_names(dc, ref, capacity=None, sizing=False, hint=True, max_col=None):
    import torch
    dev = dc.dev
    containers = [buf for _, buf, _, _, _, _ in ref]
    d_in = torch.from_numpy(np.frombuffer(b"".join(containers) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    in_off = torch.tensor(_prefix([len(c) for c in containers])[:-1], dtype=torch.int64, device=dev)
    in_size = torch.from_numpy(_i32([len(c) for c in containers])).to(dev)
    r = _outputs(dev, len(ref), sum(len(want) for _, _, _, _, want, _ in ref), 1000, capacity, sizing)
    dc.tok3_decode_names(d_in, in_off, in_size, r.d_out, r.d_off, r.d_per[0], r.d_per[1], r.d_per[2], 64,
                         max(len(c) for c in containers), max_col or max(w.largest_col for _, _, w, _, _, _ in ref), 1000, 32,
                         total_col_size=sum(w.total for _, _, w, _, _, _ in ref) if hint else 0, name_start=r.d_ns, out_capacity=r.cap)
    return _collect(r)


def _expect_fixtures(ref, cap):
    out, off = [], 0
    for _, _, _, _, want, starts in ref:
        start, off = off, off + len(want)
        out.append((start, len(want), 0, want, starts, True) if off <= cap else (start, len(want), N.CAPACITY, b"", [], False))
    return out


def test_decode_names_of_all_fixtures_in_one_call(dc, ref):
    total = sum(len(want) for _, _, _, _, want, _ in ref)
    r = _decode_names(dc, ref)
    assert _check(r, _expect_fixtures(ref, total), "all") == 55
    assert sum(r.nn) == 55000
    # a capacity that ends inside block 20: that block is not written, the rest are whole
    cut = r.off[20] + 100
    short = _decode_names(dc, ref, capacity=cut)
    expect = _expect_fixtures(ref, cut)
    assert [e[2] for e in expect] == [0] * 20 + [N.CAPACITY] * 35
    assert _check(short, expect, "cut") == 20
    sizing = _decode_names(dc, ref, sizing=True)
    assert sizing.off == r.off and all(s == N.CAPACITY for s in sizing.st) and not any(sizing.osz) and not any(sizing.nn)


def test_the_names_arena_grows_and_is_reused(dc, ref):
    """A fresh context, the one-call form over 3 fixtures (containers of 2 to 11 KiB), then 13, then 3 again: the first
    call allocates the names arena (the columns, then the histories), the second finds it too small and grows it -
    synchronize, free, allocate - and the third lays both out in an arena larger than it asked for."""
    import htscodecs_amd
    fresh = htscodecs_amd.DeviceCodec(0)
    assert fresh.L.rans4x16_hip_set_dev_stripe_planes(fresh.ctx.h, 4, 2 * max(w.largest_col for _, _, w, _, _, _ in ref)) == 0
    for n in (3, 13, 3):
        part = ref[:n]
        r = _decode_names(fresh, part)
        assert _check(r, _expect_fixtures(part, r.cap), ("regrow", n)) == n


def test_decode_names_without_a_size_hint(dc, ref):
    part = ref[:3]
    r = _decode_names(dc, part, hint=False, max_col=max(w.largest_col for _, _, w, _, _, _ in part))
    assert _check(r, _expect_fixtures(part, r.cap), "no hint") == 3


def test_unpack_then_names_gives_the_same_arena(dc, ref):
    import torch
    dev = dc.dev
    containers = [buf for _, buf, _, _, _, _ in ref]
    n, maxc = len(containers), 64
    d_in = torch.from_numpy(np.frombuffer(b"".join(containers) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    in_off = torch.tensor(_prefix([len(c) for c in containers])[:-1], dtype=torch.int64, device=dev)
    in_size = torch.from_numpy(_i32([len(c) for c in containers])).to(dev)
    d_cols = torch.zeros(sum(w.total for _, _, w, _, _, _ in ref), dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    per = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(5)]
    cid = torch.zeros(n * maxc, dtype=torch.int32, device=dev)
    coff = torch.zeros(n * maxc, dtype=torch.int64, device=dev)
    csz = torch.zeros(n * maxc, dtype=torch.int32, device=dev)
    dc.tok3_unpack(d_in, in_off, in_size, d_cols, off, per[0], per[1], per[2], per[3], per[4], cid, coff, csz, maxc,
                   max(len(c) for c in containers), max(w.largest_col for _, _, w, _, _, _ in ref))
    total = sum(len(want) for _, _, _, _, want, _ in ref)
    r = _outputs(dev, n, total, 1000, None, False)
    dc.tok3_names(d_cols, cid, coff, csz, per[2], per[3], per[4], r.d_out, r.d_off, r.d_per[0], r.d_per[1], r.d_per[2],
                  maxc, 1000, 32, blk_status=per[1], name_start=r.d_ns)
    _collect(r)
    assert _check(r, _expect_fixtures(ref, total), "two calls") == 55
    one = _decode_names(dc, ref)
    assert np.array_equal(one.arena, r.arena) and one.off == r.off and one.ns.tolist() == r.ns.tolist()
    assert any(int(x) & TYPE_COLUMN for x in cid.cpu().numpy())                    # synthesised type columns went through


# ---- constructed blocks ------------------------------------------------------------------------------------------
class Builder:
    """Token columns written by hand.  name(kind, dist, tokens): tokens for positions 1, 2, ..:
    ("char", c) ("alpha", bytes) ("digits0", v, vl) ("digits", v) ("ddelta", d) ("ddelta0", d) ("match",) ("nop",)
    ("end",) ("type", t): a bare type byte."""

    def __init__(self):
        self.cols = {}
        self.count = 0

    def put(self, cid, data):
        self.cols.setdefault(cid, bytearray()).extend(data)

    def name(self, kind, dist, tokens=()):
        self.count += 1
        self.put(0, [kind])
        self.put(kind, dist.to_bytes(4, "little"))
        for t, tok in enumerate(tokens, 1):
            what, args = tok[0], tok[1:]
            base = t << 4
            if what == "char":
                self.put(base, [N.N_CHAR]); self.put(base | N.N_CHAR, args[0])
            elif what == "alpha":
                self.put(base, [N.N_ALPHA]); self.put(base | N.N_ALPHA, args[0] + b"\0")
            elif what == "digits0":
                self.put(base, [N.N_DIGITS0]); self.put(base | N.N_DZLEN, [args[1]]); self.put(base | N.N_DIGITS0, args[0].to_bytes(4, "little"))
            elif what == "digits":
                self.put(base, [N.N_DIGITS]); self.put(base | N.N_DIGITS, args[0].to_bytes(4, "little"))
            elif what == "ddelta":
                self.put(base, [N.N_DDELTA]); self.put(base | N.N_DDELTA, [args[0]])
            elif what == "ddelta0":
                self.put(base, [N.N_DDELTA0]); self.put(base | N.N_DDELTA0, [args[0]])
            elif what == "match":
                self.put(base, [N.N_MATCH])
            elif what == "nop":
                self.put(base, [N.N_NOP])
            elif what == "end":
                self.put(base, [N.N_END])
            else:
                self.put(base, [args[0]])
        return self

    def block(self, last_start=None, nreads=None, delta=0, synth=(), skip=0, edit=None):
        """last_start None: what the block decodes to (64 for one that fails anyway), plus delta."""
        cols = {k: bytes(v) for k, v in self.cols.items()}
        if edit:
            edit(cols)
        cols = sorted(cols.items())
        nreads = self.count if nreads is None else nreads
        if last_start is None:
            st, data, _ = N.decode(cols, None, max(nreads, self.count))
            last_start = (len(data) if st == 0 else 64) + delta
        return Block(cols, last_start, nreads, skip=skip, synth=synth)


E, MT = ("end",), ("match",)


def _blocks_of_every_kind():
    out = {}
    b = Builder()
    b.name(N.N_DIFF, 0, [("alpha", b"SRR"), ("char", b":"), ("digits0", 42, 5), ("char", b"."), ("digits", 1234567), ("nop",), ("alpha", b"x"), E])
    b.name(N.N_DIFF, 1, [MT, MT, MT, MT, MT, ("nop",), MT, E])                      # N_MATCH of each of the four kinds
    b.name(N.N_DIFF, 1, [MT, MT, ("ddelta0", 3), MT, ("ddelta", 255), ("nop",), ("alpha", b""), E])
    b.name(N.N_DIFF, 3, [MT, ("char", b"/"), ("digits0", 7, 0), MT, ("digits", 0), ("nop",), MT, E])      # vl 0, N_DIGITS 0
    b.name(N.N_DIFF, 0, [("digits", 4294967290), ("digits0", 99, 2), ("digits0", 123456789, 9), ("digits0", 1234, 2), E])
    b.name(N.N_DIFF, 1, [("ddelta", 10), ("ddelta0", 5), ("ddelta0", 1), MT, E])     # wraps at 2^32; overflows its width
    b.name(N.N_DIFF, 1, [MT, MT, MT, MT, E])
    b.name(N.N_DIFF, 0, [E])                                                         # an empty name
    out["kinds"] = b.block()
    assert N.decode(out["kinds"].cols, out["kinds"].last_start, 8)[1].split(b"\0")[:6] == [
        b"SRR:00042.1234567x", b"SRR:00042.1234567x", b"SRR:00045.1234822", b"SRR/.x", b"429496729099123456789" + bytes([123 + 48]) + b"4",
        b"4" + bytes([10 + 48]) + b"4123456790" + bytes([123 + 48]) + b"4"]

    b = Builder()                                                                    # distances
    for i in range(70):
        special = {60: 1, 61: 2, 64: 63, 65: 64, 66: 65, 69: 69}.get(i)
        if special is None:
            b.name(N.N_DIFF, 0, [("alpha", b"a%d" % i), ("char", b"-"), ("digits", i), E])
        else:
            b.name(N.N_DIFF, special, [MT, MT, ("digits", 1000 + i), E])
    out["dist"] = b.block()
    got = N.decode(out["dist"].cols, out["dist"].last_start, 70)[1].split(b"\0")
    assert (got[60], got[61], got[64], got[65], got[66], got[69]) == (b"a59-1060", b"a59-1061", b"a1-1064", b"a1-1065", b"a1-1066", b"a0-1069")

    b = Builder()                                                                    # a duplicate of a duplicate, then a name against it
    b.name(N.N_DIFF, 0, [("alpha", b"read"), ("digits", 7), ("nop",), ("digits0", 5, 3), E])
    b.name(N.N_DUP, 1).name(N.N_DUP, 1)
    b.name(N.N_DIFF, 1, [MT, ("ddelta", 1), ("nop",), ("ddelta0", 1), E])
    b.name(N.N_DUP, 3).name(N.N_DUP, 2)
    out["dup"] = b.block()
    assert N.decode(out["dup"].cols, out["dup"].last_start, 6)[1] == b"read7005\0" * 3 + b"read8006\0" + b"read7005\0" + b"read8006\0"

    b = Builder()                                                                    # names that end at positions 1, 2, 63, 64, 65, 127
    for end in (127, 1, 2, 63, 64, 65):
        b.name(N.N_DIFF, 0, [("char", bytes([65 + (t * 7 + end) % 26])) for t in range(1, end)] + [E])
    b.name(N.N_DIFF, 6, [MT] * 126 + [E])                                            # all of the first, both passes
    b.name(N.N_DIFF, 1, [MT] * 63 + [("char", b"!")] + [MT] * 62 + [E])
    b.name(N.N_DUP, 1)
    b.name(N.N_DIFF, 4, [MT] * 64 + [("alpha", b"tail"), E])
    out["ends"] = b.block()
    got = N.decode(out["ends"].cols, out["ends"].last_start, 10)[1].split(b"\0")
    assert [len(g) for g in got[:10]] == [126, 0, 1, 62, 63, 64, 126, 126, 126, 68] and got[6] == got[0] and got[7][63:64] == b"!"

    b = Builder()                                                                    # an elided end: the type column of position 2 runs out
    b.name(N.N_DIFF, 0, [("char", b"a"), E]).name(N.N_DIFF, 1, [MT]).name(N.N_DIFF, 0, [("char", b"c")])
    out["elided"] = b.block()
    assert N.decode(out["elided"].cols, 6, 3) == (0, b"a\0a\0c\0", [0, 2, 4])

    b = Builder()                                                                    # strings
    for n in (0, 1, 7, 8, 9, 255, 256, 1000, 1021, 1022, 2000):                       # 1021: the longest name that is staged in LDS
        s = bytes(97 + (i * 31 + n) % 26 for i in range(n))
        b.name(N.N_DIFF, 0, [("char", b"<"), ("alpha", s), ("char", b">"), E])
        b.name(N.N_DIFF, 1, [MT, MT, ("char", b"]"), E])
    out["alpha"] = b.block()

    for count in (1, 2, 64, 65):
        b = Builder()
        for i in range(count):
            b.name(N.N_DIFF, 0 if i == 0 else 1, [("alpha", b"q")] + [("digits", 100 + i) if i % 9 == 0 else ("ddelta", 1)] + [E])
        out["count %d" % count] = b.block()
    assert N.decode(out["count 65"].cols, out["count 65"].last_start, 65)[1].endswith(b"q163\0q164\0")

    b = Builder()                                                                    # a synthesised type column: the type, then N_MATCH
    b.name(N.N_DIFF, 0, [("char", b"x"), ("digits", 5), E])
    for i in range(4):
        b.name(N.N_DIFF, 1, [MT, ("ddelta", 2), E])
    blk = b.block(synth=(0x12,))
    assert dict(blk.cols)[0x10] == bytes([N.N_CHAR]) + bytes([N.N_MATCH]) * 4 and blk.ndesc == len(blk.cols) - 1
    out["synth"] = blk
    return out


def test_constructed_blocks(dc):
    kinds = _blocks_of_every_kind()
    blocks = list(kinds.values())
    assert all(N.decode(b.cols, b.last_start, b.nreads)[0] == 0 for b in blocks)
    cap = sum(b.last_start for b in blocks)
    r = _names(dc, blocks, 70)
    assert _check(r, _expected(blocks, 70, 128, cap), list(kinds)) == len(blocks)
    # without the optional arrays, and every block alone
    r = _names(dc, blocks, 70, with_status=False)
    assert _check(r, _expected(blocks, 70, 128, cap), "no status array") == len(blocks)
    for what, blk in kinds.items():
        r = _names(dc, [blk], blk.nreads, max_tokens=max(i >> 4 for i, _ in blk.cols) + 1)
        assert _check(r, _expected([blk], blk.nreads, 128, blk.last_start), what) == 1


# ---- one block per rule that refuses ---------------------------------------------------------------------------------
def _good(k):
    b = Builder()
    b.name(N.N_DIFF, 0, [("alpha", b"good%d" % k), ("digits", k), E]).name(N.N_DIFF, 1, [MT, ("ddelta", 1), E]).name(N.N_DUP, 2)
    return b.block()


def _refusals():
    """[(what, block, status)]"""
    base = lambda: Builder().name(N.N_DIFF, 0, [("alpha", b"ab"), ("digits", 7), ("nop",), ("digits0", 5, 3), ("char", b"c"), E])
    out = []
    add = lambda what, blk, st: out.append((what, blk, st))

    def cut(cid, n=1):
        def edit(cols):
            cols[cid] = cols[cid][:-n]
        return edit

    add("more names than nreads", base().name(N.N_DUP, 1).block(nreads=1), N.SIZE)
    add("nreads of zero", base().block(nreads=0), N.SIZE)
    add("a size above last_start", base().name(N.N_DUP, 1).block(delta=-1), N.SIZE)
    add("a size below last_start", base().block(delta=1), N.SIZE)
    add("last_start out of range", base().block(last_start=0x7FFFFFFF - 1024), N.SIZE)
    add("first type is a token", Builder().name(N.N_MATCH, 0, [E]).block(), N.SIZE)
    add("first type is N_END", Builder().name(N.N_DIFF, 0, [E]).name(N.N_END, 0, [E]).block(), N.SIZE)
    add("distance runs out", base().name(N.N_DIFF, 1, [MT, E]).block(edit=cut(N.N_DIFF)), N.TRUNCATED)
    add("distance beyond the first name", base().name(N.N_DIFF, 2, [E]).block(), N.SIZE)
    add("duplicate of itself", base().name(N.N_DUP, 0).block(), N.SIZE)
    add("no end", Builder().name(N.N_DIFF, 0, [("char", b"a"), ("char", b"b")]).block(), N.SIZE)
    add("match beyond the end", base().name(N.N_DIFF, 1, [MT] * 6 + [E]).block(), N.SIZE)
    add("match without an earlier name", Builder().name(N.N_DIFF, 0, [MT, E]).block(), N.SIZE)
    add("ddelta beyond the end", base().name(N.N_DIFF, 1, [MT] * 5 + [("ddelta", 1), E]).block(), N.SIZE)
    add("ddelta0 beyond the end", base().name(N.N_DIFF, 1, [MT] * 5 + [("ddelta0", 1), E]).block(), N.SIZE)
    add("match of a nop", base().name(N.N_DIFF, 1, [MT, MT, MT, E]).block(), N.SIZE)
    add("char runs out", base().block(edit=cut(0x52)), N.TRUNCATED)
    add("digits run out", base().block(edit=cut(0x27)), N.TRUNCATED)
    add("digits0 run out", base().block(edit=cut(0x43)), N.TRUNCATED)
    add("dzlen runs out", base().block(edit=cut(0x44)), N.TRUNCATED)
    add("ddelta runs out", base().name(N.N_DIFF, 1, [MT, ("ddelta", 1), E]).block(edit=cut(0x28)), N.TRUNCATED)
    add("ddelta0 runs out", base().name(N.N_DIFF, 1, [MT, MT, ("nop",), ("ddelta0", 1), E]).block(edit=cut(0x49)), N.TRUNCATED)
    add("ddelta on a string", base().name(N.N_DIFF, 1, [("ddelta", 1), E]).block(), N.SIZE)
    add("ddelta on fixed digits", base().name(N.N_DIFF, 1, [MT, MT, ("nop",), ("ddelta", 1), E]).block(), N.SIZE)
    add("ddelta0 on digits", base().name(N.N_DIFF, 1, [MT, ("ddelta0", 1), E]).block(), N.SIZE)
    add("a width of ten", Builder().name(N.N_DIFF, 0, [("digits0", 5, 10), E]).block(), N.SIZE)
    add("a string without its end", base().block(edit=cut(0x11)), N.TRUNCATED)
    add("a string of no bytes at all", base().block(edit=cut(0x11, 3)), N.TRUNCATED)
    add("the lowest position decides", Builder().name(N.N_DIFF, 0, [("digits", 1), MT, E]).block(edit=cut(0x17)), N.TRUNCATED)
    add("skipped", base().block(skip=N.TRUNCATED), N.TRUNCATED)
    return out


def test_every_rule_that_refuses_beside_a_good_neighbour(dc):
    cases = _refusals()
    blocks = []
    for k, (what, blk, st) in enumerate(cases):
        got = blk.skip or N.decode(blk.cols, blk.last_start, blk.nreads)[0]
        assert got == st, (what, got)
        blocks += [blk, _good(k)]
    assert len(blocks) <= 64
    cap = sum(b.last_start for b in blocks if not b.skip)
    expect = _expected(blocks, 8, 128, cap)
    assert [e[2] for e in expect] == [x for _, _, st in cases for x in (st, 0)]
    r = _names(dc, blocks, 8)
    assert _check(r, expect, [c[0] for c in cases]) == len(cases)


def test_limits_one_short_of_need(dc):
    kinds = _blocks_of_every_kind()
    blk, good = kinds["ends"], _good(1)
    for max_names, max_tokens, st in ((10, 128, 0), (9, 128, N.UNSUPPORTED), (10, 127, N.UNSUPPORTED)):
        blocks = [good, blk, good]
        expect = _expected(blocks, max_names, max_tokens, sum(b.last_start for b in blocks))
        assert [e[2] for e in expect] == [0, st, 0]
        r = _names(dc, blocks, max_names, max_tokens=max_tokens)
        _check(r, expect, (max_names, max_tokens))


def test_history_that_does_not_fit_under_a_lowered_workspace(dc):
    blk = _blocks_of_every_kind()["ends"]                                               # 10 names x 128 positions: 10,400 bytes
    assert N.history_units(blk.cols) * 16 == 10 * (128 * 8 + 16)
    blocks = [blk] * 64
    saved = dc.get_option("max_workspace_mb")
    dc.set_option("max_workspace_mb", 1)
    try:
        r = _names(dc, blocks, 10)
    finally:
        dc.set_option("max_workspace_mb", saved)
    expect = _expected(blocks, 10, 128, 64 * blk.last_start, hist_cap=(1 << 20) // 2)
    assert [e[2] for e in expect] == [0] * 50 + [N.UNSUPPORTED] * 14                  # 50 histories fit half a megabyte
    assert _check(r, expect, "history") == 50
    r = _names(dc, blocks, 10)
    assert _check(r, _expected(blocks, 10, 128, 64 * blk.last_start), "history, default workspace") == 64


# ---- damaged columns -------------------------------------------------------------------------------------------------
def damaged_blocks(ref, seed=20250117, n=300):
    rng = np.random.default_rng(seed)
    blocks = []
    for _ in range(n):
        _, _, w, cols, _, _ = ref[int(rng.integers(len(ref)))]
        k = int(rng.choice([i for i, (_, d) in enumerate(cols) if d]))
        data = bytearray(cols[k][1])
        data[int(rng.integers(len(data)))] ^= 1 << int(rng.integers(8))
        blocks.append(Block(cols[:k] + [(cols[k][0], bytes(data))] + cols[k + 1:], w.last_start, w.nreads))
    return blocks


def test_damaged_columns_in_one_batch(dc, ref):
    blocks = damaged_blocks(ref)
    cap = sum(b.last_start for b in blocks)
    expect = _expected(blocks, 1000, 32, cap)
    good = sum(e[2] == 0 for e in expect)
    assert good >= 20 and len(blocks) - good >= 20, good
    r = _names(dc, blocks, 1000, max_tokens=32)
    assert _check(r, expect, "damaged") == good
