"""tok3 names on the device against the REFERENCE's answers at the tokeniser's branches (tests/golden/tok3/edge.bin,
README.edge.md beside it: 153 small blocks, one per branch and side, with the containers the reference wrote for them in
both flavours): rans4x16_hip_tok3_tokenise_dev against the reference's columns, rans4x16_hip_tok3_encode_names_dev
against its containers byte for byte, rans4x16_hip_tok3_decode_names_dev (and unpack, then names) over its containers of
both flavours in one batch, the host entry points, and the tokeniser kernel against the Python model - which
tests/test_tok3_edge_cpu.py pins to the reference where the kernel's branches are - on 200 random blocks.

Nothing here runs the reference: the fixture is read, and that is all.  Output arenas carry the position pattern of
test_gpu_confinement.py and every byte outside the results is compared; the blocks lie 3 or 5 bytes apart in the input,
so that they start at every address mod 8.  The reference's columns are decoded once per module and not changed."""
import numpy as np
import pytest

import tok3_arith_model as TA
import tok3_edge_cases as X
import tok3_enc_model as E
import tok3_model as M
import test_gpu_tok3_enc as TE
import test_gpu_tok3_names as TN
from test_tok3_edge_cpu import KINDS, described, reference_columns

pytestmark = pytest.mark.gpu

DECODE, ENCODE = 1, 2
LIMITS = dict(max_in_size=1 << 14, max_names=1024, max_name_len=256, max_tokens=128, max_columns=512)


@pytest.fixture(scope="module")
def ref(oracle):
    """{(case name, level, use_arith): (walk, [(id, bytes)] of every column of the reference's container)}"""
    out = {}
    for c in X.cases():
        for v in c.vectors:
            out[c.name, v.level, v.use_arith] = reference_columns(v.container, oracle)
    assert len(out) == 489
    assert max(w.ndesc for w, _ in out.values()) <= LIMITS["max_columns"]
    assert max(len(c.block) for c in X.cases()) <= LIMITS["max_in_size"]
    return out


@pytest.fixture(scope="module")
def dc(ref):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    d = htscodecs_amd.DeviceCodec(0)
    # (for the decodes: X_STRIPE columns of the levels 3, 5 and 9; a plane buffer per column slot of the batch, so no larger
    #  than the largest column)
    assert d.L.rans4x16_hip_set_dev_stripe_planes(d.ctx.h, 4, max(w.largest_col for w, _ in ref.values())) == 0
    assert d.set_tok3_arith(0) == 0
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
    return codec._Ctx()


class _mode:
    """the tok3_arith mode of a device codec for a with-block"""

    def __init__(self, dc, mode):
        self.dc, self.mode = dc, mode

    def __enter__(self):
        self.was = self.dc.set_tok3_arith(self.mode)

    def __exit__(self, *exc):
        assert self.dc.set_tok3_arith(self.was) == self.mode


# ---- the tokeniser against the reference's columns -----------------------------------------------------------------
def _reference_expectation(cases, ref):
    """What TE._check takes per block - (start, claim, status, [(id, bytes)], last_start, nreads) - from the columns of the
    reference's level-1 rANS container (every vector of a case holds the same columns: test_tok3_edge_cpu.py)."""
    out, off = [], 0
    for c in cases:
        w, cols = ref[c.name, 1, 0]
        want = described(w, cols)
        claim = sum(len(d) for _, d in want)
        out.append((off, claim, 0, want, w.last_start, w.nreads))
        off += claim
    return out


@pytest.mark.parametrize("slots", [0, 1, 64])
def test_tokenise_gives_the_references_columns_in_one_batch(dc, ref, slots):
    """search_slots 0: the default table; 1: the exact search alone; 64: a table that fills up inside dup_999."""
    cases = X.cases()
    expect = _reference_expectation(cases, ref)
    r = TE._tokenise(dc, [c.block for c in cases], LIMITS, search_slots=slots)
    assert TE._check(r, expect, "edge.bin, search_slots %d" % slots) == 153


def test_tokenise_gives_the_references_columns_case_by_case(dc, ref):
    for k, c in enumerate(X.cases()):
        expect = _reference_expectation([c], ref)
        r = TE._tokenise(dc, [c.block], LIMITS, gap=1 + k % 8)
        assert TE._check(r, expect, c.name) == 1, c.name


# ---- the encoder against the reference's containers ----------------------------------------------------------------
@pytest.mark.parametrize("level,use_arith", KINDS)
def test_encode_names_writes_the_references_containers(dc, level, use_arith):
    picked = X.vectors(use_arith, level)
    assert len(picked) == (153 if level in (1, 7) else 10)
    blocks = [c.block for c, _ in picked]
    with _mode(dc, ENCODE if use_arith else 0):
        r = TE._encode_names(dc, blocks, M.REF_LISTS[level], LIMITS)
    got = TE._containers(r, (level, use_arith))
    assert r.st == [0] * len(picked)
    differ = [c.name for (c, v), mine in zip(picked, got) if mine != v.container]
    assert not differ, differ


# ---- the decoder over the reference's containers -------------------------------------------------------------------
def _decode_names(dc, containers, walks, total, gap=5):
    """rans4x16_hip_tok3_decode_names_dev over `containers`, laid out `gap` bytes apart."""
    import torch
    dev = dc.dev
    raw, offs = bytearray(b"\xee" * gap), []
    for buf in containers:
        offs.append(len(raw))
        raw += buf + b"\xee" * gap
    d_in = torch.from_numpy(np.frombuffer(bytes(raw) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    in_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    in_size = torch.from_numpy(TN._i32([len(c) for c in containers])).to(dev)
    r = TN._outputs(dev, len(containers), total, LIMITS["max_names"], None, False)
    dc.tok3_decode_names(d_in, in_off, in_size, r.d_out, r.d_off, r.d_per[0], r.d_per[1], r.d_per[2], max(w.ndesc for w in walks),
                         max(len(c) for c in containers), max(w.largest_col for w in walks), LIMITS["max_names"], 128,
                         total_col_size=sum(w.total for w in walks), name_start=r.d_ns, out_capacity=r.cap)
    return TN._collect(r), (d_in, in_off, in_size)


def _names_expectation(picked):
    out, off = [], 0
    for c, v in picked:
        want = X.names_of(c.block, v.last_start)
        starts = [0] + [i + 1 for i, ch in enumerate(want[:-1]) if ch == 0] if want else []
        out.append((off, len(want), 0, want, starts, True))
        off += len(want)
    return out


def test_decode_names_of_the_references_containers_of_both_flavours(dc, ref):
    """All 489 containers, rANS and arith side by side, in one call; then unpack and names as two calls: the same arena."""
    import torch
    picked = X.vectors()
    assert len(picked) == 489 and sum(v.use_arith for _, v in picked) == 153
    containers = [v.container for _, v in picked]
    walks = [ref[c.name, v.level, v.use_arith][0] for c, v in picked]
    expect = _names_expectation(picked)
    total = sum(e[1] for e in expect)
    with _mode(dc, DECODE):
        one, (d_in, in_off, in_size) = _decode_names(dc, containers, walks, total)
        assert TN._check(one, expect, "edge.bin, both flavours") == 489
        dev, n, maxc = dc.dev, len(containers), max(w.ndesc for w in walks)
        d_cols = torch.zeros(sum(w.total for w in walks), dtype=torch.uint8, device=dev)
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        per = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(5)]
        cid = torch.zeros(n * maxc, dtype=torch.int32, device=dev)
        coff = torch.zeros(n * maxc, dtype=torch.int64, device=dev)
        csz = torch.zeros(n * maxc, dtype=torch.int32, device=dev)
        dc.tok3_unpack(d_in, in_off, in_size, d_cols, off, per[0], per[1], per[2], per[3], per[4], cid, coff, csz, maxc,
                       max(len(c) for c in containers), max(w.largest_col for w in walks))
    torch.cuda.synchronize()
    assert per[1].cpu().numpy().tolist() == [0] * n
    # the unpacked columns are the reference's
    arena, at = d_cols.cpu().numpy(), off.cpu().numpy().tolist()
    for k, (c, v) in enumerate(picked):
        want = b"".join(d for _, d in ref[c.name, v.level, v.use_arith][1])
        assert arena[at[k]:at[k + 1]].tobytes() == want, (c.name, v.level, v.use_arith)
    two = TN._outputs(dev, n, total, LIMITS["max_names"], None, False)
    dc.tok3_names(d_cols, cid, coff, csz, per[2], per[3], per[4], two.d_out, two.d_off, two.d_per[0], two.d_per[1], two.d_per[2],
                  maxc, LIMITS["max_names"], 128, blk_status=per[1], name_start=two.d_ns)
    TN._collect(two)
    assert TN._check(two, expect, "unpack, then names") == 489
    assert np.array_equal(one.arena, two.arena) and one.off == two.off and one.ns.tolist() == two.ns.tolist()


# ---- the host entry points -----------------------------------------------------------------------------------------
def test_host_entry_points_on_the_largest_and_the_smallest_cases(H):
    """encode_names / decode_names of include/tok3_names_hip.h (the two single-block symbols per flavour behind them) and
    the two _batch calls: the ten largest blocks - the ones with vectors at all five levels - and the five smallest."""
    from htscodecs_amd import codec
    by_size = sorted(X.cases(), key=lambda c: -len(c.block))
    cases = by_size[:10] + by_size[-5:]
    assert all(len(c.vectors) == 6 for c in cases[:10]) and all(len(c.vectors) == 3 for c in cases[10:])
    for c in cases:
        for v in c.vectors:
            tag = (c.name, v.level, v.use_arith)
            assert codec.encode_names(c.block, v.level, use_arith=v.use_arith) == (v.container, v.last_start), tag
            assert codec.decode_names(v.container) == X.names_of(c.block, v.last_start), tag
    for level, use_arith in KINDS:
        picked = [(c, v) for c in cases for v in c.vectors if (v.level, v.use_arith) == (level, use_arith)]
        assert len(picked) == (15 if level in (1, 7) else 10)
        res, last_start, st = codec.tok3_encode_names_batch([c.block for c, _ in picked], methods=M.REF_LISTS[level], ctx=H, tok3_arith=use_arith)
        assert st == [0] * len(picked) and res == [v.container for _, v in picked], (level, use_arith)
        assert last_start == [v.last_start for _, v in picked], (level, use_arith)
        assert codec.tok3_encode_names_batch([c.block for c, _ in picked], level=level, ctx=H, tok3_arith=use_arith)[0] == res
    every = [(c, v) for c in cases for v in c.vectors]
    names, st = codec.tok3_decode_names_batch([v.container for _, v in every], ctx=H, tok3_arith=1)
    assert st == [0] * len(every) and names == [X.names_of(c.block, v.last_start) for c, v in every]
    assert codec.set_tok3_arith(0, H) == 0


# ---- the kernel against the model ----------------------------------------------------------------------------------
def test_tokenise_against_the_model_on_random_blocks(dc):
    """200 seeded random blocks in one batch: a quarter with names of 65 to 120 tokens (the tokeniser's second pass), a
    quarter with 300 and more names from a pool of 10 (N_DUP and exact hits), and between them one block of each kind the
    model refuses (README.edge.md's inputs that are no vectors): statuses, directory and bytes."""
    kinds = (X.PLAIN, X.LONG, X.PLAIN, X.DUPS)
    blocks = X.random_blocks(4242, 200, kinds, max_names=60, max_len=40)
    body = (b"a1" * 64)[:127]
    refused = [(17, b"ab\n" + body + b"\n", E.UNSUPPORTED), (58, b"ok\ncaf\xc3\xa9\nok\n", E.UNSUPPORTED), (99, b"no end", E.SIZE),
               (140, b"", E.SIZE)]
    for at, block, _ in refused:
        blocks.insert(at, block)
    blocks.insert(181, b"ok\nfine\ncaf\xc3\xa9")                          # a byte >= 0x80 in the tail: coded
    assert max(len(b) for b in blocks) <= LIMITS["max_in_size"]
    alloc = sum(E.bound(len(b)) for b in blocks)
    expect = TE._expected(blocks, LIMITS, alloc)
    assert all(expect[at][2] == st for at, _, st in refused) and expect[181][2:] == (0, E.tokenise(b"ok\nfine\n")[1], 8, 2)
    assert sum(e[2] == 0 for e in expect) == 201
    tall = sum(e[2] == 0 and max(cid >> 4 for cid, _ in e[3]) >= 66 for e in expect)
    many = sum(e[5] >= 300 for e in expect)
    assert tall >= 50 and many == 50, (tall, many)
    dups = sum(dict(e[3]).get(0, b"").count(E.N_DUP) for e in expect)
    assert dups >= 10000, dups
    assert TE._check(TE._tokenise(dc, blocks, LIMITS), expect, "random blocks") == 201
