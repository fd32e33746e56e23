"""How the device calls start, and how the plain slot calls walk a batch in chunks.

Entry: every slot call (eight arrays, a slot per block) and every packed call (results back to back, the offsets written
by the call) of rANS 4x16, rANS 4x8 and the packed best-of-k of arith_dynamic, through the bindings of htscodecs_amd.lib
on one context.  One block of 64 bytes.  What a call returns and what rans4x16_hip_last_error holds afterwards, for a
required pointer that is null, a negative count, an empty batch, a method table the call refuses - with and without
blocks - and a null pointer beside such a table.  The expected values are literals: the texts of the C sources, and the
order in which each call tests.  Every refused call returns before anything is enqueued; the others run the one block.

Chunks: the four plain slot calls over 40 blocks of 4 KiB under a ceiling that cuts the batch into three chunks with a
shorter last one, against the same call under the default ceiling."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIPES_256 = (256 << 8) | 8            # X_STRIPE with 256 planes
MARK = "peek_dev: bad arguments"        # the text a refused rans4x16_hip_peek_dev leaves: a call that succeeds keeps it
PRESET = 0x5a5a5a5a
OUT = 1 << 18                           # above the bound of 64 bytes under order 1 (its table alone may take 198,147)

# name -> (the text of its refusal, what follows d_status)
SLOT = {
    "rans4x16_hip_compress_dev_sized": ("compress_dev: bad arguments", (1, None, 64, 0)),
    "rans4x16_hip_uncompress_dev_sized": ("uncompress_dev: bad arguments", (4096, OUT, 0)),
    "rans4x8_hip_compress_dev": ("rans4x8 compress_dev: bad arguments", (1, None, 64)),
    "rans4x8_hip_uncompress_dev": ("rans4x8 uncompress_dev: bad arguments", ()),
    "rans4x16_hip_compress_best_dev": ("compress_best_dev: bad arguments", ("k", "methods", None, 64, 0)),
    "rans4x8_hip_compress_best_dev": ("rans4x8 compress_best_dev: bad arguments", ("k", "methods", None, 64)),
}
PACKED = {
    "rans4x16_hip_compress_packed_dev": ("compress_packed_dev: bad arguments", (1, None, 64, 0)),
    "rans4x16_hip_compress_best_packed_dev": ("compress_best_packed_dev: bad arguments", ("k", "methods", None, 64, 0)),
    "rans4x16_hip_uncompress_packed_dev": ("uncompress_packed_dev: bad arguments", (None, 4096, 64)),
    "rans4x8_hip_compress_packed_dev": ("rans4x8 compress_packed_dev: bad arguments", (1, None, 64)),
    "rans4x8_hip_compress_best_packed_dev": ("rans4x8 compress_best_packed_dev: bad arguments", ("k", "methods", None, 64)),
    "rans4x8_hip_uncompress_packed_dev": ("rans4x8 uncompress_packed_dev: bad arguments", (4096, 64)),
    "rans4x16_hip_arith_compress_best_packed_dev": ("arith_compress_best_packed_dev: bad arguments", ("k", "methods", None, 64, 0)),
}
# the calls that take a method table: name -> [(k, methods or None, the refusal's text)], the good table first (text None)
TABLES = {
    "rans4x16_hip_compress_best_dev": [(2, [0, 1], None), (1, [STRIPES_256], "compress_best_dev: more than 255 stripes"),
                                       (0, [0], "compress_best_dev: bad arguments"), (33, [0] * 33, "compress_best_dev: bad arguments"),
                                       (1, None, "compress_best_dev: bad arguments")],
    "rans4x8_hip_compress_best_dev": [(2, [0, 1], None), (3, [0, 1, 0], "rans4x8 compress_best_dev: k must be 1 or 2"),
                                      (0, [0], "rans4x8 compress_best_dev: k must be 1 or 2"),
                                      (1, None, "rans4x8 compress_best_dev: k must be 1 or 2"),
                                      (2, [0, 2], "rans4x8 compress_best_dev: a method must be 0 or 1")],
    "rans4x16_hip_compress_best_packed_dev": [(2, [0, 1], None), (2, [0, STRIPES_256], "compress_best_packed_dev: more than 255 stripes"),
                                              (0, [0], "compress_best_packed_dev: bad arguments"),
                                              (33, [0] * 33, "compress_best_packed_dev: bad arguments"),
                                              (1, None, "compress_best_packed_dev: bad arguments")],
    "rans4x8_hip_compress_best_packed_dev": [(2, [0, 1], None), (3, [0, 1, 0], "rans4x8 compress_best_packed_dev: k must be 1 or 2"),
                                             (1, None, "rans4x8 compress_best_packed_dev: k must be 1 or 2"),
                                             (1, [-1], "rans4x8 compress_best_packed_dev: a method must be 0 or 1")],
    "rans4x16_hip_arith_compress_best_packed_dev": [(2, [0, 1], None), (1, [STRIPES_256], "arith_compress_best_packed_dev: more than 255 stripes"),
                                                    (0, [0], "arith_compress_best_packed_dev: bad arguments"),
                                                    (33, [0] * 33, "arith_compress_best_packed_dev: bad arguments"),
                                                    (1, None, "arith_compress_best_packed_dev: bad arguments")],
}
DECODES = {"rans4x16_hip_uncompress_dev_sized": 16, "rans4x16_hip_uncompress_packed_dev": 16,
           "rans4x8_hip_uncompress_dev": 8, "rans4x8_hip_uncompress_packed_dev": 8}
RAW = bytes((7 * i * i + i // 5) % 23 for i in range(64))


@pytest.fixture(scope="module")
def dc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    return htscodecs_amd.DeviceCodec(0)


@pytest.fixture(scope="module")
def streams(dc):
    """RAW as a rANS 4x16 and a rANS 4x8 stream (order 1), made by the slot calls of DeviceCodec."""
    out = {}
    for bits, call in ((16, dc.compress), (8, dc.compress_4x8)):
        a = _Arrays(dc, RAW)
        call(a.d_in, a.in_off, a.in_size, a.d_out, a.off1, a.cap, a.osz, a.st, 1, 64)
        dc.torch.cuda.synchronize()
        assert a.st.item() == 0
        out[bits] = a.d_out[:a.osz.item()].cpu().numpy().tobytes()
    return out


class _Arrays:
    """One block in device arrays; every output array preset, so that a write is seen."""

    def __init__(self, dc, data):
        t = dc.torch
        dev = dc.dev
        self.t = t
        self.d_in = t.zeros(4096, dtype=t.uint8, device=dev)
        self.d_in[:len(data)] = t.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
        self.in_off = t.zeros(1, dtype=t.int64, device=dev)
        self.in_size = t.full((1,), len(data), dtype=t.int32, device=dev)
        self.d_out = t.full((OUT,), 0xee, dtype=t.uint8, device=dev)
        self.off1 = t.zeros(1, dtype=t.int64, device=dev)                          # the slot form's d_out_off
        self.off2 = t.full((2,), PRESET, dtype=t.int64, device=dev)                 # the packed form's
        self.cap = t.full((1,), OUT, dtype=t.int32, device=dev)
        self.osz = t.full((1,), PRESET, dtype=t.int32, device=dev)
        self.st = t.full((1,), PRESET, dtype=t.int32, device=dev)
        t.cuda.synchronize()

    def untouched(self, off0=PRESET):
        self.t.cuda.synchronize()
        return (bool((self.d_out == 0xee).all()) and self.off2.tolist() == [off0, PRESET] and self.off1.item() == 0
                and self.osz.item() == PRESET and self.st.item() == PRESET)


def _call(dc, name, a, n=1, null=None, k=2, methods=(0, 1)):
    """The call `name` over the arrays `a`, the argument called `null` passed as a null pointer.  Returns (rc, the text)."""
    L, h = dc.L, dc.ctx.h
    packed = name in PACKED
    tail = (PACKED if packed else SLOT)[name][1]
    meth = None if methods is None else (C.c_int * len(methods))(*methods)
    tail = [k if v == "k" else meth if v == "methods" else v for v in tail]
    p = {"d_in": a.d_in, "d_in_off": a.in_off, "d_in_size": a.in_size, "d_out": a.d_out, "d_out_off": a.off2 if packed else a.off1,
         "d_out_cap": a.cap, "d_out_size": a.osz, "d_status": a.st}
    ptr = lambda key: None if key == null else p[key].data_ptr()
    if packed:
        args = [ptr("d_in"), ptr("d_in_off"), ptr("d_in_size"), ptr("d_out"), OUT, ptr("d_out_off"), ptr("d_out_size"), ptr("d_status")]
    else:
        args = [ptr(key) for key in ("d_in", "d_in_off", "d_in_size", "d_out", "d_out_off", "d_out_cap", "d_out_size", "d_status")]
    rc = getattr(L, name)(h, n, *args, *tail, dc._stream())
    return rc, dc.ctx.error()


def _mark(dc):
    """Leaves MARK in the context's error text: what a call that refuses nothing must not change."""
    assert dc.L.rans4x16_hip_peek_dev(dc.ctx.h, -1, None, None, None, None, None, None, 0, None) == -1
    assert dc.ctx.error() == MARK


def _input(name, streams):
    return streams[DECODES[name]] if name in DECODES else RAW


SLOT_POINTERS = ("d_in", "d_in_off", "d_in_size", "d_out", "d_out_off", "d_out_cap", "d_out_size", "d_status")
PACKED_POINTERS = ("d_in", "d_in_off", "d_in_size", "d_out", "d_out_off", "d_out_size", "d_status")     # (d_out: the capacity is not 0)


@pytest.mark.parametrize("name", list(SLOT) + list(PACKED))
def test_a_null_pointer_or_a_negative_count_is_refused(dc, streams, name):
    bad = (PACKED if name in PACKED else SLOT)[name][0]
    a = _Arrays(dc, _input(name, streams))
    for null in (PACKED_POINTERS if name in PACKED else SLOT_POINTERS):
        _mark(dc)
        assert _call(dc, name, a, 1, null=null) == (-1, bad), null
    _mark(dc)
    assert _call(dc, name, a, -1) == (-1, bad)
    assert a.untouched()


@pytest.mark.parametrize("name", list(SLOT) + list(PACKED))
def test_an_empty_batch_returns_zero_and_writes_the_first_offset_alone(dc, streams, name):
    a = _Arrays(dc, _input(name, streams))
    _mark(dc)
    assert _call(dc, name, a, 0) == (0, MARK)
    assert a.untouched(off0=0 if name in PACKED else PRESET)
    # the pointers of the blocks are not looked at; the packed form still needs its offsets
    for null in ("d_in", "d_out_size", "d_status"):
        assert _call(dc, name, a, 0, null=null) == (0, MARK)
    if name in PACKED:
        bad = PACKED[name][0]
        assert _call(dc, name, a, 0, null="d_out_off") == (-1, bad)
    else:
        assert _call(dc, name, a, 0, null="d_out_off") == (0, MARK)


@pytest.mark.parametrize("name", list(TABLES))
def test_a_method_table_is_refused_with_and_without_blocks(dc, name):
    bad = (PACKED if name in PACKED else SLOT)[name][0]
    a = _Arrays(dc, RAW)
    for k, methods, text in TABLES[name][1:]:
        for n in (0, 1):
            _mark(dc)
            assert _call(dc, name, a, n, k=k, methods=methods) == (-1, text), (k, methods, n)
        # a null pointer beside it: the pointers are tested first
        _mark(dc)
        assert _call(dc, name, a, 1, null="d_in_size", k=k, methods=methods) == (-1, bad), (k, methods)
        if name in PACKED:
            _mark(dc)
            assert _call(dc, name, a, 0, null="d_out_off", k=k, methods=methods) == (-1, bad), (k, methods)
    assert a.untouched()                      # (the refused empty batches did not zero the first offset either)


@pytest.mark.parametrize("name", list(SLOT) + list(PACKED))
def test_one_block_of_64_bytes_runs(dc, streams, name):
    data = _input(name, streams)
    a = _Arrays(dc, data)
    _mark(dc)
    assert _call(dc, name, a, 1) == (0, MARK)
    dc.torch.cuda.synchronize()
    assert a.st.item() == 0
    size = a.osz.item()
    got = a.d_out[:size].cpu().numpy().tobytes()
    if name in PACKED:
        assert a.off2.tolist() == [0, size]
    if name in DECODES:
        assert got == RAW
    elif "best" not in name:
        assert got == streams[8 if "4x8" in name else 16]
    elif "arith" not in name:
        assert got in (streams[8 if "4x8" in name else 16], _order0(dc, "4x8" in name))
    else:
        assert 0 < size < OUT
    if name in PACKED:
        assert bool((a.d_out[size:] == 0xee).all())


def _order0(dc, x8):
    a = _Arrays(dc, RAW)
    (dc.compress_4x8 if x8 else dc.compress)(a.d_in, a.in_off, a.in_size, a.d_out, a.off1, a.cap, a.osz, a.st, 0, 64)
    dc.torch.cuda.synchronize()
    return a.d_out[:a.osz.item()].cpu().numpy().tobytes()


# ---- the plain slot calls in chunks ------------------------------------------------------------------------------
NBLK, BLK = 40, 4096


def _blocks():
    rng = np.random.default_rng(20)
    return [(rng.integers(0, 12, BLK) + (i % 5) * (np.arange(BLK) % 3)).astype(np.uint8).tobytes() for i in range(NBLK)]


class _Batch:
    def __init__(self, dc, ins, cap):
        t, dev = dc.torch, dc.dev
        n = len(ins)
        self.dc, self.n, self.cap_each = dc, n, cap
        stride = (max(len(b) for b in ins) + 511) // 256 * 256
        arena = np.zeros(n * stride + 512, dtype=np.uint8)
        for i, b in enumerate(ins):
            arena[i * stride:i * stride + len(b)] = np.frombuffer(b, dtype=np.uint8)
        self.max_in = max(len(b) for b in ins)
        self.d_in = t.from_numpy(arena).to(dev)
        self.in_off = t.from_numpy(np.arange(n, dtype=np.int64) * stride).to(dev)
        self.in_size = t.from_numpy(np.array([len(b) for b in ins], dtype=np.int32)).to(dev)
        self.out_stride = (cap + 511) // 256 * 256
        self.out_off = t.from_numpy(np.arange(n, dtype=np.int64) * self.out_stride).to(dev)
        self.cap = t.full((n,), cap, dtype=t.int32, device=dev)

    def run(self, dc, which):
        t, dev = dc.torch, dc.dev
        d_out = t.full((self.n * self.out_stride + 512,), 0xee, dtype=t.uint8, device=dev)
        osz = t.full((self.n,), -3, dtype=t.int32, device=dev)
        st = t.full((self.n,), -3, dtype=t.int32, device=dev)
        head = (self.d_in, self.in_off, self.in_size, d_out, self.out_off, self.cap, osz, st)
        if which == "compress":
            dc.compress(*head, 1, self.max_in)
        elif which == "compress_4x8":
            dc.compress_4x8(*head, 1, self.max_in)
        elif which == "uncompress":
            dc.uncompress(*head, self.max_in, self.cap_each)
        else:
            dc.uncompress_4x8(*head)
        t.cuda.synchronize()
        return d_out.cpu().numpy(), osz.tolist(), st.tolist()


def _bound(dc, which):
    return dc.L.rans4x8_hip_compress_bound(BLK) if which.endswith("4x8") else dc.L.rans_compress_bound_4x16(BLK, 1)


@pytest.fixture(scope="module")
def chunk_inputs(dc):
    """The 40 blocks, and their streams of either codec under the default ceiling: what the decode calls read."""
    raw = _blocks()
    ins = {"compress": raw, "compress_4x8": raw}
    for which, dec in (("compress", "uncompress"), ("compress_4x8", "uncompress_4x8")):
        b = _Batch(dc, raw, _bound(dc, which))
        out, osz, st = b.run(dc, which)
        assert st == [0] * NBLK
        ins[dec] = [out[i * b.out_stride:i * b.out_stride + osz[i]].tobytes() for i in range(NBLK)]
    return ins


@pytest.mark.parametrize("which", ["compress", "uncompress", "compress_4x8", "uncompress_4x8"])
def test_a_slot_call_in_three_chunks_gives_what_one_chunk_gives(dc, chunk_inputs, which):
    """The workspace is linear in the blocks of a chunk but for roundings to 256 bytes: two small calls on a fresh context
    give its slope and its fixed part (rans4x16_hip_workspace_bytes is the workspace as the last growth left it).  A
    ceiling that holds 14 to 19 blocks cuts 40 blocks into 14, 14 and 12 (equal chunks: 3 rounds, 14 a round); the option
    counts in MiB, the nearest to 16.5 blocks is taken.
    The rANS 4x16 calls count a chain launch per chunk under the launch route; rANS 4x8 has no such count, its chunk is
    read off the workspace the call grew."""
    import htscodecs_amd as H
    ins = chunk_inputs[which]
    cap = _bound(dc, which) if which.startswith("compress") else BLK
    whole = _Batch(dc, ins, cap).run(dc, which)
    assert whole[2] == [0] * NBLK
    if which.startswith("uncompress"):
        raw = _blocks()
        stride = (cap + 511) // 256 * 256
        assert all(whole[0][i * stride:i * stride + BLK].tobytes() == raw[i] for i in range(NBLK))

    small = H.DeviceCodec(0)                                          # (fresh: its workspace starts at nothing)
    _Batch(small, ins[:1], cap).run(small, which)
    w1 = small.workspace_bytes()
    _Batch(small, ins[:2], cap).run(small, which)
    per = small.workspace_bytes() - w1
    fixed = w1 - per
    assert per > 0 and fixed >= 0, (w1, per)
    ceiling_mb = int(round((fixed + 16.5 * per) / 2 ** 20))
    fits = ((ceiling_mb << 20) - fixed - 4096) // per
    assert 14 <= fits <= 19, (w1, per, ceiling_mb, fits)

    small = H.DeviceCodec(0)
    small.set_option("max_workspace_mb", ceiling_mb)
    small.set_option("route_count", 1)
    small.route_read("launch")
    got = _Batch(small, ins, cap).run(small, which)
    launches = sum(small.route_read("launch").values())
    chunk = round((small.workspace_bytes() - fixed) / per)
    print(which, "workspace of one block", w1, "per block", per, "ceiling MiB", ceiling_mb, "chunk", chunk, "launches", launches)
    assert chunk == 14, (small.workspace_bytes(), fixed, per)        # 14 + 14 + 12
    if not which.endswith("4x8"):
        assert launches == 3
    assert got[1] == whole[1] and got[2] == whole[2]
    assert np.array_equal(got[0], whole[0])
