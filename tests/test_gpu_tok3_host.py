"""tok3 names with host buffers (include/rans4x16_hip.h part 2f): rans4x16_hip_tok3_encode_names_batch,
rans4x16_hip_tok3_decode_names_batch and the two single-block functions behind include/tok3_names_hip.h.

Expected bytes come from the CPU side alone: the tokeniser model (tok3_enc_model.tokenise), the framing model over the
oracle's compress (tok3_model.frame), the names model (tok3_names_model.decode) and the committed fixtures - never from
another GPU path.  The models' results are computed once per module and not changed."""
import ctypes as C

import numpy as np
import pytest

import tok3_enc_model as E
import tok3_model as M
import tok3_names_model as N
from test_gpu_confinement import pattern
from test_tok3_cpu import _descriptor_bytes

pytestmark = pytest.mark.gpu

# what the host calls clamp their measured limits to (part 2f): the device calls' hard limits
HARD = dict(max_in_size=16776960, max_names=(1 << 24) - 1, max_name_len=16384, max_tokens=128, max_columns=2048)
LEVELS = (1, 3, 5, 7, 9)


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
    yield ctx
    assert ctx.L.rans4x16_hip_set_names_chunk_blocks(ctx.h, 0) == 0


@pytest.fixture(scope="module")
def files():
    """[(key, block)]: the reference's 11 names files, in name order."""
    return sorted(N.names_files().items())


@pytest.fixture(scope="module")
def toks(files):
    """Per file the tokeniser model's (status, [(id, bytes)], last_start, nreads)."""
    out = [E.tokenise(b, **HARD) for _, b in files]
    assert [t[0] for t in out] == [0] * 11
    return out


_frames = {}


def _framed(oracle, toks, level):
    """The model's 11 containers of a level, made once."""
    if level not in _frames:
        _frames[level] = [M.frame(oracle.compress, cols, M.LISTS[level], ls, nr)[0] for _, cols, ls, nr in toks]
    return _frames[level]


def _nul(block, last_start):
    return bytes(0 if ch <= 10 else ch for ch in block[:last_start])


class _Res:
    pass


def _call(ctx, blocks, encode, methods=None, place=None, in_ptrs=None):
    """One batch call through ctypes.  place: None - every out[i] NULL, the library allocates -, or (arena, offsets,
    capacities): out[i] inside the caller's numpy array.  in_ptrs: addresses of the blocks where the test laid them out itself."""
    L = ctx.L
    n = len(blocks)
    srcs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in blocks]
    dummy = np.zeros(1, dtype=np.uint8)
    if in_ptrs is None:
        in_ptrs = [(s.ctypes.data if len(s) else dummy.ctypes.data) for s in srcs]
    in_p = (C.c_void_p * n)(*in_ptrs)
    in_sz = (C.c_uint * n)(*[len(b) for b in blocks])
    out_p = (C.c_void_p * n)()
    out_sz = (C.c_uint * n)()
    if place is not None:
        arena, offs, caps = place
        for i in range(n):
            out_p[i] = arena.ctypes.data + offs[i]
            out_sz[i] = caps[i]
    a, b = (C.c_uint * n)(*([0xDEAD] * n)), (C.c_uint * n)(*([0xDEAD] * n))
    status = (C.c_int * n)(*([-5] * n))
    if encode:
        meth = (C.c_int * len(methods))(*methods)
        rc = L.rans4x16_hip_tok3_encode_names_batch(ctx.h, n, in_p, in_sz, out_p, out_sz, len(methods), meth, a, b, status)
    else:
        rc = L.rans4x16_hip_tok3_decode_names_batch(ctx.h, n, in_p, in_sz, out_p, out_sz, a, status)
    assert rc >= 0, ctx.error()
    r = _Res()
    r.rc, r.status, r.size, r.a, r.b = rc, list(status), list(out_sz), list(a), list(b)
    r.null = [not out_p[i] for i in range(n)]
    r.data = []
    from htscodecs_amd import codec
    for i in range(n):
        if place is None:
            r.data.append(C.string_at(out_p[i], out_sz[i]) if out_p[i] else None)
            if out_p[i]:
                codec._free(out_p[i])
        else:
            r.data.append(place[0][place[1][i]:place[1][i] + out_sz[i]].tobytes())
    assert rc == sum(1 for s in r.status if s != 0)
    assert all(sz == 0 for sz, s in zip(r.size, r.status) if s != 0)
    return r


# ---- 1. encode, the reference's files ----------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_encode_batch_writes_the_reference_containers(H, oracle, files, toks, level):
    fx = dict(M.fixtures())
    r = _call(H, [b for _, b in files], True, methods=M.LISTS[level])
    assert r.status == [0] * 11 and r.rc == 0
    want = _framed(oracle, toks, level)
    same = 0
    for i, (key, _) in enumerate(files):
        name = "%s.names.%d" % (key, level)
        assert r.data[i] == want[i], name
        if name not in M.EXCEPTIONS:
            assert r.data[i] == fx[name], name
            same += 1
        head = fx[name][:8]
        assert (r.a[i], r.b[i]) == (int.from_bytes(head[:4], "little"), int.from_bytes(head[4:], "little")), name
        assert (r.a[i], r.b[i]) == (toks[i][2], toks[i][3]), name
    assert same == (11 if level in (1, 7, 9) else 9)


# ---- 2. decode ----------------------------------------------------------------------------------------------------
def test_decode_batch_of_all_fixtures_gives_the_names_files(H, files):
    by = dict(files)
    fx = M.fixtures()
    assert len(fx) == 55
    r = _call(H, [buf for _, buf in fx], False)
    assert r.status == [0] * 55
    for i, (name, buf) in enumerate(fx):
        assert r.data[i] == by[name.split(".")[0]].replace(b"\n", b"\0"), name
        assert r.a[i] == int.from_bytes(buf[4:8], "little"), name


# ---- 3. refused blocks between good ones ---------------------------------------------------------------------------
def test_refused_blocks_leave_their_neighbours_alone(H, oracle):
    built = E.constructed()
    blocks = [b for _, b, _ in built]
    model = [E.tokenise(b, **HARD) for b in blocks]
    want_st = [m[0] for m in model]
    assert {0, E.SIZE, E.UNSUPPORTED} == set(want_st)
    r = _call(H, blocks, True, methods=M.LISTS[7])
    assert r.status == want_st
    empty = [i for i, b in enumerate(blocks) if len(b) == 0]
    assert empty and all(r.status[i] == E.SIZE for i in empty)
    good = []
    for i, (st, cols, ls, nr) in enumerate(model):
        what = built[i][0]
        if st != 0:
            assert r.null[i] and r.size[i] == 0, what                 # a NULL out[i] of a refused block stays NULL
            continue
        assert r.data[i] == M.frame(oracle.compress, cols, M.LISTS[7], ls, nr)[0], what
        assert (r.a[i], r.b[i]) == (ls, nr), what
        good.append(i)
    assert len(good) >= 40
    d = _call(H, [r.data[i] for i in good], False)
    assert d.status == [0] * len(good)
    for j, i in enumerate(good):
        assert d.data[j] == _nul(blocks[i], model[i][2]), built[i][0]
        assert d.a[j] == model[i][3], built[i][0]


# ---- 4. caller buffers ---------------------------------------------------------------------------------------------
def _placed(sizes, gap):
    offs, at = [], 5
    for s in sizes:
        offs.append(at)
        at += s + gap
    return offs, at + 64


@pytest.mark.parametrize("encode", [True, False])
def test_caller_buffers_exact_one_byte_short_and_nothing_outside(H, oracle, files, toks, encode):
    frames = _framed(oracle, toks, 3)
    pick = [0, 3, 5, 8]
    if encode:
        blocks, want = [files[i][1] for i in pick], [frames[i] for i in pick]
    else:
        blocks, want = [frames[i] for i in pick], [_nul(files[i][1], toks[i][2]) for i in pick]
    sizes = [len(w) for w in want]
    offs, total = _placed(sizes, 3)
    pat = pattern(total)

    def run(caps):
        arena = pat.copy()
        r = _call(H, blocks, encode, methods=M.LISTS[3], place=(arena, offs, caps))
        mask = np.zeros(total, dtype=bool)
        for o, sz in zip(offs, r.size):
            mask[o:o + sz] = True
        assert np.array_equal(arena[~mask], pat[~mask]), "a byte outside the written ranges changed"
        return r

    r = run(sizes)
    assert r.status == [0] * 4 and r.size == sizes and r.data == want
    caps = list(sizes)
    caps[1] -= 1
    r = run(caps)
    assert r.status == [0, M.CAPACITY, 0, 0] and r.size == [sizes[0], 0, sizes[2], sizes[3]]
    assert [r.data[i] for i in (0, 2, 3)] == [want[i] for i in (0, 2, 3)]
    assert not any(r.null)


# ---- 5. chunks -----------------------------------------------------------------------------------------------------
def test_chunks_of_four_and_of_one_give_the_same_bytes(H, oracle, files, toks):
    L = H.L
    frames = _framed(oracle, toks, 9)
    names = [_nul(b, t[2]) for (_, b), t in zip(files, toks)]
    try:
        assert L.rans4x16_hip_set_names_chunk_blocks(H.h, 4) == 0
        H.route_read("names")
        r = _call(H, [b for _, b in files], True, methods=M.LISTS[9])
        assert r.status == [0] * 11 and r.data == frames
        route = H.route_read("names")
        assert route == {"enc_chunks": 3, "dec_chunks": 0, "uploaded": 11, "refused": 0}
        d = _call(H, frames, False)
        assert d.status == [0] * 11 and d.data == names
        assert H.route_read("names") == {"enc_chunks": 0, "dec_chunks": 3, "uploaded": 11, "refused": 0}
        # three blocks, one per chunk, at addresses 1, 2 and 3 bytes behind an aligned one
        assert L.rans4x16_hip_set_names_chunk_blocks(H.h, 1) == 0
        pick = [1, 4, 9]
        for encode in (True, False):
            blocks = [files[i][1] if encode else frames[i] for i in pick]
            room = [(len(b) + 64 + 63) // 64 * 64 for b in blocks]
            host = np.zeros(sum(room) + 128, dtype=np.uint8)
            base = (-host.ctypes.data) % 64
            ptrs, at = [], base
            for k, b in enumerate(blocks):
                host[at + k + 1:at + k + 1 + len(b)] = np.frombuffer(b, dtype=np.uint8)
                ptrs.append(host.ctypes.data + at + k + 1)
                at += room[k]
            assert [p % 64 for p in ptrs] == [1, 2, 3]
            before = host.copy()
            r = _call(H, blocks, encode, methods=M.LISTS[9], in_ptrs=ptrs)
            assert r.status == [0] * 3
            assert r.data == [frames[i] if encode else names[i] for i in pick]
            assert np.array_equal(host, before)                        # the input is never written
            route = H.route_read("names")
            assert route["enc_chunks" if encode else "dec_chunks"] == 3 and route["uploaded"] == 3
        assert L.rans4x16_hip_set_names_chunk_blocks(H.h, -1) == -1
    finally:
        assert L.rans4x16_hip_set_names_chunk_blocks(H.h, 0) == 0


# ---- 6. the single-block functions ---------------------------------------------------------------------------------
def test_single_block_functions(H, oracle, files, toks):
    from htscodecs_amd import codec
    L = H.L
    i = 2
    block = files[i][1]
    want = _framed(oracle, toks, 7)[i]
    batch = _call(H, [block], True, methods=codec.tok3_level_methods(7))
    assert codec.tok3_level_methods(7) == M.LISTS[7] and batch.data == [want]

    def encode(data, use_arith=0, with_last_start=True):
        buf = C.create_string_buffer(data, len(data))
        out_len, ls = C.c_int(-1), C.c_int(-1)
        p = L.rans4x16_hip_tok3_encode_names(buf, len(data), 7, use_arith, C.byref(out_len), C.byref(ls) if with_last_start else None)
        got = None
        if p:
            got = C.string_at(p, out_len.value)
            codec._free(p)
        return got, ls.value, buf.raw

    got, ls, after = encode(block)
    assert got == want and ls == len(block) == toks[i][2]
    assert after == _nul(block, ls)                                     # NULs for the separators in front of last_start
    tail = b"partial"
    got, ls, after = encode(block + tail)
    assert got == want and ls == len(block)
    assert after == _nul(block, ls) + tail                              # the bytes from last_start on are left alone
    got, ls, _ = encode(block, with_last_start=False)
    assert got == want and ls == -1
    got, _, after = encode(block, use_arith=1)
    assert got is None and after == block
    # decode_names
    fx = dict(M.fixtures())["%s.names.7" % files[i][0]]
    assert codec.decode_names(fx) == block.replace(b"\n", b"\0")
    arith = bytearray(fx)
    arith[8] = 1
    assert codec.decode_names(bytes(arith)) is None
    d = _call(H, [bytes(arith)], False)
    assert d.status == [M.UNSUPPORTED] and d.null == [True]
    assert codec.encode_names(block, 7) == (want, len(block))


# ---- 7. damaged containers ---------------------------------------------------------------------------------------
def test_damaged_containers_in_one_decode_batch(H, oracle):
    """Malformed data is rejected, as in the hostile-input modules: 200 variants of the two smallest fixtures, every
    header and descriptor byte edited in turn (the generator of tests/test_tok3_cpu.py)."""
    from htscodecs_amd import codec
    small = sorted(M.fixtures(), key=lambda f: len(f[1]))[:2]
    variants = []
    for name, buf in small:
        edits = [(p, x) for p in _descriptor_bytes(buf) for x in (0x01, 0x40, 0x80, 0xFF)]
        step = max(len(edits) // 100, 1)
        for p, x in edits[::step][:100]:
            b = bytearray(buf)
            b[p] ^= x
            variants.append(bytes(b))
    assert len(variants) == 200
    scans = [codec.tok3_scan(v)[0] for v in variants]
    assert 0 in scans and len(set(scans)) >= 3
    r = _call(H, variants, False)
    accepted = 0
    for i, v in enumerate(variants):
        if scans[i] != 0:
            assert r.status[i] == scans[i], i                          # the scan's status, unchanged
            assert r.null[i]
            continue
        if r.status[i] != 0:
            continue
        w = M.walk(v)
        assert w.status == 0, i
        data = M.columns(v, w, lambda stream, size: oracle.uncompress(stream, capacity=size, out_size_hint=size))
        assert data is not None, i
        cols = [(c["id"], d) for c, d in zip(w.cols, data)]
        st, names, starts = N.decode(cols, w.last_start, w.nreads)
        assert st == 0 and r.data[i] == names and r.a[i] == len(starts), i
        accepted += 1
    assert accepted >= 5, accepted


# ---- 8. the stripe setting ---------------------------------------------------------------------------------------
def test_a_host_names_decode_leaves_the_stripe_setting_alone(oracle, files):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    from htscodecs_amd import codec
    dc = htscodecs_amd.DeviceCodec(0)
    plain = bytes(range(256)) * 16
    comp = oracle.compress(plain, 0x08)
    assert comp[0] & 0x08

    def stripe_decode():
        dev = dc.dev
        d_in = torch.from_numpy(np.frombuffer(comp + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
        d_out = torch.zeros(len(plain) + 64, dtype=torch.uint8, device=dev)
        i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)
        i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
        size, status = i32(-1), i32(-1)
        dc.uncompress(d_in, i64(0), i32(len(comp)), d_out, i64(0), i32(len(plain)), size, status, len(comp), len(plain))
        torch.cuda.synchronize()
        return int(status.item())

    assert stripe_decode() == M.UNSUPPORTED
    fx = [(n, b) for n, b in M.fixtures() if n.endswith(".9")]
    names, st = codec.tok3_decode_names_batch([b for _, b in fx], ctx=dc.ctx)
    assert st == [0] * 11
    assert names == [dict(files)[n.split(".")[0]].replace(b"\n", b"\0") for n, _ in fx]
    assert stripe_decode() == M.UNSUPPORTED


# ---- the command-line tool ---------------------------------------------------------------------------------------
def test_the_names_tool_round_trips_a_file_in_blocks_and_raw(H, oracle, files, toks, tmp_path):
    """tools/tok3_hip: 1 MiB blocks behind their 4-byte sizes in one batch call, -r one naked block, levels from 11 refused."""
    import os
    import subprocess
    tool = os.path.join(M.ROOT, "tools", "tok3_hip")
    assert os.path.exists(tool), "tools/tok3_hip is built by build()"
    key, block = files[2]
    big = block * (2 * (1 << 20) // len(block) + 1)                      # more than two blocks of 1 MiB
    src, packed, back = tmp_path / "names", tmp_path / "packed", tmp_path / "back"
    src.write_bytes(big)
    run = lambda *a: subprocess.run([tool] + [str(x) for x in a], capture_output=True, text=True, timeout=120)
    r = run("-7", src, packed)
    assert r.returncode == 0, r.stderr
    data = packed.read_bytes()
    sizes, at = [], 0
    while at < len(data):
        n = int.from_bytes(data[at:at + 4], "little")
        sizes.append(n)
        at += 4 + n
    assert at == len(data) and len(sizes) == 3
    r = run("-d", packed, back)
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == big
    src.write_bytes(block)
    r = run("-7", "-r", src, packed)
    assert r.returncode == 0, r.stderr
    assert packed.read_bytes() == _framed(oracle, toks, 7)[2]
    r = run("-d", "-r", packed, back)
    assert r.returncode == 0 and back.read_bytes() == block, r.stderr
    r = run("-11", src, packed)
    assert r.returncode == 1 and "arithmetic" in r.stderr


def test_a_block_above_the_size_limit_is_refused_before_upload(H, oracle, files, toks):
    """max_in_size is 16,776,960: one byte more is not uploaded, reports UNSUPPORTED (the model's verdict under that limit)
    and leaves the blocks on either side alone."""
    big = b"r1\n" * (HARD["max_in_size"] // 3 + 1)
    assert len(big) > HARD["max_in_size"] and E.tokenise(big, **HARD)[0] == E.UNSUPPORTED
    frames = _framed(oracle, toks, 1)
    H.route_read("names")
    r = _call(H, [files[0][1], big, files[1][1]], True, methods=M.LISTS[1])
    assert r.status == [0, E.UNSUPPORTED, 0] and r.null == [False, True, False]
    assert [r.data[0], r.data[2]] == frames[:2]
    assert H.route_read("names") == {"enc_chunks": 1, "dec_chunks": 0, "uploaded": 2, "refused": 1}
