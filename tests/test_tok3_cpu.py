"""tok3 column containers (include/rans4x16_hip.h part 2c), the half that needs no GPU: the symbols, and
rans4x16_hip_tok3_scan against the Python model of the walk (tok3_model.py) on the 55 reference-made containers of
tests/golden/tok3 and on about 2,500 damaged variants of them.  The scan runs the text the device walk runs
(htscodecs_amd/csrc/r4x16_tok3_walk.h), so what is pinned here is pinned for rans4x16_hip_tok3_unpack_dev's walk too."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tok3_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rans4x16_hip_tok3_scan", "rans4x16_hip_tok3_pack_dev", "rans4x16_hip_tok3_unpack_dev")


@pytest.fixture(scope="module")
def fx():
    f = M.fixtures()
    assert len(f) == 55 and sum(len(b) for _, b in f) > 250000
    return f


def _scan(buf, **kw):
    from htscodecs_amd import codec
    return codec.tok3_scan(buf, **kw)


def _same(buf, what, **kw):
    w = M.walk(buf, **{k: v for k, v in kw.items() if v})
    st, info = _scan(buf, **kw)
    assert st == w.status, (what, st, w.status)
    assert info == {"last_start": w.last_start, "nreads": w.nreads, "ndesc": w.ndesc, "ncol": w.ncol,
                    "total_col_size": w.total, "largest_col": w.largest_col, "largest_stream": w.largest_stream}, what
    return st


def test_tok3_symbols_are_declared_exported_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    assert callable(codec.tok3_scan)
    for meth in ("tok3_pack", "tok3_unpack"):
        assert hasattr(codec.DeviceCodec, meth), meth


def test_tok3_calls_refuse_a_null_context():
    import htscodecs_amd
    L = htscodecs_amd.load()
    meth = (C.c_int * 2)(0, 1)
    off = (C.c_uint64 * 1)()
    assert L.rans4x16_hip_tok3_pack_dev(None, 0, 0, None, None, None, None, None, None, None, None, 0, off, None, None,
                                        2, meth, None, 0, 0, None) == -1
    assert L.rans4x16_hip_tok3_unpack_dev(None, 0, None, None, None, None, 0, off, None, None, None, None, None, None, None,
                                          None, 64, 0, 0, None) == -1


def test_scan_refuses_bad_arguments():
    import htscodecs_amd
    L = htscodecs_amd.load()
    assert L.rans4x16_hip_tok3_scan(None, 9, 0, 0, None, None, None, None, None, None, None) == -1
    assert L.rans4x16_hip_tok3_scan(b"\0" * 9, 9, 2049, 0, None, None, None, None, None, None, None) == -1
    assert L.rans4x16_hip_tok3_scan(b"\0" * 9, 9, 0, 0, None, None, None, None, None, None, None) == 0      # a header alone


def test_scan_equals_the_model_on_the_fixtures(fx):
    ncols, streams, dups = [], 0, 0
    for name, buf in fx:
        assert _same(buf, name) == 0, name
        w = M.walk(buf)
        ncols.append(w.ncol)
        streams += sum(c["kind"] == M.PLAIN for c in w.cols)
        dups += sum(c["kind"] == M.DUP for c in w.cols)
        # the limits: exactly enough, and one short
        assert _same(buf, name, max_columns=w.ndesc, max_col_size=w.largest_col) == 0
        if w.ndesc > 1:
            assert _same(buf, name, max_columns=w.ndesc - 1) == M.UNSUPPORTED
        assert _same(buf, name, max_col_size=w.largest_col - 1) == M.UNSUPPORTED
    assert (streams + dups, dups) == (1415, 160), (streams, dups)
    assert max(M.walk(b).ndesc for _, b in fx) <= 60 and max(ncols) > 60       # (type columns come on top of the descriptors)


def _descriptor_bytes(buf):
    """Positions of the header bytes and of every descriptor byte (type, duplicate reference, clen varint) of a container."""
    w = M.walk(buf)
    assert w.status == 0
    pos = list(range(9))
    o = 9
    for c in w.cols:
        if c["kind"] == M.SYNTH:
            continue
        if c["kind"] == M.PLAIN:
            pos += list(range(o, c["stream_off"] + 2))            # type, clen, and the stream's flag byte and first size byte
            o = c["stream_off"] + c["clen"]
        else:
            pos += [o, o + 1, o + 2]
            o += 3
    assert o == len(buf)
    return pos


def test_scan_equals_the_model_on_damaged_containers(fx):
    by = dict(fx)
    seen = {}
    count = 0

    def check(buf, what):
        nonlocal count
        st = _same(bytes(buf), what)
        seen[st] = seen.get(st, 0) + 1
        count += 1

    # every header byte and every descriptor byte of three fixtures, edited in turn
    for name in ("01.names.9", "rr.names.7", "20.names.1"):
        buf = by[name]
        for p in _descriptor_bytes(buf):
            for x in (0x01, 0x40, 0x80, 0xFF):
                b = bytearray(buf)
                b[p] ^= x
                check(b, (name, p, x))
    # truncations at every length of the smallest fixture
    small = min((b for _, b in fx), key=len)
    for n in range(len(small)):
        check(small[:n], ("cut", n))
    # random damage
    rng = np.random.default_rng(20240607)
    for r in range(400):
        name, buf = fx[int(rng.integers(len(fx)))]
        b = bytearray(buf)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(len(b)))] = int(rng.integers(256))
        if r % 4 == 0:
            del b[int(rng.integers(9, len(b))):]
        check(b, ("random", r, name))
    assert count >= 2000, count
    # the damage reaches every status the walk can give, and leaves some containers walkable
    assert {M.OK, M.TRUNCATED, M.SIZE, M.UNSUPPORTED, M.EMPTY} <= set(seen), seen


def _container(*descs, last_start=5, nreads=3):
    return (last_start.to_bytes(4, "little") + nreads.to_bytes(4, "little") + b"\0" + b"".join(descs))


def _plain(t, stream):
    return bytes([t]) + M.var_put(len(stream)) + stream


# one edited container per rule of the walk (include/rans4x16_hip.h part 2c): (what, container, status)
# (the streams are X_CAT streams: a flag byte, the size, the bytes themselves)
WALK_CASES = [
    ("short header", b"\0" * 8, M.TRUNCATED),
    ("use_arith", b"\0" * 8 + b"\1", M.UNSUPPORTED),
    ("last_start negative", _container(last_start=0x80000000), M.SIZE),
    ("no position opened", _container(_plain(0x00, b"\x20\3abc")), M.SIZE),
    ("type column of no reads", _container(_plain(0x81, b"\x20\3abc"), nreads=0), M.SIZE),
    ("duplicate at the end", _container(_plain(0x80, b"\x20\3abc"), bytes([0x41, 0, 0])), M.TRUNCATED),
    ("duplicate of itself", _container(_plain(0x80, b"\x20\3abc"), bytes([0x41, 0, 1]), _plain(0x02, b"\x20\1a")), M.SIZE),
    ("duplicate of a later id", _container(_plain(0x80, b"\x20\3abc"), bytes([0x41, 0, 2]), _plain(0x03, b"\x20\1a")), M.SIZE),
    ("duplicate of a column that never was", _container(_plain(0x80, b"\x20\3abc"), bytes([0x43, 0, 2]), _plain(0x04, b"\x20\1a")), M.OK),
    ("ids do not ascend", _container(_plain(0x81, b"\x20\3abc"), _plain(0x01, b"\x20\3abc")), M.UNSUPPORTED),
    ("type column then type 0", _container(_plain(0x81, b"\x20\3abc"), _plain(0x00, b"\x20\3abc")), M.UNSUPPORTED),
    ("X_NOSZ stream", _container(_plain(0x80, b"\x10abcd")), M.SIZE),
    ("clen beyond the end", _container(bytes([0x80, 9]) + b"\x20\3abc"), M.TRUNCATED),
    ("clen without an end", _container(bytes([0x80, 0x81])), M.TRUNCATED),
    ("no clen", _container(bytes([0x80])), M.TRUNCATED),
    ("clen of zero", _container(bytes([0x80, 0]), _plain(0x01, b"\x20\1a")), M.EMPTY),
    ("size field runs out", _container(_plain(0x80, b"\x20\x83")), M.TRUNCATED),
    ("129 positions", _container(*[_plain(0x80, b"\x20\1a")] * 129), M.SIZE),
    ("128 positions", _container(*[_plain(0x80, b"\x20\1a")] * 128), M.OK),
]


@pytest.mark.parametrize("what,buf,status", WALK_CASES)
def test_every_walk_rule(what, buf, status):
    assert M.walk(buf).status == status, what
    assert _same(buf, what) == status


def test_limits_of_the_walk():
    buf = _container(_plain(0x81, b"\x20\3abc"), _plain(0x02, b"\x20\x20" + b"x" * 32), nreads=7)
    w = M.walk(buf)
    assert (w.status, w.ncol, w.ndesc, w.total, w.largest_col) == (0, 3, 2, 7 + 3 + 32, 32)
    assert _same(buf, "fits", max_columns=2, max_col_size=32) == 0
    assert _same(buf, "columns", max_columns=1, max_col_size=32) == M.UNSUPPORTED
    assert _same(buf, "claim", max_columns=2, max_col_size=31) == M.UNSUPPORTED
    assert _same(buf, "type column", max_columns=2, max_col_size=6) == M.UNSUPPORTED
