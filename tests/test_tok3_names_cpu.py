"""tok3 name decoding (include/rans4x16_hip.h part 2d), the half that needs no GPU: the Python model of the decoder
(tok3_names_model.py) against the reference's own input files - the 55 containers of tests/golden/tok3 were made from
the files kept gzip-compressed in tests/golden/names, so their columns must decode to those files with every line end
a NUL - and the symbols."""
import ctypes as C
import os
import re

import pytest

import tok3_model as M
import tok3_names_model as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rans4x16_hip_tok3_names_dev", "rans4x16_hip_tok3_decode_names_dev")


def block_columns(buf, w, oracle):
    """[(id, bytes)] of a walked container, type columns included."""
    data = M.columns(buf, w, lambda stream, size: oracle.uncompress(stream, capacity=size, out_size_hint=size))
    assert data is not None
    return [(c["id"], d) for c, d in zip(w.cols, data)]


def test_model_decodes_the_55_fixtures_to_the_names_files(oracle):
    files = N.names_files()
    assert sorted(files) == ["01", "02", "03", "05", "08", "09", "10", "20", "nv", "nv2", "rr"]
    fx = M.fixtures()
    assert len(fx) == 55
    names = dups = far = zero = top = longest = 0
    for name, buf in fx:
        w = M.walk(buf)
        assert w.status == 0, name
        cols = block_columns(buf, w, oracle)
        st, out, starts = N.decode(cols, w.last_start, w.nreads)
        want = files[name.split(".")[0]].replace(b"\n", b"\0")
        assert st == 0 and out == want, name
        assert w.last_start == len(out) and w.nreads == len(starts) == 1000, name
        assert starts == [0] + [i + 1 for i, ch in enumerate(want[:-1]) if ch == 0], name
        by = dict(cols)
        names += len(starts)
        dups += by[0].count(N.N_DUP)
        dist = [int.from_bytes(by[k][i:i + 4], "little") for k in (N.N_DUP, N.N_DIFF) if k in by for i in range(0, len(by[k]), 4)]
        far += sum(d >= 2 for d in dist)
        zero += sum(d == 0 for d in dist)
        top = max(top, max(cid >> 4 for cid, _ in cols))
        longest = max(longest, max(b - a for a, b in zip(starts, starts[1:] + [len(out)])) - 1)
    assert (names, dups, far, zero, top, longest) == (55000, 8035, 12275, 855, 31, 88)


def test_digits_of_zero_write_no_byte():
    assert N.uint32_var(0) == b"" and N.uint32_var(7) == b"7" and N.uint32_var(4294967295) == b"4294967295"
    cols = [(0x00, bytes([N.N_DIFF])), (0x06, bytes(4)), (0x10, bytes([N.N_CHAR])), (0x12, b"x"),
            (0x20, bytes([N.N_DIGITS])), (0x27, bytes(4)), (0x30, bytes([N.N_END]))]
    assert N.decode(cols, 2, 1) == (0, b"x\0", [0])
    assert N.decode(cols, 3, 1)[0] == N.SIZE                      # the size is last_start, exactly


def test_fixed_width_rules():
    assert N.uint32_fixed(5, 0) == b"" and N.uint32_fixed(42, 5) == b"00042" and N.uint32_fixed(123456789, 9) == b"123456789"
    assert N.uint32_fixed(1234, 2) == bytes([(123 + 48) & 0xFF]) + b"4"                   # kept from the reference
    assert N.uint32_fixed(4294967295, 1) == bytes([(4294967295 + 48) & 0xFF])

    def block(vl):
        return [(0x00, bytes([N.N_DIFF])), (0x06, bytes(4)), (0x10, bytes([N.N_DIGITS0])), (0x13, (77).to_bytes(4, "little")),
                (0x14, bytes([vl])), (0x20, bytes([N.N_END]))]
    assert N.decode(block(9), 10, 1) == (0, b"000000077\0", [0])
    assert N.decode(block(0), 1, 1) == (0, b"\0", [0])
    assert N.decode(block(10), 11, 1)[0] == N.SIZE                # stricter than the reference


def test_names_symbols_are_declared_exported_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    for meth in ("tok3_names", "tok3_decode_names"):
        assert hasattr(codec.DeviceCodec, meth), meth


def test_names_calls_refuse_a_null_context():
    import htscodecs_amd
    L = htscodecs_amd.load()
    off = (C.c_uint64 * 1)()
    assert L.rans4x16_hip_tok3_names_dev(None, 0, None, 0, None, None, None, None, None, None, None, None, 0, off, None, None,
                                         None, None, 64, 1000, 128, None) == -1
    assert L.rans4x16_hip_tok3_decode_names_dev(None, 0, None, None, None, None, 0, off, None, None, None, None,
                                                64, 0, 0, 1000, 128, 0, None) == -1
