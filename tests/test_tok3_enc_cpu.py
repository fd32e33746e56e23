"""tok3 name encoding (include/rans4x16_hip.h part 2e), the half that needs no GPU: the Python model of the tokeniser
(tok3_enc_model.py) against the reference's own files - the names of tests/golden/names must tokenise to the columns of
the 55 containers of tests/golden/tok3 - and against the model of the decoder on blocks built for what those files lack;
the bound on a block's column bytes; and the symbols."""
import ctypes as C
import os
import re

import pytest

import tok3_enc_model as E
import tok3_model as M
import tok3_names_model as N
from test_tok3_names_cpu import block_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rans4x16_hip_tok3_tokenise_dev", "rans4x16_hip_tok3_encode_names_dev")


def test_model_tokenises_the_names_files_to_the_columns_of_the_55_fixtures(oracle):
    files = N.names_files()
    mine = {}
    for key, data in files.items():
        mine[key] = E.tokenise(data)
        st, cols, last_start, nreads = mine[key]
        assert st == 0 and last_start == len(data) and nreads == 1000, key
        assert all(len(d) for _, d in cols) and [c for c, _ in cols] == sorted({c for c, _ in cols}), key
        assert sum(len(d) for _, d in cols) <= E.bound(len(data)), key
    fx = M.fixtures()
    assert len(fx) == 55
    for name, buf in fx:
        w = M.walk(buf)
        assert w.status == 0, name
        want = [(c["id"], d) for c, (_, d) in zip(w.cols, block_columns(buf, w, oracle)) if c["kind"] != M.SYNTH]
        st, cols, last_start, nreads = mine[name.split(".")[0]]
        assert (last_start, nreads) == (w.last_start, w.nreads), name
        assert [c for c, _ in cols] == [c for c, _ in want], name
        assert cols == want, name


def test_constructed_blocks_decode_to_their_names():
    trace = {}
    whole = 0
    blocks = E.constructed()
    for what, block, want in blocks:
        st, cols, last_start, nreads = E.tokenise(block, trace=trace)
        assert st == want, what
        if st != 0:
            assert cols == [], what
            continue
        whole += 1
        assert sum(len(d) for _, d in cols) <= E.bound(len(block)), what
        assert all(len(d) for _, d in cols), what
        names = bytes(0 if ch <= 10 else ch for ch in block[:last_start])
        got = N.decode(E.with_type_columns(cols, nreads), last_start, nreads)
        assert got[0] == 0 and got[1] == names, what
        assert len(got[2]) == nreads, what
    assert whole >= 40
    # what the reference's files lack (no exact hit on a longer name, few distances of 0), and the rarer branches
    assert trace["exact_longer"] >= 3 and trace["dist0"] >= 20 and trace["goto_digits0"] >= 3 and trace["delta_refused"] >= 1


def test_the_bound_is_met_with_equality_and_limits_refuse():
    st, cols, last_start, nreads = E.tokenise(b"0\n")
    assert st == 0 and sum(len(d) for _, d in cols) == 10 <= E.bound(2)              # both one-byte type columns are dropped: 4 + 5 + 1
    st, cols, _, _ = E.tokenise(b"0\n" * 3)
    assert [c for c, _ in cols] == [0x00, 0x05, 0x06, 0x13, 0x14, 0x20] and sum(len(d) for _, d in cols) == 21
    block = b"ab1\nab2\nabc\n"
    assert E.tokenise(block)[0] == 0
    assert E.tokenise(block, max_names=2)[0] == E.UNSUPPORTED
    assert E.tokenise(block, max_name_len=2)[0] == E.UNSUPPORTED
    assert E.tokenise(block, max_in_size=len(block) - 1)[0] == E.UNSUPPORTED
    assert E.tokenise(block, max_tokens=4)[0] == 0 and E.tokenise(block, max_tokens=3)[0] == E.UNSUPPORTED
    ncol = len(E.tokenise(block)[1])
    assert E.tokenise(block, max_columns=ncol)[0] == 0 and E.tokenise(block, max_columns=ncol - 1)[0] == E.UNSUPPORTED


def test_prefix_rule_quirks():
    ill = b"HS25_09827:2:1101:1234:5678#49"
    assert E.prefix_rule(ill) == (11, True, 11) and E.prefix_rule(b"@" + ill) == (12, True, 12)
    assert E.prefix_rule(ill + b" 1:N:0:ATCACG")[0] == 11                            # counted back from the first blank
    assert E.prefix_rule(b"a:b:c") == (E.NO_PREFIX, False, 0)
    assert E.prefix_rule(b"ABCDE:00123:00456") == (6, True, 6) and E.prefix_rule(b"@ABCDE:00123:00456") == (6, True, 6)
    assert E.prefix_rule(b">BCDE:0:0123:00456")[0] != 6 and E.prefix_rule(b">ABCD:00123:00456")[0] != 6
    ont = b"f33d30d5-6eb8-4115-8f46-154c2620a5da_Basecall_1D_template"
    assert E.prefix_rule(ont) == (37, True, 37) and E.prefix_rule(b"@" + ont) == (37, True, 37)
    assert E.prefix_rule(b"g" + ont[1:])[0] != 37
    for what, block, _ in E.constructed():
        if what.startswith("PacBio"):
            assert all(E.prefix_rule(n) == (60, False, 0) for n in block.split(b"\n")[:9]), what


def test_tokenise_symbols_are_declared_exported_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    for meth in ("tok3_tokenise", "tok3_encode_names"):
        assert hasattr(codec.DeviceCodec, meth), meth


def test_tokenise_calls_refuse_a_null_context():
    import htscodecs_amd
    L = htscodecs_amd.load()
    off = (C.c_uint64 * 1)()
    first = (C.c_uint32 * 1)()
    assert L.rans4x16_hip_tok3_tokenise_dev(None, 0, None, None, None, None, 0, off, None, None, first, None, None, None, None,
                                            None, 1 << 20, 1000, 256, 128, 64, 0, 0, None) == -1
    meth = (C.c_int * 1)(0)
    assert L.rans4x16_hip_tok3_encode_names_dev(None, 0, None, None, None, None, 0, off, None, None, 1, meth, None, None,
                                                1 << 20, 1000, 256, 128, 64, 0, 0, 0, None) == -1
