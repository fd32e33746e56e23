"""tok3 containers of the arith flavour (use_arith = 1), the half that needs no GPU: rans4x16_hip_tok3_scan_any against
rans4x16_hip_tok3_scan and against the model walk on the 110 reference-made containers and on damaged variants, the
composed model (tok3_arith_model.py) against the reference's containers and names files, the drop-in header with both
flavours from C and from C++, and the setter's refusal of a NULL context."""
import ctypes as C
import os
import re
import subprocess

import pytest

import tok3_arith_model as TA
import tok3_model as M
import tok3_names_model as N
from test_tok3_cpu import WALK_CASES, _descriptor_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "htscodecs_amd")
NEW = ("rans4x16_hip_tok3_scan_any", "rans4x16_hip_set_tok3_arith", "rans4x16_hip_tok3_arith_encode_names",
       "rans4x16_hip_tok3_arith_decode_names", "rans4x16_hip_arith_compress_best_packed_dev",
       "rans4x16_hip_arith_best_chunk_blocks", "rans4x16_hip_thread_ctx")


def _gpu():
    import torch
    return torch.cuda.is_available()


def _info(w):
    return {"last_start": w.last_start, "nreads": w.nreads, "ndesc": w.ndesc, "ncol": w.ncol, "total_col_size": w.total,
            "largest_col": w.largest_col, "largest_stream": w.largest_stream}


def _same_as_model(buf, what, **kw):
    """scan_any equals the model walk of either flavour: status, counts and the flavour.  Returns the status."""
    from htscodecs_amd import codec
    w, arith = TA.walk(buf, **{k: v for k, v in kw.items() if v})
    st, info, got = codec.tok3_scan_any(buf, **kw)
    assert st == w.status, (what, st, w.status)
    assert info == _info(w), what
    assert got == arith, (what, got, arith)
    return st


def test_the_new_symbols_are_declared_exported_bound_and_wrapped():
    import htscodecs_amd
    from htscodecs_amd import codec, lib as hlib
    L = htscodecs_amd.load()
    header = open(os.path.join(ROOT, "include", "rans4x16_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in hlib.SIGNATURES, name
    assert re.search(r"#define\s+R4X16_TOK3_ARITH_DECODE\s+1\b", header) and re.search(r"#define\s+R4X16_TOK3_ARITH_ENCODE\s+2\b", header)
    assert callable(codec.tok3_scan_any) and callable(codec.set_tok3_arith)
    for meth in ("set_tok3_arith", "arith_compress_best_packed"):
        assert hasattr(codec.DeviceCodec, meth), meth


def test_the_calls_refuse_a_null_context():
    import htscodecs_amd
    L = htscodecs_amd.load()
    for mode in (0, 1, 2, 3):
        assert L.rans4x16_hip_set_tok3_arith(None, mode) == -1
    meth = (C.c_int * 2)(0, 1)
    off = (C.c_uint64 * 1)()
    assert L.rans4x16_hip_arith_compress_best_packed_dev(None, 0, None, None, None, None, 0, off, None, None, 2, meth, None, 0, 0, None) == -1
    assert L.rans4x16_hip_arith_best_chunk_blocks(None, 1, 2, meth, 8, 0) == -1
    if not _gpu():
        assert not L.rans4x16_hip_thread_ctx()                       # no device: no context (and no CPU path)


def test_scan_any_refuses_bad_arguments_like_scan():
    import htscodecs_amd
    L = htscodecs_amd.load()
    assert L.rans4x16_hip_tok3_scan_any(None, 9, 0, 0, None, None, None, None, None, None, None, None) == -1
    assert L.rans4x16_hip_tok3_scan_any(b"\0" * 9, 9, 2049, 0, None, None, None, None, None, None, None, None) == -1
    assert L.rans4x16_hip_tok3_scan_any(b"\0" * 9, 9, 0, 0, None, None, None, None, None, None, None, None) == 0
    assert L.rans4x16_hip_tok3_scan_any(b"\0" * 8 + b"\7", 9, 0, 0, None, None, None, None, None, None, None, None) == 0


def test_scan_any_equals_scan_on_the_rans_flavour():
    from htscodecs_amd import codec
    fx = M.fixtures()
    assert len(fx) == 55
    cases = [(name, buf) for name, buf in fx] + [(what, buf) for what, buf, _ in WALK_CASES if len(buf) < 9 or buf[8] == 0]
    assert len(cases) == 55 + len(WALK_CASES) - 1
    for what, buf in cases:
        st, info = codec.tok3_scan(buf)
        assert codec.tok3_scan_any(buf) == (st, info, 0), what
        assert _same_as_model(buf, what) == st


def test_scan_any_walks_the_arith_fixtures_and_scan_still_refuses_them():
    from htscodecs_amd import codec
    fx = TA.fixtures()
    assert len(fx) == 55 and sum(len(b) for _, b in fx) == 235243 and max(len(b) for _, b in fx) == 9798
    for name, buf in fx:
        assert buf[8] == 1, name
        st, info, arith = codec.tok3_scan_any(buf)
        assert (st, arith) == (0, 1), name
        assert (0, info) == codec.tok3_scan(TA.cleared(buf)), name
        assert _same_as_model(buf, name) == 0
        refused, seen = codec.tok3_scan(buf)
        assert refused == M.UNSUPPORTED and seen["ndesc"] == 0, name
        # the limits: exactly enough, and one short
        w, _ = TA.walk(buf)
        assert _same_as_model(buf, name, max_columns=w.ndesc, max_col_size=w.largest_col) == 0
        assert _same_as_model(buf, name, max_col_size=w.largest_col - 1) == M.UNSUPPORTED


def test_scan_any_equals_the_model_on_damaged_arith_containers():
    by = dict(TA.fixtures())
    small = [(n, by[n]) for n in ("nv2.names.17", "20.names.17")]       # the smallest fixtures of two names files
    assert small[0][1] == min(by.values(), key=len)
    seen = {}
    count = 0
    for name, buf in small:
        for p in _descriptor_bytes(TA.cleared(buf)):
            for x in (0x01, 0x40, 0x80, 0xFF):
                b = bytearray(buf)
                b[p] ^= x
                st = _same_as_model(bytes(b), (name, p, x))
                seen[st] = seen.get(st, 0) + 1
                count += 1
    for n in range(len(small[0][1])):
        st = _same_as_model(small[0][1][:n], ("cut", n))
        seen[st] = seen.get(st, 0) + 1
        count += 1
    assert count >= 1000, count
    # (EMPTY needs a clen edited to 0, which no xor of this set does to these containers: tests/test_tok3_cpu.py has it)
    assert {M.OK, M.TRUNCATED, M.SIZE, M.UNSUPPORTED} <= set(seen), seen


# ---- the composed model against the reference's own data ------------------------------------------------------------
@pytest.fixture(scope="module")
def files():
    return N.names_files()


@pytest.mark.parametrize("name", [n for n, _ in TA.fixtures()])
def test_the_model_decodes_every_arith_fixture_to_its_names_file(files, name):
    buf = dict(TA.fixtures())[name]
    st, out = TA.names(buf)
    assert st == 0 and out == files[name.split(".")[0]].replace(b"\n", b"\0"), name


@pytest.mark.parametrize("name", TA.BYTE_EXACT)
def test_the_model_reproduces_the_byte_exact_fixtures(name):
    assert len(TA.BYTE_EXACT) == 22
    buf = dict(TA.fixtures())[name]
    out, chosen = TA.reframed(buf, TA.ROWS[TA.level_of(name)])
    assert out == buf, name
    assert len(chosen) == len(M.described(M.walk(TA.cleared(buf))))


# ---- the drop-in header ---------------------------------------------------------------------------------------------
SHIM_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "tok3_names_hip.h"
int main(int argc, char **argv)
{
    int flavour, bad = 0;
    (void)argv;
    for (flavour = 0; flavour < 2; flavour++) {
        char names[] = "read.1\nread.2\nread.3\n";
        int out_len = -1, last_start = -1;
        int use_arith = argc > 5 ? 1 - flavour : flavour;            /* a run-time flag: both branches stay */
        unsigned char *c = encode_names(names, (int)strlen(names), 7, use_arith, &out_len, &last_start);
        unsigned char junk[16] = {0};
        uint32_t n = 0;
        unsigned char *d;
        junk[8] = (unsigned char)use_arith;
        d = decode_names(junk, sizeof junk, &n);
        printf("%s %s\n", c ? "container" : "null", d ? "names" : "null");
        if (c && (out_len < 9 || c[8] != use_arith || last_start != (int)strlen(names) || names[6] != 0)) bad = 2;
        free(c);
        free(d);
    }
    return bad;
}
"""


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_drop_in_header_serves_both_flavours(tmp_path, lang):
    import htscodecs_amd
    htscodecs_amd.load()
    src = tmp_path / ("shim." + ("c" if lang == "c" else "cpp"))
    src.write_text(SHIM_MAIN)
    exe = str(tmp_path / "shim")
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-std=c++11"]
    r = subprocess.run(cc + ["-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                             "-L", LIBDIR, "-lrans4x16_hip", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    und = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1].split("@")[0] for ln in und.splitlines() if ln.strip()}
    assert {"rans4x16_hip_tok3_encode_names", "rans4x16_hip_tok3_decode_names", "rans4x16_hip_tok3_arith_encode_names",
            "rans4x16_hip_tok3_arith_decode_names"} <= names
    assert "encode_names" not in names and "decode_names" not in names
    if _gpu():
        return                                                      # (tests/test_gpu_tok3_arith.py runs the calls)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr)
    assert run.stdout.split("\n")[:2] == ["null null", "null null"]
