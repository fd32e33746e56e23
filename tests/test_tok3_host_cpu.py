"""The host-buffer names calls (include/rans4x16_hip.h part 2f) as far as they go without a GPU: the method rows of the
levels, the drop-in header include/tok3_names_hip.h from C and from C++, and the refusals of a machine without a device
(NULL from the two functions, -1 from the batches: the library has no CPU path)."""
import ctypes as C
import os
import subprocess

import pytest

import htscodecs_amd
from htscodecs_amd import codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "htscodecs_amd")

# tokenise_name3.c:1254-1260, the methods of each row
ROWS = [[0, 128], [0, 200], [0, 128, 201], [0, 1, 129, 65, 193, 201], [0, 1, 128, 129, 64, 65, 192, 193, 201]]


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_level_methods_are_the_reference_rows():
    L = htscodecs_amd.load()
    for level in range(-3, 26):
        row = ROWS[min(max(int((level - 1) / 2), 0), 4)]          # C division: towards zero
        assert codec.tok3_level_methods(level) == row, level
    assert [codec.tok3_level_methods(v) for v in (1, 3, 5, 7, 9)] == ROWS
    assert L.rans4x16_hip_tok3_level_methods(5, None) == -1


SHIM_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "tok3_names_hip.h"
int main(void)
{
    char names[] = "read.1\nread.2\nread.3\n";
    int out_len = -1, last_start = -1;
    unsigned char *c = encode_names(names, (int)strlen(names), 7, 0, &out_len, &last_start);
    unsigned char junk[16] = {0};
    uint32_t n = 0;
    unsigned char *d = decode_names(junk, sizeof junk, &n);
    printf("%s %s\n", c ? "container" : "null", d ? "names" : "null");
    if (c && (out_len < 9 || last_start != (int)strlen(names) || names[6] != 0)) return 2;
    free(c);
    free(d);
    return 0;
}
"""


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_drop_in_header_compiles_links_and_fails_cleanly_without_a_gpu(tmp_path, lang):
    htscodecs_amd.load()
    src = tmp_path / ("shim." + ("c" if lang == "c" else "cpp"))
    src.write_text(SHIM_MAIN)
    exe = str(tmp_path / "shim")
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-std=c++11"]
    r = subprocess.run(cc + ["-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                             "-L", LIBDIR, "-lrans4x16_hip", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the header's two functions stay the program's own: nothing but rans4x16_hip_* is asked of the library
    und = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1].split("@")[0] for ln in und.splitlines() if ln.strip()}
    assert {"rans4x16_hip_tok3_encode_names", "rans4x16_hip_tok3_decode_names"} <= names
    assert "encode_names" not in names and "decode_names" not in names
    if _gpu():
        return                                                      # (tests/test_gpu_tok3_host.py runs the calls)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr)
    assert run.stdout.strip() == "null null"
    assert run.stderr.count("no CPU path") == 1, run.stderr


def test_without_a_gpu_the_calls_refuse():
    if _gpu():
        pytest.skip("GPU present")
    L = htscodecs_amd.load()
    assert codec.encode_names(b"a.1\na.2\n", 7) is None
    assert codec.decode_names(b"\0" * 16) is None
    blk = b"a.1\na.2\n"
    in_p = (C.c_char_p * 1)(blk)
    in_sz = (C.c_uint * 1)(len(blk))
    out_p = (C.c_void_p * 1)()
    out_sz = (C.c_uint * 1)()
    meth = (C.c_int * 1)(0)
    assert L.rans4x16_hip_tok3_encode_names_batch(None, 1, in_p, in_sz, out_p, out_sz, 1, meth, None, None, None) == -1
    assert L.rans4x16_hip_tok3_decode_names_batch(None, 1, in_p, in_sz, out_p, out_sz, None, None) == -1
    assert not out_p[0]
    assert L.rans4x16_hip_set_names_chunk_blocks(None, 4) == -1
