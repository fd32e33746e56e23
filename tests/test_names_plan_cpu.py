"""The cut of a host names batch into chunks (r4x16_cut_ranges, htscodecs_amd/csrc/r4x16_plan.h) needs neither a GPU nor
the library: tests/host/names_plan_check.cpp includes that header alone, is built here with the address and
undefined-behaviour sanitizers and runs as a program of its own - the cut against a brute-force scan on random
footprints, contiguous ranges that cover 0 .. n, every range within the cap or of one block, the item limit, zero blocks
and one huge block."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_range_cut_passes_its_stand_alone_check_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/names_plan_check.cpp"
    exe = str(tmp_path / "names_plan_check")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "htscodecs_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "names_plan_check.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().endswith("names_plan_check: ok"), run.stdout
