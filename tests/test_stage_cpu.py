"""The staging layout of the host-buffer calls (htscodecs_amd/csrc/r4x16_stage.h: the slot planner and the one layout of
payload regions and per-item arrays) needs neither a GPU nor the library: tests/host/stage_check.cpp includes that header
alone, is built here with the address and undefined-behaviour sanitizers and runs as a program of its own."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_stage_header_passes_its_stand_alone_check_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/stage_check.cpp"
    exe = str(tmp_path / "stage_check")
    # (the sanitizer runtimes linked in: the program stands alone whatever the environment preloads)
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "htscodecs_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "stage_check.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().endswith("stage_check: ok"), run.stdout
