"""What the tiled Hamming matcher (csrc/m3t_texture_tiled.hip) shares with the host, on the host:
tests/cpp/texture_tiled_check.cpp joins the best two of contiguous ranges with m3t_tex_best2_append (m3t_texture.h) and
compares with one sequential pass of m3t_tex_best2_update -- every split of every sequence of up to 6 distances out of
{0, 1, 2}, four-way splits with empty ranges, ties, empty and one-entry sides -- and runs the launch plan
(m3t_texture_plan.h) for every mode, 0 / 1 / 64 Hamming modalities and n_keyframes 1 and 8."""
import os
import re
import subprocess

import pytest

import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "texture_tiled_check.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]


def _check(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    m = re.search(r"^checks (\d+) errors (\d+)$", out.stdout, re.M)
    assert m and out.returncode == 0, out.stdout + out.stderr
    assert int(m.group(2)) == 0 and int(m.group(1)) >= 10000
    assert out.stderr == ""


def test_append_and_plan(tmp_path):
    path = str(tmp_path / "texture_tiled_check")
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", path, SRC], check=True)
    _check(path)


def test_append_and_plan_under_address_and_undefined_sanitizers(tmp_path):
    """the same stand-alone program, instrumented (needs the host compiler's sanitizer runtimes)"""
    have = [subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()
            for lib in ("libasan.so", "libubsan.so")]
    if not all(os.path.isabs(p) for p in have):
        pytest.skip("the host compiler's sanitizer runtimes are not installed")
    path = str(tmp_path / "texture_tiled_check_san")
    subprocess.run(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                                                    path, SRC], check=True)
    _check(path)
