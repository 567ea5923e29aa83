"""The argument blocks of the enqueued calls (3dobjecttracking_amd/csrc/m3t_call_args.h: Layout, the three calls'
segments, the Put functions) on the host: tests/cpp/call_args_check.cpp fills blocks of exactly the size the layout
asks for in ordinary memory and compares offsets, sizes and every byte with written-down expectations -- where the
poses of reset_bodies and reset_structures begin at each residue of the int count, where the renderer pairs go, a call
without poses, and the poses-first block of judge_bodies with and without region modalities."""
import os
import re
import subprocess

import pytest

import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "call_args_check.cpp")


def _check(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    m = re.search(r"^checks (\d+) errors (\d+)$", out.stdout, re.M)
    assert m and out.returncode == 0, out.stdout + out.stderr
    assert int(m.group(2)) == 0 and int(m.group(1)) >= 50
    assert out.stderr == ""


def test_blocks_match_the_written_down_layouts(tmp_path):
    path = str(tmp_path / "call_args_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", path, SRC], check=True)
    _check(path)


def test_blocks_under_address_and_undefined_sanitizers(tmp_path):
    """the same stand-alone program, instrumented (needs the host compiler's sanitizer runtimes): a segment that ran
    over the end of its block would be a heap overflow here"""
    have = [subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()
            for lib in ("libasan.so", "libubsan.so")]
    if not all(os.path.isabs(p) for p in have):
        pytest.skip("the host compiler's sanitizer runtimes are not installed")
    path = str(tmp_path / "call_args_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", path, SRC], check=True)
    _check(path)
