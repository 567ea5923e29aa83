"""The ordering ledger of asynchronous frame ingest (3dobjecttracking_amd/csrc/m3t_ingest_plan.h: Ledger) on the host:
tests/cpp/ingest_plan_check.cpp drives it the way the upload entry points and the tracking step do and compares every
decision with written-down expectations -- the one synchronisation behind untracked launches, the two-slot loop for 40
steps (one event wait per copy stream per step, indices past the 16 step events), a slot overwritten 17 steps after its
only reader (the upload side takes the recycled index, the slot-sync side the whole stream), a slot never read, enqueued
calls with and without cameras, the pending mask."""
import os
import re
import subprocess

import pytest

import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "ingest_plan_check.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror"]


def _check(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    m = re.search(r"^checks (\d+) errors (\d+)$", out.stdout, re.M)
    assert m and out.returncode == 0, out.stdout + out.stderr
    assert int(m.group(2)) == 0 and int(m.group(1)) >= 100
    assert out.stderr == ""


def test_ledger_matches_the_written_down_decisions(tmp_path):
    path = str(tmp_path / "ingest_plan_check")
    subprocess.run(FLAGS + ["-o", path, SRC], check=True)
    _check(path)


def test_ledger_under_address_and_undefined_sanitizers(tmp_path):
    """the same stand-alone program, instrumented (needs the host compiler's sanitizer runtimes)"""
    have = [subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()
            for lib in ("libasan.so", "libubsan.so")]
    if not all(os.path.isabs(p) for p in have):
        pytest.skip("the host compiler's sanitizer runtimes are not installed")
    path = str(tmp_path / "ingest_plan_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", path, SRC], check=True)
    _check(path)
