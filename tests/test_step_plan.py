"""The launch choice of the tracking step (3dobjecttracking_amd/csrc/m3t_step_plan.h: StepKernel, ReadStepOverrides,
SplitParts, PlanRigidStep) on the host: tests/cpp/step_plan_check.cpp runs it against written-down expectations with a
stub in the place of the occupancy query -- the headline shape [64, 4, 512, 1] and its variants, the forced shapes, the
part counts and their three refusals, the compact kernels with the wide gap, the table gap and the overflow word, the
guard kernels behind rectangles, the 256-thread rule, and how each developer override reads its variable."""
import os
import re
import subprocess

import pytest

import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "step_plan_check.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror"]

# every enumerator of StepKernel in order: what m3t_hip_get_step_kernel / _variant can report ("": per-sub-step launches)
NAMES = [
    "",
    "tracking_step_kernel",
    "tracking_step_lds_kernel",
    "tracking_step_pair_kernel",
    "tracking_step_lds_pair_kernel",
    "tracking_step_guard_kernel",
    "tracking_step_lds_guard_kernel",
    "tracking_step_split_kernel",
    "tracking_step_split_pair_kernel",
    "tracking_step_split_moments_kernel",
    "tracking_step_split_guard_kernel",
    "tracking_step_split_render_kernel",
    "tracking_step_compact_kernel",
    "tracking_step_compact_table_kernel",
    "tracking_step_compact_wide_kernel",
    "tracking_step_compact_guard_kernel",
    "tracking_step_tree_kernel",
    "tracking_step_tree_constrained_kernel",
    "tracking_step_tree_split_kernel",
    "tracking_step_tree_segment_kernel",
    "tracking_step_tree_segment_constrained_kernel",
]


def _check(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    m = re.search(r"^checks (\d+) errors (\d+)$", out.stdout, re.M)
    assert m and out.returncode == 0, out.stdout + out.stderr
    assert int(m.group(2)) == 0 and int(m.group(1)) >= 100
    assert out.stderr == ""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("step_plan") / "step_plan_check")
    subprocess.run(FLAGS + ["-o", path, SRC], check=True)
    return path


def test_plan_matches_the_written_down_decision(exe):
    _check(exe)


def test_kernel_names(exe):
    out = subprocess.run([exe, "--names"], capture_output=True, text=True, timeout=60, check=True)
    assert out.stdout.split("\n")[:-1] == NAMES
    # every one of them is a kernel of the library's sources
    csrc = os.path.join(util.ROOT, "3dobjecttracking_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith(".hip"))
    for name in NAMES[1:]:
        assert re.search(r"^%s\(" % name, text, re.M), name


def test_plan_under_address_and_undefined_sanitizers(tmp_path):
    """the same stand-alone program, instrumented (needs the host compiler's sanitizer runtimes)"""
    have = [subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()
            for lib in ("libasan.so", "libubsan.so")]
    if not all(os.path.isabs(p) for p in have):
        pytest.skip("the host compiler's sanitizer runtimes are not installed")
    path = str(tmp_path / "step_plan_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", path, SRC], check=True)
    _check(path)
