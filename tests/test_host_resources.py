"""The owners of the context's HIP handles (3dobjecttracking_amd/csrc/m3t_host_resources.h: DevMem, Event, EventPair,
Stream, HostBlock, HostRing) on the host: tests/cpp/host_resources_check.cpp runs them against stand-ins for the runtime
functions the header calls -- what is live after every case (nothing), the flags each handle was made with, lazy creation,
moves without a second destroy, the ring's turns and its two ways to grow, and what a failing call leaves behind."""
import os
import re
import subprocess

import pytest

import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "host_resources_check.cpp")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
# the host compiler alone: the header needs the runtime's declarations, the program no runtime library
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", ROCM_INCLUDE]

CALLS = ["hipEventCreate", "hipEventDestroy", "hipStreamCreate", "hipExtStreamCreateWithCUMask", "hipStreamDestroy",
         "hipHostMalloc", "hipHostFree", "hipMalloc", "hipFree"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("host_resources") / "host_resources_check")
    subprocess.run(FLAGS + ["-o", path, SRC], check=True)
    return path


def test_owners_against_the_stand_in_runtime(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    m = re.search(r"^checks (\d+) errors (\d+)$", out.stdout, re.M)
    assert m and out.returncode == 0, out.stdout + out.stderr
    assert int(m.group(2)) == 0 and int(m.group(1)) >= 150
    assert out.stderr == ""


def test_no_other_source_creates_or_destroys_a_handle():
    """the search that stands in the place of a list in m3t_hip_destroy"""
    csrc = os.path.join(util.ROOT, "3dobjecttracking_amd", "csrc")
    pattern = re.compile(r"\b(%s)" % "|".join(CALLS))
    for name in sorted(os.listdir(csrc)):
        if name == "m3t_host_resources.h" or not name.endswith((".hip", ".h", ".inc")):
            continue
        text = open(os.path.join(csrc, name)).read()
        assert not pattern.search(text), (name, pattern.search(text).group(0))
    api = open(os.path.join(csrc, "m3t_hip_api.hip")).read()
    assert "Shutdown" not in api and "cam_stage" not in api
    # one destructor written by hand: it records the end of a timed launch and hands its events on; it frees nothing
    assert re.findall(r"~(\w+)\(\)", api) == ["ScopedKernelTimer"]
