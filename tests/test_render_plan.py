"""The launch choice of the focused renderers (3dobjecttracking_amd/csrc/m3t_render_plan.h: ReadRenderOverrides,
RenderShape, LdsRasterFits, RowsOfBand) on the host: tests/cpp/render_plan_check.cpp runs it against written-down
expectations -- 1, 2, 8 and 128 pairs at S = 8, 9, 13, 64, 200, 333 and 1024, each developer override and how it is read
from the environment, both sides of the 160 KB boundary, and how the bands cut the images (vector and scalar stores,
one-row, partial and empty bands)."""
import os
import re
import subprocess

import pytest

import render_edges
import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "render_plan_check.cpp")


def _check(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    m = re.search(r"^checks (\d+) errors (\d+)$", out.stdout, re.M)
    assert m and out.returncode == 0, out.stdout + out.stderr
    assert int(m.group(2)) == 0 and int(m.group(1)) >= 74
    assert out.stderr == ""


def test_plan_matches_the_written_down_decision():
    _check(render_edges.plan_exe())


def test_plan_on_the_command_line():
    assert render_edges.plan(1, 200) == dict(form="lds", slices=128, bands=100, lds=11908, band_rows=2, vector_bands=100,
                                             scalar_bands=0, one_row_bands=0, partial_bands=0, empty_bands=0)
    assert render_edges.plan(1, 13, env={"M3T_HIP_RASTER_BANDS": "4", "M3T_HIP_RASTER_SLICES": "3"}) == dict(
        form="lds", slices=3, bands=4, lds=10516, band_rows=4, vector_bands=3, scalar_bands=1, one_row_bands=1,
        partial_bands=1, empty_bands=0)
    three = render_edges.plan(1, 64, env={"M3T_HIP_NO_LDS_RASTER": "1"})
    assert three["form"] == "three" and three["slices"] == 32 and three["bands"] == 0
    assert render_edges.plan(1, 333, env={"M3T_HIP_RASTER_BANDS": "2"})["form"] == "three"
    assert render_edges.plan(1, 333, env={"M3T_HIP_RASTER_BANDS": "3"})["form"] == "lds"
    small = render_edges.plan(2, 333, image=8)
    assert small["bands"] == 128 and small["band_rows"] == 1 and small["empty_bands"] == 120


def test_the_library_uses_the_header():
    """the rule is stated once: the library's translation unit includes the header and keeps no copy of the formula"""
    text = open(os.path.join(util.ROOT, "3dobjecttracking_amd", "csrc", "m3t_hip_api.hip")).read()
    assert '#include "m3t_render_plan.h"' in text
    assert "M3T_HIP_RASTER_BANDS" not in text and "M3T_HIP_NO_LDS_RASTER" not in text and "256 / std::max" not in text


def test_plan_under_address_and_undefined_sanitizers(tmp_path):
    """the same stand-alone program, instrumented (needs the host compiler's sanitizer runtimes)"""
    have = [subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()
            for lib in ("libasan.so", "libubsan.so")]
    if not all(os.path.isabs(p) for p in have):
        pytest.skip("the host compiler's sanitizer runtimes are not installed")
    path = str(tmp_path / "render_plan_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", path, SRC], check=True)
    _check(path)
