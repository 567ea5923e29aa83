"""Tracker::ResetBodies of the C++ host mirror (include/m3t_hip.hpp): the demo compiles with plain g++ against the
C-ABI (CPU check), and on the GPU it runs the batch's reset-on-loss loop -- the resets the single oracle runs make,
handed to it as a plan -- to the poses of those single runs bit for bit (tests/selective_reset.py)."""
import os
import subprocess

import numpy as np
import pytest

import reset_loop
import scenes
import selective_reset as sr
import util

ROOT = util.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "reset_bodies_demo.cpp")


def _build(tmp_path):
    exe = str(tmp_path / "reset_bodies_demo")
    libdir = os.path.dirname(util.pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", libdir, "-lm3t_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_reset_bodies_demo_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path))


def _write_scene(d, inputs, resets, gt):
    i0 = inputs.intr
    dp0 = inputs.region_models[0][0]
    (d / "scene.txt").write_text("%d %d %d %d %r %r %r %r %d %d\n" % (
        inputs.n_objects, inputs.n_frames, i0["width"], i0["height"], i0["fu"], i0["fv"], i0["ppu"], i0["ppv"],
        dp0.shape[0], dp0.shape[1]))
    for i in range(inputs.n_objects):
        dp, ori, cl = inputs.region_models[inputs.model_of[i]]
        with open(d / ("model_%d.bin" % i), "wb") as f:
            f.write(np.ascontiguousarray(dp, np.float32).tobytes())
            f.write(np.ascontiguousarray(ori, np.float32).tobytes())
            f.write(np.ascontiguousarray(cl, np.float32).tobytes())
        np.ascontiguousarray(np.asarray(inputs.start[i], np.float32).T).tofile(d / ("start_%d.bin" % i))
        for k in range(inputs.n_frames):
            np.ascontiguousarray(inputs.color[i][k]).tofile(d / ("frame_%d_%d.bin" % (i, k)))
    lines = []
    for k in sorted({f for f, _ in resets}):
        ids = [i for f, i in resets if f == k]
        lines.append("%d %d %s" % (k, len(ids), " ".join(str(i) for i in ids)))
        np.stack([np.ascontiguousarray(np.asarray(gt[k][i], np.float32).T).reshape(16) for i in ids]).tofile(
            d / ("reset_%d.bin" % k))
    (d / "resets.txt").write_text("\n".join(lines) + "\n")


@pytest.mark.gpu
def test_cpp_reset_bodies_match_the_single_runs(tmp_path):
    inputs = scenes.Inputs(6, 7, n_divides=2)
    schedule = reset_loop.default_schedule(inputs.n_objects, inputs.n_frames)
    sr.check_schedule(schedule, inputs.n_objects, inputs.n_frames)
    ref_poses, ref_resets, _ = sr.expectation(inputs, schedule)
    d = tmp_path / "scene"
    d.mkdir()
    _write_scene(d, inputs, ref_resets, reset_loop.ground_truth(inputs, schedule))
    out = subprocess.run([_build(tmp_path), str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert "twice" in out.stderr  # the refused call said why
    cpp = np.array([[float.fromhex(x) for x in line.split()] for line in out.stdout.strip().splitlines()], np.float32)
    cpp = cpp.reshape(inputs.n_frames - 1, inputs.n_objects, 4, 4).transpose(0, 1, 3, 2)
    for k, ref in enumerate(ref_poses):
        assert np.array_equal(cpp[k], ref), (k + 1, np.argwhere(np.any(cpp[k] != ref, axis=(1, 2))).ravel().tolist())
