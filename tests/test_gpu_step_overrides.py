"""The developer overrides of the tracking step are read at the top of EVERY step (m3t_step_plan.h, ReadStepOverrides),
not once per context: one context steps four frames with the variables changed between its steps, takes the launch
shape each of them asks for, and ends every frame on the poses of a fresh context that stepped the same frames without
any override, bit for bit (the launch shapes compute the same bits)."""
import ctypes as C
import os

import numpy as np
import pytest

import scenes
import util

pytestmark = pytest.mark.gpu

OVERRIDES = ("M3T_HIP_NO_SPLIT", "M3T_HIP_SPLIT_PARTS", "M3T_HIP_THREADS", "M3T_HIP_COMPACT", "M3T_HIP_COMPACT_TABLE",
             "M3T_HIP_COMPACT_WIDE", "M3T_HIP_NO_PAIR", "M3T_HIP_NO_FUSED_HISTOGRAM", "M3T_HIP_NO_MOMENTS_FIRST")


def shape_of(api):
    shape = (C.c_int * 4)()
    api.call("get_step_shape", shape)
    return list(shape)


def trajectory(inputs, envs):
    """poses and launch shape after every frame, frame k stepped with the variables envs[k] set"""
    api = util.open_hip()
    a = scenes.Instance(api, inputs)
    a.upload_frame(0)
    assert a.tracker.StartModalities(0)
    poses, shapes = [], []
    for k in range(inputs.n_frames):
        for name in OVERRIDES:
            os.environ.pop(name, None)
        os.environ.update(envs[k])
        try:
            a.upload_frame(k)
            assert a.tracker.ExecuteTrackingStep(k)
        finally:
            for name in envs[k]:
                os.environ.pop(name, None)
        poses.append(np.stack(a.poses()))
        shapes.append(shape_of(api))
    return poses, shapes


def test_overrides_are_read_at_every_step():
    inputs = scenes.Inputs(2, 4, n_divides=2, n_models=2)
    ref, ref_shapes = trajectory(inputs, [{}] * 4)
    got, shapes = trajectory(inputs, [{"M3T_HIP_SPLIT_PARTS": "4"}, {"M3T_HIP_NO_SPLIT": "1"},
                                      {"M3T_HIP_NO_SPLIT": "1", "M3T_HIP_THREADS": "256"}, {}])
    print("shapes", shapes, "fresh context", ref_shapes)
    assert shapes[0][:2] == [2, 4]
    assert shapes[1] == [2, 1, 512, 1]
    assert shapes[2] == [2, 1, 256, 0]
    assert shapes[3] == ref_shapes[3] and ref_shapes[3][0] == 2 and ref_shapes[3][1] > 1
    for k in range(inputs.n_frames):
        assert np.array_equal(got[k], ref[k]), k
