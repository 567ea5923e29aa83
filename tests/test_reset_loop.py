"""The reset-on-loss loop of tests/reset_loop.py over the CPU oracle: the injected losses make exactly the resets they
are meant to, the batch is tracked to the end, and every rotation entry moves the model's closest view out of the
neighbour row the device's view search starts from (closest_view_local, m3t_kernels.hip) -- what the GPU tests of the
same loop (test_gpu_reset_on_loss.py) rely on."""
import pytest

import reset_loop
import scenes
import util


@pytest.fixture(scope="module")
def inputs():
    return scenes.Inputs(6, 6, n_divides=4)  # 2562-view models, like the benchmarked batch


@pytest.mark.parametrize("mode", ["restart", "pose-only"])
def test_oracle_resets_as_scheduled(inputs, mode):
    schedule = reset_loop.default_schedule(inputs.n_objects, inputs.n_frames)
    assert {kind for _, _, kind in schedule} == {"a", "b", "c"}
    assert schedule[0][0] == 1 and max(f for f, _, _ in schedule) == inputs.n_frames - 1
    poses, resets, hist, before = reset_loop.run(util.open_oracle(), inputs, schedule, mode)
    assert len(poses) == inputs.n_frames - 1 and len(hist) == inputs.n_objects
    assert resets == reset_loop.expected_resets(schedule, inputs.n_frames, mode), resets
    # the batch is a meaningful one: every object ends within 5 cm / 5 degrees of its ground truth
    assert reset_loop.check_tracked(inputs, poses, schedule) == []
    # a rotation reset leaves the neighbour row of the view the body was at: the full view scan has to run
    jumps = reset_loop.view_jumps(inputs, schedule, before)
    assert len(jumps) == 2 and all(outside for _, _, outside in jumps), jumps


def test_offsets_are_deterministic(inputs):
    schedule = reset_loop.default_schedule(inputs.n_objects, inputs.n_frames)
    a, b = reset_loop.ground_truth(inputs, schedule), reset_loop.ground_truth(inputs, schedule)
    for frame, obj, kind in schedule:
        assert (a[frame][obj] == b[frame][obj]).all()
        t, r, ok = util.pkg.evaluation.rbot_pose_result(a[frame][obj], inputs.gt[obj][frame])
        assert ok == 0.0, (frame, obj, kind)
        if kind == "c":  # the body's origin on a vertical image border
            p, intr = a[frame][obj], inputs.intr
            u = intr["fu"] * p[0, 3] / p[2, 3] + intr["ppu"]
            assert min(abs(u), abs(u - intr["width"])) < 1e-2, u
