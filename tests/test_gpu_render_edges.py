"""The focused renderers' kernels (csrc/m3t_render.hip: focused_setup_kernel, focused_resolve_kernel and the three-launch
form focused_clear_kernel / focused_raster_kernel / focused_unpack_kernel) against the oracle on the cases of
tests/render_edges.py: later trips of the set-up and resolve loops, the LDS queue of the three-launch form and its
overflow, every band geometry and both store paths, twins in both creation orders, and geometry at the edges of the
arithmetic.  Bit for bit: depth image, silhouette image, corner, scale and n_visible, of both twins on the tracker path.
tests/test_render_edge_cases.py shows on the host that every case reaches its branch."""
import numpy as np
import pytest

import render_edges as re_
import util

pytestmark = pytest.mark.gpu

CASES = re_.cases()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": depth image"
    assert (got[1] is None and want[1] is None) or np.array_equal(got[1], want[1]), what + ": silhouette image"
    assert np.array_equal(np.array(got[2:5], np.float32), np.array(want[2:5], np.float32)), what + ": corner, scale"
    assert got[5] == want[5], what + ": n_visible"


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_rendering_equals_the_oracle(c):
    got = re_.render_case(util.open_hip(), c)
    want = re_.render_case(util.open_oracle(), c)
    assert len(got) == len(want) == (2 if c["path"] == "tracker" or c["moved"] is not None else 1)
    for k, ((name, a), (_, b)) in enumerate(zip(got, want)):
        _same(a, b, "%s, %s" % (c["name"], name))
        drawn = int((a[0] != 65535).sum())
        if c["drawn"] or k == 1:
            assert drawn > 0 and (not c.get("last_row") or (a[0][-1] != 65535).any())
        else:
            assert drawn == 0 and (a[1] is None or not a[1].any())
            if a[5] == 0:
                assert a[2:5] == (0.0, 0.0, 1.0)


def test_crop_sweep_equals_the_oracle():
    """256 poses of one small body through one context: visibility at its thresholds, the crop, the images"""
    poses, _ = re_.sweep_poses()
    got = re_.render_sweep(util.open_hip(), poses)
    want = re_.render_sweep(util.open_oracle(), poses)
    for k, (a, b) in enumerate(zip(got, want)):
        _same(a, b, "pose %d" % k)
    visible = [a[5] for a in got]
    assert 50 < sum(visible) < 220 and sum(int((a[0] != 65535).any()) for a in got) > 50
