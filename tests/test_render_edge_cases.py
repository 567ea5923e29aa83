"""Every case of tests/render_edges.py is live, shown on the host: the counters of tests/cpp/raster_stats.cpp
(raster_edge_stats: what becomes of every triangle and pixel under the case's projection) and the plan of
csrc/m3t_render_plan.h say that the case reaches the branch it was written for, and the oracle's images equal the host
restatement of the device's arithmetic (raster_body) -- the reference is validated on these scenes before a GPU is
involved.  Each test prints the counter that makes its case live (pytest -s shows them)."""
import numpy as np
import pytest

import render_edges as re_
import util

CASES = re_.cases()


@pytest.fixture(scope="module")
def oracle():
    return util.open_oracle


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case_is_live_and_the_oracle_equals_the_host_restatement(c, oracle):
    pl = re_.case_plan(c)
    bodies, intr = re_.case_scene(c)
    st = re_.case_stats(c, bodies, c["S"], pl["slices"], intr=intr)
    print("\n%s: %s" % (c["name"], c["live"](st, pl)))
    assert (st["covered"] > 0) == c["drawn"]
    renderings = re_.render_case(oracle(), c)
    assert len(renderings) == (2 if c["path"] == "tracker" or c["moved"] is not None else 1)
    for k, (name, (depth, sil, corner_u, corner_v, scale, n_visible)) in enumerate(renderings):
        scene = bodies
        if c["moved"] is not None and k == 1:
            scene = [dict(bodies[0], pose=c["moved"])] + list(bodies[1:])
        S = depth.shape[0]
        want_depth, want_sil, pr = re_.host_rendering(c, scene, S, sil is not None, c["id_type"], intr=intr)
        assert n_visible == pr["n_visible"]
        assert (np.float32(corner_u), np.float32(corner_v), np.float32(scale)) == (pr["corner_u"], pr["corner_v"], pr["scale"])
        assert np.array_equal(depth, want_depth), name
        if sil is not None:
            assert np.array_equal(sil, want_sil), name
        assert ((depth != 65535).sum() > 0) == (c["drawn"] or k == 1)
        if c.get("last_row"):  # something is drawn in the last band's rows: a store that is left out shows
            assert (depth[-1] != 65535).any()
        if "owner" in c:  # two bodies at equal depth: the first drawn owns every pixel
            assert set(np.unique(sil)) == {0, c["owner"]}
        if "ids" in c:
            assert c["ids"] <= set(np.unique(sil)) and (sil[depth != 65535] == 0).any()


def test_the_set_of_band_cases_takes_every_store_path():
    plans = [re_.case_plan(c) for c in CASES if c["name"].startswith(("bands_", "twins_"))]
    plans += [p["small"] for p in plans if "small" in p]
    for key in ("vector_bands", "scalar_bands", "one_row_bands", "partial_bands", "empty_bands"):
        assert any(p[key] > 0 for p in plans), key
    twins = [re_.case_plan(c) for c in CASES if c["name"].startswith("twins_")]
    assert any(p["vector_bands"] > 0 and p["scalar_bands"] > 0 for p in twins)  # both twin store paths in one launch


def test_crop_sweep_straddles_every_threshold():
    """the oracle's visibility and crop equal the float32 restatement at all 256 poses, and inside each group of four
    consecutive float32 values around a threshold the outcome changes between the second and the third"""
    poses, groups = re_.sweep_poses()
    assert len(poses) == 256
    got = re_.render_sweep(util.open_oracle(), poses)
    seen = []
    for (pose, which), (depth, sil, corner_u, corner_v, scale, n_visible) in zip(poses, got):
        pr = re_.sweep_projection(pose, which)
        assert n_visible == pr["n_visible"]
        assert (np.float32(corner_u), np.float32(corner_v), np.float32(scale)) == (pr["corner_u"], pr["corner_v"], pr["scale"])
        seen.append(n_visible)
    for a, b in groups:
        print("threshold group %d: n_visible %s" % (a // 4, seen[a:b]))
        assert seen[a + 1] != seen[a + 2]  # (the outer two may flip again: the rounded bounds are not monotone)
    rest = seen[groups[-1][1]:]
    assert 20 < sum(rest) < len(rest) - 20  # seeded poses on both sides
    assert sum((d != 65535).any() for d, *_ in got) > 50
