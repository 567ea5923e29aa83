"""The built-in texture detector on the CPU: the functions of csrc/m3t_features.h, assembled by
tests/cpp/feature_check.cpp, against the numpy restatement (tests/feature_reference.py) byte for byte on seeded images,
the same program under the address and undefined-behaviour sanitizers, and properties of the restatement itself:
corners of a checker land where they are drawn, selection keeps the first corners in raster order among equals, and a
descriptor changes in fewer bits under a turn of the patch than between unrelated patches."""
import os
import re
import subprocess

import numpy as np
import pytest

import feature_reference as FR
import feature_scenes as FS
import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "feature_check.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
# (bgr image, scale, n_features, fast_threshold): scale below and above 1, sides that are no multiple of anything,
# fewer and more corners than n_features
CASES = [
    (FS.blocks(97, 131, seed=1), 0.83, 500, 20),
    (FS.blocks(61, 77, seed=2, n=40, low=3, high=9), 1.37, 25, 12),
    (FS.as_bgr(FS.squares(90, 90, period=12, size=6, origin=(3, 5))), 1.0, 30, 20),
    (FS.as_bgr(np.full((70, 50), 93, np.uint8)), 1.21, 500, 20),
]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("feature_check") / "feature_check")
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", path, SRC], check=True)
    return path


def _run(exe, tmp_path, case=None):
    args = [exe]
    if case is not None:
        image, scale, n_features, threshold = case
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([image.shape[1], image.shape[0], n_features, threshold], np.int32).tobytes())
            f.write(np.float32(scale).tobytes())
            f.write(np.ascontiguousarray(image, np.uint8).tobytes())
        args += [src, dst]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    m = re.search(r"^checks (\d+) errors (\d+)$", out.stdout, re.M)
    assert m and out.returncode == 0, out.stdout + out.stderr
    assert int(m.group(2)) == 0 and int(m.group(1)) >= 100
    assert out.stderr == ""
    return open(dst, "rb").read() if case is not None else None


def _parse(blob):
    fw, fh = np.frombuffer(blob, np.int32, 2)
    at = 8
    focused = np.frombuffer(blob, np.uint8, fw * fh, at).reshape(fh, fw)
    at += fw * fh
    scores = np.frombuffer(blob, np.uint16, fw * fh, at).reshape(fh, fw)
    at += 2 * fw * fh
    n = int(np.frombuffer(blob, np.int32, 1, at)[0])
    at += 4
    rows = np.frombuffer(blob, np.int32, 3 * n, at).reshape(n, 3)
    at += 12 * n
    descriptors = np.frombuffer(blob, np.uint8, 32 * n, at).reshape(n, 32)
    assert at + 32 * n == len(blob)
    return focused, scores, rows, descriptors


def _compare(blob, case):
    image, scale, n_features, threshold = case
    focused, scores, rows, descriptors = _parse(blob)
    roi = (0, 0, image.shape[1], image.shape[0])
    expected = FR.focus(image, roi, np.float32(scale))
    assert np.array_equal(focused, expected)
    assert np.array_equal(scores, FR.suppress(FR.fast_scores(expected, threshold)))
    xy, _, bins, expected_descriptors = FR.detect_focused(expected, n_features, threshold)
    assert np.array_equal(rows[:, :2], xy) and np.array_equal(rows[:, 2], bins)
    assert np.array_equal(descriptors, expected_descriptors)
    return len(xy), int(np.count_nonzero(scores))


def test_header_functions_equal_the_restatement_on_seeded_images(check_exe, tmp_path):
    kept = [_compare(_run(check_exe, tmp_path, case), case) for case in CASES]
    # not vacuous: fewer corners than n_features, more than n_features (twice), none
    assert 20 < kept[0][0] == kept[0][1] < 500
    assert kept[1][0] == 25 < kept[1][1]
    assert kept[2][0] == 30 < kept[2][1]
    assert kept[3] == (0, 0)


def test_header_functions_under_address_and_undefined_sanitizers(tmp_path):
    """the same stand-alone program, instrumented (needs the host compiler's sanitizer runtimes)"""
    have = [subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()
            for lib in ("libasan.so", "libubsan.so")]
    if not all(os.path.isabs(p) for p in have):
        pytest.skip("the host compiler's sanitizer runtimes are not installed")
    path = str(tmp_path / "feature_check_san")
    subprocess.run(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                                                    path, SRC], check=True)
    for case in CASES[:2]:
        _compare(_run(path, tmp_path, case), case)


def test_pattern_header_is_what_the_tool_describes():
    """256 distinct tests of two different points within radius 13; the tables are the rounded cosines and sines"""
    p = FR.PATTERN
    assert p.shape == (256, 4) and np.abs(p).max() <= 13
    assert ((p[:, 0] ** 2 + p[:, 1] ** 2) <= 169).all() and ((p[:, 2] ** 2 + p[:, 3] ** 2) <= 169).all()
    assert not ((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])).any()
    assert len({tuple(r) for r in p}) == 256
    angles = 2 * np.pi * np.arange(30) / 30
    assert np.array_equal(FR.COS, np.rint(16384 * np.cos(angles)).astype(np.int64))
    assert np.array_equal(FR.SIN, np.rint(16384 * np.sin(angles)).astype(np.int64))
    for k in range(30):  # a turned point stays within the radius the border allows for
        assert np.abs(FR.rotated_pattern(k)).max() <= 13


def test_checker_corners_land_where_they_are_drawn():
    """a cell corner of a checker is an X junction, which the segment test does not answer; the corners of isolated
    squares are L corners: every drawn corner inside the border is found at the corner pixel of its square"""
    image = FS.squares(100, 100, period=20, size=8, origin=(6, 6))
    score_map = FR.suppress(FR.fast_scores(image, 20))
    found = {(int(x), int(y)) for y, x in zip(*np.nonzero(score_map))}
    drawn = set()
    for y in range(6, 93, 20):
        for x in range(6, 93, 20):
            drawn |= {(x, y), (x + 7, y), (x, y + 7), (x + 7, y + 7)}
    inside = {(x, y) for x, y in drawn if FR.BORDER <= x < 100 - FR.BORDER and FR.BORDER <= y < 100 - FR.BORDER}
    assert len(inside) >= 36 and found == inside
    assert not FR.suppress(FR.fast_scores(FS.checker(100, 100, 10), 20)).any()  # X junctions only
    assert not FR.fast_scores(np.full((100, 100), 77, np.uint8)).any()


def test_border_and_suppression():
    def square_at(x, y, size=64):
        image = np.full((size, size), 60, np.uint8)
        image[y:, x:] = 200  # one L corner at (x, y)
        return image
    for x, y, expected in ((16, 16, True), (15, 16, False), (16, 15, False), (47, 47, True), (48, 47, False)):
        image = square_at(x, y) if x < 32 else square_at(0, 0)
        if x >= 32:  # the corner near the far edges: the bright part is the top left
            image = np.full((64, 64), 60, np.uint8)
            image[:y + 1, :x + 1] = 200
        assert bool(FR.suppress(FR.fast_scores(image))[y, x]) == expected, (x, y)
    # two adjacent pixels of equal score: neither is strictly greater, both vanish
    scores = np.zeros((40, 40), np.int64)
    scores[20, 20] = scores[20, 21] = 50
    scores[10, 10] = 50
    out = FR.suppress(scores)
    assert out[20, 20] == 0 and out[20, 21] == 0 and out[10, 10] == 50


def test_selection_prefers_score_then_raster_order():
    scores = np.zeros((6, 8), np.int64)
    scores[1, 2], scores[1, 6], scores[3, 1], scores[4, 4], scores[5, 7] = 30, 40, 30, 30, 90
    assert list(FR.select(scores, 10)) == [10, 14, 25, 36, 47]
    assert list(FR.select(scores, 5)) == [10, 14, 25, 36, 47]
    assert list(FR.select(scores, 3)) == [10, 14, 47]  # of the three at 30 the first in raster order
    assert list(FR.select(scores, 4)) == [10, 14, 25, 47]
    assert list(FR.select(scores, 1)) == [47]


def _descriptor_at_centre(image):
    c = image.shape[0] // 2
    k = FR.direction_bin(*FR.moments(image, c, c))
    return k, FR.describe(FR.box_sums(image), c, c, k)


def _hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def test_descriptor_follows_a_turn_of_the_patch():
    """Observed on these seeds (profiles/r13_texture_detector.txt): the distances are printed, the assertion is the
    order alone -- a turned patch is nearer than an unrelated one"""
    size = 65
    turned_12, turned_90, unrelated = [], [], []
    for seed in range(8):
        patch = FS.texture(size, seed)
        k0, d0 = _descriptor_at_centre(patch)
        k12, d12 = _descriptor_at_centre(FS.turned(patch, 12.0))
        k90, d90 = _descriptor_at_centre(np.rot90(patch).copy())
        assert (k0 - k12) % 30 in (0, 1, 2) and (k0 - k90) % 30 in (7, 8)  # the direction went with the patch
        _, other = _descriptor_at_centre(FS.texture(size, 100 + seed))
        turned_12.append(_hamming(d0, d12))
        turned_90.append(_hamming(d0, d90))
        unrelated.append(_hamming(d0, other))
    print("hamming turned 12:", turned_12, "turned 90:", turned_90, "unrelated:", unrelated)
    assert max(turned_12) < min(unrelated) and max(turned_90) < min(unrelated)
    assert 96 <= np.mean(unrelated) <= 160  # about half of 256 bits
