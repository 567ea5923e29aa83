"""The L2 matcher's arithmetic that host and device share (3dobjecttracking_amd/csrc/m3t_texture.h) on the host:
tests/cpp/texture_l2_check.cpp runs it on vectors written here and compares bits with tests/texture_l2_reference.py --
sums, distances, the best two (plainly, through the shortcut on the sums, and joined from four ranges as the kernel
joins them) and the ratio test; integer-valued and float descriptors, duplicates, the two sums of one distance, NaN and
overflowing rows, all-equal rows, a ratio at the threshold, and 0, 1 and 2 train rows."""
import os
import re
import subprocess

import numpy as np
import pytest

import texture_l2_reference as L
import util

F = np.float32
SRC = os.path.join(util.ROOT, "tests", "cpp", "texture_l2_check.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]


def _cases():
    rng = np.random.default_rng(11)
    cases = []
    for n_floats, integer, n_query, n_train in ((128, True, 5, 70), (200, False, 4, 33), (4, False, 6, 9),
                                                (256, False, 3, 8), (128, True, 3, 0), (128, True, 3, 1), (8, False, 3, 2)):
        queries, train = L.seeded_rows(rng, n_query, n_floats, integer), L.seeded_rows(rng, n_train, n_floats, integer)
        if n_train >= 33:  # duplicates across the ranges the kernel splits the train rows into; a query equal to both
            train[30] = train[5]
            queries[1] = train[5]
        cases.append((queries, train, 0.7))
    tie = np.array([[2000, 2000, 1, 0], [2000, 2000, 0, 0], [2000, 2000, 1, 0], [3000, 0, 0, 0]], F)
    cases.append((np.zeros((1, 4), F), tie, 0.7))
    cases.append((np.zeros((1, 4), F), tie[::-1].copy(), 0.7))
    nan_row = np.array([np.nan, 1, 2, 3], F)
    special = np.array([nan_row, [3, 0, 0, 0], nan_row, [3e38, 3e38, 0, 0], [4, 0, 0, 0], [0, 0, 0, 0]], F)
    cases.append((np.zeros((2, 4), F), special, 0.75))
    cases.append((np.zeros((1, 4), F), special[[0, 1, 2]], 0.75))          # one entry beside NaN rows: no match
    cases.append((np.zeros((1, 4), F), special[[1, 4]], 0.75))              # 3 / 4: exactly the threshold
    cases.append((np.zeros((1, 4), F), special[[3, 3]], 0.75))              # inf / inf
    cases.append((np.ones((3, 8), F), np.ones((5, 8), F), 0.7))             # all equal: 0 / 0
    return cases


def _write(path):
    words = [np.array([len(_cases())], np.int32).tobytes()]
    expected_kept = []
    for queries, train, threshold in _cases():
        words.append(np.array([len(queries), len(train), queries.shape[1]], np.int32).tobytes())
        words.append(F(threshold).tobytes() + queries.tobytes() + train.tobytes())
        sums = np.array([L.l2_squared_rows(q, train) for q in queries], F).reshape(len(queries), len(train))
        for q in range(min(len(queries), 2)):  # (the rows-at-once form against the scalar loop)
            assert sums[q].tobytes() == np.array([L.l2_squared(queries[q], t) for t in train], F).tobytes()
        with np.errstate(invalid="ignore"):
            words.append(sums.tobytes() + np.sqrt(sums).tobytes())
        for best in L.knn_match2_l2_sequential(queries, train):
            if best is None:
                words.append(np.array([0, 0, -1, 0], np.int32).tobytes())
                expected_kept.append(False)
            else:
                kept = L.ratio_keeps_l2(best[0], best[1], threshold)
                words.append(F(best[0]).tobytes() + F(best[1]).tobytes() + np.array([best[2], kept], np.int32).tobytes())
                expected_kept.append(kept)
    assert True in expected_kept and False in expected_kept
    with open(path, "wb") as f:
        f.write(b"".join(words))


def _check(exe, vectors):
    out = subprocess.run([exe, vectors], capture_output=True, text=True, timeout=60)
    m = re.search(r"^checks (\d+) errors (\d+)$", out.stdout, re.M)
    assert m and out.returncode == 0, out.stdout + out.stderr
    assert int(m.group(2)) == 0 and int(m.group(1)) >= 1000
    assert out.stderr == ""


def test_shared_l2_arithmetic_equals_the_restatement(tmp_path):
    vectors = str(tmp_path / "vectors.bin")
    _write(vectors)
    path = str(tmp_path / "texture_l2_check")
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", path, SRC], check=True)
    _check(path, vectors)


def test_shared_l2_arithmetic_under_address_and_undefined_sanitizers(tmp_path):
    """the same stand-alone program, instrumented (needs the host compiler's sanitizer runtimes)"""
    have = [subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()
            for lib in ("libasan.so", "libubsan.so")]
    if not all(os.path.isabs(p) for p in have):
        pytest.skip("the host compiler's sanitizer runtimes are not installed")
    vectors = str(tmp_path / "vectors.bin")
    _write(vectors)
    path = str(tmp_path / "texture_l2_check_san")
    subprocess.run(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                                                    path, SRC], check=True)
    _check(path, vectors)
