"""tests/texture_l2_reference.py against independent formulations: exact f64 arithmetic in any order for integer-valued
descriptors, the tie rule on two sums that round to one distance, NaN, 0 / 0 and a ratio exactly at the threshold; and
that the fixed order of the sum matters on the non-integer inputs the GPU test uses."""
import numpy as np

import texture_l2_reference as L

F = np.float32


def test_integer_valued_descriptors_equal_exact_arithmetic_in_any_order():
    rng = np.random.default_rng(1)
    queries, train = L.seeded_rows(rng, 6, 128, True), L.seeded_rows(rng, 9, 128, True)
    queries[0], train[0] = 0.0, 255.0  # the largest sum there is: 128 * 255^2
    for q in queries:
        for t in train:
            e = q.astype(np.float64) - t.astype(np.float64)
            exact = (e * e).sum()
            assert exact <= 128 * 255 ** 2 < 2 ** 24
            assert (e[::-1] * e[::-1]).sum() == exact == np.sum(rng.permutation(e) ** 2)
            s = L.l2_squared(q, t)
            assert np.float64(s) == exact
            assert L.l2_distance(q, t).tobytes() == F(np.sqrt(exact)).tobytes()  # (f64 root of an f32 value, rounded once more:
            # innocuous double rounding for sqrt; and numpy's float32 root beside it)
        assert np.array_equal(L.l2_squared_rows(q, train), np.array([L.l2_squared(q, t) for t in train], F))
    assert np.float64(L.l2_squared(queries[0], train[0])) == 128 * 255 ** 2


def test_rows_at_once_equal_the_scalar_loop_on_floats():
    rng = np.random.default_rng(2)
    queries, train = L.seeded_rows(rng, 4, 200, False), L.seeded_rows(rng, 7, 200, False)
    for q in queries:
        rows = L.l2_squared_rows(q, train)
        assert rows.tobytes() == np.array([L.l2_squared(q, t) for t in train], F).tobytes()


def test_the_lower_index_wins_where_two_sums_round_to_one_distance():
    query = np.zeros((1, 4), F)
    train = np.array([[2000, 2000, 1, 0], [2000, 2000, 0, 0], [3000, 0, 0, 0]], F)
    s = [L.l2_squared(query[0], t) for t in train]
    assert (s[0], s[1]) == (8000001.0, 8000000.0)  # different sums, the later one smaller ...
    assert L.l2_distance(query[0], train[0]).tobytes() == L.l2_distance(query[0], train[1]).tobytes()  # ... one distance
    assert L.knn_match2_l2_sequential(query, train) == [(np.sqrt(F(8000001.0)), np.sqrt(F(8000000.0)), 0)]
    # a comparison of the sums would have ranked index 1 first
    assert int(np.argmin(s)) == 1
    # plain duplicates: the first of them; and the same with the rows the other way round
    assert L.knn_match2_l2_sequential(query, train[[2, 1, 1]])[0][2] == 1
    assert L.knn_match2_l2_sequential(query, train[[1, 0, 2]])[0][2] == 0


def test_nan_never_enters_and_infinity_is_a_distance():
    query = np.zeros((1, 4), F)
    nan_row = np.array([np.nan, 0, 0, 0], F)
    train = np.array([nan_row, [3, 0, 0, 0], nan_row, [4, 0, 0, 0], nan_row], F)
    assert L.knn_match2_l2_sequential(query, train) == [(F(3.0), F(4.0), 1)]
    assert L.knn_match2_l2_sequential(query, train[:3]) == [None]  # one entry only: no match
    assert L.knn_match2_l2_sequential(query, train[:1]) == [None] and L.knn_match2_l2_sequential(query, train[:0]) == [None]
    huge = np.full((2, 4), 3e38, F)  # the sum overflows: +inf, a distance like any other
    assert L.knn_match2_l2_sequential(query, huge) == [(F(np.inf), F(np.inf), 0)]
    assert L.ratio_keeps_l2(F(np.inf), F(np.inf), 0.7)  # inf / inf: NaN, kept


def test_ratio_test_at_zero_over_zero_and_exactly_at_the_threshold():
    assert L.ratio_keeps_l2(F(0.0), F(0.0), 0.7)  # 0 / 0: NaN, kept
    assert not L.ratio_keeps_l2(F(3.0), F(4.0), 0.75)  # exactly the threshold: dropped
    assert L.ratio_keeps_l2(np.nextafter(F(3.0), F(0.0)), F(4.0), 0.75)
    assert not L.ratio_keeps_l2(F(1.0), F(0.0), 0.75)  # x / 0 = inf
    # the threshold is compared in f32: 0.7 is not a float
    assert not L.ratio_keeps_l2(F(0.7) * F(8.0), F(8.0), 0.7) and L.ratio_keeps_l2(np.nextafter(F(0.7), F(0)) * F(8.0), F(8.0), 0.7)


def test_the_order_of_the_sum_matters_on_the_gpu_tests_inputs():
    """on uniform floats (D = 200, seed 5: the inputs of tests/test_gpu_texture_l2.py) the sequential sum and numpy's
    pairwise one differ for many pairs: a kernel that sums in another order does not pass by accident"""
    rng = np.random.default_rng(5)
    queries, train = L.seeded_rows(rng, 8, 200, False), L.seeded_rows(rng, 8, 200, False)
    differ = 0
    for q in queries:
        for t in train:
            e = q - t
            differ += L.l2_squared(q, t).tobytes() != np.sum(e * e, dtype=F).tobytes()
    assert differ >= 1, differ
