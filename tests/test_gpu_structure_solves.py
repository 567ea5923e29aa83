"""The structure solve alone on the device (m3t_links.hip: links_solve_sums_kernel, links_project_kernel + links_solve_kernel,
ldlt_solve_any and the three routines behind it) against the oracle, at the sizes, joint shapes, constraint rows and
degenerate pivots of tests/structure_edges.py, SOLVE_CASES: no images -- the stacked link sums CalculateOptimizationBegin
hands out are overwritten with the case's seeded sums on both sides, CalculateOptimizationEnd solves, and after each of
three rounds link2world, joint2parent and body2joint of every link are np.array_equal.  There is no tolerance in this
module.  tests/test_structure_edge_cases.py shows on the CPU that every case is live and checks the oracle itself
against float64."""
import ctypes as C

import numpy as np
import pytest

import structure_edges as se
import util

pytestmark = pytest.mark.gpu

_oracle = {}  # case id -> SolveRun of the oracle, computed once


def _reference(case):
    if case.id not in _oracle:
        _oracle[case.id] = se.solve_run(util.open_oracle(), case)
    return _oracle[case.id]


def _device_writer(api):
    import torch

    def write(ptr, n, data):
        api.call("sync")  # (the launch that formed the sums has finished)
        addr = C.cast(ptr, C.c_void_p).value

        class _Buf:  # zero-copy view of the library's device buffer
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (addr, False), "version": 2}
        torch.as_tensor(_Buf(), device="cuda").copy_(torch.from_numpy(data))
        torch.cuda.synchronize()
    return write


@pytest.mark.parametrize("case", se.SOLVE_CASES, ids=repr)
def test_structure_solve_equals_the_oracle(case):
    ref = _reference(case)
    api = util.open_hip()
    got = se.solve_run(api, case, write=_device_writer(api))
    for k in range(len(case.structures)):
        assert np.array_equal(got.start[k], ref.start[k]), k
        for r in range(case.ROUNDS):
            assert np.array_equal(got.states[r][k], ref.states[r][k]), (k, r)
        if not case.moves[k]:  # (a NaN in the sums, an all-zero system: the poses stay bit for bit)
            assert all(np.array_equal(s[k], got.start[k]) for s in got.states), k
        else:
            assert not np.array_equal(got.states[-1][k], got.start[k]), k
