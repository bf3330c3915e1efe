"""The routes of the backward-route cases (tests/backward_cases.py), pinned on filter descriptions: no tensor, no device.  A change to a
gate of ops._route / ops._wgrad_route shows up here as the row whose route moved -- without this the GPU cases of
tests/test_gpu_backward_routes.py would quietly end up on another kernel."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_cases as BC  # noqa: E402


@pytest.mark.parametrize("case", BC.CASES, ids=BC.case_id)
def test_case_takes_its_routes_in_every_mode(case):
    from rendernet_amd import ops
    row, want = case
    for mode in BC.MODES:
        with ops.gemm_mode(mode):
            assert BC.routes_of(ops, row) == want[mode], (BC.case_id(case), mode)


@pytest.mark.parametrize("case", BC.BLOCK_CASES, ids=BC.block_id)
def test_res_block_input_gradient_route(case):
    """The route of conv1's input-gradient launch decides how the carried skip gradient is added: in the launch's residual epilogue
    (ops.CARRY_IN_EPILOGUE) or by one add_ afterwards."""
    from rendernet_amd import ops
    block, want = case
    for mode in BC.MODES:
        with ops.gemm_mode(mode):
            r = BC.block_dgrad_route(ops, block)
        assert BC.route_name(r) == want[mode], (BC.block_id(case), mode)
        assert (r.name in ops.CARRY_IN_EPILOGUE) == (want[mode] != "direct")
    assert {w.split(":")[0] for _, want in BC.BLOCK_CASES for w in want.values()} == set(ops.CARRY_IN_EPILOGUE) | {"direct"}


def test_the_table_reaches_every_route():
    """Every forward / input-gradient route of ops._route and every filter-gradient route of ops._wgrad_route is taken by some row in
    some mode, with every scheme of the three-launch path."""
    fwd, dgrad, wgrad = set(), set(), set()
    for _row, want in BC.CASES:
        for mode in BC.MODES:
            f, d, w = want[mode].split()
            fwd.add(f), dgrad.add(d), wgrad.add(w)
    routes = {"direct", "wino2", "wino4", "wino3d", "split3d", "split11:f11", "wino3l:f43", "wino3l:f63", "wino3l:f44"}
    assert fwd == routes | {"convt_s2_wino"} and dgrad == routes
    assert wgrad == {"direct", "wino2", "wino43", "wino44", "wino3l_split", "split3d"}
    epilogues = [row[7] for row, _ in BC.CASES]
    assert epilogues.count("elu") == 2 and all(e in ("prelu", "res", "elu") for e in epilogues)
    assert all(row[1] == 2 for row, _ in BC.CASES)
