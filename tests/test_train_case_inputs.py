"""CPU check of the training shape matrix's inputs (tests/train_cases.py), with the oracle alone.

tests/test_gpu_train_shapes.py gates every case at fixed bounds with no max(..., floor) term and no
near-kink exemption.  That is legitimate only if, for every case, none left out:

  * aniso: the fp64 trajectory stays >= 1e-5 tau away from the soft threshold's kink on every plane
    (kink_margins), ten times the distance at which test_gpu_grad.py stops trusting an fp32 gradient;
  * between 5 % and 95 % of the difference pixels have an active shrink, so both branches of the
    shrink Jacobian run;
  * the reference op sequence (solve_spatial) run in fp32 already meets the gates against itself in
    fp64, with a factor 2 to spare: half a gate for the reference's own fp32 arithmetic leaves the
    other half to a kernel whose fp32 arithmetic is no worse.

The figures are printed (pytest -s)."""
import pytest
import torch

import train_cases as tc


@pytest.mark.parametrize("case", tc.ALL_SOLVES, ids=str)
def test_case_is_fit_for_fixed_gates(case):
    from oracle.admm_oracle import kink_margins
    x, k = tc.inputs(case)
    share = tc.active_share(case)
    if case.iso:
        margin = float("inf")
    else:
        margin = kink_margins(x, case.lam, case.rho, k, case.maxit).min().item()
    ref = tc.reference(case)
    floor = tc.errors(tc.oracle_grads(case, torch.float32), ref)
    print(f"{case.name}: kink margin {margin:.2e}, active share {100 * share:.1f} %, fp32 floor {tc.fmt(floor)}")
    assert margin >= tc.KINK_MARGIN
    assert tc.ACTIVE_SHARE[0] <= share <= tc.ACTIVE_SHARE[1]
    assert floor["out"] <= tc.GATE_FWD / 2
    assert all(floor[key] <= case.gate / 2 for key in floor if key != "out"), floor


def test_table_reaches_every_instantiation():
    """The matrix's reason to exist: every row width N, column height H, strip height R and iteration count
    the fused training path has untested instantiations for."""
    solves = tc.TABLE_CASES + tc.STRIP_CASES + tc.GROUPED_CASES
    assert {c.shape[3] // 2 for c in solves} >= {8, 128, 512, 1024}
    assert {c.shape[2] for c in solves} >= {16, 256, 1024, 2048, 4096}
    assert {c.shape[2] for c in solves if c.learn_psf} >= {16, 256, 2048, 4096}  # pass_b out of place, xspec_h
    assert {c.maxit for c in tc.MAXIT_CASES} == {1, 2}
    assert all(R <= c.shape[2] for c in tc.STRIP_CASES for R in tc.STRIP_ROWS)
    assert len({c.name for c in solves}) == len(solves)
    for c in tc.GROUPED_CASES:  # modules change inside a block of 64 two-row strips (row kernels of N <= 16)
        strips_per_module = c.shape[0] * c.shape[1] * c.shape[2] // 2
        assert c.shape[3] // 2 <= 16 and strips_per_module % 64 != 0 and len(c.lam) == 3
