"""CPU check of the training shape matrices' inputs (tests/train_cases.py for the power-of-two backend,
tests/mixed_cases.py for the mixed-radix one), with the oracle alone.

tests/test_gpu_train_shapes.py and tests/test_gpu_mixed_shapes.py gate every case at fixed bounds with no
max(..., floor) term and no near-kink exemption.  That is legitimate only if, for every case, none left out:

  * aniso: the fp64 trajectory stays >= 1e-5 tau away from the soft threshold's kink on every plane
    (kink_margins), ten times the distance at which test_gpu_grad.py stops trusting an fp32 gradient;
  * between 5 % and 95 % of the difference pixels have an active shrink, so both branches of the
    shrink Jacobian run;
  * the reference op sequence (solve_spatial) run in fp32 already meets the gates against itself in
    fp64, with a factor 2 to spare: half a gate for the reference's own fp32 arithmetic leaves the
    other half to a kernel whose fp32 arithmetic is no worse.

The figures are printed (pytest -s)."""
import os
import re

import pytest
import torch

import mixed_cases as mc
import train_cases as tc


@pytest.mark.parametrize("case", tc.ALL_SOLVES + mc.ALL_SOLVES, ids=str)
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


@pytest.mark.parametrize("case", [c for c in mc.ALL_SOLVES if c.iso], ids=str)
def test_mixed_iso_case_stays_off_the_block_kink(case):
    """The mixed table's iso cases reach 10^5 ... 10^6 pixels at tau down to 0.04, where the block factor's
    switch at ||a|| = tau is crossed somewhere by an fp32 solve unless the fp64 trajectory keeps away from it:
    the aniso bound, on mixed_cases.iso_kink_margin."""
    margin = mc.iso_kink_margin(case)
    print(f"{case.name}: iso kink margin {margin:.2e}")
    assert margin >= tc.KINK_MARGIN


# ------------------------------------------------------------------ the mixed-radix backend's table
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "torch-admm-deconv_amd", "csrc")


def _dispatched(fn):
    """The lengths of with_row / with_col in mixed_capi.hip: every `case L:` of the function's switch."""
    text = open(os.path.join(CSRC, "mixed_capi.hip")).read()
    body = re.search(r"hipError_t %s\(int \w+, F&& f\) \{(.*?)\n\}" % fn, text, re.S).group(1)
    return {int(v) for v in re.findall(r"case (\d+):", body)}


def _bwd_lanes(N):
    """Lanes of the reverse row pass's row group (mixed_kernels.hpp BPlan, ADMM_TRAIN_BWD_PLAN = 3: the
    training plan unless it would widen the inference plan's group to 4 waves).  The power-of-two lengths have
    one plan, N / E lanes (fft_core.hpp RowCfg)."""
    from test_mixed_plans import ROWS, TRAIN_ROWS
    row = {n: int(v["Lg"]) for n, v, *_ in ROWS}
    if N not in row:
        e = re.search(r"RowCfg<%d> \{ static constexpr int E = (\d+)" % N, open(os.path.join(CSRC, "fft_core.hpp")).read())
        return N // int(e.group(1))
    a = row[N]
    b = {n: int(v["Lg"]) for n, v, *_ in TRAIN_ROWS}.get(N, a)
    return b if (b < 256 or a == 256) else a


def test_mixed_table_reaches_every_plan():
    """Every row length the mixed dispatcher has, in both shrink modes; every column length; 1 and 2 iterations
    on a narrow, a 2-wave and a 4-wave row plan; the strip heights, a partial last block and a wide group past
    the last strip.  A plan added to with_row / with_col fails here until it gets a case."""
    from admmtor import _native
    import test_gpu_mixed
    rows, cols = _dispatched("with_row"), _dispatched("with_col")
    assert len(rows) >= 20 and len(cols) >= 23
    solves = mc.ALL_SOLVES
    assert len({c.name for c in solves}) == len(solves)
    for c in solves:  # the library's own answer: trained on the mixed kernels
        B, C, H, W = c.shape
        assert not c.learn_psf and not isinstance(c.lam, tuple)
        assert _native.path(_native.desc(B, C, H, W, c.psf[1] if c.psf else 0, c.iso, c.maxit), train=True) \
            == "fused mixed-radix", c.name
    for iso in (False, True):
        assert {c.shape[3] // 2 for c in mc.WIDTH_CASES if c.iso == iso} == rows, iso
    with_psf = sum(c.psf is not None for c in mc.WIDTH_CASES) / len(mc.WIDTH_CASES)
    assert 0.25 <= with_psf <= 0.5
    # column lengths: all but the one mixed_cases.py leaves to the inference cases, which must have it
    trained = {c.shape[2] for c in solves}
    assert cols - trained == {4096}
    assert {shape[2] for shape, *_ in test_gpu_mixed.CASES} >= cols - trained
    # the plane-pair walk of the column pass (H >= 1024, under 8 columns a block) with a partial last group
    assert {c.shape[2] for c in mc.HEIGHT_CASES if c.shape[0] * c.shape[1] == 3} >= {1536, 2160, 2048}
    # maxit 1 and 2, aniso and iso, on a narrow, a 2-wave and a 4-wave reverse plan
    for lanes in (lambda l: l <= 64, lambda l: l == 128, lambda l: l == 256):
        got = {(c.iso, c.maxit) for c in mc.MAXIT_CASES if lanes(_bwd_lanes(c.shape[3] // 2))}
        assert got == {(i, k) for i in (False, True) for k in (1, 2)}
    # strip heights
    tall = [(c, rs) for c, rs in mc.STRIP_CASES if c.shape[2] == 240]
    wide = [(c, rs) for c, rs in mc.STRIP_CASES if c.shape[2] in (16, 32)]
    assert {c.shape[3] for c, _ in tall} == {32, 64} and {c.iso for c, _ in tall} == {False, True}
    assert all(set(rs) >= {1, 2, 3, 5, 8, 15, 16, 30} for _, rs in tall)
    assert all(set(rs) >= {1, 2, 4, 8, 16} for _, rs in wide)
    assert {(_bwd_lanes(c.shape[3] // 2), c.iso) for c, _ in wide} == {(l, i) for l in (128, 256) for i in (False, True)}
    assert any(c.psf for c, _ in mc.STRIP_CASES)
    assert all(c.shape[0] * c.shape[1] == 3 for c, _ in mc.STRIP_CASES)
    partial = odd_wide = False
    for c, rs in mc.STRIP_CASES:
        B, C, H, W = c.shape
        lanes = _bwd_lanes(W // 2)
        sizes = []
        for R in rs:
            assert H % R == 0, (c.name, R)  # the knob is ignored otherwise
            strips = B * C * H // R
            sizes.append(-(-c.maxit * strips * 16 // 256) * 256)  # the fp64 partial pairs, 256-byte aligned
            partial |= lanes <= 64 and strips % (256 // lanes) != 0
            odd_wide |= lanes == 128 and strips % 2 == 1
        # ... so that the GPU test can tell from the backward workspace that the knob took
        assert all(a > b for a, b in zip(sizes, sizes[1:])), (c.name, sizes)
    assert partial and odd_wide
