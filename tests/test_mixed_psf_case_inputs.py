"""CPU check of tests/mixed_psf_cases.py (the smooth-size training matrix with a learnable PSF), with the
oracle alone, and the host-side answers of the library for it.

tests/test_gpu_mixed_psf.py gates every case at fixed bounds -- output <= 1e-5, every gradient, the PSF's
included, <= 1e-3 -- with no floor term and no near-kink exemption.  As for the tables of
test_train_case_inputs.py that is legitimate only if, for every case, none left out:

  * the fp64 trajectory stays >= 1e-5 tau away from the kink of its shrink (aniso: kink_margins; iso:
    mixed_cases.iso_kink_margin);
  * between 5 % and 95 % of the difference pixels have an active shrink -- except the cases the table marks
    kink-free (mixed_psf_cases.KINK_FREE: one iteration, or tau above every |a|), where no such case exists;
  * the reference op sequence (solve_spatial) in fp32 meets half of each gate against itself in fp64.

The figures are printed (pytest -s)."""
import os
import re

import pytest
import torch

import mixed_cases as mc
import mixed_psf_cases as pc
import train_cases as tc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "torch-admm-deconv_amd", "csrc")


def fitness(case):
    """(kink margin, active share, fp32 floor errors) of a case, from the oracle."""
    from oracle.admm_oracle import kink_margins
    x, k = tc.inputs(case)
    if case.iso:
        margin = mc.iso_kink_margin(case)
    else:
        margin = kink_margins(x, case.lam, case.rho, k, case.maxit).min().item()
    share = tc.active_share(case)
    ref = tc.reference(case)
    # oracle_grads in fp32 marks its inputs themselves as requiring grad (Tensor.to returns the tensor where the
    # dtype already matches), and the inputs are shared with the fixed-PSF cases of the other tables: the
    # fp32 evaluation gets copies
    key = (case.shape, case.psf, case.seed)
    tc._inputs[key] = (x.clone(), k.clone())
    try:
        floor = tc.errors(tc.oracle_grads(case, torch.float32), ref)
    finally:
        tc._inputs[key] = (x, k)
    return margin, share, floor


@pytest.mark.parametrize("case", pc.TABLE_CASES, ids=str)
def test_case_is_fit_for_fixed_gates(case):
    assert case.learn_psf and case.psf is not None and case.gate == tc.GATE_GRAD_PSF
    margin, share, floor = fitness(case)
    free = case.name in pc.KINK_FREE
    print(f"{case.name}: kink margin {margin:.2e}, active share {100 * share:.1f} %"
          f"{' (kink-free case)' if free else ''}, fp32 floor {tc.fmt(floor)}")
    assert "gk" in floor
    assert margin >= tc.KINK_MARGIN
    if not free:
        assert tc.ACTIVE_SHARE[0] <= share <= tc.ACTIVE_SHARE[1]
    assert floor["out"] <= tc.GATE_FWD / 2
    assert all(floor[key] <= case.gate / 2 for key in floor if key != "out"), floor


def test_kink_free_cases_are_the_marked_ones():
    """Only the heights from 512 on beside W = 480 come without an active shrink, and they are of the two
    kinds: one iteration, or three with tau above the defaults' 0.1 by a factor of ten or more."""
    marked = [c for c in pc.TABLE_CASES if c.name in pc.KINK_FREE]
    assert {c.shape[2] for c in marked} == {512, 1024, 2048, 4096}
    assert all(c.shape[3] == 480 and c.group == "height" for c in marked)
    assert all(c.maxit == 1 or (c.maxit == 3 and c.lam / c.rho >= 1.0) for c in marked)
    assert {c.maxit for c in marked} == {1, 3}
    assert not any(c.shape[2] >= 512 and c.shape[3] == 480 for c in pc.TABLE_CASES if c.name not in pc.KINK_FREE)


def _dispatched(fn):
    """The lengths of with_row / with_col in mixed_capi.hip: every `case L:` of the function's switch."""
    text = open(os.path.join(CSRC, "mixed_capi.hip")).read()
    body = re.search(r"hipError_t %s\(int \w+, F&& f\) \{(.*?)\n\}" % fn, text, re.S).group(1)
    return {int(v) for v in re.findall(r"case (\d+):", body)}


def test_table_reaches_every_column_plan():
    """Every column length of with_col (a plan added later fails here until it gets a case), the row plans
    whose row pass writes the history, 1 and 2 iterations, a partial last plane group of the cross spectra and
    the 4-column instances of an 8-column plan."""
    rows, cols = _dispatched("with_row"), _dispatched("with_col")
    assert len(cols) >= 23
    assert len({c.name for c in pc.TABLE_CASES}) == len(pc.TABLE_CASES)
    assert {c.shape[2] for c in pc.HEIGHT_CASES} == cols
    assert all(c.shape[3] in (32, 64) or c.shape[3] == 480 for c in pc.HEIGHT_CASES)
    wide = [c for c in pc.TABLE_CASES if c.group in ("width", "height") and c.shape[2] == 16]
    assert {(c.shape[3] // 2, c.iso) for c in wide} >= {(n, i) for n in (240, 960, 800) for i in (False, True)}
    assert {(c.shape[3] // 2, c.maxit) for c in pc.MAXIT_CASES} == {(n, k) for n in (240, 960) for k in (1, 2)}
    assert any(c.shape[0] * c.shape[1] >= 9 and c.shape[0] * c.shape[1] % 8 != 0 for c in pc.PLANE_CASES)
    # with_row's lengths are multiples of 4, and 540 alone is no multiple of 8
    assert all(n % 4 == 0 for n in rows) and {n for n in rows if n % 8} == {540}
    assert {c.shape[3] // 2 for c in pc.CC_CASES} == {540} and {c.iso for c in pc.CC_CASES} == {False, True}


# ------------------------------------------------------------------ the library's host-side answers
def _desc(case, flags):
    from admmtor import _native
    B, C, H, W = case.shape
    return _native.desc(B, C, H, W, case.psf[1], case.iso, case.maxit, flags=flags)


@pytest.mark.parametrize("case", pc.TABLE_CASES, ids=str)
def test_learnable_psf_trains_on_the_mixed_kernels(case):
    from admmtor import _native
    assert _native.supported(case.shape[2], case.shape[3])
    assert _native.path(_desc(case, _native.ADMM_TV_FLAG_PSF_GRAD), train=True) == "fused mixed-radix", case.name
    assert _native.path(_desc(case, 0), train=True) == "fused mixed-radix", case.name


@pytest.mark.parametrize("shape", [(1, 3, 240, 480), (2, 3, 1080, 1920)], ids=str)
@pytest.mark.parametrize("maxit", [1, 6])
def test_history_keeps_one_row_spectrum_set_per_iteration(shape, maxit):
    """With ADMM_TV_FLAG_PSF_GRAD the history holds every r_k's packed row spectra besides a_k (and N_k): one
    image-sized slot per iteration (B C H (W / 2) complex values, rounded up to 256 bytes), not the generic
    path's H (W / 2 + 1) half spectra."""
    from admmtor import _native
    B, C, H, W = shape
    slot = -(-B * C * H * (W // 2) * 8 // 256) * 256
    for iso in (False, True):
        plain = _native.history_size(_native.desc(B, C, H, W, 5, iso, maxit))
        kept = _native.history_size(_native.desc(B, C, H, W, 5, iso, maxit, flags=_native.ADMM_TV_FLAG_PSF_GRAD))
        assert kept - plain == maxit * slot, (shape, iso, kept - plain, maxit * slot)


def test_grouped_modules_with_a_psf_gradient_stay_unsupported():
    from admmtor import _native
    d = _native.desc(1, 3, 240, 480, 5, False, 4, flags=_native.ADMM_TV_FLAG_PSF_GRAD, groups=2)
    with pytest.raises(_native.NativeError) as err:
        _native.path(d, train=True)
    assert err.value.code == _native.ADMM_TV_EUNSUPPORTED
