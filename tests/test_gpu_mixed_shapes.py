"""The fused mixed-radix training path (k_pass_a_m and k_iso_norm_m with HIST, the column pass k_pass_b_m,
k_bwd_pass_a_m, k_bwd_iso_q_m) at every row plan in both shrink modes, every column plan, 1 and 2
iterations and strips of more than one row, against the fp64 oracle's autograd (solve_spatial, the
reference's op sequence).  The cases are tests/mixed_cases.py's; tests/test_train_case_inputs.py shows on
the CPU that each stays >= 1e-5 tau away from the kink of its shrink (soft threshold or block factor) and
that the reference op sequence in fp32 already meets the gates, so the gates here are fixed, as in test_gpu_train_shapes.py: relative L2,
training forward <= 1e-5; x, lambda, rho gradients <= 1e-4 without a PSF, <= 1e-3 with a (fixed) one.  No
max(..., floor) term, no near-kink exemption.  A lambda / rho reference gradient that is exactly 0 is
compared absolutely.

Strip heights.  strip_rows_mixed() gives R = 1 for all but the two tallest shapes here (the blocks fit one
round), so R is pinned in the A/B build (ADMM_MIXED_R; forward and backward inside _native.ab_library()).
Read from k_pass_a_m (HIST) and k_bwd_pass_a_m: a row's arithmetic does not depend on the strip it sits in
-- every row g is transformed from its own spectrum, differenced against row g - 1 and finalized from the
same operands in the same order whether row g - 1 is the strip's halo (recomputed) or its previous row, the
row after the strip's last is recomputed for the y differences alone and stores nothing, and k_iso_norm_m /
k_bwd_iso_q_m work per row -- so the output and the x gradient must be torch.equal between the R values, and
that is asserted (it held on an MI355X at every R of every case).  The lambda / rho gradients sum per-strip
fp64 partials, whose grouping follows R: <= 1e-5 (measured: equal after the rounding to fp32).

Every case prints its errors (pytest -s); the worst per group are recorded in DESIGN.md section 2."""
import pytest
import torch

import mixed_cases as mc
import train_cases as tc

pytestmark = pytest.mark.gpu


def descriptor(case):
    """The case's descriptor; the library must answer that it trains on the mixed kernels."""
    from admmtor import _native
    B, C, H, W = case.shape
    assert not case.learn_psf
    d = _native.desc(B, C, H, W, case.psf[1] if case.psf else 0, case.iso, case.maxit)
    assert _native.path(d, train=True) == "fused mixed-radix"
    return d


def hip_train(case, dev):
    """fft_admm_tv with x, lambda, rho requiring gradients (the PSF fixed), and its gradients against the
    case's cotangent: dict(out, gx, glam, grho) on the CPU."""
    from admmtor.eops.deconv import fft_admm_tv
    x, k = tc.inputs(case)
    xg = x.to(dev).requires_grad_(True)
    lam = torch.tensor([case.lam], device=dev, requires_grad=True)
    rho = torch.tensor([case.rho], device=dev, requires_grad=True)
    out = fft_admm_tv(xg, lam, rho, k.to(dev), case.iso, case.maxit)
    g = torch.autograd.grad(out, (xg, lam, rho), tc.cotangent(case).to(dev))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), gx=g[0].cpu(), glam=g[1].cpu(), grho=g[2].cpu())


# ------------------------------------------------------------------ row plans, column plans, maxit
@pytest.mark.parametrize("case", mc.TABLE_CASES, ids=str)
def test_mixed_training_vs_oracle(cuda_dev, case):
    descriptor(case)
    e = tc.errors(hip_train(case, cuda_dev), tc.reference(case))
    print(f"[{case.group}] {case.name} {case.shape} maxit {case.maxit}: {tc.fmt(e)}")
    tc.check_gates(case, e)


# ------------------------------------------------------------------ strip heights (A/B build)
_ab = {}


def ab_train(monkeypatch, case, R, dev):
    """The case solved and differentiated in the A/B build with strips of R rows (0: the rule), once."""
    from admmtor import _native
    if (case.name, R) not in _ab:
        monkeypatch.delenv("ADMM_MIXED", raising=False)
        if R:
            monkeypatch.setenv("ADMM_MIXED_R", str(R))
        else:
            monkeypatch.delenv("ADMM_MIXED_R", raising=False)
        with _native.ab_library():
            ws = _native.backward_workspace_size(descriptor(case))
            _ab[(case.name, R)] = (hip_train(case, dev), ws)
    return _ab[(case.name, R)]


@pytest.mark.parametrize("case,R", mc.STRIP_RUNS, ids=lambda v: str(v))
def test_strip_height_vs_oracle(cuda_dev, monkeypatch, case, R):
    got, _ = ab_train(monkeypatch, case, R, cuda_dev)
    e = tc.errors(got, tc.reference(case))
    print(f"[strip] {case.name} {case.shape} R = {R}: {tc.fmt(e)}")
    tc.check_gates(case, e)


@pytest.mark.parametrize("case,rows", mc.STRIP_CASES, ids=lambda v: str(v) if isinstance(v, tc.Case) else "")
def test_strip_heights_agree(cuda_dev, monkeypatch, case, rows):
    runs = [ab_train(monkeypatch, case, R, cuda_dev) for R in rows]
    # the knob took: the backward workspace holds maxit x nstrips fp64 partial pairs, fewer with taller
    # strips; and the rule's own choice for these shapes is R = 1
    sizes = [ws for _, ws in runs]
    assert all(a > b for a, b in zip(sizes, sizes[1:])), sizes
    assert rows[0] == 1 and ab_train(monkeypatch, case, 0, cuda_dev)[1] == sizes[0]
    base = runs[0][0]
    for R, (got, _) in zip(rows[1:], runs[1:]):
        el, er = tc.scalar_err(got["glam"], base["glam"]), tc.scalar_err(got["grho"], base["grho"])
        print(f"[strip] {case.name} R = {R} vs R = 1: out {tc.rel(got['out'], base['out']):.2e} "
              f"x^ {tc.rel(got['gx'], base['gx']):.2e} lambda^ {el:.2e} rho^ {er:.2e}")
        assert torch.equal(got["out"], base["out"])
        assert torch.equal(got["gx"], base["gx"])
        assert el <= 1e-5 and er <= 1e-5


def test_ab_build_equals_release(cuda_dev, monkeypatch):
    """With no knob set the A/B build is the release library: element for element, gradients included
    (a stale A/B library would make the strip-height cases above test old kernels)."""
    case = mc.STRIP_CASES[0][0]
    ab, _ = ab_train(monkeypatch, case, 0, cuda_dev)
    release = hip_train(case, cuda_dev)
    assert sorted(ab) == sorted(release)
    for key in release:
        assert torch.equal(ab[key], release[key]), key


# ------------------------------------------------------------------ the history row pass beside the inference one
def test_training_output_equals_inference(cuda_dev):
    """Training and inference take the same row plan (MPlan: the training plan at equal group width, for
    both) and the same strips.  k_pass_a_m's HIST variant keeps a_k and rebuilds u_k = a_k - S(a_k) from it
    with the operands the inference variant stored u_k from, so on an aniso solve the two outputs are
    equal bit for bit; both against the oracle."""
    from admmtor.eops.deconv import fft_admm_tv
    case = next(c for c, _ in mc.STRIP_CASES if not c.iso and c.psf is None)
    x, k = tc.inputs(case)
    train = hip_train(case, cuda_dev)["out"]
    infer = fft_admm_tv(x.to(cuda_dev), case.lam, case.rho, k.to(cuda_dev), case.iso, case.maxit).cpu()
    ref = tc.reference(case)["out"]
    et, ei = tc.rel(train, ref), tc.rel(infer, ref)
    print(f"[infer] {case.name}: training {et:.2e}, inference {ei:.2e} vs oracle; training vs inference "
          f"{tc.rel(train, infer):.2e}")
    assert et <= tc.GATE_FWD and ei <= tc.GATE_FWD
    assert torch.equal(train, infer)
