"""Training with a learnable PSF at smooth sizes on the fused mixed-radix kernels: the forward that keeps
every r_k's packed row spectra in the history (k_pass_b_m out of place, the row pass writing r_{k+1} into the
history) and the backward's PSF gradient (k_xspec_m, then k_xspec_reduce and k_psf_grad as on the
power-of-two path), against the fp64 oracle's autograd (solve_spatial, the reference's op sequence).  The
cases are tests/mixed_psf_cases.py's; tests/test_mixed_psf_case_inputs.py shows on the CPU that each is fit
for fixed gates, so the gates here are the project's fixed ones: relative L2, training forward <= 1e-5,
every gradient -- x, lambda, rho and the PSF -- <= 1e-3.  No max(..., floor) term, no near-kink exemption.  A
lambda / rho reference gradient that is exactly 0 (one iteration, or tau above every |a|) is compared
absolutely.

Every case prints its errors and, beside them, the same step's errors on the generic kernels (the A/B build
with ADMM_MIXED=0: where this training ran before; printed, never gated).  pytest -s shows them; the worst
per group are recorded in DESIGN.md section 2."""
import pytest
import torch

import mixed_psf_cases as pc
import train_cases as tc

pytestmark = pytest.mark.gpu


def descriptor(case, learn=True):
    from admmtor import _native
    B, C, H, W = case.shape
    return _native.desc(B, C, H, W, case.psf[1], case.iso, case.maxit,
                        flags=_native.ADMM_TV_FLAG_PSF_GRAD if learn else 0)


def hip_train(case, dev, learn=True):
    """fft_admm_tv with x, lambda, rho (and, learn, the PSF) requiring gradients, and its gradients against
    the case's cotangent: dict(out, gx, glam, grho[, gk]) on the CPU."""
    from admmtor.eops.deconv import fft_admm_tv
    x, k = tc.inputs(case)
    xg = x.to(dev).requires_grad_(True)
    lam = torch.tensor([case.lam], device=dev, requires_grad=True)
    rho = torch.tensor([case.rho], device=dev, requires_grad=True)
    kg = k.detach().to(dev).requires_grad_(learn)
    out = fft_admm_tv(xg, lam, rho, kg, case.iso, case.maxit)
    g = torch.autograd.grad(out, (xg, lam, rho) + ((kg,) if learn else ()), tc.cotangent(case).to(dev))
    torch.cuda.synchronize()
    got = dict(out=out.detach().cpu(), gx=g[0].cpu(), glam=g[1].cpu(), grho=g[2].cpu())
    if learn:
        got["gk"] = g[3].cpu()
    return got


def generic_train(monkeypatch, case, dev):
    """The same step in the A/B build with the mixed path switched off: the generic kernels."""
    from admmtor import _native
    monkeypatch.setenv("ADMM_MIXED", "0")
    with _native.ab_library():
        assert _native.path(descriptor(case), train=True) == "generic"
        return hip_train(case, dev)


@pytest.mark.parametrize("case", pc.TABLE_CASES, ids=str)
def test_learnable_psf_training_vs_oracle(cuda_dev, monkeypatch, case):
    from admmtor import _native
    assert _native.path(descriptor(case), train=True) == "fused mixed-radix"
    ref = tc.reference(case)
    e = tc.errors(hip_train(case, cuda_dev), ref)
    print(f"[{case.group}] {case.name} {case.shape} maxit {case.maxit}: {tc.fmt(e)}")
    print(f"    generic kernels (ADMM_MIXED=0): {tc.fmt(tc.errors(generic_train(monkeypatch, case, cuda_dev), ref))}")
    assert "gk" in e
    tc.check_gates(case, e)


@pytest.mark.parametrize("name", ["p-h540-aniso-motion5", "p-n960-iso-motion5"])
def test_learnable_psf_changes_no_other_result(cuda_dev, name):
    """The out-of-place column pass computes what the in-place one does, operand for operand, and the kept
    row spectra are extra stores; the backward's cross spectra only read.  So the output, x^, lambda^ and rho^
    of a step with a learnable PSF equal those of the same step with the PSF fixed, bit for bit."""
    case = next(c for c in pc.TABLE_CASES if c.name == name)
    learn, fixed = hip_train(case, cuda_dev), hip_train(case, cuda_dev, learn=False)
    for key in ("out", "gx", "glam", "grho"):
        assert torch.equal(learn[key], fixed[key]), (case.name, key, tc.rel(learn[key], fixed[key]))


def test_training_output_equals_inference(cuda_dev):
    """The aniso training forward with a learnable PSF gives the inference solve's output bit for bit (as
    test_gpu_mixed_shapes.py shows for the forward without kept spectra)."""
    from admmtor.eops.deconv import fft_admm_tv
    case = next(c for c in pc.TABLE_CASES if c.name == "p-h540-aniso-motion5")
    x, k = tc.inputs(case)
    train = hip_train(case, cuda_dev)["out"]
    infer = fft_admm_tv(x.to(cuda_dev), case.lam, case.rho, k.to(cuda_dev), case.iso, case.maxit).cpu()
    assert tc.rel(infer, tc.reference(case)["out"]) <= tc.GATE_FWD
    assert torch.equal(train, infer)


def test_admmdeconv_module_trains_its_psf(cuda_dev):
    """ADMMDeconv((5, 5), max_iters=6, iso=True) at 240 x 480: w, lmbda and rho are nn.Parameters, so its
    training step asks for every gradient; all four against the oracle, on the mixed kernels."""
    from admmtor import _native
    from admmtor.elayers.admmdeconv import ADMMDeconv
    case = pc.MODULE_CASE
    x, k = tc.inputs(case)
    m = ADMMDeconv((5, 5), max_iters=case.maxit, iso=True)
    assert all(isinstance(p, torch.nn.Parameter) for p in (m.w, m.lmbda, m.rho))
    with torch.no_grad():
        m.w.copy_(k.reshape(m.w.shape))
        m.lmbda.fill_(case.lam)
        m.rho.fill_(case.rho)
    m = m.to(cuda_dev)
    assert _native.path(descriptor(case), train=True) == "fused mixed-radix"
    xg = x.to(cuda_dev).requires_grad_(True)
    out = m(xg)
    (out * tc.cotangent(case).to(cuda_dev)).sum().backward()
    torch.cuda.synchronize()
    got = dict(out=out.detach().cpu(), gx=xg.grad.cpu(), glam=m.lmbda.grad.cpu(), grho=m.rho.grad.cpu(),
               gk=m.w.grad.cpu())
    assert got["gk"].shape == m.w.shape
    e = tc.errors(got, tc.reference(case))
    print(f"[module] ADMMDeconv((5, 5), 6, iso) {case.shape}: {tc.fmt(e)}")
    tc.check_gates(case, e)


@pytest.mark.parametrize("iso", [False, True])
def test_opcheck_at_a_smooth_size_with_a_learnable_psf(cuda_dev, iso):
    """The fake kernels size the history from the same native query as the real ones: with the PSF-gradient
    flag at a smooth size that is one packed row-spectrum set per iteration."""
    import admmtor._ops  # noqa: F401
    from admmtor.synth import blurred_batch, make_psf
    k = make_psf("motion", 5)
    x = blurred_batch(1, 2, 16, 480, k, seed=5).to(cuda_dev).requires_grad_(True)
    k = k.to(cuda_dev).requires_grad_(True)
    lam = torch.tensor([0.02], device=cuda_dev, requires_grad=True)
    rho = torch.tensor([0.2], device=cuda_dev, requires_grad=True)
    torch.library.opcheck(torch.ops.admm_hip.fft_admm_tv_fwd_train.default, (x, lam, rho, k, iso, 3, True),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor",
                                      "test_aot_dispatch_static"))
    out, hist = torch.ops.admm_hip.fft_admm_tv_fwd_train(x.detach(), lam.detach(), rho.detach(), k.detach(), iso, 3, True)
    torch.library.opcheck(torch.ops.admm_hip.fft_admm_tv_bwd.default,
                          (torch.randn_like(out), x.detach(), lam.detach(), rho.detach(), k.detach(), hist, iso, 3, True,
                           True, True, True))
