"""Training with a PSF bank on the GPU (fft_admm_tv_bank_train, ADMM_TV_FLAG_PSF_BANK_TRAIN): the output and the
gradients to x, lambda, rho and every PSF of the bank against the fp64 restatement of
tests/bank_train_cases.py, at the training tables' fixed gates (output 1e-5, every gradient 1e-3, the PSF
gradient also per table) -- test_bank_train_case_inputs.py is what makes those gates legitimate -- and against
the library's own shared-PSF training step where the two must agree."""
import itertools

import pytest
import torch

import bank_cases as bc
import bank_train_cases as btc
import train_cases as tc

pytestmark = pytest.mark.gpu


def _step(dev, x, kerns, iso, maxit, cot, lam=btc.LAM, rho=btc.RHO, need=(True, True, True, True), fn=None):
    """One training step on the device -> dict(out, gx, glam, grho, gk) on the CPU (None where not required)."""
    from admmtor.eops.deconv import fft_admm_tv_bank_train
    fn = fn or fft_admm_tv_bank_train
    xd = x.to(dev).requires_grad_(need[0])
    lt = torch.tensor([lam], device=dev, requires_grad=need[1])
    rt = torch.tensor([rho], device=dev, requires_grad=need[2])
    kd = kerns.to(dev).requires_grad_(need[3])
    out = fn(xd, lt, rt, kd, iso, maxit)
    out.backward(cot.to(dev))
    torch.cuda.synchronize()
    c = lambda t: None if t.grad is None else t.grad.detach().cpu()  # noqa: E731
    return dict(out=out.detach().cpu(), gx=c(xd), glam=c(lt), grho=c(rt), gk=c(kd))


@pytest.mark.parametrize("name,mode,iso,maxit", btc.PARAMS)
def test_parity_with_the_fp64_restatement(cuda_dev, name, mode, iso, maxit):
    from admmtor import _native
    r = btc.reference(name, mode, iso, maxit)
    (B, C, H, W), k, path = btc.CASES[name][:3]
    flags = _native.bank_flags(r["kerns"].shape, B, C) | _native.ADMM_TV_FLAG_PSF_BANK_TRAIN | _native.ADMM_TV_FLAG_PSF_GRAD
    assert _native.path(_native.desc(B, C, H, W, k, iso, maxit, flags=flags), train=True) == path
    got = _step(cuda_dev, r["x"], r["kerns"], iso, maxit, r["cot"], lam=r["lam"])
    assert got["gk"].shape == r["kerns"].shape
    e = btc.errors(got, r["ref"])
    print(f"{name} {mode} iso={iso} maxit={maxit}: {tc.fmt(e)}")
    btc.check_gates((name, mode, iso, maxit), e)


@pytest.mark.parametrize("iso", btc.ISOS)
@pytest.mark.parametrize("name", ["pow2_16x32", "smooth_240x480", "gen_15x17"])
def test_shared_bank_is_fft_admm_tv_bit_for_bit(cuda_dev, name, iso):
    from admmtor.eops.deconv import fft_admm_tv
    shape, k = btc.CASES[name][:2]
    x, cot, kern = btc.case_input(name, iso), btc.cotangent(name), bc.make_bank("shared", shape[0], shape[1], k)
    a = _step(cuda_dev, x, kern, iso, 3, cot)
    b = _step(cuda_dev, x, kern, iso, 3, cot, fn=fft_admm_tv)
    for key in ("out", "gx", "glam", "grho", "gk"):
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("iso", btc.ISOS)
@pytest.mark.parametrize("mode", btc.MODES)
@pytest.mark.parametrize("name", ["pow2_16x32", "pow2_1024x32", "smooth_240x480"])
def test_equal_tables_give_the_shared_step(cuda_dev, name, mode, iso):
    """T copies of one PSF: the solve is the shared-PSF one, so out, gx, glam, grho are its bits (fused paths)
    and the tables' gradients add up to its PSF gradient."""
    from admmtor.eops.deconv import fft_admm_tv
    shape, k = btc.CASES[name][:2]
    x, cot, lam = btc.case_input(name, iso), btc.cotangent(name), btc.lam_of(name, iso)
    one = bc.make_bank("shared", shape[0], shape[1], k)
    Bk, Ck = bc.bank_dims(mode, shape[0], shape[1])
    a = _step(cuda_dev, x, one.expand(Bk, Ck, k, k).contiguous(), iso, 3, cot, lam=lam)
    b = _step(cuda_dev, x, one, iso, 3, cot, lam=lam, fn=fft_admm_tv)
    for key in ("out", "gx", "glam", "grho"):
        assert torch.equal(a[key], b[key]), key
    assert tc.rel(a["gk"].sum(dim=(0, 1), keepdim=True), b["gk"]) <= tc.GATE_GRAD_PSF


@pytest.mark.parametrize("name", ["pow2_16x32", "smooth_240x480", "gen_15x17"])
def test_per_image_bank_equals_the_loop_of_single_image_steps(cuda_dev, name):
    """Independent of the restatement: aniso planes are independent, so a per-image bank is the loop of
    single-image fft_admm_tv training steps -- gx and gkerns[b] per image, glam / grho summed."""
    from admmtor.eops.deconv import fft_admm_tv
    x, cot, kerns, lam = btc.case_input(name, False), btc.cotangent(name), btc.case_bank(name, "image"), btc.lam_of(name, False)
    a = _step(cuda_dev, x, kerns, False, 3, cot, lam=lam)
    gl = gr = 0.0
    for b in range(x.shape[0]):
        s = _step(cuda_dev, x[b:b + 1], kerns[b:b + 1], False, 3, cot[b:b + 1], lam=lam, fn=fft_admm_tv)
        assert tc.rel(a["out"][b:b + 1], s["out"]) <= tc.GATE_FWD
        assert tc.rel(a["gx"][b:b + 1], s["gx"]) <= tc.GATE_GRAD_PSF
        assert tc.rel(a["gk"][b:b + 1], s["gk"]) <= tc.GATE_GRAD_PSF
        gl, gr = gl + s["glam"].double(), gr + s["grho"].double()
    assert tc.scalar_err(a["glam"], gl) <= tc.GATE_GRAD_PSF and tc.scalar_err(a["grho"], gr) <= tc.GATE_GRAD_PSF


_NEEDS = [n for n in itertools.product((False, True), repeat=4) if any(n)]  # the 15 non-empty combinations


@pytest.fixture(scope="module")
def all_on_step(cuda_dev):
    name, mode, iso, maxit = "pow2_16x32", "plane", True, 3
    x, cot, kerns = btc.case_input(name, iso), btc.cotangent(name), btc.case_bank(name, mode)
    return x, cot, kerns, iso, maxit, _step(cuda_dev, x, kerns, iso, maxit, cot)


@pytest.mark.parametrize("need", _NEEDS, ids=lambda n: "".join(c for c, on in zip("xlrk", n) if on))
def test_which_inputs_require_grad(cuda_dev, all_on_step, monkeypatch, need):
    """Every combination gives the all-on step's values, and the public call keeps the r_k spectra (the
    PSF-gradient flag, seen in the descriptor whose history it sizes) only when kerns requires grad."""
    from admmtor import _native
    x, cot, kerns, iso, maxit, full = all_on_step
    seen = []
    sized = _native.history_size

    def record(d):
        seen.append((bool(d.flags & _native.ADMM_TV_FLAG_PSF_GRAD), sized(d)))
        return seen[-1][1]
    monkeypatch.setattr(_native, "history_size", record)
    got = _step(cuda_dev, x, kerns, iso, maxit, cot, need=need)
    monkeypatch.undo()
    assert torch.equal(got["out"], full["out"])
    for key, on in zip(("gx", "glam", "grho", "gk"), need):
        if on:
            assert torch.equal(got[key], full[key]), key
        else:
            assert got[key] is None, key
    B, C, H, W = x.shape
    plain = _native.history_size(_native.desc(B, C, H, W, 5, iso, maxit))
    kept = _native.history_size(_native.desc(B, C, H, W, 5, iso, maxit, flags=_native.ADMM_TV_FLAG_PSF_GRAD))
    assert kept > plain
    assert seen == [(need[3], kept if need[3] else plain)], seen


@pytest.mark.parametrize("mode", btc.MODES)
@pytest.mark.parametrize("name", ["pow2_16x32", "smooth_240x480", "gen_15x17"])
def test_no_iterations_zero_every_gradient(cuda_dev, name, mode):
    """maxit == 0: the output is zero, and so is every gradient -- all T k k taps of the bank, not the first
    table's alone (the gradient buffers come from torch.empty: they are pre-filled here through the caching
    allocator, so a tap the library left alone would not read as zero)."""
    x, cot, kerns = btc.case_input(name, False), btc.cotangent(name), btc.case_bank(name, mode)
    junk = [torch.full((kerns.numel(),), 7.0, device=cuda_dev) for _ in range(4)]
    del junk
    got = _step(cuda_dev, x, kerns, False, 0, cot)
    assert got["gk"].shape == kerns.shape
    for key in ("out", "gx", "glam", "grho", "gk"):
        assert torch.count_nonzero(got[key]) == 0, key


@pytest.mark.parametrize("name", ["pow2_16x32", "smooth_240x480", "gen_15x17"])
def test_no_grad_is_the_inference_call(cuda_dev, name):
    from admmtor.eops.deconv import fft_admm_tv_bank, fft_admm_tv_bank_train
    x, kerns = btc.case_input(name, True).to(cuda_dev), btc.case_bank(name, "plane").to(cuda_dev)
    ref = fft_admm_tv_bank(x, btc.LAM, btc.RHO, kerns, True, 3)
    assert torch.equal(fft_admm_tv_bank_train(x, btc.LAM, btc.RHO, kerns, True, 3), ref)  # nothing requires grad
    with torch.no_grad():
        assert torch.equal(fft_admm_tv_bank_train(x, btc.LAM, btc.RHO, kerns.clone().requires_grad_(True), True, 3), ref)
    # and the training forward's output is the same solve
    assert torch.equal(fft_admm_tv_bank_train(x, btc.LAM, btc.RHO, kerns.clone().requires_grad_(True), True, 3).detach(), ref)


def test_second_backward_and_double_backward_raise(cuda_dev):
    from admmtor.eops.deconv import fft_admm_tv_bank_train
    x = btc.case_input("pow2_16x32", False).to(cuda_dev).requires_grad_(True)
    kerns = btc.case_bank("pow2_16x32", "channel").to(cuda_dev).requires_grad_(True)
    out = fft_admm_tv_bank_train(x, btc.LAM, btc.RHO, kerns, False, 3)
    out.sum().backward()
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        out.sum().backward()
    out = fft_admm_tv_bank_train(x, btc.LAM, btc.RHO, kerns, False, 3)
    with pytest.raises(NotImplementedError, match="double backward"):
        g = torch.autograd.grad(out.sum(), (x, kerns), create_graph=True)
        (g[0].sum() + g[1].sum()).backward()


@pytest.mark.parametrize("iso,psf_grad", [(False, True), (True, False), (True, True)])
def test_opcheck(cuda_dev, iso, psf_grad):
    import admmtor._ops  # noqa: F401
    x = btc.case_input("pow2_16x32", iso).to(cuda_dev).requires_grad_(True)
    kerns = btc.case_bank("pow2_16x32", "plane").to(cuda_dev).requires_grad_(psf_grad)
    lam = torch.tensor([btc.LAM], device=cuda_dev, requires_grad=True)
    rho = torch.tensor([btc.RHO], device=cuda_dev, requires_grad=True)
    torch.library.opcheck(torch.ops.admm_hip.fft_admm_tv_bank_fwd_train.default, (x, lam, rho, kerns, iso, 3, psf_grad),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor",
                                      "test_aot_dispatch_static"))
    out, hist = torch.ops.admm_hip.fft_admm_tv_bank_fwd_train(x.detach(), lam.detach(), rho.detach(), kerns.detach(),
                                                               iso, 3, psf_grad)
    torch.library.opcheck(torch.ops.admm_hip.fft_admm_tv_bank_bwd.default,
                          (torch.randn_like(out), x.detach(), lam.detach(), rho.detach(), kerns.detach(), hist, iso, 3,
                           psf_grad, True, True, psf_grad))


def test_module_step(cuda_dev):
    """One ADMMDeconvBank step: w.grad is fft_admm_tv_bank_train's gkerns for the same inputs."""
    from admmtor.elayers.admmdeconv import ADMMDeconvBank
    torch.manual_seed(5)
    m = ADMMDeconvBank((5, 5), 3, channels=3, lmbda=btc.LAM, rho=btc.RHO, iso=True).to(cuda_dev)
    x, cot = btc.case_input("pow2_16x32", True), btc.cotangent("pow2_16x32")
    m(x.to(cuda_dev)).backward(cot.to(cuda_dev))
    ref = _step(cuda_dev, x, m.w.detach().cpu(), True, 3, cot, need=(False, False, False, True))
    assert m.w.grad.shape == (1, 3, 5, 5) and torch.equal(m.w.grad.cpu(), ref["gk"])
