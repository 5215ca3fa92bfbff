"""The fused training path (HIST row pass, history iso norm pass, out-of-place column pass, k_bwd_pass_a,
k_bwd_iso_q, k_xspec / k_psf_grad) at every row width, column height and strip height, against the fp64
oracle's autograd (solve_spatial, the reference's op sequence).  The cases are tests/train_cases.py's;
tests/test_train_case_inputs.py shows on the CPU that each stays >= 1e-5 tau away from the soft threshold's
kink and that the reference op sequence in fp32 already meets the gates, so the gates here are fixed:
relative L2, the project's own (test_gpu_grad.py) -- training forward <= 1e-5; x, lambda, rho gradients
<= 1e-4 without a PSF; every gradient, the PSF's included, <= 1e-3 with one.  No max(..., floor) term, no
near-kink exemption.  A lambda / rho reference gradient that is exactly 0 is compared absolutely.

Strip heights.  strip_rows() gives R = 2 for shapes this small, so R = 2, 4, 8, 16 are pinned in the A/B
build (ADMM_PASSA_R; forward and backward inside _native.ab_library()).  Read from k_pass_a (HIST) and
k_bwd_pass_a: a row's arithmetic does not depend on the strip it sits in -- every row g is transformed,
differenced against row g - 1 and finalized from the same operands in the same order whether row g - 1 is
the strip's halo (recomputed) or its previous row, and k_iso_norm / k_bwd_iso_q work per row -- so the
output, the x gradient and the PSF gradient must be torch.equal between the R values, and that is
asserted (it held on an MI355X at every R of every case).  The lambda / rho gradients sum per-strip fp64
partials, whose grouping follows R: <= 1e-5 (measured: equal after the rounding to fp32).

Every case prints its errors (pytest -s); the worst per group are recorded in DESIGN.md section 2."""
import pytest
import torch

import train_cases as tc

pytestmark = pytest.mark.gpu


def assert_fused(case):
    from admmtor import _native
    B, C, H, W = case.shape
    G = len(case.lam) if isinstance(case.lam, tuple) else 1
    d = _native.desc(B, C, H, W, case.psf[1] if case.psf else 0, case.iso, case.maxit,
                     _native.ADMM_TV_FLAG_PSF_GRAD if case.learn_psf else 0, G)
    assert _native.path(d, train=True) == "fused"
    return d


def hip_train(case, dev, dtype=torch.float32):
    """fft_admm_tv with x, lambda, rho (and the PSF where learnable) requiring gradients, and its
    gradients against the case's cotangent: dict(out, gx, glam, grho[, gk]) on the CPU.  dtype: of every
    input (torch.float64: the fp64 solve)."""
    from admmtor.eops.deconv import fft_admm_tv
    x, k = tc.inputs(case)
    xg = x.to(dev, dtype).requires_grad_(True)
    lam = torch.tensor([case.lam], device=dev, dtype=dtype, requires_grad=True)
    rho = torch.tensor([case.rho], device=dev, dtype=dtype, requires_grad=True)
    kg = k.to(dev, dtype).requires_grad_(case.learn_psf) if k.numel() else torch.empty(0, device=dev, dtype=dtype)
    out = fft_admm_tv(xg, lam, rho, kg, case.iso, case.maxit)
    wrt = (xg, lam, rho) + ((kg,) if case.learn_psf else ())
    g = torch.autograd.grad(out, wrt, tc.cotangent(case).to(dev, dtype))
    torch.cuda.synchronize()
    got = dict(out=out.detach().cpu(), gx=g[0].cpu(), glam=g[1].cpu(), grho=g[2].cpu())
    if case.learn_psf:
        got["gk"] = g[3].cpu()
    return got


# ------------------------------------------------------------------ row widths, column heights, maxit
@pytest.mark.parametrize("case", tc.TABLE_CASES, ids=str)
def test_training_vs_oracle(cuda_dev, case):
    assert_fused(case)
    e = tc.errors(hip_train(case, cuda_dev), tc.reference(case))
    print(f"[{case.group}] {case.name} {case.shape} maxit {case.maxit}: {tc.fmt(e)}")
    tc.check_gates(case, e)


# ------------------------------------------------------------------ strip heights (A/B build)
_ab = {}


def ab_train(monkeypatch, case, R, dev):
    """The case solved and differentiated in the A/B build with strips of R rows (0: the rule), once."""
    from admmtor import _native
    if (case.name, R) not in _ab:
        monkeypatch.delenv("ADMM_PASSA_COOP", raising=False)
        if R:
            monkeypatch.setenv("ADMM_PASSA_R", str(R))
        else:
            monkeypatch.delenv("ADMM_PASSA_R", raising=False)
        with _native.ab_library():
            ws = _native.backward_workspace_size(assert_fused(case))
            _ab[(case.name, R)] = (hip_train(case, dev), ws)
    return _ab[(case.name, R)]


@pytest.mark.parametrize("R", tc.STRIP_ROWS)
@pytest.mark.parametrize("case", tc.STRIP_CASES, ids=str)
def test_strip_height_vs_oracle(cuda_dev, monkeypatch, case, R):
    got, _ = ab_train(monkeypatch, case, R, cuda_dev)
    e = tc.errors(got, tc.reference(case))
    print(f"[strip] {case.name} {case.shape} R = {R}: {tc.fmt(e)}")
    tc.check_gates(case, e)


@pytest.mark.parametrize("case", tc.STRIP_CASES, ids=str)
def test_strip_heights_agree(cuda_dev, monkeypatch, case):
    runs = [ab_train(monkeypatch, case, R, cuda_dev) for R in tc.STRIP_ROWS]
    # the knob took: the backward workspace holds maxit x nstrips fp64 partial pairs, fewer with taller strips
    sizes = [ws for _, ws in runs]
    assert all(a > b for a, b in zip(sizes, sizes[1:])), sizes
    base = runs[0][0]
    for R, (got, _) in zip(tc.STRIP_ROWS[1:], runs[1:]):
        el, er = tc.scalar_err(got["glam"], base["glam"]), tc.scalar_err(got["grho"], base["grho"])
        print(f"[strip] {case.name} R = {R} vs R = 2: out / x^ / PSF^ equal, lambda^ {el:.2e} rho^ {er:.2e}")
        assert torch.equal(got["out"], base["out"])
        assert torch.equal(got["gx"], base["gx"])
        if case.learn_psf:
            assert torch.equal(got["gk"], base["gk"])
        assert el <= 1e-5 and er <= 1e-5


def test_ab_build_equals_release(cuda_dev, monkeypatch):
    """With no knob set the A/B build is the release library: element for element, gradients included
    (a stale A/B library would make the strip-height cases above test old kernels)."""
    case = tc.STRIP_CASES[0]
    ab, _ = ab_train(monkeypatch, case, 0, cuda_dev)
    release = hip_train(case, cuda_dev)
    assert sorted(ab) == sorted(release)
    for key in release:
        assert torch.equal(ab[key], release[key]), key


# ------------------------------------------------------------------ grouped: blocks of strips across modules
@pytest.mark.parametrize("case", tc.GROUPED_CASES, ids=str)
def test_grouped_blocks_across_modules(cuda_dev, case):
    """Three modules whose strips share blocks (mod = p / ppm changes inside a block): against three
    separate calls at test_gpu_grouped.py's gates, and every module against the oracle."""
    from admmtor.eops.deconv import fft_admm_tv, fft_admm_tv_grouped
    assert_fused(case)
    mods = tc.modules(case)
    x, k = tc.inputs(case)
    x, k = x.to(cuda_dev), k.to(cuda_dev)
    cots = [tc.cotangent(m).to(cuda_dev) for m in mods]

    def run(grouped):
        xr = x.clone().requires_grad_(True)
        lt = [torch.tensor([m.lam], device=cuda_dev, requires_grad=True) for m in mods]
        rt = [torch.tensor([m.rho], device=cuda_dev, requires_grad=True) for m in mods]
        outs = fft_admm_tv_grouped(xr, lt, rt, k, case.iso, case.maxit) if grouped else \
            [fft_admm_tv(xr, l, r, k, case.iso, case.maxit) for l, r in zip(lt, rt)]
        g = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cots)), [xr] + lt + rt)
        torch.cuda.synchronize()
        n = len(mods)
        return [o.detach().cpu() for o in outs], g[0].cpu(), torch.cat(g[1:1 + n]).cpu(), torch.cat(g[1 + n:]).cpu()

    (o_sep, gx_sep, gl_sep, gr_sep), (o_grp, gx_grp, gl_grp, gr_grp) = run(False), run(True)
    for a, b in zip(o_grp, o_sep):
        if case.iso:
            assert tc.rel(a, b) <= 1e-6
        else:
            assert torch.equal(a, b)
    e = (tc.rel(gx_grp, gx_sep), tc.rel(gl_grp, gl_sep), tc.rel(gr_grp, gr_sep))
    print(f"[grouped] {case.name} vs separate calls: x^ {e[0]:.2e} lambda^ {e[1]:.2e} rho^ {e[2]:.2e}")
    assert e[0] <= 1e-6 and e[1] <= 1e-5 and e[2] <= 1e-5
    refs = [tc.reference(m) for m in mods]
    ex = tc.rel(gx_grp, sum(r["gx"] for r in refs))  # the modules share x: its gradient is their sum
    print(f"[grouped] {case.name} vs oracle: x^ {ex:.2e}")
    assert ex <= case.gate
    for i, (m, r) in enumerate(zip(mods, refs)):
        em = dict(out=tc.rel(o_grp[i], r["out"]), glam=tc.scalar_err(gl_grp[i], r["glam"]),
                  grho=tc.scalar_err(gr_grp[i], r["grho"]))
        print(f"[grouped] {m.name} vs oracle: {tc.fmt(em)}")
        assert em["out"] <= tc.GATE_FWD and em["glam"] <= case.gate and em["grho"] <= case.gate, (m.name, em)


# ------------------------------------------------------------------ the history row pass beside the cooperative one
def test_history_pass_beside_cooperative_pass(cuda_dev):
    """RowOps::pass_a picks the cooperative kernel by !hist: at 1,024-pixel rows an inference solve runs it
    (release library), a training solve of the same input the plain history kernel.  k_pass_a's HIST
    variant keeps a_k and rebuilds u_k = a_k - S(a_k) from it with the operands the inference variant
    stored u_k from, so the two outputs are equal bit for bit; both against the oracle."""
    from admmtor.eops.deconv import fft_admm_tv
    case = tc.COOP_CASE
    assert case.shape[3] == 1024 and not case.iso
    x, k = tc.inputs(case)
    train = hip_train(case, cuda_dev)["out"]
    infer = fft_admm_tv(x.to(cuda_dev), case.lam, case.rho, k.to(cuda_dev), case.iso, case.maxit).cpu()
    ref = tc.reference(case)["out"]
    et, ei = tc.rel(train, ref), tc.rel(infer, ref)
    print(f"[coop] {case.name}: training {et:.2e}, inference {ei:.2e} vs oracle; training vs inference "
          f"{tc.rel(train, infer):.2e}")
    assert et <= tc.GATE_FWD and ei <= tc.GATE_FWD
    assert torch.equal(train, infer)
