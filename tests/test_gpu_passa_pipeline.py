"""The pipelined cooperative row pass (admm_kernels.hpp k_pass_a PF: every row stream -- the x spectrum
row, u_y, b, u_x -- is requested a row ahead of its use, through buffer resources, and the request after
a strip's last step is issued past the resource's end so that the hardware drops it).  It changes no
arithmetic, so every comparison is torch.equal: the A/B build (admmtor._native.ab_library) with
ADMM_PASSA_PF=1 against ADMM_PASSA_PF=0, the cooperative kernel without the pipeline.

As in tests/test_gpu_passa_coop.py the strip height is pinned in the A/B build (the release rule picks 2
rows for inputs this small): R = 8, and R = 4, what the release rule takes for this kernel at the
headline's size.  The release library's own solve is compared against the same reference: with R = 2 the
loop runs one step per strip, the one whose next-row requests are all dropped ones.

Both image layouts are run: pixel order (ADMM_PL=0, what a solve at 1,024-pixel rows takes by default)
and lane-paired (ADMM_PL=1, 16-byte accesses); the layout is a permutation inside each row, so all
results are equal across it as well."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_REF64 = 1e-5
W = 1024  # rows of 1,024 pixels: the 512-point row kernel, four one-wave sub-groups per block


def solve(x, k, it, dev, lam=0.01, rho=0.02):
    from admmtor.eops.deconv import fft_admm_tv
    out = fft_admm_tv(x.to(dev), lam, rho, k.to(dev), False, it)
    torch.cuda.synchronize()
    return out.cpu()


def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return ((a - b).norm() / b.norm()).item()


_inputs = {}


def inputs(H, planes=(1, 3)):
    from admmtor.synth import blurred_batch, make_psf
    if H not in _inputs:
        k = make_psf("gauss:1.5", 9)
        _inputs[H] = (blurred_batch(planes[0], planes[1], H, W, k, seed=H + W), k)
    return _inputs[H]


def ab_solve(monkeypatch, x, k, it, dev, pf, pl=0, R=8):
    from admmtor import _native
    monkeypatch.setenv("ADMM_PASSA_PF", str(pf))
    monkeypatch.setenv("ADMM_PL", str(pl))
    monkeypatch.setenv("ADMM_PASSA_R", str(R))
    monkeypatch.delenv("ADMM_PASSA_COOP", raising=False)
    with _native.ab_library():
        return solve(x, k, it, dev)


# H = 32 with R = 8: one block per plane, both outer halos wrap onto the block's own rows;
# H = 64, and R = 4: several blocks per plane (halos between blocks).  Three planes: the per-plane
# resources matter.
# maxit = 1: no row pass; 2: the FIRST launch is also the last (no u loads, no u output: its stores go
# to an empty resource); 3: one steady launch, which is also the last; 5: steady launches and a last one.
@pytest.mark.parametrize("pl", [0, 1])
@pytest.mark.parametrize("R", [8, 4])
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("it", [1, 2, 3, 5])
def test_pipelined_equals_unpipelined(cuda_dev, monkeypatch, H, it, R, pl):
    x, k = inputs(H)
    ref = ab_solve(monkeypatch, x, k, it, cuda_dev, pf=0, pl=pl, R=R)
    got = ab_solve(monkeypatch, x, k, it, cuda_dev, pf=1, pl=pl, R=R)
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref)
    # the release library: its own strip height (2 rows here), the pipelined kernel on by default
    assert torch.equal(solve(x, k, it, cuda_dev), ref)


@pytest.mark.parametrize("pl", [0, 1])
def test_refused_shape_runs_the_plain_kernel(cuda_dev, monkeypatch, pl):
    """H = 16 with R = 8: two strips per plane, so the cooperative kernel is refused (a block would
    straddle planes) and with it the pipeline: the plain kernel runs with the knob on and off."""
    x, k = inputs(16)
    ref = ab_solve(monkeypatch, x, k, 5, cuda_dev, pf=0, pl=pl)
    assert torch.isfinite(ref).all()
    assert torch.equal(ab_solve(monkeypatch, x, k, 5, cuda_dev, pf=1, pl=pl), ref)


@pytest.mark.parametrize("it", [2, 5])
def test_pipelined_vs_fp64_oracle(cuda_dev, monkeypatch, it):
    """The pipelined kernel (R = 8 in both layouts, and the release's R = 2) against the fp64 oracle."""
    from oracle.admm_oracle import solve_fourier
    x, k = inputs(32)
    ref = solve_fourier(x.double(), 0.01, 0.02, k.double(), False, it)
    e0 = rel(ab_solve(monkeypatch, x, k, it, cuda_dev, pf=1, pl=0), ref)
    e1 = rel(ab_solve(monkeypatch, x, k, it, cuda_dev, pf=1, pl=1), ref)
    e2 = rel(solve(x, k, it, cuda_dev), ref)
    print(f"32x{W} maxit {it}: rel-L2 vs fp64 oracle {e0:.2e} (R = 8), {e1:.2e} (R = 8, lane-paired), {e2:.2e} (release)")
    assert e0 <= TOL_REF64 and e1 <= TOL_REF64 and e2 <= TOL_REF64
