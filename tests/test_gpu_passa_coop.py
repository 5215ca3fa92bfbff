"""The cooperative row pass (admm_kernels.hpp k_pass_a COOP: the strips of a block share their halo
rows through LDS, even strips walked downwards, odd ones upwards) and the u-store skip of a solve's
last row pass.  Both change no arithmetic, so every comparison is torch.equal: against the A/B build
(admmtor._native.ab_library) with ADMM_PASSA_COOP=0, the plain kernel.

The release rule picks strips of 2 rows for inputs this small (strip_rows: too few strips to fill the
chip), so the strip height of the headline, R = 8, is pinned in the A/B build (ADMM_PASSA_R=8) and the
knob is compared on / off there; the release library's own solve (R = 2: the shortest strip the
cooperative kernel takes) is compared against the same reference, which it must equal because the
results do not depend on the strip height.

The iso variant of the cooperative kernel is not built (it does not fit 3 waves per SIMD without
spilling) and the odd-length row pass keeps its u stores (its deferred stores are a different loop), so
neither has a case here.  The training side -- the history row pass that RowOps::pass_a keeps on the plain
kernel (!hist), beside the cooperative one at the same shape -- is in tests/test_gpu_train_shapes.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_REF64 = 1e-5
W = 1024  # rows of 1,024 pixels: the 512-point row kernel, four one-wave sub-groups per block


def solve(x, k, iso, it, dev, lam=0.01, rho=0.02):
    from admmtor.eops.deconv import fft_admm_tv
    out = fft_admm_tv(x.to(dev), lam, rho, k.to(dev), iso, it)
    torch.cuda.synchronize()
    return out.cpu()


def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return ((a - b).norm() / b.norm()).item()


_inputs = {}


def inputs(H, w=W, planes=(1, 3)):
    from admmtor.synth import blurred_batch, make_psf
    key = (H, w, planes)
    if key not in _inputs:
        k = make_psf("gauss:1.5", 9)
        _inputs[key] = (blurred_batch(planes[0], planes[1], H, w, k, seed=H + w), k)
    return _inputs[key]


def ab_solve(monkeypatch, x, k, it, dev, coop, R=8):
    from admmtor import _native
    monkeypatch.setenv("ADMM_PASSA_COOP", str(coop))
    if R:
        monkeypatch.setenv("ADMM_PASSA_R", str(R))
    else:
        monkeypatch.delenv("ADMM_PASSA_R", raising=False)
    with _native.ab_library():
        return solve(x, k, False, it, dev)


# H = 32 with R = 8: one block per plane, both outer halos wrap onto the block's own rows;
# H = 64: two blocks per plane (block-to-block halos).  Three planes: the plane offsets matter.
# maxit = 1: no row pass; 2: the first row pass is also the last (no u stores on the FIRST variant);
# 5: steady launches and a last one.
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("it", [1, 2, 5])
def test_coop_equals_plain_kernel(cuda_dev, monkeypatch, H, it):
    x, k = inputs(H)
    ref = ab_solve(monkeypatch, x, k, it, cuda_dev, coop=0)
    got = ab_solve(monkeypatch, x, k, it, cuda_dev, coop=1)
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref)
    # the release library: its own strip height (2 rows here), the cooperative kernel on by default
    assert torch.equal(solve(x, k, False, it, cuda_dev), ref)


def test_refused_shape_runs_the_plain_kernel(cuda_dev, monkeypatch):
    """H = 16 with R = 8: two strips per plane, not a multiple of the four sub-groups of a block, so a
    block would straddle planes: the host's selection rule keeps the plain kernel (equal result, and
    above all no block waiting at a barrier for waves that never come)."""
    x, k = inputs(16)
    ref = ab_solve(monkeypatch, x, k, 5, cuda_dev, coop=0)
    assert torch.equal(ab_solve(monkeypatch, x, k, 5, cuda_dev, coop=1), ref)
    assert torch.equal(solve(x, k, False, 5, cuda_dev), ref)  # release: R = 2, eight strips per plane


@pytest.mark.parametrize("it", [2, 5])
def test_coop_vs_fp64_oracle(cuda_dev, monkeypatch, it):
    """The cooperative kernel (R = 8 and the release's R = 2) against the fp64 oracle: this also pins
    the u-store skip to the right launch (a u dropped one iteration early would be read as garbage)."""
    from oracle.admm_oracle import solve_fourier
    x, k = inputs(32)
    ref = solve_fourier(x.double(), 0.01, 0.02, k.double(), False, it)
    e8 = rel(ab_solve(monkeypatch, x, k, it, cuda_dev, coop=1), ref)
    e2 = rel(solve(x, k, False, it, cuda_dev), ref)
    print(f"32x{W} maxit {it}: rel-L2 vs fp64 oracle {e8:.2e} (R = 8), {e2:.2e} (release)")
    assert e8 <= TOL_REF64 and e2 <= TOL_REF64


@pytest.mark.parametrize("it", [2, 5])
def test_mixed_radix_last_pass_without_u(cuda_dev, monkeypatch, it):
    """240 x 480 runs the mixed-radix row pass (fused_forward on MixedOps), whose last launch writes no u either:
    against the fp64 oracle, and equal to the A/B build's solve."""
    from admmtor import _native
    from oracle.admm_oracle import solve_fourier
    assert _native.load().admm_tv_supported(240, 480) == 3
    x, k = inputs(240, 480, (1, 2))
    got = solve(x, k, False, it, cuda_dev)
    assert rel(got, solve_fourier(x.double(), 0.01, 0.02, k.double(), False, it)) <= TOL_REF64
    assert torch.equal(ab_solve(monkeypatch, x, k, it, cuda_dev, coop=0, R=0), got)
