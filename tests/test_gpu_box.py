"""The solve with bounds on x on the GPU (admm_tv_forward_box; admmtor.eops.deconv.fft_admm_tv_box).

Every parity assertion is the project's gate, 1e-5 rel-L2 against the fp64 restatement of the iteration
(tests/box_cases.py), never against fft_admm_tv, whose iterates these are not.  The cases carry negative
controls (seven wrong variants of the restatement each miss it by >= 1e-4 at K = 3 and K = 6, and the projection
is active on 5 % .. 95 % of the pixels in every iteration), so a kernel that drops, mis-signs or fails to
accumulate any part of the new term cannot pass.  Measured on one MI355X: 7.4e-8 .. 1.4e-6 over all cases and K."""
import ctypes

import pytest
import torch

import box_cases as bc
from box_cases import BOUNDS, LAM, RHO, TOL_REF64

pytestmark = pytest.mark.gpu

INF = float("inf")


def rel(a, b):
    a, b = a.double().reshape(-1).cpu(), b.double().reshape(-1).cpu()
    return ((a - b).norm() / b.norm()).item()


def kern_on(k, dev):
    return k.to(dev) if k.numel() else torch.empty(0, device=dev)


def gpu_box(x, k, iso, K, dev, lo=BOUNDS[0], hi=BOUNDS[1], project=False):
    from admmtor.eops.deconv import fft_admm_tv_box
    out = fft_admm_tv_box(x.to(dev), LAM, RHO, kern_on(k, dev), lo, hi, iso, K, project)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- 1: parity with the fp64 restatement
@pytest.mark.parametrize("name,iso,K", bc.PARAMS)
def test_box_matches_the_restatement(cuda_dev, name, iso, K):
    from admmtor import _native
    r = bc.reference(name, iso, K)
    x, k = r["x"], r["k"]
    kk = int(k.shape[-1]) if k.numel() else 0
    path = _native.path(_native.desc(*x.shape, kk, iso, K), mode=3)
    assert path == bc.CASES[name][3], path
    got = gpu_box(x, k, iso, K, cuda_dev)
    assert got.dtype == torch.float32 and got.shape == x.shape and got.device.type == "cuda"
    e = rel(got, r["ref"])
    weakest = min(v[Kc] for v in r["controls"].values() for Kc in v)
    print(name, iso, K, path, f"vs fp64 restatement {e:.2e} (controls >= {weakest:.1e})")
    assert e <= TOL_REF64


@pytest.mark.parametrize("lo,hi", [(0.0, INF), (-INF, INF)])
@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("name", ["pow2_16", "generic_15x17"])
def test_default_and_infinite_bounds(cuda_dev, name, iso, lo, hi):
    """The defaults (0, +inf), and no bounds at all: v stays 0, w = x_k, and the result is the restatement's
    proximal-point iterate -- not fft_admm_tv's."""
    r = bc.restated(name, iso, lo, hi)
    for K in (3, 6):
        e = rel(gpu_box(r["x"], r["k"], iso, K, cuda_dev, lo, hi), r["xs"][K - 1])
        print(name, iso, (lo, hi), K, f"{e:.2e}")
        assert e <= TOL_REF64
    if (lo, hi) == (0.0, INF):  # the wrapper's defaults are these bounds
        from admmtor.eops.deconv import fft_admm_tv_box
        a = fft_admm_tv_box(r["x"].to(cuda_dev), LAM, RHO, kern_on(r["k"], cuda_dev), iso=iso, maxit=6, project=False)
        assert torch.equal(a, gpu_box(r["x"], r["k"], iso, 6, cuda_dev, lo, hi))


# ---------------------------------------------------------------- 2: the wrapper's contract
EDGE_CASES = [("pow2_16", False), ("pow2_16", True), ("pow2_1024_pixel", False), ("generic_15x17", True),
              ("generic_one_row", False)]


@pytest.mark.parametrize("name,iso", EDGE_CASES)
def test_project_is_the_clamp_and_the_call_is_pure(cuda_dev, name, iso):
    """project=True is the clamp of project=False bit for bit (and feasible); bounds as device tensors give the
    bits of Python floats; xin is unchanged by a call."""
    x, k = bc.make_input(*bc.CASES[name][:2])
    xd = x.to(cuda_dev)
    keep = xd.clone()
    raw = gpu_box(xd, k, iso, 4, cuda_dev)
    proj = gpu_box(xd, k, iso, 4, cuda_dev, project=True)
    assert torch.equal(proj, raw.clamp(*BOUNDS))
    assert proj.min().item() >= BOUNDS[0] and proj.max().item() <= BOUNDS[1]
    assert not torch.equal(proj, raw)  # x_4 is not feasible yet: the clamp does something
    assert torch.equal(xd, keep)
    lo_t, hi_t = torch.tensor(BOUNDS[0], device=cuda_dev), torch.tensor([BOUNDS[1]], device=cuda_dev)
    assert torch.equal(gpu_box(xd, k, iso, 4, cuda_dev, lo_t, hi_t), raw)
    assert torch.equal(gpu_box(xd, k, iso, 4, cuda_dev, lo_t.cpu(), BOUNDS[1]), raw)
    assert torch.equal(gpu_box(xd, k, iso, 4, cuda_dev, lo_t, hi_t, project=True), proj)


def raw_call(x, k, iso, K, ws=None, bounds=BOUNDS):
    """admm_tv_forward_box through ctypes on device tensors; ws: the workspace to use (default: a new one)."""
    from admmtor import _native
    dev = x.device
    d = _native.desc(*x.shape, int(k.shape[-1]) if k.numel() else 0, iso, K)
    if ws is None:
        ws = torch.empty(_native.box_workspace_size(d), dtype=torch.uint8, device=dev)
    lam_t, rho_t = torch.full((1,), LAM, device=dev), torch.full((1,), RHO, device=dev)
    b_t = torch.tensor(bounds, dtype=torch.float32, device=dev)
    out = torch.empty_like(x)
    _native.check(_native.load().admm_tv_forward_box(
        d, x.data_ptr(), k.data_ptr() if k.numel() else None, lam_t.data_ptr(), rho_t.data_ptr(), b_t.data_ptr(),
        out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return out, ws


@pytest.mark.parametrize("name,iso", EDGE_CASES)
def test_one_workspace_twice_gives_the_same_bits(cuda_dev, name, iso):
    """Two calls with one workspace: the second starts from whatever v the first left there and must not read
    it (v_0 = 0 is the first row pass's, not the buffer's)."""
    x, k = bc.make_input(*bc.CASES[name][:2])
    xd, kd = x.to(cuda_dev), kern_on(k, cuda_dev)
    a, ws = raw_call(xd, kd, iso, 5)
    ws.fill_(0xFF)  # NaNs in every region
    b, _ = raw_call(xd, kd, iso, 5, ws)
    c, _ = raw_call(xd, kd, iso, 5, ws)
    assert torch.equal(a, b) and torch.equal(b, c)
    assert torch.equal(a, gpu_box(xd, k, iso, 5, cuda_dev))  # the wrapper is this call


def test_workspace_too_small_is_refused(cuda_dev):
    """The plain solve's workspace lacks the image of v: refused, not overrun."""
    from admmtor import _native
    x, k = bc.make_input(*bc.CASES["pow2_16"][:2])
    xd, kd = x.to(cuda_dev), kern_on(k, cuda_dev)
    d = _native.desc(*x.shape, int(k.shape[-1]), False, 3)
    ws = torch.empty(_native.workspace_size(d), dtype=torch.uint8, device=cuda_dev)
    with pytest.raises(_native.NativeError) as ei:
        raw_call(xd, kd, False, 3, ws)
    assert ei.value.code == _native.ADMM_TV_EWORKSPACE


@pytest.mark.parametrize("name,iso", [("pow2_16", False), ("generic_15x17", True)])
def test_zero_iterations_give_zeros(cuda_dev, name, iso):
    x, k = bc.make_input(*bc.CASES[name][:2])
    out = gpu_box(x, k, iso, 0, cuda_dev)
    assert out.shape == x.shape and not out.any()
    raw, _ = raw_call(x.to(cuda_dev), kern_on(k, cuda_dev), iso, 0)
    assert not raw.any()


@pytest.mark.parametrize("name,iso", [("pow2_16", True), ("generic_15x17", False)])
def test_host_tensors_come_back_on_the_host(cuda_dev, name, iso):
    from admmtor.eops.deconv import fft_admm_tv_box
    x, k = bc.make_input(*bc.CASES[name][:2])
    out = fft_admm_tv_box(x, LAM, RHO, k, *BOUNDS, iso, 3, project=False)
    assert out.device.type == "cpu" and out.dtype == torch.float32
    assert torch.equal(out, gpu_box(x, k, iso, 3, cuda_dev).cpu())


def test_opcheck(cuda_dev):
    """torch.library.opcheck on admm_hip::fft_admm_tv_box: schema, the fake kernel against the real one,
    autograd registration (none: the op is inference only), AOT dispatch."""
    import admmtor._ops  # noqa: F401
    x, k = bc.make_input(*bc.CASES["pow2_16"][:2])
    one = lambda v: torch.full((1,), v, device=cuda_dev)  # noqa: E731
    b = torch.tensor(BOUNDS, device=cuda_dev)
    for kk in (k.to(cuda_dev), torch.empty(0, device=cuda_dev)):
        torch.library.opcheck(torch.ops.admm_hip.fft_admm_tv_box.default, (x.to(cuda_dev), one(LAM), one(RHO), kk, b, True, 3))
