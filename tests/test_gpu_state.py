"""Solver state across calls on the GPU (admm_tv_forward_state; admmtor.eops.deconv.fft_admm_tv_state and
fft_admm_tv_until): resume, warm start, stop on a tolerance.

Every parity assertion is the project's gate, 1e-5 rel-L2 against the fp64 oracle (TOL_REF64).  The cases
continue for K2 in {1, 2, 3} iterations only and carry negative controls (tests/state_cases.py: a continuation
from any of six wrong states misses the oracle by >= 1e-4), so a state that is not the reference's (z, u)
cannot pass.  Tests 2 and 3 hand the state across the GPU / fp64-restatement boundary in both directions:
the tensors are the reference's z_x, z_y, u_x, u_y, not an internal representation."""
import ctypes

import pytest
import torch

import state_cases as sc
from state_cases import LAM, RHO, TOL_REF64

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.double().reshape(-1).cpu(), b.double().reshape(-1).cpu()
    return ((a - b).norm() / b.norm()).item()


def kern_on(k, dev):
    return k.to(dev) if k.numel() else torch.empty(0, device=dev)


def gpu_state(x, k, iso, it, dev, state=None, lam=LAM, rho=RHO):
    from admmtor.eops.deconv import fft_admm_tv_state
    out, st = fft_admm_tv_state(x.to(dev), lam, rho, kern_on(k, dev), iso, it, state)
    torch.cuda.synchronize()
    return out.cpu(), st


def to_state(st, dev):
    from admmtor.eops.deconv import ADMMState
    return ADMMState(*(t.float().to(dev) for t in st))


def check_path(name, shape, k, iso):
    from admmtor import _native
    kk = int(k.shape[-1]) if k.numel() else 0
    path = _native.path(_native.desc(*shape, kk, iso, 5), mode=2)
    if sc.CASES[name][3]:
        assert path in ("fused", "fused mixed-radix"), path
    else:
        assert path == "generic", path


# ---------------------------------------------------------------- 1: split equals unsplit
@pytest.mark.parametrize("name,iso,k1,k2", sc.PARAMS)
def test_split_equals_unsplit(cuda_dev, name, iso, k1, k2):
    from admmtor.eops.deconv import fft_admm_tv
    r = sc.reference(name, iso, k1, k2)
    x, k = r["x"], r["k"]
    check_path(name, tuple(x.shape), k, iso)
    _, st = gpu_state(x, k, iso, k1, cuda_dev)
    got, _ = gpu_state(x, k, iso, k2, cuda_dev, st)
    plain = fft_admm_tv(x.to(cuda_dev), LAM, RHO, kern_on(k, cuda_dev), iso, k1 + k2).cpu()
    e_ref, e_plain, e_split = rel(got, r["ref"]), rel(plain, r["ref"]), rel(got, plain)
    print(name, iso, (k1, k2), f"split vs fp64 {e_ref:.2e}, plain vs fp64 {e_plain:.2e}, split vs plain {e_split:.2e}")
    assert e_ref <= TOL_REF64
    assert e_split <= 2 * max(e_plain, 1e-7) + e_ref


# ---------------------------------------------------------------- 2: the exported state is the reference's
@pytest.mark.parametrize("name,iso,k1,k2", sc.PARAMS)
def test_state_out_continued_in_fp64(cuda_dev, name, iso, k1, k2):
    r = sc.reference(name, iso, k1, k2)
    x, k = r["x"], r["k"]
    _, st = gpu_state(x, k, iso, k1, cuda_dev)
    assert all(t.dtype == torch.float32 and t.shape == x.shape and not t.requires_grad for t in st)
    cont, _ = sc.restate(x.double(), LAM, RHO, k.double(), iso, k2, tuple(t.cpu().double() for t in st))
    e = rel(cont, r["ref"])
    print(name, iso, (k1, k2), f"GPU state after {k1}, fp64 for {k2} more: {e:.2e} (controls >= "
          f"{min(r['controls'].values(), default=float('nan')):.1e})")
    assert e <= TOL_REF64


# ---------------------------------------------------------------- 3: the imported state is the reference's
@pytest.mark.parametrize("name,iso,k1,k2", sc.PARAMS)
def test_state_in_from_fp64(cuda_dev, name, iso, k1, k2):
    r = sc.reference(name, iso, k1, k2)
    x, k = r["x"], r["k"]
    got, _ = gpu_state(x, k, iso, k2, cuda_dev, to_state(r["state1"], cuda_dev))
    e = rel(got, r["ref"])
    print(name, iso, (k1, k2), f"fp64 state after {k1} (cast to fp32), GPU for {k2} more: {e:.2e}")
    assert e <= TOL_REF64


# ---------------------------------------------------------------- 4: edges
def raw_call(x, k, iso, it, st_in, st_out, lam=LAM, rho=RHO, out=None):
    """admm_tv_forward_state through ctypes on device tensors; st_in / st_out: lists of four tensors or None;
    out: the tensor to solve into (default: a new one)."""
    from admmtor import _native
    dev = x.device
    B, C, H, W = x.shape
    d = _native.desc(B, C, H, W, int(k.shape[-1]) if k.numel() else 0, iso, it)
    ws = torch.empty(_native.state_workspace_size(d), dtype=torch.uint8, device=dev)
    lam_t, rho_t = torch.full((1,), lam, device=dev), torch.full((1,), rho, device=dev)
    out = torch.empty_like(x) if out is None else out
    si = _native.state_of(*st_in) if st_in is not None else None
    so = _native.state_of(*st_out) if st_out is not None else None
    _native.check(_native.load().admm_tv_forward_state(
        d, x.data_ptr(), k.data_ptr() if k.numel() else None, lam_t.data_ptr(), rho_t.data_ptr(),
        ctypes.byref(si) if si is not None else None, ctypes.byref(so) if so is not None else None,
        out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return out


EDGE_CASES = [("pow2_16_lanepaired", False), ("pow2_16_lanepaired", True), ("smooth_240x480", False),
              ("generic_15x17", True)]


@pytest.mark.parametrize("name,iso", EDGE_CASES)
def test_zero_iterations_pass_the_state_through(cuda_dev, name, iso):
    x, k = sc.make_input(*sc.CASES[name][:2])
    _, st = gpu_state(x, k, iso, 3, cuda_dev)
    out, same = gpu_state(x, k, iso, 0, cuda_dev, st)
    assert not out.any() and all(torch.equal(a, b) for a, b in zip(same, st))
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(same, st))  # new tensors
    out, zeros = gpu_state(x, k, iso, 0, cuda_dev)
    assert not out.any() and not any(t.any() for t in zeros)


@pytest.mark.parametrize("name,iso", EDGE_CASES)
def test_state_out_only_and_aliasing_through_the_c_abi(cuda_dev, name, iso):
    """state_in NULL starts from the reference's zeros (the exported state, continued in fp64, meets the
    gate); state_out NULL is allowed; state_in == state_out (in place) equals the out-of-place result bit for
    bit; two identical calls are bit-identical."""
    r = sc.reference(name, iso, 5, 1)
    x, k = r["x"].to(cuda_dev), kern_on(r["k"], cuda_dev)
    st = [torch.empty_like(x) for _ in range(4)]
    x5 = raw_call(x, k, iso, 5, None, st)
    cont, _ = sc.restate(r["x"].double(), LAM, RHO, r["k"].double(), iso, 1, tuple(t.cpu().double() for t in st))
    assert rel(cont, r["ref"]) <= TOL_REF64
    assert torch.equal(raw_call(x, k, iso, 5, None, None), x5)  # no state wanted: the same x
    oop = [torch.empty_like(x) for _ in range(4)]
    x_oop = raw_call(x, k, iso, 2, st, oop)
    again = [torch.empty_like(x) for _ in range(4)]
    assert torch.equal(raw_call(x, k, iso, 2, st, again), x_oop)
    assert all(torch.equal(a, b) for a, b in zip(again, oop))
    inplace = [t.clone() for t in st]
    x_in = raw_call(x, k, iso, 2, inplace, inplace)
    assert torch.equal(x_in, x_oop) and all(torch.equal(a, b) for a, b in zip(inplace, oop))


# ---------------------------------------------------------------- 5: a new frame, new parameters
@pytest.mark.parametrize("shape,psf", [((1, 2, 16, 16), ("gauss:1.0", 5)), ((1, 2, 240, 480), ("motion", 7))])
@pytest.mark.parametrize("iso", [False, True])
def test_new_frame_and_new_rho(cuda_dev, shape, psf, iso):
    from admmtor.synth import blurred_batch, make_psf
    k = make_psf(*psf)
    xa, xb = blurred_batch(*shape, k, seed=3), blurred_batch(*shape, k, seed=4)
    _, st_gpu = gpu_state(xa, k, iso, 5, cuda_dev)
    _, st_ref = sc.restate(xa.double(), LAM, RHO, k.double(), iso, 5)
    for what, frame, rho in (("frame B", xb, RHO), ("rho 0.05", xa, 0.05)):
        got, _ = gpu_state(frame, k, iso, 2, cuda_dev, st_gpu, rho=rho)
        want, _ = sc.restate(frame.double(), LAM, rho, k.double(), iso, 2, st_ref)
        cold, _ = sc.restate(frame.double(), LAM, rho, k.double(), iso, 2)
        e, e_cold = rel(got, want), rel(cold, want)
        print(shape, iso, what, f"{e:.2e} (the same two iterations from zero: {e_cold:.2e})")
        assert e_cold >= sc.CONTROL_MIN  # teeth: the carried state matters to the result
        assert e <= TOL_REF64


# ---------------------------------------------------------------- 6: graph capture
@pytest.mark.parametrize("iso", [False, True])
def test_state_graph_capture(cuda_dev, iso):
    """A stateful solve enqueues only asynchronous work: captured in a HIP graph and replayed, it gives the
    eager x and state bit for bit."""
    from admmtor.eops.deconv import fft_admm_tv_state
    x, k = sc.make_input((2, 3, 16, 16), ("gauss:1.0", 5))
    sx, k = x.to(cuda_dev), k.to(cuda_dev)
    _, st0 = fft_admm_tv_state(sx, LAM, RHO, k, iso, 4)
    eager_x, eager_st = fft_admm_tv_state(sx, LAM, RHO, k, iso, 3, st0)
    s = torch.cuda.Stream(cuda_dev)
    s.wait_stream(torch.cuda.current_stream(cuda_dev))
    with torch.cuda.stream(s):
        fft_admm_tv_state(sx, LAM, RHO, k, iso, 3, st0)
    torch.cuda.current_stream(cuda_dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_x, static_st = fft_admm_tv_state(sx, LAM, RHO, k, iso, 3, st0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_x, eager_x) and all(torch.equal(a, b) for a, b in zip(static_st, eager_st))


# ---------------------------------------------------------------- 7: stop on a tolerance
@pytest.mark.parametrize("iso", [False, True])
def test_until_stops_where_the_fp64_criterion_does(cuda_dev, iso):
    from admmtor.eops.deconv import fft_admm_tv_until
    from oracle.admm_oracle import solve_fourier
    x, k = sc.make_input((1, 3, 32, 32), ("gauss:1.0", 5))
    xd, kd = x.double(), k.double()
    every, chunks = 5, 12
    crit, prev, st = [], torch.zeros_like(xd), None
    for _ in range(chunks):  # c_j = ||x_j - x_{j-1}|| / ||x_j|| after chunk j, in fp64
        cur, st = sc.restate(xd, LAM, RHO, kd, iso, every, st)
        crit.append(((cur - prev).norm() / cur.norm()).item())
        prev = cur
    # tol between two consecutive chunk values at least 10 % apart (fp32 cannot land on the other side), all
    # earlier values above it; the last such pair, so that the run spans several chunks
    j = max(j for j in range(1, chunks) if crit[j - 1] / crit[j] >= 1.1 and min(crit[:j]) > (crit[j - 1] * crit[j]) ** 0.5)
    tol = (crit[j - 1] * crit[j]) ** 0.5
    got, state, its = fft_admm_tv_until(x.to(cuda_dev), LAM, RHO, k.to(cuda_dev), iso, tol=tol, check_every=every,
                                        maxit=every * chunks + 3)
    print(iso, "criterion per chunk", [f"{c:.2e}" for c in crit], "tol", f"{tol:.2e}", "stopped after", its)
    assert its == (j + 1) * every
    assert rel(got, solve_fourier(xd, LAM, RHO, kd, iso, its)) <= TOL_REF64
    more, _ = gpu_state(x, k, iso, 2, cuda_dev, state)  # the returned state continues the solve
    assert rel(more, solve_fourier(xd, LAM, RHO, kd, iso, its + 2)) <= TOL_REF64
    got, _, its = fft_admm_tv_until(x.to(cuda_dev), LAM, RHO, k.to(cuda_dev), iso, tol=0.0, check_every=4, maxit=10)
    assert its == 10 and rel(got, solve_fourier(xd, LAM, RHO, kd, iso, 10)) <= TOL_REF64
    # host inputs: staged once, x back on the host, the state on the device, the same bits
    host, hstate, its = fft_admm_tv_until(x, LAM, RHO, k, iso, tol=0.0, check_every=4, maxit=10)
    assert its == 10 and not host.is_cuda and all(t.is_cuda for t in hstate) and torch.equal(host, got.cpu())


# ---------------------------------------------------------------- pointers that are only float-aligned
def at_offset(t, off):
    """A contiguous copy of t that starts `off` floats into its allocation."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


ALIGN_CASES = [("pow2_16_lanepaired", False), ("pow2_16_lanepaired", True), ("pow2_1024_lanepaired", True),
               ("pow2_1024_plain_pixel", False), ("pow2_1024_coop_pixel", False), ("smooth_240x480", True),
               ("generic_15x17", False)]


@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("name,iso", ALIGN_CASES)
def test_state_at_an_odd_float_offset(cuda_dev, name, iso, off):
    """The state images, xin and out need only be float-aligned: with every one of them `off` floats into its
    allocation (4- or 8-byte aligned: one or two pixels per thread, not four) the solve gives the bits it gives
    on aligned tensors, on the lane-paired and the pixel-order routes alike."""
    x, k = sc.make_input(*sc.CASES[name][:2])
    x, k = x.to(cuda_dev), kern_on(k, cuda_dev)
    st = [torch.empty_like(x) for _ in range(4)]
    raw_call(x, k, iso, 3, None, st)
    want_st = [torch.empty_like(x) for _ in range(4)]
    want = raw_call(x, k, iso, 2, st, want_st)
    xo, sto = at_offset(x, off), [at_offset(t, off) for t in st]
    got_st = [at_offset(torch.zeros_like(x), off) for _ in range(4)]
    got = raw_call(xo, k, iso, 2, sto, got_st, out=at_offset(torch.zeros_like(x), off))
    assert all(t.data_ptr() % 16 == 4 * off for t in (xo, got, *sto, *got_st))
    assert torch.equal(got, want) and all(torch.equal(a, b) for a, b in zip(got_st, want_st))
    first_st = [at_offset(torch.zeros_like(x), off) for _ in range(4)]  # ... and from no state (export only)
    raw_call(xo, k, iso, 3, None, first_st, out=at_offset(torch.zeros_like(x), off))
    assert all(torch.equal(a, b) for a, b in zip(first_st, st))


def test_state_views_at_an_odd_offset_through_python(cuda_dev):
    """Contiguous views at an odd element offset pass every check of the wrapper: they must give the same x."""
    from admmtor.eops.deconv import ADMMState, fft_admm_tv_state
    x, k = sc.make_input((2, 3, 16, 16), ("gauss:1.0", 5))
    x, k = x.to(cuda_dev), k.to(cuda_dev)
    for iso in (False, True):
        _, st = fft_admm_tv_state(x, LAM, RHO, k, iso, 3)
        buf = torch.empty(4 * x.numel() + 1, device=cuda_dev)
        views = buf[1:].view(4, *x.shape)
        views.copy_(torch.stack(list(st)))
        assert all(v.is_contiguous() and v.data_ptr() % 8 == 4 for v in views)
        a, sa = fft_admm_tv_state(x, LAM, RHO, k, iso, 2, ADMMState(*views))
        b, sb = fft_admm_tv_state(x, LAM, RHO, k, iso, 2, st)
        assert torch.equal(a, b) and all(torch.equal(p, q) for p, q in zip(sa, sb))


# ---------------------------------------------------------------- past 2^31 pixels
def test_state_past_2_31_pixels(cuda_dev):
    """One stateful chain (2 + 2 iterations, the state updated in place) over more than 2^31 pixels: the state
    kernels index in 64 bits.  Distinct noise planes (a plane read through a wrapped 32-bit offset could not pass
    as its neighbour); around the plane holding element 2^31 and at the end of the batch, x and the state equal
    the same planes' chain in a small batch bit for bit (aniso planes are independent), and x meets the fp64
    gate.  In place, the chain holds x, out and one state next to the workspace: the memory the plain solve's
    test of this size asks for (tests/test_gpu_large.py), so the two run or skip together."""
    from admmtor.synth import make_psf
    from oracle.admm_oracle import solve_fourier
    P, H, W = 2100, 1024, 1024
    assert P * H * W > 2 ** 31
    free, _ = torch.cuda.mem_get_info(cuda_dev)
    if free < 140e9:
        pytest.skip(f"needs ~125 GB of free device memory, {free / 1e9:.0f} GB free")
    psf = make_psf("gauss:1.5", 9).to(cuda_dev)
    g = torch.Generator(device=cuda_dev).manual_seed(11)
    x = torch.rand((P // 3, 3, H, W), generator=g, device=cuda_dev)
    st = [torch.empty_like(x) for _ in range(4)]
    out = raw_call(x, psf, False, 2, None, st)
    raw_call(x, psf, False, 2, st, st, out=out)
    b31 = 2 ** 31 // (H * W)  # the plane holding element 2^31
    for p0 in ((b31 - 2) // 2 * 2, P - 6):
        xs = x.reshape(P, H, W)[p0:p0 + 6].reshape(2, 3, H, W).contiguous()
        s = [torch.empty_like(xs) for _ in range(4)]
        raw_call(xs, psf, False, 2, None, s)
        small = raw_call(xs, psf, False, 2, s, s)
        assert torch.equal(small.reshape(6, H, W), out.reshape(P, H, W)[p0:p0 + 6]), p0
        for a, b in zip(s, st):
            assert torch.equal(a.reshape(6, H, W), b.reshape(P, H, W)[p0:p0 + 6]), p0
    for p in (b31, P - 1):
        xp = x.reshape(P, H, W)[p].reshape(1, 1, H, W).double().cpu()
        e = rel(out.reshape(P, H, W)[p].reshape(1, 1, H, W), solve_fourier(xp, LAM, RHO, psf.double().cpu(), False, 4))
        print(f"{P}x{H}x{W} plane {p}: stateful 2 + 2 vs fp64 oracle {e:.2e}")
        assert e <= TOL_REF64
    del out, st, x
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 8: errors
def test_state_errors(cuda_dev):
    from admmtor.eops.deconv import ADMMState, fft_admm_tv_state
    x, k = sc.make_input((1, 2, 16, 16), ("gauss:1.0", 5))
    x, k = x.to(cuda_dev), k.to(cuda_dev)
    _, st = fft_admm_tv_state(x, LAM, RHO, k, False, 2)
    with pytest.raises(ValueError):
        fft_admm_tv_state(x, LAM, RHO, k, False, 2, st._replace(u_x=st.u_x[:, :1]))
    with pytest.raises(ValueError):
        fft_admm_tv_state(x, LAM, RHO, k, False, 2, st._replace(z_y=st.z_y.double()))
    with pytest.raises(ValueError):
        fft_admm_tv_state(x, LAM, RHO, k, False, 2, st._replace(z_x=st.z_x.cpu()))
    with pytest.raises(ValueError):
        fft_admm_tv_state(x, LAM, RHO, k, False, 2, tuple(st)[:3])
    with pytest.raises(NotImplementedError):
        fft_admm_tv_state(x.double(), LAM, RHO, k.double(), False, 2)
    with pytest.raises(RuntimeError, match="fft_admm_tv"):
        fft_admm_tv_state(x.clone().requires_grad_(True), LAM, RHO, k, False, 2)
    with pytest.raises(RuntimeError, match="fft_admm_tv"):
        fft_admm_tv_state(x, torch.tensor([LAM], device=cuda_dev, requires_grad=True), RHO, k, False, 2)
    with torch.no_grad():  # ... and fine where no graph is being recorded
        out, st2 = fft_admm_tv_state(x.clone().requires_grad_(True), LAM, RHO, k, False, 2)
    assert not out.requires_grad and not any(t.requires_grad for t in st2)
    # non-contiguous state tensors are made contiguous
    nc = ADMMState(*(t.transpose(-1, -2).contiguous().transpose(-1, -2) for t in st))
    assert not nc.z_x.is_contiguous()
    a, _ = fft_admm_tv_state(x, LAM, RHO, k, False, 2, nc)
    b, _ = fft_admm_tv_state(x, LAM, RHO, k, False, 2, st)
    assert torch.equal(a, b)
