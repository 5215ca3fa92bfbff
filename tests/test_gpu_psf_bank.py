"""PSF banks on the GPU (ADMM_TV_FLAG_PSF_PER_IMAGE / _PER_CHANNEL; admmtor.eops.deconv.fft_admm_tv_bank and
fft_admm_tv_bank_state): a PSF per image, per channel or per plane in one solve.

Every parity assertion is the project's gate, 1e-5 rel-L2 against the fp64 restatement of tests/bank_cases.py,
which is built from the oracle's pieces per table and carries negative controls: the same solve with the tables
of the wrong planes -- table 0 everywhere, the next plane's, the bank reversed, (b, c) swapped, one index only; on
the Wiener factor alone, on b = H_t(xin) alone, on both -- misses the right one by >= 1e-3 (asserted inside
bank_cases.reference before anything runs here), so a kernel that indexes either table wrongly cannot pass.
The cases are the smallest shapes at which each column-pass kernel and each index can go wrong."""
import ctypes

import pytest
import torch

import bank_cases as bc
from bank_cases import LAM, RHO, TOL_REF64

pytestmark = pytest.mark.gpu

MODE_FLAGS = {"image": 4, "channel": 8, "plane": 12, "shared": 0}
ONE_PER_PATH = ["pow2_16x32", "pow2_1024x32", "smooth_240x480", "gen_15x17", "c4_17x481"]
STATE_CASES = ["pow2_16x32", "smooth_240x480", "gen_15x17"]


def rel(a, b):
    a, b = a.double().reshape(-1).cpu(), b.double().reshape(-1).cpu()
    return ((a - b).norm() / b.norm()).item()


def bank_solve(x, kerns, iso, it, dev):
    from admmtor.eops.deconv import fft_admm_tv_bank
    out = fft_admm_tv_bank(x.to(dev), LAM, RHO, kerns.to(dev), iso, it)
    torch.cuda.synchronize()
    return out.cpu()


def path_of(name, mode, iso, it, state=False):
    from admmtor import _native
    shape, k, _ = bc.CASES[name]
    return _native.path(_native.desc(*shape, k, iso, it, flags=MODE_FLAGS[mode]), mode=2 if state else 0)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name,mode,iso,maxit", bc.PARAMS)
def test_bank_parity(cuda_dev, name, mode, iso, maxit):
    r = bc.reference(name, mode, iso, maxit)
    assert path_of(name, mode, iso, maxit) == bc.CASES[name][2]
    got = bank_solve(r["x"], r["kerns"], iso, maxit, cuda_dev)
    e = rel(got, r["ref"])
    print(name, mode, iso, maxit, f"bank vs fp64 restatement {e:.2e} (weakest control "
          f"{min(r['controls'].values()):.1e})")
    assert e <= TOL_REF64


# ---------------------------------------------------------------- b = H_t(xin) with each plane's PSF
@pytest.mark.parametrize("mode", bc.MODES)
@pytest.mark.parametrize("name", ["pow2_16x32", "smooth_240x480", "gen_15x17"])
def test_psf_transpose_bank(cuda_dev, name, mode):
    """admm_tv_psf_transpose through ctypes: plane (b, c) of the result is apply_psf_transpose with table t."""
    from admmtor import _native
    from oracle.admm_oracle import apply_psf_transpose
    (B, C, H, W), k, _ = bc.CASES[name]
    x = bc.case_input(name)
    kerns = bc.make_bank(mode, B, C, k)
    R = bc.right_map(kerns, B, C)
    tabs = kerns.double().reshape(-1, 1, 1, k, k)
    want = torch.stack([torch.stack([apply_psf_transpose(x[b:b + 1, c:c + 1].double(), tabs[R[b, c]])[0, 0]
                                     for c in range(C)]) for b in range(B)])
    wrong = torch.stack([torch.stack([apply_psf_transpose(x[b:b + 1, c:c + 1].double(), tabs[0])[0, 0]
                                      for c in range(C)]) for b in range(B)])
    assert rel(wrong, want) >= 1e-3  # (the control: table 0 for every plane)
    d = _native.desc(B, C, H, W, k, False, 1, flags=MODE_FLAGS[mode])
    xd, kd = x.to(cuda_dev), kerns.to(cuda_dev).contiguous()
    out = torch.empty_like(xd)
    ws = torch.empty(_native.workspace_size(d), dtype=torch.uint8, device=cuda_dev)
    _native.check(_native.load().admm_tv_psf_transpose(ctypes.byref(d), xd.data_ptr(), kd.data_ptr(), out.data_ptr(),
                                                       ws.data_ptr(), ws.numel(),
                                                       torch.cuda.current_stream(cuda_dev).cuda_stream))
    torch.cuda.synchronize()
    e = rel(out, want)
    print(name, mode, f"H_t with a bank vs the oracle per table {e:.2e}")
    assert e <= TOL_REF64


# ---------------------------------------------------------------- shared-PSF equivalences
@pytest.mark.parametrize("iso", bc.ISOS)
@pytest.mark.parametrize("name", ONE_PER_PATH)
def test_shared_bank_is_fft_admm_tv(cuda_dev, name, iso):
    """A (1, 1, k, k) bank sets no bit: the same native call, the same bits."""
    from admmtor.eops.deconv import fft_admm_tv
    (B, C, H, W), k, _ = bc.CASES[name]
    x = bc.case_input(name).to(cuda_dev)
    kern = bc.make_bank("shared", B, C, k, first=1).to(cuda_dev)
    plain = fft_admm_tv(x, LAM, RHO, kern, iso, 3)
    assert torch.equal(bank_solve(x, kern, iso, 3, cuda_dev), plain.cpu())


@pytest.mark.parametrize("iso", bc.ISOS)
@pytest.mark.parametrize("mode", bc.MODES)
@pytest.mark.parametrize("name", ONE_PER_PATH + ["gen_17x15"])
def test_bank_of_equal_psfs_is_the_shared_solve(cuda_dev, monkeypatch, name, mode, iso):
    """A bank whose tables all hold the same PSF is the shared-PSF solve bit for bit: the tables hold the same
    values and the bank only changes which copy a block reads.  No path reorders anything.

    At H = 17 and at the odd row lengths the shared-PSF solve runs OTHER kernels than a bank (the matrix-core
    column product; the odd-length two-launch iteration; a bank keeps the LDS column pass and the generic
    iteration), so there the bit-for-bit comparison is with the shared-PSF solve on the bank's kernels (the A/B
    build with ADMM_GCOL_MM=0 ADMM_ODD=0).  Against the default shared-PSF solve the two are two fp32 solves
    of different transforms; the 1e-6 meant for a reordered sum holds at H = 17 x 15 but not at 17 x 481
    (measured 1.04e-6, per-image aniso: the odd-length row pass's prime-factor transforms against the generic
    ones), so that comparison carries the gate the project's cross-path tests carry (tests/test_gpu_odd.py):
    twice the reference solve's own error against fp64 plus the bank solve's."""
    from admmtor import _native
    from admmtor.eops.deconv import fft_admm_tv
    from oracle.admm_oracle import solve_fourier
    (B, C, H, W), k, _ = bc.CASES[name]
    x = bc.case_input(name).to(cuda_dev)
    one = bc.make_bank("shared", B, C, k, first=1)
    Bk, Ck = bc.bank_dims(mode, B, C)
    kerns = one.expand(Bk, Ck, k, k).contiguous()
    got = bank_solve(x, kerns, iso, 3, cuda_dev)
    plain = fft_admm_tv(x, LAM, RHO, one.to(cuda_dev), iso, 3).cpu()
    same_kernels = path_of(name, mode, iso, 3) == path_of(name, "shared", iso, 3) and H != 17
    e = rel(got, plain)
    print(name, mode, iso, f"bank of equal PSFs vs shared: {e:.2e}", "bit-identical" if torch.equal(got, plain) else "")
    if same_kernels:
        assert torch.equal(got, plain)
        return
    monkeypatch.setenv("ADMM_GCOL_MM", "0")
    monkeypatch.setenv("ADMM_ODD", "0")
    with _native.ab_library():
        forced = fft_admm_tv(x, LAM, RHO, one.to(cuda_dev), iso, 3).cpu()
    assert torch.equal(got, forced)
    ref = solve_fourier(x.cpu().double(), LAM, RHO, one.double(), iso, 3)
    e_ref, e_plain = rel(got, ref), rel(plain, ref)
    print(name, mode, iso, f"  vs fp64: bank {e_ref:.2e}, default shared-PSF kernels {e_plain:.2e}")
    assert e_ref <= TOL_REF64 and e <= 2 * max(e_plain, 1e-7) + e_ref


# ---------------------------------------------------------------- state
def bank_state(x, kerns, iso, it, dev, state=None):
    from admmtor.eops.deconv import fft_admm_tv_bank_state
    out, st = fft_admm_tv_bank_state(x.to(dev), LAM, RHO, kerns.to(dev), iso, it, state)
    torch.cuda.synchronize()
    return out.cpu(), st


@pytest.mark.parametrize("k1,k2", [(2, 1), (0, 2)])
@pytest.mark.parametrize("iso", bc.ISOS)
@pytest.mark.parametrize("name", STATE_CASES)
def test_bank_state_split(cuda_dev, name, iso, k1, k2):
    """K1 iterations, then K2 from the returned state, are K1 + K2 of the restatement (per-plane bank)."""
    r = bc.reference(name, "plane", iso, 3)  # (asserts the controls of the case)
    x, kerns = r["x"], r["kerns"]
    assert path_of(name, "plane", iso, k2, state=True) == bc.CASES[name][2]
    tables = bc.case_tables(name, "plane")[1]
    ref, _ = bc.restate(x.double(), LAM, RHO, kerns.double(), iso, k1 + k2, tables=tables)
    _, st = bank_state(x, kerns, iso, k1, cuda_dev)
    got, st2 = bank_state(x, kerns, iso, k2, cuda_dev, st)
    e = rel(got, ref)
    print(name, iso, (k1, k2), f"split bank solve vs fp64 {e:.2e}")
    assert e <= TOL_REF64
    assert all(t.dtype == torch.float32 and t.shape == x.shape for t in st2)


@pytest.mark.parametrize("iso", bc.ISOS)
def test_bank_changes_between_calls(cuda_dev, iso):
    """A video: frame 0's kernels for two iterations, then frame 1's from that state -- against the
    restatement doing the same."""
    name = "pow2_16x32"
    (B, C, H, W), k, _ = bc.CASES[name]
    x = bc.case_input(name)
    k0, k1 = bc.make_bank("plane", B, C, k, first=0), bc.make_bank("plane", B, C, k, first=2)
    _, st_ref = bc.restate(x.double(), LAM, RHO, k0.double(), iso, 2)
    ref, _ = bc.restate(x.double(), LAM, RHO, k1.double(), iso, 2, st_ref)
    stale, _ = bc.restate(x.double(), LAM, RHO, k0.double(), iso, 2, st_ref)
    assert rel(stale, ref) >= bc.CONTROL_MIN  # (the control: the second call keeps frame 0's kernels)
    _, st = bank_state(x, k0, iso, 2, cuda_dev)
    got, _ = bank_state(x, k1, iso, 2, cuda_dev, st)
    e = rel(got, ref)
    print(iso, f"bank changed between the calls vs fp64 {e:.2e}")
    assert e <= TOL_REF64


# ---------------------------------------------------------------- iso couples the images
@pytest.mark.parametrize("name", ["pow2_16x32", "smooth_240x480", "gen_15x17"])
def test_iso_bank_keeps_the_coupling_a_loop_loses(cuda_dev, name):
    """The block shrinkage's norm runs over batch and channel: the per-image iso bank solve is not the loop of
    B = 1 iso solves (they differ by more than 1e-3), and it is the restatement."""
    from admmtor.eops.deconv import fft_admm_tv
    r = bc.reference(name, "image", True, 3)
    x, kerns = r["x"], r["kerns"]
    got = bank_solve(x, kerns, True, 3, cuda_dev)
    loop = torch.cat([fft_admm_tv(x[b:b + 1].to(cuda_dev), LAM, RHO, kerns[b:b + 1].to(cuda_dev), True, 3).cpu()
                      for b in range(x.shape[0])])
    e, e_loop = rel(got, r["ref"]), rel(loop, r["ref"])
    print(name, f"iso per-image bank vs fp64 {e:.2e}; the loop of single-image solves {e_loop:.2e}")
    assert e <= TOL_REF64
    assert e_loop > 1e-3 and rel(got, loop) > 1e-3


# ---------------------------------------------------------------- graph capture, op checks, refusals
def test_bank_graph_capture(cuda_dev):
    """A bank solve enqueues only asynchronous work: captured in a HIP graph and replayed, it gives the eager
    result bit for bit."""
    from admmtor.eops.deconv import fft_admm_tv_bank
    name = "pow2_16x32"
    (B, C, H, W), k, _ = bc.CASES[name]
    static_x = bc.case_input(name).to(cuda_dev)
    kerns = bc.make_bank("plane", B, C, k).to(cuda_dev)
    eager = fft_admm_tv_bank(static_x, LAM, RHO, kerns, False, 8)
    s = torch.cuda.Stream(cuda_dev)
    s.wait_stream(torch.cuda.current_stream(cuda_dev))
    with torch.cuda.stream(s):
        fft_admm_tv_bank(static_x, LAM, RHO, kerns, False, 8)
    torch.cuda.current_stream(cuda_dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_out = fft_admm_tv_bank(static_x, LAM, RHO, kerns, False, 8)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, eager)


@pytest.mark.parametrize("mode", bc.MODES)
def test_opcheck_with_a_bank(cuda_dev, mode):
    import admmtor._ops  # noqa: F401
    name = "pow2_16x32"
    (B, C, H, W), k, _ = bc.CASES[name]
    x = bc.case_input(name).to(cuda_dev)
    kerns = bc.make_bank(mode, B, C, k).to(cuda_dev)
    lam, rho = torch.tensor([LAM], device=cuda_dev), torch.tensor([RHO], device=cuda_dev)
    torch.library.opcheck(torch.ops.admm_hip.fft_admm_tv_fwd.default, (x, lam, rho, kerns, True, 3))
    torch.library.opcheck(torch.ops.admm_hip.fft_admm_tv_state.default, (x, lam, rho, kerns, [], False, 3))
    st = [torch.zeros_like(x) for _ in range(4)]
    torch.library.opcheck(torch.ops.admm_hip.fft_admm_tv_state.default, (x, lam, rho, kerns, st, True, 2))


def test_bank_refuses_grad_and_fp64(cuda_dev):
    from admmtor.eops.deconv import fft_admm_tv_bank, fft_admm_tv_bank_state
    x = bc.case_input("pow2_16x16").to(cuda_dev)
    kerns = bc.make_bank("plane", 2, 3, 5).to(cuda_dev)
    for f in (fft_admm_tv_bank, fft_admm_tv_bank_state):
        with pytest.raises(RuntimeError, match="inference only"):
            f(x.clone().requires_grad_(True), LAM, RHO, kerns, False, 2)
        with pytest.raises(RuntimeError, match="inference only"):
            f(x, LAM, RHO, kerns.clone().requires_grad_(True), False, 2)
        with pytest.raises(NotImplementedError, match="fp32"):
            f(x.double(), LAM, RHO, kerns.double(), False, 2)
        with torch.no_grad():  # under no_grad an input that requires grad is accepted, as by fft_admm_tv_state
            f(x.clone().requires_grad_(True), LAM, RHO, kerns, False, 1)
    with pytest.raises(NotImplementedError, match="inference only"):
        torch.ops.admm_hip.fft_admm_tv_fwd_train(x, torch.tensor([LAM], device=cuda_dev),
                                                 torch.tensor([RHO], device=cuda_dev), kerns, False, 2, False)
