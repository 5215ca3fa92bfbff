"""CPU side of the solver-state feature (admm_tv_forward_state): the fp64 restatement the GPU tests check
against (tests/state_cases.py) is pinned to the oracle, the negative controls hold for every GPU case, and the
new C entry points answer their host-only questions (symbols, error codes, workspace size, path)."""
import ctypes

import pytest
import torch

import state_cases as sc
from oracle.admm_oracle import rel_l2, solve_fourier, solve_spatial

PIN_INPUTS = [((2, 3, 16, 16), ("gauss:1.0", 5)), ((1, 2, 15, 17), ("motion", 5)), ((1, 2, 32, 64), None)]


@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("shape,psf", PIN_INPUTS)
def test_restatement_equals_the_oracle_and_splits_exactly(shape, psf, iso):
    """From the zero state the restatement is solve_spatial and solve_fourier; K1 then K2 iterations are
    K1 + K2 (1e-12: fp64 rounding, measured <= 2.7e-15), also with the state rounded to fp32 in between
    (1e-7: fp32's 6e-8 relative rounding of the state, measured <= 5.8e-9); every wrong state misses by >= 1e-4
    (measured 3.9e-4 .. 3.3e-1)."""
    x, k = sc.make_input(shape, psf)
    xd, kd = x.double(), k.double()
    for k1, k2 in [(5, 1), (5, 2), (6, 3), (1, 1)]:
        n = k1 + k2
        whole, st = sc.restate(xd, sc.LAM, sc.RHO, kd, iso, n)
        assert rel_l2(whole, solve_spatial(xd, sc.LAM, sc.RHO, kd, iso, n)) <= 1e-12
        ref = solve_fourier(xd, sc.LAM, sc.RHO, kd, iso, n)
        assert rel_l2(whole, ref) <= 1e-12
        _, st1 = sc.restate(xd, sc.LAM, sc.RHO, kd, iso, k1)
        split, st2 = sc.restate(xd, sc.LAM, sc.RHO, kd, iso, k2, st1)
        e_split = rel_l2(split, ref)
        assert e_split <= 1e-12
        assert max(rel_l2(a, b) for a, b in zip(st2, st) if b.abs().max() > 0) <= 1e-12
        e32 = rel_l2(sc.restate(xd, sc.LAM, sc.RHO, kd, iso, k2, tuple(t.float() for t in st1))[0], ref)
        assert e32 <= 1e-7
        worst = {w: rel_l2(sc.restate(xd, sc.LAM, sc.RHO, kd, iso, k2, bad)[0], ref)
                 for w, bad in sc.wrong_states(st1).items()}
        print(shape, psf, iso, (k1, k2), f"split {e_split:.1e} fp32 state {e32:.1e} controls",
              {w: f"{v:.1e}" for w, v in worst.items()})
        assert min(worst.values()) >= sc.CONTROL_MIN, worst


def test_restatement_zero_iterations():
    x, k = sc.make_input((1, 2, 15, 17), ("motion", 5))
    _, st = sc.restate(x.double(), sc.LAM, sc.RHO, k.double(), False, 3)
    out, same = sc.restate(x.double(), sc.LAM, sc.RHO, k.double(), False, 0, st)
    assert not out.any() and all(torch.equal(a, b) for a, b in zip(same, st))


@pytest.mark.parametrize("name,iso,k1,k2", sc.PARAMS)
def test_gpu_cases_have_teeth(name, iso, k1, k2):
    """Every case of tests/test_gpu_state.py: the split restatement is the unsplit solve, and each negative
    control misses it by >= 1e-4 (asserted inside state_cases.reference)."""
    r = sc.reference(name, iso, k1, k2)
    assert (k1 == 0) == (not r["controls"])


# ---------------------------------------------------------------- the C entry points, host only
def test_state_entry_points_host():
    from admmtor import _native
    lib = _native.load()
    assert lib.admm_tv_abi_version() == 7
    assert {"admm_tv_forward_state", "admm_tv_state_workspace_size"} <= set(_native.EXPORTED)
    assert lib.admm_tv_forward_state is not None and lib.admm_tv_state_workspace_size is not None
    n = ctypes.c_size_t(0)
    for shape, k, iso in (((64, 3, 1024, 1024), 21, False), ((2, 3, 240, 480), 7, True), ((1, 2, 15, 17), 5, True),
                          ((1, 2, 17, 481), 5, False), ((1, 2, 481, 17), 5, False), ((2, 1, 1, 7), 0, True)):
        d = _native.desc(*shape, k, iso, 10)
        assert _native.state_workspace_size(d) >= _native.workspace_size(d)

    def call(d, st_in=None, st_out=None):
        one = ctypes.c_void_p(256)  # never dereferenced: every call here is refused before any device work
        return lib.admm_tv_forward_state(ctypes.byref(d), one, one, one, one, st_in, st_out, one, one, 1 << 40, None)

    grouped = _native.desc(1, 2, 64, 64, 3, False, 5, groups=2)
    assert call(grouped) == _native.ADMM_TV_EUNSUPPORTED and b"groups" in lib.admm_tv_last_error()
    assert lib.admm_tv_state_workspace_size(ctypes.byref(grouped), ctypes.byref(n)) == _native.ADMM_TV_EUNSUPPORTED
    assert lib.admm_tv_path(ctypes.byref(grouped), 2) == _native.ADMM_TV_EUNSUPPORTED
    # more than 2^31 - 1 image rows: the call, the size query and the path query refuse alike (the plain solve's
    # size query does not)
    rows = _native.desc(1 << 20, 1 << 11, 1, 7, 0, False, 5)
    assert call(rows) == _native.ADMM_TV_EUNSUPPORTED and b"rows" in lib.admm_tv_last_error()
    assert lib.admm_tv_state_workspace_size(ctypes.byref(rows), ctypes.byref(n)) == _native.ADMM_TV_EUNSUPPORTED
    assert lib.admm_tv_path(ctypes.byref(rows), 2) == _native.ADMM_TV_EUNSUPPORTED
    assert lib.admm_tv_workspace_size(ctypes.byref(rows), ctypes.byref(n)) == 0
    hooked = _native.desc(1, 2, 64, 64, 3, True, 5)
    hooked.allreduce = _native.ALLREDUCE_FN(lambda *a: None)
    assert call(hooked) == _native.ADMM_TV_EUNSUPPORTED and b"hook" in lib.admm_tv_last_error()
    assert call(_native.desc(1, 2, 64, 64, 3, False, 5, f64=True)) == _native.ADMM_TV_EINVAL
    assert b"F64" in lib.admm_tv_last_error()
    assert call(_native.desc(1, 2, 64, 64, 3, False, 5, flags=_native.ADMM_TV_FLAG_PSF_GRAD)) == _native.ADMM_TV_EINVAL
    ok = _native.desc(1, 2, 64, 64, 3, False, 5)
    full = _native.AdmmTvState(256, 256, 256, 256)
    for hole in ("zx", "zy", "ux", "uy"):
        st = _native.AdmmTvState(256, 256, 256, 256)
        setattr(st, hole, None)
        assert call(ok, ctypes.byref(st), ctypes.byref(full)) == _native.ADMM_TV_EINVAL
        assert call(ok, None, ctypes.byref(st)) == _native.ADMM_TV_EINVAL
        assert b"null member" in lib.admm_tv_last_error()


def test_state_op_fake_kernel_and_host_refusals():
    """admm_hip::fft_admm_tv_state has a fake kernel (five tensors shaped like x, with or without a state) and
    no CPU kernel; the wrapper refuses fp64 and inputs that require grad before it looks for a device."""
    import admmtor._ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    from admmtor.eops.deconv import fft_admm_tv_state
    with FakeTensorMode():
        x, one, k = torch.empty(2, 3, 64, 32), torch.empty(1), torch.empty(1, 1, 5, 5)
        for state in ([], [torch.empty_like(x) for _ in range(4)]):
            outs = torch.ops.admm_hip.fft_admm_tv_state(x, one, one, k, state, True, 10)
            assert len(outs) == 5 and all(o.shape == x.shape and o.dtype == x.dtype for o in outs)
    x = torch.rand(1, 1, 16, 16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        torch.ops.admm_hip.fft_admm_tv_state(x, torch.ones(1), torch.ones(1), torch.empty(0), [], False, 2)
    with pytest.raises(NotImplementedError):
        fft_admm_tv_state(x.double(), 0.01, 0.02, torch.empty(0, dtype=torch.float64), False, 2)
    with pytest.raises(RuntimeError, match="fft_admm_tv is the differentiable call"):
        fft_admm_tv_state(x.clone().requires_grad_(True), 0.01, 0.02, torch.empty(0), False, 2)


def test_state_path_per_size_class():
    """admm_tv_path(desc, 2): fused at power-of-two and smooth sizes; the generic loop elsewhere, the odd row
    lengths included (admm_tv_forward runs them on the odd-length row pass, which carries no state)."""
    from admmtor import _native
    want = {(64, 64): "fused", (32, 1024): "fused", (240, 480): "fused mixed-radix", (1080, 1920): "fused mixed-radix",
            (15, 17): "generic", (1, 7): "generic", (17, 481): "generic", (481, 17): "generic"}
    for (H, W), path in want.items():
        for iso in (False, True):
            assert _native.path(_native.desc(1, 2, H, W, 0, iso, 5), mode=2) == path, (H, W, iso)
    # modes 0 and 1 are what they were
    d = _native.desc(1, 2, 17, 481, 0, False, 5)
    assert _native.path(d) == _native.path(d, mode=0) == "fused odd-length" and _native.path(d, train=True) == "generic"
