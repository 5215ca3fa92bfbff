"""CPU side of the solve with bounds on x (admm_tv_forward_box): the fp64 restatement the GPU tests check
against (tests/box_cases.py) is pinned to the oracle, the negative controls hold for every GPU case, the
iteration converges into the bounds, and the new C entry points and the Python wrapper answer their host-only
questions (symbols, refusals, workspace size, path, input checks, the op's fake kernel)."""
import ctypes
import os
import re

import pytest
import torch

import box_cases as bc
from conftest import ROOT
from oracle.admm_oracle import rel_l2, solve_fourier

INF = float("inf")
PIN_INPUTS = [((2, 3, 16, 16), ("gauss:1.0", 5)), ((1, 2, 15, 17), ("motion", 5)), ((2, 1, 1, 7), None)]


@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("shape,psf", PIN_INPUTS)
def test_restatement_without_the_box_is_the_oracle(shape, psf, iso):
    """restate_box(box=False) is solve_fourier (1e-12: fp64 rounding, measured <= 2.8e-15), so everything the
    restatement shares with the reference's loop is the oracle's.  With the box and infinite bounds it is NOT:
    rho x_k stays in the right-hand side (a proximal-point variant with the same limit)."""
    x, k = bc.make_input(shape, psf)
    xd, kd = x.double(), k.double()
    for K in bc.KS:
        ref = solve_fourier(xd, bc.LAM, bc.RHO, kd, iso, K)
        assert rel_l2(bc.restate_box(xd, bc.LAM, bc.RHO, kd, iso, K, *bc.BOUNDS, box=False), ref) <= 1e-12
    free = rel_l2(bc.restate_box(xd, bc.LAM, bc.RHO, kd, iso, 6, -INF, INF), solve_fourier(xd, bc.LAM, bc.RHO, kd, iso, 6))
    print(shape, psf, iso, f"infinite bounds vs solve_fourier at K = 6: {free:.1e}")  # 1.5e-5 (one row) .. 4e-2
    assert free > 1e-12  # the measure of "equal" above


def test_restatement_zero_iterations():
    x, k = bc.make_input((1, 2, 15, 17), ("motion", 5))
    assert not bc.restate_box(x.double(), bc.LAM, bc.RHO, k.double(), False, 0, *bc.BOUNDS).any()


@pytest.mark.parametrize("name,iso", bc.CASE_PARAMS)
def test_gpu_cases_have_teeth(name, iso):
    """Every case of tests/test_gpu_box.py: each of the seven wrong variants misses the restatement by >= 1e-4 at
    K = 3 and K = 6, and the projection is active on 5 % .. 95 % of the pixels in every iteration (asserted
    inside box_cases.teeth; measured: weakest control 1.9e-3 at K = 3 and 4.3e-3 at K = 6, both "upper bound
    ignored" on the one-row case; shares 50 % .. 75 %)."""
    c = bc.teeth(name, iso)
    r = bc.reference(name, iso, 6)
    print(name, iso, "active", [f"{a:.2f}" for a in r["active"]], {w: {K: f"{e:.1e}" for K, e in v.items()} for w, v in c.items()})
    assert set(c) == set(bc.WRONG) and all(set(v) == set(bc.CONTROL_KS) for v in c.values())


@pytest.mark.parametrize("name", ["pow2_16", "generic_15x17"])
def test_iteration_converges_into_the_bounds(name):
    """x_K is not clamped, but it approaches the feasible set: at rho = 0.5 after 400 iterations no pixel is
    farther than 1e-4 from [lo, hi] (measured 2.0e-6 and 2.4e-9)."""
    x, k = bc.make_input(*bc.CASES[name][:2])
    xk = bc.restate_box(x.double(), bc.LAM, 0.5, k.double(), False, 400, *bc.BOUNDS)
    d = (xk - xk.clamp(*bc.BOUNDS)).abs().max().item()
    print(name, f"max |x - clamp(x)| = {d:.1e}")
    assert d <= 1e-4


@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("name", ["pow2_16", "generic_15x17"])
def test_default_bounds_are_active(name, iso):
    """With the defaults (0, +inf) the constraint binds on the project's own inputs: in iteration 6 at least
    2 % of the pixels have p < 0 (measured 2.4 % .. 7.1 %)."""
    a = bc.restated(name, iso, 0.0, INF)["active"]
    print(name, iso, [f"{v:.3f}" for v in a])
    assert a[5] >= 0.02


# ---------------------------------------------------------------- the C entry points, host only
def test_box_symbols_header_binding_library():
    from admmtor import _native
    new = {"admm_tv_box_workspace_size", "admm_tv_forward_box"}
    assert new <= set(_native.EXPORTED)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "admm_tv.h")).read(), flags=re.S)
    assert new <= set(re.findall(r"\b(admm_tv_\w+)\s*\(", txt))
    lib = _native.load()
    assert lib.admm_tv_abi_version() == 7  # additive: the ABI version stays
    assert lib.admm_tv_box_workspace_size is not None and lib.admm_tv_forward_box is not None


def _entry_points(lib):
    from admmtor import _native  # noqa: F401
    n = ctypes.c_size_t(0)
    one = ctypes.c_void_p(256)  # never dereferenced: every call here is refused before any device work

    def call(d, bounds=one):
        return lib.admm_tv_forward_box(ctypes.byref(d), one, one, one, one, bounds, one, one, 1 << 40, None)

    def size(d):
        return lib.admm_tv_box_workspace_size(ctypes.byref(d), ctypes.byref(n))

    def path(d):
        return lib.admm_tv_path(ctypes.byref(d), 3)
    return call, size, path


def test_box_refusals_by_all_three_entry_points():
    from admmtor import _native
    lib = _native.load()
    entries = _entry_points(lib)
    hooked = _native.desc(1, 2, 64, 64, 3, True, 5)
    hooked.allreduce = _native.ALLREDUCE_FN(lambda *a: None)
    refused = [
        (_native.desc(1, 2, 64, 64, 3, False, 5, groups=2), _native.ADMM_TV_EUNSUPPORTED, b"groups"),
        (hooked, _native.ADMM_TV_EUNSUPPORTED, b"hook"),
        (_native.desc(2, 2, 64, 64, 3, False, 5, flags=_native.ADMM_TV_FLAG_PSF_PER_IMAGE), _native.ADMM_TV_EUNSUPPORTED, b"bank"),
        (_native.desc(2, 2, 64, 64, 3, False, 5, flags=_native.ADMM_TV_FLAG_PSF_PER_CHANNEL), _native.ADMM_TV_EUNSUPPORTED, b"bank"),
        (_native.desc(2, 2, 15, 17, 3, False, 5, flags=_native.ADMM_TV_FLAG_PSF_PER_IMAGE | _native.ADMM_TV_FLAG_PSF_PER_CHANNEL),
         _native.ADMM_TV_EUNSUPPORTED, b"bank"),
        (_native.desc(1, 2, 64, 64, 3, False, 5, f64=True), _native.ADMM_TV_EINVAL, b"F64"),
        (_native.desc(1, 2, 64, 64, 3, False, 5, flags=_native.ADMM_TV_FLAG_PSF_GRAD), _native.ADMM_TV_EINVAL, b"PSF_GRAD"),
        (_native.desc(2, 2, 64, 64, 3, False, 5, flags=_native.ADMM_TV_FLAG_PSF_PER_IMAGE | _native.ADMM_TV_FLAG_PSF_BANK_TRAIN),
         _native.ADMM_TV_EINVAL, b"BANK_TRAIN"),
        # more than 2^31 - 1 image rows where the generic step's grid needs it
        (_native.desc(1 << 20, 1 << 11, 1, 7, 0, False, 5), _native.ADMM_TV_EUNSUPPORTED, b"rows"),
    ]
    for d, code, word in refused:
        for ask in entries:
            assert ask(d) == code, (word, ask.__name__)
            assert word in lib.admm_tv_last_error(), (word, ask.__name__, lib.admm_tv_last_error())
    # the plain solve's queries still answer for the descriptors only the box refuses
    n = ctypes.c_size_t(0)
    assert lib.admm_tv_workspace_size(ctypes.byref(refused[0][0]), ctypes.byref(n)) == 0
    assert lib.admm_tv_workspace_size(ctypes.byref(refused[2][0]), ctypes.byref(n)) == 0
    assert lib.admm_tv_workspace_size(ctypes.byref(refused[-1][0]), ctypes.byref(n)) == 0
    # a null bounds_dev: the call only (the queries take no bounds)
    ok = _native.desc(1, 2, 64, 64, 3, False, 5)
    call, size, path = entries
    assert call(ok, None) == _native.ADMM_TV_EINVAL and b"bounds" in lib.admm_tv_last_error()
    assert size(ok) == 0 and path(ok) == 1
    # ... and the descriptor errors every entry point shares come first
    bad = _native.desc(1, 2, 64, 64, 3, False, 5)
    bad.kw = 5
    assert [ask(bad) for ask in entries] == [_native.ADMM_TV_ENONSQUARE] * 3


@pytest.mark.parametrize("name,iso", bc.CASE_PARAMS)
def test_box_workspace_and_path_per_case(name, iso):
    """admm_tv_box_workspace_size is admm_tv_workspace_size plus one image for v, up to the regions' 256-byte
    alignment; admm_tv_path(desc, 3) is fused at power-of-two sizes and generic at every other -- the smooth
    sizes and the odd row lengths included; with or without a PSF, at any maxit."""
    from admmtor import _native
    shape, psf, _, want = bc.CASES[name]
    k = psf[1] if psf else 0
    for maxit in (0, 1, 6):
        d = _native.desc(*shape, k, iso, maxit)
        img = 4 * shape[0] * shape[1] * shape[2] * shape[3]
        extra = _native.box_workspace_size(d) - _native.workspace_size(d)
        assert img <= extra <= img + 512, (extra, img)
        assert _native.path(d, mode=3) == want


def test_other_modes_answer_as_before():
    """Modes 0, 1 and 2 of admm_tv_path for the cases' descriptors: what they were before mode 3 existed."""
    from admmtor import _native
    want = {  # (mode 0 aniso, mode 0 iso, mode 1, mode 2)
        (16, 16): ("fused",) * 4, (32, 64): ("fused",) * 4, (32, 256): ("fused",) * 4, (32, 1024): ("fused",) * 4,
        (16, 1024): ("fused",) * 4, (16, 2048): ("fused",) * 4,
        (15, 17): ("generic",) * 4, (1, 7): ("generic",) * 4,
        (240, 480): ("fused mixed-radix",) * 4,
        (17, 481): ("fused odd-length", "generic", "generic", "generic"),
    }
    seen = set()
    for name, (shape, psf, _, _) in bc.CASES.items():
        H, W = shape[2:]
        seen.add((H, W))
        k = psf[1] if psf else 0
        m0a, m0i, m1, m2 = want[(H, W)]
        assert _native.path(_native.desc(*shape, k, False, 5), mode=0) == _native.path(_native.desc(*shape, k, False, 5)) == m0a
        assert _native.path(_native.desc(*shape, k, True, 5), mode=0) == m0i
        for iso in (False, True):
            assert _native.path(_native.desc(*shape, k, iso, 5), mode=1) == _native.path(_native.desc(*shape, k, iso, 5), train=True) == m1
            assert _native.path(_native.desc(*shape, k, iso, 5), mode=2) == m2
    assert seen == set(want)
    # a PSF bank still has its paths in modes 0 and 2, and its refusal of training without the opt-in bit
    bank = _native.desc(2, 2, 64, 64, 3, False, 5, flags=_native.ADMM_TV_FLAG_PSF_PER_IMAGE)
    assert _native.path(bank, mode=0) == _native.path(bank, mode=2) == "fused"
    assert _native.load().admm_tv_path(ctypes.byref(bank), 1) == _native.ADMM_TV_EUNSUPPORTED


# ---------------------------------------------------------------- the Python wrapper, host only
def test_wrapper_is_public_and_checks_its_inputs():
    from admmtor.eops import deconv
    from admmtor.eops.deconv import fft_admm_tv_box
    assert "fft_admm_tv_box" in deconv.__all__
    x, k = torch.rand(1, 1, 16, 16), torch.full((1, 1, 3, 3), 1 / 9)
    with pytest.raises(ValueError, match="lo"):
        fft_admm_tv_box(x, 0.01, 0.02, k, lo=1.0, hi=0.0)
    with pytest.raises(ValueError, match="lo"):
        fft_admm_tv_box(x, 0.01, 0.02, k, 0.5, 0.25, project=False)
    # fft_admm_tv's error classes for bad shapes and dtypes (_check_inputs)
    with pytest.raises(ValueError):
        fft_admm_tv_box(x[0], 0.01, 0.02, k)
    with pytest.raises(IndexError):
        fft_admm_tv_box(x, 0.01, 0.02, k[0, 0])
    with pytest.raises(RuntimeError, match="non-square"):
        fft_admm_tv_box(x, 0.01, 0.02, torch.rand(1, 1, 3, 5))
    with pytest.raises(RuntimeError, match="shape"):
        fft_admm_tv_box(x, 0.01, 0.02, torch.rand(2, 1, 3, 3))
    with pytest.raises(RuntimeError, match="dtype"):
        fft_admm_tv_box(x, 0.01, 0.02, k.double())
    with pytest.raises(RuntimeError, match="Unsupported dtype"):
        fft_admm_tv_box(x.half(), 0.01, 0.02, k.half())
    with pytest.raises(TypeError):
        fft_admm_tv_box([[1.0]], 0.01, 0.02, k)
    # fp64 names its limitation; inputs that require grad are refused as fft_admm_tv_state refuses them
    with pytest.raises(NotImplementedError, match="fp32 solves only"):
        fft_admm_tv_box(x.double(), 0.01, 0.02, k.double())
    with pytest.raises(RuntimeError, match="fft_admm_tv is the differentiable call"):
        fft_admm_tv_box(x.clone().requires_grad_(True), 0.01, 0.02, k)
    with pytest.raises(RuntimeError, match="fft_admm_tv is the differentiable call"):
        fft_admm_tv_box(x, torch.tensor(0.01, requires_grad=True), 0.02, k)
    # an empty batch needs no device, as in fft_admm_tv
    out = fft_admm_tv_box(torch.empty(0, 3, 16, 16), 0.01, 0.02, k)
    assert out.shape == (0, 3, 16, 16) and out.dtype == torch.float32


def test_box_op_fake_kernel():
    """admm_hip::fft_admm_tv_box has a fake kernel (one tensor shaped like x, contiguous) and no CPU kernel."""
    import admmtor._ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x, one, two = torch.empty(2, 3, 64, 32), torch.empty(1), torch.empty(2)
        for k in (torch.empty(1, 1, 5, 5), torch.empty(0)):
            for xx in (x, x.transpose(2, 3)):
                out = torch.ops.admm_hip.fft_admm_tv_box(xx, one, one, k, two, True, 10)
                assert out.shape == xx.shape and out.dtype == x.dtype and out.is_contiguous()
    x = torch.rand(1, 1, 16, 16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        torch.ops.admm_hip.fft_admm_tv_box(x, torch.ones(1), torch.ones(1), torch.empty(0), torch.tensor([0.0, 1.0]), False, 2)
