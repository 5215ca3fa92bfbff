"""CPU side of the PSF-bank feature (ADMM_TV_FLAG_PSF_PER_IMAGE / _PER_CHANNEL, fft_admm_tv_bank): the fp64
restatement the GPU tests check against (tests/bank_cases.py) is pinned to the oracle, the negative controls hold
for every GPU case, the C ABI answers its host-only questions (workspace growth, refusals, paths) and the Python
calls validate their arguments before they look for a device."""
import ctypes
import json
import os

import pytest
import torch

import bank_cases as bc


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", list(bc.CASES))
def test_restatement_pins(name):
    """A (1, 1, k, k) bank is solve_fourier, and an aniso per-image bank is the per-image solve_fourier calls
    concatenated: <= 1e-12 (fp64 rounding; measured <= 1.1e-14)."""
    for iso in bc.ISOS:
        for maxit in bc.MAXITS:
            e = bc.pin_shared(name, iso, maxit)
            print(name, iso, maxit, f"shared bank vs solve_fourier {e:.1e}")
            assert e <= 1e-12
    for maxit in bc.MAXITS:
        e = bc.pin_per_image(name, maxit)
        print(name, maxit, f"per-image bank vs the loop of solves {e:.1e}")
        assert e <= 1e-12


def test_index_maps():
    """The right map is the header's t = (Bk > 1 ? b : 0) Ck + (Ck > 1 ? c : 0); every wrong map differs."""
    for mode, want in (("image", [[0, 0, 0], [1, 1, 1]]), ("channel", [[0, 1, 2], [0, 1, 2]]),
                       ("plane", [[0, 1, 2], [3, 4, 5]]), ("shared", [[0, 0, 0], [0, 0, 0]])):
        kerns = bc.make_bank(mode, 2, 3, 5)
        R = bc.right_map(kerns, 2, 3)
        assert R.tolist() == want
        if mode != "shared":
            wrong = bc.wrong_maps(kerns, 2, 3)
            assert len(wrong) == (6 if mode == "plane" else 3)
            assert all(not torch.equal(m, R) and int(m.min()) >= 0 and int(m.max()) < kerns.shape[0] * kerns.shape[1]
                       for m in wrong.values())
    ps = bc.bank_psfs(5)
    assert all(not torch.equal(ps[i], ps[j]) for i in range(6) for j in range(i))


@pytest.mark.parametrize("name,mode,iso,maxit", bc.PARAMS)
def test_gpu_cases_have_teeth(name, mode, iso, maxit):
    """Every case of tests/test_gpu_psf_bank.py: each wrong index map -- on the factor alone, on b alone, on
    both -- misses the right fp64 solve by >= 1e-3 (asserted inside bank_cases.reference)."""
    r = bc.reference(name, mode, iso, maxit)
    worst = min(r["controls"], key=r["controls"].get)
    print(name, mode, iso, maxit, "weakest control", worst, f"{r['controls'][worst]:.1e}")
    assert len(r["controls"]) == (18 if mode == "plane" else 9)
    assert r["controls"][worst] >= bc.CONTROL_MIN


# ---------------------------------------------------------------- the C ABI, host only
def _flags(mode):
    from admmtor import _native
    return {"image": _native.ADMM_TV_FLAG_PSF_PER_IMAGE, "channel": _native.ADMM_TV_FLAG_PSF_PER_CHANNEL,
            "plane": _native.ADMM_TV_FLAG_PSF_PER_IMAGE | _native.ADMM_TV_FLAG_PSF_PER_CHANNEL}[mode]


def test_flag_constants_match_the_header():
    from admmtor import _native
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "admm_tv.h")).read()
    assert f"#define ADMM_TV_FLAG_PSF_PER_IMAGE {_native.ADMM_TV_FLAG_PSF_PER_IMAGE} " in hdr
    assert f"#define ADMM_TV_FLAG_PSF_PER_CHANNEL {_native.ADMM_TV_FLAG_PSF_PER_CHANNEL} " in hdr
    assert (_native.ADMM_TV_FLAG_PSF_PER_IMAGE, _native.ADMM_TV_FLAG_PSF_PER_CHANNEL) == (4, 8)
    assert _native.load().admm_tv_abi_version() == 7
    assert "not implemented" in hdr and "bank" in hdr  # training with a bank: refused, the next step


@pytest.mark.parametrize("name", list(bc.CASES))
def test_workspace_grows_by_the_tables(name):
    """T tables cost T - 1 more copies of the PSF regions and nothing else: the Wiener factor (+ its packed /
    mixed copy), the H_t multiplier (+ its mixed copy), the PSF row spectra; every region 256-byte aligned.
    (Where the shared-PSF solve takes another path -- the matrix-core column pass's transposed factor, the
    odd-length row pass's second spectrum buffer -- the bank solve needs less of those, so only the upper
    bound holds.)"""
    from admmtor import _native
    (B, C, H, W), k, _ = bc.CASES[name]
    N = W // 2
    for iso in bc.ISOS:
        base = _native.workspace_size(_native.desc(B, C, H, W, k, iso, 3))
        last = base
        for mode in ("image", "channel", "plane"):
            T = {"image": B, "channel": C, "plane": B * C}[mode]
            d = _native.desc(B, C, H, W, k, iso, 3, flags=_flags(mode))
            n = _native.workspace_size(d)
            assert _native.state_workspace_size(d) == n
            # per table: fcT + copy (8 B/point), mT (8), fcM (<= 8), mM (8), G (16 k (N + 1))
            per_table = (N + 1) * H * 32 + 16 * k * (N + 1)
            assert n <= base + (T - 1) * per_table + 5 * 256 * T, (name, mode, n, base)
            if bc.CASES[name][2] != "generic":
                assert n > base and (mode != "plane" or n > last), (name, mode, n, base)
            last = n


def _null_calls(lib, d):
    """Every entry point of `d`'s kind called with pointers that are never dereferenced: -> {name: code}."""
    one = ctypes.c_void_p(256)
    big = 1 << 40
    return {
        "forward": lib.admm_tv_forward(ctypes.byref(d), one, one, one, one, one, one, big, None),
        "forward_state": lib.admm_tv_forward_state(ctypes.byref(d), one, one, one, one, None, None, one, one, big, None),
        "psf_transpose": lib.admm_tv_psf_transpose(ctypes.byref(d), one, one, one, one, big, None),
    }


def test_refusals():
    """The refusals of include/admm_tv.h, from the size queries, admm_tv_path and the entry points alike, each
    with a message."""
    from admmtor import _native
    lib = _native.load()
    n = ctypes.c_size_t(0)
    EINVAL, EUNSUP = _native.ADMM_TV_EINVAL, _native.ADMM_TV_EUNSUPPORTED

    def refused_everywhere(d, code, word):
        for what, got in {"workspace_size": lib.admm_tv_workspace_size(ctypes.byref(d), ctypes.byref(n)),
                          "state_workspace_size": lib.admm_tv_state_workspace_size(ctypes.byref(d), ctypes.byref(n)),
                          "path 0": lib.admm_tv_path(ctypes.byref(d), 0),
                          "path 2": lib.admm_tv_path(ctypes.byref(d), 2), **_null_calls(lib, d)}.items():
            assert got == code, (what, got, code)
            assert word in lib.admm_tv_last_error(), (what, lib.admm_tv_last_error())

    for mode in bc.MODES:
        f = _flags(mode)
        refused_everywhere(_native.desc(2, 3, 64, 64, 0, False, 5, flags=f), EINVAL, b"kh == 0")
        refused_everywhere(_native.desc(2, 3, 64, 64, 5, False, 5, flags=f, groups=2), EUNSUP, b"groups")
        hooked = _native.desc(2, 3, 64, 64, 5, True, 5, flags=f)
        hooked.allreduce = _native.ALLREDUCE_FN(lambda *a: None)
        refused_everywhere(hooked, EUNSUP, b"hook")
        refused_everywhere(_native.desc(2, 3, 64, 64, 5, False, 5, flags=f, f64=True), EUNSUP, b"fp32 only")
        refused_everywhere(_native.desc(2, 3, 64, 64, 5, False, 5, flags=f | _native.ADMM_TV_FLAG_PSF_GRAD), EUNSUP,
                           b"PSF gradient")
        # the training entry points and their size queries
        d = _native.desc(2, 3, 64, 64, 5, False, 5, flags=f)
        one, big = ctypes.c_void_p(256), 1 << 40
        train = {
            "path 1": lib.admm_tv_path(ctypes.byref(d), 1),
            "history_size": lib.admm_tv_history_size(ctypes.byref(d), ctypes.byref(n)),
            "backward_workspace_size": lib.admm_tv_backward_workspace_size(ctypes.byref(d), ctypes.byref(n)),
            "forward_train": lib.admm_tv_forward_train(ctypes.byref(d), one, one, one, one, one, one, big, one, big, None),
            "backward": lib.admm_tv_backward(ctypes.byref(d), one, one, one, one, one, one, big, one, one, one, one, one,
                                             big, None),
        }
        for what, got in train.items():
            assert got == EUNSUP, (what, got)
        assert b"inference only" in lib.admm_tv_last_error()
        # every _f64 entry point, with and without ADMM_TV_FLAG_F64 beside the bank bit
        for f64 in (False, True):
            d64 = _native.desc(2, 3, 64, 64, 5, False, 5, flags=f, f64=f64)
            got = {
                "forward_f64": lib.admm_tv_forward_f64(ctypes.byref(d64), one, one, one, one, one, one, big, None),
                "forward_train_f64": lib.admm_tv_forward_train_f64(ctypes.byref(d64), one, one, one, one, one, one, big,
                                                                   one, big, None),
                "backward_f64": lib.admm_tv_backward_f64(ctypes.byref(d64), one, one, one, one, one, one, big, one, one,
                                                         one, one, one, big, None),
            }
            assert all(v == EUNSUP for v in got.values()), got
            assert b"fp32 only" in lib.admm_tv_last_error()
    # the bits change nothing else: without them the same descriptors are accepted as before
    assert lib.admm_tv_workspace_size(ctypes.byref(_native.desc(2, 3, 64, 64, 0, False, 5)), ctypes.byref(n)) == 0
    assert lib.admm_tv_workspace_size(ctypes.byref(_native.desc(2, 3, 64, 64, 5, False, 5, groups=2)), ctypes.byref(n)) == 0


@pytest.mark.parametrize("name", list(bc.CASES))
def test_paths(name):
    """admm_tv_path(desc, 0) and (desc, 2) with a bank: fused at the power-of-two cases, mixed at 240 x 480, the
    generic iteration elsewhere -- both odd orientations included, where the shared-PSF solve takes the
    odd-length row pass."""
    from admmtor import _native
    (B, C, H, W), k, want = bc.CASES[name]
    for mode in bc.MODES:
        for iso in bc.ISOS:
            d = _native.desc(B, C, H, W, k, iso, 3, flags=_flags(mode))
            assert _native.path(d, mode=0) == want, (name, mode, iso)
            assert _native.path(d, mode=2) == want, (name, mode, iso)
    if name.startswith("c4_"):
        assert _native.path(_native.desc(B, C, H, W, k, False, 3), mode=0) == "fused odd-length"


def test_path_of_an_unknown_code_is_a_native_error(monkeypatch):
    from admmtor import _native

    class Lib:
        @staticmethod
        def admm_tv_path(d, mode):
            return 99

    monkeypatch.setattr(_native, "load", lambda: Lib)
    with pytest.raises(_native.NativeError, match="99"):
        _native.path(_native.desc(1, 1, 16, 16, 0, False, 1))


# ---------------------------------------------------------------- the Python calls, host tensors only
@pytest.mark.parametrize("call", ["fft_admm_tv_bank", "fft_admm_tv_bank_state"])
def test_python_validation(call):
    """Every refusal is raised before a device is looked for (this machine may have none)."""
    from admmtor.eops import deconv
    assert call in deconv.__all__
    f = getattr(deconv, call)
    x = torch.rand(2, 3, 16, 16)
    for shape in [(3, 1, 5, 5), (1, 2, 5, 5), (2, 2, 5, 5), (4, 3, 5, 5), (5, 5), (1, 5, 5), (1, 1, 1, 5, 5)]:
        with pytest.raises(ValueError, match="PSF bank"):
            f(x, 0.01, 0.02, torch.rand(*shape))
    with pytest.raises(ValueError, match="fft_admm_tv "):
        f(x, 0.01, 0.02, torch.empty(0))
    with pytest.raises(ValueError):
        f(torch.rand(3, 16, 16), 0.01, 0.02, torch.rand(2, 3, 5, 5))
    with pytest.raises(RuntimeError, match="non-square"):
        f(x, 0.01, 0.02, torch.rand(2, 3, 5, 3))
    with pytest.raises(RuntimeError, match="dtype"):
        f(x, 0.01, 0.02, torch.rand(2, 3, 5, 5, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="fp32"):
        f(x.double(), 0.01, 0.02, torch.rand(2, 3, 5, 5, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="Unsupported dtype"):
        f(x.half(), 0.01, 0.02, torch.rand(2, 3, 5, 5).half())
    for bad in ("x", "kerns", "lam"):
        xs = x.clone().requires_grad_(bad == "x")
        ks = torch.rand(2, 3, 5, 5).requires_grad_(bad == "kerns")
        lam = torch.tensor(0.01, requires_grad=bad == "lam")
        with pytest.raises(RuntimeError, match="inference only"):
            f(xs, lam, 0.02, ks)


def test_fft_admm_tv_keeps_its_recorded_errors():
    """fft_admm_tv and fft_admm_tv_state do not become bank calls: (2,1,3,3) and (1,2,3,3) kerns raise what
    tests/golden/errors.json records for the reference."""
    from admmtor.eops.deconv import fft_admm_tv, fft_admm_tv_state
    rec = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "errors.json")))
    assert rec["kernel_2ch"] == "RuntimeError"  # the reference with a (1, 2, 3, 3) kern on two channels
    x = torch.rand(2, 2, 16, 16)
    for shape in ((2, 1, 3, 3), (1, 2, 3, 3)):
        for f in (fft_admm_tv, fft_admm_tv_state):
            with pytest.raises(RuntimeError, match=r"\(1, 1, kh, kw\)"):
                f(x, 0.01, 0.02, torch.rand(*shape), False, 2)


def test_fake_kernels_with_a_bank():
    """The ops' fake kernels: the output shapes do not depend on the bank; the training op refuses one."""
    import admmtor._ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    x, one = torch.empty(2, 3, 64, 32, device="meta"), torch.empty(1, device="meta")
    for shape in ((2, 1, 5, 5), (1, 3, 5, 5), (2, 3, 5, 5), (1, 1, 5, 5)):
        k = torch.empty(*shape, device="meta")
        assert torch.ops.admm_hip.fft_admm_tv_fwd(x, one, one, k, False, 10).shape == x.shape
        outs = torch.ops.admm_hip.fft_admm_tv_state(x, one, one, k, [], True, 10)
        assert len(outs) == 5 and all(o.shape == x.shape and o.dtype == x.dtype for o in outs)
    with FakeTensorMode():
        xf, of, kf = torch.empty(2, 3, 64, 32), torch.empty(1), torch.empty(2, 3, 5, 5)
        assert torch.ops.admm_hip.fft_admm_tv_fwd(xf, of, of, kf, True, 10).shape == xf.shape
    # the real kernels: a wrong leading shape is a ValueError, a bank on the training op NotImplementedError
    from admmtor import _ops
    xr, lr = torch.rand(2, 3, 16, 16), torch.ones(1)
    with pytest.raises(ValueError, match="PSF bank"):
        _ops._bank(xr, torch.rand(3, 3, 5, 5))
    assert _ops._bank(xr, torch.rand(1, 1, 5, 5)) == 0 and _ops._bank(xr, torch.empty(0)) == 0
    assert _ops._bank(xr, torch.rand(2, 1, 5, 5)) == 4 and _ops._bank(xr, torch.rand(1, 3, 5, 5)) == 8
    assert _ops._bank(xr, torch.rand(2, 3, 5, 5)) == 12
    with pytest.raises(NotImplementedError, match="inference only"):
        torch.ops.admm_hip.fft_admm_tv_fwd_train(xr, lr, lr, torch.rand(2, 3, 5, 5), False, 2, False)
