"""Training with a PSF bank, host side (no GPU): the C ABI's answers for ADMM_TV_FLAG_PSF_BANK_TRAIN on the built
library -- sizes, paths, refusals -- the new dispatcher ops' fake kernels, fft_admm_tv_bank_train's validation
on host tensors and the ADMMDeconvBank layer's parameters."""
import ctypes
import os

import pytest
import torch

import bank_cases as bc
import bank_train_cases as btc


def _bits(mode):
    from admmtor import _native
    return {"image": _native.ADMM_TV_FLAG_PSF_PER_IMAGE, "channel": _native.ADMM_TV_FLAG_PSF_PER_CHANNEL,
            "plane": _native.ADMM_TV_FLAG_PSF_PER_IMAGE | _native.ADMM_TV_FLAG_PSF_PER_CHANNEL}[mode]


def _up(n):
    return -(-n // 256) * 256


def test_flag_constant_matches_the_header():
    from admmtor import _native
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "admm_tv.h")).read()
    assert f"#define ADMM_TV_FLAG_PSF_BANK_TRAIN {_native.ADMM_TV_FLAG_PSF_BANK_TRAIN} " in hdr
    assert _native.ADMM_TV_FLAG_PSF_BANK_TRAIN == 16 and _native.load().admm_tv_abi_version() == 7
    assert "admm_tv_bank" not in " ".join(_native.EXPORTED)  # no function added


@pytest.mark.parametrize("name", list(btc.CASES))
def test_sizes_and_paths(name):
    """The history is per plane (the shared-PSF descriptor's); the backward workspace grows with T when the PSF
    gradient is on, by no more than the documented per-table regions; admm_tv_path(desc, 1) names the path."""
    from admmtor import _native
    (B, C, H, W), k, path = btc.CASES[name][:3]
    TR, PG = _native.ADMM_TV_FLAG_PSF_BANK_TRAIN, _native.ADMM_TV_FLAG_PSF_GRAD
    nf, N1 = (W // 2 + 1) * H, W // 2 + 1
    for iso in btc.ISOS:
        for pg in (0, PG):
            shared = _native.desc(B, C, H, W, k, iso, 3, flags=pg)
            last = 0
            for mode in btc.MODES:
                T = {"image": B, "channel": C, "plane": B * C}[mode]
                d = _native.desc(B, C, H, W, k, iso, 3, flags=_bits(mode) | TR | pg)
                assert _native.path(d, train=True) == path, (name, mode)
                assert _native.path(d, mode=0) == _native.path(_native.desc(B, C, H, W, k, iso, 3, flags=_bits(mode)), mode=0)
                assert _native.history_size(d) == _native.history_size(shared)
                fwd = _native.workspace_size(d)
                plain = _native.workspace_size(_native.desc(B, C, H, W, k, iso, 3, flags=_bits(mode)))
                assert fwd == plain + (_up(T * nf * 16) if pg else 0)  # the same layout, plus T sigma tables
                n = _native.backward_workspace_size(d)
                base = _native.backward_workspace_size(shared)
                # forward tables per table (test_bank_restatement), sigma (16 B/point); with the gradient A real
                # and Z complex fp64 (24), the chunks' partials (8 per chunk: at most planes / 8 + T chunks) and
                # the taps' k rows of W/2 + 1 complex sums and phase tables
                per_table = nf * 32 + 16 * k * N1
                bound = base + (T - 1) * per_table + 5 * 256 * T
                if pg:
                    chunks = -(-B * C // btc.XPPG) + T
                    bound += T * nf * (16 + 24) + chunks * nf * 8 + T * k * N1 * 16 + k * (H + N1) * 16 + 6 * 256
                    assert n > base, (name, mode, iso, n, base)
                    if mode == "plane":  # grows with T (image and channel banks hold fewer tables)
                        assert n > last, (name, mode, iso, n, last)
                    last = max(last, n)
                assert n <= bound, (name, mode, iso, pg, n, bound)


def _calls(lib, d, infer=True):
    """Every query and entry point of `d`'s kind -> {name: code}.  The entry points get pointers that are never
    dereferenced, so they are called only where the library refuses `d`: infer=False leaves out the inference
    calls, for a descriptor that those accept (they would launch kernels on the dummy pointers)."""
    n = ctypes.c_size_t(0)
    one, big = ctypes.c_void_p(256), 1 << 40
    got = {
        "workspace_size": lib.admm_tv_workspace_size(ctypes.byref(d), ctypes.byref(n)),
        "history_size": lib.admm_tv_history_size(ctypes.byref(d), ctypes.byref(n)),
        "backward_workspace_size": lib.admm_tv_backward_workspace_size(ctypes.byref(d), ctypes.byref(n)),
        "path 0": lib.admm_tv_path(ctypes.byref(d), 0),
        "path 1": lib.admm_tv_path(ctypes.byref(d), 1),
    }
    if infer:
        got["forward"] = lib.admm_tv_forward(ctypes.byref(d), one, one, one, one, one, one, big, None)
        got["psf_transpose"] = lib.admm_tv_psf_transpose(ctypes.byref(d), one, one, one, one, big, None)
    got["forward_train"] = lib.admm_tv_forward_train(ctypes.byref(d), one, one, one, one, one, one, big, one, big, None)
    got["backward"] = lib.admm_tv_backward(ctypes.byref(d), one, one, one, one, one, one, big, one, one, one, one, one,
                                           big, None)
    return got


def _state_calls(lib, d):
    n = ctypes.c_size_t(0)
    one, big = ctypes.c_void_p(256), 1 << 40
    return {
        "state_workspace_size": lib.admm_tv_state_workspace_size(ctypes.byref(d), ctypes.byref(n)),
        "path 2": lib.admm_tv_path(ctypes.byref(d), 2),
        "forward_state": lib.admm_tv_forward_state(ctypes.byref(d), one, one, one, one, None, None, one, one, big, None),
    }


def test_refusals_with_the_bit():
    from admmtor import _native
    lib = _native.load()
    EINVAL, EUNSUP = _native.ADMM_TV_EINVAL, _native.ADMM_TV_EUNSUPPORTED
    TR, PG = _native.ADMM_TV_FLAG_PSF_BANK_TRAIN, _native.ADMM_TV_FLAG_PSF_GRAD

    def refused(d, code, word, calls=_calls):
        for what, got in calls(lib, d).items():
            assert got == code, (what, got, code)
        assert word in lib.admm_tv_last_error(), lib.admm_tv_last_error()

    for mode in btc.MODES:
        f = _bits(mode) | TR
        refused(_native.desc(2, 3, 64, 64, 0, False, 5, flags=f), EINVAL, b"kh == 0")
        refused(_native.desc(2, 3, 64, 64, 5, False, 5, flags=f, groups=2), EUNSUP, b"groups")
        hooked = _native.desc(2, 3, 64, 64, 5, True, 5, flags=f)
        hooked.allreduce = _native.ALLREDUCE_FN(lambda *a: None)
        refused(hooked, EUNSUP, b"hook")
        refused(_native.desc(2, 3, 64, 64, 5, False, 5, flags=f, f64=True), EUNSUP, b"fp32 only")
        one, big = ctypes.c_void_p(256), 1 << 40
        for f64 in (False, True):
            d64 = _native.desc(2, 3, 64, 64, 5, False, 5, flags=f, f64=f64)
            got = [lib.admm_tv_forward_f64(ctypes.byref(d64), one, one, one, one, one, one, big, None),
                   lib.admm_tv_forward_train_f64(ctypes.byref(d64), one, one, one, one, one, one, big, one, big, None),
                   lib.admm_tv_backward_f64(ctypes.byref(d64), one, one, one, one, one, one, big, one, one, one, one, one,
                                            big, None)]
            assert got == [EUNSUP] * 3 and b"fp32 only" in lib.admm_tv_last_error()
        # the stateful solve refuses the bit as it refuses ADMM_TV_FLAG_PSF_GRAD
        refused(_native.desc(2, 3, 64, 64, 5, False, 5, flags=f), EINVAL, b"ADMM_TV_FLAG_PSF_BANK_TRAIN", _state_calls)
        refused(_native.desc(2, 3, 64, 64, 5, False, 5, flags=f | PG), EINVAL, b"ADMM_TV_FLAG_PSF_BANK_TRAIN", _state_calls)
    refused(_native.desc(70000, 1, 16, 16, 3, False, 5, flags=_bits("image") | TR), EUNSUP, b"65,535")
    # the bit without a bank bit
    for extra in (0, PG):
        d = _native.desc(2, 3, 64, 64, 5, False, 5, flags=TR | extra)
        refused(d, EINVAL, b"without a PSF bank")
        refused(d, EINVAL, b"without a PSF bank", _state_calls)


def test_without_the_bit_a_bank_answers_as_before():
    """test_bank_restatement.py's descriptors: the training entry points refuse a bank with 'inference only',
    bank | PSF_GRAD everywhere with 'PSF gradient' -- and bank | bit is accepted, so a caller can probe."""
    from admmtor import _native
    lib = _native.load()
    EUNSUP = _native.ADMM_TV_EUNSUPPORTED
    for mode in btc.MODES:
        d = _native.desc(2, 3, 64, 64, 5, False, 5, flags=_bits(mode))
        got = _calls(lib, d, infer=False)  # a plain bank: the inference calls accept it
        for what in ("history_size", "backward_workspace_size", "path 1", "forward_train", "backward"):
            assert got[what] == EUNSUP, (what, got)
        assert b"inference only" in lib.admm_tv_last_error()
        assert got["workspace_size"] == 0 and got["path 0"] > 0
        g = _calls(lib, _native.desc(2, 3, 64, 64, 5, False, 5, flags=_bits(mode) | _native.ADMM_TV_FLAG_PSF_GRAD))
        assert set(g.values()) == {EUNSUP}
        n = ctypes.c_size_t(0)
        gd = _native.desc(2, 3, 64, 64, 5, False, 5, flags=_bits(mode) | _native.ADMM_TV_FLAG_PSF_GRAD)
        assert lib.admm_tv_workspace_size(ctypes.byref(gd), ctypes.byref(n)) == EUNSUP
        assert b"PSF gradient" in lib.admm_tv_last_error()
        ok = _native.desc(2, 3, 64, 64, 5, False, 5, flags=_bits(mode) | _native.ADMM_TV_FLAG_PSF_BANK_TRAIN)
        assert _native.path(ok, train=True) == "fused" and _native.history_size(ok) > 0


@pytest.mark.parametrize("mode", btc.MODES)
@pytest.mark.parametrize("psf_grad", [False, True])
def test_fake_kernels(mode, psf_grad):
    from admmtor import _native, _ops  # noqa: F401
    B, C, H, W, k = 2, 3, 16, 32, 5
    x = torch.empty(B, C, H, W, device="meta")
    lam = torch.empty(1, device="meta")
    kerns = torch.empty(*bc.bank_dims(mode, B, C), k, k, device="meta")
    out, hist = torch.ops.admm_hip.fft_admm_tv_bank_fwd_train(x, lam, lam, kerns, True, 4, psf_grad)
    assert out.shape == x.shape and hist.dtype == torch.uint8
    assert hist.numel() == _native.history_size(_native.desc(B, C, H, W, k, True, 4,
                                                             flags=_native.ADMM_TV_FLAG_PSF_GRAD if psf_grad else 0))
    gx, gl, gr, gk = torch.ops.admm_hip.fft_admm_tv_bank_bwd(out, x, lam, lam, kerns, hist, True, 4, psf_grad, True, True,
                                                              psf_grad)
    assert gx.shape == x.shape and gl.shape == gr.shape == (1,)
    assert gk.shape == (kerns.shape if psf_grad else (0,))
    gx, gl, gr, gk = torch.ops.admm_hip.fft_admm_tv_bank_bwd(out, x, lam, lam, kerns, hist, True, 4, psf_grad, False,
                                                              False, False)
    assert gx.numel() == gl.numel() == gr.numel() == gk.numel() == 0


def test_shared_op_still_refuses_a_bank():
    from admmtor import _ops  # noqa: F401
    x, lam = torch.empty(2, 3, 16, 32), torch.empty(1)
    with pytest.raises(NotImplementedError, match="inference only"):
        torch.ops.admm_hip.fft_admm_tv_fwd_train(x, lam, lam, torch.empty(2, 1, 5, 5), False, 3, False)


def test_validation_on_host_tensors():
    from admmtor.eops import deconv
    assert "fft_admm_tv_bank_train" in deconv.__all__
    f = deconv.fft_admm_tv_bank_train
    x = torch.zeros(2, 3, 16, 16, requires_grad=True)
    with pytest.raises(ValueError):
        f(x[0], 0.02, 0.2, torch.zeros(2, 1, 5, 5))
    with pytest.raises(ValueError):
        f(x, 0.02, 0.2, torch.zeros(3, 1, 5, 5))        # Bk not in (1, B)
    with pytest.raises(ValueError):
        f(x, 0.02, 0.2, torch.zeros(0))                 # an empty bank
    with pytest.raises(RuntimeError, match="non-square"):
        f(x, 0.02, 0.2, torch.zeros(2, 1, 5, 3))
    with pytest.raises(RuntimeError, match="dtype"):
        f(x, 0.02, 0.2, torch.zeros(2, 1, 5, 5, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="fp32"):
        f(x.double(), 0.02, 0.2, torch.zeros(2, 1, 5, 5, dtype=torch.float64))
    # the inference calls keep refusing inputs that require grad
    with pytest.raises(RuntimeError, match="inference only"):
        deconv.fft_admm_tv_bank(x, 0.02, 0.2, torch.zeros(2, 1, 5, 5))


def test_layer_parameters_and_seeded_init():
    from admmtor.elayers.admmdeconv import ADMMDeconv, ADMMDeconvBank
    torch.manual_seed(7)
    m = ADMMDeconvBank((5, 5), 4, channels=3, lmbda=0.02, bias=True)
    torch.manual_seed(7)
    one = ADMMDeconv((5, 5), 4, lmbda=0.02, bias=True)
    assert list(m.state_dict()) == list(one.state_dict())  # names and registration order
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in one.named_parameters()]
    assert m.w.shape == (1, 3, 5, 5) and m.w.requires_grad
    assert torch.equal(m.w[0, 0], one.w[0, 0])  # channel 0 of a seeded init is ADMMDeconv's PSF
    bound = (6.0 / 50.0) ** 0.5                # xavier-uniform of a (1, 1, 5, 5) tensor
    assert m.w.abs().max() <= bound and not torch.equal(m.w[0, 0], m.w[0, 1])
    with pytest.raises(ValueError):
        ADMMDeconvBank((), 4, channels=3)
