"""Training on the generic kernels at every transform plan (run_forward_gen with a history, run_backward_gen:
the column pass's spectrum dump and MODE 3, the HIST step / iso norm kernels, k_gbwd, k_giso_q, k_gxspec_acc,
k_psf_grad, the backward's own scratch slots for long lines, the fp64 instantiations, the fp64 route of an
fp32 solve past F32_MAX_PRIME) against the fp64 oracle's autograd (solve_spatial, the reference's op sequence).

The cases are tests/generic_train_cases.py's, one or two per plan class and dimension; the class of each is
derived from a restatement of the library's plan selection and checked on the CPU, together with what makes
the fixed gates legitimate, by tests/test_generic_train_case_inputs.py.  Gates (relative L2), the project's own:

  fp32  train_cases': forward <= 1e-5; gradients <= 1e-4 without a PSF, <= 1e-3 (the PSF's included) with one
  fp64  test_gpu_f64.py's: forward <= 1e-12, gradients <= 1e-9

No floor term, no near-kink exemption; a lambda / rho reference gradient that is exactly 0 is compared
absolutely (scalar_err).  Every case prints its errors (pytest -s); the worst per class are in DESIGN.md."""
import pytest
import torch

import generic_train_cases as gc
import train_cases as tc
from test_gpu_f64 import TOL64, TOL64_GRAD
from test_gpu_train_shapes import hip_train

pytestmark = pytest.mark.gpu

_runs = {}


def train(case, dev):
    """A case's training step on the release library, once: dict(out, gx, glam, grho[, gk])."""
    if case.name not in _runs:
        _runs[case.name] = hip_train(case, dev, torch.float64 if gc.is_f64(case) else torch.float32)
    return _runs[case.name]


def infer(case, dev):
    from admmtor.eops.deconv import fft_admm_tv
    dtype = torch.float64 if gc.is_f64(case) else torch.float32
    x, k = tc.inputs(case)
    kd = k.to(dev, dtype) if k.numel() else torch.empty(0, device=dev, dtype=dtype)
    return fft_admm_tv(x.to(dev, dtype), case.lam, case.rho, kd, case.iso, case.maxit).cpu()


def check_gates_f64(case, e):
    assert e["out"] <= TOL64, (case.name, e)
    for key in ("gx", "glam", "grho", "gk"):
        if key in e:
            assert e[key] <= TOL64_GRAD, (case.name, key, e)


def _dtypes(got):
    return {v.dtype for v in got.values()}


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("case", gc.COL_CASES + gc.ROW_CASES + gc.BOTH_MM_CASES + gc.EDGE_CASES, ids=str)
def test_training_vs_oracle(cuda_dev, case):
    got = train(case, cuda_dev)
    e = tc.errors(got, tc.reference(case))
    print(f"[{case.group}] {case.name} {case.shape} maxit {case.maxit}: {tc.fmt(e)}")
    assert _dtypes(got) == {torch.float32}
    assert ("gk" in e) == case.learn_psf
    tc.check_gates(case, e)


@pytest.mark.parametrize("case", gc.F64_CASES, ids=str)
def test_f64_training_vs_oracle(cuda_dev, case):
    got = train(case, cuda_dev)
    e = tc.errors(got, tc.reference(case))
    print(f"[{case.group}] {case.name} {case.shape} maxit {case.maxit}: {tc.fmt(e)}")
    assert _dtypes(got) == {torch.float64}
    assert ("gk" in e) == case.learn_psf
    check_gates_f64(case, e)


def test_f32_past_max_prime_trains_in_f64(cuda_dev):
    """An fp32 training step at a 13,003-point line (a prime above F32_MAX_PRIME) goes through the fp64 train and
    backward entry points and hands back an fp32 output and fp32 gradients.  That it took the fp64 route shows in
    the output: closer to the fp64 oracle than 1e-7 (the rounding of its storage, 2^-24 relative per value,
    is ~3.5e-8 in relative L2; the fp32 kernels measured 7.1e-6 at 13,001)."""
    case = gc.F32MAX_CASE
    got = train(case, cuda_dev)
    e = tc.errors(got, tc.reference(case))
    print(f"[{case.group}] {case.name} {case.shape} maxit {case.maxit}: {tc.fmt(e)}")
    assert _dtypes(got) == {torch.float32}
    assert "gk" in e
    tc.check_gates(case, e)
    assert e["out"] <= 1e-7


# ------------------------------------------------------------------ the plan was taken (A/B build)
def _named(name):
    return next(c for c in gc.F32_CASES if c.name == name)


# one case per Bluestein size (column and row) and per matrix-core plan, with the knob that turns the plan off
KNOB_CASES = [
    ("c301-blue128-aniso-gauss3", "ADMM_BLUE_MIN"),
    ("c469-blue256-iso-motion5", "ADMM_BLUE_MIN"),
    ("c131-blue512-aniso-gauss5", "ADMM_BLUE_MIN"),
    ("c257-blue1024-iso-gauss3", "ADMM_BLUE_MIN"),
    ("r262-blue512-iso-gauss5", "ADMM_BLUE_MIN"),
    ("c148-mm4-iso-motion5", "ADMM_GCOL_MM"),
    ("r214-mm2-iso-gauss5", "ADMM_GROW_MM"),
    ("r481-mm13-aniso-gauss3", "ADMM_GROW_MM"),
]


@pytest.mark.parametrize("name,knob", KNOB_CASES)
def test_plan_was_taken(cuda_dev, monkeypatch, name, knob):
    """The case trained in the A/B build with the plan's knob at 0 and again with it unset: both meet the gates
    and the two outputs differ in bits, so the plan the table names is the one that ran (the proof
    test_gpu_gcol_mm.py uses for inference).  Classes without a knob -- the direct prime stage, the 512-thread
    blocks, twiddles and line buffers in global memory -- rely on the plan restatement."""
    from admmtor import _native
    case = _named(name)
    for k in ("ADMM_BLUE_MIN", "ADMM_GCOL_MM", "ADMM_GROW_MM"):
        monkeypatch.delenv(k, raising=False)
    with _native.ab_library():
        on = hip_train(case, cuda_dev)
        monkeypatch.setenv(knob, "0")
        off = hip_train(case, cuda_dev)
    ref = tc.reference(case)
    e_on, e_off = tc.errors(on, ref), tc.errors(off, ref)
    print(f"[knob] {case.name} plan: {tc.fmt(e_on)}")
    print(f"[knob] {case.name} {knob}=0: {tc.fmt(e_off)}; outputs differ by {tc.rel(on['out'], off['out']):.2e}")
    tc.check_gates(case, e_on)
    tc.check_gates(case, e_off)
    assert not torch.equal(on["out"], off["out"])
    release = train(case, cuda_dev)  # with no knob set the A/B build is the release library
    assert all(torch.equal(on[key], release[key]) for key in release)


# ------------------------------------------------------------------ training forward = inference
def _first_per_class():
    """The first case of every class and dimension (of every S of the row inverse), both cases where inference
    pitches the spectrum rows, and every degenerate plane."""
    seen, out = set(), []
    for c in gc.COL_CASES + gc.ROW_CASES + gc.F64_CASES:
        key = (c.group, gc.mm_plan_row(c.shape[3]) if c.group == "row:mm" else None)
        if key not in seen and c.group != "f64:edge":
            seen.add(key)
            out.append(c)
    return out + gc.BOTH_MM_CASES + gc.EDGE_CASES + [c for c in gc.F64_CASES if c.group == "f64:edge"]


@pytest.mark.parametrize("case", _first_per_class(), ids=str)
def test_training_forward_equals_inference(cuda_dev, case):
    """The training forward keeps a history, dumps the column spectra, runs the step as a kernel of its own
    (inference runs it inside the forward row transform, grow_fwd_step) and keeps the spectrum rows unpitched
    where inference pitches them (both matrix-core plans); the arithmetic per value is the same, so the output
    is equal bit for bit.  The one exception is stated: at an odd row length with a fused row pass instance
    (481) the aniso inference solve runs the odd-length kernels (odd_kernels.hpp), other transforms with other
    roundings; there both are compared with the oracle."""
    from admmtor import _native
    B, C, H, W = case.shape
    f64 = gc.is_f64(case)
    t, i = train(case, cuda_dev)["out"], infer(case, cuda_dev)
    ref = tc.reference(case)["out"]
    et, ei = tc.rel(t, ref), tc.rel(i, ref)
    print(f"[infer] {case.name}: training {et:.2e}, inference {ei:.2e} vs oracle; between {tc.rel(t, i):.2e}")
    gate = TOL64 if f64 else tc.GATE_FWD
    assert et <= gate and ei <= gate
    d = _native.desc(B, C, H, W, case.psf[1] if case.psf else 0, case.iso, case.maxit, f64=f64)
    if _native.path(d) == "generic":
        assert torch.equal(t, i)
    else:
        assert _native.path(d) == "fused odd-length" and not case.iso
