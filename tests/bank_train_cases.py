"""Shared by the tests of training with a PSF bank (test_bank_train_case_inputs.py, test_bank_train_abi.py,
test_gpu_psf_bank_train.py); no test in here.

* ``solve_bank``: a differentiable restatement of the reference loop (deconv.py:103-115) with a PSF per image,
  per channel or per plane, written like ``oracle.admm_oracle.solve_spatial`` -- the same stencils, shrinks and
  FFT x-update -- with the Wiener factor and ``b = H_t(xin)`` per plane.  ``bank_cases.restate`` builds its
  factor with ``wiener_factor``, which detaches the PSF, so it cannot be differentiated in ``kerns``; this one
  is differentiable in ``xin``, ``lmbd``, ``rho`` and ``kerns`` through ordinary autograd.  The index maps are
  ``bank_cases``'s.
* the case table: the smallest shapes that reach each kernel instance of the bank's backward, every one in
  modes image, channel and plane, aniso and iso, at 1, 2 and 3 iterations (1: the LASTK && FIRSTK reverse step
  alone; 2: the first reverse step is also the last but one).
* the negative controls of the PSF gradient: the fp64 ``gkerns`` with the per-plane gradients summed over the
  planes of a wrong index map, and with the factor or ``b`` taken from the wrong table.  Each must miss the
  right fp64 gradient by CONTROL_MIN = 1e-2, ten times the 1e-3 gate; ``reference`` asserts it before it
  returns anything to compare with.

Gates and parameters are the training tables' (train_cases): lambda = 0.02, rho = 0.2 (one case's iso solves
take a larger lambda, see CASES)."""
import functools
import math

import torch

import bank_cases as bc
import train_cases as tc
from oracle.admm_oracle import _circ_dwconv, _dw, apply_psf_transpose, shrink_block, shrink_soft

LAM, RHO = tc.LAM, tc.RHO
CONTROL_MIN = 1e-2
XPPG = 8  # planes per cross-spectrum chunk (make_bwd_layout's xppg)

MODES = bc.MODES
ISOS = (False, True)
MAXITS = (1, 2, 3)

# name -> (shape, k, the path admm_tv_path(desc, 1) reports, seeds (aniso, iso), lambdas (aniso, iso)).
# Seeds -- and, where no seed serves at lambda = 0.02, lambda -- are the first that test_bank_train_case_inputs.py
# accepts in every mode at 1, 2 and 3 iterations (kink margin, active share, the fp32 restatement at half of
# each gate); rho = 0.2 throughout.  The small shapes' rho gradient is a sum that nearly cancels for some inputs
# (the fp32 restatement itself then misses fp64 by 4e-4 and more): their seeds keep it at 1e-4.
CASES = {
    "pow2_16x16": ((2, 3, 16, 16), 5, "fused", (2, 6), (LAM, LAM)),          # k_pass_b, N < 16; per-image C = 3
    "pow2_16x32": ((2, 3, 16, 32), 5, "fused", (2, 2), (LAM, LAM)),          # k_pass_b2 forward, MODE 2: k_pass_b
    "pow2_1024x32": ((2, 2, 1024, 32), 5, "fused", (1, 1), (LAM, LAM)),      # H = 1024, packed factors
    # k_xspec_m, generic MODE 2 (aniso: kink-free parameters, KINK_FREE below)
    "smooth_240x480": ((2, 3, 240, 480), 7, "fused mixed-radix", (1, 2), (0.2, LAM)),
    "gen_15x17": ((2, 3, 15, 17), 5, "generic", (1, 7), (LAM, LAM)),         # generic loop, dump
    "gen_17x15": ((2, 3, 17, 15), 5, "generic", (1, 2), (LAM, LAM)),
    "c4_17x481": ((2, 2, 17, 481), 5, "generic", (1, 4), (LAM, LAM)),        # odd row length, falls to generic
    # per-channel: B = chunk + 1, a partial chunk (18 planes under one block norm: lambda = 0.06 for iso)
    "chunk_16x32": ((XPPG + 1, 2, 16, 32), 5, "fused", (1, 4), (LAM, 0.06)),
}


def lam_of(name, iso):
    return CASES[name][4][int(bool(iso))]


PARAMS = [(name, mode, iso, maxit) for name in CASES for mode in MODES for iso in ISOS for maxit in MAXITS]
# cases whose parameters keep every soft shrink off (tau = 1 above every |a|: no kink to stay away from), with
# the reason -- as mixed_psf_cases.KINK_FREE.  The block shrink of the same shape runs with active shrinks.
KINK_FREE = {p: "blurred 240 x 480 inputs, seeds 1-59: under 5 % of the difference pixels above tau at lambda 0.02 to "
                "0.005, and at 0.0025 a trajectory closer than 1e-5 tau to the kink"
             for p in PARAMS if p[0] == "smooth_240x480" and not p[2]}


def solve_bank(xin, lmbd, rho, kerns, iso, maxit, fmap=None, bmap=None, trace=None):
    """``maxit`` iterations from zero with the bank ``kerns`` (Bk, Ck, k, k) -> x, in xin's dtype.
    fmap / bmap: (B, C) table index maps for the Wiener factor / for b (None: the right one).
    trace: a list that receives (a_x, a_y) = D x_k + u_{k-1} of every iteration (detached)."""
    B, C, H, W = xin.shape
    dt = xin.dtype
    lmbd = torch.as_tensor(lmbd, dtype=dt)
    rho = torch.as_tensor(rho, dtype=dt)
    tau = lmbd / rho
    k = kerns.shape[-1]
    R = bc.right_map(kerns, B, C)
    fmap = R if fmap is None else fmap
    bmap = R if bmap is None else bmap
    tabs = kerns.reshape(-1, k, k)
    # the Wiener factor in the working dtype, built like deconv.py:46-57, per table
    sig = torch.fft.rfftn(tabs, s=(H, W), dim=(1, 2))
    s2 = sig.real ** 2 + sig.imag ** 2
    kx = torch.arange(W // 2 + 1, dtype=dt)
    ky = torch.arange(H, dtype=dt).reshape(H, 1)
    lap = (2 - 2 * torch.cos(2 * math.pi * kx / W)) + (2 - 2 * torch.cos(2 * math.pi * ky / H))
    fc = (1.0 / (s2 + rho * lap))[fmap]  # (B, C, H, W/2+1)
    b_t = torch.stack([apply_psf_transpose(xin, t.reshape(1, 1, k, k)) for t in tabs])  # (T, B, C, H, W)
    bi = torch.arange(B).reshape(B, 1).expand(B, C)
    ci = torch.arange(C).reshape(1, C).expand(B, C)
    b = b_t[bmap, bi, ci]
    wdx, wdy = _dw([[0, 0], [-1, 1]], C, xin), _dw([[0, -1], [0, 1]], C, xin)
    wdxt, wdyt = _dw([[1, -1], [0, 0]], C, xin), _dw([[1, 0], [-1, 0]], C, xin)
    back, fwd = (1, 0, 1, 0), (0, 1, 0, 1)
    shrink = shrink_block if iso else shrink_soft
    x = torch.zeros_like(xin)
    zx, zy, ux, uy = (torch.zeros_like(xin) for _ in range(4))
    for _ in range(int(maxit)):
        rhs = b + rho * (_circ_dwconv(zx - ux, wdxt, fwd) + _circ_dwconv(zy - uy, wdyt, fwd))
        x = torch.fft.irfftn(fc * torch.fft.rfftn(rhs, dim=(2, 3)), s=(H, W), dim=(2, 3))
        gx, gy = _circ_dwconv(x, wdx, back), _circ_dwconv(x, wdy, back)
        if trace is not None:
            trace.append(((gx + ux).detach(), (gy + uy).detach()))
        zx, zy = shrink(gx + ux, tau), shrink(gy + uy, tau)
        ux, uy = ux + gx - zx, uy + gy - zy
    return x


def grads(x, kerns, iso, maxit, cot, dtype=torch.float64, lam=LAM, rho=RHO, fmap=None, bmap=None):
    """solve_bank and its autograd in `dtype`: dict(out, gx, glam, grho, gk), gk shaped like kerns."""
    xd = x.detach().to(dtype).clone().requires_grad_(True)
    kd = kerns.detach().to(dtype).clone().requires_grad_(True)
    lt = torch.tensor([lam], dtype=dtype, requires_grad=True)
    rt = torch.tensor([rho], dtype=dtype, requires_grad=True)
    out = solve_bank(xd, lt, rt, kd, iso, maxit, fmap, bmap)
    g = torch.autograd.grad(out, (xd, lt, rt, kd), cot.to(dtype), allow_unused=True)
    z = torch.zeros(1, dtype=dtype)
    return dict(out=out.detach(), gx=g[0], glam=g[1] if g[1] is not None else z, grho=g[2] if g[2] is not None else z,
                gk=g[3])


def sum_by_map(gplane, m, T):
    """gk[t] = sum of the per-plane PSF gradients (B, C, k, k) over the planes p with m[p] == t."""
    k = gplane.shape[-1]
    out = torch.zeros(T, k, k, dtype=gplane.dtype)
    return out.index_add(0, m.reshape(-1), gplane.reshape(-1, k, k))


def per_table_err(got, ref):
    """The worst table's rel-L2: each k x k block against that table's own reference norm."""
    k = ref.shape[-1]
    g, r = got.detach().double().cpu().reshape(-1, k, k), ref.detach().double().cpu().reshape(-1, k, k)
    return max(tc.rel(g[t], r[t]) for t in range(r.shape[0]))


@functools.lru_cache(maxsize=None)
def case_input(name, iso):
    from admmtor.synth import blurred_batch, gaussian_psf
    shape, k, _, seeds, _ = CASES[name]
    return blurred_batch(*shape, gaussian_psf(k, 1.0), seed=seeds[int(bool(iso))])


@functools.lru_cache(maxsize=None)
def case_bank(name, mode):
    shape, k = CASES[name][:2]
    return bc.make_bank(mode, shape[0], shape[1], k)


@functools.lru_cache(maxsize=None)
def cotangent(name):
    shape = CASES[name][0]
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 + len(name) + shape[3]))


@functools.lru_cache(maxsize=None)
def reference(name, mode, iso, maxit):
    """Everything fp64 a test of one case needs, computed once and shared (do not modify): the input, the bank,
    the cotangent, the right step's dict(out, gx, glam, grho, gk) -- and the controls' condition, asserted here
    so that no test of the case can compare with the reference without it."""
    shape, k = CASES[name][:2]
    B, C = shape[:2]
    x, kerns, cot, lam = case_input(name, iso), case_bank(name, mode), cotangent(name), lam_of(name, iso)
    ref = grads(x, kerns, iso, maxit, cot, lam=lam)
    R = bc.right_map(kerns, B, C)
    T = kerns.shape[0] * kerns.shape[1]
    # the per-plane PSF gradients: the same solve with every plane's PSF a table of its own
    gplane = grads(x, kerns[R // kerns.shape[1], R % kerns.shape[1]], iso, maxit, cot, lam=lam)["gk"]
    own = tc.rel(sum_by_map(gplane, R, T), ref["gk"].reshape(T, k, k))
    assert own <= 1e-10, (name, mode, iso, maxit, own)
    controls = {}
    for what, m in bc.wrong_maps(kerns, B, C).items():
        assert not torch.equal(m, R), (name, mode, what)
        controls[what, "sum"] = tc.rel(sum_by_map(gplane, m, T), ref["gk"].reshape(T, k, k))
        controls[what, "factor"] = tc.rel(grads(x, kerns, iso, maxit, cot, lam=lam, fmap=m)["gk"], ref["gk"])
        controls[what, "b"] = tc.rel(grads(x, kerns, iso, maxit, cot, lam=lam, bmap=m)["gk"], ref["gk"])
    for key, e in controls.items():
        assert e >= CONTROL_MIN, (name, mode, iso, maxit, key, e)
    return {"x": x, "kerns": kerns, "cot": cot, "lam": lam, "ref": ref, "controls": controls}


def errors(got, ref):
    """rel-L2 errors of dict(out, gx, glam, grho, gk) against the reference's, gk also per table (gk_table)."""
    e = tc.errors(got, ref)
    e["gk_table"] = per_table_err(got["gk"], ref["gk"])
    return e


def check_gates(tag, e):
    assert e["out"] <= tc.GATE_FWD, (tag, e)
    for key in ("gx", "glam", "grho", "gk", "gk_table"):
        assert e[key] <= tc.GATE_GRAD_PSF, (tag, key, e)


def fitness(name, mode, iso, maxit):
    """(kink margin, active share) of the fp64 trajectory: the margin as kink_margins / iso_kink_margin take it
    (iterations 1..maxit-1; inf at maxit = 1), the share as train_cases.active_share (aniso: on iteration
    max(maxit - 1, 1); iso: on the last)."""
    lam = lam_of(name, iso)
    tau = lam / RHO
    tr = []
    solve_bank(case_input(name, iso).double(), lam, RHO, case_bank(name, mode).double(), iso, maxit, trace=tr)

    def dist(a):
        v = torch.sqrt((a * a).sum(dim=(0, 1)) + 1e-15) + 1e-15 if iso else a.abs()
        return ((v - tau).abs() / tau).min().item()
    margin = min([dist(a) for pair in tr[:maxit - 1] for a in pair], default=float("inf"))
    ax, ay = tr[maxit - 1] if iso else tr[max(maxit - 1, 1) - 1]
    if iso:
        on = [1.0 - tau / (torch.sqrt((a * a).sum(dim=(0, 1)) + 1e-15) + 1e-15) > 0 for a in (ax, ay)]
    else:
        on = [a.abs() > tau for a in (ax, ay)]
    return margin, torch.cat([o.reshape(-1) for o in on]).double().mean().item()
