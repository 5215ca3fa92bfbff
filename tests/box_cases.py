"""Shared by the tests of the solve with bounds on x (test_box_restatement.py, test_gpu_box.py): an fp64
restatement of the iteration admm_tv_forward_box runs, the cases, and the negative controls that give the
tests teeth.

The iteration (include/admm_tv.h, "bounds on x") splits w = x beside z = Dx, with one scaled dual v and the
same rho; everything else is the reference's loop (deconv.py:103-115), b = H_t(xin) and the zero start
(w_0 = v_0 = 0) included:

    fc_box = 1 / (|sigma|^2 + rho (|dx|^2 + |dy|^2 + 1))
    x_k = irfft2(fc_box rfft2(b + rho (Dx^T (z_x - u_x) + Dy^T (z_y - u_y)) + rho (w - v)))
    z, u as in the reference
    p = x_k + v;  w = min(max(p, lo), hi);  v = p - w

With infinite bounds v stays 0 and w = x_k, but rho x_k remains in the right-hand side: a proximal-point
variant, NOT fft_admm_tv's iterates.  So the GPU is compared with restate_box, never with solve_fourier;
restate_box(..., box=False) is pinned to solve_fourier (1e-12) so that the restatement's shared part is the
oracle's.

Teeth: before any test of a case can pass, seven wrong variants of the restatement (WRONG) must each miss the
right one by at least CONTROL_MIN = 1e-4, ten times the 1e-5 gate, at K = 3 and K = 6, and the share of pixels
whose p lies outside the bounds must stay between 5 % and 95 % in every iteration -- a projection that is
never or always active would leave most of the new arithmetic untested.
"""
import functools

import torch

from oracle.admm_oracle import (_circ_dwconv, _dw, apply_psf_transpose, rel_l2, shrink_block, shrink_soft,
                                wiener_factor)

LAM, RHO, SEED = 0.01, 0.02, 3
BOUNDS = (0.25, 0.75)
TOL_REF64 = 1e-5
CONTROL_MIN = 1e-4
# K = 1 runs no row pass (fc_box alone), K = 2 the row pass's first-iteration kernel, K = 3 the steady kernel
# (the first K at which accumulating v matters), K = 6 is the control point
KS = (1, 2, 3, 6)
CONTROL_KS = (3, 6)
ACTIVE_RANGE = (0.05, 0.95)

# name -> (shape, psf or None, iso values, the path admm_tv_path(desc, 3) must report)
CASES = {
    "pow2_16": ((2, 3, 16, 16), ("gauss:1.0", 5), (False, True), "fused"),         # lane-paired, sub-wave strips
    "pow2_64": ((1, 2, 32, 64), ("motion", 7), (False, True), "fused"),            # several strips per plane
    "pow2_256": ((1, 2, 32, 256), ("gauss:1.0", 5), (False,), "fused"),
    # inference would take the cooperative kernel here; the solve with bounds must not
    "pow2_1024_pixel": ((1, 3, 32, 1024), ("gauss:1.0", 5), (False,), "fused"),
    "pow2_1024_pl": ((1, 2, 16, 1024), None, (True,), "fused"),                    # lane-paired wide rows
    "pow2_2048": ((1, 2, 16, 2048), None, (False,), "fused"),                      # 16 values per lane
    "generic_15x17": ((1, 2, 15, 17), ("motion", 5), (False, True), "generic"),
    "generic_one_row": ((2, 1, 1, 7), None, (False, True), "generic"),             # neighbours wrap onto themselves
    "smooth_240x480": ((1, 2, 240, 480), ("motion", 7), (False,), "generic"),      # a smooth size: generic here
    "class4_17x481": ((1, 2, 17, 481), ("gauss:1.0", 5), (False,), "generic"),     # an odd row length: generic here
}
PARAMS = [(name, iso, K) for name, c in CASES.items() for iso in c[2] for K in KS]
CASE_PARAMS = [(name, iso) for name, c in CASES.items() for iso in c[2]]

# the wrong variants a faulty kernel could compute
WRONG = ("box term dropped", "fc without rho", "v dropped", "v sign flipped", "w dropped", "upper bound ignored",
         "v not accumulated")


def restate_box(xin, lmbd, rho, kern, iso, maxit, lo, hi, box=True, wrong=None, trace=None, active=None):
    """The iteration above in xin's dtype: `maxit` iterations from zero -> x_maxit.

    box=False: the reference's loop (no w, no v, the plain Wiener factor) -- solve_fourier's result.
    wrong: one of WRONG, a deliberately faulty variant (the negative controls).
    trace / active: lists that receive every x_k and every iteration's share of pixels with p outside [lo, hi]."""
    assert wrong is None or wrong in WRONG
    B, C, H, W = xin.shape
    dt = xin.dtype
    lmbd = torch.as_tensor(lmbd, dtype=dt)
    rho = torch.as_tensor(rho, dtype=dt)
    tau = lmbd / rho
    fc = wiener_factor(H, W, kern, rho, dtype=torch.float64)
    if box and wrong != "fc without rho":
        fc = fc / (1.0 + rho.double() * fc)  # 1 / (1 / fc + rho)
    fc = fc.to(dt)
    if wrong == "upper bound ignored":
        hi = float("inf")
    wdx, wdy = _dw([[0, 0], [-1, 1]], C, xin), _dw([[0, -1], [0, 1]], C, xin)
    wdxt, wdyt = _dw([[1, -1], [0, 0]], C, xin), _dw([[1, 0], [-1, 0]], C, xin)
    back, fwd = (1, 0, 1, 0), (0, 1, 0, 1)
    shrink = shrink_block if iso else shrink_soft
    b = apply_psf_transpose(xin, kern)
    zx, zy, ux, uy, w, v = (torch.zeros_like(xin) for _ in range(6))
    x = torch.zeros_like(xin)
    for _ in range(int(maxit)):
        rhs = b + rho * (_circ_dwconv(zx - ux, wdxt, fwd) + _circ_dwconv(zy - uy, wdyt, fwd))
        if box:
            term = {None: w - v, "fc without rho": w - v, "upper bound ignored": w - v, "v not accumulated": w - v,
                    "box term dropped": None, "v dropped": w, "v sign flipped": w + v, "w dropped": -v}[wrong]
            if term is not None:
                rhs = rhs + rho * term
        x = torch.fft.irfftn(fc * torch.fft.rfftn(rhs, dim=(2, 3)), s=(H, W), dim=(2, 3))
        gx, gy = _circ_dwconv(x, wdx, back), _circ_dwconv(x, wdy, back)
        zx, zy = shrink(gx + ux, tau), shrink(gy + uy, tau)
        ux, uy = ux + gx - zx, uy + gy - zy
        if box:
            p = x + v
            w = torch.clamp(p, lo, hi)
            v = (x if wrong == "v not accumulated" else p) - w
            if active is not None:
                active.append(((p < lo) | (p > hi)).double().mean().item())
        if trace is not None:
            trace.append(x)
    return x


def make_input(shape, psf):
    from admmtor.synth import blurred_batch, make_psf
    k = make_psf(*psf) if psf else torch.empty(0)
    return blurred_batch(*shape, k, seed=SEED), k


@functools.lru_cache(maxsize=None)
def restated(name, iso, lo, hi):
    """One case's inputs and fp64 iterates x_1 .. x_6 of the restatement with bounds (lo, hi), computed once:
    {"x", "k", "xs": [x_1, ...], "active": [...]}."""
    shape, psf, _, _ = CASES[name]
    x, k = make_input(shape, psf)
    xs, active = [], []
    restate_box(x.double(), LAM, RHO, k.double(), iso, max(KS), lo, hi, trace=xs, active=active)
    return {"x": x, "k": k, "xs": xs, "active": active}


@functools.lru_cache(maxsize=None)
def teeth(name, iso):
    """The controls of one case, asserted: {wrong variant: {K: its distance from the restatement}}."""
    r = restated(name, iso, *BOUNDS)
    for it, a in enumerate(r["active"], 1):
        assert ACTIVE_RANGE[0] <= a <= ACTIVE_RANGE[1], (name, iso, it, "share of pixels with p outside the bounds", a)
    xd, kd = r["x"].double(), r["k"].double()
    out = {}
    for what in WRONG:
        xs = []
        restate_box(xd, LAM, RHO, kd, iso, max(CONTROL_KS), *BOUNDS, wrong=what, trace=xs)
        out[what] = {K: rel_l2(xs[K - 1], r["xs"][K - 1]) for K in CONTROL_KS}
        for K, e in out[what].items():
            assert e >= CONTROL_MIN, (name, iso, K, what, e)
    return out


def reference(name, iso, K):
    """Everything fp64 a test of one case needs: the inputs and the restatement's x_K with BOUNDS -- and the
    case's teeth, asserted here so that no test of the case can pass without them."""
    controls = teeth(name, iso)
    r = restated(name, iso, *BOUNDS)
    return {"x": r["x"], "k": r["k"], "ref": r["xs"][K - 1], "controls": controls, "active": r["active"]}
