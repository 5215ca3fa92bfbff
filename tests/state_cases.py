"""Shared by the solver-state tests (test_state_restatement.py, test_gpu_state.py): an fp64 restatement of the
reference loop (deconv.py:103-115) with the state ``(z_x, z_y, u_x, u_y)`` exposed, the cases, and the negative
controls that give the tests teeth.

ADMM forgets where it started, so a long continuation would hide a wrong state: every case continues for only
K2 in {1, 2, 3} iterations, and before anything runs on the GPU the controls -- the same continuation from
six WRONG states -- must each miss the unsplit fp64 solve by at least CONTROL_MIN = 1e-4, ten times the 1e-5
gate the right state has to meet.
"""
import functools

import torch

from oracle.admm_oracle import (_circ_dwconv, _dw, apply_psf_transpose, rel_l2, shrink_block, shrink_soft,
                                solve_fourier, wiener_factor)

LAM, RHO, SEED = 0.01, 0.02, 3
TOL_REF64 = 1e-5
CONTROL_MIN = 1e-4

# (K1, K2): K1 iterations, the state handed over, K2 more
SPLITS = [(5, 1), (5, 2), (6, 3), (1, 1), (0, 2)]

# name -> (shape, psf or None, iso values, fused: the stateful solve must report a fused path)
CASES = {
    "pow2_16_lanepaired": ((2, 3, 16, 16), ("gauss:1.0", 5), (False, True), True),
    "pow2_1024_coop_pixel": ((1, 3, 32, 1024), ("gauss:1.5", 9), (False,), True),   # cooperative row pass, R = 2
    # ... whose (1, 1) split runs with a sharper PSF: behind gauss:1.5 no gradient of x_1 reaches tau = 0.5, so
    # z_1 is exactly zero and "z dropped" IS the true state (control 4.5e-15 at every seed tried, 1..8); with
    # gauss:1.0 k5 the weakest control is 3.9e-4
    "pow2_1024_coop_sharp": ((1, 3, 32, 1024), ("gauss:1.0", 5), (False,), True),
    "pow2_1024_plain_pixel": ((1, 3, 16, 1024), None, (False,), True),               # the cooperative kernel refuses it
    "pow2_1024_lanepaired": ((1, 2, 16, 1024), None, (True,), True),
    "pow2_2048": ((1, 2, 16, 2048), None, (False,), True),
    "smooth_240x480": ((1, 2, 240, 480), ("motion", 7), (False, True), True),
    "smooth_240x640": ((1, 1, 240, 640), None, (False,), True),                      # a second row plan
    "generic_15x17": ((1, 2, 15, 17), ("motion", 5), (False, True), False),
    "generic_one_row": ((2, 1, 1, 7), None, (False, True), False),
    "class4_17x481": ((1, 2, 17, 481), ("gauss:1.0", 5), (False, True), False),
    "class4_481x17": ((1, 2, 481, 17), ("gauss:1.0", 5), (False, True), False),
}

ONLY = {"pow2_1024_coop_sharp": [(1, 1)]}
SKIP = {"pow2_1024_coop_pixel": [(1, 1)]}
PARAMS = [(name, iso, k1, k2) for name, c in CASES.items() for iso in c[2]
          for (k1, k2) in ONLY.get(name, SPLITS) if (k1, k2) not in SKIP.get(name, ())]


def zero_state(x):
    return tuple(torch.zeros_like(x) for _ in range(4))


def restate(xin, lmbd, rho, kern, iso, maxit, state=None):
    """solve_spatial (oracle.admm_oracle) with the state exposed: ``maxit`` iterations from ``state`` ->
    ``(x, (z_x, z_y, u_x, u_y))``.  The reference's operator sequence (pad + depthwise conv, FFT x-update);
    H_t(xin) is evaluated once, as its value does not change."""
    B, C, H, W = xin.shape
    dt = xin.dtype
    lmbd = torch.as_tensor(lmbd, dtype=dt)
    rho = torch.as_tensor(rho, dtype=dt)
    tau = lmbd / rho
    fc = wiener_factor(H, W, kern, rho, dtype=torch.float64).to(dt)
    wdx, wdy = _dw([[0, 0], [-1, 1]], C, xin), _dw([[0, -1], [0, 1]], C, xin)
    wdxt, wdyt = _dw([[1, -1], [0, 0]], C, xin), _dw([[1, 0], [-1, 0]], C, xin)
    back, fwd = (1, 0, 1, 0), (0, 1, 0, 1)
    shrink = shrink_block if iso else shrink_soft
    b = apply_psf_transpose(xin, kern)
    zx, zy, ux, uy = (t.to(dt).clone() for t in (state if state is not None else zero_state(xin)))
    x = torch.zeros_like(xin)
    for _ in range(int(maxit)):
        rhs = b + rho * (_circ_dwconv(zx - ux, wdxt, fwd) + _circ_dwconv(zy - uy, wdyt, fwd))
        x = torch.fft.irfftn(fc * torch.fft.rfftn(rhs, dim=(2, 3)), s=(H, W), dim=(2, 3))
        gx, gy = _circ_dwconv(x, wdx, back), _circ_dwconv(x, wdy, back)
        zx, zy = shrink(gx + ux, tau), shrink(gy + uy, tau)
        ux, uy = ux + gx - zx, uy + gy - zy
    return x, (zx, zy, ux, uy)


def wrong_states(state):
    """The negative controls: states a faulty import / export could produce."""
    zx, zy, ux, uy = state
    o = torch.zeros_like(zx)
    return {
        "zero state": (o, o, o, o),
        "u dropped": (zx, zy, o, o),
        "z dropped": (o, o, ux, uy),
        "x and y swapped": (zy, zx, uy, ux),
        "u negated": (zx, zy, -ux, -uy),
        "u replaced by a": (zx, zy, zx + ux, zy + uy),  # a = D x + u_prev = z + u
    }


def make_input(shape, psf):
    from admmtor.synth import blurred_batch, make_psf
    k = make_psf(*psf) if psf else torch.empty(0)
    return blurred_batch(*shape, k, seed=SEED), k


@functools.lru_cache(maxsize=None)
def reference(name, iso, k1, k2):
    """Everything fp64 a test of one case needs, computed once: the inputs, the unsplit solve_fourier(K1 + K2),
    the restatement's state after K1 -- and the controls' condition, asserted here so that no test of the case
    can pass without it."""
    shape, psf, _, _ = CASES[name]
    x, k = make_input(shape, psf)
    xd, kd = x.double(), k.double()
    ref = solve_fourier(xd, LAM, RHO, kd, iso, k1 + k2)
    x1, st1 = restate(xd, LAM, RHO, kd, iso, k1)
    split, _ = restate(xd, LAM, RHO, kd, iso, k2, st1)
    assert rel_l2(split, ref) <= 1e-12, (name, iso, k1, k2, rel_l2(split, ref))
    controls = {}
    if k1 > 0:  # (from K1 = 0 the true state IS the zero state: that split covers the null-state entry instead)
        for what, bad in wrong_states(st1).items():
            controls[what] = rel_l2(restate(xd, LAM, RHO, kd, iso, k2, bad)[0], ref)
            assert controls[what] >= CONTROL_MIN, (name, iso, k1, k2, what, controls[what])
    return {"x": x, "k": k, "ref": ref, "x1": x1, "state1": st1, "controls": controls}
