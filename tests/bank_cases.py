"""Shared by the PSF-bank tests (test_bank_restatement.py, test_gpu_psf_bank.py): an fp64 restatement of the
reference loop (deconv.py:103-115) with a PSF per image, per channel or per plane, the cases, and the negative
controls that give the tests teeth.

The restatement is built only from the oracle's own pieces, per table: ``wiener_factor`` and
``apply_psf_transpose`` of every PSF of the bank, ``shrink_soft`` / ``shrink_block`` (the block norm over ALL
planes, as the reference's), and the difference stencils of ``state_cases.restate``.  Plane ``(b, c)`` takes the
Wiener factor of table ``fmap[b, c]`` and ``b = H_t(xin)`` of table ``bmap[b, c]``; both default to the bank's
index ``(b if Bk > 1 else 0) * Ck + (c if Ck > 1 else 0)``, and the controls mis-index either alone or both.

Before anything runs on a GPU the controls -- the same solve with the tables of the wrong planes -- must each miss
the right fp64 solve by at least CONTROL_MIN = 1e-3 rel-L2, a hundred times the 1e-5 gate the kernels have to meet.
"""
import functools

import torch

from oracle.admm_oracle import (_circ_dwconv, _dw, apply_psf_transpose, rel_l2, shrink_block, shrink_soft,
                                solve_fourier, wiener_factor)

LAM, RHO, SEED = 0.01, 0.02, 3
TOL_REF64 = 1e-5
CONTROL_MIN = 1e-3

MODES = ("image", "channel", "plane")
ISOS = (False, True)
MAXITS = (1, 3)

# name -> (shape, k, the path admm_tv_path reports for modes 0 and 2)
CASES = {
    "pow2_16x16": ((2, 3, 16, 16), 5, "fused"),                    # k_pass_b (N < 16)
    "pow2_16x32": ((2, 3, 16, 32), 5, "fused"),                    # k_pass_b2
    "pow2_1024x32": ((2, 2, 1024, 32), 5, "fused"),                # k_pass_b at H = 1024: E = 16, packed factors, plane order 2
    "smooth_240x480": ((2, 3, 240, 480), 7, "fused mixed-radix"),  # k_pass_b_m, real and CM
    "gen_15x17": ((2, 3, 15, 17), 5, "generic"),                   # k_gcol, two plane parts
    "gen_17x15": ((2, 3, 17, 15), 5, "generic"),                   # H = 17: the matrix-core column plan's size
    "c4_17x481": ((2, 2, 17, 481), 5, "generic"),                  # odd row length -> generic
    "c4_481x17": ((2, 2, 481, 17), 5, "generic"),                  # transposed odd -> generic, wrapper not entered
}
PARAMS = [(name, mode, iso, maxit) for name in CASES for mode in MODES for iso in ISOS for maxit in MAXITS]


def bank_psfs(k):
    """Six distinct k x k PSFs, cycled through a bank's tables."""
    from admmtor.synth import gaussian_psf, make_psf, motion_psf
    return [gaussian_psf(k, 0.7), motion_psf(k, 30), gaussian_psf(k, 1.5), motion_psf(k, 120), make_psf("random", k),
            gaussian_psf(k, 1.0)]


def bank_dims(mode, B, C):
    return {"image": (B, 1), "channel": (1, C), "plane": (B, C), "shared": (1, 1)}[mode]


def make_bank(mode, B, C, k, first=0):
    """(Bk, Ck, k, k) fp32 bank of `mode`: table t is PSF (first + t) % 6 of bank_psfs."""
    Bk, Ck = bank_dims(mode, B, C)
    ps = bank_psfs(k)
    return torch.cat([ps[(first + t) % len(ps)] for t in range(Bk * Ck)]).reshape(Bk, Ck, k, k).contiguous()


def right_map(kerns, B, C):
    """(B, C) table index of every plane: the library's contract (include/admm_tv.h)."""
    Bk, Ck = kerns.shape[:2]
    b = torch.arange(B).reshape(B, 1).expand(B, C)
    c = torch.arange(C).reshape(1, C).expand(B, C)
    return (b if Bk > 1 else 0 * b) * Ck + (c if Ck > 1 else 0 * c)


def wrong_maps(kerns, B, C):
    """Index maps a faulty kernel could use instead."""
    Bk, Ck = kerns.shape[:2]
    T = Bk * Ck
    R = right_map(kerns, B, C)
    b = torch.arange(B).reshape(B, 1).expand(B, C)
    c = torch.arange(C).reshape(1, C).expand(B, C)
    maps = {
        "table 0": torch.zeros_like(R),
        "next plane's table": torch.roll(R.reshape(-1), -1).reshape(B, C),
        "bank reversed": T - 1 - R,
    }
    if Bk > 1 and Ck > 1:
        maps["b and c swapped"] = c * B + b
        maps["image index only"] = b.clone()
        maps["channel index only"] = c.clone()
    return maps


def bank_tables(xin, kerns, rho):
    """Per table t: the Wiener factor (T, H, W/2+1) and H_t of every plane with that PSF (T, B, C, H, W)."""
    B, C, H, W = xin.shape
    k = kerns.shape[-1]
    tabs = kerns.reshape(-1, 1, 1, k, k)
    fc = torch.stack([wiener_factor(H, W, t, rho, dtype=torch.float64).to(xin.dtype) for t in tabs])
    b = torch.stack([apply_psf_transpose(xin, t.to(xin.dtype)) for t in tabs])
    return fc, b


def restate(xin, lmbd, rho, kerns, iso, maxit, state=None, fmap=None, bmap=None, tables=None):
    """``maxit`` iterations from ``state`` (None: zeros) with the bank ``kerns`` -> ``(x, (z_x, z_y, u_x, u_y))``.
    fmap / bmap: (B, C) table index maps for the Wiener factor / for b (None: the right one).  tables:
    bank_tables(xin, kerns, rho), when the caller has them already."""
    B, C, H, W = xin.shape
    dt = xin.dtype
    lmbd = torch.as_tensor(lmbd, dtype=dt)
    rho = torch.as_tensor(rho, dtype=dt)
    tau = lmbd / rho
    R = right_map(kerns, B, C)
    fmap = R if fmap is None else fmap
    bmap = R if bmap is None else bmap
    fc_t, b_t = tables if tables is not None else bank_tables(xin, kerns, rho)
    fc = fc_t[fmap]  # (B, C, H, W/2+1)
    bi = torch.arange(B).reshape(B, 1).expand(B, C)
    ci = torch.arange(C).reshape(1, C).expand(B, C)
    b = b_t[bmap, bi, ci]  # (B, C, H, W)
    wdx, wdy = _dw([[0, 0], [-1, 1]], C, xin), _dw([[0, -1], [0, 1]], C, xin)
    wdxt, wdyt = _dw([[1, -1], [0, 0]], C, xin), _dw([[1, 0], [-1, 0]], C, xin)
    back, fwd = (1, 0, 1, 0), (0, 1, 0, 1)
    shrink = shrink_block if iso else shrink_soft
    zx, zy, ux, uy = (t.to(dt).clone() for t in (state if state is not None else [torch.zeros_like(xin)] * 4))
    x = torch.zeros_like(xin)
    for _ in range(int(maxit)):
        rhs = b + rho * (_circ_dwconv(zx - ux, wdxt, fwd) + _circ_dwconv(zy - uy, wdyt, fwd))
        x = torch.fft.irfftn(fc * torch.fft.rfftn(rhs, dim=(2, 3)), s=(H, W), dim=(2, 3))
        gx, gy = _circ_dwconv(x, wdx, back), _circ_dwconv(x, wdy, back)
        zx, zy = shrink(gx + ux, tau), shrink(gy + uy, tau)
        ux, uy = ux + gx - zx, uy + gy - zy
    return x, (zx, zy, ux, uy)


@functools.lru_cache(maxsize=None)
def case_input(name):
    from admmtor.synth import blurred_batch, gaussian_psf
    shape, k, _ = CASES[name]
    return blurred_batch(*shape, gaussian_psf(k, 1.0), seed=SEED)


@functools.lru_cache(maxsize=None)
def case_tables(name, mode, first=0):
    """The bank of a case and mode with its fp64 tables, computed once."""
    shape, k, _ = CASES[name]
    kerns = make_bank(mode, shape[0], shape[1], k, first)
    return kerns, bank_tables(case_input(name).double(), kerns.double(), RHO)


@functools.lru_cache(maxsize=None)
def reference(name, mode, iso, maxit):
    """Everything fp64 a test of one case needs, computed once: the input, the bank, the right solve -- and the
    controls' condition, asserted here so that no test of the case can pass without it."""
    shape, k, _ = CASES[name]
    B, C = shape[:2]
    x = case_input(name)
    kerns, tables = case_tables(name, mode)
    xd, kd = x.double(), kerns.double()
    ref, state = restate(xd, LAM, RHO, kd, iso, maxit, tables=tables)
    R = right_map(kerns, B, C)
    controls = {}
    for what, m in wrong_maps(kerns, B, C).items():
        assert not torch.equal(m, R), (name, mode, what)
        for part, (fm, bm) in {"factor": (m, None), "b": (None, m), "both": (m, m)}.items():
            e = rel_l2(restate(xd, LAM, RHO, kd, iso, maxit, fmap=fm, bmap=bm, tables=tables)[0], ref)
            controls[what, part] = e
            assert e >= CONTROL_MIN, (name, mode, iso, maxit, what, part, e)
    return {"x": x, "kerns": kerns, "ref": ref, "state": state, "controls": controls}


def pin_shared(name, iso, maxit):
    """rel-L2 of the restatement with a (1, 1, k, k) bank against solve_fourier."""
    shape, k, _ = CASES[name]
    xd = case_input(name).double()
    kd = make_bank("shared", shape[0], shape[1], k).double()
    return rel_l2(restate(xd, LAM, RHO, kd, iso, maxit)[0], solve_fourier(xd, LAM, RHO, kd, iso, maxit))


def pin_per_image(name, maxit):
    """rel-L2 of the aniso per-image restatement against the per-image solve_fourier calls, concatenated."""
    shape, k, _ = CASES[name]
    xd = case_input(name).double()
    kd = make_bank("image", shape[0], shape[1], k).double()
    loop = torch.cat([solve_fourier(xd[b:b + 1], LAM, RHO, kd[b:b + 1], False, maxit) for b in range(shape[0])])
    return rel_l2(restate(xd, LAM, RHO, kd, False, maxit)[0], loop)
