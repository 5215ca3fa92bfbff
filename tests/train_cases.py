"""The case table of the fused training path's shape matrix (no test in here).

tests/test_gpu_train_shapes.py runs every case on the GPU against the fp64 oracle's autograd with
fixed gates and no near-kink exemption; tests/test_train_case_inputs.py is what makes that
legitimate: on the CPU, with the oracle alone, it checks that every case stays away from the soft
threshold's kink, runs both branches of the shrink Jacobian, and that the reference op sequence in
fp32 already meets the gates.  Both import the table and the helpers below, so they cannot drift.

Shapes are the smallest that still reach the kernel instantiation named by the group:

  width    the row kernels RowOps<N>, N = W / 2 in {8, 128, 512, 1024} (HIST k_pass_a, history
           k_iso_norm, k_bwd_pass_a, k_bwd_iso_q); three planes of 16 rows leave the last block of
           strips partial
  height   the column kernels pass_b_h<H> (out of place with a learnable PSF) and xspec_h<H>,
           H in {256, 1024, 2048, 4096}; H = 16 comes with the width cases
  maxit    1: the LASTK && FIRSTK reverse step alone; 2: the first reverse step is also the last but one
  strip    solved with strips of R = 2, 4, 8, 16 rows pinned in the A/B build
  grouped  three modules with their own lambda / rho whose planes share blocks of strips

lambda = 0.02, rho = 0.2 (tau = 0.1): on blurred_batch inputs 6-25 % of the difference pixels sit
above the threshold after the first iteration.  Seeds of the aniso cases are picked so that
kink_margins >= 1e-5 on every plane (test_train_case_inputs.py asserts it)."""
from __future__ import annotations

from dataclasses import dataclass, replace
from itertools import product
from typing import Optional, Tuple, Union

import torch

LAM, RHO = 0.02, 0.2

# gates (relative L2), the project's own (tests/test_gpu_grad.py)
GATE_FWD = 1e-5
GATE_GRAD = 1e-4      # x, lambda, rho gradients without a PSF
GATE_GRAD_PSF = 1e-3  # every gradient, the PSF's included, with a PSF

KINK_MARGIN = 1e-5    # ten times the distance at which test_gpu_grad.py stops trusting an fp32 gradient
ACTIVE_SHARE = (0.05, 0.95)

G3, M5, M7, G5, G9 = ("gauss:0.7", 3), ("motion", 5), ("motion", 7), ("gauss:1.0", 5), ("gauss:1.5", 9)


@dataclass(frozen=True)
class Case:
    name: str
    shape: Tuple[int, int, int, int]
    psf: Optional[Tuple[str, int]]
    iso: bool
    maxit: int
    seed: int
    learn_psf: bool = False
    lam: Union[float, Tuple[float, ...]] = LAM   # a tuple: one value per module (grouped solve)
    rho: Union[float, Tuple[float, ...]] = RHO
    group: str = "width"
    module: int = 0   # index of a grouped case's module (modules()): it has a cotangent of its own

    def __str__(self):
        return self.name

    @property
    def gate(self) -> float:
        return GATE_GRAD_PSF if self.psf else GATE_GRAD


def _c(name, shape, psf, iso, maxit, seed, group, **kw):
    return Case(name, shape, psf, iso, maxit, seed, learn_psf=psf is not None and group != "grouped", group=group, **kw)


WIDTH_CASES = [
    _c("w16-aniso", (1, 3, 16, 16), None, False, 6, 1, "width"),
    _c("w16-iso-gauss3", (1, 3, 16, 16), G3, True, 5, 2, "width"),
    _c("w256-iso-motion5", (1, 3, 16, 256), M5, True, 5, 3, "width"),
    _c("w256-aniso", (1, 3, 16, 256), None, False, 6, 104, "width"),
    _c("w1024-aniso-gauss9", (1, 3, 32, 1024), G9, False, 5, 1305, "width"),
    _c("w1024-iso", (1, 3, 16, 1024), None, True, 6, 106, "width"),
    _c("w1024-aniso", (1, 3, 16, 1024), None, False, 5, 707, "width"),
    _c("w2048-aniso-motion7", (1, 3, 32, 2048), M7, False, 5, 408, "width"),
    _c("w2048-iso", (1, 2, 16, 2048), None, True, 6, 9, "width"),
]
HEIGHT_CASES = [
    _c("h256-aniso-motion5", (1, 2, 256, 16), M5, False, 5, 110, "height"),
    _c("h1024-iso", (1, 2, 1024, 32), None, True, 6, 11, "height"),
    _c("h2048-aniso-gauss5", (1, 1, 2048, 16), G5, False, 5, 112, "height"),
    _c("h4096-iso", (1, 1, 4096, 16), None, True, 5, 113, "height"),
    _c("h4096-iso-gauss5", (1, 1, 4096, 16), G5, True, 5, 14, "height"),
]
MAXIT_CASES = [
    _c(f"{tag}-{'iso' if iso else 'aniso'}-maxit{it}", shape, None, iso, it, 20 + i, "maxit")
    for i, ((tag, shape), iso, it) in enumerate(product(
        (("w1024", (1, 3, 16, 1024)), ("w2048", (1, 2, 16, 2048))), (False, True), (1, 2)))
]
# 32 rows: 16 strips of 2 rows per plane, 4 of 8, 2 of 16.  At N = 512 (four strips per block) the three
# planes make 48 strips of 2 rows (whole blocks), 12 of 8 (none partial), 6 of 16 (the second block partial).
STRIP_CASES = [
    replace(WIDTH_CASES[4], name="r-w1024-aniso-gauss9", group="strip"),
    _c("r-w1024-iso", (1, 3, 32, 1024), None, True, 5, 31, "strip"),
    _c("r-w2048-aniso", (1, 2, 32, 2048), None, False, 5, 432, "strip"),
    _c("r-w64-iso", (1, 3, 32, 64), None, True, 6, 33, "strip"),
]
STRIP_ROWS = (2, 4, 8, 16)
# Three modules: at W = 16 a block of the row kernels holds 64 strips of 2 rows = eight 16-row planes, so
# modules of three planes change inside a block (W = 32: six planes a module, 48 of a block's 64 strips).
_GL, _GR = (0.02, 0.03, 0.015), (0.2, 0.25, 0.2)
GROUPED_CASES = [
    _c("g-w16-aniso", (1, 3, 16, 16), None, False, 6, 41, "grouped", lam=_GL, rho=_GR),
    _c("g-w16-iso", (1, 3, 16, 16), None, True, 6, 142, "grouped", lam=_GL, rho=_GR),
    _c("g-w32-aniso-motion5", (2, 3, 16, 32), M5, False, 5, 43, "grouped", lam=_GL, rho=_GR),
]
# the history row pass beside the cooperative (inference) one
COOP_CASE = STRIP_CASES[0]

TABLE_CASES = WIDTH_CASES + HEIGHT_CASES + MAXIT_CASES


def modules(case: Case):
    """The single-module cases of a grouped one (same input, the module's lambda / rho)."""
    if not isinstance(case.lam, tuple):
        return [case]
    return [replace(case, name=f"{case.name}-m{m}", lam=l, rho=r, module=m)
            for m, (l, r) in enumerate(zip(case.lam, case.rho))]


# every (single-module) solve the GPU tests compare with the oracle: the CPU input check covers all
ALL_SOLVES = TABLE_CASES + STRIP_CASES[1:] + [m for c in GROUPED_CASES for m in modules(c)]


def rel(a, b) -> float:
    a = torch.as_tensor(a).double().cpu().reshape(-1)
    b = torch.as_tensor(b).double().cpu().reshape(-1)
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b)).item()


def scalar_err(got, ref) -> float:
    """Relative error of a lambda / rho gradient; absolute where the reference is exactly 0 (lambda at
    maxit = 1), as tests/test_gpu_grad.py does."""
    ref = torch.as_tensor(ref).double().cpu().reshape(-1)
    got = torch.as_tensor(got).double().cpu().reshape(-1)
    return rel(got, ref) if ref.abs().max().item() > 0 else got.abs().max().item()


_inputs, _oracle = {}, {}


def cotangent(case: Case) -> torch.Tensor:
    """The fixed-seed cotangent of a case's output (one per module of a grouped case)."""
    g = torch.Generator().manual_seed(1000 + case.seed + 100 * case.module)
    return torch.randn(case.shape, generator=g)


def inputs(case: Case):
    """(x, psf) fp32 on the CPU; psf is empty without one.  Shared: do not modify."""
    key = (case.shape, case.psf, case.seed)
    if key not in _inputs:
        from admmtor.synth import blurred_batch, make_psf
        k = make_psf(*case.psf) if case.psf else torch.empty(0)
        _inputs[key] = (blurred_batch(*case.shape, k, seed=case.seed), k)
    return _inputs[key]


def oracle_grads(case: Case, dtype=torch.float64):
    """solve_spatial (the reference's op sequence) and its autograd in `dtype`:
    dict(out, gx, glam, grho, gk); gk is None unless the PSF is learnable."""
    assert not isinstance(case.lam, tuple)
    from oracle.admm_oracle import solve_spatial
    x, k = inputs(case)
    c = cotangent(case)
    xd = x.to(dtype).requires_grad_(True)
    lam = torch.tensor([case.lam], dtype=dtype, requires_grad=True)
    rho = torch.tensor([case.rho], dtype=dtype, requires_grad=True)
    kd = k.to(dtype).requires_grad_(case.learn_psf)
    out = solve_spatial(xd, lam, rho, kd, case.iso, case.maxit)
    wrt = (xd, lam, rho) + ((kd,) if case.learn_psf else ())
    g = torch.autograd.grad(out, wrt, c.to(dtype), allow_unused=True)
    z = torch.zeros(1, dtype=dtype)
    return dict(out=out.detach(), gx=g[0], glam=g[1] if g[1] is not None else z,
                grho=g[2] if g[2] is not None else z, gk=g[3] if case.learn_psf else None)


def reference(case: Case):
    """The fp64 oracle's output and gradients of a case, computed once.  Shared: do not modify."""
    key = replace(case, name="", group="")
    if key not in _oracle:
        _oracle[key] = oracle_grads(case)
    return _oracle[key]


def difference_pixels(case: Case, k: int):
    """(a_x, a_y) of iteration k >= 1 in fp64: a_k = D x_k + u_{k-1}, what the shrink of iteration k sees."""
    from oracle.admm_oracle import solve_fourier
    x, kern = inputs(case)
    x, kern = x.double(), kern.double()
    _, st = solve_fourier(x, case.lam, case.rho, kern, case.iso, k - 1, return_state=True)
    xk = solve_fourier(x, case.lam, case.rho, kern, case.iso, k)
    return xk - torch.roll(xk, 1, 3) + st["ux"], xk - torch.roll(xk, 1, 2) + st["uy"]


def active_share(case: Case) -> float:
    """Share of the difference pixels whose shrink is active (|a| > tau; iso: block factor > 0), so that both
    branches of the shrink Jacobian run.  Aniso: on the last iteration kink_margins walks (maxit - 1; the
    first where maxit = 1); iso: on the final iteration."""
    tau = case.lam / case.rho
    ax, ay = difference_pixels(case, case.maxit if case.iso else max(case.maxit - 1, 1))
    if case.iso:
        on = [1.0 - tau / (torch.sqrt((a * a).sum(dim=(0, 1)) + 1e-15) + 1e-15) > 0 for a in (ax, ay)]
    else:
        on = [a.abs() > tau for a in (ax, ay)]
    return torch.cat([o.reshape(-1) for o in on]).double().mean().item()


def errors(got: dict, ref: dict) -> dict:
    """Relative-L2 errors of dict(out, gx, glam, grho[, gk]) against the reference's."""
    e = dict(out=rel(got["out"], ref["out"]), gx=rel(got["gx"], ref["gx"]),
             glam=scalar_err(got["glam"], ref["glam"]), grho=scalar_err(got["grho"], ref["grho"]))
    if ref.get("gk") is not None:
        e["gk"] = rel(got["gk"], ref["gk"])
    return e


def check_gates(case: Case, e: dict) -> None:
    assert e["out"] <= GATE_FWD, (case.name, e)
    for key in ("gx", "glam", "grho", "gk"):
        if key in e:
            assert e[key] <= case.gate, (case.name, key, e)


def fmt(e: dict) -> str:
    return " ".join(f"{k} {v:.2e}" for k, v in e.items())
