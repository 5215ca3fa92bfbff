"""The case table of the fused mixed-radix training path with a learnable PSF (no test in here).

At a smooth size a module whose PSF is an nn.Parameter trains on the mixed kernels too: the forward keeps
every r_k's packed row spectra in the history, so its column pass k_pass_b_m runs out of place (history slot
in, spectrum buffer out) and its row pass writes r_{k+1} into the history; the backward forms the cross
spectra of the PSF gradient with k_xspec_m (csrc/mixed_kernels.hpp, MixedOps in admm_capi.hip).  This is
tests/mixed_cases.py's matrix for that ground, learn_psf = True in every case, with train_cases' Case,
inputs, reference, errors and gates: tests/test_gpu_mixed_psf.py runs every case on the GPU against the fp64
oracle's autograd at the fixed gates (every gradient, the PSF's included, <= 1e-3), and
tests/test_mixed_psf_case_inputs.py checks on the CPU that every case is fit for them.

  height   every column length of with_col (mixed_capi.hip): the smooth heights at W = 32 / 64, the
           power-of-two ones beside W = 480 -- the out-of-place column pass and k_xspec_m at every H
  width    a narrow (N = 240), a 2-wave (960) and a 4-wave (800) row plan beside H = 16, aniso and iso: the
           row pass writes r_{k+1} into the history
  maxit    1 and 2 at N = 240 and 960 (1: r_1 is the only kept spectrum)
  planes   nine planes: the cross spectra's last group of eight is partial
  cc       N = 540 beside an 8-column plan: the only row length of with_row that is no multiple of 8, so the
           only way to the 4-column instances of an 8-column plan (every length is a multiple of 4: the
           2-column fall-back of a wider plan cannot be reached); beside H = 16 and 32, and beside the smooth
           H = 240 and 540
  module   240 x 480, six iso iterations: the solve an ADMMDeconv layer with a 5 x 5 PSF runs

KINK_FREE.  From 512 rows on beside W = 480 a case with 5 % of its shrinks active does not exist: the fp64
trajectory comes within 1e-6 tau of the block kink at every seed tried and the reference's own fp32 x
gradient is then 5e-4 ... 3e-3 off.  The column kernels do not depend on the shrink state, and the row
kernels' two Jacobian branches are covered by the rest of this table and by mixed_cases.py, so those heights
come without an active shrink: one iteration (the output depends on no shrink), or three iterations with tau
above every |a| (lambda = rho = 0.2 aniso, lambda = 0.4 iso: a kink margin of ~0.5).  The active-share
condition does not apply to them; every other condition does.

Seeds (and the lambdas) are searched so that tests/test_mixed_psf_case_inputs.py passes for every case."""
from __future__ import annotations

from train_cases import G3, G5, M5, Case

_A, _I = False, True


def _p(name, shape, psf, iso, maxit, seed, group, **kw):
    return Case(name, shape, psf, iso, maxit, seed, learn_psf=True, group=group, **kw)


HEIGHT_CASES = [
    # the smooth column plans
    _p("p-h240-iso-gauss3", (1, 3, 240, 32), G3, _I, 5, 1, "height"),
    _p("p-h360-aniso-motion5", (1, 3, 360, 32), M5, _A, 5, 1, "height"),
    _p("p-h480-iso-gauss3", (1, 3, 480, 64), G3, _I, 5, 1, "height"),
    _p("p-h540-aniso-motion5", (1, 3, 540, 32), M5, _A, 5, 3, "height"),
    _p("p-h600-iso-gauss5", (1, 3, 600, 32), G5, _I, 5, 1, "height"),
    _p("p-h720-aniso-motion5", (1, 3, 720, 32), M5, _A, 5, 4, "height"),
    _p("p-h768-iso-gauss3", (1, 3, 768, 32), G3, _I, 5, 1, "height"),
    _p("p-h800-aniso-motion5", (1, 2, 800, 32), M5, _A, 5, 6, "height"),
    _p("p-h960-iso-gauss5", (1, 3, 960, 32), G5, _I, 5, 1, "height"),
    _p("p-h1080-aniso-gauss5", (1, 1, 1080, 64), G5, _A, 5, 2, "height"),
    _p("p-h1200-iso-gauss3", (1, 3, 1200, 32), G3, _I, 5, 1, "height"),
    _p("p-h1440-aniso-motion5", (1, 1, 1440, 32), M5, _A, 5, 1, "height"),
    _p("p-h1536-iso-motion5", (1, 3, 1536, 32), M5, _I, 5, 1, "height"),
    _p("p-h2160-iso-gauss3", (1, 3, 2160, 32), G3, _I, 4, 1, "height"),
    _p("p-h2160-aniso-gauss5", (1, 1, 2160, 32), G5, _A, 4, 1, "height"),
    # the power-of-two column plans beside 240-point rows
    _p("p-h16-aniso-motion5", (1, 3, 16, 480), M5, _A, 5, 1, "height"),
    _p("p-h32-aniso-motion5", (1, 3, 32, 480), M5, _A, 5, 1, "height"),
    _p("p-h64-iso-gauss5", (1, 3, 64, 480), G5, _I, 5, 1, "height"),
    _p("p-h128-aniso-gauss3", (1, 1, 128, 480), G3, _A, 4, 1, "height", lam=0.007),
    _p("p-h256-iso-gauss3", (1, 3, 256, 480), G3, _I, 4, 14, "height", lam=0.005),
    # kink-free from here on (KINK_FREE below)
    _p("p-h512-aniso-gauss3-maxit1", (1, 2, 512, 480), G3, _A, 1, 1, "height"),
    _p("p-h512-iso-motion5-tau2", (1, 2, 512, 480), M5, _I, 3, 1, "height", lam=0.4),
    _p("p-h1024-iso-gauss5-maxit1", (1, 2, 1024, 480), G5, _I, 1, 1, "height"),
    _p("p-h2048-aniso-motion5-maxit1", (1, 3, 2048, 480), M5, _A, 1, 1, "height"),
    _p("p-h4096-aniso-gauss5-tau1", (1, 1, 4096, 480), G5, _A, 3, 1, "height", lam=0.2),
    _p("p-h4096-iso-motion5-tau2", (1, 2, 4096, 480), M5, _I, 3, 1, "height", lam=0.4),
]
KINK_FREE = frozenset(c.name for c in HEIGHT_CASES if c.shape[2] >= 512 and c.shape[3] == 480)

WIDTH_CASES = [
    _p("p-n240-iso-gauss3", (1, 3, 16, 480), G3, _I, 5, 1, "width"),  # aniso: p-h16-aniso-motion5
    _p("p-n960-aniso-gauss5", (1, 3, 16, 1920), G5, _A, 5, 4, "width"),
    _p("p-n960-iso-motion5", (1, 3, 16, 1920), M5, _I, 5, 1, "width"),
    _p("p-n800-aniso-gauss3", (1, 3, 16, 1600), G3, _A, 5, 3, "width"),
    _p("p-n800-iso-motion5", (1, 3, 16, 1600), M5, _I, 5, 2, "width"),
]
MAXIT_CASES = [
    _p("p-n240-aniso-maxit1", (1, 3, 16, 480), G3, _A, 1, 1, "maxit"),
    _p("p-n240-iso-maxit2", (1, 3, 16, 480), M5, _I, 2, 1, "maxit"),
    _p("p-n960-iso-maxit1", (1, 3, 16, 1920), G5, _I, 1, 1, "maxit"),
    _p("p-n960-aniso-maxit2", (1, 3, 16, 1920), M5, _A, 2, 1, "maxit"),
]
PLANE_CASES = [
    _p("p-planes9-aniso-motion5", (3, 3, 16, 480), M5, _A, 5, 2, "planes"),
]
CC_CASES = [
    _p("p-n540-h16-aniso-motion5", (1, 3, 16, 1080), M5, _A, 5, 1, "cc"),
    _p("p-n540-h32-iso-gauss3", (1, 3, 32, 1080), G3, _I, 5, 1, "cc"),
    # smooth heights (guarded column stages at 4 columns a block); 1,080-pixel rows beside them keep 5 % of the
    # shrinks active and the trajectory off the kink only at a lower tau and two iterations
    _p("p-n540-h240-iso-motion5", (1, 3, 240, 1080), M5, _I, 2, 1, "cc", lam=0.004),
    _p("p-n540-h540-iso-motion5", (1, 3, 540, 1080), M5, _I, 2, 2, "cc", lam=0.004),
]
# the input and parameters test_gpu_mixed_psf.py gives an ADMMDeconv((5, 5), max_iters=6, iso=True) module
MODULE_CASE = _p("p-module-iso-gauss5", (1, 3, 240, 480), G5, _I, 6, 1, "module", lam=0.007)

TABLE_CASES = HEIGHT_CASES + WIDTH_CASES + MAXIT_CASES + PLANE_CASES + CC_CASES + [MODULE_CASE]
