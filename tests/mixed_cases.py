"""The case table of the fused mixed-radix training path's shape matrix (no test in here).

The smooth-size backend (csrc/mixed_kernels.hpp, mixed_capi.hip, MixedOps in admm_capi.hip) shares
fused_forward / fused_backward with the power-of-two one, whose matrix is tests/train_cases.py.  This is
the same matrix for the mixed kernels, with train_cases' Case, inputs, reference, errors and gates:
tests/test_gpu_mixed_shapes.py runs every case on the GPU against the fp64 oracle's autograd at the fixed
gates, tests/test_train_case_inputs.py checks on the CPU that every case is fit for them.  No case learns
its PSF: a PSF gradient keeps the generic path (Layout::mixed_train), so a PSF here is a fixed one (make_b
on the mixed transforms, apply_ht_t) and every case must answer "fused mixed-radix" for training.

  width    every row length N = W / 2 of with_row (mixed_capi.hip), aniso and iso: the power-of-two
           lengths beside H = 240 (N = 2048: beside H = 16, which 4,096-pixel rows turn into a mixed
           size), the smooth ones beside H = 16
  height   every column length of with_col beside a partner that makes the size a mixed one: the smooth
           heights at W = 32 / 64, the power-of-two heights beside W = 480
  maxit    1 and 2 on a narrow (N = 240), a 2-wave (N = 960) and a 4-wave (N = 800) row plan
  strip    solved with strips of R rows pinned in the A/B build (ADMM_MIXED_R); the rule itself gives R = 1
           for every shape in this file but the two tallest (m-h1024-iso: 2, m-h2048-iso: 3 in the backward)

Shapes stay thin.  A frame's active share falls with its area (at 240 x 1920 under 2 % of the
difference pixels sit above tau = 0.1), and lowering tau puts so many pixels near the kink that the
reference's own fp32 gradient leaves the gates; so wide rows come with 16 rows and tall columns with 32
or 64 pixels a row, where the defaults lambda = 0.02, rho = 0.2 work.  Where a length admits no thin mixed
size (the power-of-two N beside H = 240, the power-of-two H beside W = 480) the cases carry a lambda of
their own (tau 0.025 ... 0.05) and the largest have 3 iterations and, aniso, one plane; what is left
to the inference tests for that reason is listed at HEIGHT_CASES.  Seeds (and those lambdas) are searched
so that tests/test_train_case_inputs.py passes for every case, none exempted.

The iso cases keep the same distance from their kink: the block factor max(1 - tau / ||a||, 0) switches at
||a|| = tau as the soft threshold does at |a| = tau, and with 10^5 ... 10^6 pixels at these lower tau an fp32
solve does land on the other side somewhere unless the seed keeps the trajectory away (iso_kink_margin
below; 1024 x 480 at a margin of 3e-8 gave an x gradient 2e-3 off on the GPU with a forward error of 1.6e-7,
while the reference's own fp32 run happened to stay on the fp64 side)."""
from __future__ import annotations

from itertools import product

import torch

from train_cases import G3, G5, M5, Case, inputs

_A, _I = False, True


def _m(name, shape, psf, iso, maxit, seed, group, **kw):
    return Case(name, shape, psf, iso, maxit, seed, learn_psf=False, group=group, **kw)


# row lengths: N = W / 2.  Three planes leave the last block of strips partial at the narrow plans.
WIDTH_CASES = [
    # the power-of-two row plans beside 240-point columns
    _m("m-n16-aniso-motion5", (1, 3, 240, 32), M5, _A, 5, 1, "width"),
    _m("m-n16-iso", (1, 3, 240, 32), None, _I, 5, 102, "width"),
    _m("m-n32-aniso", (1, 3, 240, 64), None, _A, 5, 903, "width"),
    _m("m-n32-iso-gauss3", (1, 3, 240, 64), G3, _I, 5, 4, "width"),
    _m("m-n64-aniso", (1, 2, 240, 128), None, _A, 4, 5, "width", lam=0.007),
    _m("m-n64-iso", (1, 3, 240, 128), None, _I, 5, 6, "width", lam=0.01),
    _m("m-n128-aniso-gauss5", (1, 3, 240, 256), G5, _A, 5, 807, "width"),
    _m("m-n128-iso", (1, 3, 240, 256), None, _I, 5, 308, "width", lam=0.01),
    _m("m-n256-aniso", (1, 1, 240, 512), None, _A, 4, 409, "width", lam=0.0065),
    _m("m-n256-iso-motion5", (1, 3, 240, 512), M5, _I, 5, 1110, "width", lam=0.01),
    _m("m-n512-aniso", (1, 1, 240, 1024), None, _A, 3, 2111, "width", lam=0.005),
    _m("m-n512-iso", (1, 3, 240, 1024), None, _I, 4, 4412, "width", lam=0.01),
    _m("m-n1024-aniso", (1, 1, 240, 2048), None, _A, 3, 3313, "width", lam=0.005),
    _m("m-n1024-iso", (1, 3, 240, 2048), None, _I, 3, 314, "width", lam=0.008),
    _m("m-n2048-aniso", (1, 2, 16, 4096), None, _A, 5, 12, "width"),
    _m("m-n2048-iso-gauss5", (1, 3, 16, 4096), G5, _I, 5, 316, "width"),
    # the smooth row plans beside 16-point columns
    _m("m-n240-aniso", (1, 3, 16, 480), None, _A, 5, 2, "width"),
    _m("m-n240-iso-motion5", (1, 3, 16, 480), M5, _I, 5, 18, "width"),
    _m("m-n320-aniso-gauss3", (1, 3, 16, 640), G3, _A, 5, 19, "width"),
    _m("m-n320-iso", (1, 3, 16, 640), None, _I, 5, 20, "width"),
    _m("m-n360-aniso", (1, 3, 16, 720), None, _A, 5, 21, "width"),
    _m("m-n360-iso", (1, 3, 16, 720), None, _I, 5, 222, "width"),
    _m("m-n400-aniso", (1, 3, 16, 800), None, _A, 5, 23, "width"),
    _m("m-n400-iso-gauss5", (1, 3, 16, 800), G5, _I, 5, 24, "width"),
    _m("m-n480-aniso-motion5", (1, 3, 16, 960), M5, _A, 5, 125, "width"),
    _m("m-n480-iso", (1, 3, 16, 960), None, _I, 5, 26, "width"),
    _m("m-n540-aniso", (1, 3, 16, 1080), None, _A, 5, 627, "width"),
    _m("m-n540-iso", (1, 3, 16, 1080), None, _I, 5, 228, "width"),
    _m("m-n640-aniso", (1, 3, 16, 1280), None, _A, 5, 829, "width"),
    _m("m-n640-iso-gauss3", (1, 3, 16, 1280), G3, _I, 5, 30, "width"),
    _m("m-n720-aniso-gauss5", (1, 3, 16, 1440), G5, _A, 5, 131, "width"),
    _m("m-n720-iso", (1, 3, 16, 1440), None, _I, 5, 232, "width"),
    _m("m-n800-aniso", (1, 3, 16, 1600), None, _A, 5, 133, "width"),
    _m("m-n800-iso", (1, 3, 16, 1600), None, _I, 5, 134, "width"),
    _m("m-n960-aniso", (1, 3, 16, 1920), None, _A, 5, 7, "width"),
    _m("m-n960-iso-motion5", (1, 3, 16, 1920), M5, _I, 5, 36, "width"),
    _m("m-n1280-aniso", (1, 2, 16, 2560), None, _A, 5, 37, "width"),
    _m("m-n1280-iso", (1, 3, 16, 2560), None, _I, 5, 138, "width"),
    _m("m-n1920-aniso", (1, 1, 16, 3840), None, _A, 5, 639, "width"),
    _m("m-n1920-iso-gauss3", (1, 3, 16, 3840), G3, _I, 5, 40, "width"),
]

# column lengths.  H = 16 and 240 come with the width cases.  Three planes at 1536, 2160 and 2048: the
# column pass walks the planes in groups of two there (pb_tile; under 8 columns a block at H >= 1024), with
# a partial last group.  The power-of-two heights need W = 480 to make a mixed size, so from 256 rows on
# the cases are iso with a lower tau.
# Left to the inference tests (tests/test_gpu_mixed.py), which the reverse step's column pass shares its
# kernel with: H = 4096 (4096 x 480 at a tau that keeps 5 % of the pixels active: the reference's own fp32
# x gradient is 8e-4 from its fp64 one, iso); aniso at 512 x 480 and above (no seed in 240 keeps the
# trajectory 1e-5 tau from the kink with 5 % active).
HEIGHT_CASES = [
    _m("m-h360-aniso", (1, 3, 360, 32), None, _A, 5, 51, "height"),
    _m("m-h480-iso", (1, 3, 480, 64), None, _I, 5, 552, "height"),
    _m("m-h540-aniso-motion5", (1, 3, 540, 32), M5, _A, 5, 53, "height"),
    _m("m-h600-iso", (1, 3, 600, 32), None, _I, 5, 154, "height"),
    _m("m-h720-aniso", (1, 2, 720, 64), None, _A, 5, 55, "height", lam=0.006),
    _m("m-h768-iso-gauss3", (1, 3, 768, 32), G3, _I, 5, 56, "height"),
    _m("m-h800-aniso", (1, 2, 800, 32), None, _A, 5, 57, "height"),
    _m("m-h960-iso", (1, 3, 960, 64), None, _I, 5, 1458, "height", lam=0.01),
    _m("m-h1080-aniso-gauss5", (1, 1, 1080, 64), G5, _A, 5, 2, "height"),
    _m("m-h1200-iso", (1, 3, 1200, 32), None, _I, 5, 60, "height"),
    _m("m-h1440-aniso", (1, 1, 1440, 32), None, _A, 5, 261, "height"),
    _m("m-h1536-iso-motion5", (1, 3, 1536, 32), M5, _I, 5, 62, "height"),
    _m("m-h1536-aniso", (1, 3, 1536, 32), None, _A, 4, 263, "height"),
    _m("m-h2160-aniso", (1, 1, 2160, 32), None, _A, 4, 64, "height"),
    _m("m-h2160-iso", (1, 3, 2160, 32), None, _I, 4, 65, "height"),
    # the power-of-two column plans beside 240-point rows
    _m("m-h32-aniso", (1, 3, 32, 480), None, _A, 5, 166, "height"),
    _m("m-h64-iso-gauss5", (1, 3, 64, 480), G5, _I, 5, 67, "height"),
    _m("m-h128-aniso", (1, 1, 128, 480), None, _A, 4, 168, "height", lam=0.007),
    _m("m-h256-iso", (1, 3, 256, 480), None, _I, 5, 169, "height", lam=0.01),
    _m("m-h512-iso", (1, 3, 512, 480), None, _I, 4, 8770, "height", lam=0.008),
    _m("m-h1024-iso", (1, 3, 1024, 480), None, _I, 3, 72, "height", lam=0.008),
    _m("m-h2048-iso", (1, 3, 2048, 480), None, _I, 3, 8173, "height", lam=0.008),
]

# 1: the LASTK && FIRSTK reverse step alone, the FIRST row pass the only one; 2: the first reverse step is
# the last but one.  N = 240: a narrow row group; 960: two waves; 800: four waves.
MAXIT_CASES = [
    _m(f"m-{tag}-{'iso' if iso else 'aniso'}-maxit{it}", shape, None, iso, it, seed, "maxit")
    for ((tag, shape), iso, it), seed in zip(product(
        (("n240", (1, 3, 16, 480)), ("n960", (1, 3, 16, 1920)), ("n800", (1, 3, 16, 1600))), (_A, _I), (1, 2)),
        (80, 181, 82, 83, 84, 185, 86, 187, 88, 89, 90, 91))
]

# Strip heights.  240 rows, three planes, N = 16 / 32 (64 / 32 strips a block): R = 15 makes 48 strips, a
# partial last block of a narrow plan; 6 iterations keep the backward workspace (maxit x strips partial
# pairs, rounded up to 256 bytes) strictly smaller from each R to the next.  16 rows, three planes: N = 960
# (two waves, two strips a block) has an odd strip count at R = 16 -- the wide group past the last strip
# redoes it without storing; N = 800 (four waves) runs one strip a block.
STRIP_TALL = (1, 2, 3, 5, 8, 15, 16, 30)
STRIP_WIDE = (1, 2, 4, 8, 16)
STRIP_CASES = [
    (_m("mr-n16-aniso-motion5", (1, 3, 240, 32), M5, _A, 6, 1, "strip"), STRIP_TALL),
    (_m("mr-n32-iso", (1, 3, 240, 64), None, _I, 6, 491, "strip"), STRIP_TALL),
    (_m("mr-n960-aniso", (1, 3, 16, 1920), None, _A, 5, 7, "strip"), STRIP_WIDE),
    (_m("mr-n960-iso", (1, 3, 16, 1920), None, _I, 5, 693, "strip"), STRIP_WIDE),
    (_m("mr-n800-aniso", (1, 3, 16, 1600), None, _A, 5, 133, "strip"), STRIP_WIDE),
    (_m("mr-n800-iso", (1, 3, 16, 1600), None, _I, 5, 395, "strip"), STRIP_WIDE),
]
STRIP_RUNS = [(c, R) for c, rs in STRIP_CASES for R in rs]

TABLE_CASES = WIDTH_CASES + HEIGHT_CASES + MAXIT_CASES
# every solve the GPU tests compare with the oracle: the CPU input check covers all
ALL_SOLVES = TABLE_CASES + [c for c, _ in STRIP_CASES]


def iso_kink_margin(case: Case) -> float:
    """oracle.admm_oracle.kink_margins for the block shrink: min over iterations 1..maxit-1 and pixels of
    | ||a||_(B,C) - tau | / tau on the fp64 trajectory.  The block factor max(1 - tau / ||a||, 0) has the soft
    threshold's kink at ||a|| = tau -- its Jacobian jumps from 0 to a a^T / tau^2 there -- so an fp32 solver
    that lands on the other side of it has a legitimately different gradient, as in the aniso case."""
    from oracle.admm_oracle import shrink_block, solve_fourier
    x, k = inputs(case)
    x, k = x.double(), k.double()
    tau = case.lam / case.rho
    _, st = solve_fourier(x, case.lam, case.rho, k, True, 0, return_state=True)
    b, fc = st["b"], st["fc"]
    H, W = x.shape[2:]
    ux, uy, wx, wy = (torch.zeros_like(x) for _ in range(4))
    margin = float("inf")
    for _ in range(case.maxit - 1):
        r = b + case.rho * ((wx - torch.roll(wx, -1, 3)) + (wy - torch.roll(wy, -1, 2)))
        xx = torch.fft.irfftn(fc * torch.fft.rfftn(r, dim=(2, 3)), s=(H, W), dim=(2, 3))
        ax = xx - torch.roll(xx, 1, 3) + ux
        ay = xx - torch.roll(xx, 1, 2) + uy
        for a in (ax, ay):
            n = torch.sqrt(torch.sum(a * a, dim=(0, 1)) + 1e-15) + 1e-15
            margin = min(margin, ((n - tau).abs() / tau).min().item())
        zx, zy = shrink_block(ax, tau), shrink_block(ay, tau)
        ux, uy = ax - zx, ay - zy
        wx, wy = zx - ux, zy - uy
    return margin
