"""One training step with a PSF bank (fft_admm_tv_bank_train: forward with history plus backward, the PSFs
requiring grad) against the alternatives, 21x21 PSFs, aniso, 50 iterations, at C3-like and HD-like shapes whose
batch fits the history (2 K + K image-sized slots per step):

  shared     one learnable PSF for every plane                       fft_admm_tv
  per_image  a learnable PSF per image (B tables)                    fft_admm_tv_bank_train
  per_plane  a learnable PSF per image and channel (B C tables)      fft_admm_tv_bank_train
  loop       today's alternative: B single-image training steps      fft_admm_tv

  python tools/bench_bank_train.py [steps] [shape ...]
Warmed, HIP-event times, interleaved steps (default 10), the median per variant; prints ms per step, the ratios
to the shared-PSF step and to the loop, and one JSON line per shape.  DESIGN.md §7g is where the figures go.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-admm-deconv_amd"))
import torch  # noqa: E402

from admmtor import _native  # noqa: E402
from admmtor.eops.deconv import fft_admm_tv, fft_admm_tv_bank_train  # noqa: E402
from admmtor.synth import blurred_batch, gaussian_psf, motion_psf  # noqa: E402

SHAPES = {"C3": (8, 3, 1024, 1024), "HD": (4, 3, 1080, 1920)}
LAM, RHO, K, ITERS = 0.01, 0.02, 21, 50


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bank(n, dev):
    ps = [gaussian_psf(K, 1.5 + 0.02 * t) if t % 2 == 0 else motion_psf(K, 3.0 * t) for t in range(n)]
    return torch.cat(ps).to(dev)


def step(fn, x, kern):
    k = kern.detach().requires_grad_(True)
    fn(x, LAM, RHO, k, False, ITERS).square().sum().backward()
    return k.grad


def main():
    args = sys.argv[1:]
    steps = int(args[0]) if args else 10
    names = args[1:] or list(SHAPES)
    dev = torch.device("cuda:0")
    for name in names:
        shape = SHAPES[name]
        B, C, H, W = shape
        one = gaussian_psf(K, 3.0).to(dev)
        x = blurred_batch(*shape, one.cpu(), seed=1, device=dev)
        k_img = bank(B, dev).reshape(B, 1, K, K).contiguous()
        k_pl = bank(B * C, dev).reshape(B, C, K, K).contiguous()
        variants = {
            "shared": lambda: step(fft_admm_tv, x, one),
            "per_image": lambda: step(fft_admm_tv_bank_train, x, k_img),
            "per_plane": lambda: step(fft_admm_tv_bank_train, x, k_pl),
            "loop": lambda: [step(fft_admm_tv, x[b:b + 1], k_img[b:b + 1]) for b in range(B)],
        }
        for fn in variants.values():  # warm-up: allocator, tables, code objects
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(steps):
            for k, fn in variants.items():
                ms[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        TR, PG = _native.ADMM_TV_FLAG_PSF_BANK_TRAIN, _native.ADMM_TV_FLAG_PSF_GRAD
        flags = {"shared": PG, "per_image": PG | TR | _native.ADMM_TV_FLAG_PSF_PER_IMAGE,
                 "per_plane": PG | TR | _native.ADMM_TV_FLAG_PSF_PER_IMAGE | _native.ADMM_TV_FLAG_PSF_PER_CHANNEL}
        descs = {k: _native.desc(*shape, K, False, ITERS, flags=f) for k, f in flags.items()}
        res = {"shape": name, "dims": shape, "iso": False, "iterations": ITERS, "steps": steps,
               "paths": {k: _native.path(d, train=True) for k, d in descs.items()},
               "ms": {k: round(v, 3) for k, v in med.items()},
               "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
               "ratio_to_shared": {k: round(med[k] / med["shared"], 4) for k in med},
               "speedup_over_loop": {k: round(med["loop"] / med[k], 3) for k in med},
               "backward_workspace_MiB": {k: round(_native.backward_workspace_size(d) / 2 ** 20, 1) for k, d in descs.items()},
               "history_MiB": round(_native.history_size(descs["shared"]) / 2 ** 20, 1)}
        print(f"{name} {shape}: " + ", ".join(f"{k} {res['ms'][k]} ms ({res['speedup_over_loop'][k]:.2f}x the loop)"
                                             for k in med), flush=True)
        print(json.dumps(res), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
