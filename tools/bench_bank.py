"""What a PSF bank costs and what it saves (ADMM_TV_FLAG_PSF_PER_IMAGE / _PER_CHANNEL; fft_admm_tv_bank), at C3
(64x3x1024^2) and HD (8x3x1080x1920), 21x21 PSFs, aniso, 50 iterations:

  shared     one PSF for every plane                              fft_admm_tv
  per_image  a PSF per image (B tables)                           fft_admm_tv_bank
  per_plane  a PSF per image and channel (B C tables)             fft_admm_tv_bank
  loop       today's alternative: B calls of one image each       fft_admm_tv

  python tools/bench_bank.py [steps]
Warmed, HIP-event times, interleaved steps (default 20), the median per variant; prints iterations/s, the ratios
to the shared-PSF solve and to the loop, and one JSON line per shape.  DESIGN.md §7g holds the estimate from the
bytes (a factor per plane in the column pass) and the figures measured with this tool.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-admm-deconv_amd"))
import torch  # noqa: E402

from admmtor import _native  # noqa: E402
from admmtor.eops.deconv import fft_admm_tv, fft_admm_tv_bank  # noqa: E402
from admmtor.synth import blurred_batch, gaussian_psf, motion_psf  # noqa: E402

SHAPES = {"C3": (64, 3, 1024, 1024), "HD": (8, 3, 1080, 1920)}
LAM, RHO, K, ITERS = 0.01, 0.02, 21, 50


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bank(n, dev):
    """n distinct 21x21 PSFs: Gaussians of growing width and motion blurs of turning angle."""
    ps = [gaussian_psf(K, 1.5 + 0.02 * t) if t % 2 == 0 else motion_psf(K, 3.0 * t) for t in range(n)]
    return torch.cat(ps).to(dev)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    for name, shape in SHAPES.items():
        B, C, H, W = shape
        one = gaussian_psf(K, 3.0).to(dev)
        x = blurred_batch(*shape, one.cpu(), seed=1, device=dev)
        k_img = bank(B, dev).reshape(B, 1, K, K).contiguous()
        k_pl = bank(B * C, dev).reshape(B, C, K, K).contiguous()

        def shared():
            fft_admm_tv(x, LAM, RHO, one, False, ITERS)

        def per_image():
            fft_admm_tv_bank(x, LAM, RHO, k_img, False, ITERS)

        def per_plane():
            fft_admm_tv_bank(x, LAM, RHO, k_pl, False, ITERS)

        def loop():
            for b in range(B):
                fft_admm_tv(x[b:b + 1], LAM, RHO, k_img[b:b + 1], False, ITERS)

        variants = {"shared": shared, "per_image": per_image, "per_plane": per_plane, "loop": loop}
        for fn in variants.values():  # warm-up: allocator, tables, code objects
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(steps):
            for k, fn in variants.items():
                ms[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        flags = {"shared": 0, "per_image": _native.ADMM_TV_FLAG_PSF_PER_IMAGE,
                 "per_plane": _native.ADMM_TV_FLAG_PSF_PER_IMAGE | _native.ADMM_TV_FLAG_PSF_PER_CHANNEL}
        paths = {k: _native.path(_native.desc(*shape, K, False, ITERS, flags=f)) for k, f in flags.items()}
        paths["loop"] = _native.path(_native.desc(1, C, H, W, K, False, ITERS))
        ws = {k: _native.workspace_size(_native.desc(*shape, K, False, ITERS, flags=f)) for k, f in flags.items()}
        res = {"shape": name, "iso": False, "iterations": ITERS, "steps": steps, "paths": paths,
               "ms": {k: round(v, 3) for k, v in med.items()},
               "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
               "iterations_per_s": {k: round(1e3 * ITERS / v, 1) for k, v in med.items()},
               "ratio_to_shared": {k: round(med[k] / med["shared"], 4) for k in med},
               "speedup_over_loop": {k: round(med["loop"] / med[k], 3) for k in med},
               "workspace_MiB": {k: round(v / 2 ** 20, 1) for k, v in ws.items()}}
        print(f"{name} ({paths['shared']}): " + ", ".join(
            f"{k} {res['iterations_per_s'][k]} it/s ({res['ratio_to_shared'][k]:.3f}x shared time)" for k in med),
            flush=True)
        print(json.dumps(res), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
