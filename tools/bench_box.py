"""What bounds on x cost (admm_tv_forward_box), at C3 (64x3x1024^2) and HD (8x3x1080x1920), 21x21 Gaussian PSF,
aniso and iso:

  plain50    one plain 50-iteration solve                   fft_admm_tv
  box50      one 50-iteration solve with bounds (0, 1)      fft_admm_tv_box (project=False: the library's call)

  python tools/bench_box.py [rounds]
Interleaved rounds (default 5), HIP-event times, the median per variant; prints ms and the ratio, then the row
pass (pass A) of each variant from the library's per-kernel timers (one profiled solve each, after the timed
rounds): ms per launch, TB/s on its byte count (28 B/px plain, 36 B/px with bounds: v read and written; the iso
norm maps are two images per solve, not per plane, and are not counted) and the fraction of the 8 TB/s HBM
peak.  Where the A/B build of the library is present, the plain solve's row pass is also profiled with the
cooperative kernel off (ADMM_PASSA_COOP=0): the plain kernel the BOX instantiation derives from, the
like-for-like comparison at C3.  One JSON line per shape and shrinkage.  At HD the plain solve runs the fused
mixed-radix kernels and the solve with bounds the generic loop: the ratio there compares two paths, not two row
passes, and the generic aniso solve launches its step once per plane part (ADMM_GEN_STREAMS: twice the launches
over half the planes each, on two streams), so its per-launch TB/s is not a whole-image figure.  DESIGN.md §7h
holds the estimate from the bytes and the figures measured with this tool.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-admm-deconv_amd"))
import torch  # noqa: E402

from admmtor import _native  # noqa: E402
from admmtor.eops.deconv import fft_admm_tv, fft_admm_tv_box  # noqa: E402
from admmtor.synth import blurred_batch, make_psf  # noqa: E402

SHAPES = {"C3": (64, 3, 1024, 1024), "HD": (8, 3, 1080, 1920)}
LAM, RHO = 0.01, 0.02
PEAK_TBS = 8.0
ITERS = 50


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def pass_a_ms(fn):
    """ms per launch of the row pass (the generic path: the step fused into the row transform) in one solve."""
    _native.profile_enable(True)
    _native.profile_reset()
    fn()
    torch.cuda.synchronize()
    ms, n = _native.profile_read()
    _native.profile_enable(False)
    return (ms[0] / n[0], n[0]) if n[0] else (float("nan"), 0)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")
    psf = make_psf("gauss:3", 21).to(dev)
    for name, shape in SHAPES.items():
        x = blurred_batch(*shape, psf.cpu(), seed=1, device=dev)
        px = shape[0] * shape[1] * shape[2] * shape[3]
        for iso in (False, True):
            def plain50():
                fft_admm_tv(x, LAM, RHO, psf, iso, ITERS)

            def box50():
                fft_admm_tv_box(x, LAM, RHO, psf, 0.0, 1.0, iso, ITERS, project=False)

            variants = {"plain50": plain50, "box50": box50}
            for fn in variants.values():  # warm-up: allocator, tables, code objects
                fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(rounds):
                for k, fn in variants.items():
                    ms[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in ms.items()}
            d = _native.desc(*shape, 21, iso, ITERS)
            paths = {"plain50": _native.path(d, mode=0), "box50": _native.path(d, mode=3)}
            bytes_px = {"plain50": 28, "box50": 36}
            rowpass = {}
            for k, fn in variants.items():
                t, n = pass_a_ms(fn)
                tbs = bytes_px[k] * px / (t * 1e-3) / 1e12
                rowpass[k] = {"ms": round(t, 4), "launches": n, "bytes_per_px": bytes_px[k], "TBps": round(tbs, 3),
                              "of_peak": round(tbs / PEAK_TBS, 3)}
            if paths["plain50"] == "fused" and not iso and os.path.exists(_native.AB_LIB_PATH):
                os.environ["ADMM_PASSA_COOP"] = "0"  # the A/B build reads its knobs from the environment
                with _native.ab_library():
                    plain50()
                    t, n = pass_a_ms(plain50)
                del os.environ["ADMM_PASSA_COOP"]
                tbs = bytes_px["plain50"] * px / (t * 1e-3) / 1e12
                rowpass["plain50_noncoop"] = {"ms": round(t, 4), "launches": n, "bytes_per_px": bytes_px["plain50"],
                                              "TBps": round(tbs, 3), "of_peak": round(tbs / PEAK_TBS, 3)}
            res = {"shape": name, "iso": iso, "paths": paths, "rounds": rounds,
                   "ms": {k: round(v, 3) for k, v in med.items()},
                   "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                   "box_over_plain": round(med["box50"] / med["plain50"], 3), "row_pass": rowpass}
            print(f"{name} iso={iso}: plain50 ({paths['plain50']}) {med['plain50']:.2f} ms, box50 ({paths['box50']}) "
                  f"{med['box50']:.2f} ms, ratio {res['box_over_plain']}; row pass "
                  + ", ".join(f"{k} {v['ms']} ms = {v['TBps']} TB/s" for k, v in rowpass.items()), flush=True)
            print(json.dumps(res), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
