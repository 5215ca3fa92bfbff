"""What carrying the solver state costs (admm_tv_forward_state), at C3 (64x3x1024^2) and HD (8x3x1080x1920),
21x21 Gaussian PSF, aniso and iso:

  plain50    one plain 50-iteration solve                       fft_admm_tv
  chain5x10  five chained 10-iteration stateful solves           fft_admm_tv_state, state handed on
  state50    one 50-iteration stateful solve (state out)         fft_admm_tv_state

  python tools/bench_state.py [rounds]
Interleaved rounds (default 5), HIP-event times, the median per variant; prints ms, the cost of one
10-iteration chunk in plain iterations, and one JSON line per shape.  DESIGN.md §7f holds the estimate from the
bytes (a chunk ~ two extra iterations) and the figures measured with this tool.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-admm-deconv_amd"))
import torch  # noqa: E402

from admmtor import _native  # noqa: E402
from admmtor.eops.deconv import fft_admm_tv, fft_admm_tv_state  # noqa: E402
from admmtor.synth import blurred_batch, make_psf  # noqa: E402

SHAPES = {"C3": (64, 3, 1024, 1024), "HD": (8, 3, 1080, 1920)}
LAM, RHO = 0.01, 0.02


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")
    psf = make_psf("gauss:3", 21).to(dev)
    for name, shape in SHAPES.items():
        x = blurred_batch(*shape, psf.cpu(), seed=1, device=dev)
        for iso in (False, True):
            def plain50():
                fft_admm_tv(x, LAM, RHO, psf, iso, 50)

            def chain5x10():
                st = None
                for _ in range(5):
                    _, st = fft_admm_tv_state(x, LAM, RHO, psf, iso, 10, st)

            def state50():
                fft_admm_tv_state(x, LAM, RHO, psf, iso, 50)

            variants = {"plain50": plain50, "chain5x10": chain5x10, "state50": state50}
            for fn in variants.values():  # warm-up: allocator, tables, code objects
                fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(rounds):
                for k, fn in variants.items():
                    ms[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in ms.items()}
            it = med["plain50"] / 50
            path = _native.path(_native.desc(*shape, 21, iso, 10), mode=2)
            res = {"shape": name, "iso": iso, "path": path, "rounds": rounds,
                   "ms": {k: round(v, 3) for k, v in med.items()},
                   "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                   "plain_ms_per_iteration": round(it, 4),
                   "chunk10_in_plain_iterations": round(med["chain5x10"] / 5 / it, 2),
                   "state50_in_plain_iterations": round(med["state50"] / it, 2)}
            print(f"{name} iso={iso} ({path}): plain50 {med['plain50']:.2f} ms, chain5x10 {med['chain5x10']:.2f} ms, "
                  f"state50 {med['state50']:.2f} ms; a 10-iteration chunk costs "
                  f"{res['chunk10_in_plain_iterations']} plain iterations", flush=True)
            print(json.dumps(res), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
