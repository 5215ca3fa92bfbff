"""The case table of the generic backend's training path at every transform plan (no test in here).

Training at a size that is neither a power of two nor smooth, every fp64 solve and every fp32 solve past
eops.deconv.F32_MAX_PRIME run on the generic kernels (generic_kernels.hpp, run_forward_gen / run_backward_gen
in admm_capi.hip).  tests/test_gpu_generic_train.py differentiates every case below on the GPU against the
fp64 oracle's autograd at train_cases' fixed gates; tests/test_generic_train_case_inputs.py shows on the CPU,
with the oracle alone, that every case is fit for them (kink margin, active share, the reference op sequence
in fp32 within half of each gate) and that a solve with one iteration fewer misses the reference by >= 1e-2.

A case names in `group` the plan class it is there for: "col:<class>" (H carries it, W is 1-9), "row:<class>"
(W carries it, H is 1-9), "edge" (planes whose neighbours coincide) or "f32max" (the fp64 route of an fp32
solve).  The classes are the kernel instantiations of a line's transform plan:

  blue128 ... blue1024  a Bluestein stage of that size M (BM > 0)
  direct                a prime radix above 512 on the O(R)-per-output stage
  r11_13                radix-11 / radix-13 butterflies
  wide                  >= 1,024 points without a Bluestein stage: 512-thread blocks
  twg                   twiddles read from global memory (TWG)
  glb                   the line buffers in global scratch too (GLB)
  mm                    the matrix-core column pass (k_gcol_mm) / row inverse (k_grow_inv_mm)
  pow2, prime           fp64 only: a power of two, a prime radix above 5 (the double kernels have no Bluestein)

The library has no host query for a generic plan, so the selection is restated here: make_plan_radices,
make_plan, make_plan_f64, glds, gen_wide, mm_plan and mm_plan_row of admm_capi.hip, with their constants read
from the source.  line_tags() turns a plan into the classes above; test_table_reaches_every_class asserts that
every case still reaches the class it names and that the table is complete.

lambda = 0.02, rho = 0.2 as in train_cases (lambda = 0.01 at 107 x 214); seeds picked so that every case passes
the CPU check."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field
from typing import List

import torch

import train_cases as tc
from train_cases import G3, G5, M5, Case, _c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torch-admm-deconv_amd", "csrc")

# ------------------------------------------------------------------ the library's constants, from its source
_capi = open(os.path.join(CSRC, "admm_capi.hip")).read()
_gk = open(os.path.join(CSRC, "generic_kernels.hpp")).read()


def _int(pattern, text=_capi):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


BLUE_MIN = _int(r'env_int\("ADMM_BLUE_MIN", (\d+)\)')
BLUE_MAX_M = _int(r"2 \* R - 1 > (\d+)\) continue;")
MAX_LDS = _int(r"constexpr size_t kMaxLds = (\d+) \* 1024;") * 1024
GEN_WIDE_MIN = _int(r'env_int\("ADMM_GEN_WIDE_MIN", (\d+)\)')
GENERIC_MAX = _int(r"constexpr int64_t kGenericMax = (\d+);")
GNT = _int(r"#define ADMM_GNT (\d+)", _gk)
_mm_lo, _mm_hi = (int(v) for v in re.search(r"if \(big < (\d+) \|\| big > (\d+)\) return m;", _capi).groups())
MM_COL_S = [s for s in range(1, _int(r"for \(int S = 1; S <= (\d+); \+\+S\)") + 1)
            if s != _int(r"if \(S == (\d+) \|\| H % S\) continue;")]
MM_ROW_S = [int(v) for v in re.search(r"for \(int S : \{([\d, ]+)\}\) \{\s*if \(W % S\)", _capi).group(1).split(",")]
_e = re.search(r"blue_e\(int M\) \{ return M <= (\d+) \? (\d+) : M <= (\d+) \? (\d+) : (\d+); \}", _gk)
_BE = [int(v) for v in _e.groups()]
CF, CD = 8, 16  # bytes of a complex value: fp32, fp64


def blue_e(M):
    return _BE[1] if M <= _BE[0] else _BE[3] if M <= _BE[2] else _BE[4]


# ------------------------------------------------------------------ the plan selection, restated
@dataclass
class Plan:
    n: int
    rad: List[int] = field(default_factory=list)
    bst: List[int] = field(default_factory=list)
    bm: int = 0
    ntab: int = 0
    xslots: int = 0
    twg: bool = False
    glb: bool = False


def _take_all(p, m, q):
    while m % q == 0 and m > 1:
        p.rad.append(q)
        m //= q
    return m


def _other_primes(n, small, first):
    """The primes of n beyond `small`, ascending, by trial division from `first` (make_plan_radices / _f64)."""
    r = n
    for q in small:
        while r % q == 0:
            r //= q
    out, f = [], first
    while f * f <= r:
        if r % f == 0:
            out.append(f)
            while r % f == 0:
                r //= f
        f += 2
    if r > 1:
        out.append(r)
    return out


def make_plan_radices(n):
    """Any prime beyond 13 first, then 16, 8, 4, 2, 3, 5, 7, 11, 13 (ADMM_GPLAN_PRIME_FIRST, ADMM_GPLAN_R16)."""
    p, m = Plan(n), n
    for q in _other_primes(n, (2, 3, 5, 7, 11, 13), 11) + [16, 8, 4, 2, 3, 5, 7, 11, 13]:
        m = _take_all(p, m, q)
    assert m == 1 or n == 1
    return p


def glds(n, lines, p, csz=CF):
    if p.glb:
        return 0
    return csz * ((0 if p.twg else n + p.ntab) + 2 * n * lines + p.xslots)


def _is_blue(R):
    return BLUE_MIN > 0 and R > 7 and (R & (R - 1)) != 0 and R >= BLUE_MIN and 2 * R - 1 <= BLUE_MAX_M


def make_plan_f64(n):
    p, m = Plan(n), n
    for q in _other_primes(n, (2, 3, 5), 7) + [4, 2, 3, 5]:
        m = _take_all(p, m, q)
    p.bst = [0] * len(p.rad)
    p.twg = glds(n, 1, p, CD) > MAX_LDS
    p.glb = p.twg and glds(n, 1, p, CD) > MAX_LDS
    return p


def make_plan(n, f64=False):
    if f64:
        return make_plan_f64(n)
    p = make_plan_radices(n)
    M = 0
    for R in p.rad:
        if _is_blue(R):
            m = 32
            while m < 2 * R - 1:
                m *= 2
            M = max(M, m)
    p.bst = [M if (M > 0 and _is_blue(R)) else 0 for R in p.rad]
    p.bm = M
    p.ntab = sum(R + 2 * M for R, b in zip(p.rad, p.bst) if b)
    p.xslots = (GNT // (M // blue_e(M))) * (M + M // 8) if M > 0 else 0
    if glds(n, 1, p) <= MAX_LDS:
        return p
    q = make_plan_radices(n)
    q.bst = [0] * len(q.rad)
    q.twg = glds(n, 1, q) > MAX_LDS
    q.glb = q.twg and glds(n, 1, q) > MAX_LDS
    return q


def gen_wide(n, p):
    return p.bm == 0 and GEN_WIDE_MIN > 0 and n >= GEN_WIDE_MIN


def _largest_prime(n):
    big, f = 1, 2
    while f * f <= n:
        while n % f == 0:
            big, n = f, n // f
        f += 1
    return max(big, n)


def _mm(n, S_list, row):
    """(R, S) of the matrix-core plan of a line, or None: mm_plan (columns) / mm_plan_row (rows)."""
    if n < _mm_lo:
        return None
    big = _largest_prime(n)
    if big < _mm_lo or big > _mm_hi:
        return None
    for S in S_list:
        if n % S:
            continue
        R = n // S
        if R > _mm_hi or not (R & 1) or R % big:
            continue
        h = (R - 1) // 2
        KS, MT = (h + 4) // 4, (h + 16) // 16
        G = 1 if MT == 3 else 4 // MT
        tiles = lambda NL: ((NL * S + 7) // 8 + G - 1) // G
        NL = 16
        while NL > 1 and ((row and NL * (h + 1) > 256) or tiles(NL) > 8):
            NL //= 2
        if (row and NL * (h + 1) > 256) or tiles(NL) > 8:
            return None
        RP = max(4 * NL * S, 32 * ((NL * S + 7) // 8))
        while RP % 64 != 32:
            RP += 16
        stage = 2 * NL * (n // 2 + 1) * 2 if row else 0
        lds = max(stage, 4 * KS * RP) * 4 + n * CF
        return (R, S) if lds <= MAX_LDS else None
    return None


def mm_plan(H):
    return _mm(H, MM_COL_S, False)


def mm_plan_row(W):
    return _mm(W, MM_ROW_S, True)


def line_tags(n, f64=False):
    """The plan classes the forward / inverse LDS transforms of an n-point line fall in."""
    p = make_plan(n, f64)
    tags = set()
    if p.glb:
        tags.add("glb")
    elif p.twg:
        tags.add("twg")
    if f64:
        if any(r > 5 for r in p.rad):
            tags.add("prime")
        if n > 1 and (n & (n - 1)) == 0:
            tags.add("pow2")
        return tags
    if p.bm:
        tags.add(f"blue{p.bm}")
    if any(r > 512 for r, b in zip(p.rad, p.bst) if not b):
        tags.add("direct")
    if 11 in p.rad or 13 in p.rad:
        tags.add("r11_13")
    if gen_wide(n, p):
        tags.add("wide")
    return tags


def col_tags(case, f64=False):
    """A case's column classes: the matrix-core pass replaces the LDS column pass where its plan holds."""
    if not f64 and mm_plan(case.shape[2]):
        return {"mm"}
    return line_tags(case.shape[2], f64)


def row_tags(case, f64=False):
    """A case's row classes: the forward rows run the LDS plan; the matrix-core plan takes the row inverse."""
    t = line_tags(case.shape[3], f64)
    return t | ({"mm"} if not f64 and mm_plan_row(case.shape[3]) else set())


BLUE = ("blue128", "blue256", "blue512", "blue1024")
CLASSES = BLUE + ("direct", "r11_13", "wide", "twg", "glb", "mm")
CLASSES_F64 = ("prime", "pow2", "twg", "glb")

# ------------------------------------------------------------------ the table
# Every class twice per dimension: with a learnable PSF (the column spectrum dump and the MODE 3 column pass feed
# only the PSF gradient) and without one; both shrink modes; maxit 2-3, and 1 on one class of each kind.
COL_CASES = [
    _c("c301-blue128-aniso-gauss3", (1, 2, 301, 6), G3, False, 3, 1, "col:blue128"),
    _c("c301-blue128-iso", (1, 2, 301, 5), None, True, 2, 2, "col:blue128"),
    _c("c469-blue256-iso-motion5", (1, 1, 469, 7), M5, True, 2, 1, "col:blue256"),
    _c("c469-blue256-aniso", (2, 1, 469, 4), None, False, 3, 2, "col:blue256"),
    _c("c131-blue512-aniso-gauss5", (1, 3, 131, 9), G5, False, 2, 1, "col:blue512"),
    _c("c131-blue512-iso-gauss3-maxit1", (1, 2, 131, 4), G3, True, 1, 2, "col:blue512"),
    _c("c131-blue512-aniso", (1, 2, 131, 3), None, False, 3, 1, "col:blue512"),
    _c("c257-blue1024-iso-gauss3", (1, 1, 257, 8), G3, True, 3, 2, "col:blue1024"),
    _c("c257-blue1024-aniso", (1, 2, 257, 3), None, False, 2, 1, "col:blue1024"),
    _c("c521-direct-aniso-motion5", (1, 1, 521, 5), M5, False, 2, 2, "col:direct"),
    _c("c521-direct-iso", (1, 2, 521, 3), None, True, 3, 1, "col:direct"),
    _c("c143-r11_13-iso-gauss5", (1, 2, 143, 7), G5, True, 3, 1, "col:r11_13"),
    _c("c143-r11_13-aniso", (1, 3, 143, 2), None, False, 2, 2, "col:r11_13"),
    _c("c1026-wide-aniso-gauss3", (1, 1, 1026, 6), G3, False, 2, 1, "col:wide"),
    _c("c1026-wide-iso", (1, 2, 1026, 3), None, True, 2, 2, "col:wide"),
    _c("c8192-twg-iso-gauss3", (1, 1, 8192, 5), G3, True, 2, 1, "col:twg"),
    _c("c8192-twg-aniso", (1, 1, 8192, 4), None, False, 2, 2, "col:twg"),
    _c("c12000-glb-aniso-gauss3", (1, 1, 12000, 3), G3, False, 2, 3, "col:glb"),
    _c("c12000-glb-iso", (1, 1, 12000, 2), None, True, 2, 2, "col:glb"),
    _c("c148-mm4-iso-motion5", (1, 2, 148, 9), M5, True, 3, 1, "col:mm"),
    _c("c136-mm8-aniso", (1, 1, 136, 5), None, False, 2, 1, "col:mm"),
    _c("c214-mm2-aniso-gauss3-maxit1", (1, 2, 214, 3), G3, False, 1, 1, "col:mm"),
]
ROW_CASES = [
    _c("r301-blue128-iso-gauss3", (1, 2, 5, 301), G3, True, 3, 1, "row:blue128"),      # an odd W
    _c("r301-blue128-aniso", (1, 1, 7, 301), None, False, 2, 1, "row:blue128"),
    _c("r469-blue256-aniso-motion5", (1, 1, 6, 469), M5, False, 2, 1, "row:blue256"),  # an odd W
    _c("r469-blue256-iso", (1, 2, 3, 469), None, True, 3, 2, "row:blue256"),
    _c("r262-blue512-iso-gauss5", (1, 2, 9, 262), G5, True, 2, 1, "row:blue512"),
    _c("r262-blue512-aniso-maxit1", (1, 3, 4, 262), None, False, 1, 2, "row:blue512"),
    _c("r514-blue1024-aniso-gauss3", (1, 1, 8, 514), G3, False, 3, 1, "row:blue1024"),
    _c("r514-blue1024-iso", (2, 1, 2, 514), None, True, 2, 1, "row:blue1024"),
    _c("r521-direct-iso-gauss3", (1, 1, 4, 521), G3, True, 2, 1, "row:direct"),
    _c("r521-direct-aniso", (1, 2, 3, 521), None, False, 3, 2, "row:direct"),
    _c("r286-r11_13-aniso-motion5", (1, 2, 7, 286), M5, False, 3, 1, "row:r11_13"),
    _c("r286-r11_13-iso", (1, 3, 2, 286), None, True, 2, 2, "row:r11_13"),
    _c("r1026-wide-iso-gauss3", (1, 1, 5, 1026), G3, True, 2, 1, "row:wide"),
    _c("r1026-wide-aniso", (1, 2, 3, 1026), None, False, 2, 2, "row:wide"),
    _c("r8192-twg-aniso-gauss3", (1, 1, 4, 8192), G3, False, 2, 2, "row:twg"),
    _c("r8192-twg-iso", (1, 1, 5, 8192), None, True, 2, 2, "row:twg"),
    _c("r12000-glb-iso-gauss3", (1, 1, 3, 12000), G3, True, 2, 1, "row:glb"),
    _c("r12000-glb-aniso", (1, 1, 2, 12000), None, False, 2, 2, "row:glb"),
    _c("r107-mm1-aniso", (1, 1, 9, 107), None, False, 3, 1, "row:mm"),                 # 9 rows in all: the last line has one
    _c("r214-mm2-iso-gauss5", (1, 2, 7, 214), G5, True, 2, 2, "row:mm"),
    _c("r481-mm13-aniso-gauss3", (1, 3, 5, 481), G3, False, 3, 1, "row:mm"),
    _c("r481-mm13-iso-maxit1", (1, 2, 6, 481), None, True, 1, 2, "row:mm"),
]
# (lambda = 0.01: at 107 x 214 pixels under 5 % of the shrinks are active at 0.02)
# both matrix-core plans: where inference pitches the spectrum rows (Layout::ldw) and training keeps W / 2 + 1
BOTH_MM_CASES = [
    _c("c107-r214-both-mm-aniso-gauss5", (1, 2, 107, 214), G5, False, 2, 3, "col:mm", lam=0.01),
    _c("c107-r214-both-mm-iso", (1, 1, 107, 214), None, True, 3, 3, "row:mm", lam=0.01),
]
# planes whose left / right (upper / lower) neighbours coincide or are the pixel itself
EDGE_CASES = [
    _c("e1x7-aniso", (2, 2, 1, 7), None, False, 3, 1, "edge"),
    _c("e7x1-iso", (2, 2, 7, 1), None, True, 3, 2, "edge"),
    _c("e2x2-aniso", (2, 3, 2, 2), None, False, 3, 1, "edge"),
    _c("e2x9-iso", (1, 2, 2, 9), None, True, 2, 2, "edge"),
    _c("e9x2-aniso", (1, 2, 9, 2), None, False, 3, 1, "edge"),
    _c("e9x2-aniso-maxit1", (1, 2, 9, 2), None, False, 1, 2, "edge"),
    _c("e3x3-iso-gauss3", (2, 2, 3, 3), G3, True, 3, 3, "edge"),
]
# an fp32 solve past F32_MAX_PRIME: cast through the fp64 train / backward entry points, fp32 gradients back
F32MAX_CASE = _c("f32max-13003-aniso-gauss3", (1, 1, 3, 13003), G3, False, 2, 5, "f32max")

F32_CASES = COL_CASES + ROW_CASES + BOTH_MM_CASES + EDGE_CASES + [F32MAX_CASE]

# fp64 inputs (the generic kernels' double instantiation at every size; plans of make_plan_f64)
F64_CASES = [
    _c("d97x101-prime-iso-motion5", (1, 2, 97, 101), M5, True, 3, 1, "f64:prime"),
    _c("d35x7-prime-aniso", (1, 1, 35, 7), None, False, 2, 1, "f64:prime"),
    _c("d64x32-pow2-aniso", (1, 2, 64, 32), None, False, 3, 2, "f64:pow2"),
    _c("d16x16-pow2-iso-gauss3-maxit1", (1, 1, 16, 16), G3, True, 1, 1, "f64:pow2"),
    _c("d4096x5-twg-aniso-gauss3", (1, 1, 4096, 5), G3, False, 2, 1, "f64:col:twg"),
    _c("d3x4096-twg-iso", (1, 1, 3, 4096), None, True, 2, 2, "f64:row:twg"),
    _c("d6000x2-glb-iso", (1, 1, 6000, 2), None, True, 2, 1, "f64:col:glb"),
    _c("d4x6000-glb-aniso-gauss3", (1, 1, 4, 6000), G3, False, 2, 2, "f64:row:glb"),
    _c("d1x9-aniso", (2, 2, 1, 9), None, False, 3, 1, "f64:edge"),
    _c("d9x2-iso", (1, 2, 9, 2), None, True, 3, 2, "f64:edge"),
]

ALL_CASES = F32_CASES + F64_CASES


def is_f64(case: Case) -> bool:
    return case.group.startswith("f64")


def class_of(case: Case):
    """(dimension, class) a case names: ("col" | "row" | "both", class), or (None, None) for the edges."""
    parts = case.group.split(":")
    if parts[0] == "f64":
        parts = parts[1:]
        if len(parts) == 1:
            return (None, None) if parts[0] == "edge" else ("both", parts[0])
    return (parts[0], parts[1]) if len(parts) == 2 else (None, None)


# ------------------------------------------------------------------ one iteration fewer (the negative control)
CONTROL_MIN = 1e-2  # ten times the loosest gate: a backward that drops or repeats a history step cannot pass


def control_errors(case: Case, dtype=torch.float64) -> dict:
    """errors() of the case solved with maxit - 1 iterations (the oracle in `dtype`) against the reference, for
    every figure whose reference is not exactly 0 (lambda's gradient at maxit = 1).  maxit - 1 = 0: the solve
    returns zeros and every gradient is zero."""
    from dataclasses import replace
    ref = tc.reference(case)
    if case.maxit > 1:
        got = tc.oracle_grads(replace(case, maxit=case.maxit - 1), dtype)
    else:
        got = {k: torch.zeros_like(v) for k, v in ref.items() if v is not None}
    e = tc.errors(got, ref)
    return {k: v for k, v in e.items() if torch.as_tensor(ref[k]).abs().max().item() > 0}
