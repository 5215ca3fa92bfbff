"""CPU check of the generic training table (tests/generic_train_cases.py), with the oracle alone.

tests/test_gpu_generic_train.py gates every case at train_cases' fixed bounds with no floor term and no
near-kink exemption.  As for the other two backends (tests/test_train_case_inputs.py) that is legitimate only
if, for every fp32 case: the aniso trajectory stays >= 1e-5 tau away from the soft threshold's kink, 5-95 % of
the difference pixels have an active shrink, and the reference op sequence in fp32 meets half of each gate.

The negative control: the same case solved with one iteration fewer misses the reference in the output and in
every gradient by >= 1e-2, ten times the loosest gate, so a backward that drops or repeats a history step (or
a forward that runs one iteration short) cannot pass the GPU test.  A figure whose reference is exactly 0
(lambda's gradient at maxit = 1) has no relative error and is left out.  The fp64 cases run at gates
(1e-12 / 1e-9) no input choice can endanger; for them the control is the check.

The table test derives every case's plan class from the Python restatement of the library's plan selection
and asserts that the set is complete; the figures are printed (pytest -s)."""
import pytest
import torch

import generic_train_cases as gc
import train_cases as tc


def _control(case):
    e = gc.control_errors(case)
    print(f"{case.name}: one iteration fewer misses by {tc.fmt(e)}")
    assert "out" in e and "gx" in e and "grho" in e and (("gk" in e) == case.learn_psf)
    assert case.maxit == 1 or "glam" in e
    assert all(v >= gc.CONTROL_MIN for v in e.values()), e


@pytest.mark.parametrize("case", gc.F32_CASES, ids=str)
def test_case_is_fit_for_fixed_gates(case):
    from oracle.admm_oracle import kink_margins
    x, k = tc.inputs(case)
    share = tc.active_share(case)
    if case.iso:
        margin = float("inf")
    else:
        margin = kink_margins(x, case.lam, case.rho, k, case.maxit).min().item()
    ref = tc.reference(case)
    floor = tc.errors(tc.oracle_grads(case, torch.float32), ref)
    print(f"{case.name}: kink margin {margin:.2e}, active share {100 * share:.1f} %, fp32 floor {tc.fmt(floor)}")
    assert margin >= tc.KINK_MARGIN
    assert tc.ACTIVE_SHARE[0] <= share <= tc.ACTIVE_SHARE[1]
    assert floor["out"] <= tc.GATE_FWD / 2
    assert all(floor[key] <= case.gate / 2 for key in floor if key != "out"), floor
    _control(case)


@pytest.mark.parametrize("case", gc.F64_CASES, ids=str)
def test_f64_case_misses_with_one_iteration_fewer(case):
    share = tc.active_share(case)
    print(f"{case.name}: active share {100 * share:.1f} %")
    assert tc.ACTIVE_SHARE[0] <= share <= tc.ACTIVE_SHARE[1]  # a shrink that never acts has no lambda gradient
    _control(case)


def test_plan_restatement_on_known_sizes():
    """The restatement against what the library's comments and the inference suite state about known sizes."""
    assert gc.make_plan(481).rad == [37, 13] and gc.make_plan(481).bm == 0     # BSD rows: 37 below ADMM_BLUE_MIN
    assert gc.make_plan(321).rad == [107, 3] and gc.make_plan(321).bm == 256   # BSD columns
    assert gc.make_plan(1920).rad == [16, 8, 3, 5] and gc.gen_wide(1920, gc.make_plan(1920))
    assert gc.make_plan(509).bm == 1024 and gc.make_plan(521).bm == 0
    assert gc.mm_plan(321) == (107, 3) and gc.mm_plan_row(481) == (37, 13) and gc.mm_plan(136) == (17, 8)
    assert gc.mm_plan(301) is None and gc.mm_plan(469) is None  # S = 7 has no instance; 43 and 67 carry no odd R
    # lines in the LDS image up to ~6,800 points, twiddles from global memory up to 10,240 (5,120 in fp64)
    assert not gc.make_plan(6800).twg and gc.make_plan(6840).twg and not gc.make_plan(10240).glb
    assert gc.make_plan(10241).glb and not gc.make_plan(5120, True).glb and gc.make_plan(5121, True).glb


def test_table_reaches_every_class():
    """Every plan class in a column case and in a row case, with a learnable PSF and without one, in fp32 and
    fp64; a case whose size stops reaching the class it names fails here."""
    cases = gc.ALL_CASES
    assert len({c.name for c in cases}) == len(cases)
    seen = {}
    for c in cases:
        f64 = gc.is_f64(c)
        dim, cls = gc.class_of(c)
        B, C, H, W = c.shape
        assert not c.psf or min(H, W) >= c.psf[1], c.name
        assert 1 <= c.maxit <= 3 and c.learn_psf == (c.psf is not None)
        if dim is None:
            continue
        if dim in ("col", "both"):
            assert cls in gc.col_tags(c, f64), (c.name, gc.col_tags(c, f64))
            seen.setdefault((f64, "col", cls), []).append(c)
        if dim in ("row", "both"):
            assert cls in gc.row_tags(c, f64), (c.name, gc.row_tags(c, f64))
            seen.setdefault((f64, "row", cls), []).append(c)
        if dim != "both" and c not in gc.BOTH_MM_CASES:  # the other dimension at 1-9
            assert (W if dim == "col" else H) <= 9, c.name
    print()
    for f64, classes in ((False, gc.CLASSES), (True, gc.CLASSES_F64)):
        for dim in ("col", "row"):
            got = {cls: cs for (f, d, cls), cs in seen.items() if f == f64 and d == dim}
            print(f"{'fp64' if f64 else 'fp32'} {dim}: " + ", ".join(f"{k} ({len(v)})" for k, v in sorted(got.items())))
            assert set(got) == set(classes), (f64, dim)
            if not f64:
                for cls, cs in got.items():
                    assert any(c.learn_psf for c in cs) and any(not c.psf for c in cs), (dim, cls)
        for cls in classes:  # fp64: a PSF and none per class, over both dimensions
            cs = [c for (f, d, k), v in seen.items() if f == f64 and k == cls for c in v]
            assert any(c.learn_psf for c in cs) and any(not c.psf for c in cs), (f64, cls)
    f32 = gc.F32_CASES
    # the matrix-core instances: a column S in {2, 4, 8} beside test_gpu_gcol_mm.py's 1 and 3; row S = 1, 2, 13, S = 1
    # with an odd number of rows in all; one case where both plans hold
    col_S = {gc.mm_plan(c.shape[2])[1] for c in f32 if gc.class_of(c) == ("col", "mm")}
    row_S = {gc.mm_plan_row(c.shape[3])[1] for c in f32 if gc.class_of(c) == ("row", "mm")}
    assert col_S & {2, 4, 8} and row_S >= {1, 2, 13}
    assert any(gc.mm_plan_row(c.shape[3]) == (107, 1) and (c.shape[0] * c.shape[1] * c.shape[2]) % 2 for c in f32)
    assert all(gc.mm_plan(c.shape[2]) and gc.mm_plan_row(c.shape[3]) for c in gc.BOTH_MM_CASES)
    assert any(c.shape[3] % 2 for c in gc.ROW_CASES if gc.class_of(c)[1] in gc.BLUE)  # an odd W among the Bluestein rows
    # both shrink modes over every kind, and maxit = 1 (the LASTK && FIRSTK step alone) once per kind
    for kind in (gc.COL_CASES, gc.ROW_CASES, gc.EDGE_CASES, gc.F64_CASES):
        assert {c.iso for c in kind} == {False, True}
        assert 1 in {c.maxit for c in kind} and {c.maxit for c in kind} & {2, 3}
    assert 1 in {c.maxit for c in gc.COL_CASES if gc.class_of(c)[1] in gc.BLUE}
    assert 1 in {c.maxit for c in f32 if gc.class_of(c)[1] == "mm"}
    # the degenerate wraps
    planes = {c.shape[2:] for c in gc.EDGE_CASES}
    assert planes >= {(1, 7), (7, 1), (2, 2), (2, 9), (9, 2), (3, 3)}
    assert any(c.shape[2:] == (3, 3) and c.psf == tc.G3 for c in gc.EDGE_CASES)
    assert {c.shape[2] for c in gc.F64_CASES} >= {1} and {c.shape[3] for c in gc.F64_CASES} >= {2}
    # the fp32 solve past F32_MAX_PRIME: fp64 kernels, the long line's buffers in global scratch
    from admmtor.eops.deconv import F32_MAX_PRIME, _largest_prime
    c = gc.F32MAX_CASE
    assert _largest_prime(c.shape[3]) > F32_MAX_PRIME and gc.line_tags(c.shape[3], True) >= {"glb", "prime"}
    assert all(max(map(_largest_prime, c.shape[2:])) <= F32_MAX_PRIME for c in f32 if c is not gc.F32MAX_CASE)


def test_every_case_trains_on_the_generic_kernels():
    """The library's own answer (admm_tv_path, training entry points): every case reports "generic"."""
    from admmtor import _native
    from admmtor.eops.deconv import F32_MAX_PRIME, _largest_prime
    for c in gc.ALL_CASES:
        B, C, H, W = c.shape
        f64 = gc.is_f64(c) or max(_largest_prime(H), _largest_prime(W)) > F32_MAX_PRIME
        assert _native.supported(H, W, f64), c.name
        d = _native.desc(B, C, H, W, c.psf[1] if c.psf else 0, c.iso, c.maxit,
                         _native.ADMM_TV_FLAG_PSF_GRAD if c.learn_psf else 0, f64=f64)
        assert _native.path(d, train=True) == "generic", c.name
