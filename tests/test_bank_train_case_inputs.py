"""CPU check of tests/bank_train_cases.py, with the restatement alone.

tests/test_gpu_psf_bank_train.py gates every case at fixed bounds -- output <= 1e-5, every gradient, each
table's PSF gradient included, <= 1e-3 -- with no floor term and no near-kink exemption.  As for the tables of
test_train_case_inputs.py that is legitimate only if, for every case, none left out:

  * the fp64 trajectory stays >= 1e-5 tau away from the kink of its shrink;
  * between 5 % and 95 % of the difference pixels have an active shrink (bank_train_cases.KINK_FREE names the
    cases where no such input exists, with the reason);
  * the negative controls of the PSF gradient miss the right gradient by 1e-2 or more (asserted inside
    bank_train_cases.reference, checked again here);
  * the restatement in fp32 meets half of every gate against itself in fp64, the PSF gradient also per table.

And the restatement is pinned: to bank_cases.restate in value, to solve_spatial's autograd for a (1, 1, k, k)
bank, and to the per-image solve_spatial calls for an aniso per-image bank.  The figures are printed (pytest -s)."""
import pytest
import torch

import bank_cases as bc
import bank_train_cases as btc
import train_cases as tc


@pytest.mark.parametrize("name,mode,iso,maxit", btc.PARAMS)
def test_case_is_fit_for_fixed_gates(name, mode, iso, maxit):
    r = btc.reference(name, mode, iso, maxit)  # asserts the controls
    margin, share = btc.fitness(name, mode, iso, maxit)
    floor = btc.errors(btc.grads(r["x"], r["kerns"], iso, maxit, r["cot"], torch.float32, lam=r["lam"]), r["ref"])
    worst = min(r["controls"], key=r["controls"].get)
    free = (name, mode, iso, maxit) in btc.KINK_FREE
    print(f"{name} {mode} iso={iso} maxit={maxit}: kink margin {margin:.2e}, active share {100 * share:.1f} %"
          f"{' (kink-free)' if free else ''}, fp32 floor {tc.fmt(floor)}, weakest control {worst} "
          f"{r['controls'][worst]:.2e}")
    assert margin >= tc.KINK_MARGIN
    if not free:
        assert tc.ACTIVE_SHARE[0] <= share <= tc.ACTIVE_SHARE[1]
    assert r["controls"][worst] >= btc.CONTROL_MIN
    # half of each gate: the kernels' fp32 sums run in another order and need room of their own
    assert floor["out"] <= tc.GATE_FWD / 2
    assert all(floor[key] <= tc.GATE_GRAD_PSF / 2 for key in floor if key != "out"), floor


def test_table_reaches_the_instances():
    """Every path, 1-3 iterations, a per-image bank of C = 3, and a per-channel bank whose tables own one plane
    more than a cross-spectrum chunk."""
    assert {c[2] for c in btc.CASES.values()} == {"fused", "fused mixed-radix", "generic"}
    assert btc.MAXITS == (1, 2, 3) and btc.MODES == ("image", "channel", "plane")
    assert any(s[1] == 3 for s, *_ in btc.CASES.values())
    assert any(s[0] == btc.XPPG + 1 and s[1] > 1 for s, *_ in btc.CASES.values())
    assert not btc.KINK_FREE or all(isinstance(v, str) and v for v in btc.KINK_FREE.values())


@pytest.mark.parametrize("name", ["pow2_16x32", "gen_15x17"])
@pytest.mark.parametrize("mode", btc.MODES)
@pytest.mark.parametrize("iso", btc.ISOS)
def test_values_equal_the_inference_restatement(name, mode, iso):
    xd, kd = btc.case_input(name, iso).double(), btc.case_bank(name, mode).double()
    got = btc.solve_bank(xd, btc.LAM, btc.RHO, kd, iso, 3)
    assert tc.rel(got, bc.restate(xd, btc.LAM, btc.RHO, kd, iso, 3)[0]) <= 1e-12


@pytest.mark.parametrize("iso", btc.ISOS)
def test_shared_bank_equals_solve_spatial(iso):
    """A (1, 1, k, k) bank: values and gradients are solve_spatial's autograd."""
    from oracle.admm_oracle import solve_spatial
    name = "pow2_16x32"
    x, cot = btc.case_input(name, iso), btc.cotangent(name)
    kern = bc.make_bank("shared", 2, 3, 5)
    got = btc.grads(x, kern, iso, 3, cot)
    xd = x.double().requires_grad_(True)
    kd = kern.double().requires_grad_(True)
    lt = torch.tensor([btc.LAM], dtype=torch.float64, requires_grad=True)
    rt = torch.tensor([btc.RHO], dtype=torch.float64, requires_grad=True)
    out = solve_spatial(xd, lt, rt, kd, iso, 3)
    g = torch.autograd.grad(out, (xd, lt, rt, kd), cot.double())
    for a, b in zip((got["out"], got["gx"], got["glam"], got["grho"], got["gk"]), (out.detach(), *g)):
        assert tc.rel(a, b) <= 1e-10


def test_per_image_bank_equals_the_loop():
    """Aniso, per-image: gx and gk[b] per image, glam / grho summed over the single-image solve_spatial calls."""
    from oracle.admm_oracle import solve_spatial
    name = "pow2_16x32"
    x, cot, kerns = btc.case_input(name, False), btc.cotangent(name), btc.case_bank(name, "image")
    got = btc.grads(x, kerns, False, 3, cot)
    gl = gr = 0.0
    for b in range(x.shape[0]):
        xd = x[b:b + 1].double().requires_grad_(True)
        kd = kerns[b:b + 1].double().requires_grad_(True)
        lt = torch.tensor([btc.LAM], dtype=torch.float64, requires_grad=True)
        rt = torch.tensor([btc.RHO], dtype=torch.float64, requires_grad=True)
        out = solve_spatial(xd, lt, rt, kd, False, 3)
        g = torch.autograd.grad(out, (xd, lt, rt, kd), cot[b:b + 1].double())
        assert tc.rel(got["out"][b:b + 1], out.detach()) <= 1e-10
        assert tc.rel(got["gx"][b:b + 1], g[0]) <= 1e-10
        assert tc.rel(got["gk"][b:b + 1], g[3]) <= 1e-10
        gl, gr = gl + g[1], gr + g[2]
    assert tc.rel(got["glam"], gl) <= 1e-10 and tc.rel(got["grho"], gr) <= 1e-10
