"""Row f4 at its limits, on the CPU: the torch evaluation of windgym_amd/steady.py (float64) against the scalar oracle
(oracle/steady_oracle.py) on the case table of tests/steady_cases.py — the table k_steady is held to on the MI355X
(tests/test_gpu_steady_limits.py).  Three independent statements of each model (HIP kernel, batched torch, scalar numpy)
must agree at every limit; this file runs two of them on every machine."""
import numpy as np
import pytest

import steady_cases as sc

# the float64 bars of test_torch_evaluation_matches_the_oracle_restatement
RTOL, ATOL = 1e-9, 1e-3
TORCH_CASES = [(n, m) for n, c in sc.cases().items() if c.constants is None for m in c.models]


@pytest.mark.parametrize("name,model", TORCH_CASES, ids=[f"{n}-{m}" for n, m in TORCH_CASES])
def test_torch_evaluation_matches_the_oracle_at_the_limits(name, model):
    case = sc.cases()[name]
    got, ref = sc.torch_power(case, model), sc.oracle_power(case, model)
    assert got.shape == ref.shape == case.yaw.shape and np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)


def test_the_table_reaches_what_it_claims():
    """the cases exist for a reason each: assert that reason on the oracle's side, so that a retuned turbine table or layout
    cannot quietly turn a limit into an ordinary case"""
    c = sc.cases()
    tab = sc.table_of(c["n1"])
    # N = 1: the table at ws cos(yaw), nothing else
    n1 = c["n1"]
    ref = np.array([tab.power(w * np.cos(np.radians(g))) for w, g in zip(n1.ws, n1.yaw[:, 0])])
    np.testing.assert_allclose(sc.oracle_power(n1, "m0")[:, 0], ref, rtol=1e-12)
    np.testing.assert_allclose(sc.oracle_power(n1, "blondel_jimenez")[:, 0], ref, rtol=1e-12)
    assert ref[3] == 0.0 and ref[4] == tab.power_tab[-1] and ref[5] == 0.0            # on cut-in, on cut-out, above it
    # table ends: nothing below cut-in or above cut-out, full power on the last node, and at least one case in which the
    # first rotor runs and a waked one has dropped below cut-in
    te = c["table_ends"]
    p = sc.oracle_power(te, "m0")
    below, above = te.ws < tab.ws_tab[0], te.ws > tab.ws_tab[-1]
    assert below.sum() >= 2 and above.sum() >= 2 and (p[below | above] == 0).all()
    assert (p[te.ws == tab.ws_tab[-1], 0] == tab.power_tab[-1]).all()
    assert ((p[:, 0] > 0) & (p[:, 1:] == 0).any(axis=1)).any()
    # both clamps are exceeded by the high-thrust table at the speeds of its case
    ht = sc.table_of(c["ct_clamp"])
    assert (ht.ct(c["ct_clamp"].ws) > 0.999).sum() >= 3
    # the 5-sigma cut-off is crossed inside the wd sweep of the two-turbine cases (m0): waked in the middle, free at the ends
    # (at 0.5 D the wake is wider than the pair is long: waked at every direction of the sweep)
    for tag in ("0p5D", "3D", "40D"):
        p = sc.oracle_power(c["n2_" + tag], "m0", rows=range(25))
        free = tab.power(8.0)
        assert p[12, 1] < 0.95 * free and (tag == "0p5D" or (p[0, 1] == free and p[24, 1] == free))
    # sizes
    assert [len(c[k].x) for k in ("n64", "n65", "horns_rev80", "n128")] == [64, 65, 80, 128]


@pytest.mark.parametrize("model", sc.MODELS)
def test_sampled_sweep_cases_on_the_cpu(model):
    """the 64 sampled rows of the 36 864-case launch (tests/test_gpu_steady_limits.py), torch against the oracle"""
    case = sc.sweep_case()
    assert case.yaw.shape == (36864, 16)
    rows = np.random.default_rng(5).choice(len(case.ws), 64, replace=False)
    np.testing.assert_allclose(sc.torch_power(case, model, rows), sc.oracle_power(case, model, rows), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("model", sc.MODELS)
def test_reference_side_perturbations_break_the_float64_bars(model):
    """the negative controls of the GPU file, against the torch evaluation: every perturbation of the reference side is
    seen (the comparison is able to fail)"""
    for name, rows in sc.NEGATIVE_CONTROL_ROWS.items():
        case = sc.cases()[name]
        got = sc.torch_power(case, model, rows)
        np.testing.assert_allclose(got, sc.oracle_power(case, model, rows), rtol=RTOL, atol=ATOL)
        swapped = case.yaw.copy()
        swapped[:, [0, 1]] = swapped[:, [1, 0]]
        for kw in (dict(n_quad=47 if model == "m0" else 19), dict(yaw=swapped),
                   dict(hill=0.4 * 1.02) if model == "m0" else dict(jimenez_beta=0.1 * 1.02),
                   dict(zip("xy", sc.rotated(case.x, case.y, 0.05)))):
            with pytest.raises(AssertionError):
                np.testing.assert_allclose(got, sc.oracle_power(case, model, rows, **kw), rtol=RTOL, atol=ATOL)
