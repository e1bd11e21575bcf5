"""Row f4 at its limits, on the MI355X: k_steady (HipBatch.steady_power -> wg_steady_power) against the scalar float64
oracle (oracle/steady_oracle.py) on every case of tests/steady_cases.py — N = 1 .. 128 (both sides of the 64-lane loop),
the full wind rose, exactly and nearly aligned rows, the turbine table's ends and the Ct clamps, yaw +-45 deg, TI 1 % and 30 %,
S = 1 / 4 / 7, non-default model constants, a 36 864-case launch.  tests/test_steady_limits.py holds the torch evaluation to
the same oracle on the same table (float64 bars), so each model has three statements that agree at every limit.

Errors are reported (-s) as worst absolute error [W], worst relative error (turbines above 1 kW) and `u`: the worst error in
units of the bar k_steady has always been held to, |got - ref| <= 30 W + 1e-4 |ref| (tests/test_steady_kernel.py).  MEASURED
holds the `u` observed on the MI355X per case and model; each bar is 5 x that, and never looser than u = 1."""
import time

import numpy as np
import pytest

import steady_cases as sc

pytestmark = pytest.mark.gpu

# worst u per case and model on the MI355X (gfx950, ROCm 7.0).  Nothing comes near today's bar: model 0 stays below 2 W and
# u = 0.015 everywhere; model 1 is the looser one (exp2f / tgammaf / powf per source, summed over up to 127 sources): at most
# 4.7 W and u = 0.13 (N = 128).  Its worst relative errors (1.4e-4, N = 65 and 128) sit on rotors just above cut-in, where
# those 4 W are 1e-4 of the power; no case needed watts of allowance for a table kink.
MEASURED = {
    ("n1", "m0"): 0.0009,                                                # worst abs 0.10 W, worst rel 1.2e-07
    ("n1", "blondel_jimenez"): 0.0009,                                   # worst abs 0.10 W, worst rel 1.2e-07
    ("n2_0p5D", "m0"): 0.0019,                                           # worst abs 0.13 W, worst rel 3.7e-07
    ("n2_0p5D", "blondel_jimenez"): 0.0024,                              # worst abs 0.12 W, worst rel 6.2e-07
    ("n2_3D", "m0"): 0.0020,                                             # worst abs 0.14 W, worst rel 4.4e-07
    ("n2_3D", "blondel_jimenez"): 0.0020,                                # worst abs 0.13 W, worst rel 9.3e-07
    ("n2_40D", "m0"): 0.0014,                                            # worst abs 0.13 W, worst rel 2.0e-07
    ("n2_40D", "blondel_jimenez"): 0.0017,                               # worst abs 0.17 W, worst rel 2.5e-07
    ("n64", "m0"): 0.0076,                                               # worst abs 0.70 W, worst rel 1.6e-06
    ("n64", "blondel_jimenez"): 0.0507,                                  # worst abs 1.86 W, worst rel 2.8e-05
    ("n65", "m0"): 0.0134,                                               # worst abs 1.11 W, worst rel 2.1e-06
    ("n65", "blondel_jimenez"): 0.0881,                                  # worst abs 4.11 W, worst rel 1.4e-04
    ("horns_rev80", "m0"): 0.0126,                                       # worst abs 1.79 W, worst rel 1.6e-06
    ("horns_rev80", "blondel_jimenez"): 0.0592,                          # worst abs 4.73 W, worst rel 3.1e-05
    ("n128", "m0"): 0.0147,                                              # worst abs 0.97 W, worst rel 6.1e-06
    ("n128", "blondel_jimenez"): 0.1327,                                 # worst abs 4.71 W, worst rel 1.3e-04
    ("rose_4x4", "m0"): 0.0026,                                          # worst abs 0.19 W, worst rel 5.3e-07
    ("rose_4x4", "blondel_jimenez"): 0.0165,                             # worst abs 0.60 W, worst rel 4.8e-05
    ("aligned_8x1", "m0"): 0.0010,                                       # worst abs 0.07 W, worst rel 2.7e-07
    ("aligned_8x1", "blondel_jimenez"): 0.0045,                          # worst abs 0.15 W, worst rel 5.6e-06
    ("nearly_aligned_8x1", "m0"): 0.0020,                                # worst abs 0.10 W, worst rel 4.8e-07
    ("nearly_aligned_8x1", "blondel_jimenez"): 0.0366,                   # worst abs 1.40 W, worst rel 1.7e-05
    ("aligned_4x4", "m0"): 0.0020,                                       # worst abs 0.10 W, worst rel 4.7e-07
    ("aligned_4x4", "blondel_jimenez"): 0.0073,                          # worst abs 0.25 W, worst rel 5.8e-06
    ("nearly_aligned_4x4", "m0"): 0.0023,                                # worst abs 0.11 W, worst rel 6.1e-07
    ("nearly_aligned_4x4", "blondel_jimenez"): 0.0177,                   # worst abs 0.61 W, worst rel 1.4e-05
    ("table_ends", "m0"): 0.0022,                                        # worst abs 0.43 W, worst rel 1.6e-05
    ("table_ends", "blondel_jimenez"): 0.0031,                           # worst abs 0.17 W, worst rel 1.9e-06
    ("ct_clamp", "m0"): 0.0025,                                          # worst abs 0.23 W, worst rel 5.5e-07
    ("ct_clamp", "blondel_jimenez"): 0.0314,                             # worst abs 2.71 W, worst rel 8.0e-06
    ("yaw45_8x1", "m0"): 0.0015,                                         # worst abs 0.10 W, worst rel 4.1e-07
    ("yaw45_8x1", "blondel_jimenez"): 0.0037,                            # worst abs 0.17 W, worst rel 1.9e-06
    ("yaw45_4x4", "m0"): 0.0013,                                         # worst abs 0.08 W, worst rel 4.3e-07
    ("yaw45_4x4", "blondel_jimenez"): 0.0050,                            # worst abs 0.24 W, worst rel 1.7e-06
    ("ti_ends", "m0"): 0.0037,                                           # worst abs 0.22 W, worst rel 9.0e-07
    ("ti_ends", "blondel_jimenez"): 0.0138,                              # worst abs 0.76 W, worst rel 6.7e-06
    ("S1", "m0"): 0.0033,                                                # worst abs 0.36 W, worst rel 4.6e-07
    ("S4", "m0"): 0.0023,                                                # worst abs 0.42 W, worst rel 3.8e-07
    ("S7", "m0"): 0.0048,                                                # worst abs 0.37 W, worst rel 7.9e-07
    ("constants", "m0"): 0.0025,                                         # worst abs 0.42 W, worst rel 3.1e-07
    ("sweep_36864", "m0"): 0.0049,                                       # worst abs 0.71 W, worst rel 1.0e-06
    ("sweep_36864", "blondel_jimenez"): 0.0720,                          # worst abs 4.26 W, worst rel 1.5e-05
}


def bar(name, model):
    return min(1.0, 5.0 * MEASURED[(name, model)])


def _batch(case):
    from windgym_amd import steady
    return steady.hip_batch_for(case.x, case.y, turbine=case.turbine, n_rotor_pts=case.S, model_constants=case.constants)


def _report(tag, model, got, ref):
    a, r, u = sc.errors(got, ref)
    print(f"[k_steady {tag} {model}] worst abs {a:.3e} W, worst rel {r:.3e}, u {u:.4f}")
    return u


ALL = [(n, m) for n, c in sc.cases().items() for m in c.models]


@pytest.mark.parametrize("name,model", ALL, ids=[f"{n}-{m}" for n, m in ALL])
def test_kernel_matches_the_oracle_at_the_limits(name, model):
    case = sc.cases()[name]
    b = _batch(case)
    got = b.steady_power(case.ws, case.wd, case.ti, case.yaw, model=model).cpu().numpy()
    b.close()
    assert got.shape == case.yaw.shape and got.dtype == np.float32
    assert np.isfinite(got).all() and (got >= 0).all()
    u = _report(name, model, got, sc.oracle_power(case, model))
    assert u <= bar(name, model), (u, bar(name, model))


@pytest.mark.parametrize("model", sc.MODELS)
def test_wind_from_0_and_from_360_degrees_is_the_same_wind(model):
    case = sc.cases()["rose_4x4"]
    assert case.wd[0] == 0.0 and case.wd[9] == 360.0 and np.array_equal(case.yaw[0], case.yaw[9])
    b = _batch(case)
    got = b.steady_power(case.ws, case.wd, case.ti, case.yaw, model=model).cpu().numpy()
    b.close()
    assert np.array_equal(got[0], got[9])                          # bit for bit
    assert not np.array_equal(got[0], got[4])                      # (and the rose is not one answer eight times)


def test_constants_reach_the_kernel():
    """the handle's model constants are copied into SteadyP: the same cases on a default handle differ by far more than any
    bar, and the oracle with default constants no longer matches the kernel"""
    case = sc.cases()["constants"]
    b = _batch(case)
    got = b.steady_power(case.ws, case.wd, case.ti, case.yaw).cpu().numpy()
    b.close()
    d = _batch(case._replace(constants=None))
    plain = d.steady_power(case.ws, case.wd, case.ti, case.yaw).cpu().numpy()
    d.close()
    assert sc.errors(got, plain)[2] > 100.0
    assert sc.errors(got, sc.oracle_power(case._replace(constants=None), "m0"))[2] > 100.0
    for k, v in case.constants.items():                            # every single constant is seen by the comparison
        one = sc.oracle_power(case._replace(constants={**case.constants, k: v * 1.1}), "m0")
        assert sc.errors(got, one)[2] > 5.0 * bar("constants", "m0"), k


@pytest.mark.parametrize("model", sc.MODELS)
def test_one_launch_of_a_sweep(model):
    """36 864 cases in one launch (4096 conditions x 9 candidates, what one refine step of a sweep launches): 64 sampled
    cases against the oracle; the same cases launched alone and the whole launch repeated are BIT-EQUAL to it (one workgroup
    per case, no state shared between cases or launches)"""
    case = sc.sweep_case()
    b = _batch(case)
    big = b.steady_power(case.ws, case.wd, case.ti, case.yaw, model=model).cpu().numpy()
    assert big.shape == (36864, 16) and np.isfinite(big).all() and (big >= 0).all()
    rows = np.random.default_rng(5).choice(len(case.ws), 64, replace=False)
    rows[:2] = [0, len(case.ws) - 1]                               # the first and the last workgroup of the grid
    u = _report("sweep_36864", model, big[rows], sc.oracle_power(case, model, rows))
    assert u <= bar("sweep_36864", model), (u, bar("sweep_36864", model))
    alone = b.steady_power(case.ws[rows], case.wd[rows], case.ti[rows], case.yaw[rows], model=model).cpu().numpy()
    assert np.array_equal(alone, big[rows])
    for r in rows[:4]:                                             # a launch of one case
        one = b.steady_power(case.ws[r], case.wd[r], case.ti[r], case.yaw[r][None], model=model).cpu().numpy()
        assert np.array_equal(one[0], big[r])
    again = b.steady_power(case.ws, case.wd, case.ti, case.yaw, model=model).cpu().numpy()
    b.close()
    assert np.array_equal(again, big)


@pytest.mark.parametrize("name", ["horns_rev80", "n128", "yaw45_8x1"])
@pytest.mark.parametrize("model", sc.MODELS)
def test_the_same_launch_twice_is_bit_equal(name, model):
    case = sc.cases()[name]
    b = _batch(case)
    a1 = b.steady_power(case.ws, case.wd, case.ti, case.yaw, model=model).cpu().numpy()
    a2 = b.steady_power(case.ws, case.wd, case.ti, case.yaw, model=model).cpu().numpy()
    b.close()
    assert np.array_equal(a1, a2)


@pytest.mark.parametrize("model", sc.MODELS)
def test_reference_side_perturbations_break_every_bar(model):
    """negative controls: the kernel stays as it is, the REFERENCE is made slightly wrong (one quadrature point fewer, the
    yaws of two turbines swapped, the deflection constant 2 % off, the layout turned by 0.05 deg) — each must fail the
    comparison.  The three physical ones break even today's widest bar (u = 1) several times over; one quadrature point is
    a 4 % change of a small quadrature error and is held to the case's own bar."""
    missed = []
    for name, rows in sc.NEGATIVE_CONTROL_ROWS.items():
        case = sc.cases()[name]
        b = _batch(case)
        got = b.steady_power(case.ws[rows], case.wd[rows], case.ti[rows], case.yaw[rows], model=model).cpu().numpy()
        b.close()
        ok = sc.errors(got, sc.oracle_power(case, model, rows))[2]
        assert ok <= bar(name, model)
        swapped = case.yaw.copy()
        swapped[:, [0, 1]] = swapped[:, [1, 0]]
        wrong = {"n_quad - 1": dict(n_quad=47 if model == "m0" else 19), "two yaws swapped": dict(yaw=swapped),
                 "deflection constant + 2 %": dict(hill=0.4 * 1.02) if model == "m0" else dict(jimenez_beta=0.1 * 1.02),
                 "layout turned by 0.05 deg": dict(zip("xy", sc.rotated(case.x, case.y, 0.05)))}
        for what, kw in wrong.items():
            u = sc.errors(got, sc.oracle_power(case, model, rows, **kw))[2]
            print(f"[k_steady control {name} {model}] {what}: u {u:.3f} (unperturbed {ok:.4f}, bar {bar(name, model):.4f})")
            if not (u > bar(name, model) and (what == "n_quad - 1" or u > 5.0)):
                missed.append((name, what, u))
    assert not missed, missed


def test_yaws_optimised_on_the_kernel_are_as_good_as_the_torch_path_on_horns_rev():
    """yaw_optimizer_srf on Horns Rev (N = 80) with every refine step evaluated by k_steady, and on the torch path: the farm
    power of the kernel's optimum, evaluated by the oracle, is within 2e-3 of the torch path's (the form of
    test_serial_refine_on_the_kernel_reference_inequality, which does it for N = 2).  2 conditions x 2 passes x 5 candidates:
    measured 0.3 s for the kernel path and 6.5 s for the torch path's 160 refine steps on the GPU machine's host (45 s on
    an 8-core desktop CPU); both paths chose the same yaws there."""
    from windgym_amd import steady
    from windgym_amd.presets import horns_rev1_layout
    x, y = horns_rev1_layout()
    case = sc._case(x, y, [8.0, 10.0], [270.0, 221.0], [0.06, 0.08], np.zeros((2, 80)))
    t0 = time.perf_counter()
    b = _batch(case)
    y_hip = steady.yaw_optimizer_srf(x, y, case.ws, case.wd, case.ti, refine_pass_n=2, yaw_n=5, batch=b)
    b.close()
    t1 = time.perf_counter()
    y_cpu = steady.yaw_optimizer_srf(x, y, case.ws, case.wd, case.ti, refine_pass_n=2, yaw_n=5)
    t2 = time.perf_counter()
    assert y_hip.shape == y_cpu.shape == (2, 80) and np.abs(y_hip).max() <= 30.0
    p = lambda yaw: sc.oracle_power(case, "m0", yaw=yaw).sum(-1)      # noqa: E731
    p_hip, p_cpu, p_zero = p(y_hip), p(y_cpu), p(np.zeros((2, 80)))
    print(f"[k_steady optimiser, Horns Rev] kernel path {t1 - t0:.1f} s, torch path {t2 - t1:.1f} s; farm power / unyawed: "
          f"kernel {p_hip / p_zero}, torch {p_cpu / p_zero}; largest yaw difference {np.abs(y_hip - y_cpu).max():.2f} deg")
    assert (p_hip >= p_cpu * (1 - 2e-3)).all() and (p_cpu >= p_hip * (1 - 2e-3)).all()
    assert (p_hip >= p_zero).all()                                 # (7 D pitch: two coarse passes gain a fraction of a percent)
