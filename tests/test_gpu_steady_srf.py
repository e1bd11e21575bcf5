"""k_steady_srf (wg_steady_optimize, HipBatch.steady_optimize): the whole Serial-Refine optimisation of every wind condition in
ONE launch, on the MI355X.  The contract is bit equality — yaws and farm power — with the host twin
(tests/steady_srf_twin.py) that follows the rules in include/windgym_hip.h, visits the turbines in the order the kernel
reports and gets every power from wg_steady_power (k_steady); tests/test_steady_srf.py pins that twin against the product's
own loop on the CPU.  Then: the loop `yaw_optimizer_srf(batch=b)` itself, the reference's inequality, the refusals, and the
batched agent on a vector env across autoresets and inside eval_sweep."""
import ctypes as C

import numpy as np
import pytest

import steady_cases as sc
import steady_srf_twin as tw

pytestmark = pytest.mark.gpu


def _layout_4x3():
    x, y = np.meshgrid(np.linspace(0, 1280, 4), np.linspace(0, 853.3, 3))
    return x.ravel(), y.ravel()


def _random_conditions(C_, seed=3):
    rng = np.random.default_rng(seed)                      # (the conditions of test_steady_kernel.py)
    return rng.uniform(6.0, 14.0, C_), rng.uniform(240.0, 300.0, C_), rng.uniform(0.03, 0.12, C_)


def _kernel_inputs(ws, wd, ti):
    """the float32 numbers steady_optimize hands the kernel (1e-3 deg added to wd in double, as the host loop does)"""
    ws, wd, ti = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (ws, wd, ti))
    return ws.astype(np.float32), (wd + 1e-3).astype(np.float32), ti.astype(np.float32)


def _power_fn(b, model, ws32, wd32, ti32):
    """wg_steady_power for [C, K, N] candidate yaws: ONE launch"""
    def power(yaw):
        C_, K, N = yaw.shape
        rep = lambda a: np.repeat(a, K)      # noqa: E731
        return b.steady_power(rep(ws32), rep(wd32), rep(ti32), yaw.reshape(-1, N).astype(np.float32),
                              model=model).cpu().numpy().reshape(C_, K, N)
    return power


def _check_against_twin(b, x, y, ws, wd, ti, model, passes, yaw_n, yaw_max=30.0, tag=""):
    from windgym_amd import steady
    yaw, power, order = (a.cpu().numpy() for a in b.steady_optimize(ws, wd, ti, model=model, refine_pass_n=passes, yaw_n=yaw_n,
                                                                    yaw_max=yaw_max, return_order=True))
    C_, N = len(np.atleast_1d(ws)), len(x)
    assert yaw.shape == (C_, N) and yaw.dtype == np.float64 and power.shape == (C_,) and power.dtype == np.float64
    assert order.shape == (C_, N) and order.dtype == np.int32
    ws32, wd32, ti32 = _kernel_inputs(ws, wd, ti)
    tw.check_order(order, x, y, wd32.astype(np.float64))
    fn = _power_fn(b, model, ws32, wd32, ti32)
    t_yaw, t_best = tw.srf_twin(fn, order, steady.srf_offsets(passes, yaw_n, yaw_max).numpy(), yaw_max)
    moved = int((np.abs(yaw) > 0).sum())
    print(f"[k_steady_srf {tag} {model} {passes}x{yaw_n}] {C_} conditions x {N} turbines: {moved} yaws moved, "
          f"largest |yaw - twin| {np.abs(yaw - t_yaw).max():.3e} deg, largest |P - twin| {np.abs(power - t_best).max():.3e} W")
    assert np.array_equal(yaw, t_yaw)
    assert np.array_equal(power, t_best)
    # power_dev is the farm power AT yaw_dev wherever the final clamp did not act
    free = np.abs(t_yaw).max(axis=1) < yaw_max
    at = tw.index_order_sum(fn(yaw.astype(np.float32).astype(np.float64)[:, None, :]))[:, 0]
    assert np.array_equal(power[free], at[free])
    return yaw, power, free


@pytest.fixture(scope="module")
def small():
    from windgym_amd import steady
    x, y = _layout_4x3()
    b = steady.hip_batch_for(x, y)
    yield b, x, y
    b.close()


@pytest.mark.parametrize("model", sc.MODELS)
def test_bit_equal_to_the_twin_37_random_conditions(small, model):
    b, x, y = small
    ws, wd, ti = _random_conditions(37)
    yaw, _, free = _check_against_twin(b, x, y, ws, wd, ti, model, 8, 9, tag="4x3")
    assert (np.abs(yaw).max(axis=1) > 1.0).sum() > 10 and free.sum() > 10      # (it optimised, and the power check had rows)


@pytest.mark.parametrize("model", sc.MODELS)
@pytest.mark.parametrize("name", ["n1", "n2_3D", "aligned_4x4", "nearly_aligned_4x4"])
def test_bit_equal_to_the_twin_small_cases(name, model):
    case = sc.cases()[name]
    from windgym_amd import steady
    b = steady.hip_batch_for(case.x, case.y)
    try:
        _check_against_twin(b, case.x, case.y, case.ws, case.wd, case.ti, model, 8, 9, tag=name)
    finally:
        b.close()


@pytest.mark.parametrize("model", sc.MODELS)
@pytest.mark.parametrize("name", ["n64", "n65", "horns_rev80", "n128"])
def test_bit_equal_to_the_twin_large_farms(name, model):
    """both sides of the 64-lane source loop and the build's limit; 2 passes x 5 candidates keep the twin's launch count down"""
    case = sc.cases()[name]
    from windgym_amd import steady
    b = steady.hip_batch_for(case.x, case.y)
    try:
        yaw, _, _ = _check_against_twin(b, case.x, case.y, case.ws, case.wd, case.ti, model, 2, 5, tag=name)
    finally:
        b.close()
    assert np.abs(yaw).max() > 0.0


@pytest.mark.parametrize("model", sc.MODELS)
@pytest.mark.parametrize("passes", [1, 16])
@pytest.mark.parametrize("yaw_n", [2, 9, 16])
def test_bit_equal_to_the_twin_at_the_limits_of_passes_and_candidates(small, model, passes, yaw_n):
    b, x, y = small
    ws, wd, ti = _random_conditions(5, seed=11)
    _check_against_twin(b, x, y, ws, wd, ti, model, passes, yaw_n, tag="limits")


@pytest.mark.parametrize("model", sc.MODELS)
def test_bit_equal_to_the_twin_with_offsets_float32_cannot_hold(small, model):
    b, x, y = small
    ws, wd, ti = _random_conditions(6, seed=12)
    from windgym_amd import steady
    offs = steady.srf_offsets(8, 9, 25.3).numpy()
    assert (offs.astype(np.float32).astype(np.float64) != offs).any()
    _check_against_twin(b, x, y, ws, wd, ti, model, 8, 9, yaw_max=25.3, tag="yaw_max 25.3")


@pytest.mark.parametrize("model", sc.MODELS)
def test_power_is_the_farm_power_at_the_returned_yaws(small, model):
    """one pass cannot leave +-yaw_max, so the clamp is idle and every row is checked (Horns Rev too)"""
    from windgym_amd import steady
    from windgym_amd.presets import horns_rev1_layout
    b, x, y = small
    ws, wd, ti = _random_conditions(37)
    xh, yh = horns_rev1_layout()
    h = steady.hip_batch_for(xh, yh)
    try:
        for bb, cond, n in ((b, (ws, wd, ti), 12), (h, ([8.0, 10.0], [270.0, 221.0], [0.06, 0.08]), 80)):
            yaw, power = (a.cpu().numpy() for a in bb.steady_optimize(*cond, model=model, refine_pass_n=1, yaw_n=9))
            assert np.abs(yaw).max() <= 30.0 and yaw.shape[1] == n
            p = bb.steady_power(*_kernel_inputs(*cond), yaw.astype(np.float32), model=model).cpu().numpy()
            assert np.array_equal(power, tw.index_order_sum(p))
    finally:
        h.close()


@pytest.mark.parametrize("model", sc.MODELS)
def test_a_condition_does_not_depend_on_its_batch_and_launches_repeat(small, model):
    b, x, y = small
    ws, wd, ti = _random_conditions(300, seed=5)
    kw = dict(model=model, refine_pass_n=2, yaw_n=5, return_order=True)
    big = [a.cpu().numpy() for a in b.steady_optimize(ws, wd, ti, **kw)]
    again = [a.cpu().numpy() for a in b.steady_optimize(ws, wd, ti, **kw)]
    for a1, a2 in zip(big, again):
        assert np.array_equal(a1, a2)
    for r in (0, 137, 299):
        one = [a.cpu().numpy() for a in b.steady_optimize(ws[r], wd[r], ti[r], **kw)]
        for a1, a2 in zip(big, one):
            assert a2.shape[0] == 1 and np.array_equal(a1[r], a2[0])
    assert not np.array_equal(big[0][0], big[0][137])


@pytest.mark.parametrize("model", sc.MODELS)
def test_as_good_as_the_host_loop(small, model):
    """today's loop (one launch of k_steady per refine step) takes its visiting order from a float64 argsort, the kernel from
    float32 ranks: on an exact tie the two may walk differently, so equal yaws are printed and the farm powers are asserted,
    each within 1e-6 of the other (the form of test_batched_optimizer_many_conditions_one_launch_per_refine_step)"""
    from windgym_amd import steady
    b, x, y = small
    ws = np.array([7.0, 9.0, 9.0, 11.0]); wd = np.array([270.0, 270.0, 250.0, 285.0]); ti = np.array([0.04, 0.04, 0.08, 0.06])
    for passes, yaw_n in ((4, 5), (8, 9)):
        loop = steady.yaw_optimizer_srf(x, y, ws, wd, ti, refine_pass_n=passes, yaw_n=yaw_n, model=model, batch=b)
        fused = steady.yaw_optimizer_srf(x, y, ws, wd, ti, refine_pass_n=passes, yaw_n=yaw_n, model=model, batch=b, fused=True)
        assert fused.shape == loop.shape == (4, 12) and fused.dtype == np.float64 and np.abs(fused).max() <= 30.0
        P = lambda yaw: b.steady_power(ws, wd + 1e-3, ti, yaw, model=model).double().sum(-1).cpu().numpy()      # noqa: E731
        p_f, p_l, p_0 = P(fused), P(loop), P(np.zeros((4, 12)))
        print(f"[k_steady_srf vs loop {model} {passes}x{yaw_n}] equal yaws: {np.array_equal(fused, loop)}, largest difference "
              f"{np.abs(fused - loop).max():.3e} deg, farm power fused / loop - 1: {p_f / p_l - 1}")
        assert (p_f >= p_l * (1 - 1e-6)).all() and (p_l >= p_f * (1 - 1e-6)).all()
        # row 0 looks straight down the rows of the layout: yawing must pay.  1 % is what the suite asks of the loop for m0
        # (test_steady_kernel.py:103); the Blondel model's wakes recover faster, there the gain only has to be a gain
        assert (p_f >= p_0 * (1 - 1e-6)).all() and p_f[0] > p_0[0] * (1.01 if model == "m0" else 1.0)


@pytest.mark.parametrize("cls", ["SteadyStateYawAgent", "PyWakeAgent"])
def test_reference_inequality_through_the_fused_path(cls):
    """tests/test_pywake_agent.py:11-45 of the reference, the optimisation being one launch"""
    from windgym_amd import steady
    A = getattr(steady, cls)
    agent = A(x_pos=[0, 500], y_pos=[0, 0], wind_speed=6, wind_dir=270, TI=0.02, device="cuda", fused=True)
    nominal = agent.power([30, 0])
    agent.optimize()
    assert agent.power(agent.optimized_yaws) >= nominal
    assert agent.power(agent.optimized_yaws) > agent.power([0, 0])
    loop = A(x_pos=[0, 500], y_pos=[0, 0], wind_speed=6, wind_dir=270, TI=0.02, device="cuda")
    loop.optimize()
    print(f"[k_steady_srf {cls}] fused {agent.optimized_yaws}, loop {loop.optimized_yaws}")
    assert loop.power(agent.optimized_yaws) >= loop.power(loop.optimized_yaws) * (1 - 1e-6)
    a, _ = agent.predict(None)
    assert a.shape == (2,) and a.dtype == np.float32 and np.all(np.abs(a) <= 1)
    agent.close(); loop.close()


def test_refusals(small):
    import torch
    from windgym_amd import binding, steady
    b, x, y = small
    cond = ([8.0, 9.0], [270.0, 265.0], [0.06, 0.06])
    for kw in (dict(yaw_n=1), dict(yaw_n=17), dict(refine_pass_n=0), dict(refine_pass_n=17)):
        with pytest.raises(ValueError):                    # WG_ERR_INVALID
            b.steady_optimize(*cond, **kw)
    sg = steady.hip_batch_for(x, y, deficit="super_gaussian")
    with pytest.raises(NotImplementedError):               # WG_ERR_UNSUPPORTED: model 0 is the HANDLE's flow model
        sg.steady_optimize(*cond, model="m0")
    yaw, power = sg.steady_optimize(*cond, model="blondel_jimenez", refine_pass_n=1, yaw_n=3)
    assert tuple(yaw.shape) == (2, len(x)) and tuple(power.shape) == (2,)
    sg.close()
    # the C entry itself: null pointers, and the same limits
    L = binding.load_library()
    w = torch.tensor([8.0, 270.001, 0.06], dtype=torch.float32, device="cuda")
    offs = steady.srf_offsets(2, 5, 30.0).cuda()
    out = torch.zeros(len(x), dtype=torch.float64, device="cuda")
    ptr = lambda t, k=0: C.c_void_p(t.data_ptr() + k * t.element_size())      # noqa: E731
    good = [b._h, 0, 1, ptr(w), ptr(w, 1), ptr(w, 2), 2, 5, ptr(offs), 30.0, ptr(out), None, None, None]
    assert L.wg_steady_optimize(*good) == 0                                   # power_dev and order_dev may be NULL
    torch.cuda.synchronize()
    for k in (0, 3, 4, 5, 8, 10):
        bad = list(good); bad[k] = None
        assert L.wg_steady_optimize(*bad) == -1, k
        assert b"null" in L.wg_last_error()
    for k, v in ((1, 2), (2, 0), (6, 0), (6, 17), (7, 1), (7, 17), (9, -1.0)):
        bad = list(good); bad[k] = v
        assert L.wg_steady_optimize(*bad) == -1, (k, v)
        assert b"wg_steady_optimize" in L.wg_last_error()


def _yaml(tmp_path, d, name="cfg.yaml"):
    import yaml
    p = tmp_path / name
    p.write_text(yaml.safe_dump(d))
    return str(p)


def _separate_handle(venv):
    """a handle of the same layout that shares nothing with the env"""
    from windgym_amd import steady
    return steady.hip_batch_for(np.array(venv.cfg.x_pos, dtype=np.float64), np.array(venv.cfg.y_pos, dtype=np.float64))


def test_optimal_yaws_and_the_vec_agent_across_autoresets(tmp_path):
    import windgym_amd as wg
    from windgym_amd import presets
    venv = wg.WindFarmVecEnv(wg.V80(), 16, yaml_path=_yaml(tmp_path, presets.env1_config()), turbtype="None", n_passthrough=1, seed=7)
    venv.reset()
    b = venv.batch
    other = _separate_handle(venv)
    try:
        for model in sc.MODELS:
            w = b.info("wind_f64").cpu().numpy()
            got = b.optimal_yaws(model=model, refine_pass_n=3, yaw_n=5)
            assert got.is_cuda and tuple(got.shape) == (16, venv.n_turb)
            want = b.steady_optimize(w[:, 0], w[:, 1], w[:, 2], model=model, refine_pass_n=3, yaw_n=5)[0]
            assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
        agent = wg.SteadyStateYawVecAgent(env=venv, refine_pass_n=3, yaw_n=5)
        a, _ = agent.predict(None)
        assert isinstance(a, np.ndarray) and a.shape == (16, venv.n_turb) and a.dtype == np.float32
        w0 = b.info("wind_f64").cpu().numpy()
        y0 = agent.optimized_yaws.cpu().numpy().copy()
        assert np.array_equal(y0, other.steady_optimize(w0[:, 0], w0[:, 1], w0[:, 2], refine_pass_n=3, yaw_n=5)[0].cpu().numpy())
        assert np.array_equal(a, agent.scale_yaw(y0).astype(np.float32))
        done = np.zeros(16, dtype=bool)
        for _ in range(1500):                                  # (env1, one flow passage: episodes of a few hundred steps)
            _, _, _, trunc, _ = venv.step(a)
            a, _ = agent.predict(None)
            if trunc.any():
                done |= trunc
                w1 = b.info("wind_f64").cpu().numpy()
                y1 = agent.optimized_yaws.cpu().numpy()
                assert np.array_equal(y1, other.steady_optimize(w1[:, 0], w1[:, 1], w1[:, 2], refine_pass_n=3, yaw_n=5)[0].cpu().numpy())
                assert np.array_equal(a, agent.scale_yaw(y1).astype(np.float32))
            if done.all():
                break
        assert done.any()
        moved = (w1 != w0).any(axis=1)
        assert moved[done].all() and (np.abs(y1[moved] - y0[moved]).max(axis=1) > 0).any()
        b.check()
    finally:
        other.close()
        venv.close()


def test_eval_sweep_gives_every_condition_its_own_yaws(tmp_path):
    import windgym_amd as wg
    from windgym_amd import presets
    from windgym_amd.evaluate import eval_sweep
    ypath = _yaml(tmp_path, presets.env1_config())
    wds, wss = [255.0, 270.0, 285.0], [8.0, 11.0]
    agent = wg.PyWakeVecAgent(refine_pass_n=3, yaw_n=5)          # unbound: eval_sweep binds it to its env
    eval_sweep(wg.V80(), ypath, agent, winddirs=wds, windspeeds=wss, turbintensities=[0.06], t_sim=4, turbtype="None")
    yaws = agent.optimized_yaws.cpu().numpy()
    one = wg.WindFarmVecEnv(wg.V80(), 1, yaml_path=ypath, turbtype="None", seed=0)
    one.reset()
    other = _separate_handle(one)
    one.close()
    try:
        conds = [(s, d) for s in wss for d in wds]                # eval_sweep's env order: speeds outermost
        assert yaws.shape == (len(conds), yaws.shape[1])
        for row, (s, d) in zip(yaws, conds):
            want = other.steady_optimize([s], [d], [0.06], model="blondel_jimenez", refine_pass_n=3, yaw_n=5)[0].cpu().numpy()[0]
            assert np.array_equal(row, want), (s, d)
        assert not np.array_equal(yaws[0], yaws[1]) and not np.array_equal(yaws[1], yaws[2])
    finally:
        other.close()
