"""GPU tests of the yaw table (windgym_amd/yaw_table.py; k_yaw_table_rows / _targets / _act of wg_yaw_table.hip, wg_rollout_table)
against the twins of tests/yaw_table_twin.py and tests/imitation_twin.py.  Every comparison is bit for bit: each rule is a fixed fp64
expression rounded at most once.  Envs and short-episode settings as in tests/test_gpu_imitation.py / tests/test_gpu_curriculum.py."""
import ctypes as C

import numpy as np
import pytest

import imitation_twin as itw
import rl_helpers
import yaw_table_twin as tw
from rl_helpers import _torch, _venv

pytestmark = pytest.mark.gpu
SEARCH = dict(refine_pass_n=3, yaw_n=5, search_yaw_max=30.0)        # a small Serial-Refine: the tests are about the table
TI, WS, WD = np.array([0.04, 0.11]), np.array([7.0, 8.5, 10.0, 12.0, 14.5]), np.array([258.0, 270.0, 281.0])      # 2 x 5 x 3 nodes


def _bits(x):
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def _small_venv(n_envs, method):
    """the small env of tests/test_gpu_imitation.py (presets.env1_config: two turbines by two)"""
    from windgym_amd import presets
    d = presets.env1_config()
    d["ActionMethod"] = method
    return _venv(n_envs, yaml_dict=d, n_passthrough=0.5)


def _env_table(v, model="blondel_jimenez", **kw):
    """a table over the env's own wind ranges, coarse: every sampled wind has a row, most are between nodes"""
    from windgym_amd.yaw_table import YawTable, default_axis
    c = v.cfg
    return YawTable.build(v, ws=default_axis(c.ws_min, c.ws_max, 2.0), wd=default_axis(c.wd_min, c.wd_max, 7.0), model=model, **SEARCH, **kw)


# ---- 1. build ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("farm", ["two_turbine", "farm_4x4"])
def test_build_rows_are_the_optimiser_at_the_nodes(farm):
    from windgym_amd.yaw_table import YawTable, node_winds
    t = _torch()
    from windgym_amd import presets
    v = _venv(4, yaml_dict=presets.two_turb_config(), n_passthrough=0.5) if farm == "two_turbine" else _venv(4, n_passthrough=0.3)
    assert v.n_turb == (2 if farm == "two_turbine" else 16)
    w = node_winds(TI, WS, WD)
    assert w.shape == (30, 3) and list(w[0]) == [7.0, 258.0, 0.04] and list(w[1]) == [7.0, 270.0, 0.04] and list(w[3]) == [8.5, 258.0, 0.04]
    for model in ("m0", "blondel_jimenez"):
        tab = YawTable.build(v, ws=WS, wd=WD, ti=TI, model=model, **SEARCH)
        yaw, power = v.batch.steady_optimize(w[:, 0], w[:, 1], w[:, 2], model=model, refine_pass_n=3, yaw_n=5, yaw_max=30.0)
        assert (tab.n_rows, tab.N) == (30, v.n_turb) and tab.yaw.dtype == t.float64 and tab.args["model"] == model
        assert t.equal(tab.yaw, yaw) and t.equal(tab.power, power)
        assert float(tab.yaw.abs().max()) > 0.0                            # (the optimiser steers somewhere on this grid)
        # a node's own wind finds its own row, and its yaws
        wd_ = t.from_numpy(w).to(v.batch.device)
        assert t.equal(tab.rows(wd_).cpu(), t.arange(30, dtype=t.int32)) and t.equal(tab.targets(wd_), tab.yaw)
        tab.close()
    # the defaults: the env's ranges every 1 m/s and every degree, three TI nodes
    c = v.cfg
    if farm == "two_turbine":
        tab = YawTable.build(v, refine_pass_n=1, yaw_n=3)
        assert np.array_equal(tab.ws, np.arange(c.ws_min, c.ws_max + 1.0)) and np.array_equal(tab.wd, np.arange(c.wd_min, c.wd_max + 1.0))
        assert np.array_equal(tab.ti, np.linspace(c.TI_min, c.TI_max, 3)) and tab.n_rows == len(tab.ws) * len(tab.wd) * 3
        tab.close()
    v.batch.check()
    v.close()


# ---- 2. rows / targets -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_env():
    v = _small_venv(4, "yaw")
    yield v
    v.close()


@pytest.mark.parametrize("wrap", [False, True], ids=["plain", "wrap"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_rows_and_targets_equal_the_twin(small_env, n, wrap):
    from windgym_amd.yaw_table import YawTable
    t = _torch()
    v = small_env
    rng = np.random.default_rng(100 * n + wrap)
    ti = np.array([0.06])                                                       # one node, two nodes, 37 non-uniform ones
    ws = np.array([6.0, 11.5])
    wd = np.cumsum(rng.uniform(0.5, 9.5, 37)) + (-20.0 if wrap else 200.0)
    yaw = rng.uniform(-30.0, 30.0, (74, v.n_turb))
    tab = YawTable(ti, ws, wd, yaw, wrap_wd=wrap, venv=v)
    # random winds, every node, every exact midpoint, values outside both ends, +-inf / NaN
    mid = lambda a: (a[:-1] + a[1:]) / 2.0                                      # noqa: E731
    pick = lambda a, k: rng.choice(np.concatenate([a, mid(np.append(a, a[0] + 360.0)), [a[0] - 1e3, a[-1] + 1e3, a[0] - 1e-9, a[-1] + 1e-9],  # noqa: E731
                                                   rng.uniform(a[0] - 720.0, a[0] + 720.0, 64)]), k)
    wind = np.stack([pick(ws, n), pick(wd, n), pick(ti, n)], axis=1)
    bad = np.array([[np.nan, 270.0, 0.06], [8.0, np.inf, 0.06], [8.0, 270.0, -np.inf], [np.nan, np.nan, np.nan]])
    k = min(n, 4) if n > 1 else 0
    wind[n - k:] = bad[:k]
    mask = (rng.uniform(size=n) < 0.6).astype(np.uint8)
    if n >= 63:
        assert 0 < mask.sum() < n
    ref = tw.rows(ti, ws, wd, wind, wrap_wd=wrap)
    if k:
        assert list(ref[n - k:]) == [-1] * k and ref[:n - k].min() >= 0
    dw, dm = rl_helpers.dev(wind, mask)
    assert np.array_equal(tab.rows(dw).cpu().numpy(), ref)
    assert np.array_equal(tab.rows(dw, dm).cpu().numpy(), tw.rows(ti, ws, wd, wind, mask, wrap))
    out = t.full((n, v.n_turb), -77.0, dtype=t.float64, device=dw.device)
    tab.targets(dw, out=out)
    assert np.array_equal(_bits(out), _bits(tw.targets(yaw, ref, np.full((n, v.n_turb), -77.0))))      # a -1 row leaves its row untouched
    tab.close()


# ---- 3. act --------------------------------------------------------------------------------------------------------------------------------------
def _act_twin(v, tab):
    b, c = v.batch, v.cfg
    wind, prev = b.info("wind_f64").cpu().numpy(), b.info("yaw_agent").cpu().numpy()
    r = tw.rows(tab.ti, tab.ws, tab.wd, wind, wrap_wd=tab.wrap_wd)
    assert r.min() >= 0
    return tw.action(c.ActionMethod, tab.yaw.cpu().numpy()[r], prev, c.yaw_min, c.yaw_max, c.yaw_step), r


@pytest.mark.parametrize("method", ["yaw", "wind"])
def test_act_equals_the_label_expression(method):
    from windgym_amd.yaw_table import YawTableAgent
    t = _torch()
    v = _small_venv(33, method)
    tab = _env_table(v)
    agent = YawTableAgent(tab, env=v)
    ref, r = _act_twin(v, tab)
    assert len(set(r.tolist())) > 4                                              # the envs' winds spread over the table
    a, state = agent.predict(None)
    assert state is None and a.is_cuda and np.array_equal(_bits(a), _bits(ref))
    rnd = rl_helpers.dev(np.random.default_rng(3).uniform(-1, 1, (5, 33, v.n_turb)).astype(np.float32))[0]
    for k in range(5):                                                           # yaws away from their start, then the table takes over
        v.step(rnd[k])
    for k in range(4):
        ref, _ = _act_twin(v, tab)
        a, _ = agent.predict(None)
        assert np.array_equal(_bits(a), _bits(ref)) and float(a.abs().max()) <= 1.0
        v.step(a)
    assert float(t.as_tensor(ref).abs().max()) > 0.0
    v.batch.check()
    tab.close(); v.close()


# ---- 4. + 5. the closed loop, and the labels that close the circle ------------------------------------------------------------------------------
KEYS = ("obs", "actions", "reward", "truncated", "final_obs", "yaw_agent")


@pytest.mark.parametrize("method", ["yaw", "wind"])
def test_rollout_equals_the_host_loop_and_its_labels(method):
    from windgym_amd.binding import ExpertLabels
    from windgym_amd.yaw_table import YawTableAgent
    t = _torch()
    B = 33
    va, vb = _small_venv(B, method), _small_venv(B, method)
    tab, tab_b = _env_table(va), _env_table(vb)
    assert t.equal(tab.yaw, tab_b.yaw)
    tm = va.batch.info("time_max").cpu().numpy()
    T = int(tm.min()) + 3                                                        # episodes end inside the rollout
    assert T < int(tm.max()) + 3 and T <= 64, tm
    b = va.batch
    yaw0, wind0 = b.info("yaw_agent").clone(), b.info("wind_f64").clone()
    steps = va._policy_steps
    out = va.rollout(YawTableAgent(tab, env=va), T, record=("yaw_agent", "wind_f64"))
    assert not any(k in out for k in ("raw", "logp", "value", "final_value")) and va._policy_steps == steps
    tr = out["truncated"].bool()
    assert bool(tr[:T - 1].any()) and not bool(tr.any(dim=0).all())             # an autoreset before the last step; an env without one
    # the host loop
    agent_b = YawTableAgent(tab_b, env=vb)
    ref = {k: [] for k in KEYS}
    ref["obs"].append(vb.batch.obs.clone())
    for _ in range(T):
        a, _ = agent_b.predict(None)
        ref["actions"].append(a.clone())
        obs, rew, _, trunc, infos = vb.step(a)
        for k, x in (("obs", obs), ("reward", rew), ("truncated", trunc.view(t.uint8)), ("final_obs", infos["final_obs"]),
                     ("yaw_agent", vb.batch.info("yaw_agent"))):
            ref[k].append(x.clone())
    for k in KEYS:
        assert np.array_equal(_bits(out[k]), _bits(t.stack(ref[k]))), k
    for x, y in ((b.obs, vb.batch.obs), (b.reward, vb.batch.reward), (b.truncated, vb.batch.truncated), (b.final_obs, vb.batch.final_obs)):
        assert t.equal(x, y)                                                     # the persistent outputs follow, as after a step()
    assert va.batch.get_state() == vb.batch.get_state()
    # 5. wg_expert_labels on that rollout, its targets from the table: the labels are the actions the table agent took
    ep_row = tab.rows(out["wind_f64"], out["truncated"])
    assert int((ep_row >= 0).sum()) == int(tr.sum()) and ep_row.dtype == t.int32 and tuple(ep_row.shape) == (T, B)
    targets = tab.targets(wind0)
    labels = t.full((T, B, b.N), 9.0, device=b.device)
    lab = ExpertLabels(b)
    lab.labels(T, yaw0, out["yaw_agent"], out["truncated"], ep_row, tab.yaw, tab.n_rows, targets, labels)
    lab.check()
    assert np.array_equal(_bits(labels), _bits(out["actions"]))
    assert t.equal(targets, tab.targets(b.info("wind_f64")))                     # the running targets followed the autoresets
    b.check()
    tab.close(); tab_b.close(); va.close(); vb.close()


# ---- 6. the curriculum -----------------------------------------------------------------------------------------------------------------------------
def test_curriculum_with_table_targets_equals_the_direct_shaping():
    from windgym_amd.binding import Curriculum
    from windgym_amd.curriculum import YawCurriculum
    t = _torch()
    B, T = 16, 40
    v = _venv(B, n_passthrough=0.3)
    b = v.batch
    tab = _env_table(v)
    p = rl_helpers.make(b.obs_dim, (64, 64), v.n_turb)[0]
    cur = YawCurriculum(v, curriculum_steps=4 * T * B, pure_similarity_steps=T * B // 2, targets=tab)
    assert cur.last_n_targets is None and t.equal(cur.targets, tab.targets(b.info("wind_f64")))
    direct = Curriculum(b)
    direct.set_targets(cur.targets.clone())
    n_trunc = 0
    for k in range(2):
        yaw0 = b.info("yaw_agent").clone()
        out = cur.rollout(p, T, num_timesteps=k * T * B)
        assert cur.last_n_targets is None
        n_trunc += int(out["truncated"].sum())
        rows = tw.rows(tab.ti, tab.ws, tab.wd, out["wind_f64"].cpu().numpy(), out["truncated"].cpu().numpy(), tab.wrap_wd)     # on the host
        ep_row = rl_helpers.dev(rows)[0]
        shaped, diff = t.zeros((T, B), device=b.device), t.zeros((T, B), device=b.device)
        direct.shape(T, yaw0, out["actions"], out["yaw_agent"], out["truncated"], ep_row, tab.yaw, tab.n_rows, out["curriculum_weight"],
                     cur.reward_momentum, out["env_reward"], shaped, diff)
        assert np.array_equal(_bits(out["reward"]), _bits(shaped)) and np.array_equal(_bits(out["yaw_diff"]), _bits(diff)), k
        assert t.equal(cur.targets, tab.targets(b.info("wind_f64")))
        if k == 0:
            assert n_trunc > 0                                                   # the second rollout is shaped against targets the first one set
    assert cur.state() == direct.state()
    b.check()
    cur.close(); direct.close(); p.close(); tab.close(); v.close()


# ---- 7. behaviour cloning, and no Serial-Refine launch left -----------------------------------------------------------------------------------------
def test_trainers_run_from_the_table_alone(monkeypatch, tmp_path):
    from windgym_amd.imitation import BehaviorCloning
    from windgym_amd.ppo import PPO
    t = _torch()
    B, T = 8, 30
    v = _small_venv(B, "yaw")
    b, c = v.batch, v.cfg
    tab = _env_table(v)

    def no_optimiser(*a, **kw):
        raise AssertionError("a Serial-Refine launch with the targets coming from a table")
    monkeypatch.setattr(b, "steady_optimize", no_optimiser)
    monkeypatch.setattr(b, "optimal_yaws", no_optimiser)
    bc = BehaviorCloning("MlpPolicy", v, expert=tab, n_steps=T, n_epochs=1, seed=2)
    assert bc.last_n_targets is None
    g0, yaw0 = bc.targets.cpu().numpy(), b.info("yaw_agent").cpu().numpy()
    assert np.array_equal(g0, tab.yaw.cpu().numpy()[tw.rows(tab.ti, tab.ws, tab.wd, b.info("wind_f64").cpu().numpy())])
    out = bc.collect()
    assert int(out["truncated"].sum()) > 0 and bc.last_n_targets is None
    rows = tw.rows(tab.ti, tab.ws, tab.wd, out["wind_f64"].cpu().numpy(), out["truncated"].cpu().numpy())
    rl, rd, rg, bad = itw.labels_numpy(yaw0, out["yaw_agent"].cpu().numpy(), out["truncated"].cpu().numpy(), rows, tab.yaw.cpu().numpy(), g0,
                                       c.ActionMethod, c.yaw_min, c.yaw_max, c.yaw_step)
    assert bad is None
    assert np.array_equal(_bits(out["labels"]), _bits(rl)) and np.array_equal(_bits(out["yaw_diff"]), _bits(rd))
    assert np.array_equal(bc.targets.cpu().numpy(), rg)
    bc.learn(2 * T * B)
    assert len(bc.log) == 2 and all(np.isfinite(rec[k]) for rec in bc.log for k in ("loss", "mean_yaw_diff"))
    # the checkpoint carries the table
    path = bc.save(str(tmp_path / "bc.zip"))
    back = BehaviorCloning.load(path, v)
    assert back.table is not None and t.equal(back.table.yaw, tab.yaw) and np.array_equal(back.table.wd, tab.wd) and t.equal(back.targets, bc.targets)
    back.close(); back.policy.close(); back.table.close()
    ppo = PPO("MlpPolicy", v, n_steps=T, n_epochs=1, seed=1, curriculum=dict(curriculum_steps=8 * T * B, pure_similarity_steps=T * B, targets=tab))
    ppo.learn(2 * T * B)
    assert ppo.curriculum.table is tab and ppo.curriculum.last_n_targets is None
    assert len(ppo.log) == 2 and all(np.isfinite(rec[k]) for rec in ppo.log for k in ("curriculum_weight", "mean_yaw_diff"))
    path = ppo.save(str(tmp_path / "ppo.zip"))
    again = PPO.load(path, v)
    assert t.equal(again.curriculum.table.yaw, tab.yaw) and again.curriculum.state() == ppo.curriculum.state()
    again.curriculum.table.close(); again.close(); again.policy.close()
    b.check()
    ppo.close(); ppo.policy.close(); bc.close(); bc.policy.close(); tab.close(); v.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(small_env):
    from windgym_amd.binding import YawTableHandle
    from windgym_amd.curriculum import YawCurriculum
    from windgym_amd.imitation import BehaviorCloning
    from windgym_amd.normalize import VecNormalize
    from windgym_amd.population import Population, PPOPopulation
    from windgym_amd.ppo import PPO
    from windgym_amd.yaw_table import YawTable, YawTableAgent
    t = _torch()
    v = small_env
    b, L = v.batch, v.batch.L
    dev = b.device
    N = b.N
    yaw = t.zeros((6, N), dtype=t.float64, device=dev)
    mk = lambda ti, ws, wd, wrap=False, y=yaw: YawTableHandle(t, dev, ti, ws, wd, wrap, y)      # noqa: E731  (the library's own checks)
    # wg_yaw_table_create
    for args, msg in ((([0.1], [9.0, 8.0], [0.0, 1.0, 2.0]), "wg_yaw_table_create: ws is not strictly ascending at index 1"),
                      (([0.1], [8.0, 8.0], [0.0, 1.0, 2.0]), "ws is not strictly ascending"),
                      (([], [8.0, 9.0], [0.0, 1.0, 2.0]), r"wg_yaw_table_create: ti is empty \(n_ti = 0\)"),
                      (([0.1], [8.0, np.inf], [0.0, 1.0, 2.0]), r"ws\[1\] is not finite"),
                      (([0.1], [8.0, 9.0], [0.0, 100.0, 360.0], True), "wrap_wd: wd spans 360")):
        with pytest.raises(ValueError, match=msg):
            mk(*args)
    with pytest.raises(NotImplementedError, match="1027 nodes together"):
        mk([0.1], [8.0, 9.0], np.arange(1024.0), y=t.zeros((2048, N), dtype=t.float64, device=dev))
    with pytest.raises(ValueError, match="yaw must be a contiguous float64 CUDA tensor"):
        mk([0.1], [8.0, 9.0], [0.0, 1.0, 2.0], y=yaw.cpu())
    h = C.c_void_p()
    ax = (C.c_double * 3)(0.0, 1.0, 2.0)
    for args, msg in (((ax, 1, ax, 2, ax, 3, 0, N, None, 1, C.byref(h)), "yaw is null"), ((ax, 1, ax, 2, ax, 3, 0, 0, yaw.data_ptr(), 1, C.byref(h)), "N must be >= 1"),
                      ((ax, 1, ax, 2, ax, 3, 0, N, yaw.data_ptr(), 1, None), "out is null"), ((ax, 1, None, 2, ax, 3, 0, N, yaw.data_ptr(), 1, C.byref(h)), "ws is null"),
                      ((ax, 1, ax, 2, ax, 3, 0, N, ax, 1, C.byref(h)), "yaw is not")):
        assert L.wg_yaw_table_create(dev.index, *args) == -1 and msg in L.wg_last_error().decode(), msg
    # wg_yaw_table_rows / _targets
    tab = YawTable([0.1], [8.0, 9.0], [0.0, 1.0, 2.0], yaw, venv=v)
    hd = tab._tab._h
    wind = t.zeros((5, 3), dtype=t.float64, device=dev)
    rows, tg = t.zeros(5, dtype=t.int32, device=dev), t.zeros((5, N), dtype=t.float64, device=dev)
    host = np.zeros(64)
    hp = host.ctypes.data
    for fn, args, msg in ((L.wg_yaw_table_rows, (None, 5, wind.data_ptr(), None, rows.data_ptr(), None), "null table"),
                          (L.wg_yaw_table_rows, (hd, -1, wind.data_ptr(), None, rows.data_ptr(), None), "n must be >= 0, got -1"),
                          (L.wg_yaw_table_rows, (hd, 5, None, None, rows.data_ptr(), None), "wind_dev is null"),
                          (L.wg_yaw_table_rows, (hd, 5, wind.data_ptr(), None, None, None), "rows_out is null"),
                          (L.wg_yaw_table_rows, (hd, 5, hp, None, rows.data_ptr(), None), "wg_yaw_table_rows: wind_dev is not"),
                          (L.wg_yaw_table_rows, (hd, 5, wind.data_ptr(), hp, rows.data_ptr(), None), "wg_yaw_table_rows: mask_dev is not"),
                          (L.wg_yaw_table_rows, (hd, 5, wind.data_ptr(), None, hp, None), "wg_yaw_table_rows: rows_out is not"),
                          (L.wg_yaw_table_targets, (None, 5, wind.data_ptr(), tg.data_ptr(), None), "null table"),
                          (L.wg_yaw_table_targets, (hd, -2, wind.data_ptr(), tg.data_ptr(), None), "n must be >= 0, got -2"),
                          (L.wg_yaw_table_targets, (hd, 5, None, tg.data_ptr(), None), "wind_dev is null"),
                          (L.wg_yaw_table_targets, (hd, 5, wind.data_ptr(), None, None), "targets_out is null"),
                          (L.wg_yaw_table_targets, (hd, 5, wind.data_ptr(), hp, None), "wg_yaw_table_targets: targets_out is not"),
                          (L.wg_yaw_table_act, (None, hd, tg.data_ptr(), None), "null handle"),
                          (L.wg_yaw_table_act, (b._h, None, tg.data_ptr(), None), "tab is null"),
                          (L.wg_yaw_table_act, (b._h, hd, None, None), "action_out is null")):
        assert fn(*args) == -1 and msg in L.wg_last_error().decode(), msg
    assert L.wg_yaw_table_rows(hd, 0, wind.data_ptr(), None, rows.data_ptr(), None) == 0          # n == 0 does nothing
    for call, msg in ((lambda: tab.rows(wind.float()), "wind must be a contiguous float64 CUDA tensor"), (lambda: tab.rows(wind.cpu()), "wind must be"),
                      (lambda: tab.rows(wind, t.zeros(4, dtype=t.uint8, device=dev)), "mask must be"), (lambda: tab.targets(wind, out=tg[:4]), "out must be")):
        with pytest.raises(ValueError, match=msg):
            call()
    # a table for another farm: wg_yaw_table_act, wg_rollout_table and every Python entry
    big = _venv(4, n_passthrough=0.3)
    agent = YawTableAgent(tab, env=big)
    out16 = t.zeros((4, 16), device=dev)
    with pytest.raises(ValueError, match=f"wg_yaw_table_act: tab holds yaws of {N} turbines, the handle's n_turb is 16"):
        tab._tab.act(big.batch, out16)
    before, steps = big.batch.get_state(), big._policy_steps
    pol = rl_helpers.make(big.batch.obs_dim, (8,), 16)[0]
    bufs = {k: x.clone() for k, x in big.rollout(pol, 2).items()}
    state = big.batch.get_state()
    assert state != before
    with pytest.raises(ValueError, match=f"wg_rollout_table: tab holds yaws of {N} turbines"):
        big.batch.rollout("wg_rollout_table", (tab._tab._h,), 2, bufs, ())
    for call, msg in ((lambda: agent.predict(None), f"table holds yaws of {N} turbines"), (lambda: big.rollout(agent, 2), f"table holds yaws of {N} turbines"),
                      (lambda: YawCurriculum(big, 100, 10, targets=tab), rf"YawCurriculum\(targets=\): table holds yaws of {N} "),
                      (lambda: BehaviorCloning("MlpPolicy", big, expert=tab), rf"BehaviorCloning\(expert=\): table holds yaws of {N} "),
                      (lambda: YawCurriculum(big, 100, 10, targets="table"), "targets must be a yaw_table.YawTable"),
                      (lambda: YawTable.load(_saved(tab), big), f"venv: the table holds yaws of {N} turbines, this env has 16")):
        with pytest.raises(ValueError, match=msg):
            call()
    # wg_rollout_table's own: what a table cannot fill, what a rollout needs
    tab16 = YawTable([0.1], [8.0, 9.0], [0.0, 1.0, 2.0], t.zeros((6, 16), dtype=t.float64, device=dev), venv=big)
    plain = {k: x for k, x in bufs.items() if k not in ("raw", "logp", "value", "final_value")}
    for bad, msg in ((dict(plain, raw=bufs["raw"]), "wg_rollout_table: raw, logp, value and final_value must be NULL"),
                     (dict(plain, final_value=bufs["final_value"]), "must be NULL"),
                     ({k: x for k, x in plain.items() if k != "obs"}, "wg_rollout_table: obs, actions, reward and truncated buffers are required")):
        with pytest.raises(ValueError, match=msg):
            big.batch.rollout("wg_rollout_table", (tab16._tab._h,), 2, bad, ())
    with pytest.raises(ValueError, match="wg_rollout_table: n_steps < 0"):
        big.batch.rollout("wg_rollout_table", (tab16._tab._h,), -1, plain, ())
    with pytest.raises(ValueError, match="unknown info field"):
        big.rollout(YawTableAgent(tab16, env=big), 2, record=("no_such_field",))
    with pytest.raises(ValueError, match="n_steps must be >= 1"):
        big.rollout(YawTableAgent(tab16, env=big), 0)
    # section 3: who does not take a table agent
    good = YawTableAgent(tab16, env=big)
    for call, msg in ((lambda: PPO(good, big), "PPO: a YawTableAgent is a scripted agent"), (lambda: PPOPopulation([good, good], big), "PPOPopulation: a YawTableAgent"),
                      (lambda: Population([good]), "a population: a YawTableAgent"), (lambda: VecNormalize(big).rollout(good, 2), r"VecNormalize.rollout\(\): a YawTableAgent")):
        with pytest.raises(NotImplementedError, match=msg):
            call()
    # ... and every refusal above left the env as it was
    assert big.batch.get_state() == state and big._policy_steps == steps + 2
    out = big.rollout(good, 2)                                                   # (the same objects do run)
    assert tuple(out["actions"].shape) == (2, 4, 16) and big._policy_steps == steps + 2
    big.batch.check()
    pol.close(); tab16.close(); big.close(); tab.close()


def _saved(tab):
    import io
    return io.BytesIO(tab.to_bytes())


def test_refusals_multi_and_sample_site():
    import copy
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnvMulti
    from windgym_amd.site import hornsrev1_site
    from windgym_amd.turbine import V80
    from windgym_amd.yaw_table import YawTable, YawTableAgent
    t = _torch()
    m = WindFarmVecEnvMulti(V80(), 2, yaml_dict=copy.deepcopy(presets.multi_3x3_config()), seed=5, turbtype="None", n_rotor_pts=16, n_passthrough=0.3)
    m.reset(seed=5)
    tab = YawTable([0.1], [8.0], [270.0], t.zeros((1, m.n_turb), dtype=t.float64, device=m.batch.device), venv=m)
    state = m.batch.get_state()
    with pytest.raises(NotImplementedError, match=r"WindFarmVecEnvMulti.rollout\(\): a YawTableAgent is not implemented"):
        m.rollout(YawTableAgent(tab, env=m), 2)
    assert m.batch.get_state() == state
    tab.close(); m.close()
    vs = _venv(2, sample_site=hornsrev1_site(), n_passthrough=0.3)
    tab = YawTable([0.1], [8.0], [270.0], t.zeros((1, 16), dtype=t.float64, device=vs.batch.device), venv=vs)
    state = vs.batch.get_state()
    with pytest.raises(NotImplementedError, match=r"rollout\(\): a YawTableAgent with sample_site is not implemented"):
        vs.rollout(YawTableAgent(tab, env=vs), 2)
    assert vs.batch.get_state() == state
    tab.close(); vs.close()
