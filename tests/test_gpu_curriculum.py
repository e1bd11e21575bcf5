"""GPU tests of the yaw curriculum: k_curriculum (wg_curriculum_shape) against the float64 numpy restatement of the reference's
CurriculumWrapper (windgym_amd.curriculum.shape_numpy, itself pinned to the reference class by tests/test_curriculum.py), the
restated yaw actuation against the env's own record, targets that follow same-step autoresets, the state carried across calls,
the no-op limit, ``PPO(..., curriculum=...)`` against the hand-written loop, bit-identical resume, the shared per-turbine policy,
the refusals.

The 1-ulp bar of the by-value checks is derived, not measured: kernel and restatement evaluate the same float64 expressions on
identical float32 inputs (yaws, rewards) and float64 inputs (targets, weights) and round to float32 ONCE; they differ in the
contraction of a few float64 multiply-adds (relative 1e-16 per operation over a recurrence that forgets with the momentum), which
moves a float32 rounding by at most one unit in the last place."""
import copy
import functools
import os

import numpy as np
import pytest

import rl_helpers
from rl_helpers import _ti_farm_history_100, _torch, _venv

pytestmark = pytest.mark.gpu
make = functools.partial(rl_helpers.make, draw="normal")
CUR = dict(curriculum_steps=4000, pure_similarity_steps=400)       # 16 envs x 96 steps = 1536 env steps per rollout: the ramp is crossed


def _env(case):
    """-> (env, T, every env truncates inside T?)"""
    from windgym_amd import presets
    if case == "yaw_cfg2":                 # ActionMethod "yaw", 4 x 4 farm, episodes of 30 to 65 steps
        return _venv(16, n_passthrough=0.3), 96, True
    if case == "wind_env1":                # ActionMethod "wind", Env1.yaml's 2 x 2 farm
        return _venv(16, yaml_dict=presets.env1_config(), n_passthrough=0.5), 96, True
    if case == "farm_3x2":                 # the 3 x 2 farm with the 100-sample history (k_glue's ring staging), episodes of 21 to 43 steps
        return _venv(16, yaml_dict=_ti_farm_history_100(), n_passthrough=0.3), 96, True
    if case == "horns_rev":                # 80 turbines: per-turbine state well past any register array
        x, y = presets.horns_rev1_layout()
        return _venv(4, yaml_dict=presets.horns_rev_config(), x_pos=x, y_pos=y, n_passthrough=0.5), 8, False
    if case == "multi_3x3":                # one policy shared by the turbines
        from windgym_amd.envs import WindFarmVecEnvMulti
        from windgym_amd.turbine import V80
        m = WindFarmVecEnvMulti(V80(), 8, yaml_dict=copy.deepcopy(presets.multi_3x3_config()), seed=5, turbtype="None", n_rotor_pts=16,
                                n_passthrough=0.3)
        m.reset(seed=5)
        return m, 64, True
    raise KeyError(case)


def _policy(v):
    multi = hasattr(v, "possible_agents")
    return make(v.obs_len, (64, 64), 1)[0] if multi else make(v.batch.obs_dim, (64, 64), v.n_turb)[0]


def _ulp_equal(got32, want64):
    """got (float32, device result) within one float32 ulp of the float32-rounded float64 reference"""
    want32 = np.asarray(want64, np.float64).astype(np.float32)
    err = np.abs(got32.astype(np.float64) - want32.astype(np.float64))
    return bool(np.all(err <= np.spacing(np.abs(want32)).astype(np.float64))), float(err.max())


def _rollout_vs_numpy(v, cur, p, T, num_timesteps, every_env_truncates):
    """Checks 1 to 3 of one ``cur.rollout``; returns its dict."""
    from windgym_amd.curriculum import shape_numpy, targets_per_step
    t = _torch()
    b = v.batch
    B, N = b.B, b.N
    g0 = cur.targets.clone()
    yaw0 = b.info("yaw_agent").clone()
    assert g0.dtype == t.float64 and tuple(g0.shape) == (B, N) and g0.is_cuda
    out = cur.rollout(p, T, num_timesteps=num_timesteps, yaw_out=True)
    b.check()
    tr = out["truncated"].bool()
    if every_env_truncates:
        assert bool(tr.any(dim=0).all()), tr.sum(dim=0)
    assert tuple(out["reward"].shape) == (T, B) == tuple(out["env_reward"].shape) == tuple(out["yaw_diff"].shape)
    assert tuple(out["curriculum_weight"].shape) == (T,) and out["curriculum_weight"].dtype == t.float64
    assert cur.last_n_targets == int(tr.sum())

    # 2. the actuation restated: the record on every step that did not truncate, inside the limits where the record is the next episode's
    held, rec = out["yaw_held"], out["yaw_agent"]
    assert t.equal(held[~tr], rec[~tr])
    prev = t.cat([yaw0[None], rec[:-1]])
    c = v.cfg
    slack = float(np.spacing(np.float32(max(abs(c.yaw_min), abs(c.yaw_max)))))     # yaw +- yaw_step is itself rounded to float32
    assert bool((held >= c.yaw_min).all()) and bool((held <= c.yaw_max).all())
    assert float((held.double() - prev.double()).abs().max()) <= float(c.yaw_step) + slack
    if every_env_truncates:
        assert not t.equal(held[tr], rec[tr])                                      # (the record there IS another episode's yaw)

    # 3. the targets follow the autoresets
    assert t.equal(cur.targets, b.optimal_yaws(model=cur.model, refine_pass_n=cur.refine_pass_n, yaw_n=cur.yaw_n, yaw_max=cur.search_yaw_max))
    idx = tr.reshape(-1).nonzero().reshape(-1)
    wind = out["wind_f64"].reshape(-1, 3)[idx]
    new = np.zeros((0, N))
    if idx.numel():
        new = b.steady_optimize(wind[:, 0], wind[:, 1], wind[:, 2], model=cur.model, refine_pass_n=cur.refine_pass_n, yaw_n=cur.yaw_n,
                                yaw_max=cur.search_yaw_max)[0].cpu().numpy()
    idx = idx.cpu().numpy()
    now = cur.targets.cpu().numpy()
    for e in range(B):          # the target in force after an env's truncations is the optimum of the wind recorded at the last of them
        mine = np.flatnonzero(idx % B == e)
        assert np.array_equal(now[e], new[mine[-1]] if len(mine) else g0[e].cpu().numpy()), e
    first = int(np.flatnonzero(tr[:, 0].cpu().numpy())[0]) if bool(tr[:, 0].any()) else None
    if first is not None and int(tr[:, 0].sum()) == 1:      # env 0 truncated once: its first new target is the one in force
        w0 = out["wind_f64"][first, 0]
        assert t.equal(cur.targets[0], b.steady_optimize(w0[0:1], w0[1:2], w0[2:3], model=cur.model, refine_pass_n=cur.refine_pass_n,
                                                         yaw_n=cur.yaw_n, yaw_max=cur.search_yaw_max)[0][0])

    # 1. the kernel against the restatement, env by env
    trn, g0n = tr.cpu().numpy(), g0.cpu().numpy()
    y = np.where(trn[:, :, None], held.cpu().numpy(), rec.cpu().numpy()).astype(np.float64)
    r, w = out["env_reward"].cpu().numpy(), out["curriculum_weight"].cpu().numpy()
    assert np.array_equal(w, cur.weights(num_timesteps, T))
    shaped, diff = out["reward"].cpu().numpy(), out["yaw_diff"].cpu().numpy()
    state = getattr(cur, "_numpy_state", None) or [None] * B
    worst = [0.0, 0.0]
    for e in range(B):
        mine = new[idx % B == e]                               # this env's new episodes, in step order
        tg = targets_per_step(g0n[e], trn[:, e], mine)
        s_ref, d_ref, state[e] = shape_numpy(y[:, e], r[:, e], tg, w, cur.reward_momentum, c.yaw_max, state[e])
        (ok_s, e_s), (ok_d, e_d) = _ulp_equal(shaped[:, e], s_ref), _ulp_equal(diff[:, e], d_ref)
        worst = [max(worst[0], e_s), max(worst[1], e_d)]
        assert ok_s and ok_d, (e, e_s, e_d)
    cur._numpy_state = state
    print(f"worst |shaped - ref| = {worst[0]:.3e}, worst |yaw_diff - ref| = {worst[1]:.3e}")
    return out


@pytest.mark.parametrize("case", ["yaw_cfg2", "wind_env1", "farm_3x2", "horns_rev", "multi_3x3"])
def test_rollout_against_the_numpy_restatement(case):
    """Checks 1, 2, 3 and 8: shaped reward and yaw_diff within one float32 ulp of shape_numpy on the recorded yaws, rewards, weights
    and device-computed targets; yaw_held == the recorded yaws bit for bit where no reset intervened; the targets are the optimum of
    each env's current wind.  Two rollouts in a row: the second starts from a state with history, mid-ramp."""
    from windgym_amd.curriculum import YawCurriculum
    from windgym_amd.ppo import PPO
    v, T, full = _env(case)
    p = _policy(v)
    cur = YawCurriculum(v, **CUR)
    out = _rollout_vs_numpy(v, cur, p, T, 0, full)
    w = out["curriculum_weight"]
    if full:
        assert float(w[0]) == 0.0 and float(w[-1]) > 0.0
    _rollout_vs_numpy(v, cur, p, T, T * v.num_envs, full)
    if case == "multi_3x3":                 # one PPO iteration with a centralised critic runs on the shaped reward
        ppo = PPO("MlpPolicy", v, critic="central", n_steps=T, n_epochs=1, seed=3, curriculum=cur)
        ppo.learn(T * v.num_envs)
        assert np.isfinite(ppo.log[0]["loss"]) and 0.0 <= ppo.log[0]["curriculum_weight"] <= 1.0 and ppo.log[0]["mean_yaw_diff"] > 0
        ppo.close(); ppo.policy.close()
    v.batch.check()
    cur.close(); p.close(); v.close()


def test_m0_targets_and_reset():
    """model="m0": the targets are the env's own steady-state optimum; reset() re-targets and leaves the shaping state alone."""
    from windgym_amd.curriculum import YawCurriculum
    t = _torch()
    v = _venv(16, n_passthrough=0.3)
    cur = YawCurriculum(v, 100, 10, model="m0", refine_pass_n=2, yaw_n=5)
    assert t.equal(cur.targets, v.batch.optimal_yaws(model="m0", refine_pass_n=2, yaw_n=5))
    p = _policy(v)
    cur.rollout(p, 8)
    s0 = cur.state()
    g = cur.reset()
    assert t.equal(g, v.batch.optimal_yaws(model="m0", refine_pass_n=2, yaw_n=5))
    s1 = cur.state()
    assert np.array_equal(cur._cur.targets_of(s1), g.cpu().numpy())
    n = v.batch.B * v.batch.N * 8
    assert s0[:16 + n] == s1[:16 + n] and s0[16 + 2 * n:] == s1[16 + 2 * n:]          # everything but the targets
    cur.close(); p.close(); v.close()


def test_state_carries_across_calls():
    """4. One 96-step call == two 48-step calls on a twin env and curriculum, bit for bit: rewards, yaw_diff, targets, state blob."""
    from windgym_amd.curriculum import YawCurriculum
    t = _torch()
    va, vb = _venv(16, n_passthrough=0.3), _venv(16, n_passthrough=0.3)
    p = _policy(va)
    ca, cb = YawCurriculum(va, **CUR), YawCurriculum(vb, **CUR)
    oa = ca.rollout(p, 96)
    assert bool(oa["truncated"].bool().any(dim=0).all())
    halves = []
    for k in range(2):
        o = cb.rollout(p, 48, num_timesteps=k * 48 * 16)
        halves.append({key: o[key].clone() for key in ("reward", "yaw_diff", "env_reward", "curriculum_weight")})
    for key in halves[0]:
        assert t.equal(oa[key], t.cat([halves[0][key], halves[1][key]])), key
    assert not t.equal(oa["reward"], oa["env_reward"])
    assert t.equal(ca.targets, cb.targets)
    sa, sb = ca.state(), cb.state()
    assert sa == sb and len(sa) == 16 + 8 * (2 * 16 * 16 + 4 * 16) + 4 * 16 * 16
    # the blob: refused by another geometry, restored by its own
    vc = _venv(8, n_passthrough=0.3)
    cc = YawCurriculum(vc, **CUR)
    with pytest.raises(ValueError, match="16 envs x 16"):
        cc.load_state(sa)
    with pytest.raises(ValueError, match="not a curriculum state"):
        cb.load_state(b"\0" * len(sa))
    cb.rollout(p, 8)
    assert cb.state() != sa
    cb.load_state(sa)
    assert cb.state() == sa and t.equal(cb.targets, ca.targets)
    for x in (ca, cb, cc, p, va, vb, vc):
        x.close()


def test_no_op_limit_and_ppo_equals_plain_ppo():
    """5. Past curriculum_steps with reward_momentum = 0 the shaped reward IS the env reward, and PPO with such a curriculum leaves
    the parameters plain PPO leaves on a twin env."""
    from windgym_amd.curriculum import YawCurriculum
    from windgym_amd.ppo import PPO
    t = _torch()
    B, T = 16, 48
    va, vb = _venv(B, n_passthrough=0.3), _venv(B, n_passthrough=0.3)
    noop = dict(curriculum_steps=100, pure_similarity_steps=10, reward_momentum=0.0)
    cur = YawCurriculum(va, **noop)
    kw = dict(n_steps=T, n_epochs=2, ent_coef=0.001, seed=11)
    a, b = PPO("MlpPolicy", va, curriculum=cur, **kw), PPO("MlpPolicy", vb, **kw)
    assert a.curriculum is cur and b.curriculum is None
    a.num_timesteps = b.num_timesteps = 100
    out = a.collect()
    ref = b.collect()
    assert t.equal(out["reward"], out["env_reward"]) and t.equal(out["reward"], ref["reward"]) and float(out["curriculum_weight"].min()) == 1.0
    assert t.equal(out["advantage"], ref["advantage"])
    a.train(out, 3e-4, 0.2); b.train(ref, 3e-4, 0.2)
    for x in (a, b):
        x.num_timesteps += T * B
        x.learn(2 * T * B, reset_num_timesteps=False)
    assert a.iteration == b.iteration == 2 and t.equal(a.policy.params, b.policy.params)
    assert np.array_equal(a.opt.state()[0], b.opt.state()[0])
    assert "curriculum_weight" not in b.log[0] and a.log[0]["curriculum_weight"] == 1.0
    for x in (a, b):
        x.close(); x.policy.close()
    cur.close(); va.close(); vb.close()


def test_ppo_with_curriculum_equals_the_hand_written_loop():
    """6. PPO(..., curriculum=dict).learn == cur.rollout -> opt.gae -> train on a twin, bit for bit; the log carries the curriculum's
    entries and keeps the env's own reward."""
    from windgym_amd.curriculum import YawCurriculum
    from windgym_amd.ppo import PPO
    t = _torch()
    B, T = 16, 48
    va, vb = _venv(B, n_passthrough=0.3), _venv(B, n_passthrough=0.3)
    kw = dict(n_steps=T, n_epochs=2, ent_coef=0.001, seed=11)
    args = dict(curriculum_steps=2 * T * B, pure_similarity_steps=T * B // 2)
    a = PPO("MlpPolicy", va, curriculum=args, **kw)
    assert isinstance(a.curriculum, YawCurriculum) and a.curriculum.args()["curriculum_steps"] == 2 * T * B
    a.learn(2 * T * B)
    b, cb = PPO("MlpPolicy", vb, **kw), YawCurriculum(vb, **args)
    for it in range(2):
        out = cb.rollout(b.policy, T, num_timesteps=b.num_timesteps)
        b.opt.gae(out["reward"], out["value"], out["final_value"], out["truncated"], b.gamma, b.gae_lambda, out=(b._adv, b._ret))
        env_mean, env_abs = float(out["env_reward"].double().mean()), float(out["env_reward"].double().abs().mean())
        shaped_mean, w_mean, d_mean = float(out["reward"].double().mean()), float(out["curriculum_weight"].mean()), float(out["yaw_diff"].double().mean())
        b.train(out, 3e-4, 0.2)
        b.num_timesteps += T * B
        rec = a.log[it]
        assert rec["curriculum_weight"] == w_mean and rec["mean_yaw_diff"] == d_mean and 0.0 < w_mean < 1.0
        # wg_metrics sums the T * B float32 rewards in float32: at most n * 2^-24 of sum |r| away from the float64 mean, per term
        assert abs(rec["mean_step_reward"] - env_mean) <= (T * B + 4) * 2.0 ** -24 * env_abs
        assert abs(rec["mean_step_reward"] - shaped_mean) > 100 * T * B * 2.0 ** -24 * env_abs
    assert t.equal(a.policy.params, b.policy.params) and np.array_equal(a.opt.state()[0], b.opt.state()[0])
    assert a.curriculum.state() == cb.state() and t.equal(a.curriculum.targets, cb.targets)
    with pytest.raises(ValueError, match="another env"):
        PPO("MlpPolicy", va, curriculum=cb, **kw)
    for x in (a, b):
        x.close(); x.policy.close()
    cb.close(); a.curriculum.close(); va.close(); vb.close()


def test_save_load_resume_mid_ramp(tmp_path):
    """7. save mid-ramp, load on a NEW env restored from the state blob, one more iteration == the uninterrupted run: parameters,
    curriculum state, shaped rewards.  A checkpoint without a curriculum loads as before."""
    import zipfile
    from windgym_amd.ppo import PPO
    t = _torch()
    B, T = 16, 48
    kw = dict(n_steps=T, n_epochs=2, ent_coef=0.001, seed=11)
    args = dict(curriculum_steps=4 * T * B, pure_similarity_steps=T * B // 2, model="m0", refine_pass_n=3, yaw_n=5, reward_momentum=0.8)
    va, vb = _venv(B, n_passthrough=0.3), _venv(B, n_passthrough=0.3)
    a = PPO("MlpPolicy", va, curriculum=args, **kw)
    a.learn(3 * T * B)
    b = PPO("MlpPolicy", vb, curriculum=args, **kw)
    b.learn(2 * T * B)
    assert 0.0 < b.log[-1]["curriculum_weight"] < 1.0
    path = os.path.join(tmp_path, "ppo_curriculum.zip")
    b.save(path)
    with zipfile.ZipFile(path) as z:
        assert "curriculum_state.bin" in z.namelist() and z.read("curriculum_state.bin") == b.curriculum.state()
    vc = _venv(B, n_passthrough=0.3)
    vc.batch.set_state(vb.batch.get_state())
    for name in ("obs", "final_obs", "reward", "truncated"):                     # the last step's outputs live in the caller's tensors
        getattr(vc.batch, name).copy_(getattr(vb.batch, name))
    c = PPO.load(path, vc)
    assert c.curriculum.args() == b.curriculum.args() and c.curriculum.state() == b.curriculum.state()
    assert t.equal(c.curriculum.targets, b.curriculum.targets)
    c.learn(T * B, reset_num_timesteps=False)
    assert c.iteration == 3 and c.num_timesteps == a.num_timesteps
    assert t.equal(c.policy.params, a.policy.params) and c.curriculum.state() == a.curriculum.state()
    la, lc = a.curriculum.last_rollout, c.curriculum.last_rollout
    assert t.equal(la["reward"], lc["reward"]) and t.equal(la["yaw_diff"], lc["yaw_diff"]) and not t.equal(la["reward"], la["env_reward"])
    assert c.log[-1]["curriculum_weight"] == a.log[-1]["curriculum_weight"]
    # without a curriculum the checkpoint has neither the member nor the key, and loads without one
    d = PPO("MlpPolicy", vb, **kw)
    plain = os.path.join(tmp_path, "ppo_plain.zip")
    d.save(plain)
    with zipfile.ZipFile(plain) as z:
        assert "curriculum_state.bin" not in z.namelist() and b"curriculum" not in z.read("windgym_ppo.json")
    e = PPO.load(plain, vb)
    assert e.curriculum is None
    for x in (a, b, c, d, e):
        if x.curriculum is not None:
            x.curriculum.close()
        x.close(); x.policy.close()
    for v in (va, vb, vc):
        v.close()


def test_refusals():
    """9. WG_ERR_INVALID (ValueError) naming the argument; a population is NotImplementedError."""
    from windgym_amd.binding import Curriculum
    from windgym_amd.curriculum import YawCurriculum
    from windgym_amd.population import PPOPopulation
    t = _torch()
    v = _venv(4, n_passthrough=0.3)
    b = v.batch
    B, N, T = b.B, b.N, 2
    c = Curriculum(b)
    z = lambda shape, dtype=t.float32: t.zeros(shape, dtype=dtype, device=b.device)          # noqa: E731
    a = dict(yaw0=z((B, N)), actions=z((T, B, N)), yaw_after=z((T, B, N)), truncated=z((T, B), t.uint8), ep_row=z((T, B), t.int32) - 1,
             ep_target=z((1, N), t.float64), n_targets=1, weight=z((T,), t.float64), momentum=0.9, reward=z((T, B)), shaped=z((T, B)))
    c.shape(T, **a)
    clean = c.state()
    for key in ("yaw0", "actions", "yaw_after", "truncated", "ep_row", "weight", "reward", "shaped", "ep_target"):
        with pytest.raises(ValueError, match=f"{key}(_dev|_out) is null"):
            c.shape(T, **{**a, key: None})
    c.shape(T, **{**a, "ep_target": None, "n_targets": 0})                               # no new episode: no table needed
    c.shape(0, **a)                                                                      # nothing to do
    for m in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            c.shape(T, **{**a, "momentum": m})
    ptr = lambda k: a[k].data_ptr()                                                      # noqa: E731
    rc = c.L.wg_curriculum_shape(c._h, -1, ptr("yaw0"), ptr("actions"), ptr("yaw_after"), ptr("truncated"), ptr("ep_row"), ptr("ep_target"), 1,
                                 ptr("weight"), 0.9, ptr("reward"), ptr("shaped"), None, None, None)
    assert rc == -1 and b"T must be" in c.L.wg_last_error()
    with pytest.raises(ValueError, match="C must be"):
        c.shape(T, **{**a, "n_targets": -1})
    with pytest.raises(ValueError, match="CUDA tensor"):
        c.shape(T, **{**a, "reward": a["reward"].cpu()})
    c.load_state(clean)
    # an ep_row that is no row of ep_target: the kernel skips it and latches it; the next synchronising call names it, once
    bad = a["ep_row"].clone()
    bad[1, 2] = 1
    tr = a["truncated"].clone()
    tr[1, 2] = 1
    c.shape(T, **{**a, "ep_row": bad, "truncated": tr})
    with pytest.raises(ValueError, match=r"ep_row_dev\[1, 2\] = 1"):
        c.state()
    assert len(c.state()) == len(clean)
    b.check()
    with pytest.raises(NotImplementedError, match="population"):
        PPOPopulation("MlpPolicy", v, n_members=2, curriculum=dict(curriculum_steps=10, pure_similarity_steps=1))
    with pytest.raises(ValueError, match="as_torch"):
        YawCurriculum(_HostEnv(v), 10, 1)
    c.close(); v.close()


class _HostEnv:
    """a vector env that returns numpy arrays"""

    def __init__(self, v):
        self.batch, self.rollout, self.as_torch, self.num_envs = v.batch, v.rollout, False, v.num_envs
