"""Helpers of the training GPU tests (test_gpu_policy.py, test_gpu_ppo.py, test_gpu_closed_loop.py, test_gpu_multi_agent.py,
test_gpu_central_critic.py, test_gpu_population.py): the bars (the step outputs' are also test_gpu_spotcheck.py's), the policy shapes
at the kernel's limits, test policies, random minibatches, the cfg2 env, the eager-torch reference trainer, and the documented loop
of wg_rollout / wg_rollout_multi driven from Python on a twin env with the comparison of a rollout with it."""
import copy

import numpy as np

from helpers import OBS_ATOL  # noqa: F401  (the step outputs' bar against the CPU oracle)
from oracle import policy_oracle as po
from windgym_amd.policy import pack_params


# Frozen-box inflow (cfg5), with the worst error observed on an MI355X over the 16 sampled envs x 300 steps of the two cfg5 tests of
# test_gpu_spotcheck.py (small box / reference box) next to each bar; every bar was 30 to 70 times its worst case and is now 3.5 to 5
# times it:
TURB_OBS_ATOL = 8e-5                         # was 5e-4: worst 1.66e-5 / 1.57e-5
TURB_REW_RTOL, TURB_REW_ATOL = 1e-4, 8e-5    # was 1e-3, 1e-3: worst 1.68e-5 / 1.54e-5
TURB_UVW_RTOL, TURB_UVW_ATOL = 1e-4, 1.5e-3  # was 2e-3, 2e-3: worst 4.25e-4 / 4.21e-4 m/s (the wake deficits in float32, about 5e-5 of U)
TURB_POW_RTOL, TURB_POW_ATOL = 4e-4, 400.0   # was 5e-3, 2000 W: worst 113 / 117 W
N_SAMPLE = 16                                # envs of a batch the oracle replays
# policy outputs: the bars of test_gpu_policy.py's stochastic test (raw 1e-5 + 2e-5, logp 1e-4) and of its value checks
RAW_ATOL, LOGP_ATOL, VAL_ATOL, VAL_RTOL = 3e-5, 1e-4, 2e-5, 2e-5
SMALL_BOX, SMALL_BOX_SPACING = (256, 64, 32), (3.0, 3.0, 3.0)

# the limits of wg_policy.h as (n_in, hidden_pi, hidden_vf, n_out): four hidden layers of 256 (five layers with the head), 2048 inputs
# (eight full first-layer chunks), 256 / 257 inputs (a chunk of exactly one input), 128 outputs (four head tiles, a 128-term
# log-probability sum), and actor / critic stacks of different depth and width (SB3's net_arch=dict(pi=[...], vf=[...]))
DEEP = (256, 256, 256, 256)
LIMIT_SHAPES = [(256, DEEP, DEEP, 16), (2048, DEEP, DEEP, 128), (257, (64,), (64,), 3), (256, (32,), (32,), 33), (2048, (), (), 128),
                (256, (64, 64), DEEP, 16), (32, (64, 64), DEEP, 16), (256, DEEP, (64, 64), 16), (200, (128, 128, 128), (), 2),
                (32, (), (33,), 16), (160, (256,), (64, 64), 80)]


def _stack(h):
    return "x".join(map(str, h)) or "none"


def shape4(shape):
    """(n_in, hidden, n_out) of SHAPES or (n_in, hidden_pi, hidden_vf, n_out) of LIMIT_SHAPES -> the latter"""
    return shape if len(shape) == 4 else (shape[0], shape[1], shape[1], shape[2])


def shape_id(shape):
    return f"{shape[0]}-{_stack(shape[1])}-{shape[2]}" if len(shape) == 3 else f"{shape[0]}-pi{_stack(shape[1])}-vf{_stack(shape[2])}-{shape[3]}"


def _torch():
    import torch
    return torch


def close(a, b, tol=2e-5, rel=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= tol + rel * np.abs(b)))


def dev(*arrays):
    t = _torch()
    return [t.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def close_all(*xs):
    """close() of every handle given, singly or in lists"""
    for x in xs:
        for y in (x if isinstance(x, (list, tuple)) else [x]):
            y.close()


def flat_grad(desc, grads):
    return pack_params(desc, {k: v.astype(np.float32) for k, v in grads.items()}).astype(np.float64)


def make(n_in, hidden, n_out, activation="tanh", seed=3, hidden_vf="same", n_in_vf=None, draw="uniform", dtype=np.float32):
    """A policy (split when ``n_in_vf`` differs from ``n_in``; ``hidden_vf="same"``: the actor's) with every bias and log_std away
    from 0 + its state dict as ``dtype``.  ``draw``: the biases are ``uniform`` in +-0.3 or ``normal`` with sigma 0.3; a test file
    names the one its cases and bars were written for."""
    from windgym_amd.policy import MlpPolicy
    p = MlpPolicy(n_in, n_out, hidden, hidden if hidden_vf == "same" else hidden_vf, activation, seed=seed, n_in_vf=n_in_vf)
    rng = np.random.default_rng(seed + 1)
    sd = {k: v.cpu().numpy() for k, v in p.state_dict().items()}
    for k in sd:
        if k.endswith("bias") or k == "log_std":
            x = rng.uniform(-0.3, 0.3, sd[k].shape) if draw == "uniform" else 0.3 * rng.standard_normal(sd[k].shape)
            sd[k] = x.astype(np.float32)
    p.load_state_dict(sd)
    return p, {k: v.astype(dtype) for k, v in sd.items()}


def same_actor(p, sd, n_in_vf=None, hidden_vf=(64,)):
    """A policy with p's actor parameters (and log_std) and a critic of its own on ``n_in_vf`` (default: the actor's width)."""
    q, sq = make(p.n_in, p.desc["hidden_pi"], p.n_out, p.desc["activation"], seed=11, hidden_vf=hidden_vf, n_in_vf=n_in_vf)
    sq.update({k: v for k, v in sd.items() if "value_net" not in k})
    q.load_state_dict(sq)
    return q, sq


def batch(sd, n_in, n_out, n, activation, seed=0):
    """Random rows whose ratios straddle both clip bounds: logp_old = the true log-probability + N(0, 0.3)."""
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-1, 1, (n, n_in)).astype(np.float32)
    mean, value = po.forward(sd, obs, activation)
    std = np.exp(sd["log_std"])
    raw = (mean + std * rng.standard_normal((n, n_out))).astype(np.float32)
    z = (raw - mean) / std
    logp = np.sum(-0.5 * z * z - sd["log_std"] - 0.5 * np.log(2 * np.pi), axis=1)
    logp_old = (logp + 0.3 * rng.standard_normal(n)).astype(np.float32)
    adv = rng.standard_normal(n).astype(np.float32) * 2.0 + 0.5
    ret = (value + rng.standard_normal(n)).astype(np.float32)
    return obs, raw, logp_old, adv, ret


def shared_batch(sd, n_in, n_in_vf, n_out, n_env, agents, activation, seed=0):
    """Random agent rows whose ratios straddle both clip bounds + the env rows the critic reads, advantages and returns per env row."""
    rng = np.random.default_rng(seed)
    n = n_env * agents
    obs = rng.uniform(-1, 1, (n, n_in)).astype(np.float32)
    obs_vf = rng.uniform(-1, 1, (n_env, n_in_vf)).astype(np.float32)
    mean = po._net(sd, "mlp_extractor.policy_net", "action_net", obs, activation)
    value = po._net(sd, "mlp_extractor.value_net", "value_net", obs_vf, activation)[:, 0]
    std = np.exp(sd["log_std"].astype(np.float64))
    raw = (mean + std * rng.standard_normal((n, n_out))).astype(np.float32)
    z = (raw - mean) / std
    logp = np.sum(-0.5 * z * z - sd["log_std"] - 0.5 * np.log(2 * np.pi), axis=1)
    logp_old = (logp + 0.3 * rng.standard_normal(n)).astype(np.float32)
    adv = (rng.standard_normal(n_env) * 2.0 + 0.5).astype(np.float32)
    ret = (value + rng.standard_normal(n_env)).astype(np.float32)
    return obs, obs_vf, raw, logp_old, adv, ret


def _ti_farm_history_100():
    """test_gpu_parity.py's generic_ti_farm_current dict (TI and farm-level sensors on every channel) with 2turb.yaml's 100-sample wind
    speed history: a rolling mean with history_N != 1, which the running window sums cannot serve — the ring-staging k_glue."""
    from windgym_amd.presets import env1_config
    d = copy.deepcopy(env1_config())
    d["ActionMethod"] = "yaw"
    d["farm"].update(nx=3, ny=2)
    d["mes_level"].update(turb_ws=True, turb_wd=True, turb_TI=True, turb_power=True, farm_ws=True, farm_wd=True, farm_TI=True, farm_power=True)
    d["ws_mes"].update(ws_current=True, ws_rolling_mean=True, ws_history_N=100, ws_history_length=100, ws_window_length=1)
    d["wd_mes"].update(wd_current=True, wd_rolling_mean=True, wd_history_N=1, wd_history_length=8, wd_window_length=8)
    d["power_mes"].update(power_current=True, power_rolling_mean=True, power_history_N=1, power_history_length=20, power_window_length=30)
    d["yaw_mes"].update(yaw_current=True, yaw_rolling_mean=False)
    return d


def _venv(n_envs=64, **kw):
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.turbine import V80
    args = dict(yaml_dict=presets.bench_cfg2_config(), seed=77, as_torch=True, turbtype="None", n_passthrough=1, n_rotor_pts=16)
    args.update(kw)
    v = WindFarmVecEnv(V80(), n_envs, **args)
    v.reset(seed=77)
    return v


def _torch_trainer(policy, out, adv, ret, perm, bs, lr, clip, vf_coef, ent_coef, max_norm):
    """The reference trainer: torch_forward + autograd + torch.optim.Adam on a float32 copy of the parameters."""
    t = _torch()
    T = out["raw"].shape[0]
    O, N = policy.n_in, policy.n_out
    obs, raw, lpo = out["obs"][:T].reshape(-1, O), out["raw"].reshape(-1, N), out["logp"].reshape(-1)
    adv, ret = adv.reshape(-1), ret.reshape(-1)
    saved = policy.params
    w = saved.detach().clone().requires_grad_(True)
    policy.params = w
    opt = t.optim.Adam([w], lr=lr, eps=1e-5)
    try:
        for e in range(perm.shape[0]):
            for s in range(0, perm.shape[1], bs):
                i = perm[e, s:s + bs].long()
                mean, V = policy.torch_forward(obs[i])
                ls = w[-N:]
                z = (raw[i] - mean) / t.exp(ls)
                logp = (-0.5 * z * z - ls - 0.5 * float(np.log(2 * np.pi))).sum(1)
                ratio = t.exp(logp - lpo[i])
                A = adv[i]
                A = (A - A.mean()) / (A.std() + 1e-8)
                l_pi = -t.min(ratio * A, t.clamp(ratio, 1 - clip, 1 + clip) * A).mean()
                loss = l_pi + vf_coef * ((ret[i] - V) ** 2).mean() - ent_coef * (0.5 + 0.5 * float(np.log(2 * np.pi)) + ls).sum()
                opt.zero_grad()
                loss.backward()
                t.nn.utils.clip_grad_norm_([w], max_norm)
                opt.step()
    finally:
        policy.params = saved
    return w.detach()


def rollout_equals_the_loop(va, vb, p, T, rec=("power_agent", "yaw_agent"), out=None, min_trunc=None):
    """va.rollout(p, T) == the Python loop of act + step on the twin vb, bit for bit: every buffer, the handle's state, the
    persistent outputs, the step after it.  va / vb: two ``WindFarmVecEnv`` or two ``WindFarmVecEnvMulti`` in the same state.
    ``out``: va's rollout when the caller has already run it; ``min_trunc``: truncations the T steps must contain (default: one
    per env).  With a split policy (a centralised critic) ``act`` returns no value: V is ``p.value`` on the env's flat rows and
    the flat final rows, one value per env.  Returns the rollout's dict (valid until va's next rollout)."""
    t = _torch()
    B, N = va.num_envs, va.n_turb
    multi = hasattr(va, "possible_agents")            # one policy row per (env, turbine): noise row (row0 + e) * N + i
    rows, per_env = ((B, N), N) if multi else ((B,), 1)
    split = getattr(p, "split", False)
    vrows, vobs = ((B,), "flat_") if split else (rows, "")          # the critic's rows, the prefix of the observations it reads

    def current(v):
        """(key, key of its final rows) of every observation the steps write -> the env's persistent tensors of it"""
        flat = (v.batch.obs, v.batch.final_obs)
        return {("obs", "final_obs"): (v._obs, v._final_obs), ("flat_obs", "flat_final_obs"): flat} if multi else {("obs", "final_obs"): flat}

    seed, row0, counter0 = int((va.venv if multi else va)._base_seed), va._global_offset, vb._policy_steps
    if out is None:
        assert va._policy_steps == counter0
        out = va.rollout(p, T, record=rec)
    ref = {k: [] for k in ("actions", "raw", "logp", "value", "final_value", "reward", "truncated") + tuple(rec)}
    for (k, kf), (o, _) in current(vb).items():
        ref[k], ref[kf] = [o.clone()], []
    for i in range(T):
        a, raw, logp, v = p.act(ref["obs"][-1], counter=counter0 + i, seed=seed, row_offset=row0 * per_env)
        if split:
            assert v is None
            v = p.value(ref["flat_obs"][-1])
        a = a.reshape(B, N).clone()
        ref["actions"].append(a); ref["raw"].append(raw.reshape(B, N).clone())
        ref["logp"].append(logp.reshape(rows).clone()); ref["value"].append(v.reshape(vrows).clone())
        (vb.step if multi else vb.batch.step)(a)
        ref["reward"].append(vb.batch.reward.clone()); ref["truncated"].append(vb.batch.truncated.clone())
        for (k, kf), (o, f) in current(vb).items():
            ref[k].append(o.clone()); ref[kf].append(f.clone())
        for name in rec:
            ref[name].append(vb.batch.info(name))
        ref["final_value"].append(p.value(ref[vobs + "final_obs"][-1]).reshape(vrows).clone())
    vb._policy_steps = counter0 + T
    assert set(out) == set(ref)
    for k, x in ref.items():
        x = t.stack(x)
        assert out[k].shape == x.shape and t.equal(out[k], x), k
    assert tuple(out["value"].shape) == (T,) + vrows == tuple(out["final_value"].shape) and tuple(out["logp"].shape) == (T,) + rows
    n_trunc = int(out["truncated"].sum())
    assert n_trunc >= (B if min_trunc is None else min_trunc), n_trunc      # default: every env truncated and was swapped at least once
    va.batch.check(); vb.batch.check()
    assert va.batch.get_state() == vb.batch.get_state()
    assert va._policy_steps == counter0 + T
    # an env that did not truncate ended the step in the state the next one starts from
    tr = out["truncated"].bool()
    assert t.equal(out["final_value"][:-1][~tr[:-1]], out["value"][1:][~tr[:-1]])
    assert not tr[:-1].any() or not t.equal(out["final_value"][:-1][tr[:-1]], out["value"][1:][tr[:-1]])
    if multi:
        assert t.equal(out["final_obs"][~tr], out["obs"][1:][~tr])
        assert not tr.any() or not t.equal(out["final_obs"][tr], out["obs"][1:][tr])
    # the persistent outputs follow, and a step() after a rollout() continues from obs[T]
    for (k, kf), (o, f) in current(va).items():
        assert t.equal(o, out[k][T]) and t.equal(f, out[kf][T - 1]), k
    act = t.zeros((B, N), device="cuda")
    for x, y in zip(va.step(act), vb.step(act)):
        assert not t.is_tensor(x) or t.equal(x, y)               # (a WindFarmVecEnv's fifth element is its lazy info dict)
    return out


# ---- populations (test_gpu_population.py, test_gpu_recurrent_population.py) -----------------------------------------------------------
def pop_hyper(P):
    """a different value of every hyper-parameter for each of up to four members"""
    return dict(gamma=[0.99, 0.9, 0.95, 0.97][:P], gae_lambda=[0.95, 0.9, 1.0, 0.8][:P], ent_coef=[0.0, 0.01, 0.003, 0.0][:P],
                vf_coef=[0.5, 0.7, 0.4, 0.5][:P], max_grad_norm=[0.5, 0.05, 10.0, 0.5][:P], learning_rate=[3e-4, 1e-3, 0.0, 2e-3][:P],
                clip_range=[0.2, 0.1, 0.3, 0.2][:P], normalize_advantage=[True, False, True, True][:P])


def mlp_members(P, n_in=32, hidden=(64, 64), n_out=16, seed0=3):
    return [make(n_in, hidden, n_out, seed=seed0 + 7 * m, dtype=np.float64)[0] for m in range(P)]


def lstm_members(P, n_in=7, n_out=2, hidden=40, shared=False, heads=(16,), seed0=3):
    from windgym_amd.recurrent import MlpLstmPolicy
    return [MlpLstmPolicy(n_in, n_out, hidden, heads, heads, shared_lstm=shared, seed=seed0 + 7 * m) for m in range(P)]


# ---- recurrent policies against tests/lstm_bptt_twin.py ---------------------------------------------------------------------------------
def lstm_policy(spec, flat):
    """the device policy of a twin's spec with the twin's flat parameters; the two flat layouts are the same, tensor by tensor"""
    import lstm_bptt_twin as tw
    from windgym_amd.recurrent import MlpLstmPolicy, param_layout
    t = _torch()
    p = MlpLstmPolicy(spec["n_in"], spec["n_out"], spec["H"], spec["hidden_pi"], spec["hidden_vf"], spec["shared"], spec["activation"])
    assert [(k, tuple(s)) for k, s in param_layout(p.desc)] == [(k, tuple(s)) for k, s in tw.layout(spec)]
    with t.no_grad():
        p.params.copy_(t.from_numpy(np.asarray(flat, np.float32)))
    p.sync()
    return p


def dev_roll(roll):
    """a twin's rollout (tw.random_rollout) as the device tensors wg_lstm_ppo_grad / _update take"""
    keys = ("obs", "raw", "logp", "advantage", "returns", "episode_start", "lstm_state0")
    return dict(zip(keys, dev(*[roll[k] for k in keys])))
