"""Recurrent policies on the device (k_lstm + k_policy, wg_rollout_lstm, recurrent.MlpLstmPolicy) against the float64 twin
tests/lstm_twin.py, their bit properties, the closed loop against its documented loop, the predict protocol, evaluation, refusals.

Bar of the by-value checks: ``4 * e32 + 2e-5``, where ``e32`` is the worst absolute error, against the twin, of torch's own float32
CPU modules (``torch.nn.LSTM``, ``F.linear``) on the same inputs — computed per case, from the reference side only.  Two float32
implementations with different summation orders can sit ``2 * e32`` apart, the device's tanhf / expf differ from the host's (a
further factor 2), and 2e-5 is the project's value bar (rl_helpers.VAL_ATOL) as the floor.  logp keeps the project's 1e-4.  Every
case prints its worst device error next to e32 (profiles/r19_lstm_errors.txt holds a run's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lstm_twin as tw
from oracle import policy_oracle as po
from rl_helpers import LOGP_ATOL, VAL_ATOL, _torch, _venv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n_in, H, rows): odd K, H below / not a multiple of / equal to a tile, the chunk boundary (257 + 64 = one chunk + 65), both limits,
# partial row tiles and more than one workgroup
CELL_CASES = [(3, 1, 1), (8, 32, 33), (7, 40, 31), (257, 64, 389), (300, 256, 33), (2048, 256, 32)]


def make(n_in, n_out, H, hidden_pi=(32,), hidden_vf=(32,), shared=False, seed=3):
    """A recurrent policy with every bias and log_std away from 0 + its state dict (float32 numpy)."""
    from windgym_amd.recurrent import MlpLstmPolicy
    p = MlpLstmPolicy(n_in, n_out, H, hidden_pi, hidden_vf, shared_lstm=shared, seed=seed)
    rng = np.random.default_rng(seed + 1)
    sd = {k: v.cpu().numpy() for k, v in p.state_dict().items()}
    for k in sd:
        if (k.endswith("bias") or k == "log_std") and not k.startswith("lstm_"):
            sd[k] = rng.uniform(-0.3, 0.3, sd[k].shape).astype(np.float32)
    p.load_state_dict(sd)
    return p, sd


def dev(a, dtype=None):
    t = _torch()
    return t.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


def torch32_step(sd, x, state, start, eps=None):
    """torch's float32 CPU modules on the same inputs: nn.LSTM one step (state masked by 1 - start, sb3-contrib's way), F.linear MLPs
    -> (dict(raw, value), new state) as float32 numpy"""
    t = _torch()
    F = t.nn.functional
    nets = tw.n_nets(sd)
    n_in, H = sd["lstm_actor.weight_ih_l0"].shape[1], sd["lstm_actor.weight_hh_l0"].shape[1]
    tt = {k: t.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()}
    keep = t.from_numpy(1.0 - np.asarray(start, np.float32)).reshape(1, -1, 1)
    st = t.from_numpy(np.asarray(state, np.float32))
    hs, new = [], []
    with t.no_grad():
        for i, net in enumerate(tw.NETS[:nets]):
            m = t.nn.LSTM(n_in, H)
            m.load_state_dict({k: tt[f"{net}.{k}"] for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
            y, (h1, c1) = m(t.from_numpy(np.asarray(x, np.float32))[None], (st[i, 0][None] * keep, st[i, 1][None] * keep))
            hs.append(y[0]); new.append(t.stack([h1[0], c1[0]]))

        def mlp(prefix, head, v):
            i = 0
            while f"{prefix}.{i}.weight" in tt:
                v = t.tanh(F.linear(v, tt[f"{prefix}.{i}.weight"], tt[f"{prefix}.{i}.bias"]))
                i += 2
            return F.linear(v, tt[head + ".weight"], tt[head + ".bias"])

        mean = mlp("mlp_extractor.policy_net", "action_net", hs[0])
        value = mlp("mlp_extractor.value_net", "value_net", hs[-1])[:, 0]
        raw = mean if eps is None else mean + t.exp(tt["log_std"]) * t.from_numpy(np.asarray(eps, np.float32))
    return dict(raw=raw.numpy(), value=value.numpy()), t.stack(new).numpy()


def err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("n_in,H,rows,shared", [c + (False,) for c in CELL_CASES] + [(7, 40, 31, True)],
                         ids=[f"{a}-{b}-{c}" for a, b, c in CELL_CASES] + ["7-40-31-shared"])
def test_cell_by_value(n_in, H, rows, shared):
    """one step from a random state with a random start mask, both nets, against the twin"""
    p, sd = make(n_in, 3, H, shared=shared)
    rng = np.random.default_rng(n_in + H + rows)
    x = rng.uniform(-1, 1, (rows, n_in)).astype(np.float32)
    state = rng.uniform(-1, 1, (p.nets, 2, rows, H)).astype(np.float32)
    start = (rng.random(rows) < 0.3).astype(np.uint8)
    ref, ref_state = tw.step(sd, x, state, start)
    f32, f32_state = torch32_step(sd, x, state, start)
    e32 = max(err(f32_state, ref_state), err(f32["raw"], ref["raw"]), err(f32["value"], ref["value"]))
    (a, raw, logp, v), new = p.act(dev(x), dev(state), dev(start), deterministic=True)
    got = dict(state=err(new.cpu().numpy(), ref_state), raw=err(raw.cpu().numpy(), ref["raw"]), value=err(v.cpu().numpy(), ref["value"]))
    bar = 4 * e32 + VAL_ATOL
    print(f"lstm cell n_in={n_in} H={H} rows={rows} shared={shared}: e32={e32:.3e} bar={bar:.3e} device " +
          " ".join(f"{k}={e:.3e}" for k, e in got.items()))
    assert np.isfinite(new.cpu().numpy()).all()
    assert max(got.values()) <= bar, got
    assert np.array_equal(a.cpu().numpy(), np.clip(raw.cpu().numpy(), -1, 1))
    p.close()


def test_sequence_by_value():
    """T = 64 stochastic steps threaded through the device state, starts sprinkled: h, c, action, logp, value against the twin"""
    n_in, H, rows, T, n_out = 8, 64, 33, 64, 4
    p, sd = make(n_in, n_out, H)
    rng = np.random.default_rng(11)
    state = p.initial_state(rows)
    ref_state, f32_state = np.zeros((2, 2, rows, H)), np.zeros((2, 2, rows, H), np.float32)
    e32, worst = 0.0, dict(state=0.0, raw=0.0, action=0.0, value=0.0, logp=0.0)
    for s in range(T):
        x = rng.uniform(-1, 1, (rows, n_in)).astype(np.float32)
        start = (rng.random(rows) < 0.08).astype(np.uint8)
        eps = po.policy_noise(5, 100 + s, 7 + np.arange(rows), n_out)
        ref, ref_state = tw.step(sd, x, ref_state, start, eps=eps)
        f32, f32_state = torch32_step(sd, x, f32_state, start, eps=eps)
        e32 = max(e32, err(f32_state, ref_state), err(f32["raw"], ref["raw"]), err(f32["value"], ref["value"]))
        (a, raw, logp, v), state = p.act(dev(x), state, dev(start), counter=100 + s, seed=5, row_offset=7, state_out=state)
        for k, g, r in (("state", state, ref_state), ("raw", raw, ref["raw"]), ("action", a, ref["action"]), ("value", v, ref["value"]),
                        ("logp", logp, ref["logp"])):
            worst[k] = max(worst[k], err(g.cpu().numpy(), r))
    bar = 4 * e32 + VAL_ATOL
    print(f"lstm sequence T={T} n_in={n_in} H={H} rows={rows}: e32={e32:.3e} bar={bar:.3e} device " + " ".join(f"{k}={e:.3e}" for k, e in worst.items()))
    assert max(worst[k] for k in ("state", "raw", "action", "value")) <= bar, worst
    assert worst["logp"] <= LOGP_ATOL, worst
    p.close()


def test_bit_properties():
    t = _torch()
    n_in, H, rows = 20, 40, 389
    p, sd = make(n_in, 3, H)
    rng = np.random.default_rng(4)
    x = dev(rng.uniform(-1, 1, (rows, n_in)).astype(np.float32))
    state = dev(rng.uniform(-1, 1, (2, 2, rows, H)).astype(np.float32))
    start_np = (rng.random(rows) < 0.3).astype(np.uint8)
    start_np[:4] = (1, 0, 1, 0)
    start = dev(start_np)

    def act(x, state, start, **kw):
        (a, raw, logp, v), new = p.act(x, state, start, counter=3, seed=9, **kw)
        return [y.clone() for y in (a, raw, logp, v, new)]

    full = act(x, state, start)
    # run to run
    assert all(t.equal(a, b) for a, b in zip(full, act(x, state, start)))
    # rows 100:200 alone == the same rows of the full batch
    part = act(x[100:200].contiguous(), state[:, :, 100:200].contiguous(), start[100:200].contiguous(), row_offset=100)
    assert all(t.equal(a[100:200], b) for a, b in zip(full[:4], part)) and t.equal(full[4][:, :, 100:200], part[4])
    # a start = 1 row == the zero-state row; also where its incoming state is NaN
    fresh = t.from_numpy(start_np != 0).cuda()
    zero = state.clone(); zero[:, :, fresh] = 0.0
    nan = state.clone(); nan[:, :, fresh] = float("nan")
    none = act(x, zero, None)
    got_nan = act(x, nan, start)
    for a, b, c in zip(full, none, got_nan):
        sel = (lambda y: y[:, :, fresh]) if a.ndim == 4 else (lambda y: y[fresh])
        assert t.equal(sel(a), sel(b)) and t.equal(sel(a), sel(c))
    assert all(t.isfinite(y).all() for y in got_nan) and all(t.equal(a, b) for a, b in zip(full, got_nan))
    # state_out aliasing state_in == not aliasing
    inplace = state.clone()
    alias = act(x, inplace, start, state_out=inplace)
    assert all(t.equal(a, b) for a, b in zip(full, alias)) and t.equal(inplace, full[4])
    # net mask: the critic alone == the critic of the two-net call; the actor alone (value=False) leaves the critic's planes alone
    from windgym_amd.binding import LSTM_CRITIC
    h_vf, h2 = t.zeros((rows, H), device="cuda"), t.zeros((2, rows, H), device="cuda")
    out1 = t.full_like(state, 7.0)
    p._chk(p.L.wg_lstm_step(p._lstm, rows, x.data_ptr(), start.data_ptr(), state.data_ptr(), out1.data_ptr(), None, h_vf.data_ptr(), LSTM_CRITIC,
                            p._stream()), "wg_lstm_step")
    assert t.equal(out1[1], full[4][1]) and t.equal(h_vf, full[4][1, 0]) and bool((out1[0] == 7.0).all())
    out2 = t.full_like(state, 7.0)
    (a, raw, logp, v), new = p.act(x, state, start, counter=3, seed=9, value=False, state_out=out2)
    assert v is None and t.equal(a, full[0]) and t.equal(logp, full[2]) and t.equal(out2[0], full[4][0]) and bool((out2[1] == 7.0).all())
    # state_out NULL: h' alone, the state untouched
    keep = state.clone()
    p._chk(p.L.wg_lstm_step(p._lstm, rows, x.data_ptr(), start.data_ptr(), state.data_ptr(), None, h2[0].data_ptr(), h2[1].data_ptr(), 0,
                            p._stream()), "wg_lstm_step")
    assert t.equal(state, keep) and t.equal(h2[0], full[4][0, 0]) and t.equal(h2[1], full[4][1, 0])
    # torch_forward is the same model
    mean, value, new = p.torch_forward(x, state, start)
    det = p.act(x, state, start, deterministic=True)
    assert err(mean.cpu().numpy(), det[0][1].cpu().numpy()) < 1e-4 and err(new.cpu().numpy(), det[1].cpu().numpy()) < 1e-4
    p.close()


def _loop(vb, p, T, state, start, rec):
    """wg_rollout_lstm's documented loop from Python on the twin env -> dict of stacked buffers, the final state"""
    t = _torch()
    B, N = vb.num_envs, vb.n_turb
    seed, row0, counter0 = int(vb._base_seed), vb._global_offset, vb._policy_steps
    ref = {k: [] for k in ("actions", "raw", "logp", "value", "final_value", "reward", "truncated", "final_obs") + tuple(rec)}
    ref["obs"], ref["episode_start"] = [vb.batch.obs.clone()], [start.clone()]
    state = state.clone()
    fin_scratch = t.zeros((2, B, p.H), device="cuda")
    for i in range(T):
        (a, raw, logp, v), state = p.act(ref["obs"][-1], state, ref["episode_start"][-1], counter=counter0 + i, seed=seed, row_offset=row0,
                                         state_out=state)
        a = a.reshape(B, N).clone()
        ref["actions"].append(a); ref["raw"].append(raw.clone()); ref["logp"].append(logp.clone()); ref["value"].append(v.clone())
        vb.batch.step(a)
        ref["reward"].append(vb.batch.reward.clone()); ref["truncated"].append(vb.batch.truncated.clone())
        ref["obs"].append(vb.batch.obs.clone()); ref["final_obs"].append(vb.batch.final_obs.clone())
        ref["episode_start"].append(vb.batch.truncated.clone())
        for name in rec:
            ref[name].append(vb.batch.info(name))
        # the critic on (final_obs, the state after the step, no start), that state discarded: act() into a scratch state
        (_, _, _, fv), _ = p.act(ref["final_obs"][-1], state, None, deterministic=True, state_out=t.zeros_like(state))
        ref["final_value"].append(fv.clone())
    vb._policy_steps = counter0 + T
    return {k: t.stack(x) for k, x in ref.items()}, state


@pytest.mark.parametrize("shared", [False, True], ids=["two_lstms", "shared_lstm"])
def test_rollout_equals_its_documented_loop(shared):
    t = _torch()
    va, vb = _venv(), _venv()
    B, O, N, T, rec = va.num_envs, va.batch.obs_dim, va.n_turb, 300, ("power_agent", "yaw_agent")
    p, sd = make(O, N, 48, (64, 64), (64, 64), shared=shared)
    out = va.rollout(p, T, record=rec)
    ref, ref_state = _loop(vb, p, T, p.initial_state(B), t.ones(B, dtype=t.uint8, device="cuda"), rec)
    assert set(out) == set(ref) | {"lstm_state", "lstm_state0"}
    for k, x in ref.items():
        assert out[k].shape == x.shape and t.equal(out[k], x), k
    assert t.equal(out["lstm_state"], ref_state) and not bool(out["lstm_state0"].any())
    tr = out["truncated"].bool()
    assert int(tr.sum()) >= B                                  # every env truncated at least once
    assert t.equal(out["episode_start"][1:], out["truncated"]) and bool((out["episode_start"][0] == 1).all())
    va.batch.check(); vb.batch.check()
    assert va.batch.get_state() == vb.batch.get_state() and va._policy_steps == vb._policy_steps == T
    # an env that did not truncate ended the step in the state (env and LSTM) the next step starts from
    same = ~tr[:-1] & (out["final_obs"][:-1] == out["obs"][1:-1]).all(-1)
    assert bool(same.any()) and t.equal(out["final_value"][:-1][same], out["value"][1:][same])
    assert not t.equal(out["final_value"][:-1][tr[:-1]], out["value"][1:][tr[:-1]])
    # on truncated rows final_value is the twin's bootstrap from the pre-reset LSTM state: replay the recorded inputs in float64
    # (and, for the bar, in torch's float32 CPU modules: e32 as in the by-value tests)
    state, state32 = np.zeros((p.nets, 2, B, p.H)), np.zeros((p.nets, 2, B, p.H), np.float32)
    obs, fin, es = (out[k].cpu().numpy() for k in ("obs", "final_obs", "episode_start"))
    fv, trn, worst, e32 = out["final_value"].cpu().numpy(), tr.cpu().numpy(), 0.0, 0.0
    for i in range(T):
        state = tw.lstm_step(sd, obs[i], state, es[i])
        _, state32 = torch32_step(sd, obs[i], state32, es[i])
        if trn[i].any():
            want = tw.final_value(sd, fin[i][trn[i]], state[:, :, trn[i]])
            f32, _ = torch32_step(sd, fin[i][trn[i]], state32[:, :, trn[i]], np.zeros(int(trn[i].sum())))
            e32, worst = max(e32, err(f32["value"], want)), max(worst, err(fv[i][trn[i]], want))
    print(f"lstm rollout shared={shared}: final_value on truncated rows e32={e32:.3e} bar={4 * e32 + VAL_ATOL:.3e} device {worst:.3e}")
    assert worst <= 4 * e32 + VAL_ATOL
    # rollout(T1) then rollout(T2) == rollout(T1 + T2); the kept state continues, and the step after
    state_T, es_T = out["lstm_state"].clone(), out["episode_start"][T].clone()
    o1 = {k: v.clone() for k, v in va.rollout(p, 7).items()}
    assert t.equal(o1["lstm_state0"], state_T) and t.equal(o1["episode_start"][0], es_T)
    o2 = va.rollout(p, 5)
    r12, _ = _loop(vb, p, 12, state_T, es_T, ())
    for k in r12:
        assert t.equal(t.cat([o1[k][:7], o2[k]]), r12[k]), k          # (obs / episode_start: slot 7 of the first is slot 0 of the second)
    act = t.zeros((B, N), device="cuda")
    for x, y in zip(va.step(act), vb.step(act)):
        assert not t.is_tensor(x) or t.equal(x, y)
    # reset() marks every env as an episode start; state= overrides the kept state
    va.reset(seed=5)
    o3 = va.rollout(p, 2, state=state_T)
    assert bool((o3["episode_start"][0] == 1).all()) and t.equal(o3["lstm_state0"], state_T)
    va.close(); vb.close(); p.close()


def test_predict_protocol():
    n_in, H, B, n_out = 8, 32, 5, 4
    p, sd = make(n_in, n_out, H)
    rng = np.random.default_rng(6)
    x1, x2 = (rng.uniform(-1, 1, (B, n_in)).astype(np.float32) for _ in range(2))
    a1, s1 = p.predict(x1, deterministic=True)
    assert isinstance(a1, np.ndarray) and a1.shape == (B, n_out) and a1.dtype == np.float32
    assert isinstance(s1, tuple) and all(s.shape == (1, B, H) and s.dtype == np.float32 for s in s1)
    start = np.array([0, 1, 0, 0, 1], bool)
    a2, s2 = p.predict(x2, state=s1, episode_start=start, deterministic=True)
    r1, st = tw.step(sd, x1, np.zeros((2, 2, B, H)))
    r2, st2 = tw.step(sd, x2, st, start)
    assert err(a1, r1["action"]) <= 3e-5 and err(a2, r2["action"]) <= 3e-5
    assert err(s2[0][0], st2[0, 0]) <= 3e-5 and err(s2[1][0], st2[0, 1]) <= 3e-5
    a0, s0 = p.predict(x2, deterministic=True)                   # without the state the answer differs: it is threaded
    assert not np.array_equal(a0[~start], a2[~start]) and np.array_equal(a0[start], a2[start])
    a, s = p.predict(x1[0], deterministic=True)
    assert a.shape == (n_out,) and s[0].shape == (1, 1, H) and np.array_equal(a, a1[0])
    with pytest.raises(ValueError, match="state must be"):
        p.predict(x1, state=(s1[0][:, :2], s1[1][:, :2]))
    p.close()


class _PredictOnly:
    """Forwards predict() only: eval_sweep then takes the host loop."""

    def __init__(self, p):
        self._p = p

    def predict(self, obs, state=None, episode_start=None, deterministic=False):
        return self._p.predict(obs, state=state, episode_start=episode_start, deterministic=deterministic)


def test_eval_sweep_device_path_equals_host_loop():
    from windgym_amd import presets
    from windgym_amd.evaluate import eval_sweep
    from windgym_amd.turbine import V80
    p, _ = make(8, 4, 24)
    kw = dict(yaml_dict=presets.env1_config(), winddirs=(260.0, 270.0, 280.0), windspeeds=(8.0, 11.0), t_sim=40, turbtype="Random", seed=1)
    dev_ds = eval_sweep(V80(), None, p, **kw)
    host = eval_sweep(V80(), None, _PredictOnly(p), **kw)
    dd, hd = (d["data"] if isinstance(d, dict) else {k: d[k].values for k in d.data_vars} for d in (dev_ds, host))
    assert set(dd) == set(hd)
    for k in hd:
        assert np.array_equal(dd[k], hd[k]), k
    assert np.any(dd["yaw_a"][-1] != dd["yaw_a"][0])

    class Memoryless(_PredictOnly):          # the state thrown away: a recurrent model must NOT evaluate like this
        def predict(self, obs, deterministic=False):
            return self._p.predict(obs, deterministic=deterministic)

    lost = eval_sweep(V80(), None, Memoryless(p), **kw)
    ld = lost["data"] if isinstance(lost, dict) else {k: lost[k].values for k in lost.data_vars}
    assert not np.array_equal(ld["yaw_a"], dd["yaw_a"])
    p.close()


def test_argument_errors_and_refusals():
    from windgym_amd.curriculum import YawCurriculum
    from windgym_amd.envs import WindFarmVecEnvMulti
    from windgym_amd.normalize import VecNormalize
    from windgym_amd.policy import MlpPolicy
    from windgym_amd.population import PPOPopulation
    from windgym_amd.ppo import PPO
    from windgym_amd.recurrent import MlpLstmPolicy
    t = _torch()
    with pytest.raises(NotImplementedError, match="2048"):
        MlpLstmPolicy(4096, 4)
    with pytest.raises(NotImplementedError, match="256"):
        MlpLstmPolicy(8, 4, 512)
    v = _venv(8)
    O, N = v.batch.obs_dim, v.n_turb
    p, _ = make(O, N, 16)
    x, st = t.zeros((8, O), device="cuda"), p.initial_state(8)
    with pytest.raises(ValueError, match="obs must be"):
        p.act(t.zeros((8, O + 1), device="cuda"), st)
    with pytest.raises(ValueError, match="state must be"):
        p.act(x, p.initial_state(7))
    with pytest.raises(ValueError, match="episode_start must be"):
        p.act(x, st, t.zeros(8, device="cuda"))
    with pytest.raises(ValueError, match="net_mask"):          # a shared LSTM has no critic net
        q, _ = make(O, N, 16, shared=True)
        q._chk(q.L.wg_lstm_step(q._lstm, 8, x.data_ptr(), None, q.initial_state(8).data_ptr(), None, None, None, 2, q._stream()), "wg_lstm_step")
    with pytest.raises(ValueError, match="state_in_dev"):
        p._chk(p.L.wg_lstm_step(p._lstm, 8, x.data_ptr(), None, None, None, None, None, 0, p._stream()), "wg_lstm_step")
    with pytest.raises(ValueError, match="parameters given"):
        p._chk(p.L.wg_lstm_set_params(p._lstm, p.params.data_ptr(), 5, 1, p._stream()), "wg_lstm_set_params")
    # wg_rollout_lstm: shapes between lstm, p and the handle
    small, _ = make(O + 1, N, 16)
    with pytest.raises(ValueError, match="policy maps"):
        v.rollout(small, 4)
    wrong = MlpPolicy(O, N, (16,), (16,))                       # an MLP that does not read the LSTM's hidden rows behind p's LSTM
    keep, p.mlp = p.mlp, wrong
    try:
        with pytest.raises(ValueError, match="hidden"):
            v.rollout(p, 4)
    finally:
        p.mlp = keep
    with pytest.raises(ValueError, match="state must be"):
        v.rollout(p, 4, state=p.initial_state(3))
    with pytest.raises(ValueError, match="recurrent"):
        v.rollout(wrong, 4, state=st)
    for call, who in ((lambda: PPO(p, v), "PPO"), (lambda: PPOPopulation([p, p], v), "PPOPopulation"),
                      (lambda: VecNormalize(v).rollout(p, 4), "VecNormalize"), (lambda: YawCurriculum.rollout(None, p, 4), "YawCurriculum")):
        with pytest.raises(NotImplementedError, match="training / wrapping a recurrent policy"):
            call()
    with pytest.raises(NotImplementedError, match="recurrent"):
        WindFarmVecEnvMulti.rollout(None, p, 4)
    v.close(); p.close(); q.close(); small.close(); wrong.close()


def test_bench_policy_cli_reports_the_lstm_legs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_policy.py"), "--envs", "256", "--api-steps", "100",
                        "--preroll", "20", "--lstm", "64"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    api = json.loads(lines[0])
    for leg in ("abi", "rollout_hip_policy", "lstm_closed_loop_torch_policy", "lstm_closed_loop_hip_policy", "lstm_rollout_hip_policy"):
        assert api[leg]["value"] > 0, leg
    assert api["lstm_policy"]["lstm_hidden_size"] == 64
