"""The documented loop of wg_rollout / wg_rollout_multi driven from Python on a twin env, and the comparison of a rollout with it.
Shared by test_gpu_policy.py, test_gpu_closed_loop.py (every step path) and test_gpu_multi_agent.py."""


def rollout_equals_the_loop(va, vb, p, T, rec=("power_agent", "yaw_agent"), out=None, min_trunc=None):
    """va.rollout(p, T) == the Python loop of act + step on the twin vb, bit for bit: every buffer, the handle's state, the
    persistent outputs, the step after it.  va / vb: two ``WindFarmVecEnv`` or two ``WindFarmVecEnvMulti`` in the same state.
    ``out``: va's rollout when the caller has already run it; ``min_trunc``: truncations the T steps must contain (default: one
    per env).  Returns the rollout's dict (valid until va's next rollout)."""
    import torch as t
    B, N = va.num_envs, va.n_turb
    multi = hasattr(va, "possible_agents")            # one policy row per (env, turbine): noise row (row0 + e) * N + i
    rows, per_env = ((B, N), N) if multi else ((B,), 1)

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
        a = a.reshape(B, N).clone()
        ref["actions"].append(a); ref["raw"].append(raw.reshape(B, N).clone())
        ref["logp"].append(logp.reshape(rows).clone()); ref["value"].append(v.reshape(rows).clone())
        (vb.step if multi else vb.batch.step)(a)
        ref["reward"].append(vb.batch.reward.clone()); ref["truncated"].append(vb.batch.truncated.clone())
        for (k, kf), (o, f) in current(vb).items():
            ref[k].append(o.clone()); ref[kf].append(f.clone())
        for name in rec:
            ref[name].append(vb.batch.info(name))
        ref["final_value"].append(p.value(ref["final_obs"][-1]).reshape(rows).clone())
    vb._policy_steps = counter0 + T
    assert set(out) == set(ref)
    for k, x in ref.items():
        x = t.stack(x)
        assert out[k].shape == x.shape and t.equal(out[k], x), k
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
