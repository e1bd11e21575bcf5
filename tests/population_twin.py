"""Twins of a population built ONLY from single-policy entries: the loop of P ``MlpPolicy.act`` calls on the members' row ranges
(what one population launch must equal) and one PPO iteration per member on contiguous copies of its columns.  Shared by
test_gpu_population.py's tests."""


class MemberLoop:
    """``act`` / ``value`` of :class:`windgym_amd.population.Population`, as P single calls on slices."""

    def __init__(self, members):
        self.members, self.P = list(members), len(members)
        self.n_in, self.n_out = members[0].n_in, members[0].n_out

    def _per(self, x, m, n):
        return x[m] if isinstance(x, (list, tuple)) else n

    def act(self, obs, deterministic=False, counter=0, *, seed=None, row_offset=0, value=True):
        import torch as t
        rows = obs.reshape(-1, self.n_in)
        Bm = rows.shape[0] // self.P
        outs = []
        for m, p in enumerate(self.members):
            sd = p.seed if seed is None else seed[m] if isinstance(seed, (list, tuple)) else seed
            ro = row_offset[m] if isinstance(row_offset, (list, tuple)) else row_offset + m * Bm
            o = p.act(rows[m * Bm:(m + 1) * Bm].contiguous(), deterministic=deterministic, counter=counter, seed=sd, row_offset=ro, value=value)
            outs.append([None if x is None else x.clone() for x in o])
        return tuple(None if outs[0][i] is None else t.cat([o[i] for o in outs]) for i in range(4))

    def value(self, obs):
        import torch as t
        rows = obs.reshape(-1, self.n_in)
        Bm = rows.shape[0] // self.P
        return t.cat([p.value(rows[m * Bm:(m + 1) * Bm].contiguous()).clone() for m, p in enumerate(self.members)])


def twin_rollout(venv, loop, T, deterministic=False):
    """wg_rollout's documented loop on ``venv`` with ``loop`` (a :class:`MemberLoop`) in the policy's place -> the buffers."""
    import torch as t
    B, N = venv.num_envs, venv.n_turb
    seed, row0, c0 = int(venv._base_seed), venv._global_offset, venv._policy_steps
    ref = {k: [] for k in ("actions", "raw", "logp", "value", "final_value", "reward", "truncated", "final_obs")}
    ref["obs"] = [venv.batch.obs.clone()]
    for i in range(T):
        a, raw, logp, v = loop.act(ref["obs"][-1], deterministic=deterministic, counter=c0 + i, seed=seed, row_offset=row0)
        ref["actions"].append(a.reshape(B, N)); ref["raw"].append(raw.reshape(B, N)); ref["logp"].append(logp); ref["value"].append(v)
        venv.batch.step(ref["actions"][-1].contiguous())
        ref["reward"].append(venv.batch.reward.clone()); ref["truncated"].append(venv.batch.truncated.clone())
        ref["obs"].append(venv.batch.obs.clone()); ref["final_obs"].append(venv.batch.final_obs.clone())
        ref["final_value"].append(loop.value(ref["final_obs"][-1]))
    venv._policy_steps = c0 + T
    return {k: t.stack(x) for k, x in ref.items()}


def twin_train(opts, out, gens, n_epochs, batch_size, hyper, lr, clip):
    """One PPO update per member from existing entries: wg_gae and wg_ppo_update on CONTIGUOUS copies of the member's columns
    of ``out [T, B, ..]`` with permutations of its own rows.  ``hyper[m]``: the member's PPO arguments.  -> per-member stats."""
    import torch as t
    P = len(opts)
    T, B = out["reward"].shape
    Bm = B // P
    stats = []
    for m, opt in enumerate(opts):
        c = slice(m * Bm, (m + 1) * Bm)
        col = {k: out[k][:T, c].contiguous() for k in ("obs", "raw", "logp", "value", "final_value", "reward", "truncated")}
        h = hyper[m]
        adv, ret = opt.gae(col["reward"], col["value"], col["final_value"], col["truncated"], h["gamma"], h["gae_lambda"])
        n = T * Bm
        perm = t.stack([t.randperm(n, generator=gens[m], device="cuda") for _ in range(n_epochs)]).to(t.int32).contiguous()
        p = opt.policy
        stats.append(opt.update(col["obs"].view(-1, p.n_in), col["raw"].view(-1, p.n_out), col["logp"].view(-1), adv.view(-1), ret.view(-1),
                                perm, batch_size, clip_range=clip[m], vf_coef=h["vf_coef"], ent_coef=h["ent_coef"],
                                normalize_advantage=h["normalize_advantage"], learning_rate=lr[m], max_grad_norm=h["max_grad_norm"]).clone())
    return stats
