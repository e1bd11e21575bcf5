"""Twins of a population of recurrent policies built ONLY from single-policy entries: the loop of P ``MlpLstmPolicy.act`` calls on the
members' rows and states (what one population launch must equal), wg_rollout_lstm's documented loop with that loop in the policy's
place, and wg_lstm_pop_update / wg_lstm_ppo_update through the same arguments.  Shared by
test_gpu_recurrent_population.py's tests.  TEST INFRASTRUCTURE."""
import ctypes as C

COLUMNS = ("obs", "raw", "logp", "advantage", "returns", "episode_start")        # [T (+ 1), B, ..] entries of a recurrent rollout


def _torch():
    import torch
    return torch


class LstmMemberLoop:
    """``act`` of :class:`windgym_amd.recurrent_population.RecurrentPopulation`, as P single calls on slices; ``state`` is the
    population's ``[P, nets, 2, Bm, H]``."""

    def __init__(self, members):
        self.members, self.P = list(members), len(members)

    def act(self, obs, state, episode_start=None, deterministic=False, counter=0, *, seed=None, row_offset=0, value=True):
        t = _torch()
        Bm = obs.shape[0] // self.P
        outs, new = [], []
        for m, p in enumerate(self.members):
            r = slice(m * Bm, (m + 1) * Bm)
            sd = p.seed if seed is None else seed[m] if isinstance(seed, (list, tuple)) else seed
            ro = row_offset[m] if isinstance(row_offset, (list, tuple)) else row_offset + m * Bm
            es = None if episode_start is None else episode_start[r].contiguous()
            o, s = p.act(obs[r].contiguous(), state[m].contiguous(), es, deterministic=deterministic, counter=counter, seed=sd, row_offset=ro,
                         value=value)
            outs.append([None if x is None else x.clone() for x in o])
            new.append(s.clone())
        return tuple(None if outs[0][i] is None else t.cat([o[i] for o in outs]) for i in range(4)), t.stack(new)


def twin_rollout(vb, loop, T, state, start, deterministic=False, rec=()):
    """wg_rollout_lstm's documented loop on ``vb`` with ``loop`` (a :class:`LstmMemberLoop`) in the pair's place -> (the buffers, the
    final state ``[P, nets, 2, Bm, H]``)."""
    t = _torch()
    B, N = vb.num_envs, vb.n_turb
    seed, row0, c0 = int(vb._base_seed), vb._global_offset, vb._policy_steps
    ref = {k: [] for k in ("actions", "raw", "logp", "value", "final_value", "reward", "truncated", "final_obs") + tuple(rec)}
    ref["obs"], ref["episode_start"] = [vb.batch.obs.clone()], [start.clone()]
    state = state.clone()
    for i in range(T):
        (a, raw, logp, v), state = loop.act(ref["obs"][-1], state, ref["episode_start"][-1], deterministic, counter=c0 + i, seed=seed,
                                            row_offset=row0)
        a = a.reshape(B, N).clone()
        ref["actions"].append(a); ref["raw"].append(raw.reshape(B, N)); ref["logp"].append(logp); ref["value"].append(v)
        vb.batch.step(a)
        ref["reward"].append(vb.batch.reward.clone()); ref["truncated"].append(vb.batch.truncated.clone())
        ref["obs"].append(vb.batch.obs.clone()); ref["final_obs"].append(vb.batch.final_obs.clone())
        ref["episode_start"].append(vb.batch.truncated.clone())
        for name in rec:
            ref[name].append(vb.batch.info(name))
        # the critic on (final_obs, the state after the step, no start), that state left as it is
        (_, _, _, fv), _ = loop.act(ref["final_obs"][-1], state, None, True)
        ref["final_value"].append(fv)
    vb._policy_steps = c0 + T
    return {k: t.stack(x) for k, x in ref.items()}, state


def pop_update(pop, roll, perm, envs_per_batch, hyper, stats=None):
    """wg_lstm_pop_update through the ABI: ``roll`` the whole rollout's dict (device tensors, ``lstm_state0`` in the population's
    layout), ``perm`` int32 ``[P, E, Bm]`` of GLOBAL env ids, ``hyper``: dict of per-member lists (clip_range, vf_coef, ent_coef,
    normalize_advantage, learning_rate, max_grad_norm) -> stats ``[P, E, n_mb, 8]``."""
    from windgym_amd.binding import CLstmPpoBatch, CPpoHyper
    t = _torch()
    P, E, Bm = perm.shape
    T, B = roll["raw"].shape[:2]
    n_mb = -(-Bm // envs_per_batch)
    st = t.zeros((P, E, n_mb, 8), dtype=t.float32, device="cuda") if stats is None else stats
    b = CLstmPpoBatch(*[roll[k].data_ptr() for k in COLUMNS], roll["lstm_state0"].data_ptr(), int(T), int(B))
    hp = (CPpoHyper * P)(*[CPpoHyper(float(hyper["clip_range"][m]), float(hyper["vf_coef"][m]), float(hyper["ent_coef"][m]),
                                     int(bool(hyper["normalize_advantage"][m]))) for m in range(P)])
    f = lambda xs: (C.c_float * P)(*[float(x) for x in xs])        # noqa: E731
    params = (C.c_void_p * P)(*[p.params.data_ptr() for p in pop.members])
    pop._chk(pop.L.wg_lstm_pop_update(pop._h, params, C.byref(b), perm.data_ptr(), E, int(envs_per_batch), hp, f(hyper["learning_rate"]),
                                      f(hyper["max_grad_norm"]), st.data_ptr(), pop._stream()), "wg_lstm_pop_update")
    return st


def single_update(opt, cols, perm_local, envs_per_batch, hyper, m):
    """wg_lstm_ppo_update of one member on its contiguous columns with LOCAL env ids -> stats ``[E, n_mb, 8]``."""
    return opt.update(cols, perm_local, envs_per_batch, clip_range=hyper["clip_range"][m], vf_coef=hyper["vf_coef"][m],
                      ent_coef=hyper["ent_coef"][m], normalize_advantage=hyper["normalize_advantage"][m],
                      learning_rate=hyper["learning_rate"][m], max_grad_norm=hyper["max_grad_norm"][m]).clone()
