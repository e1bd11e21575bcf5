"""Populations: P policies of one architecture collected and trained in the kernel launches of one (include/windgym_hip.h:
``wg_pop_*``) — the seeds of a result or a sweep of ``gamma`` / ``learning_rate`` / ``ent_coef`` (the reference runs such sweeps
as job arrays: examples/longer_steps_example.py + submit.sh) on ONE env batch, member ``m`` owning the envs
``[m * Bm, (m + 1) * Bm)``, ``Bm = num_envs / P``.

The contract is the library's usual one, applied across policies: whatever a member computes — its rollout columns, its
parameters after any number of iterations — is, to the bit, what it would have computed alone on its shard of the batch.
:class:`Population` is the acting object (``venv.rollout(pop, T)``), :class:`PPOPopulation` the trainer; the members stay
ordinary :class:`~windgym_amd.policy.MlpPolicy` objects.  There is no CPU fallback; the helpers :func:`broadcast_hyper` and
:func:`global_rows` are pure host functions.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .binding import Handle
from .policy import act_buffers, device_tensor, refuse_recurrent, refuse_table_agent
from .ppo import PPO, PPOOptimizer, _schedule, check_adaptive_lr, check_batch_size, check_hyper, learn_loop, write_checkpoint

POP_MAX = 16            # WG_POP_MAX
PER_MEMBER = ("gamma", "gae_lambda", "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "learning_rate", "normalize_advantage")
SHARED = ("n_steps", "n_epochs", "batch_size")


def broadcast_hyper(name, value, n_members):
    """A per-member hyper-parameter as a list of ``n_members`` entries: a scalar (or a schedule, a callable) is every member's,
    a list / tuple / array must have one entry per member."""
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != n_members:
            raise ValueError(f"{name}: {len(value)} values for {n_members} members (a scalar, or one value per member)")
        return list(value)
    return [value] * n_members


def member_adaptive_lr(adaptive_lr, learning_rate, n_members):
    """A population's ``adaptive_lr`` — a dict whose values are scalars for all members or lists of one value per member — -> the
    members' rules, each checked against the member's starting rate as :func:`~windgym_amd.ppo.check_adaptive_lr` checks one."""
    if not isinstance(adaptive_lr, dict):
        raise ValueError("adaptive_lr must be a dict(desired_kl=..., [factor, lr_min, lr_max]) or None")
    per = {k: broadcast_hyper(f"adaptive_lr: {k}", v, n_members) for k, v in adaptive_lr.items()}
    return [check_adaptive_lr({k: v[m] for k, v in per.items()}, learning_rate[m], f"member {m}: ") for m in range(n_members)]


def global_rows(local, member, n_envs, n_envs_member):
    """Row ids of a ``[T, B]`` rollout flattened to ``T * B`` rows, for the LOCAL row ids ``r`` in ``[0, T * Bm)`` that member
    ``member`` would use on its own ``[T, Bm]`` shard: ``(r // Bm) * B + member * Bm + r % Bm``.  Works on numpy arrays and torch
    tensors alike."""
    B, Bm = int(n_envs), int(n_envs_member)
    return (local // Bm) * B + int(member) * Bm + local % Bm


def check_member_count(n_members):
    if not 1 <= n_members <= POP_MAX:
        raise ValueError(f"a population has 1 .. {POP_MAX} members, not {n_members}")


def check_population_shape(n_members, n_envs):
    """-> envs per member; raises ``ValueError`` for what wg_pop_create / wg_pop_rollout would refuse."""
    P, B = int(n_members), int(n_envs)
    check_member_count(P)
    if B % P:
        raise ValueError(f"the {P} members own equal shares of the envs: num_envs = {B} does not divide by {P}")
    return B // P


def check_members(members):
    """The members as a list: 1 .. ``POP_MAX`` of them, no object twice."""
    members = list(members)
    refuse_table_agent(members, "a population")
    check_member_count(len(members))
    for m, p in enumerate(members):
        for k in range(m):
            if p is members[k]:
                raise ValueError(f"member {m} is the same policy as member {k}")
    return members


class PopulationBase(Handle):
    """What the two acting objects (:class:`Population`, ``recurrent_population.RecurrentPopulation``) share: the members behind one
    population handle of the library.  A subclass names the check of its members and the entry that destroys its handle, and states
    ``_create(arr)`` -> the handle, ``arr`` making the ``void*[P]`` of a list of handles."""

    check, destroy = staticmethod(check_members), None

    def __init__(self, members, optimizers=None):
        from .binding import _chk
        self.members = members = self.check(members)
        self.optimizers = None if optimizers is None else list(optimizers)
        p0 = members[0]
        self.L, self._chk, self.torch, self.device = p0.L, _chk, p0.torch, p0.device
        self.n_members = P = len(members)
        self.desc, self.n_in, self.n_out = p0.desc, p0.n_in, p0.n_out
        self._h = self._create(lambda hs: (C.c_void_p * P)(*[h.value for h in hs]))
        self._out = {}

    population = property(lambda self: self)      # (what the trainers and the wrappers look for)

    def rollout_actor(self, venv):
        """Member 0's statement (the members share one architecture) with the population in its place, on equal shares of the envs."""
        if venv.num_envs % self.n_members:
            raise ValueError(f"rollout(): the {self.n_members} members own equal shares of the envs: num_envs = {venv.num_envs} "
                             f"does not divide by {self.n_members}")
        return self.members[0].rollout_actor(venv)._replace(obj=self, entry=self.rollout_entry, handles=(self._h,), members=self.n_members)

    def _u64(self, x, default):
        P = self.n_members
        v = broadcast_hyper("seed / row_offset", default if x is None else x, P)
        return (C.c_uint64 * P)(*[int(i) for i in v])

    def _seeds(self, seed):                       # (default: the members' own)
        return self._u64(seed, [m.seed for m in self.members])

    def _offsets(self, row_offset, Bm):           # (a scalar: the global row of member 0's first row)
        if not isinstance(row_offset, (list, tuple, np.ndarray)):
            row_offset = [int(row_offset) + m * Bm for m in range(self.n_members)]
        return self._u64(row_offset, 0)


class Population(PopulationBase):
    """``P`` :class:`MlpPolicy` objects of one architecture behind one ``wg_pop`` handle: ``act`` / ``value`` are ONE launch of
    the policy kernel for all members, member ``m`` on rows ``[m * Bm, (m + 1) * Bm)``; ``venv.rollout(pop, T)`` is wg_pop_rollout.
    ``optimizers``: the members' :class:`PPOOptimizer` objects (needed by wg_pop_update only)."""

    destroy, rollout_entry = "wg_pop_destroy", "wg_pop_rollout"

    def _create(self, arr):
        p0, h = self.members[0], C.c_void_p()
        self.n_in_vf, self.has_critic, self.split = p0.n_in_vf, p0.has_critic, p0.split
        self._chk(self.L.wg_pop_create(arr([m._h for m in self.members]), None if self.optimizers is None else arr([o._h for o in self.optimizers]),
                                       self.n_members, C.byref(h)), "wg_pop_create")
        return h

    def act(self, obs, deterministic=False, counter=0, *, seed=None, row_offset=0, value=True, out=None):
        """wg_pop_act on a contiguous float32 CUDA tensor ``[..., n_in]`` whose rows divide evenly among the members ->
        ``(action, raw, logp, value)`` as :meth:`MlpPolicy.act`.  ``seed``: one per member (or a scalar for all; default: the
        members' own seeds); ``row_offset``: a list per member, or a scalar = the global row of member 0's first row, member
        ``m``'s being ``row_offset + m * Bm`` — with one seed for all, the noise of one policy on the whole batch."""
        t = self.torch
        if not (device_tensor(obs, t.float32) and obs.shape[-1] == self.n_in):
            raise ValueError(f"act(): obs must be a contiguous float32 CUDA tensor [..., {self.n_in}]")
        n = obs.numel() // self.n_in
        Bm = check_population_shape(self.n_members, n)
        a, r, lp, v = out if out is not None else act_buffers(self, n)
        want_v = value and self.has_critic
        ls = self.desc["has_log_std"]
        self._chk(self.L.wg_pop_act(self._h, n, obs.data_ptr(), int(bool(deterministic)), self._seeds(seed),
                                    int(counter), self._offsets(row_offset, Bm), a.data_ptr(), r.data_ptr(), lp.data_ptr() if ls else None,
                                    v.data_ptr() if want_v else None, self._stream()), "wg_pop_act")
        return a, r, (lp if ls else None), (v if want_v else None)

    def value(self, obs, out=None):
        """Critics only: member ``m``'s V on its share of the rows -> float32 CUDA tensor [rows]."""
        t = self.torch
        if not self.has_critic:
            raise ValueError("value(): the policies have no critic")
        n = obs.numel() // self.n_in_vf
        v = out if out is not None else t.zeros(n, dtype=t.float32, device=self.device)
        self._chk(self.L.wg_pop_act(self._h, n, obs.data_ptr(), 1, None, 0, None, None, None, None, v.data_ptr(), self._stream()),
                  "wg_pop_act")
        return v


class PPOPopulation:
    """``P`` independent PPO runs of one architecture on ONE ``WindFarmVecEnv``, in the kernel launches of one run: member ``m``
    trains on the envs ``[m * Bm, (m + 1) * Bm)`` exactly as ``PPO`` would on that shard alone (same seed and
    hyper-parameters => the same parameters, to the bit, after any number of iterations).

    ``policy``: ``"MlpPolicy"`` (then ``n_members`` policies are built with SB3's orthogonal initialisation from the members'
    seeds) or a list of :class:`MlpPolicy` objects of one architecture.  ``n_steps``, ``n_epochs`` and ``batch_size`` (in rows of
    ONE member; default a quarter of ``n_steps * Bm``) are shared — the members' launches run in lockstep; ``gamma``,
    ``gae_lambda``, ``clip_range``, ``ent_coef``, ``vf_coef``, ``max_grad_norm``, ``learning_rate`` (schedules included),
    ``normalize_advantage`` and ``seed`` are a scalar for all or one value per member; so are the values of ``adaptive_lr``
    (``PPO``'s KL-adaptive learning rate: every member then has a rate of its own on the device, ``self.lr`` float32 ``[P]``,
    steered by ITS minibatches' ``approx_kl`` toward ITS ``desired_kl`` — a seed or ``gamma`` sweep needs no second sweep over
    ``learning_rate``; ``learning_rate`` holds the starting rates).  A member's ``seed`` is what ``PPO``'s is:
    initial weights and minibatch permutations; action noise follows ``venv.rollout``'s rule (the env's base seed, its running
    count of policy steps, the global index of each env).

    ``learn(total_timesteps)`` counts env steps PER MEMBER; ``log`` holds one list of per-member records per logged iteration,
    computed on the device from the member's columns of the rollout (``mean_episode_power`` is not among them: the rollout
    records no powers).  ``members[m]`` is an ordinary policy; ``save(dir)`` writes ``member_00.zip`` ...: plain ``PPO`` zips
    (``PPO.load(zip, shard venv)`` resumes a member alone)."""

    # what recurrent_population.RecurrentPPOPopulation states differently: the policy class by name, and the seven hooks
    # _check_policy, _minibatches, _build_member, _open (below), _global, _batch and _tensors (next to train and save)
    policy_name = "MlpPolicy"

    def rollout_actor(self, venv):
        return self.population.rollout_actor(venv)

    def _check_policy(self, policy):
        refuse_recurrent(policy, "PPOPopulation")
        refuse_table_agent(policy, "PPOPopulation")

    def _minibatches(self, batch_size):
        """``batch_size`` as given -> (rows of a minibatch, width of a member's permutation, minibatches per epoch)."""
        batch_size = check_batch_size(batch_size, self.n_rows, "n_steps * num_envs / n_members")
        return batch_size, self.n_rows, -(-self.n_rows // batch_size)

    def _build_member(self, venv, shape, policy_kwargs, seed):
        return PPO._build_policy(venv, shape, policy_kwargs, seed)

    def _open(self, members):
        """The members' optimisers and the population object over both."""
        self.opts = [PPOOptimizer(p) for p in members]
        self.population = Population(members, self.opts)

    def __init__(self, policy, venv, n_members=None, n_steps=128, batch_size=None, n_epochs=10, gamma=0.99, gae_lambda=0.95,
                 clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, learning_rate=3e-4, normalize_advantage=True,
                 policy_kwargs=None, seed=None, curriculum=None, normalize=None, adaptive_lr=None):
        self._check_policy(policy)
        if curriculum is not None:
            raise NotImplementedError("a curriculum for a population is not implemented (use PPO(..., curriculum=...))")
        if normalize is not None:
            raise NotImplementedError("normalize for a population is not implemented: its members would need statistics of their own "
                                      "(use PPO(..., normalize=...))")
        if getattr(venv, "possible_agents", None) is not None:
            raise NotImplementedError("populations train on a WindFarmVecEnv: a WindFarmVecEnvMulti (wg_rollout_multi) is out of scope")
        objects = not isinstance(policy, str)
        if objects:
            policy = list(policy)
            if n_members is not None and int(n_members) != len(policy):
                raise ValueError(f"n_members = {n_members} contradicts the {len(policy)} policies given")
            n_members = len(policy)
            if policy_kwargs:
                raise ValueError(f"policy_kwargs only applies to policy='{self.policy_name}'")
        elif policy != self.policy_name:
            raise ValueError(f"unknown policy {policy!r}: only '{self.policy_name}' or a list of {self.policy_name} objects")
        elif n_members is None:
            raise ValueError(f"policy='{self.policy_name}' needs n_members")
        self.n_members = P = int(n_members)
        self.n_envs = B = int(venv.num_envs)
        self.n_envs_member = Bm = check_population_shape(P, B)
        hyper = dict(gamma=gamma, gae_lambda=gae_lambda, clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef,
                     max_grad_norm=max_grad_norm, learning_rate=learning_rate, normalize_advantage=normalize_advantage)
        for k in PER_MEMBER:
            setattr(self, k, broadcast_hyper(k, hyper[k], P))
        self.seed = broadcast_hyper("seed", seed, P)
        self.adaptive_lr = None if adaptive_lr is None else member_adaptive_lr(adaptive_lr, self.learning_rate, P)
        self.lr = None
        for m in range(P):
            check_hyper(n_steps, n_epochs, self.gamma[m], self.gae_lambda[m], self.max_grad_norm[m], f"member {m}: ")
        n_steps, n_epochs = int(n_steps), int(n_epochs)
        self.n_rows = n_steps * Bm                                         # rows of ONE member
        self.n_steps, self.n_epochs = n_steps, n_epochs
        self.batch_size, perm_width, n_mb = self._minibatches(batch_size)
        self._lr = [_schedule(x, "learning_rate") for x in self.learning_rate]
        self._clip = [_schedule(x, "clip_range") for x in self.clip_range]
        self.venv = venv
        want = (int(venv.batch.obs_dim), int(venv.n_turb))
        if not objects:
            policy = [self._build_member(venv, want, dict(policy_kwargs or {}), 0 if s is None else int(s)) for s in self.seed]
        for m, p in enumerate(policy):
            if (p.n_in, p.n_out) != want:
                raise ValueError(f"member {m} maps {p.n_in} -> {p.n_out}, this env needs {want[0]} -> {want[1]}")
        self.members = policy
        self.torch = t = policy[0].torch
        dev = policy[0].device
        self._open(policy)
        self._gens = []
        for s in self.seed:
            g = t.Generator(device=dev)
            g.manual_seed(0 if s is None else int(s))
            self._gens.append(g)
        self.n_minibatches = n_mb
        self._perm = t.zeros((P, n_epochs, perm_width), dtype=t.int32, device=dev)
        self._adv = t.zeros((n_steps, B), dtype=t.float32, device=dev)
        self._ret = t.zeros_like(self._adv)
        self._stats = t.zeros((P, n_epochs, n_mb, 8), dtype=t.float32, device=dev)
        self._ep_return = t.zeros(B, dtype=t.float64, device=dev)          # running return of every env's open episode (for the log)
        self.num_timesteps, self.iteration, self.log = 0, 0, []
        self.n_env_steps = n_steps * Bm
        if self.adaptive_lr is not None:                                   # the members' rates move to the device: ``lr`` float32 [P]
            self.lr = t.tensor([float(x) for x in self.learning_rate], dtype=t.float32, device=dev)
            for m, o in enumerate(self.opts):
                o.set_kl_lr(self.adaptive_lr[m], self.lr[m:m + 1])

    # -- training -------------------------------------------------------------------------------------------------
    def _floats(self, xs):
        return (C.c_float * self.n_members)(*[float(x) for x in xs])

    def collect(self):
        """One rollout of ``n_steps`` steps of the whole batch (wg_pop_rollout) + wg_gae_pop -> the rollout dict ``[T, B, ..]``
        with ``advantage`` / ``returns`` added; member ``m`` = columns ``m * Bm : (m + 1) * Bm``."""
        pop = self.population
        out = self.venv.rollout(pop, self.n_steps)
        pop._chk(pop.L.wg_gae_pop(self.n_steps, self.n_envs, self.n_members, out["reward"].data_ptr(), out["value"].data_ptr(),
                                  out["final_value"].data_ptr(), out["truncated"].data_ptr(), self._floats(self.gamma),
                                  self._floats(self.gae_lambda), self._adv.data_ptr(), self._ret.data_ptr(), pop._stream()), "wg_gae_pop")
        out["advantage"], out["returns"] = self._adv, self._ret
        return out

    def _global(self, local, m):                  # member m's permutation of its own rows -> the batch's row ids
        return global_rows(local, m, self.n_envs, self.n_envs_member)

    def _batch(self, out):
        """-> (the batch struct of a collected rollout, the update entry that takes it, the entry's minibatch size)."""
        from .binding import CPpoBatch
        T = self.n_steps
        return CPpoBatch(out["obs"][:T].data_ptr(), out["raw"].data_ptr(), out["logp"].data_ptr(), self._adv.data_ptr(),
                         self._ret.data_ptr(), T * self.n_envs), "wg_pop_update", self.batch_size

    def _tensors(self, m):                        # what member m's checkpoint holds besides a PPO zip's entries
        return None

    def train(self, out, learning_rate, clip_range):
        """Every member's ``train`` on its columns of a collected rollout: the members' permutations (drawn as the single trainer
        draws them on its shard, mapped to the batch's ids by :meth:`_global`), then ONE update entry."""
        from .binding import CPpoHyper
        t, pop, P = self.torch, self.population, self.n_members
        for m in range(P):
            for e in range(self.n_epochs):
                local = t.randperm(self._perm.shape[2], generator=self._gens[m], device=pop.device)
                self._perm[m, e].copy_(self._global(local, m))
        b, entry, minibatch = self._batch(out)
        hp = (CPpoHyper * P)(*[CPpoHyper(float(clip_range[m]), float(self.vf_coef[m]), float(self.ent_coef[m]),
                                         int(bool(self.normalize_advantage[m]))) for m in range(P)])
        params = (C.c_void_p * P)(*[p.params.data_ptr() for p in self.members])
        pop._chk(getattr(pop.L, entry)(pop._h, params, C.byref(b), self._perm.data_ptr(), self.n_epochs, minibatch, hp,
                                       self._floats(learning_rate), self._floats(self.max_grad_norm), self._stats.data_ptr(),
                                       pop._stream()), entry)
        return self._stats

    def _member_metrics(self, out):
        """[P, 5] float64 on the device: explained variance, episodes ended, sum of their returns, sum of rewards, steps."""
        t, P, Bm = self.torch, self.n_members, self.n_envs_member
        ret, val = self._ret.double().view(-1, P, Bm), out["value"].double().view(-1, P, Bm)
        ev = 1.0 - (ret - val).transpose(0, 1).reshape(P, -1).var(dim=1) / ret.transpose(0, 1).reshape(P, -1).var(dim=1)
        rew, tr = out["reward"].double(), out["truncated"].bool()
        c = rew.cumsum(dim=0)                                              # [T, B]
        T = rew.shape[0]
        last = t.where(tr, t.arange(T, device=rew.device).view(-1, 1).expand_as(tr), t.full_like(tr, -1, dtype=t.long)).max(dim=0).values
        any_end = last >= 0
        c_last = c.gather(0, last.clamp(min=0).view(1, -1))[0]
        ep_sum = t.where(any_end, self._ep_return + c_last, t.zeros_like(c_last))     # returns of all episodes that ended, per env
        self._ep_return = t.where(any_end, c[-1] - c_last, self._ep_return + c[-1])
        per = lambda x: x.view(P, Bm).sum(dim=1)                           # noqa: E731
        return t.stack([ev, per(tr.sum(dim=0).double()), per(ep_sum), per(rew.sum(dim=0)), t.full((P,), float(T * Bm), dtype=t.float64, device=rew.device)], dim=1)

    def learn(self, total_timesteps, callback=None, log_interval=1, reset_num_timesteps=True):
        """Iterations of rollout + update until every member collected ``total_timesteps`` env steps on its own envs.
        ``callback(pop) -> bool`` runs once per iteration; False stops.  Every ``log_interval``-th iteration appends a list of
        one record per member to ``self.log`` (ONE device-to-host copy for the whole population)."""
        return learn_loop(self, total_timesteps, callback, log_interval, reset_num_timesteps,
                          lambda progress: ([float(f(progress)) for f in self._lr], [float(f(progress)) for f in self._clip]), self._record)

    def _record(self, out, stats, lr, clip, fps):
        from .binding import PPO_STATS
        t = self.torch
        self.venv.batch.metrics(reset_after=True)                 # (whole-batch sums, not used: consumed as PPO.learn does)
        cols = [stats.double().mean(dim=(1, 2)), self._member_metrics(out)]
        if self.lr is not None:                                   # the members' rates after the iteration's last minibatch
            cols.append(self.lr.double().view(-1, 1))
        host = t.cat(cols, dim=1).cpu().numpy()                   # the one copy
        if self.lr is not None:
            lr = host[:, -1].tolist()
        fps = fps()
        recs = []
        for m in range(self.n_members):
            rec = dict(zip(PPO_STATS, host[m, :8].tolist()))
            ev, n_ep, ep_sum, rew_sum, n_st = host[m, 8:13].tolist()
            rec.update(member=m, explained_variance=ev, iteration=self.iteration, num_timesteps=self.num_timesteps,
                       learning_rate=lr[m], clip_range=clip[m], n_episodes=n_ep, mean_episode_return=ep_sum / max(n_ep, 1.0),
                       mean_step_reward=rew_sum / max(n_st, 1.0), fps=fps)
            recs.append(rec)
        return recs

    # -- checkpoints ----------------------------------------------------------------------------------------------
    def member_hyper(self, m):
        """The ``PPO`` arguments of member ``m``."""
        d = {k: getattr(self, k) for k in SHARED}
        d.update({k: getattr(self, k)[m] for k in PER_MEMBER})
        return d

    def save(self, directory):
        """``directory/member_00.zip`` ...: each the single trainer's checkpoint (see :meth:`PPO.save`) of the member's run on its shard."""
        os.makedirs(directory, exist_ok=True)
        paths = []
        for m in range(self.n_members):
            tensors, extra = self._tensors(m), None
            if self.adaptive_lr is not None:          # the member's rule and rate, as PPO.save stores them
                tensors, extra = dict(tensors or {}, **{"learning_rate.npy": self.lr[m:m + 1]}), dict(adaptive_lr=self.adaptive_lr[m])
            paths.append(write_checkpoint(os.path.join(directory, f"member_{m:02d}.zip"), self.members[m], self.opts[m], self._gens[m],
                                          self.member_hyper(m), self.seed[m], self.num_timesteps, self.iteration,
                                          [recs[m] for recs in self.log], None, self.venv._policy_steps, tensors=tensors, extra=extra))
        return paths

    def close(self):
        self.population.close()
        for o in self.opts:
            o.close()
