"""Populations of recurrent policies: P ``RecurrentPPO`` runs of one architecture collected and trained in the kernel launches of one
(include/windgym_hip.h: ``wg_lstm_pop_*``) — the seeds of a result, or a sweep of ``gamma`` / ``learning_rate`` / ``ent_coef``, on ONE
env batch, member ``m`` owning the envs ``[m * Bm, (m + 1) * Bm)``, ``Bm = num_envs / P``.

One recurrent run of seed size leaves most of the device idle — a workgroup of the sequence kernels owns 32 envs for all ``n_steps``
steps, so 256 envs are 8 workgroups per LSTM — and a sweep is P such runs; in the same launches they are P times the workgroups.

The contract is :mod:`windgym_amd.population`'s, unchanged: whatever a member computes — its rollout columns, its LSTM state, its
parameters and Adam state after any number of iterations — is, to the bit, what ``RecurrentPPO`` computes alone on that shard.
:class:`RecurrentPopulation` is the acting object (``venv.rollout(pop, T)``), :class:`RecurrentPPOPopulation` the trainer; the
members stay ordinary :class:`~windgym_amd.recurrent.MlpLstmPolicy` objects.  The LSTM STATE of a population is one float32 CUDA
tensor ``[P, nets, 2, Bm, H]``: ``state[m]`` is exactly the member's own state tensor.  There is no CPU fallback; :func:`global_envs`
and :func:`member_minibatch` are pure host functions.

Not offered, refused by name: a ``WindFarmVecEnvMulti``, a curriculum or ``VecNormalize`` around a population, members of differing
architecture or ``n_steps``, ``sample_site``.
"""
from __future__ import annotations

import ctypes as C

from .policy import act_buffers, device_tensor
from .population import PopulationBase, PPOPopulation, check_members, check_population_shape
from .recurrent_ppo import RecurrentPPO, RecurrentPPOOptimizer, envs_per_minibatch


def global_envs(local, member, n_envs_member):
    """Env ids of the whole batch for the LOCAL env ids ``e`` in ``[0, Bm)`` that member ``member`` would use on its own shard:
    ``member * Bm + e``.  Works on ints, numpy arrays and torch tensors alike."""
    return local + int(member) * int(n_envs_member)


def member_minibatch(batch_size, n_steps, n_envs, n_members):
    """``batch_size`` in env steps of ONE member -> ``(envs per member, envs per minibatch, minibatches per epoch)``:
    :func:`~windgym_amd.recurrent_ppo.envs_per_minibatch` applied to ``Bm = n_envs / n_members`` (``None``: ``ceil(Bm / 4)`` envs)."""
    Bm = check_population_shape(n_members, n_envs)
    epb = envs_per_minibatch(batch_size, n_steps, Bm)
    return Bm, epb, -(-Bm // epb)


def check_same_architecture(members):
    """``ValueError`` naming the member for what wg_lstm_pop_create would refuse of the policies' shapes."""
    members = check_members(members)
    for m, p in enumerate(members):
        if not getattr(p, "recurrent", False):
            raise ValueError(f"member {m} is not a recurrent policy (MlpLstmPolicy): population.Population takes MlpPolicy objects")
        if p.desc != members[0].desc:
            raise ValueError(f"member {m} has another architecture than member 0 (n_in, lstm_hidden_size, shared_lstm, the heads and the "
                             "activation must agree): the members of a population share one")
    return members


class RecurrentPopulation(PopulationBase):
    """``P`` :class:`MlpLstmPolicy` objects of one architecture behind one ``wg_lstm_pop`` handle: ``act`` is ONE launch of the LSTM
    kernel and ONE of the policy kernel for all members, member ``m`` on rows ``[m * Bm, (m + 1) * Bm)`` with the state ``state[m]``;
    ``venv.rollout(pop, T)`` is wg_lstm_pop_rollout.  ``optimizers``: the members' :class:`RecurrentPPOOptimizer` objects (needed by
    wg_lstm_pop_update only)."""

    recurrent = True
    split = False
    has_critic = True
    check, destroy, rollout_entry = staticmethod(check_same_architecture), "wg_lstm_pop_destroy", "wg_lstm_pop_rollout"

    def _create(self, arr):
        ms, h = self.members, C.c_void_p()
        self.H, self.nets, self._hbuf = ms[0].H, ms[0].nets, {}
        self._chk(self.L.wg_lstm_pop_create(arr([m._lstm for m in ms]), arr([m.mlp._h for m in ms]),
                                            None if self.optimizers is None else arr([o._h for o in self.optimizers]), self.n_members,
                                            C.byref(h)), "wg_lstm_pop_create")
        return h

    def initial_state(self, n):
        """The zero state of ``n`` rows shared out among the members: float32 CUDA ``[P, nets, 2, n / P, H]``."""
        Bm = check_population_shape(self.n_members, n)
        return self.torch.zeros((self.n_members, self.nets, 2, Bm, self.H), dtype=self.torch.float32, device=self.device)

    def act(self, obs, state, episode_start=None, deterministic=False, counter=0, *, seed=None, row_offset=0, value=True, out=None,
            state_out=None):
        """wg_lstm_pop_act on ``obs [n, n_in]``, ``state [P, nets, 2, n / P, H]`` and ``episode_start`` (uint8 ``[n]`` or None) ->
        ``((action, raw, logp, value), new_state)`` as :meth:`MlpLstmPolicy.act`, member ``m`` on its rows with ``state[m]``.  ``seed``:
        one per member (or a scalar for all; default: the members' own seeds); ``row_offset``: a list per member, or a scalar = the
        global row of member 0's first row, member ``m``'s being ``row_offset + m * Bm``."""
        t, P = self.torch, self.n_members
        if not (device_tensor(obs, t.float32) and obs.ndim == 2 and obs.shape[1] == self.n_in):
            raise ValueError(f"act(): obs must be a contiguous float32 CUDA tensor [n, {self.n_in}]")
        n = obs.shape[0]
        Bm = check_population_shape(P, n)
        if not (device_tensor(state, t.float32) and tuple(state.shape) == (P, self.nets, 2, Bm, self.H)):
            raise ValueError(f"act(): state must be a contiguous float32 CUDA tensor [{P}, {self.nets}, 2, {Bm}, {self.H}]")
        if episode_start is not None and not (device_tensor(episode_start, t.uint8) and episode_start.numel() == n):
            raise ValueError(f"act(): episode_start must be a contiguous uint8 CUDA tensor [{n}] (or None)")
        if state_out is None:
            state_out = t.zeros_like(state)
        elif not (device_tensor(state_out, t.float32) and state_out.shape == state.shape):
            raise ValueError("act(): state_out must be a contiguous float32 CUDA tensor of state's shape")
        a, r, lp, v = out if out is not None else act_buffers(self, n)
        hbuf = self._hbuf.get(n)
        if hbuf is None:
            hbuf = self._hbuf[n] = t.zeros((2, n, self.H), dtype=t.float32, device=self.device)
        self._chk(self.L.wg_lstm_pop_act(self._h, n, obs.data_ptr(), None if episode_start is None else episode_start.data_ptr(),
                                         state.data_ptr(), state_out.data_ptr(), hbuf.data_ptr(), int(bool(deterministic)),
                                         self._seeds(seed), int(counter), self._offsets(row_offset, Bm),
                                         a.data_ptr(), r.data_ptr(), lp.data_ptr(), v.data_ptr() if value else None, self._stream()),
                  "wg_lstm_pop_act")
        return (a, r, lp, (v if value else None)), state_out


class RecurrentPPOPopulation(PPOPopulation):
    """``P`` independent ``RecurrentPPO`` runs of one architecture on ONE ``WindFarmVecEnv``, in the kernel launches of one run: member
    ``m`` trains on the envs ``[m * Bm, (m + 1) * Bm)`` exactly as ``RecurrentPPO`` would on that shard alone (same seed and
    hyper-parameters => the same parameters, to the bit, after any number of iterations).

    The arguments are :class:`~windgym_amd.population.PPOPopulation`'s.  ``policy``: ``"MlpLstmPolicy"`` (then ``n_members`` policies
    are built from ``policy_kwargs`` as ``RecurrentPPO`` builds one, each from its member's seed) or a list of :class:`MlpLstmPolicy`
    objects of one architecture.  ``batch_size`` counts env steps of ONE member, must be a multiple of ``n_steps`` (a minibatch is a
    set of envs with all their steps) and defaults to ``n_steps * ceil(Bm / 4)``.  Per epoch and member one permutation of the member's
    ``Bm`` envs is drawn from the member's generator and mapped to the batch's env ids (:func:`global_envs`).  ``adaptive_lr`` is
    ``PPOPopulation``'s: a KL-adaptive learning rate per member on the device (wg_lstm_ppo_set_kl_lr on every member's handle).

    ``learn``, ``train``, ``log`` and ``members`` are ``PPOPopulation``'s; stated here are its seven hooks: ``_check_policy``,
    ``_minibatches``, ``_build_member``, ``_open``, ``_global`` (one permutation of the member's ``Bm`` envs per epoch), ``_batch``
    (wg_lstm_pop_update on a ``CLstmPpoBatch``) and ``_tensors``.  ``save(dir)`` writes ``member_00.zip`` ...: each a ``RecurrentPPO``
    checkpoint with the member's slice of the LSTM state and of the pending episode starts (``RecurrentPPO.load(zip, shard venv)``
    resumes that member alone, bit-identically).  Refused by name: a curriculum, ``normalize``, a ``WindFarmVecEnvMulti``,
    non-recurrent members (``PPOPopulation`` trains those)."""

    policy_name = "MlpLstmPolicy"
    recurrent = True            # (what the wrappers and WindFarmVecEnvMulti.rollout look at)

    def _check_policy(self, policy):
        if not isinstance(policy, str):
            check_same_architecture(policy)

    def _minibatches(self, batch_size):
        _, self.envs_per_batch, n_mb = member_minibatch(batch_size, self.n_steps, self.n_envs, self.n_members)
        return self.envs_per_batch * self.n_steps, self.n_envs_member, n_mb

    def _build_member(self, venv, shape, policy_kwargs, seed):
        return RecurrentPPO._build_policy(venv, shape, policy_kwargs, seed)

    def _open(self, members):
        self.opts = [RecurrentPPOOptimizer(p, self.n_steps, self.envs_per_batch) for p in members]
        self.population = RecurrentPopulation(members, self.opts)

    def _global(self, local, m):
        return global_envs(local, m, self.n_envs_member)

    def _batch(self, out):
        from .binding import CLstmPpoBatch
        return CLstmPpoBatch(out["obs"].data_ptr(), out["raw"].data_ptr(), out["logp"].data_ptr(), self._adv.data_ptr(), self._ret.data_ptr(),
                             out["episode_start"].data_ptr(), out["lstm_state0"].data_ptr(), self.n_steps,
                             self.n_envs), "wg_lstm_pop_update", self.envs_per_batch

    def _tensors(self, m):                        # state[m] and the member's pending episode starts
        Bm, ent = self.n_envs_member, self.venv._lstm_pair(self.population)
        return {"lstm_state.npy": ent[1][m], "episode_start.npy": ent[2][m * Bm:(m + 1) * Bm]}
