"""Behaviour cloning into a recurrent policy on the device: :class:`~windgym_amd.imitation.BehaviorCloning`'s supervised start for an
:class:`~windgym_amd.recurrent.MlpLstmPolicy`, the policy that is hardest to train from a random start.

One iteration of :class:`RecurrentBehaviorCloning` is ``BehaviorCloning``'s, with the recurrent stack in the learner's place:

    ``venv.rollout(policy, n_steps)`` (wg_rollout_lstm; the learner acts, the pair's LSTM state carries from rollout to rollout) ->
    ONE Serial-Refine launch for the episodes that began inside the rollout, or the rows of a ``YawTable`` -> wg_expert_labels ->
    with ``vf_coef > 0`` wg_gae -> one permutation of the ENVS per epoch -> ONE wg_lstm_bc_update: backpropagation through time in
    HIP (k_lstm_seq_fwd, k_bc_grad_dh, k_lstm_seq_bwd, k_lstm_wgrad) on the ``wg_lstm_ppo`` handle ``RecurrentPPO`` trains with.

Minibatches are whole env sequences, as ``recurrent_ppo`` states it: ``batch_size`` is in env steps and a multiple of ``n_steps``.
Without ``vf_coef`` the critic is left alone and nothing of its side runs — with two LSTMs that is half of the sequence work.

There is no CPU fallback: :class:`RecurrentBehaviorCloning` needs the built library and a GPU.
"""
from __future__ import annotations

import numpy as np

from .imitation import BehaviorCloning, check_env
from .ppo import HYPER, read_checkpoint, write_checkpoint
from .recurrent_ppo import RecurrentPPO, RecurrentPPOOptimizer, envs_per_minibatch


class RecurrentBehaviorCloning(BehaviorCloning):
    """Fit an :class:`MlpLstmPolicy` to the Serial-Refine yaw optimiser by supervised learning on the states the policy itself visits
    (the module docstring states the iteration).

    The expert's arguments and their defaults are ``BehaviorCloning``'s: ``expert`` (a wake model's name or a ``YawTable``), ``loss``
    (``"mse"`` leaves ``log_std`` exactly where it was), ``ent_coef``, ``vf_coef`` (0: the critic — its MLP and, with two LSTMs, its
    LSTM — gets a gradient of exactly 0.0 and its kernels are not launched), ``deterministic``, ``refine_pass_n``, ``yaw_n``,
    ``search_yaw_max``.  The policy is handled as ``RecurrentPPO`` handles it: an :class:`MlpLstmPolicy`, or ``"MlpLstmPolicy"`` built
    from ``policy_kwargs``; ``batch_size`` is in env steps and must be a multiple of ``n_steps`` (default: ``n_steps * ceil(num_envs
    / 4)``).  Per epoch ONE permutation of the envs is drawn.

    ``learn`` / ``log`` / ``predict`` are the trainers', the log record is ``BehaviorCloning``'s.  ``RecurrentPPO(bc.policy, venv)``
    fine-tunes: a fresh optimiser on the cloned weights, and the pair's LSTM state continues.  ``save`` writes ``RecurrentPPO``'s zip
    (``lstm_state.npy`` and ``episode_start.npy`` included; ``MlpLstmPolicy.from_sb3_zip`` reads its policy) plus the JSON key
    ``bc``, ``bc_targets.npy`` and, for a ``YawTable``, ``bc_table.npz``; :meth:`load` resumes bit-identically on an env in the same
    state.  ``RecurrentPPO.load`` refuses such a zip and :meth:`load` refuses ``RecurrentPPO``'s, each by name.

    Refused: a policy that is not recurrent (``ValueError`` pointing to ``BehaviorCloning``), a ``WindFarmVecEnvMulti``, a
    population (``NotImplementedError``); ``as_torch=False``, an unknown ``loss`` or ``expert``, negative coefficients, a
    ``batch_size`` that cuts a sequence (``ValueError``)."""

    def __init__(self, policy, venv, expert="blondel_jimenez", n_steps=128, batch_size=None, n_epochs=4, learning_rate=1e-3,
                 loss="mse", ent_coef=0.0, vf_coef=0.0, gamma=0.99, gae_lambda=0.95, max_grad_norm=0.5, deterministic=False,
                 refine_pass_n=8, yaw_n=9, search_yaw_max=30.0, policy_kwargs=None, seed=None):
        who = "RecurrentBehaviorCloning"
        if isinstance(policy, str):
            if policy != "MlpLstmPolicy":
                raise ValueError(f"unknown policy {policy!r}: only 'MlpLstmPolicy' (BehaviorCloning clones into 'MlpPolicy')")
        elif getattr(policy, "population", None) is None and not getattr(policy, "recurrent", False):
            raise ValueError(f"{who} needs a recurrent policy (MlpLstmPolicy): BehaviorCloning clones into an MlpPolicy")
        elif policy_kwargs:
            raise ValueError("policy_kwargs only applies to policy='MlpLstmPolicy'")
        if getattr(venv, "possible_agents", None) is not None:
            raise NotImplementedError(f"{who} on a WindFarmVecEnvMulti (a recurrent policy shared by the turbines) is not implemented")
        check_env(venv, policy, who, recurrent=True)
        self._setup_expert(who, venv, expert, loss, ent_coef, vf_coef, deterministic, refine_pass_n, yaw_n, search_yaw_max, n_steps,
                           n_epochs, gamma, gae_lambda, max_grad_norm, learning_rate, seed)
        n_steps, B = self.n_steps, int(venv.num_envs)
        self.envs_per_batch = envs_per_minibatch(batch_size, n_steps, B)
        want = (int(venv.batch.obs_dim), int(venv.n_turb))
        if isinstance(policy, str):
            policy = RecurrentPPO._build_policy(venv, want, dict(policy_kwargs or {}), 0 if seed is None else int(seed))
        if (policy.n_in, policy.n_out) != want:
            raise ValueError(f"the policy maps {policy.n_in} -> {policy.n_out}, this env needs {want[0]} -> {want[1]}")
        self.policy, self.venv, self.torch, self.batch = policy, venv, policy.torch, venv.batch
        self.batch_size = self.envs_per_batch * n_steps
        self.n_rows = self.n_env_steps = n_steps * B
        self.multi, self.n_agents = False, 1
        self.opt = RecurrentPPOOptimizer(policy, n_steps, self.envs_per_batch)
        self._alloc(B, (n_steps, B), -(-B // self.envs_per_batch))
        self._alloc_expert()

    # -- training -------------------------------------------------------------------------------------------------
    # collect(): BehaviorCloning's — venv.rollout dispatches on the policy (wg_rollout_lstm, the pair's LSTM state kept), the targets,
    # the labels and wg_gae are policy-agnostic

    def train(self, out, learning_rate, clip_range=None):
        """One permutation of the envs per epoch, then ONE wg_lstm_bc_update on the rollout's sequences."""
        t = self.torch
        for e in range(self.n_epochs):
            self._perm[e].copy_(t.randperm(self.venv.num_envs, generator=self._gen, device=self.policy.device))
        roll = dict(out, returns=self._ret if self.vf_coef > 0.0 else None)         # (labels: collect() put them there)
        return self.opt.bc_update(roll, self._perm, self.envs_per_batch, loss=self.loss, ent_coef=self.ent_coef, vf_coef=self.vf_coef,
                                  learning_rate=learning_rate, max_grad_norm=self.max_grad_norm, stats=self._stats)

    # -- checkpoints ----------------------------------------------------------------------------------------------
    def save(self, path):
        """Everything a bit-identical resume needs except the env itself.  Synchronises; a bad ``ep_row`` entry that a
        :meth:`collect` met is reported here (``ValueError``)."""
        self._lab.check()
        ent = self.venv._lstm_pair(self.policy)
        return write_checkpoint(path, self.policy, self.opt, self._gen, {k: getattr(self, k) for k in HYPER}, self.seed,
                                self.num_timesteps, self.iteration, self.log, self.critic, self.venv._policy_steps,
                                tensors={"lstm_state.npy": ent[1], "episode_start.npy": ent[2], "bc_targets.npy": self.targets},
                                extra=dict(bc=self.args()),
                                blobs={} if self.table is None else {"bc_table.npz": self.table.to_bytes()})

    @classmethod
    def load(cls, path, venv, learning_rate=None, device=None):
        """Resume: the policy, Adam's state, the permutation generator, the counters, the target table and the pair's LSTM state
        continue where ``save`` left them.  ``learning_rate``: the schedule again, when the saved run used a callable."""
        import torch
        from .recurrent import MlpLstmPolicy
        refusal = ("not a windgym_amd RecurrentBehaviorCloning checkpoint (RecurrentPPO.load resumes a RecurrentPPO checkpoint, "
                   "BehaviorCloning.load an MlpPolicy's)")
        meta, members = read_checkpoint(path, learning_rate, None, needs=("lstm_state.npy", "episode_start.npy", "bc_targets.npy"),
                                        refusal=refusal)
        if "bc" not in meta:
            raise ValueError(refusal)
        pol = MlpLstmPolicy.from_sb3_zip(path, activation=meta["desc"]["activation"], device=venv.batch.device.index if device is None else device,
                                         seed=meta["policy_seed"])
        pol.counter = int(meta["policy_counter"])
        hy = {k: v for k, v in meta["hyper"].items() if k not in ("clip_range", "normalize_advantage")}
        bc = dict(meta["bc"])
        if "bc_table.npz" in members:
            from .yaw_table import YawTable
            bc["expert"] = YawTable.from_bytes(members["bc_table.npz"], venv)
        self = cls(pol, venv, seed=meta["seed"], **bc, **hy)
        self._restore(meta, members)
        self.targets = self.torch.from_numpy(np.ascontiguousarray(members["bc_targets.npy"], dtype=np.float64)).to(self.batch.device)
        ent = self.venv._lstm_pair(self.policy)
        ent[1].copy_(torch.from_numpy(members["lstm_state.npy"]))
        ent[2].copy_(torch.from_numpy(members["episode_start.npy"]))
        return self
