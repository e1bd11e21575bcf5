"""RecurrentPPO for :class:`~windgym_amd.recurrent.MlpLstmPolicy` on the device — sb3-contrib's ``RecurrentPPO("MlpLstmPolicy", env)``,
the reference's own trainer (examples/curriculum.py:109-146), without sb3-contrib and without leaving the GPU between rollout and
update.

One iteration of :meth:`RecurrentPPO.learn` is ``venv.rollout`` (wg_rollout_lstm) -> ``wg_gae`` -> one permutation of the ENVS per
epoch from a seeded device generator -> ONE ``wg_lstm_ppo_update``: backpropagation through time in HIP (k_lstm_seq_fwd, k_ppo_grad_dh,
k_lstm_seq_bwd, k_lstm_wgrad), clipping by the global norm, Adam over the policy's one flat vector, repack.

**Minibatches are whole env sequences.**  A minibatch is a set of envs, each with all ``n_steps`` steps; every env's sequence is
re-evaluated through time from the LSTM state the rollout began with (``lstm_state0`` — data, not a function of the parameters, and
stale after the first minibatch), with ``episode_start[t]`` as the cell's select, across which no gradient flows.  That is exactly
sb3-contrib's sequence rule — sequences cut at episode starts, initial states taken from the rollout.  The one real difference:
sb3-contrib rotates a FLAT index of the ``n_steps * num_envs`` rows, so its minibatches can cut an env's sequence in two; here they
never do.  ``batch_size`` keeps SB3's meaning (env steps) and must therefore be a multiple of ``n_steps``; the default is
``n_steps * ceil(num_envs / 4)``.  Per epoch ONE permutation of the envs is drawn; minibatch ``j`` is ``perm[j * Bm : (j + 1) * Bm]``,
the last one possibly shorter.

:class:`RecurrentPPOOptimizer` is the thin wrapper of the ``wg_lstm_ppo_*`` entries of include/windgym_hip.h.  There is no CPU
fallback: without the built library or a GPU the constructors raise.
"""
from __future__ import annotations

import ctypes as C

from .policy import device_tensor
from .ppo import HandleOptimizer, Trainer, read_checkpoint, sb3_orthogonal_init
from .recurrent import MlpLstmPolicy


def envs_per_minibatch(batch_size, n_steps, num_envs):
    """``batch_size`` in env steps (SB3's meaning) -> envs per minibatch.  ``None``: ``ceil(num_envs / 4)`` envs, i.e. ``n_steps *
    ceil(num_envs / 4)`` steps.  Anything that is not a multiple of ``n_steps`` is a ``ValueError``."""
    n_steps, num_envs = int(n_steps), int(num_envs)
    if batch_size is None:
        return -(-num_envs // 4)
    batch_size = int(batch_size)
    if batch_size < n_steps or batch_size % n_steps:
        raise ValueError(f"batch_size = {batch_size} must be a multiple of n_steps = {n_steps}: a minibatch of a recurrent policy is a set "
                         "of envs, each with all its steps")
    if batch_size > n_steps * num_envs:
        raise ValueError(f"batch_size must lie in [n_steps, n_steps * num_envs = {n_steps * num_envs}]")
    return batch_size // n_steps


class RecurrentPPOOptimizer(HandleOptimizer):
    """The ``wg_lstm_ppo`` handle of one :class:`MlpLstmPolicy` for minibatches of up to ``max_envs`` envs x ``max_steps`` steps: Adam's
    state over ``policy.params`` and the buffers of the sequence kernels.  A ROLLOUT is the dict of ``venv.rollout(policy, T)`` with
    ``advantage`` / ``returns`` ``[T, B]`` added."""

    prefix, index_is = "wg_lstm_ppo", "env list"

    def __init__(self, policy, max_steps, max_envs):
        if not getattr(policy, "recurrent", False):
            raise ValueError("RecurrentPPOOptimizer needs a recurrent policy (MlpLstmPolicy); PPOOptimizer trains an MlpPolicy")
        self._open(policy, policy._lstm, policy.mlp._h, int(max_steps), int(max_envs))
        n = C.c_size_t()
        self._call("n_params", self._h, C.byref(n))
        assert int(n.value) == policy.params.numel()

    def _batch(self, roll):
        from .binding import CLstmPpoBatch
        t, p = self.torch, self.policy
        T, B = roll["raw"].shape[:2]
        self._f32(roll["raw"], (T, B, p.n_out), "raw")
        for k in ("logp", "advantage", "returns"):
            self._f32(roll[k], (T, B), k)
        obs, es, s0 = roll["obs"], roll["episode_start"], roll["lstm_state0"]
        if not (device_tensor(obs, t.float32) and obs.ndim == 3 and obs.shape[0] >= T and tuple(obs.shape[1:]) == (B, p.n_in)):
            raise ValueError(f"obs must be a contiguous float32 CUDA tensor [>= {T}, {B}, {p.n_in}]")
        if not (device_tensor(es, t.uint8) and es.ndim == 2 and es.shape[0] >= T and es.shape[1] == B):
            raise ValueError(f"episode_start must be a contiguous uint8 CUDA tensor [>= {T}, {B}]")
        if not (device_tensor(s0, t.float32) and tuple(s0.shape) == (p.nets, 2, B, p.H)):
            raise ValueError(f"lstm_state0 must be a contiguous float32 CUDA tensor [{p.nets}, 2, {B}, {p.H}]")
        return CLstmPpoBatch(obs.data_ptr(), roll["raw"].data_ptr(), roll["logp"].data_ptr(), roll["advantage"].data_ptr(),
                             roll["returns"].data_ptr(), es.data_ptr(), s0.data_ptr(), int(T), int(B)), T, B

    def grad(self, roll, envs, *, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, normalize_advantage=True, out=None, stats=None):
        """wg_lstm_ppo_grad: the minibatch of the envs ``envs`` (int32 CUDA) with all their steps -> (flat gradient ``[n_params]``,
        statistics ``[8]`` in the order of binding.PPO_STATS)."""
        t = self.torch
        b, _, _ = self._batch(roll)
        self._index(envs, 1)
        g = self.grad_buf if out is None else out
        st = t.zeros(8, dtype=t.float32, device=self.policy.device) if stats is None else stats
        self._chk(self.L.wg_lstm_ppo_grad(self._h, self.policy.params.data_ptr(), C.byref(b), envs.data_ptr(), int(envs.numel()),
                                          C.byref(self._hyper(clip_range, vf_coef, ent_coef, normalize_advantage)), g.data_ptr(),
                                          st.data_ptr(), self.policy._stream()), "wg_lstm_ppo_grad")
        return g, st

    def update(self, roll, perm, envs_per_batch, *, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, normalize_advantage=True,
               learning_rate=3e-4, max_grad_norm=0.5, stats=None):
        """wg_lstm_ppo_update: ``perm`` int32 ``[n_epochs, B]``, a permutation of the envs per epoch -> statistics
        ``[n_epochs, n_minibatches, 8]``."""
        t = self.torch
        b, _, B = self._batch(roll)
        if perm.ndim != 2 or perm.shape[1] != B:
            raise ValueError(f"perm must be [n_epochs, {B}]")
        self._index(perm, B)
        n_epochs, n_mb = perm.shape[0], -(-B // int(envs_per_batch))
        st = t.zeros((n_epochs, n_mb, 8), dtype=t.float32, device=self.policy.device) if stats is None else stats
        self._chk(self.L.wg_lstm_ppo_update(self._h, self.policy.params.data_ptr(), C.byref(b), perm.data_ptr(), n_epochs, int(envs_per_batch),
                                            C.byref(self._hyper(clip_range, vf_coef, ent_coef, normalize_advantage)), float(learning_rate),
                                            float(max_grad_norm), st.data_ptr(), self.policy._stream()), "wg_lstm_ppo_update")
        return st

    # -- the supervised loss on the same handle (recurrent_imitation.RecurrentBehaviorCloning) ------------------------------------
    def _bc_batch(self, roll, loss, ent_coef, vf_coef):
        """-> (wg_lstm_bc_batch, T, B, wg_bc_hyper) of a rollout that carries ``labels [T, B, n_out]`` (the expert's actions) and,
        optionally, ``returns [T, B]`` (absent or ``None``: the critic is left alone)."""
        from .binding import BC_LOSS, CBcHyper, CLstmBcBatch
        t, p = self.torch, self.policy
        if loss not in BC_LOSS:
            raise ValueError(f"loss must be one of {sorted(BC_LOSS)}, not {loss!r}")
        lab, ret = roll["labels"], roll.get("returns")
        if not (device_tensor(lab, t.float32) and lab.ndim == 3 and lab.shape[2] == p.n_out):
            raise ValueError(f"labels must be a contiguous float32 CUDA tensor [T, B, {p.n_out}]")
        T, B = lab.shape[:2]
        if ret is not None:
            self._f32(ret, (T, B), "returns")
        obs, es, s0 = roll["obs"], roll["episode_start"], roll["lstm_state0"]
        if not (device_tensor(obs, t.float32) and obs.ndim == 3 and obs.shape[0] >= T and tuple(obs.shape[1:]) == (B, p.n_in)):
            raise ValueError(f"obs must be a contiguous float32 CUDA tensor [>= {T}, {B}, {p.n_in}]")
        if not (device_tensor(es, t.uint8) and es.ndim == 2 and es.shape[0] >= T and es.shape[1] == B):
            raise ValueError(f"episode_start must be a contiguous uint8 CUDA tensor [>= {T}, {B}]")
        if not (device_tensor(s0, t.float32) and tuple(s0.shape) == (p.nets, 2, B, p.H)):
            raise ValueError(f"lstm_state0 must be a contiguous float32 CUDA tensor [{p.nets}, 2, {B}, {p.H}]")
        b = CLstmBcBatch(obs.data_ptr(), lab.data_ptr(), None if ret is None else ret.data_ptr(), es.data_ptr(), s0.data_ptr(), int(T), int(B))
        return b, int(T), int(B), CBcHyper(BC_LOSS[loss], float(ent_coef), float(vf_coef))

    def bc_grad(self, roll, envs, *, loss="mse", ent_coef=0.0, vf_coef=0.0, out=None, stats=None):
        """wg_lstm_bc_grad: the supervised loss on the expert's actions ``roll["labels"]`` over the minibatch of the envs ``envs``
        (int32 CUDA) with all their steps -> (flat gradient ``[n_params]``, statistics ``[8]`` in the order of binding.BC_STATS).
        Without ``roll["returns"]`` there is no critic term."""
        t = self.torch
        b, _, _, hp = self._bc_batch(roll, loss, ent_coef, vf_coef)
        self._index(envs, 1)
        g = self.grad_buf if out is None else out
        st = t.zeros(8, dtype=t.float32, device=self.policy.device) if stats is None else stats
        self._chk(self.L.wg_lstm_bc_grad(self._h, self.policy.params.data_ptr(), C.byref(b), envs.data_ptr(), int(envs.numel()), C.byref(hp),
                                         g.data_ptr(), st.data_ptr(), self.policy._stream()), "wg_lstm_bc_grad")
        return g, st

    def bc_update(self, roll, perm, envs_per_batch, *, loss="mse", ent_coef=0.0, vf_coef=0.0, learning_rate=1e-3, max_grad_norm=0.5,
                  stats=None):
        """wg_lstm_bc_update: ``perm`` int32 ``[n_epochs, B]``, a permutation of the envs per epoch -> statistics
        ``[n_epochs, n_minibatches, 8]``."""
        t = self.torch
        b, _, B, hp = self._bc_batch(roll, loss, ent_coef, vf_coef)
        if perm.ndim != 2 or perm.shape[1] != B:
            raise ValueError(f"perm must be [n_epochs, {B}]")
        self._index(perm, B)
        n_epochs, n_mb = perm.shape[0], -(-B // int(envs_per_batch))
        st = t.zeros((n_epochs, n_mb, 8), dtype=t.float32, device=self.policy.device) if stats is None else stats
        self._chk(self.L.wg_lstm_bc_update(self._h, self.policy.params.data_ptr(), C.byref(b), perm.data_ptr(), n_epochs, int(envs_per_batch),
                                           C.byref(hp), float(learning_rate), float(max_grad_norm), st.data_ptr(), self.policy._stream()),
                  "wg_lstm_bc_update")
        return st


class RecurrentPPO(Trainer):
    """sb3-contrib's ``RecurrentPPO`` on a ``WindFarmVecEnv``: :class:`~windgym_amd.ppo.PPO`'s arguments, defaults, schedules, ``log``
    records, ``learn`` callback and checkpoint layout, for an :class:`MlpLstmPolicy` (the module docstring states the minibatch rule
    and how it relates to sb3-contrib's).

    ``policy`` is an :class:`MlpLstmPolicy` (``MlpLstmPolicy.from_sb3_zip(...)`` fine-tunes a checkpoint) or the string
    ``"MlpLstmPolicy"``; the string builds one for the env from ``policy_kwargs``: ``lstm_hidden_size`` (256), ``net_arch``
    (``dict(pi=[64, 64], vf=[64, 64])`` or a list for both), ``shared_lstm`` (False), ``activation``.  Its initialisation is
    sb3-contrib's: SB3's orthogonal initialisation for the MLP (``ortho_init``), and ``torch.nn.LSTM``'s own U(-1/sqrt(H), 1/sqrt(H))
    for every LSTM tensor — sb3-contrib creates its ``nn.LSTM`` modules after ``_build`` has applied ``ortho_init``, and ``init_weights``
    only touches Linear and Conv2d layers, so its LSTMs are NOT initialised orthogonally.

    The LSTM state of the (policy, env) pair carries from rollout to rollout, as ``venv.rollout`` keeps it.  ``predict`` takes
    ``state`` / ``episode_start`` (sb3-contrib's protocol).  Refused by name: a non-recurrent policy (``ValueError`` pointing to
    ``PPO``), a ``WindFarmVecEnvMulti``, ``target_kl``, ``clip_range_vf``, ``use_sde`` (``NotImplementedError``).  A curriculum and
    ``VecNormalize`` around a recurrent trainer are not offered.  ``adaptive_lr`` is ``PPO``'s (the KL-adaptive learning rate on the
    device, here wg_lstm_ppo_set_kl_lr: ``learning_rate`` the starting rate, ``self.lr`` the device float, the rule applied before
    every optimiser step of an update but the first).

    ``save`` writes ``PPO.save``'s zip — ``policy.pth`` under sb3-contrib's names, which ``MlpLstmPolicy.from_sb3_zip`` reads back,
    Adam's state, the generator and the counters — plus the pair's LSTM state (``lstm_state.npy``) and the pending episode starts
    (``episode_start.npy``); ``load`` resumes on the same env object bit-identically."""

    def __init__(self, policy, venv, n_steps=128, batch_size=None, n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2,
                 ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, learning_rate=3e-4, normalize_advantage=True, policy_kwargs=None,
                 seed=None, target_kl=None, clip_range_vf=None, use_sde=False, adaptive_lr=None):
        self._setup(n_steps, n_epochs, gamma, gae_lambda, clip_range, ent_coef, vf_coef, max_grad_norm, learning_rate,
                    normalize_advantage, seed, target_kl, clip_range_vf, use_sde, adaptive_lr)
        if getattr(venv, "possible_agents", None) is not None:
            raise NotImplementedError("RecurrentPPO on a WindFarmVecEnvMulti (a recurrent policy shared by the turbines) is not implemented")
        if isinstance(policy, str):
            if policy != "MlpLstmPolicy":
                raise ValueError(f"unknown policy {policy!r}: only 'MlpLstmPolicy' (PPO trains 'MlpPolicy')")
        elif not getattr(policy, "recurrent", False):
            raise ValueError("RecurrentPPO needs a recurrent policy (MlpLstmPolicy): PPO trains an MlpPolicy")
        elif policy_kwargs:
            raise ValueError("policy_kwargs only applies to policy='MlpLstmPolicy'")
        n_steps, B = self.n_steps, int(venv.num_envs)
        self.envs_per_batch = envs_per_minibatch(batch_size, n_steps, B)
        want = (int(venv.batch.obs_dim), int(venv.n_turb))
        if isinstance(policy, str):
            policy = self._build_policy(venv, want, dict(policy_kwargs or {}), 0 if seed is None else int(seed))
        if (policy.n_in, policy.n_out) != want:
            raise ValueError(f"the policy maps {policy.n_in} -> {policy.n_out}, this env needs {want[0]} -> {want[1]}")
        self.policy, self.venv, self.torch = policy, venv, policy.torch
        self.batch_size = self.envs_per_batch * n_steps
        self.n_rows = self.n_env_steps = n_steps * B
        self.opt = RecurrentPPOOptimizer(policy, n_steps, self.envs_per_batch)
        self._alloc(B, (n_steps, B), -(-B // self.envs_per_batch))

    @staticmethod
    def _build_policy(venv, shape, kw, seed):
        arch = kw.pop("net_arch", dict(pi=[64, 64], vf=[64, 64]))
        H = kw.pop("lstm_hidden_size", 256)
        shared = bool(kw.pop("shared_lstm", False))
        activation = kw.pop("activation", "tanh")
        if int(kw.pop("n_lstm_layers", 1)) != 1:
            raise NotImplementedError("n_lstm_layers > 1 is not implemented")
        if not kw.pop("enable_critic_lstm", True) and not shared:
            raise NotImplementedError("enable_critic_lstm=False (the Linear critic) is not implemented: use shared_lstm=True")
        if kw:
            raise ValueError(f"unknown policy_kwargs: {sorted(kw)}")
        pi, vf = (arch["pi"], arch["vf"]) if isinstance(arch, dict) else (arch, arch)
        p = MlpLstmPolicy(*shape, H, tuple(pi), tuple(vf), shared, activation, device=venv.batch.device.index, seed=seed)
        sd = dict(p.state_dict())                              # the LSTMs keep torch.nn.LSTM's uniform init (the class docstring)
        sd.update(sb3_orthogonal_init(p.desc["mlp"], seed))
        p.load_state_dict(sd)
        return p

    # -- training -------------------------------------------------------------------------------------------------
    def collect(self):
        """One rollout of ``n_steps`` steps (wg_rollout_lstm, from the pair's kept LSTM state) + wg_gae -> the rollout dict with
        ``advantage`` / ``returns`` ``[T, B]`` added."""
        out = self.venv.rollout(self.policy, self.n_steps)
        self.opt.gae(out["reward"], out["value"], out["final_value"], out["truncated"], self.gamma, self.gae_lambda, out=(self._adv, self._ret))
        out["advantage"], out["returns"] = self._adv, self._ret
        return out

    def train(self, out, learning_rate, clip_range):
        """sb3-contrib's ``RecurrentPPO.train`` on a collected rollout: one permutation of the envs per epoch, then ONE
        wg_lstm_ppo_update."""
        t = self.torch
        for e in range(self.n_epochs):
            self._perm[e].copy_(t.randperm(self.venv.num_envs, generator=self._gen, device=self.policy.device))
        return self.opt.update(out, self._perm, self.envs_per_batch, clip_range=clip_range, vf_coef=self.vf_coef, ent_coef=self.ent_coef,
                               normalize_advantage=self.normalize_advantage, learning_rate=learning_rate, max_grad_norm=self.max_grad_norm,
                               stats=self._stats)

    # -- checkpoints ----------------------------------------------------------------------------------------------
    def _pair(self):
        """The env's entry of this (policy, env) pair — [weakref, LSTM state, pending episode starts, buffers] — as ``venv.rollout``
        keeps it."""
        return self.venv._lstm_pair(self.policy)

    def save(self, path):
        """Everything a bit-identical resume needs except the env itself (the class docstring)."""
        ent = self._pair()
        return super().save(path, {"lstm_state.npy": ent[1], "episode_start.npy": ent[2]})      # (+ the adaptive rate, where there is one)

    @classmethod
    def load(cls, path, venv, learning_rate=None, clip_range=None, device=None):
        """Resume: the policy, Adam's state, the generator, every counter and the pair's LSTM state continue where ``save`` left them.
        ``learning_rate`` / ``clip_range``: the schedules again, when the saved run used callables."""
        import torch
        meta, members = read_checkpoint(path, learning_rate, clip_range, needs=("lstm_state.npy",),
                                        refusal="not a windgym_amd RecurrentPPO checkpoint (an sb3-contrib zip loads with "
                                                "MlpLstmPolicy.from_sb3_zip, a PPO checkpoint with PPO.load)")
        if "bc" in meta:
            raise ValueError("not a windgym_amd RecurrentPPO checkpoint: RecurrentBehaviorCloning wrote it (RecurrentBehaviorCloning.load "
                             "resumes it; MlpLstmPolicy.from_sb3_zip reads its policy for RecurrentPPO to fine-tune)")
        pol = MlpLstmPolicy.from_sb3_zip(path, activation=meta["desc"]["activation"], device=venv.batch.device.index if device is None else device,
                                         seed=meta["policy_seed"])
        pol.counter = int(meta["policy_counter"])
        self = cls(pol, venv, seed=meta["seed"], adaptive_lr=meta.get("adaptive_lr"), **meta["hyper"])
        self._restore(meta, members)
        ent = self._pair()
        ent[1].copy_(torch.from_numpy(members["lstm_state.npy"]))
        ent[2].copy_(torch.from_numpy(members["episode_start.npy"]))
        return self
