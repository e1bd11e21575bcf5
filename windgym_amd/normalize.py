"""stable-baselines3's ``VecNormalize`` for a ``WindFarmVecEnv``: running observation and return statistics on the device.

The observation statistics move at every step and the policy of step t + 1 reads rows normalised with them, so inside
``rollout`` the update runs in the closed loop (wg_rollout_norm: two small launches after every step kernel, no return to Python).
The policy never reads the reward while it collects, so the reward half is a post-pass over the rollout's ``[T, B]`` buffers
(wg_norm_reward), as GAE is.  include/windgym_hip.h restates the rules of SB3's class that are pinned; they are tested against a
float64 numpy restatement.
"""
from __future__ import annotations

import json

import numpy as np

from .policy import refuse_recurrent, refuse_table_agent

ARGS = ("norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma", "epsilon", "training")


def check_args(clip_obs, clip_reward, gamma, epsilon):
    """``ValueError`` naming the argument for what no ``VecNormalize`` accepts."""
    if not float(clip_obs) > 0.0:
        raise ValueError(f"clip_obs must be > 0, got {clip_obs!r}")
    if not float(clip_reward) > 0.0:
        raise ValueError(f"clip_reward must be > 0, got {clip_reward!r}")
    if not 0.0 <= float(gamma) <= 1.0:
        raise ValueError(f"gamma must lie in [0, 1], got {gamma!r}")
    if not 0.0 < float(epsilon) < 1.0:
        raise ValueError(f"epsilon must lie in (0, 1), got {epsilon!r}")


def check_env(venv, who="VecNormalize"):
    """The refusals that need no device: what kind of env ``venv`` is."""
    if getattr(venv, "population", None) is not None:
        raise NotImplementedError(f"{who}: venv is a population — per-member statistics are not implemented")
    if getattr(venv, "possible_agents", None) is not None:
        raise NotImplementedError(f"{who}: venv is a WindFarmVecEnvMulti — per-agent statistics are not implemented")
    if not (hasattr(venv, "batch") and hasattr(venv, "_rollout")):
        raise ValueError(f"{who}: venv must be a WindFarmVecEnv")
    if not getattr(venv, "as_torch", False):
        raise ValueError(f"{who}: venv works on CUDA tensors here: construct the env with as_torch=True")
    if getattr(venv, "_global_offset", 0) != 0 or getattr(venv, "_sharded", False):
        raise NotImplementedError(f"{who}: venv is a shard of an env spread over several ranks — its statistics would need an "
                                  "all-reduce, which is not implemented")


STATS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "returns")


def save_stats(path, args, stats):
    """The file of :meth:`VecNormalize.save`: an npz of the float64 statistics (``STATS``) and the arguments as a JSON string."""
    with open(path, "wb") as f:          # (a file object: np.savez would append ".npz" to a name without it)
        np.savez(f, args=np.array(json.dumps(args)), **{k: np.asarray(stats[k], np.float64) for k in STATS})
    return path


def load_stats(path):
    """-> ``(arguments, statistics)`` of a :func:`save_stats` file; nothing in it is unpickled."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in STATS + ("args",) if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not a VecNormalize file (no {missing[0]})")
        return json.loads(str(z["args"])), {k: z[k] for k in STATS}


class VecNormalize:
    """``VecNormalize(venv, training=True, norm_obs=True, norm_reward=True, clip_obs=10, clip_reward=10, gamma=0.99, epsilon=1e-8)``
    of SB3 around a ``WindFarmVecEnv(as_torch=True)``.  ``reset`` / ``step`` are the wrapper's for host loops; ``rollout`` is
    ``venv.rollout`` with the policy reading normalised rows (``obs`` / ``final_obs`` / ``reward`` of the returned dict are
    NORMALISED — what PPO trains on — and ``env_obs`` / ``env_final_obs`` / ``env_reward`` are the env's own).  ``venv``'s persistent
    outputs hold the env's own rows afterwards, as after ``venv.rollout``; the normalised current observation is kept here.
    ``training = False`` freezes both statistics (evaluation).  ``obs_rms`` / ``ret_rms``: ``(mean, var, count)`` float64, read from
    the device (they synchronise)."""

    def __init__(self, venv, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8, training=True):
        check_args(clip_obs, clip_reward, gamma, epsilon)
        check_env(venv)
        from .binding import Norm
        self.venv, self.batch, self.torch = venv, venv.batch, venv.batch.torch
        self.norm_obs, self.norm_reward = bool(norm_obs), bool(norm_reward)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = float(clip_obs), float(clip_reward), float(gamma), float(epsilon)
        b, t = self.batch, self.torch
        self._norm = Norm(b.obs_dim, b.B, b.device.index, self.norm_obs, self.norm_reward, self.clip_obs, self.clip_reward, self.gamma,
                          self.epsilon)
        self._training = True
        self.training = training
        f32 = dict(dtype=t.float32, device=b.device)
        self._cur = t.zeros((b.B, b.obs_dim), **f32)                   # the normalised current observation (slot 0 of the next rollout)
        self._fin = t.zeros((b.B, b.obs_dim), **f32)
        self._rew = t.zeros((b.B,), **f32)
        self._refresh()

    # -- the constructor's arguments, the statistics ---------------------------------------------------------------------
    def args(self):
        """The constructor's arguments after ``venv`` (what ``save`` and ``PPO.save`` store)."""
        return {k: getattr(self, k) for k in ARGS}

    @property
    def training(self):
        return self._training

    @training.setter
    def training(self, value):
        self._training = bool(value)
        self._norm.set_training(self._training)

    @property
    def obs_rms(self):
        s = self._norm.stats()
        return s["obs_mean"], s["obs_var"], float(s["obs_count"])

    @property
    def ret_rms(self):
        s = self._norm.stats()
        return float(s["ret_mean"]), float(s["ret_var"]), float(s["ret_count"])

    @property
    def returns(self):
        return self._norm.stats()["returns"]

    def state(self) -> bytes:
        return self._norm.state()

    def load_state(self, blob: bytes):
        """The statistics and ``returns`` of a :meth:`state` blob; the normalised current observation follows from them."""
        self._norm.load_state(blob)
        self._refresh()

    def _frozen(self, fn):
        """``fn()`` with the statistics frozen (the flag is the library's, on the host: nothing is synchronised)."""
        was = self._training
        self._norm.set_training(False)
        try:
            return fn()
        finally:
            self._norm.set_training(was)

    def _refresh(self):
        """The normalised current observation = ``normalize_obs`` of the env's, with the statistics as they stand."""
        self._frozen(lambda: self._norm.obs(self.batch.obs, self._cur))

    def close(self):
        self._norm.close()

    # -- the wrapper for host loops ---------------------------------------------------------------------------------------
    def reset(self, *, seed=None, options=None, mask=None):
        """SB3's ``VecNormalize.reset``: ``venv.reset``, ``returns = 0``, the statistics updated with the first rows when training,
        -> ``(normalised obs, infos)``."""
        _, infos = self.venv.reset(seed=seed, options=options, mask=mask)
        self._norm.reset_returns(mask)
        self._norm.obs(self.batch.obs, self._cur)
        return self._cur, infos

    def step(self, actions):
        """The wrapper's step: ``venv.step``, wg_norm_obs, wg_norm_reward (T = 1) -> ``(obs, reward, terminated, truncated, infos)``
        normalised; ``infos["final_obs"]`` are the normalised final rows."""
        obs, rew, term, trunc, infos = self.venv.step(actions)
        b = self.batch
        self._norm.obs(b.obs, self._cur, b.final_obs, self._fin)
        self._norm.reward(b.reward, b.truncated, self._rew)
        infos["final_obs"] = self._fin
        return self._cur, self._rew, term, trunc, infos

    def get_original_obs(self):
        return self.batch.obs

    def get_original_reward(self):
        return self.batch.reward

    def _rows(self, x):
        """An array or tensor as a contiguous float32 tensor on the env's device"""
        t = self.torch
        x = x if isinstance(x, t.Tensor) else t.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        return x.to(self.batch.device, dtype=t.float32).contiguous()

    def normalize_obs(self, x):
        """``clip((x - mean) / sqrt(var + epsilon))`` of rows ``[..., O]`` (array or tensor) with the statistics as they stand, by the
        kernel the closed loop uses -> a new float32 CUDA tensor.  Never updates."""
        O = self.batch.obs_dim
        x = self._rows(x)
        if not x.numel() or x.shape[-1] != O:
            raise ValueError(f"normalize_obs(): rows of {O} entries expected")
        out = self.torch.empty_like(x)
        self._frozen(lambda: self._norm.obs(x, out))
        return out

    def unnormalize_obs(self, x):
        """The inverse of :meth:`normalize_obs` where it did not clip (float64 on the host's copy of the statistics)."""
        if not self.norm_obs:
            return x
        t = self.torch
        mean, var, _ = self.obs_rms
        x = self._rows(x)
        m, s = t.from_numpy(mean).to(x.device), t.from_numpy(np.sqrt(var + self.epsilon)).to(x.device)
        return (x.double() * s + m).float()

    def normalize_reward(self, r):
        """``clip(r / sqrt(ret_rms.var + epsilon))`` of an array or tensor with the statistics as they stand (float64, rounded once)."""
        t = self.torch
        r = r if isinstance(r, t.Tensor) else t.from_numpy(np.ascontiguousarray(r, dtype=np.float32)).to(self.batch.device)
        if not self.norm_reward:
            return r
        var = self.ret_rms[1]
        return (r.double() / float(np.sqrt(var + self.epsilon))).clamp(-self.clip_reward, self.clip_reward).float()

    def reward_pass(self, reward, truncated, out=None):
        """The reward half on its own, as a post-pass over ``[T, B]`` CUDA tensors (wg_norm_reward): ``returns`` and ``ret_rms``
        move when training; -> the normalised reward (``out``, or a new tensor)."""
        out = self.torch.empty_like(reward) if out is None else out
        return self._norm.reward(reward, truncated, out)

    # -- the closed loop ----------------------------------------------------------------------------------------------------
    def rollout(self, policy, n_steps, *, deterministic=False, record=(), values=True, normalize_reward=True):
        """``venv.rollout(policy, n_steps)`` with the policy reading normalised rows (wg_rollout_norm; with ``sample_site`` the
        equivalent loop of ``act``, ``step``, wg_norm_obs from Python, as ``venv.rollout`` does).  ``normalize_reward=False`` leaves
        ``reward`` the env's and the return statistics untouched: :meth:`reward_pass` is then the caller's to run."""
        refuse_recurrent(policy, "VecNormalize.rollout()")
        refuse_table_agent(policy, "VecNormalize.rollout()")
        if getattr(policy, "population", None) is not None:
            raise NotImplementedError("VecNormalize.rollout(): policy is a population — per-member statistics are not implemented")
        v = self.venv
        out = v._rollout(policy.rollout_actor(v), n_steps, deterministic, record, values, **v._env_rows(norm=(self._norm, self._cur)))
        out["env_obs"], out["env_final_obs"], out["env_reward"] = out["obs"], out["final_obs"], out["reward"]
        out["obs"], out["final_obs"] = out.pop("norm_obs"), out.pop("norm_final_obs")
        if normalize_reward:
            key = ("norm_reward", int(n_steps))
            buf = v._rollout_bufs.get(key)
            if buf is None:
                buf = v._rollout_bufs[key] = self.torch.zeros_like(out["env_reward"])
            out["reward"] = self._norm.reward(out["env_reward"], out["truncated"], buf)
        return out

    # -- files ------------------------------------------------------------------------------------------------------------
    def save(self, path):
        """An npz of the statistics (float64 arrays) and the arguments (a JSON string): no pickle."""
        return save_stats(path, self.args(), self._norm.stats())

    @classmethod
    def load(cls, path, venv, **overrides):
        """A :meth:`save` file around ``venv`` (``overrides``: constructor arguments to replace, e.g. ``training=False``)."""
        args, s = load_stats(path)
        args.update(overrides)
        self = cls(venv, **args)
        self._load_stats(s)
        return self

    @classmethod
    def from_stats(cls, venv, obs_mean, obs_var, obs_count, ret_var=1.0, ret_mean=0.0, ret_count=1e-4, **kwargs):
        """Statistics exported from an SB3 run (``obs_rms.mean`` / ``.var`` / ``.count``, ``ret_rms.var`` ...); ``kwargs``: the
        constructor's.  ``ValueError`` for statistics of another width than the env's observation."""
        O = int(venv.batch.obs_dim) if hasattr(venv, "batch") else None
        for name, a in (("obs_mean", obs_mean), ("obs_var", obs_var)):
            if O is not None and np.asarray(a).shape != (O,):
                raise ValueError(f"{name} has shape {np.asarray(a).shape}: the env's observation has {O} entries")
        self = cls(venv, **kwargs)
        self._load_stats(dict(obs_mean=obs_mean, obs_var=obs_var, obs_count=obs_count, ret_mean=ret_mean, ret_var=ret_var,
                              ret_count=ret_count, returns=np.zeros(self.batch.B)))
        return self

    def _load_stats(self, s):
        from .binding import pack_norm_state
        b = self.batch
        if np.asarray(s["obs_mean"]).size != b.obs_dim or np.asarray(s["obs_var"]).size != b.obs_dim:
            self.close()
            raise ValueError(f"obs_mean / obs_var hold {np.asarray(s['obs_mean']).size} entries: the env's observation has {b.obs_dim}")
        returns = np.asarray(s["returns"], np.float64)
        if returns.size != b.B:                  # statistics travel between batch sizes; the discounted returns do not
            returns = np.zeros(b.B)
        self.load_state(pack_norm_state(b.obs_dim, b.B, s["obs_mean"], s["obs_var"], float(s["obs_count"]), float(s["ret_mean"]),
                                        float(s["ret_var"]), float(s["ret_count"]), returns))


def as_frozen(normalize, venv):
    """``normalize`` (a :class:`VecNormalize`, or the path of its npz) as a FROZEN wrapper of ``venv`` for evaluation:
    ``training=False``, ``norm_reward=False`` -> ``(wrapper, whether it was built here and is the caller's to close)``."""
    if isinstance(normalize, VecNormalize):
        if normalize.venv is venv and not normalize.training and not normalize.norm_reward:
            return normalize, False
        vn = VecNormalize(venv, **dict(normalize.args(), training=False, norm_reward=False))
        s = normalize._norm.stats()
        vn._load_stats(s)
        return vn, True
    return VecNormalize.load(normalize, venv, training=False, norm_reward=False), True
