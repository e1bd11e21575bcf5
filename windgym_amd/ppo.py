"""PPO for :class:`~windgym_amd.policy.MlpPolicy` on the device — the reference's training call,
``PPO("MlpPolicy", env, n_steps=2048).learn(...)`` (examples/longer_steps_example.py:212-240, examples/curriculum.py:544-560),
without stable-baselines3 and without leaving the GPU between rollout and update.

One iteration of :meth:`PPO.learn` is ``venv.rollout`` (wg_rollout; wg_rollout_multi on a multi-agent env) -> ``wg_gae`` -> one ``torch.randperm`` per epoch from a
seeded device generator -> ``wg_ppo_update`` (n_epochs x minibatches of k_ppo_grad + clipping + Adam + repack), with one
device-to-host copy of the statistics per logged iteration.  :class:`PPOOptimizer` is the thin wrapper of the ``wg_ppo_*``
entries of include/windgym_hip.h (gradient and optimiser step are separate calls: a data-parallel trainer all-reduces the
flat gradient between them).  There is no CPU fallback: without the built library or a GPU the constructors raise.
"""
from __future__ import annotations

import ctypes as C
import io
import json
import time
import zipfile

import numpy as np

from .binding import Handle
from .policy import MlpPolicy, device_tensor, param_layout, refuse_recurrent, refuse_table_agent

HYPER = ("n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "clip_range", "ent_coef", "vf_coef", "max_grad_norm",
         "learning_rate", "normalize_advantage")


ADAPTIVE_LR = dict(factor=1.5, lr_min=1e-5, lr_max=1e-2)      # rsl_rl's constants; desired_kl has no default


def check_adaptive_lr(adaptive_lr, learning_rate, who=""):
    """``adaptive_lr`` as the trainers take it — a dict of ``desired_kl`` and, optionally, ``factor`` / ``lr_min`` / ``lr_max`` — ->
    the four arguments of wg_kl_lr as Python floats, or ``ValueError`` naming the argument (what ``wg_ppo_set_kl_lr`` refuses, decided
    without a device): ``desired_kl`` not > 0 or not finite, ``factor`` < 1 or not finite, ``lr_min`` not > 0, ``lr_min > lr_max``, a
    ``learning_rate`` — the STARTING rate — that is a schedule or lies outside ``[lr_min, lr_max]``.  All comparisons are on the
    float32 values the device holds.  ``who`` (``"member 3: "``) prefixes the messages."""
    if not isinstance(adaptive_lr, dict):
        raise ValueError(f"{who}adaptive_lr must be a dict(desired_kl=..., [factor, lr_min, lr_max]) or None")
    unknown = sorted(set(adaptive_lr) - {"desired_kl", *ADAPTIVE_LR})
    if unknown:
        raise ValueError(f"{who}adaptive_lr: unknown keys {unknown}")
    if "desired_kl" not in adaptive_lr:
        raise ValueError(f"{who}adaptive_lr needs desired_kl")
    if callable(learning_rate):
        raise ValueError(f"{who}learning_rate is a schedule: with adaptive_lr it is the STARTING rate and must be a number (a schedule "
                         "and a feedback rule would fight)")
    r = {k: np.float32(v) for k, v in dict(ADAPTIVE_LR, **adaptive_lr).items()}
    if not (r["desired_kl"] > 0 and np.isfinite(r["desired_kl"])):
        raise ValueError(f"{who}adaptive_lr: desired_kl must be > 0 and finite")
    if not (r["factor"] >= 1 and np.isfinite(r["factor"])):
        raise ValueError(f"{who}adaptive_lr: factor must be >= 1 and finite")
    if not r["lr_min"] > 0:
        raise ValueError(f"{who}adaptive_lr: lr_min must be > 0")
    if not r["lr_min"] <= r["lr_max"]:
        raise ValueError(f"{who}adaptive_lr: lr_min must be <= lr_max")
    if not r["lr_min"] <= np.float32(learning_rate) <= r["lr_max"]:
        raise ValueError(f"{who}learning_rate = {float(learning_rate):g}, the starting rate of adaptive_lr, lies outside [lr_min, lr_max] = "
                         f"[{float(r['lr_min']):g}, {float(r['lr_max']):g}]")
    return {k: float(r[k]) for k in ("desired_kl", "factor", "lr_min", "lr_max")}


def sb3_orthogonal_init(desc, seed):
    """{SB3 name: float32 array}: stable-baselines3's ``ortho_init`` — orthogonal weights with gain sqrt(2) for the hidden
    layers, 0.01 for the action head, 1 for the value head, zero biases and ``log_std`` — drawn from a seeded CPU generator
    (a normal matrix, QR, columns signed by R's diagonal: torch.nn.init.orthogonal_'s construction)."""
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    out = {}
    for name, shape in param_layout(desc):
        if len(shape) != 2:
            out[name] = np.zeros(shape, np.float32)
            continue
        gain = 0.01 if name == "action_net.weight" else 1.0 if name == "value_net.weight" else float(np.sqrt(2.0))
        rows, cols = shape
        a = torch.randn((rows, cols), generator=g, dtype=torch.float32)
        if rows < cols:
            a = a.T
        q, r = torch.linalg.qr(a)
        q = q * torch.sign(torch.diagonal(r))
        if rows < cols:
            q = q.T
        out[name] = (gain * q).contiguous().numpy().astype(np.float32)
    return out


class HandleOptimizer(Handle):
    """What the ``wg_ppo`` (:class:`PPOOptimizer`) and ``wg_lstm_ppo`` (``recurrent_ppo.RecurrentPPOOptimizer``) handles share: the
    handle's lifetime, the argument checks, wg_gae, the optimiser step and Adam's state.  ``prefix`` names the family's entries,
    ``index_is`` what ``_index`` calls its argument.  All methods enqueue on torch's current stream and synchronise nothing
    (``state()`` / ``load_state()`` excepted)."""

    prefix, index_is = None, None
    destroy = property(lambda self: self.prefix + "_destroy")

    def _open(self, policy, *create_args):
        """``<prefix>_create(*create_args, &handle)`` and the gradient buffer of ``policy.params``."""
        from .binding import _chk
        self.policy, self.L, self._chk, self.torch = policy, policy.L, _chk, policy.torch
        h = C.c_void_p()
        self._call("create", *create_args, C.byref(h))
        self._h = h
        self.grad_buf = self.torch.zeros_like(policy.params)

    def _call(self, entry, *args):
        name = f"{self.prefix}_{entry}"
        self._chk(getattr(self.L, name)(*args), name)

    def _f32(self, x, shape, what):
        if not (device_tensor(x, self.torch.float32) and x.numel() == int(np.prod(shape))):
            raise ValueError(f"{what} must be a contiguous float32 CUDA tensor of {int(np.prod(shape))} elements")
        return x

    def _index(self, index, n_min):
        if not (device_tensor(index, self.torch.int32) and index.numel() >= n_min):
            raise ValueError(f"the {self.index_is} / permutation must be a contiguous int32 CUDA tensor")
        return index

    @staticmethod
    def _hyper(clip_range, vf_coef, ent_coef, normalize_advantage):
        from .binding import CPpoHyper
        return CPpoHyper(float(clip_range), float(vf_coef), float(ent_coef), int(bool(normalize_advantage)))

    def gae(self, reward, value, final_value, truncated, gamma, gae_lambda, out=None):
        """wg_gae on ``[T, B]`` CUDA tensors (``truncated`` uint8) -> (advantage, returns).  With ``value`` / ``final_value
        [T, B, A]`` per agent row, ``reward`` / ``truncated [T, B]`` shared by an env's agents: wg_gae_shared -> ``[T, B, A]``."""
        t = self.torch
        T, B = reward.shape
        dims = (T, B) + tuple(value.shape[2:] if value.ndim == 3 else ())          # [T, B, A]: wg_gae_shared
        self._f32(reward, (T, B), "reward"); self._f32(value, dims, "value"); self._f32(final_value, dims, "final_value")
        if not (device_tensor(truncated, t.uint8) and tuple(truncated.shape) == (T, B)):
            raise ValueError("truncated must be a contiguous uint8 CUDA tensor [T, B]")
        adv, ret = out if out is not None else (t.empty_like(value), t.empty_like(value))
        entry = ("wg_gae", "wg_gae_shared")[len(dims) - 2]
        self._chk(getattr(self.L, entry)(*dims, reward.data_ptr(), value.data_ptr(), final_value.data_ptr(), truncated.data_ptr(),
                                         float(gamma), float(gae_lambda), adv.data_ptr(), ret.data_ptr(), self.policy._stream()), entry)
        return adv, ret

    def gae_shared(self, reward, value, *args, **kwargs):
        """:meth:`gae` for ``value [T, B, A]`` only (A = 1 included)."""
        if value.ndim != 3:
            raise ValueError("value must be [T, B, A]")
        return self.gae(reward, value, *args, **kwargs)

    def apply(self, grad=None, learning_rate=3e-4, max_grad_norm=0.5):
        """``<prefix>_apply``: clip, Adam on ``policy.params`` in place, repack — ``policy.act`` afterwards uses the new weights."""
        g = self.grad_buf if grad is None else grad
        self._call("apply", self._h, self.policy.params.data_ptr(), g.data_ptr(), float(learning_rate), float(max_grad_norm),
                   self.policy._stream())

    def set_kl_lr(self, rule, lr):
        """``<prefix>_set_kl_lr``: from now on ``update`` ignores its ``learning_rate``, reads the rate from ``lr`` — ONE float32 CUDA
        element, the starting rate, updated in place and kept alive here — and steps it by every minibatch's ``approx_kl`` but the
        update's first (``rule``: the dict of :func:`check_adaptive_lr`).  ``rule = lr = None`` turns that off again."""
        from .binding import CKlLr
        if rule is None and lr is None:
            self._call("set_kl_lr", self._h, None, None)
            self.lr = None
            return
        if lr is None or not (device_tensor(lr, self.torch.float32) and lr.numel() == 1):
            raise ValueError("lr must be a contiguous float32 CUDA tensor of one element")
        c = None if rule is None else CKlLr(*[float(rule[k]) for k in ("desired_kl", "factor", "lr_min", "lr_max")])
        self._call("set_kl_lr", self._h, None if c is None else C.byref(c), lr.data_ptr())
        self.lr = lr

    def state(self):
        """(Adam's m then v as one float32 numpy vector ``[2 n_params]``, step count)."""
        n = 2 * self.policy.params.numel()
        mv, step = np.zeros(n, np.float32), C.c_uint64()
        self._call("get_state", self._h, mv.ctypes.data_as(C.c_void_p), n, C.byref(step))
        return mv, int(step.value)

    def load_state(self, mv, step):
        mv = np.ascontiguousarray(mv, dtype=np.float32)
        self._call("set_state", self._h, mv.ctypes.data_as(C.c_void_p), mv.size, int(step))


class PPOOptimizer(HandleOptimizer):
    """The ``wg_ppo`` handle of one :class:`MlpPolicy`: Adam's state and the scratch of the gradient kernel."""

    prefix, index_is = "wg_ppo", "index"

    def __init__(self, policy):
        if not policy.has_critic or not policy.desc["has_log_std"]:
            raise ValueError("training needs a policy with a critic and log_std")
        self._open(policy, policy._h)

    def _batch(self, obs, raw, logp, advantage, returns, obs_vf=None, agents=1):
        """-> (batch struct, agent rows, shared?).  ``obs_vf`` / ``agents``: the critic's own stream ``[n / agents, n_in_vf]`` of a
        centralised critic (wg_ppo_batch_shared, taken by wg_ppo_grad_shared / wg_ppo_update_shared; ``advantage`` / ``returns`` are
        then per ENV row); without them the plain wg_ppo_batch of wg_ppo_grad / wg_ppo_update."""
        from .binding import CPpoBatch, CPpoBatchShared
        p = self.policy
        n, agents = logp.numel(), int(agents)
        if agents < 1 or n % agents:
            raise ValueError(f"agents must be >= 1 and divide the {n} rows")
        if obs_vf is None and p.split:
            raise ValueError(f"the policy's critic reads {p.n_in_vf} inputs: pass its rows as obs_vf")
        ne = n // agents
        self._f32(obs, (n, p.n_in), "obs"); self._f32(raw, (n, p.n_out), "raw"); self._f32(logp, (n,), "logp")
        self._f32(advantage, (ne,), "advantage"); self._f32(returns, (ne,), "returns")
        b = CPpoBatch(obs.data_ptr(), raw.data_ptr(), logp.data_ptr(), advantage.data_ptr(), returns.data_ptr(), n)
        if obs_vf is None and agents == 1:
            return b, n, False
        if obs_vf is None:
            raise ValueError("agents > 1 needs obs_vf, the env rows the critic reads")
        self._f32(obs_vf, (ne, p.n_in_vf), "obs_vf")
        return CPpoBatchShared(b, obs_vf.data_ptr(), agents), n, True

    def grad(self, obs, raw, logp, advantage, returns, *, index=None, first=0, n=None, clip_range=0.2, vf_coef=0.5,
             ent_coef=0.0, normalize_advantage=True, out=None, stats=None, obs_vf=None, agents=1):
        """wg_ppo_grad: one minibatch -> (flat gradient ``[n_params]``, statistics ``[8]`` in the order of binding.PPO_STATS).
        With ``obs_vf [rows / agents, n_in_vf]`` (and ``advantage`` / ``returns [rows / agents]``): wg_ppo_grad_shared, the
        centralised critic — entry ``id`` is an agent row of env row ``id // agents``."""
        t = self.torch
        b, rows, shared = self._batch(obs, raw, logp, advantage, returns, obs_vf, agents)
        entry = "wg_ppo_grad_shared" if shared else "wg_ppo_grad"
        if index is not None:
            n = index.numel() if n is None else int(n)
            self._index(index, n)
        elif n is None:
            n = rows - int(first)
        g = self.grad_buf if out is None else out
        st = t.zeros(8, dtype=t.float32, device=self.policy.device) if stats is None else stats
        self._chk(getattr(self.L, entry)(
            self._h, self.policy.params.data_ptr(), C.byref(b), None if index is None else index.data_ptr(), int(first), int(n),
            C.byref(self._hyper(clip_range, vf_coef, ent_coef, normalize_advantage)), g.data_ptr(), st.data_ptr(),
            self.policy._stream()), entry)
        return g, st

    def update(self, obs, raw, logp, advantage, returns, perm, batch_size, *, clip_range=0.2, vf_coef=0.5, ent_coef=0.0,
               normalize_advantage=True, learning_rate=3e-4, max_grad_norm=0.5, stats=None, obs_vf=None, agents=1):
        """wg_ppo_update: ``perm`` int32 ``[n_epochs, n_rows]`` -> statistics ``[n_epochs, n_minibatches, 8]``.  ``obs_vf`` /
        ``agents`` as in :meth:`grad` (wg_ppo_update_shared; ``perm`` and ``batch_size`` stay in agent rows)."""
        t = self.torch
        b, rows, shared = self._batch(obs, raw, logp, advantage, returns, obs_vf, agents)
        entry = "wg_ppo_update_shared" if shared else "wg_ppo_update"
        if perm.ndim != 2 or perm.shape[1] != rows:
            raise ValueError(f"perm must be [n_epochs, {rows}]")
        self._index(perm, rows)
        n_epochs, n_mb = perm.shape[0], -(-rows // int(batch_size))
        st = t.zeros((n_epochs, n_mb, 8), dtype=t.float32, device=self.policy.device) if stats is None else stats
        self._chk(getattr(self.L, entry)(
            self._h, self.policy.params.data_ptr(), C.byref(b), perm.data_ptr(), n_epochs, int(batch_size),
            C.byref(self._hyper(clip_range, vf_coef, ent_coef, normalize_advantage)), float(learning_rate), float(max_grad_norm),
            st.data_ptr(), self.policy._stream()), entry)
        return st

    # -- the supervised loss on the same handle (imitation.BehaviorCloning) --------------------------------------------------
    def _bc_batch(self, obs, target, returns, loss, ent_coef, vf_coef):
        from .binding import BC_LOSS, CBcBatch, CBcHyper
        p = self.policy
        if loss not in BC_LOSS:
            raise ValueError(f"loss must be one of {sorted(BC_LOSS)}, not {loss!r}")
        if p.split:
            raise ValueError(f"the policy's critic reads {p.n_in_vf} inputs: cloning a split policy is not implemented")
        n = target.numel() // p.n_out
        self._f32(obs, (n, p.n_in), "obs"); self._f32(target, (n, p.n_out), "target")
        if returns is not None:
            self._f32(returns, (n,), "returns")
        b = CBcBatch(obs.data_ptr(), target.data_ptr(), None if returns is None else returns.data_ptr(), n)
        return b, n, CBcHyper(BC_LOSS[loss], float(ent_coef), float(vf_coef))

    def bc_grad(self, obs, target, returns=None, *, index=None, first=0, n=None, loss="mse", ent_coef=0.0, vf_coef=0.0, out=None,
                stats=None):
        """wg_bc_grad: one minibatch of the supervised loss on the expert's actions ``target [rows, n_out]`` -> (flat gradient
        ``[n_params]``, statistics ``[8]`` in the order of binding.BC_STATS).  ``returns`` ``None``: no critic term."""
        t = self.torch
        b, rows, hp = self._bc_batch(obs, target, returns, loss, ent_coef, vf_coef)
        if index is not None:
            n = index.numel() if n is None else int(n)
            self._index(index, n)
        elif n is None:
            n = rows - int(first)
        g = self.grad_buf if out is None else out
        st = t.zeros(8, dtype=t.float32, device=self.policy.device) if stats is None else stats
        self._chk(self.L.wg_bc_grad(self._h, self.policy.params.data_ptr(), C.byref(b), None if index is None else index.data_ptr(),
                                    int(first), int(n), C.byref(hp), g.data_ptr(), st.data_ptr(), self.policy._stream()), "wg_bc_grad")
        return g, st

    def bc_update(self, obs, target, returns, perm, batch_size, *, loss="mse", ent_coef=0.0, vf_coef=0.0, learning_rate=1e-3,
                  max_grad_norm=0.5, stats=None):
        """wg_bc_update: ``perm`` int32 ``[n_epochs, n_rows]`` -> statistics ``[n_epochs, n_minibatches, 8]``."""
        t = self.torch
        b, rows, hp = self._bc_batch(obs, target, returns, loss, ent_coef, vf_coef)
        if perm.ndim != 2 or perm.shape[1] != rows:
            raise ValueError(f"perm must be [n_epochs, {rows}]")
        self._index(perm, rows)
        n_epochs, n_mb = perm.shape[0], -(-rows // int(batch_size))
        st = t.zeros((n_epochs, n_mb, 8), dtype=t.float32, device=self.policy.device) if stats is None else stats
        self._chk(self.L.wg_bc_update(self._h, self.policy.params.data_ptr(), C.byref(b), perm.data_ptr(), n_epochs, int(batch_size),
                                      C.byref(hp), float(learning_rate), float(max_grad_norm), st.data_ptr(), self.policy._stream()),
                  "wg_bc_update")
        return st


def _schedule(x, name):
    if callable(x):
        return x
    v = float(x)
    if not v >= 0.0:
        raise ValueError(f"{name} must be >= 0")
    return lambda progress_remaining: v


def check_hyper(n_steps, n_epochs, gamma, gae_lambda, max_grad_norm, who=""):
    """``ValueError`` for what no trainer accepts; ``who`` (``"member 3: "``) prefixes the messages about the values a population
    holds per member."""
    if int(n_steps) < 1 or int(n_epochs) < 1:
        raise ValueError("n_steps and n_epochs must be >= 1")
    if not 0.0 <= float(gamma) <= 1.0 or not 0.0 <= float(gae_lambda) <= 1.0:
        raise ValueError(f"{who}gamma and gae_lambda must lie in [0, 1]")
    if not float(max_grad_norm) > 0.0:
        raise ValueError(f"{who}max_grad_norm must be > 0")


def check_batch_size(batch_size, n_rows, rows_are):
    """-> the minibatch size in rows: a quarter of the rollout's ``n_rows`` by default (``rows_are`` spells ``n_rows`` in the message)."""
    batch_size = max(1, n_rows // 4) if batch_size is None else int(batch_size)
    if not 1 <= batch_size <= n_rows:
        raise ValueError(f"batch_size must lie in [1, {rows_are} = {n_rows}]")
    return batch_size


def learn_loop(trainer, total_timesteps, callback, log_interval, reset_num_timesteps, schedules, record):
    """``learn`` of :class:`PPO` and ``PPOPopulation``: iterations of ``trainer.collect()`` + ``trainer.train()`` until
    ``total_timesteps`` env steps were collected (``reset_num_timesteps=False``: that many more).  ``schedules(progress_remaining)
    -> (learning_rate, clip_range)`` as ``train`` takes them; ``record(out, stats, learning_rate, clip_range, fps) -> log entry``
    runs every ``log_interval``-th iteration, ``fps()`` being the env steps per second so far WHEN it is called (after the
    record's device-to-host copy, so that it counts finished work)."""
    if reset_num_timesteps:
        trainer.num_timesteps = 0
    start, total = trainer.num_timesteps, int(total_timesteps) + (0 if reset_num_timesteps else trainer.num_timesteps)
    t0 = time.perf_counter()
    while trainer.num_timesteps < total:
        lr, clip = schedules(1.0 - (trainer.num_timesteps - 0.0) / max(total, 1))
        out = trainer.collect()
        stats = trainer.train(out, lr, clip)
        trainer.num_timesteps += trainer.n_env_steps
        trainer.iteration += 1
        if log_interval and trainer.iteration % int(log_interval) == 0:
            trainer.log.append(record(out, stats, lr, clip,
                                      lambda: (trainer.num_timesteps - start) / max(time.perf_counter() - t0, 1e-9)))
        if callback is not None and callback(trainer) is False:
            break
    return trainer


def hyper_json(hyper):
    """The ``PPO`` arguments of ``HYPER`` as a checkpoint stores them."""
    d = {k: hyper[k] for k in HYPER}
    for k in ("learning_rate", "clip_range"):
        if callable(d[k]):
            d[k] = None                     # a schedule is code: pass it to load() again
    return d


def write_checkpoint(path, policy, opt, gen, hyper, seed, num_timesteps, iteration, log, critic, env_policy_steps, curriculum=None,
                     normalize=None, tensors=None, extra=None, blobs=None):
    """The zip of :meth:`PPO.save` (format: the class docstring) from what it holds: the policy, its :class:`PPOOptimizer`, the
    permutation generator, the ``HYPER`` dict, the trainer's seed, its counters and log, the critic mode and the env's count of
    policy steps; with a ``curriculum`` (a ``YawCurriculum``) also its arguments (JSON key ``curriculum``) and its state blob
    (member ``curriculum_state.bin``) and, when its targets come from a ``YawTable``, that table (member
    ``curriculum_table.npz``); with ``normalize`` (a ``VecNormalize``) its arguments (JSON key ``normalize``) and its state
    blob (member ``normalize_state.bin``); ``tensors``: {member name: tensor}, written as further npy members; ``extra``: further
    keys of the JSON (``imitation.BehaviorCloning``: ``bc``); ``blobs``: {member name: bytes}, written as they are."""
    import torch
    mv, step = opt.state()
    sd = {k: v.detach().cpu().clone() for k, v in policy.state_dict().items()}
    pth = io.BytesIO()
    torch.save(sd, pth)

    def npy(a):
        b = io.BytesIO()
        np.save(b, a)
        return b.getvalue()
    meta = dict(format="windgym_amd.PPO/1", desc=dict(policy.desc), hyper=hyper_json(hyper), seed=seed,
                policy_seed=policy.seed, policy_counter=policy.counter, num_timesteps=num_timesteps,
                iteration=iteration, adam_step=step, env_policy_steps=env_policy_steps, log=log, critic=critic)
    if curriculum is not None:
        meta["curriculum"] = curriculum.args()
    if normalize is not None:
        meta["normalize"] = normalize.args()
    meta.update(extra or {})
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        z.writestr("policy.pth", pth.getvalue())
        z.writestr("adam_state.npy", npy(mv))
        z.writestr("generator_state.npy", npy(gen.get_state().cpu().numpy()))
        z.writestr("windgym_ppo.json", json.dumps(meta))
        if curriculum is not None:
            z.writestr("curriculum_state.bin", curriculum.state())
            if getattr(curriculum, "table", None) is not None:
                z.writestr("curriculum_table.npz", curriculum.table.to_bytes())
        if normalize is not None:
            z.writestr("normalize_state.bin", normalize.state())
        for name, x in (tensors or {}).items():
            z.writestr(name, npy(x.detach().cpu().numpy()))
        for name, x in (blobs or {}).items():
            z.writestr(name, x)
    return path


def read_checkpoint(path, learning_rate=None, clip_range=None, needs=(), refusal="not a windgym_amd PPO checkpoint"):
    """The zip of :func:`write_checkpoint` -> (the JSON, {member name: npy members as arrays, every other member as bytes}).
    ``learning_rate`` / ``clip_range``: the schedules again when the run was saved with callables — the JSON's ``hyper`` comes back with
    them filled in, and a stored ``None`` with nothing passed is a ``ValueError``.  A zip without the JSON or one of the members
    ``needs`` is a ``ValueError(refusal)``."""
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
        if any(k not in names for k in ("windgym_ppo.json",) + tuple(needs)):
            raise ValueError(refusal)
        meta = json.loads(z.read("windgym_ppo.json").decode())
        members = {k: z.read(k) for k in names if k != "windgym_ppo.json"}
    members = {k: np.load(io.BytesIO(v)) if k.endswith(".npy") else v for k, v in members.items()}
    for k, v in (("learning_rate", learning_rate), ("clip_range", clip_range)):
        if v is not None:
            meta["hyper"][k] = v
        elif meta["hyper"][k] is None:
            raise ValueError(f"the checkpoint was trained with a {k} schedule: pass it to load()")
    return meta, members


class Trainer:
    """What :class:`PPO` and ``recurrent_ppo.RecurrentPPO`` share: the refusals, the hyper-parameters and schedules, the seeded
    permutation generator and the update's buffers, ``learn``, the log record, ``predict`` and the counters of a checkpoint.  A
    subclass sets ``policy`` / ``venv`` / ``torch`` / ``opt`` / ``n_rows`` / ``n_env_steps`` / ``batch_size`` and has ``collect`` and
    ``train``; ``curriculum`` / ``normalize`` / ``critic`` stay ``None`` where a trainer offers none."""

    curriculum = normalize = critic = adaptive_lr = lr = None

    def _setup(self, n_steps, n_epochs, gamma, gae_lambda, clip_range, ent_coef, vf_coef, max_grad_norm, learning_rate,
               normalize_advantage, seed, target_kl, clip_range_vf, use_sde, adaptive_lr=None):
        for name, v in (("target_kl", target_kl), ("clip_range_vf", clip_range_vf)):
            if v is not None:
                raise NotImplementedError(f"{name} is not implemented")
        if use_sde:
            raise NotImplementedError("use_sde (state-dependent exploration) is not implemented")
        check_hyper(n_steps, n_epochs, gamma, gae_lambda, max_grad_norm)
        if adaptive_lr is not None:
            self.adaptive_lr = check_adaptive_lr(adaptive_lr, learning_rate)
        self._lr, self._clip = _schedule(learning_rate, "learning_rate"), _schedule(clip_range, "clip_range")
        self.n_steps, self.n_epochs = int(n_steps), int(n_epochs)
        self.gamma, self.gae_lambda, self.ent_coef, self.vf_coef = float(gamma), float(gae_lambda), float(ent_coef), float(vf_coef)
        self.max_grad_norm, self.normalize_advantage = float(max_grad_norm), bool(normalize_advantage)
        self.learning_rate, self.clip_range, self.seed = learning_rate, clip_range, seed
        self.num_timesteps, self.iteration, self.log = 0, 0, []

    def _alloc(self, perm_width, adv_shape, n_minibatches):
        """The generator of the permutations (seeded) and the buffers of one update: ``_perm [n_epochs, perm_width]``, ``_adv`` /
        ``_ret [*adv_shape]``, ``_stats [n_epochs, n_minibatches, 8]``."""
        t, dev = self.torch, self.policy.device
        self._gen = t.Generator(device=dev)
        self._gen.manual_seed(0 if self.seed is None else int(self.seed))
        self._perm = t.zeros((self.n_epochs, perm_width), dtype=t.int32, device=dev)
        self._adv = t.zeros(adv_shape, dtype=t.float32, device=dev)
        self._ret = t.zeros_like(self._adv)
        self._stats = t.zeros((self.n_epochs, n_minibatches, 8), dtype=t.float32, device=dev)
        if self.adaptive_lr is not None:                          # the rate moves to the device: ``lr`` float32 [1], starting at learning_rate
            self.lr = t.full((1,), float(self.learning_rate), dtype=t.float32, device=dev)
            self.opt.set_kl_lr(self.adaptive_lr, self.lr)

    def learn(self, total_timesteps, callback=None, log_interval=1, reset_num_timesteps=True):
        """Iterations of rollout + update until ``total_timesteps`` env steps were collected (``reset_num_timesteps=False``:
        that many more).  ``callback(trainer) -> bool`` runs once per iteration; False stops.  Every ``log_interval``-th iteration
        appends a record to ``self.log`` (one device-to-host copy; ``log_interval=None``: never, and no synchronisation)."""
        return learn_loop(self, total_timesteps, callback, log_interval, reset_num_timesteps,
                          lambda progress: (float(self._lr(progress)), float(self._clip(progress))), self._record)

    def _record(self, out, stats, lr, clip, fps):
        from .binding import PPO_STATS
        from .parallel import METRIC_NAMES, derive
        t = self.torch
        ret, val = self._ret.double(), out["value"].double()
        ev = 1.0 - (ret - val).var() / ret.var()
        parts = [stats.double().mean(dim=(0, 1)), ev.reshape(1), self.venv.batch.metrics(reset_after=True).double().reshape(-1)]
        if self.curriculum is not None:
            parts += [out["curriculum_weight"].mean().reshape(1), out["yaw_diff"].double().mean().reshape(1)]
        if self.normalize is not None:
            parts += [out["reward"].double().mean().reshape(1)]
        if self.lr is not None:
            parts += [self.lr.double()]
        vec = t.cat(parts)
        host = vec.cpu().numpy()                                  # the iteration's one device-to-host copy
        if self.lr is not None:                                   # the rate after the iteration's last minibatch (float32, exact in a double)
            lr, host = float(host[-1]), host[:-1]
        rec = dict(zip(PPO_STATS, host[:8].tolist()))
        rec["explained_variance"] = float(host[8])
        m = derive(host[9:9 + len(METRIC_NAMES)])
        rec.update(iteration=self.iteration, num_timesteps=self.num_timesteps, learning_rate=lr, clip_range=clip,
                   n_episodes=m["n_episodes"], mean_episode_return=m["mean_episode_return"],
                   mean_episode_power=m["mean_episode_power"], mean_step_reward=m["mean_step_reward"], fps=fps())
        if self.curriculum is not None:
            rec.update(curriculum_weight=float(host[-2]), mean_yaw_diff=float(host[-1]))
        if self.normalize is not None:
            rec.update(mean_norm_reward=float(host[-1]), ret_rms_var=self.normalize.ret_rms[1])      # (the statistics: a copy of their own)
        return rec

    def predict(self, obs, state=None, episode_start=None, deterministic=False):
        if self.normalize is not None:
            obs = self.normalize.normalize_obs(obs)
        return self.policy.predict(obs, state, episode_start, deterministic)

    def save(self, path, tensors=None):
        """Everything a bit-identical resume needs except the env itself (the class docstring states the format)."""
        extra = None
        if self.adaptive_lr is not None:
            tensors, extra = dict(tensors or {}, **{"learning_rate.npy": self.lr}), dict(adaptive_lr=self.adaptive_lr)
        return write_checkpoint(path, self.policy, self.opt, self._gen, {k: getattr(self, k) for k in HYPER}, self.seed,
                                self.num_timesteps, self.iteration, self.log, self.critic, self.venv._policy_steps, self.curriculum,
                                self.normalize, tensors, extra)

    def _restore(self, meta, members):
        """Adam's state, the generator and the counters of a checkpoint (:func:`read_checkpoint`)."""
        self.opt.load_state(members["adam_state.npy"], meta["adam_step"])
        if self.lr is not None:
            self.lr.copy_(self.torch.from_numpy(np.asarray(members["learning_rate.npy"], np.float32).reshape(1)))
        self._gen.set_state(self.torch.from_numpy(members["generator_state.npy"]))
        self.num_timesteps, self.iteration, self.log = int(meta["num_timesteps"]), int(meta["iteration"]), list(meta["log"])
        self.venv._policy_steps = int(meta["env_policy_steps"])

    def close(self):
        self.opt.close()


class PPO(Trainer):
    """Proximal policy optimisation with stable-baselines3's argument names and defaults, on a ``WindFarmVecEnv``, or on a
    ``WindFarmVecEnvMulti`` with ONE policy shared by the turbines (``obs_len -> 1``): there a row is an AGENT row — ``n_rows``
    = ``n_steps * num_envs * n_turb``, the ``batch_size`` default and the permutations are in agent rows, advantages come
    from wg_gae_shared (the farm reward is every agent's reward, each agent's critic sees its own observation: independent PPO
    with shared parameters) — while ``num_timesteps``, ``fps`` and the episode means stay in env steps.
    ``critic="central"`` on a ``WindFarmVecEnvMulti`` is multi-agent PPO with a CENTRALISED critic (MAPPO: centralised training,
    decentralised execution): the actor still maps one agent's ``obs_len -> 1``, the critic reads the env's flat observation
    (``MlpPolicy(obs_len, 1, pi, vf, n_in_vf=obs_dim)``), there is one value and one advantage per env (wg_gae on ``[T, B]``),
    shared by its agents, and the update is wg_ppo_update_shared on the same agent rows.  With a policy OBJECT the mode is the
    policy's (``n_in_vf == obs_dim``: central); ``critic=None`` / ``"agent"`` with the string is the per-agent critic.  The mode
    is told by the critic's width, so it needs ``obs_dim != obs_len``: on a farm of ONE turbine (one agent per env) there is nothing
    to centralise and ``critic="central"`` is a ``ValueError``.

    Two defaults differ from SB3's, which sized them for a handful of host envs: ``n_steps`` = 128 (SB3: 2048) steps of EVERY env
    of the batch per rollout, and ``batch_size`` = a quarter of the rollout (SB3: 64 rows).  ``policy`` is an
    :class:`MlpPolicy` or the string ``"MlpPolicy"``; the string builds one for the env with SB3's orthogonal initialisation
    (``policy_kwargs``: ``net_arch=dict(pi=[...], vf=[...])`` or a list for both, ``activation`` ``"tanh"`` / ``"relu"``).
    ``learning_rate`` and ``clip_range`` may be callables of ``progress_remaining`` (1 -> 0), evaluated on the host once per
    iteration.  Not implemented (``NotImplementedError``): ``target_kl``, ``clip_range_vf``, ``use_sde``.

    ``adaptive_lr``: ``dict(desired_kl=..., factor=1.5, lr_min=1e-5, lr_max=1e-2)`` — the KL-adaptive learning rate of rsl_rl /
    rl_games, on the device (wg_ppo_set_kl_lr): ``learning_rate`` is then the STARTING rate and must be a number (a schedule with it is
    a ``ValueError``), the rate lives in ``self.lr`` (a float32 CUDA tensor ``[1]``) and every minibatch of an update but the first
    multiplies it by ``1 / factor`` when its ``approx_kl > 2 desired_kl`` and by ``factor`` when ``0 < approx_kl < desired_kl / 2``,
    clamped to ``[lr_min, lr_max]``, before its optimiser step — inside the Adam kernel, with no launch and no host round trip added
    (the first minibatch still has the rollout's parameters: its KL is rounding noise).  The log's ``learning_rate`` is then the rate
    after the iteration's last minibatch, read in the record's one copy; ``save`` stores the arguments under the JSON key
    ``adaptive_lr`` and the rate as ``learning_rate.npy``.  It works on both env kinds and both critic modes and composes with
    ``curriculum`` / ``normalize``, which act before the update.  ``None`` changes nothing.

    ``curriculum``: a ``curriculum.YawCurriculum`` of this env, or a dict of its arguments — the reference's
    examples/curriculum.py: rollouts come from ``curriculum.rollout`` (one host synchronisation per rollout, see there; none with
    ``targets=`` a ``yaw_table.YawTable`` among the arguments, which ``save`` then stores as ``curriculum_table.npz``), GAE and the
    update run on the shaped reward, the log gains ``curriculum_weight`` (mean of the rollout) and ``mean_yaw_diff`` while
    ``mean_step_reward`` / ``mean_episode_return`` stay the env's own.  ``None`` changes nothing.

    ``normalize``: a ``normalize.VecNormalize`` of this env (a ``WindFarmVecEnv``), or a dict of its arguments — SB3's usual
    set-up around the env: rollouts come from its ``rollout`` (the statistics move inside the closed loop), GAE and the update run
    on the normalised rows and reward, ``predict`` normalises the rows it is given, the log gains ``mean_norm_reward`` and
    ``ret_rms_var`` while ``mean_step_reward`` / ``mean_episode_return`` stay the env's own.  Not together with ``curriculum``
    (``NotImplementedError``).  ``None`` changes nothing.

    ``save`` writes a zip whose ``policy.pth`` is a ``torch.save`` of the state dict under SB3's names (``read_sb3_zip`` and
    ``MlpPolicy.from_sb3_zip`` read it), next to Adam's state, the counters and the hyper-parameters as npy / JSON (with a
    curriculum: its arguments under the JSON key ``curriculum`` and its state blob as ``curriculum_state.bin``; with ``normalize``:
    the JSON key ``normalize`` and ``normalize_state.bin``); a zip that
    SB3's own ``PPO.load`` accepts needs cloudpickled members and is out of scope."""

    def __init__(self, policy, venv, n_steps=128, batch_size=None, n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2,
                 ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, learning_rate=3e-4, normalize_advantage=True, policy_kwargs=None,
                 seed=None, target_kl=None, clip_range_vf=None, use_sde=False, critic=None, curriculum=None, normalize=None,
                 adaptive_lr=None):
        refuse_recurrent(policy, "PPO")
        refuse_table_agent(policy, "PPO")
        self._setup(n_steps, n_epochs, gamma, gae_lambda, clip_range, ent_coef, vf_coef, max_grad_norm, learning_rate,
                    normalize_advantage, seed, target_kl, clip_range_vf, use_sde, adaptive_lr)
        n_steps = self.n_steps
        if normalize is not None:
            from .normalize import VecNormalize, check_env
            if curriculum is not None:
                raise NotImplementedError("curriculum and normalize together are not implemented (VecNormalize.reward_pass is the seam "
                                          "for shaping the reward before it is normalised)")
            check_env(venv, "normalize")
            if not isinstance(normalize, (dict, VecNormalize)):
                raise ValueError("normalize must be a VecNormalize of this env or a dict of its arguments")
            if isinstance(normalize, VecNormalize) and normalize.venv is not venv:
                raise ValueError("normalize: the VecNormalize was built for another env")
        multi = getattr(venv, "possible_agents", None) is not None       # WindFarmVecEnvMulti: one row per (env, turbine)
        n_agents = int(venv.n_turb) if multi else 1
        n_rows = n_steps * int(venv.num_envs) * n_agents
        batch_size = check_batch_size(batch_size, n_rows, f"n_steps * num_envs{' * n_turb' if multi else ''}")
        if isinstance(policy, str) and policy != "MlpPolicy":
            raise ValueError(f"unknown policy {policy!r}: only 'MlpPolicy'")
        if policy_kwargs and not isinstance(policy, str):
            raise ValueError("policy_kwargs only applies to policy='MlpPolicy'")
        want = (int(venv.obs_len), 1) if multi else (int(venv.batch.obs_dim), int(venv.n_turb))       # the policy's n_in -> n_out
        if critic not in (None, "agent", "central"):
            raise ValueError(f"critic must be None, 'agent' or 'central', not {critic!r}")
        if critic == "central" and not multi:
            raise ValueError("critic='central' needs a WindFarmVecEnvMulti: on a WindFarmVecEnv the one agent's critic already reads "
                             "the flat observation, there is nothing to centralise")
        if critic == "central" and int(venv.batch.obs_dim) == want[0]:
            raise ValueError(f"critic='central' needs a farm of more than one turbine: here the flat observation and an agent's have "
                             f"the same {want[0]} values (one agent per env), there is nothing to centralise")
        if isinstance(policy, str):
            policy = self._build_policy(venv, want, dict(policy_kwargs or {}), 0 if seed is None else int(seed),
                                        int(venv.batch.obs_dim) if critic == "central" else None)
        if (policy.n_in, policy.n_out) != want:
            raise ValueError(f"the policy maps {policy.n_in} -> {policy.n_out}, this env needs {want[0]} -> {want[1]} "
                             "(accepted shapes: obs_dim -> n_turb on a WindFarmVecEnv, obs_len -> 1 — one policy shared by the "
                             "turbines — on a WindFarmVecEnvMulti)")
        central = bool(multi and policy.has_critic and policy.split)
        if policy.has_critic and policy.split and (not multi or policy.n_in_vf != int(venv.batch.obs_dim)):
            raise ValueError(f"the policy's critic reads {policy.n_in_vf} inputs: a split policy only fits a WindFarmVecEnvMulti, as "
                             f"its centralised critic on the flat observation (n_in_vf = obs_dim)")
        if critic is not None and (critic == "central") != central:
            raise ValueError(f"critic={critic!r} contradicts the policy, whose critic reads {policy.n_in_vf} inputs "
                             f"({'central' if central else 'agent'}): with a policy object the mode is the policy's")
        self.central, self.critic = central, "central" if central else "agent" if multi else None
        self.policy, self.venv, self.torch = policy, venv, policy.torch
        self.batch_size, self.n_rows = batch_size, n_rows
        self.multi, self.n_agents, self.n_env_steps = multi, n_agents, n_steps * int(venv.num_envs)
        self.opt = PPOOptimizer(policy)
        self._alloc(n_rows, (n_steps, venv.num_envs) + ((n_agents,) if multi and not central else ()), -(-n_rows // batch_size))
        self._owns_curriculum = isinstance(curriculum, dict)       # built here: closed with the trainer
        if self._owns_curriculum:
            from .curriculum import YawCurriculum
            curriculum = YawCurriculum(venv, **curriculum)
        if curriculum is not None and curriculum.venv is not venv:
            raise ValueError("the curriculum was built for another env")
        self.curriculum = curriculum
        self._owns_normalize = isinstance(normalize, dict)         # built here: closed with the trainer
        if self._owns_normalize:
            from .normalize import VecNormalize
            normalize = VecNormalize(venv, **normalize)
        self.normalize = normalize

    @staticmethod
    def _build_policy(venv, shape, kw, seed, n_in_vf=None):
        arch = kw.pop("net_arch", dict(pi=[64, 64], vf=[64, 64]))
        activation = kw.pop("activation", "tanh")
        if kw:
            raise ValueError(f"unknown policy_kwargs: {sorted(kw)}")
        pi, vf = (arch["pi"], arch["vf"]) if isinstance(arch, dict) else (arch, arch)
        p = MlpPolicy(*shape, tuple(pi), tuple(vf), activation, device=venv.batch.device.index, seed=seed, n_in_vf=n_in_vf)
        p.load_state_dict(sb3_orthogonal_init(p.desc, seed))
        return p

    # -- training -------------------------------------------------------------------------------------------------
    def collect(self):
        """One rollout of ``n_steps`` steps + wg_gae -> the rollout dict with ``advantage`` / ``returns`` ``[T, B]`` added
        (``[T, B, N]`` from wg_gae_shared on a ``WindFarmVecEnvMulti``; ``[T, B]`` again under its centralised critic)."""
        if self.normalize is not None:
            out = self.normalize.rollout(self.policy, self.n_steps)
        elif self.curriculum is None:
            out = self.venv.rollout(self.policy, self.n_steps)
        else:
            out = self.curriculum.rollout(self.policy, self.n_steps, num_timesteps=self.num_timesteps)
        self.opt.gae(out["reward"], out["value"], out["final_value"], out["truncated"], self.gamma, self.gae_lambda, out=(self._adv, self._ret))
        out["advantage"], out["returns"] = self._adv, self._ret
        return out

    def train(self, out, learning_rate, clip_range):
        """SB3's ``PPO.train`` on a collected rollout: the epochs' permutations, then ONE wg_ppo_update."""
        t = self.torch
        for e in range(self.n_epochs):
            self._perm[e].copy_(t.randperm(self.n_rows, generator=self._gen, device=self.policy.device))
        T, O, N = self.n_steps, self.policy.n_in, self.policy.n_out
        shared = dict(obs_vf=out["flat_obs"][:T].view(-1, self.policy.n_in_vf), agents=self.n_agents) if self.central else {}
        return self.opt.update(out["obs"][:T].view(-1, O), out["raw"].view(-1, N), out["logp"].view(-1), self._adv.view(-1),
                               self._ret.view(-1), self._perm, self.batch_size, clip_range=clip_range, vf_coef=self.vf_coef,
                               ent_coef=self.ent_coef, normalize_advantage=self.normalize_advantage,
                               learning_rate=learning_rate, max_grad_norm=self.max_grad_norm, stats=self._stats, **shared)

    # -- checkpoints ----------------------------------------------------------------------------------------------
    @classmethod
    def load(cls, path, venv, learning_rate=None, clip_range=None, device=None):
        """Resume: the policy, Adam's state, the permutation generator and every counter continue where ``save`` left them, so
        that on an env in the same state ``learn(..., reset_num_timesteps=False)`` computes what the uninterrupted run would
        have.  ``learning_rate`` / ``clip_range``: the schedules again, when the saved run used callables."""
        from .policy import read_sb3_zip
        meta, members = read_checkpoint(path, learning_rate, clip_range,
                                        refusal="not a windgym_amd PPO checkpoint (for an SB3 zip use MlpPolicy.from_sb3_zip)")
        desc, tensors = read_sb3_zip(path, activation=meta["desc"]["activation"])
        pol = MlpPolicy(desc["n_in"], desc["n_out"], desc["hidden_pi"], desc["hidden_vf"], desc["activation"],
                        device=venv.batch.device.index if device is None else device, seed=meta["policy_seed"],
                        n_in_vf=desc["n_in_vf"])
        pol.load_state_dict(tensors)
        pol.counter = int(meta["policy_counter"])
        if "curriculum_table.npz" in members:
            from .yaw_table import YawTable
            meta["curriculum"] = dict(meta["curriculum"], targets=YawTable.from_bytes(members["curriculum_table.npz"], venv))
        self = cls(pol, venv, seed=meta["seed"], critic=meta.get("critic"), curriculum=meta.get("curriculum"),
                   normalize=meta.get("normalize"), adaptive_lr=meta.get("adaptive_lr"), **meta["hyper"])   # (no key: written before there was one)
        if self.normalize is not None and "normalize_state.bin" in members:
            self.normalize.load_state(members["normalize_state.bin"])
        if self.curriculum is not None and "curriculum_state.bin" in members:
            self.curriculum.load_state(members["curriculum_state.bin"])
        self._restore(meta, members)
        return self

    def close(self):
        super().close()
        if self._owns_curriculum:
            self.curriculum.close()
        if self._owns_normalize:
            self.normalize.close()
