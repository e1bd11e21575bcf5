"""Learned policies on the device: SB3 ``MlpPolicy`` checkpoints evaluated by the HIP kernel ``k_policy``.

The reference evaluates a stable-baselines3 model on the host (``model.predict(obs, deterministic=...)[0]`` per step,
WindGym/AgentEval.py:179-190; examples/Example 2: ``PPO.load("PPO_2975000")``).  :class:`MlpPolicy` is that model without
stable-baselines3: the actor(-critic) MLP of SB3's default ``MlpPolicy`` (separate actor / critic nets, tanh or ReLU,
state-independent ``log_std``) on CUDA tensors, one kernel launch per ``act()``, and the ``predict()`` protocol so that the
object goes wherever the scripted agents of :mod:`windgym_amd.agents` go.

:func:`read_sb3_zip` is pure host code and NEVER unpickles anything: ``policy.pth`` is read with
``torch.load(weights_only=True)``, ``data`` as plain JSON whose ``":serialized:"`` cloudpickle blobs are not touched.

Flat parameter order (``wg_policy_set_params``, include/windgym_hip.h): actor hidden layers (W ``[out][in]`` then b),
actor head, critic hidden layers, critic head, ``log_std``.

A policy may be SPLIT: its critic maps ``n_in_vf`` inputs, not the actor's ``n_in`` (``wg_policy_create_vf``) — the centralised
critic of multi-agent PPO, which reads the env's flat observation while the actor reads one agent's.  ``desc["n_in_vf"]`` is
``None`` (or absent, as in every dict written before it existed) for the critic on the actor's width.
"""
from __future__ import annotations

import ctypes as C
import io
import json
import re
import zipfile
from typing import NamedTuple

import numpy as np

from .binding import Handle, device_tensor  # noqa: F401  (device_tensor: re-exported, the trainers import it from here)

MAX_HIDDEN = 4


# ----------------------------------------------------------------------------------------------------------------------
# architecture description + flat layout (host only)
# ----------------------------------------------------------------------------------------------------------------------
def make_desc(n_in, n_out, hidden_pi=(64, 64), hidden_vf=(64, 64), activation="tanh", has_log_std=True, n_in_vf=None):
    """Architecture dict; ``hidden_vf=None`` = no critic; ``n_in_vf``: the critic's own input width (``None`` = ``n_in``)."""
    if activation not in ("tanh", "relu"):
        raise ValueError(f"activation must be 'tanh' or 'relu', not {activation!r}")
    if n_in_vf is not None:
        if hidden_vf is None:
            raise ValueError("n_in_vf is the input width of the critic: the policy needs one (hidden_vf is None)")
        if int(n_in_vf) < 1:
            raise ValueError("n_in_vf must be >= 1")
    return dict(n_in=int(n_in), n_out=int(n_out), hidden_pi=tuple(int(h) for h in hidden_pi),
                hidden_vf=None if hidden_vf is None else tuple(int(h) for h in hidden_vf),
                activation=activation, has_log_std=bool(has_log_std), n_in_vf=None if n_in_vf is None else int(n_in_vf))


def critic_width(desc):
    """The critic's input width: ``desc["n_in_vf"]``, or ``n_in`` where it is ``None`` or absent."""
    w = desc.get("n_in_vf")
    return int(desc["n_in"] if w is None else w)


def param_layout(desc):
    """[(SB3 state-dict name, shape)] in flat-vector order."""
    out = []
    k = desc["n_in"]
    for i, h in enumerate(desc["hidden_pi"]):
        out += [(f"mlp_extractor.policy_net.{2 * i}.weight", (h, k)), (f"mlp_extractor.policy_net.{2 * i}.bias", (h,))]
        k = h
    out += [("action_net.weight", (desc["n_out"], k)), ("action_net.bias", (desc["n_out"],))]
    if desc["hidden_vf"] is not None:
        k = critic_width(desc)
        for i, h in enumerate(desc["hidden_vf"]):
            out += [(f"mlp_extractor.value_net.{2 * i}.weight", (h, k)), (f"mlp_extractor.value_net.{2 * i}.bias", (h,))]
            k = h
        out += [("value_net.weight", (1, k)), ("value_net.bias", (1,))]
    if desc["has_log_std"]:
        out.append(("log_std", (desc["n_out"],)))
    return out


def layout_n_params(layout):
    """Floats of a ``[(name, shape)]`` layout (``param_layout`` here, ``recurrent.param_layout``)."""
    return int(sum(int(np.prod(s)) for _, s in layout))


def layout_pack(layout, tensors):
    """{name: array} -> flat float32 vector in the layout's order."""
    parts = []
    for name, shape in layout:
        if name not in tensors:
            raise ValueError(f"missing tensor {name!r}")
        a = np.asarray(tensors[name], dtype=np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(a.shape)}, expected {tuple(shape)}")
        parts.append(a.reshape(-1))
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def layout_unpack(layout, flat):
    """flat vector -> {name: float32 array}."""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    if flat.size != layout_n_params(layout):
        raise ValueError(f"{flat.size} parameters given, the architecture has {layout_n_params(layout)}")
    out, o = {}, 0
    for name, shape in layout:
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].reshape(shape).copy()
        o += n
    return out


def n_params(desc):
    return layout_n_params(param_layout(desc))


def pack_params(desc, tensors):
    """{name: array} -> flat float32 vector."""
    return layout_pack(param_layout(desc), tensors)


def unpack_params(desc, flat):
    """flat vector -> {name: float32 array}."""
    return layout_unpack(param_layout(desc), flat)


# ----------------------------------------------------------------------------------------------------------------------
# SB3 checkpoint reader (host only, no unpickling)
# ----------------------------------------------------------------------------------------------------------------------
def _chain(tensors, prefix, n_in, what):
    idx = sorted({int(m.group(1)) for k in tensors for m in [re.fullmatch(re.escape(prefix) + r"\.(\d+)\.weight", k)] if m})
    hidden, k = [], n_in
    for i in idx:
        w, b = tensors[f"{prefix}.{i}.weight"], tensors.get(f"{prefix}.{i}.bias")
        if b is None:
            raise ValueError(f"missing tensor {prefix}.{i}.bias")
        if w.ndim != 2 or w.shape[1] != k or b.shape != (w.shape[0],):
            raise ValueError(f"{what}: shapes do not chain at {prefix}.{i} (weight {w.shape}, bias {b.shape}, input width {k})")
        hidden.append(int(w.shape[0]))
        k = int(w.shape[0])
    return hidden, k


def _read_policy_pth(path):
    """{name: float32 array} of the ``policy.pth`` of an SB3 / sb3-contrib ``.zip``.  Nothing is unpickled: the tensors by
    ``torch.load(weights_only=True)``, ``data`` as plain JSON (read only to refuse ``use_sde``)."""
    import torch
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
        if "policy.pth" not in names:
            raise ValueError("not an SB3 checkpoint: no policy.pth in the archive")
        if "data" in names:
            data = json.loads(z.read("data").decode())          # plain JSON; ":serialized:" blobs stay strings
            if isinstance(data, dict) and data.get("use_sde") is True:
                raise ValueError("use_sde: true — state-dependent exploration is not supported")
        sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
    return {k: v.detach().cpu().numpy().astype(np.float32) for k, v in sd.items()}


def read_sb3_zip(path, activation="tanh"):
    """-> (desc, {SB3 name: float32 array}) of a stable-baselines3 >= 2.0 ``MlpPolicy`` checkpoint (PPO / A2C ``.zip``).

    The architecture comes from the tensor names and shapes; the activation is not in the tensors (SB3's default: tanh).
    Raises ValueError naming the reason for: ``use_sde``, a shared trunk, a non-flatten feature extractor, missing tensors,
    shapes that do not chain."""
    tensors = _read_policy_pth(path)
    if any(k.startswith("lstm_actor.") for k in tensors):
        raise ValueError("recurrent checkpoint (lstm_actor.* tensors: sb3-contrib's RecurrentPPO): load it with "
                         "MlpLstmPolicy.from_sb3_zip (windgym_amd.recurrent)")
    if any(k.startswith("mlp_extractor.shared_net.") for k in tensors):
        raise ValueError("shared trunk (mlp_extractor.shared_net.*): only separate actor / critic nets are supported")
    if any(k.startswith(("features_extractor.", "pi_features_extractor.", "vf_features_extractor.")) for k in tensors):
        raise ValueError("non-flatten feature extractor (features_extractor.* parameters) is not supported")
    for k in ("action_net.weight", "action_net.bias"):
        if k not in tensors:
            raise ValueError(f"missing tensor {k}")
    aw = tensors["action_net.weight"]
    first = tensors.get("mlp_extractor.policy_net.0.weight", aw)
    n_in, n_out = int(first.shape[1]), int(aw.shape[0])
    hidden_pi, k = _chain(tensors, "mlp_extractor.policy_net", n_in, "actor")
    if aw.shape != (n_out, k) or tensors["action_net.bias"].shape != (n_out,):
        raise ValueError(f"actor: shapes do not chain at action_net (weight {aw.shape}, input width {k})")
    hidden_vf, n_in_vf = None, None
    if "value_net.weight" in tensors:
        if "value_net.bias" not in tensors:
            raise ValueError("missing tensor value_net.bias")
        # the critic's input width is its own first layer's (SB3 itself always writes the actor's; a split policy's differs)
        vfirst = tensors.get("mlp_extractor.value_net.0.weight", tensors["value_net.weight"])
        if vfirst.ndim == 2 and int(vfirst.shape[1]) != n_in:
            n_in_vf = int(vfirst.shape[1])
        hidden_vf, k = _chain(tensors, "mlp_extractor.value_net", n_in if n_in_vf is None else n_in_vf, "critic")
        if tensors["value_net.weight"].shape != (1, k) or tensors["value_net.bias"].shape != (1,):
            raise ValueError(f"critic: shapes do not chain at value_net (weight {tensors['value_net.weight'].shape}, input width {k})")
    elif any(k2.startswith("mlp_extractor.value_net.") for k2 in tensors):
        raise ValueError("missing tensor value_net.weight")
    has_ls = "log_std" in tensors
    if has_ls and tensors["log_std"].shape != (n_out,):
        raise ValueError(f"log_std: shape {tensors['log_std'].shape}, expected ({n_out},)")
    desc = make_desc(n_in, n_out, hidden_pi, hidden_vf, activation, has_ls, n_in_vf)
    return desc, {name: tensors[name] for name, _ in param_layout(desc)}


# ----------------------------------------------------------------------------------------------------------------------
# the device object
# ----------------------------------------------------------------------------------------------------------------------
def refuse_recurrent(policy, who):
    """What the trainers and the wrappers say to a ``recurrent.MlpLstmPolicy`` (or a list holding one): they are not built for it."""
    if any(getattr(p, "recurrent", False) for p in (policy if isinstance(policy, (list, tuple)) else (policy,))):
        raise NotImplementedError(f"{who}: training / wrapping a recurrent policy (MlpLstmPolicy) is not implemented; "
                                  "venv.rollout(policy, T) and eval_sweep run it")


def refuse_table_agent(policy, who):
    """What the trainers, the populations and the wrappers say to a ``yaw_table.YawTableAgent`` (or a list holding one): it is a
    scripted agent with nothing to train, sample or normalise for."""
    if any(getattr(p, "yaw_table_agent", False) for p in (policy if isinstance(policy, (list, tuple)) else (policy,))):
        raise NotImplementedError(f"{who}: a YawTableAgent is a scripted agent, not a policy: this is not implemented for it; "
                                  "venv.rollout(agent, T), AgentEval and eval_sweep run it")


class RolloutActor(NamedTuple):
    """How an object enters the closed loop of ``WindFarmVecEnv.rollout``: every object that method accepts states one, in its
    ``rollout_actor(venv)``, which also makes the object's own refusals of ``venv``."""
    obj: object                 # what acts: its ``act`` / ``value`` stand in under ``sample_site``, its identity keys a kept LSTM state
    entry: str                  # the library's closed-loop entry, and the handles its signature names after the env's
    handles: tuple
    shape: tuple = None         # the (n_in, n_out) it maps; None: it reads no rows
    samples: bool = True        # ``raw`` exists, ``deterministic`` and the noise counter apply ...
    log_std: bool = False       # ... and so does ``logp``, a stochastic rollout is possible
    critic: int = None          # the width of the rows its critic reads (``shape[0]``: the actor's own rows); None: no critic
    lstm: bool = False          # the env keeps an LSTM state pair for it
    members: int = None         # a population: its members, each on an equal share of the envs


def refuse_site(venv, what):
    """What an actor without a Python loop of ``act`` + ``step`` says to an env with ``sample_site``."""
    if venv._site is not None:
        raise NotImplementedError(f"rollout(): {what} with sample_site is not implemented")


def act_buffers(owner, n):
    """The persistent ``(action, raw, logp, value)`` outputs of ``act()`` on ``n`` rows, made once per ``n`` and kept in
    ``owner._out`` (``owner``: a policy or a population — ``torch``, ``device``, ``n_out``)."""
    b = owner._out.get(n)
    if b is None:
        t, f32 = owner.torch, dict(dtype=owner.torch.float32, device=owner.device)
        b = owner._out[n] = (t.zeros((n, owner.n_out), **f32), t.zeros((n, owner.n_out), **f32), t.zeros(n, **f32), t.zeros(n, **f32))
    return b


class MlpPolicy(Handle):
    """SB3's default ``MlpPolicy`` (actor ``n_in -> hidden_pi -> n_out``, critic ``n_in -> hidden_vf -> 1``) on one GPU.
    With ``n_in_vf`` the critic maps ``n_in_vf -> hidden_vf -> 1`` instead (a split policy: ``act()`` evaluates the actor only,
    ``value()`` takes rows of ``n_in_vf``).

    ``params`` is ONE flat float32 CUDA leaf tensor (a torch optimiser can own it); ``state_dict()`` returns views of it
    under SB3's names.  The kernel reads its own packed copy: after changing ``params`` call :meth:`sync`.
    Raises ``WindGymHipError`` without the built library or a GPU — there is no CPU fallback."""

    destroy = "wg_policy_destroy"

    def __init__(self, n_in, n_out, hidden_pi=(64, 64), hidden_vf=(64, 64), activation="tanh", device=None, seed=0,
                 has_log_std=True, n_in_vf=None):
        import torch
        from .binding import ACTV, CPolicyDesc, WindGymHipError, _chk, load_library
        self.desc = make_desc(n_in, n_out, hidden_pi, hidden_vf, activation, has_log_std, n_in_vf)
        if len(self.desc["hidden_pi"]) > MAX_HIDDEN or len(self.desc["hidden_vf"] or ()) > MAX_HIDDEN:
            raise NotImplementedError(f"at most {MAX_HIDDEN} hidden layers per net")
        self.L = load_library()
        if not torch.cuda.is_available():
            raise WindGymHipError("no HIP device visible: MlpPolicy only runs on the GPU (no CPU fallback; the numpy "
                                  "restatement under oracle/ is test-only)")
        self.torch, self._chk = torch, _chk
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        d = CPolicyDesc()
        d.n_in, d.n_out, d.activation = self.desc["n_in"], self.desc["n_out"], ACTV[activation]
        d.n_hidden_pi = len(self.desc["hidden_pi"])
        for i, h in enumerate(self.desc["hidden_pi"]):
            d.hidden_pi[i] = h
        d.n_hidden_vf = -1 if self.desc["hidden_vf"] is None else len(self.desc["hidden_vf"])
        for i, h in enumerate(self.desc["hidden_vf"] or ()):
            d.hidden_vf[i] = h
        d.has_log_std = int(self.desc["has_log_std"])
        h = C.c_void_p()
        if self.desc["n_in_vf"] is None:
            _chk(self.L.wg_policy_create(C.byref(d), self.device_index, C.byref(h)), "wg_policy_create")
        else:
            _chk(self.L.wg_policy_create_vf(C.byref(d), self.desc["n_in_vf"], self.device_index, C.byref(h)), "wg_policy_create_vf")
        self._h = h
        n = C.c_size_t()
        _chk(self.L.wg_policy_n_params(self._h, C.byref(n)), "wg_policy_n_params")
        assert n.value == n_params(self.desc)
        self.n_in, self.n_out, self.has_critic = self.desc["n_in"], self.desc["n_out"], self.desc["hidden_vf"] is not None
        self.n_in_vf = critic_width(self.desc)          # what value() reads
        self.split = self.n_in_vf != self.n_in          # the critic reads other rows than the actor
        # seeded init: N(0, 1 / fan_in) weights, zero biases and log_std (SB3's orthogonal init is a trainer's business)
        rng = np.random.default_rng(seed)
        t = {name: (rng.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32) if len(shape) == 2
             else np.zeros(shape, np.float32) for name, shape in param_layout(self.desc)}
        self.params = torch.from_numpy(pack_params(self.desc, t)).to(self.device).requires_grad_(False)
        self._views = None
        self._out = {}
        self.counter = 0            # running count of stochastic act() calls: no noise is ever reused
        self.seed = int(seed)
        self.sync()

    @classmethod
    def from_sb3_zip(cls, path, activation="tanh", device=None, seed=0):
        desc, tensors = read_sb3_zip(path, activation=activation)
        p = cls(desc["n_in"], desc["n_out"], desc["hidden_pi"], desc["hidden_vf"], activation, device=device, seed=seed,
                has_log_std=desc["has_log_std"], n_in_vf=desc["n_in_vf"])
        p.load_state_dict(tensors)
        return p

    def rollout_actor(self, venv):
        return RolloutActor(self, "wg_rollout", (self._h,), (self.n_in, self.n_out), log_std=self.desc["has_log_std"],
                            critic=self.n_in_vf if self.has_critic else None)

    # -- parameters ---------------------------------------------------------------------------------
    def state_dict(self):
        """{SB3 name: view of ``params``}."""
        out, o = {}, 0
        for name, shape in param_layout(self.desc):
            n = int(np.prod(shape))
            out[name] = self.params.detach()[o:o + n].view(shape)
            o += n
        return out

    def load_state_dict(self, sd):
        flat = pack_params(self.desc, {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else v) for k, v in sd.items()})
        with self.torch.no_grad():
            self.params.copy_(self.torch.from_numpy(flat))
        self.sync()
        return self

    def sync(self):
        """Push ``params`` (device pointer, no host trip) into the kernel's packed copy — after an optimiser step."""
        self._chk(self.L.wg_policy_set_params(self._h, C.c_void_p(self.params.data_ptr()), self.params.numel(), 1,
                                              self._stream()), "wg_policy_set_params")

    def torch_forward(self, obs, obs_vf=None):
        """(mean, value) with ``F.linear`` / tanh on the same parameters — differentiable (a trainer's loss goes through
        it); value is None without a critic.  The critic reads ``obs_vf`` (rows of ``n_in_vf``) when given, else ``obs``; on a
        split policy without ``obs_vf`` there is nothing it could read and value is None."""
        F = self.torch.nn.functional
        act = self.torch.tanh if self.desc["activation"] == "tanh" else F.relu
        views, o = {}, 0
        for name, shape in param_layout(self.desc):
            n = int(np.prod(shape))
            views[name] = self.params[o:o + n].view(shape)
            o += n

        def net(prefix, n_hidden, head, x):
            for i in range(n_hidden):
                x = act(F.linear(x, views[f"{prefix}.{2 * i}.weight"], views[f"{prefix}.{2 * i}.bias"]))
            return F.linear(x, views[head + ".weight"], views[head + ".bias"])

        mean = net("mlp_extractor.policy_net", len(self.desc["hidden_pi"]), "action_net", obs)
        xv = obs_vf if obs_vf is not None else None if self.split else obs
        value = net("mlp_extractor.value_net", len(self.desc["hidden_vf"]), "value_net", xv)[..., 0] if self.has_critic and xv is not None else None
        return mean, value

    # -- evaluation ---------------------------------------------------------------------------------
    def act(self, obs, deterministic=False, counter=None, *, seed=None, row_offset=0, value=True, out=None):
        """ONE launch of k_policy on a contiguous float32 CUDA tensor ``[..., n_in]`` -> persistent ``(action, raw, logp,
        value)`` tensors (rows = the leading dimensions flattened; valid until the next ``act()`` on as many rows; value is
        None without a critic, with ``value=False`` or on a split policy, whose critic reads other rows: :meth:`value`).  No
        synchronisation.  ``counter`` defaults to a running count."""
        t = self.torch
        if not (device_tensor(obs, t.float32) and obs.shape[-1] == self.n_in):
            raise ValueError(f"act(): obs must be a contiguous float32 CUDA tensor [..., {self.n_in}]")
        n = obs.numel() // self.n_in
        a, r, lp, v = out if out is not None else act_buffers(self, n)
        want_v = value and self.has_critic and not self.split
        stochastic = not deterministic
        if counter is None:
            counter = self.counter
            if stochastic:
                self.counter += 1
        ls = self.desc["has_log_std"]
        rc = self.L.wg_policy_act(self._h, n, obs.data_ptr(), int(bool(deterministic)),
                                  self.seed if seed is None else int(seed), int(counter), int(row_offset),
                                  a.data_ptr(), r.data_ptr(), lp.data_ptr() if ls else None,
                                  v.data_ptr() if want_v else None, self._stream())
        if rc:
            self._chk(rc, "wg_policy_act")
        return a, r, (lp if ls else None), (v if want_v else None)

    def value(self, obs, out=None):
        """Critic only: V(obs) on a contiguous float32 CUDA tensor ``[..., n_in_vf]`` -> float32 CUDA tensor [rows]."""
        t = self.torch
        if not self.has_critic:
            raise ValueError("value(): the policy has no critic")
        if self.split and not (device_tensor(obs, t.float32) and obs.shape[-1] == self.n_in_vf):
            raise ValueError(f"value(): obs must be a contiguous float32 CUDA tensor [..., {self.n_in_vf}] (the critic's input width)")
        n = obs.numel() // self.n_in_vf
        v = out if out is not None else t.zeros(n, dtype=t.float32, device=self.device)
        self._chk(self.L.wg_policy_act(self._h, n, obs.data_ptr(), 1, 0, 0, 0, None, None, None, v.data_ptr(),
                                       self._stream()), "wg_policy_act")
        return v

    def predict(self, obs, state=None, episode_start=None, deterministic=False):
        """stable-baselines3's protocol: numpy or tensor, ``[O]`` or ``[B, O]`` -> ``(numpy action, None)``."""
        t = self.torch
        x = obs if isinstance(obs, t.Tensor) else t.from_numpy(np.ascontiguousarray(obs, dtype=np.float32))
        single = x.ndim == 1
        x = x.to(self.device, dtype=t.float32).reshape(-1, self.n_in).contiguous()
        a = self.act(x, deterministic=deterministic, value=False)[0]
        a = a.detach().cpu().numpy().copy()
        return (a[0] if single else a), None
