"""Recurrent policies on the device: sb3-contrib's ``MlpLstmPolicy`` (``RecurrentPPO``) evaluated by the HIP kernels ``k_lstm``
and ``k_policy``.

Wake steering is partially observed: a yaw change reaches the turbine behind it only after the wake has advected there, tens of
env steps later, and the reference's own trainer puts an ``nn.LSTM`` in front of its actor and critic for that reason
(examples/curriculum.py:109-146).  :class:`MlpLstmPolicy` is that model without sb3-contrib:

* two one-layer LSTMs of hidden size ``H``, ``lstm_actor`` and ``lstm_critic`` (``n_in -> H``), or ONE with ``shared_lstm=True``
  (the critic's MLP then reads the actor's ``h'``);
* behind them SB3's MLP actor-critic on the hidden rows: actor ``H -> hidden_pi... -> n_out``, critic ``H -> hidden_vf... -> 1``,
  and a state-independent ``log_std`` — an ordinary :class:`windgym_amd.policy.MlpPolicy` of ``H`` inputs (``.mlp``).

The cell is ``torch.nn.LSTM``'s, gate order ``i, f, g, o``::

    (h, c) <- (0, 0) for rows with episode_start = 1
    z  = W_ih x + b_ih + W_hh h + b_hh
    c' = sigmoid(z_f) c + sigmoid(z_i) tanh(z_g);   h' = sigmoid(z_o) tanh(c')

The episode-start mask is a SELECT: such a row does not depend on its incoming state at all, also where that state holds NaN.
sb3-contrib multiplies the state by ``1 - episode_start``; for finite states the two agree.

Not supported, refused by name: ``n_lstm_layers > 1``, the Linear critic of ``enable_critic_lstm=False`` without ``shared_lstm``,
feature extractors, ``use_sde``.  Limits: ``n_in <= 2048``, ``1 <= H <= 256``.  Training is ``recurrent_ppo.RecurrentPPO``
(backpropagation through time in HIP, wg_lstm_ppo.hip) on what ``venv.rollout`` records for it (``lstm_state0``, ``episode_start``);
``torch_forward`` is the differentiable restatement an eager-torch trainer goes through.

A STATE is one float32 CUDA tensor ``[nets, 2, n, H]`` (per net ``h`` then ``c``; nets = 2, or 1 with ``shared_lstm``) — the layout
of ``wg_lstm_step``.  Flat parameter order: per LSTM (the actor's first) ``weight_ih_l0 [4H, n_in]``, ``weight_hh_l0 [4H, H]``,
``bias_ih_l0 [4H]``, ``bias_hh_l0 [4H]``, then the MLP's parameters in ``policy.param_layout`` order.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import policy as _mlp
from .binding import Handle

MAX_IN, MAX_H = 2048, 256


# ----------------------------------------------------------------------------------------------------------------------
# architecture description + flat layout (host only)
# ----------------------------------------------------------------------------------------------------------------------
def make_lstm_desc(n_in, n_out, lstm_hidden_size=256, hidden_pi=(64, 64), hidden_vf=(64, 64), shared_lstm=False, activation="tanh"):
    """Architecture dict: ``n_in``, ``n_out``, ``hidden`` (H), ``shared_lstm``, ``nets`` and ``mlp`` (``policy.make_desc`` of the MLP
    on the hidden rows).  ``has_log_std`` is always true."""
    n_in, H = int(n_in), int(lstm_hidden_size)
    if n_in < 1 or H < 1:
        raise ValueError("n_in and lstm_hidden_size must be >= 1")
    if n_in > MAX_IN:
        raise NotImplementedError(f"n_in = {n_in} > {MAX_IN}")
    if H > MAX_H:
        raise NotImplementedError(f"lstm_hidden_size = {H} > {MAX_H}")
    if hidden_vf is None:
        raise ValueError("a recurrent policy has a critic: hidden_vf must not be None")
    mlp = _mlp.make_desc(H, n_out, hidden_pi, hidden_vf, activation, True)
    if len(mlp["hidden_pi"]) > _mlp.MAX_HIDDEN or len(mlp["hidden_vf"]) > _mlp.MAX_HIDDEN:
        raise NotImplementedError(f"at most {_mlp.MAX_HIDDEN} hidden layers per net")
    return dict(n_in=n_in, n_out=int(n_out), hidden=H, shared_lstm=bool(shared_lstm), nets=1 if shared_lstm else 2, mlp=mlp,
                activation=activation, has_log_std=True)


def lstm_layout(desc):
    """[(sb3-contrib state-dict name, shape)] of the LSTM parameters in flat-vector order."""
    H, n_in, out = desc["hidden"], desc["n_in"], []
    for net in ("lstm_actor", "lstm_critic")[:desc["nets"]]:
        out += [(f"{net}.weight_ih_l0", (4 * H, n_in)), (f"{net}.weight_hh_l0", (4 * H, H)),
                (f"{net}.bias_ih_l0", (4 * H,)), (f"{net}.bias_hh_l0", (4 * H,))]
    return out


def param_layout(desc):
    """[(name, shape)] of ALL parameters in flat-vector order: the LSTMs', then the MLP's."""
    return lstm_layout(desc) + _mlp.param_layout(desc["mlp"])


def n_params(desc):
    return _mlp.layout_n_params(param_layout(desc))


def pack_params(desc, tensors):
    """{name: array} -> flat float32 vector."""
    return _mlp.layout_pack(param_layout(desc), tensors)


def unpack_params(desc, flat):
    """flat vector -> {name: float32 array}."""
    return _mlp.layout_unpack(param_layout(desc), flat)


# ----------------------------------------------------------------------------------------------------------------------
# sb3-contrib RecurrentPPO checkpoint reader (host only, no unpickling)
# ----------------------------------------------------------------------------------------------------------------------
def read_sb3_lstm_zip(path, activation="tanh"):
    """-> (desc, {sb3-contrib name: float32 array}) of a ``RecurrentPPO`` ``MlpLstmPolicy`` checkpoint (``.zip``).

    Nothing is unpickled (``policy.pth`` by ``torch.load(weights_only=True)``, ``data`` as plain JSON).  The architecture comes from
    the tensor names and shapes; the activation is not in the tensors (default: tanh).  Raises ValueError naming the reason for:
    more than one LSTM layer, the Linear critic of ``enable_critic_lstm=False``, a feature extractor, ``use_sde``, a shared MLP
    trunk, missing tensors, shapes that do not chain."""
    tensors = _mlp._read_policy_pth(path)
    if not any(k.startswith("lstm_actor.") for k in tensors):
        raise ValueError("not a recurrent checkpoint: no lstm_actor.* tensors (an MlpPolicy zip loads with MlpPolicy.from_sb3_zip)")
    for net in ("lstm_actor", "lstm_critic"):
        if any(k.startswith(f"{net}.") and k.endswith("_l1") for k in tensors):
            raise ValueError(f"n_lstm_layers > 1 ({net}.weight_ih_l1): only one-layer LSTMs are supported")
    if any(k.startswith(("features_extractor.", "pi_features_extractor.", "vf_features_extractor.")) for k in tensors):
        raise ValueError("non-flatten feature extractor (features_extractor.* parameters) is not supported")
    if any(k.startswith("mlp_extractor.shared_net.") for k in tensors):
        raise ValueError("shared trunk (mlp_extractor.shared_net.*): only separate actor / critic nets are supported")
    has_critic_lstm = any(k.startswith("lstm_critic.") for k in tensors)
    if not has_critic_lstm and "critic.weight" in tensors:
        raise ValueError("Linear critic (critic.weight without lstm_critic.*: enable_critic_lstm=False) is not supported: "
                         "the critic needs an LSTM of its own or shared_lstm=True")
    for k in ("lstm_actor.weight_ih_l0", "lstm_actor.weight_hh_l0", "action_net.weight", "action_net.bias", "value_net.weight",
              "value_net.bias", "log_std"):
        if k not in tensors:
            raise ValueError(f"missing tensor {k}")
    wih, whh = tensors["lstm_actor.weight_ih_l0"], tensors["lstm_actor.weight_hh_l0"]
    if wih.ndim != 2 or whh.ndim != 2 or whh.shape[0] != 4 * whh.shape[1] or wih.shape[0] != whh.shape[0]:
        raise ValueError(f"lstm_actor: shapes do not chain (weight_ih_l0 {wih.shape}, weight_hh_l0 {whh.shape})")
    n_in, H, n_out = int(wih.shape[1]), int(whh.shape[1]), int(tensors["action_net.weight"].shape[0])
    hidden_pi, k = _mlp._chain(tensors, "mlp_extractor.policy_net", H, "actor")
    if tensors["action_net.weight"].shape != (n_out, k) or tensors["action_net.bias"].shape != (n_out,):
        raise ValueError(f"actor: shapes do not chain at action_net (weight {tensors['action_net.weight'].shape}, input width {k})")
    hidden_vf, k = _mlp._chain(tensors, "mlp_extractor.value_net", H, "critic")
    if tensors["value_net.weight"].shape != (1, k) or tensors["value_net.bias"].shape != (1,):
        raise ValueError(f"critic: shapes do not chain at value_net (weight {tensors['value_net.weight'].shape}, input width {k})")
    if tensors["log_std"].shape != (n_out,):
        raise ValueError(f"log_std: shape {tensors['log_std'].shape}, expected ({n_out},)")
    desc = make_lstm_desc(n_in, n_out, H, hidden_pi, hidden_vf, not has_critic_lstm, activation)
    for name, shape in lstm_layout(desc):
        if name not in tensors:
            raise ValueError(f"missing tensor {name}")
        if tuple(tensors[name].shape) != tuple(shape):
            raise ValueError(f"{name}: shapes do not chain (shape {tuple(tensors[name].shape)}, expected {tuple(shape)})")
    return desc, {name: tensors[name] for name, _ in param_layout(desc)}


# ----------------------------------------------------------------------------------------------------------------------
# the device object
# ----------------------------------------------------------------------------------------------------------------------
class MlpLstmPolicy(Handle):
    """sb3-contrib's ``MlpLstmPolicy`` on one GPU (module docstring).  ``params`` is ONE flat float32 CUDA tensor: the LSTM parameters,
    then the MLP's in ``policy.param_layout`` order; ``state_dict()`` returns views of it under sb3-contrib's names.  The kernels
    read packed copies: after changing ``params`` call :meth:`sync`.  Raises ``WindGymHipError`` without the built library or a
    GPU — there is no CPU fallback."""

    recurrent = True            # what rollout / the trainers / the wrappers look at
    split = False
    has_critic = True

    def __init__(self, n_in, n_out, lstm_hidden_size=256, hidden_pi=(64, 64), hidden_vf=(64, 64), shared_lstm=False, activation="tanh",
                 device=None, seed=0):
        import torch
        from .binding import CLstmDesc, WindGymHipError, _chk, load_library
        self.desc = make_lstm_desc(n_in, n_out, lstm_hidden_size, hidden_pi, hidden_vf, shared_lstm, activation)
        self.L = load_library()
        if not torch.cuda.is_available():
            raise WindGymHipError("no HIP device visible: MlpLstmPolicy only runs on the GPU (no CPU fallback; the numpy "
                                  "restatement under tests/ is test-only)")
        self.torch, self._chk = torch, _chk
        self.n_in, self.n_out, self.H, self.nets = self.desc["n_in"], self.desc["n_out"], self.desc["hidden"], self.desc["nets"]
        self.shared_lstm = self.desc["shared_lstm"]
        # the MLP on the hidden rows: an ordinary MlpPolicy whose parameters become a view of this object's flat vector
        m = self.desc["mlp"]
        self.mlp = _mlp.MlpPolicy(self.H, self.n_out, m["hidden_pi"], m["hidden_vf"], activation, device=device, seed=seed)
        self.device_index, self.device = self.mlp.device_index, self.mlp.device
        d = CLstmDesc(self.n_in, self.H, self.nets)
        h = C.c_void_p()
        _chk(self.L.wg_lstm_create(C.byref(d), self.device_index, C.byref(h)), "wg_lstm_create")
        self._lstm = h
        n = C.c_size_t()
        _chk(self.L.wg_lstm_n_params(self._lstm, C.byref(n)), "wg_lstm_n_params")
        self.n_lstm_params = int(n.value)
        assert self.n_lstm_params + self.mlp.params.numel() == n_params(self.desc)
        # seeded init: torch.nn.LSTM's U(-1 / sqrt(H), 1 / sqrt(H)) for every LSTM tensor; the MLP's is MlpPolicy's
        rng = np.random.default_rng([int(seed), 0x4C53544D])
        k = 1.0 / np.sqrt(self.H)
        lstm0 = np.concatenate([rng.uniform(-k, k, size=int(np.prod(s))).astype(np.float32) for _, s in lstm_layout(self.desc)])
        self.params = torch.cat([torch.from_numpy(lstm0).to(self.device), self.mlp.params]).contiguous().requires_grad_(False)
        self.mlp.params = self.params[self.n_lstm_params:]
        self._out = {}
        self._h = {}                # act()'s h' rows [2, n, H] by n
        self.counter = 0            # running count of stochastic act() calls: no noise is ever reused
        self.seed = int(seed)
        self.sync()

    @classmethod
    def from_sb3_zip(cls, path, activation="tanh", device=None, seed=0):
        desc, tensors = read_sb3_lstm_zip(path, activation=activation)
        m = desc["mlp"]
        p = cls(desc["n_in"], desc["n_out"], desc["hidden"], m["hidden_pi"], m["hidden_vf"], desc["shared_lstm"], activation,
                device=device, seed=seed)
        p.load_state_dict(tensors)
        return p

    # -- lifetime -----------------------------------------------------------------------------------
    destroy, handle_attr = "wg_lstm_destroy", "_lstm"      # (``_h`` holds act()'s h' rows here)

    def close(self):
        super().close()
        if getattr(self, "mlp", None) is not None:
            self.mlp.close()

    def rollout_actor(self, venv):
        _mlp.refuse_site(venv, "a recurrent policy")
        return _mlp.RolloutActor(self, "wg_rollout_lstm", (self._lstm, self.mlp._h), (self.n_in, self.n_out), log_std=True, critic=self.n_in, lstm=True)

    # -- parameters ---------------------------------------------------------------------------------
    def _views(self, params):
        out, o = {}, 0
        for name, shape in param_layout(self.desc):
            n = int(np.prod(shape))
            out[name] = params[o:o + n].view(shape)
            o += n
        return out

    def state_dict(self):
        """{sb3-contrib name: view of ``params``}."""
        return self._views(self.params.detach())

    def load_state_dict(self, sd):
        flat = pack_params(self.desc, {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else v) for k, v in sd.items()})
        with self.torch.no_grad():
            self.params.copy_(self.torch.from_numpy(flat))
        self.sync()
        return self

    def sync(self):
        """Push ``params`` (device pointer, no host trip) into the kernels' packed copies."""
        self._chk(self.L.wg_lstm_set_params(self._lstm, C.c_void_p(self.params.data_ptr()), self.n_lstm_params, 1, self._stream()),
                  "wg_lstm_set_params")
        self.mlp.sync()

    def initial_state(self, n):
        """The zero state of ``n`` rows: float32 CUDA ``[nets, 2, n, H]``."""
        return self.torch.zeros((self.nets, 2, int(n), self.H), dtype=self.torch.float32, device=self.device)

    def torch_forward(self, obs, state, episode_start=None):
        """``(mean, value, new_state)`` with ``F.linear`` / sigmoid / tanh on the same parameters — differentiable (a trainer's loss
        goes through it).  ``obs [n, n_in]``, ``state [nets, 2, n, H]``, ``episode_start [n]`` (bool / uint8) or None."""
        t = self.torch
        F = t.nn.functional
        v = self._views(self.params)
        fresh = None if episode_start is None else episode_start.reshape(-1, 1).to(t.bool)
        hs, new = [], []
        for i, net in enumerate(("lstm_actor", "lstm_critic")[:self.nets]):
            h, c = state[i, 0], state[i, 1]
            if fresh is not None:
                h, c = t.where(fresh, t.zeros_like(h), h), t.where(fresh, t.zeros_like(c), c)
            z = F.linear(obs, v[f"{net}.weight_ih_l0"], v[f"{net}.bias_ih_l0"]) + F.linear(h, v[f"{net}.weight_hh_l0"], v[f"{net}.bias_hh_l0"])
            zi, zf, zg, zo = z.chunk(4, dim=-1)
            cn = t.sigmoid(zf) * c + t.sigmoid(zi) * t.tanh(zg)
            hn = t.sigmoid(zo) * t.tanh(cn)
            hs.append(hn)
            new.append(t.stack([hn, cn]))
        mean, value = self.mlp.torch_forward(hs[0], obs_vf=hs[-1])
        return mean, value, t.stack(new)

    # -- evaluation ---------------------------------------------------------------------------------
    def _check_rows(self, what, obs, state, episode_start):
        t = self.torch
        if not (_mlp.device_tensor(obs, t.float32) and obs.ndim == 2 and obs.shape[1] == self.n_in):
            raise ValueError(f"{what}: obs must be a contiguous float32 CUDA tensor [n, {self.n_in}]")
        n = obs.shape[0]
        if not (_mlp.device_tensor(state, t.float32) and tuple(state.shape) == (self.nets, 2, n, self.H)):
            raise ValueError(f"{what}: state must be a contiguous float32 CUDA tensor [{self.nets}, 2, {n}, {self.H}]")
        if episode_start is not None and not (_mlp.device_tensor(episode_start, t.uint8) and episode_start.numel() == n):
            raise ValueError(f"{what}: episode_start must be a contiguous uint8 CUDA tensor [{n}] (or None)")
        return n

    def act(self, obs, state, episode_start=None, deterministic=False, counter=None, *, seed=None, row_offset=0, value=True, out=None,
            state_out=None):
        """TWO launches (k_lstm, k_policy) on ``obs [n, n_in]``, ``state [nets, 2, n, H]`` and ``episode_start`` (uint8 ``[n]`` or None:
        no row starts an episode) -> ``((action, raw, logp, value), new_state)``.  The outputs are persistent tensors, valid until
        the next ``act()`` on as many rows; ``new_state`` is a new tensor, or ``state_out`` when given (it may be ``state``: in
        place).  With ``value=False`` the critic's LSTM is not evaluated and its planes of ``new_state`` are not written.  No
        synchronisation.  ``counter`` defaults to a running count."""
        t = self.torch
        n = self._check_rows("act()", obs, state, episode_start)
        if state_out is None:
            state_out = t.zeros_like(state)
        elif not (_mlp.device_tensor(state_out, t.float32) and state_out.shape == state.shape):
            raise ValueError("act(): state_out must be a contiguous float32 CUDA tensor of state's shape")
        a, r, lp, v = out if out is not None else _mlp.act_buffers(self, n)
        hbuf = self._h.get(n)
        if hbuf is None:
            hbuf = self._h[n] = t.zeros((2, n, self.H), dtype=t.float32, device=self.device)
        if counter is None:
            counter = self.counter
            if not deterministic:
                self.counter += 1
        self._chk(self.L.wg_lstm_act(self._lstm, self.mlp._h, n, obs.data_ptr(), None if episode_start is None else episode_start.data_ptr(),
                                     state.data_ptr(), state_out.data_ptr(), hbuf.data_ptr(), int(bool(deterministic)),
                                     self.seed if seed is None else int(seed), int(counter), int(row_offset), a.data_ptr(), r.data_ptr(),
                                     lp.data_ptr(), v.data_ptr() if value else None, self._stream()), "wg_lstm_act")
        return (a, r, lp, (v if value else None)), state_out

    def predict(self, obs, state=None, episode_start=None, deterministic=False):
        """sb3-contrib's protocol: numpy or tensor ``[O]`` / ``[B, O]`` -> ``(numpy action, (h, c))`` with ``h``, ``c`` numpy
        ``[1, B, H]``: the ACTOR's state, as sb3-contrib returns it (the critic's LSTM is not evaluated).  ``state=None`` means
        zeros, ``episode_start=None`` that no env restarted."""
        t = self.torch
        x = obs if isinstance(obs, t.Tensor) else t.from_numpy(np.ascontiguousarray(obs, dtype=np.float32))
        single = x.ndim == 1
        x = x.to(self.device, dtype=t.float32).reshape(-1, self.n_in).contiguous()
        n = x.shape[0]
        full = self.initial_state(n)
        if state is not None:
            h, c = state
            for j, s in enumerate((h, c)):
                s = np.asarray(s, dtype=np.float32)
                if s.shape != (1, n, self.H):
                    raise ValueError(f"predict(): state must be (h, c), each [1, {n}, {self.H}]")
                full[0, j].copy_(t.from_numpy(np.ascontiguousarray(s[0])))
        es = None
        if episode_start is not None:
            es = t.from_numpy(np.ascontiguousarray(np.asarray(episode_start).reshape(-1) != 0).astype(np.uint8)).to(self.device)
            if es.numel() != n:
                raise ValueError(f"predict(): episode_start must have {n} entries")
        (a, _, _, _), new = self.act(x, full, es, deterministic=deterministic, value=False, state_out=full)
        a = a.detach().cpu().numpy().copy()
        hc = new[0].detach().cpu().numpy()
        return (a[0] if single else a), (hc[0][None].copy(), hc[1][None].copy())
