"""Yaw table: the Serial-Refine optimiser's yaws on a grid of wind conditions, computed once and looked up on the device.

The steady-state yaw optimiser (k_steady_srf, ``HipBatch.steady_optimize``) is the project's expert: the baseline a learned policy is
compared with, the target of ``curriculum.YawCurriculum`` and the teacher of ``imitation.BehaviorCloning``.  A :class:`YawTable`
holds its answers on a grid over (TI, wind speed, wind direction) — what a wind-farm operator runs for wake steering — so that
nothing is optimised at run time:

    table = YawTable.build(venv)                               # once: one Serial-Refine launch per chunk of node winds
    out = venv.rollout(YawTableAgent(table, env=venv), 128)    # the table as a scripted agent in the closed loop (wg_rollout_table)
    cur = YawCurriculum(venv, ..., targets=table)              # the curriculum's targets without the per-rollout optimisation
    bc = BehaviorCloning("MlpPolicy", venv, expert=table)      # ... and behaviour cloning's

**The lookup takes the nearest node of every axis; it does not interpolate.**  A Serial-Refine optimum is an argmax over discrete
candidates and is not continuous in the wind: halfway between a node whose answer is +25 degrees and one whose answer is -25
degrees the interpolated answer is 0 degrees, the worst of the three.  The rule for one axis with nodes ``a_0 < ... < a_{n-1}`` and
a value ``x``, in float64: the index is the number of midpoints ``(a_k + a_{k+1}) / 2`` below ``x`` — a tie goes to the lower
node, ``x`` outside the axis to the end node; ``row = (i_ti * n_ws + i_ws) * n_wd + i_wd``; a non-finite wind has row -1.  With
``wrap_wd=True`` (the caller's statement that the ``wd`` axis covers the full circle) ``x`` is first reduced to ``[a_0, a_0 + 360)``
and a virtual node ``a_0 + 360`` maps to index 0.  windgym_amd/csrc/wg_yaw_table.h is the one statement of the rule.

The table itself needs no device (:meth:`YawTable.save`, the checks); its lookups need the built library and a GPU.
"""
from __future__ import annotations

import io
import json

import numpy as np

from .agents import BaseAgent
from .policy import RolloutActor, refuse_site

MAX_NODES = 1024          # WG_YT_MAX_NODES: nodes of the three axes together
CHUNK = 8192              # node winds per Serial-Refine launch of build()


def default_axis(lo, hi, step):
    """Nodes over ``[lo, hi]`` with both ends and a spacing of at most ``step``; a degenerate range gives one node."""
    lo, hi = float(lo), float(hi)
    if not hi > lo:
        return np.array([lo], dtype=np.float64)
    return np.linspace(lo, hi, int(np.ceil((hi - lo) / float(step) - 1e-9)) + 1, dtype=np.float64)


def check_axes(ti, ws, wd, wrap_wd=False):
    """The three axes as float64 arrays, or ``ValueError`` naming the argument: empty, not one-dimensional, not finite, not strictly
    ascending, more than ``MAX_NODES`` nodes together, ``wrap_wd`` on a ``wd`` axis spanning 360 degrees or more."""
    out = []
    for name, a in (("ti", ti), ("ws", ws), ("wd", wd)):
        a = np.array(a, dtype=np.float64)
        if a.ndim != 1 or a.size < 1:
            raise ValueError(f"{name}: an axis is a non-empty one-dimensional array of nodes, got shape {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"{name}: the nodes must be finite")
        if not (np.diff(a) > 0).all():
            raise ValueError(f"{name}: the nodes must be strictly ascending")
        out.append(a)
    if sum(a.size for a in out) > MAX_NODES:
        raise ValueError(f"ti / ws / wd: {sum(a.size for a in out)} nodes together, the lookup kernels stage at most {MAX_NODES}")
    if wrap_wd and not out[2][-1] - out[2][0] < 360.0:
        raise ValueError(f"wrap_wd: wd spans {out[2][-1] - out[2][0]} degrees; an axis that wraps must span less than 360 "
                         "(its first node returns as wd[0] + 360)")
    return tuple(out)


def node_winds(ti, ws, wd):
    """The wind of every row of a table over these axes, float64 ``[C, 3]`` (ws, wd, ti), in row order (``ti`` slowest)."""
    ti, ws, wd = np.meshgrid(ti, ws, wd, indexing="ij")
    return np.stack([ws.reshape(-1), wd.reshape(-1), ti.reshape(-1)], axis=1)


class YawTable:
    """``yaw [C, N]`` (float64 degrees) and ``power [C]`` (the optimiser's farm power) on the nodes of ``ti`` x ``ws`` x ``wd``
    (``ti`` slowest, ``wd`` fastest; ``C = n_ti * n_ws * n_wd``) — the module docstring states the lookup.  Make one with
    :meth:`build` or :meth:`load`.  With ``venv`` the table lives on that env's device (``yaw`` / ``power`` are CUDA tensors, the
    lookups work); without, it is a host object that can be inspected and saved.

    ``rows(wind, mask=None)``: int32 rows of ``wind [..., 3]`` (float64 CUDA: ws, wd, ti — the layout of the info ``wind_f64``), -1
    where ``mask`` is 0 or the wind is not finite; with ``wind = out["wind_f64"]`` and ``mask = out["truncated"]`` of a rollout that
    is the ``ep_row`` of wg_curriculum_shape / wg_expert_labels, whose ``ep_target`` is ``yaw``.  ``targets(wind)``: the yaws
    ``[..., N]`` of every wind's row.  Both are one launch and synchronise nothing.

    ``ValueError`` naming the argument: what :func:`check_axes` refuses, ``yaw`` not ``[C, N]``, ``power`` not ``[C]``, ``venv``
    with another turbine count than ``yaw``'s."""

    def __init__(self, ti, ws, wd, yaw, power=None, wrap_wd=False, args=None, venv=None):
        self.ti, self.ws, self.wd = check_axes(ti, ws, wd, wrap_wd)
        self.wrap_wd = bool(wrap_wd)
        self.args = dict(args or {})
        C = self.ti.size * self.ws.size * self.wd.size
        shape = tuple(yaw.shape)
        if len(shape) != 2 or shape[0] != C or shape[1] < 1:
            raise ValueError(f"yaw: expected [{C}, N] (one row per node of ti x ws x wd), got {list(shape)}")
        if power is not None and tuple(power.shape) != (C,):
            raise ValueError(f"power: expected [{C}], got {list(power.shape)}")
        self.n_rows, self.N = C, int(shape[1])
        self.yaw, self.power = yaw, power
        self.device, self._tab = None, None
        if venv is not None:
            self._to_device(venv)

    def _to_device(self, venv):
        from .binding import YawTableHandle
        b = getattr(venv, "batch", None)
        if b is None:
            raise ValueError("venv: a YawTable lives on the device of a WindFarmVecEnv / WindFarmVecEnvMulti (or anything with a .batch)")
        if int(b.N) != self.N:
            raise ValueError(f"venv: the table holds yaws of {self.N} turbines, this env has {int(b.N)}")
        t = b.torch
        up = lambda a: (a if t.is_tensor(a) else t.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).to(b.device, t.float64).contiguous()  # noqa: E731
        self.yaw = up(self.yaw)
        self.power = None if self.power is None else up(self.power)
        self.device, self.torch = b.device, t
        self._tab = YawTableHandle(t, b.device, self.ti, self.ws, self.wd, self.wrap_wd, self.yaw)

    def close(self):
        if self._tab is not None:
            self._tab.close()
            self._tab = None

    def _handle(self, who):
        if self._tab is None:
            raise ValueError(f"{who}: this table is not on a device (YawTable.build(venv) / YawTable.load(path, venv))")
        return self._tab

    def check_env(self, venv, who):
        """``ValueError`` naming ``table`` unless the table can serve ``venv``: on its device, for its turbine count."""
        tab, b = self._handle(who), venv.batch
        if self.N != int(b.N):
            raise ValueError(f"{who}: table holds yaws of {self.N} turbines, the env has {int(b.N)}")
        if self.device != b.device:
            raise ValueError(f"{who}: table lives on {self.device}, the env on {b.device}")
        return tab

    # -- lookups ----------------------------------------------------------------------------------------------------
    def rows(self, wind, mask=None, out=None):
        return self._handle("rows()").rows(wind, mask, out)

    def targets(self, wind, out=None):
        return self._handle("targets()").targets(wind, out)

    def node_winds(self):
        """The wind of every row, float64 ``[C, 3]`` (ws, wd, ti) on the host, in row order."""
        return node_winds(self.ti, self.ws, self.wd)

    # -- construction -----------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, venv, ws=None, wd=None, ti=None, model="blondel_jimenez", refine_pass_n=8, yaw_n=9, search_yaw_max=30.0, wrap_wd=False):
        """The table of ``venv``'s farm: row r is, bit for bit, what ``venv.batch.steady_optimize`` returns for node r's wind (that
        call's own +1e-3 degrees on ``wd`` included) — nothing new is computed, the nodes go through the optimiser in chunks.  The
        axes default to the env's sampling ranges (``ws_min .. ws_max`` every 1 m/s, ``wd_min .. wd_max`` every degree, ``TI_min``,
        the middle and ``TI_max``; a degenerate range gives one node)."""
        from .steady import MODEL_IDS
        if model not in MODEL_IDS:
            raise ValueError(f"model must be one of {sorted(MODEL_IDS)}, not {model!r}")
        b, c = venv.batch, venv.cfg
        ws = default_axis(c.ws_min, c.ws_max, 1.0) if ws is None else ws
        wd = default_axis(c.wd_min, c.wd_max, 1.0) if wd is None else wd
        ti = default_axis(c.TI_min, c.TI_max, 0.5 * (float(c.TI_max) - float(c.TI_min))) if ti is None else ti
        ti, ws, wd = check_axes(ti, ws, wd, wrap_wd)
        args = dict(model=model, refine_pass_n=int(refine_pass_n), yaw_n=int(yaw_n), search_yaw_max=float(search_yaw_max))
        w = node_winds(ti, ws, wd)
        t = b.torch
        yaws, powers = [], []
        for lo in range(0, len(w), CHUNK):
            y, p = b.steady_optimize(w[lo:lo + CHUNK, 0], w[lo:lo + CHUNK, 1], w[lo:lo + CHUNK, 2], model=model, refine_pass_n=refine_pass_n,
                                     yaw_n=yaw_n, yaw_max=search_yaw_max)
            yaws.append(y)
            powers.append(p)
        return cls(ti, ws, wd, t.cat(yaws).contiguous(), t.cat(powers).contiguous(), wrap_wd=wrap_wd, args=args, venv=venv)

    # -- persistence ------------------------------------------------------------------------------------------------
    def arrays(self):
        """The table as host arrays (what :meth:`save` writes and the trainers' checkpoints embed)."""
        host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()      # noqa: E731
        d = dict(ti=self.ti, ws=self.ws, wd=self.wd, yaw=np.ascontiguousarray(host(self.yaw), dtype=np.float64),
                 meta=np.array(json.dumps(dict(wrap_wd=self.wrap_wd, args=self.args))))
        if self.power is not None:
            d["power"] = np.ascontiguousarray(host(self.power), dtype=np.float64)
        return d

    def save(self, path):
        """An npz of the axes, the yaws, the power and the arguments (a JSON string): no pickle."""
        with open(path, "wb") as f:          # (a file object: np.savez would append ".npz" to a name without it)
            np.savez(f, **self.arrays())
        return path

    def to_bytes(self):
        """The file of :meth:`save` as bytes (what the trainers' checkpoints embed)."""
        f = io.BytesIO()
        np.savez(f, **self.arrays())
        return f.getvalue()

    @classmethod
    def from_bytes(cls, blob, venv=None):
        return cls.load(io.BytesIO(blob), venv)

    @classmethod
    def load(cls, path, venv=None):
        """A :meth:`save` file, on ``venv``'s device (``None``: a host table).  Nothing in the file is unpickled."""
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("ti", "ws", "wd", "yaw", "meta") if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a YawTable file (no {missing[0]})")
            meta = json.loads(str(z["meta"]))
            return cls(z["ti"], z["ws"], z["wd"], z["yaw"], z["power"] if "power" in z.files else None, wrap_wd=meta["wrap_wd"],
                       args=meta["args"], venv=venv)


class YawTableAgent(BaseAgent):
    """The table as a scripted agent for a whole batch of envs (``WindFarmVecEnv``): ``predict`` is ONE launch of k_yaw_table_act,
    which reads every env's CURRENT wind and yaws on the device, looks the row up and writes the action that moves the farm
    towards the table's yaws as fast as the env's actuation rule allows (wg_expert_labels' action, both action methods) — no host
    synchronisation, and nothing to do at an autoreset: the lookup is repeated every step.  ``venv.rollout(agent, T)`` runs the
    closed loop inside the library (wg_rollout_table).  ``UseEnv``: ``eval_sweep`` / ``AgentEval`` bind it to their env.  The
    actions are a CUDA tensor ``[B, N]`` (reused by the next ``predict``) unless the env works on numpy arrays."""

    yaw_table_agent = True

    def __init__(self, table, env=None, yaw_max=45, yaw_min=-45):
        super().__init__(yaw_max, yaw_min)
        if not isinstance(table, YawTable):
            raise ValueError("table must be a YawTable")
        self.UseEnv = True
        self.table, self.env = table, env
        self._out = None

    def rollout_actor(self, venv):
        refuse_site(venv, "a YawTableAgent")
        return RolloutActor(self, "wg_rollout_table", (self.table.check_env(venv, "rollout()")._h,), samples=False)

    def _batch(self):
        if self.env is None:
            raise ValueError("YawTableAgent needs an env (env=, or eval_sweep binds it)")
        b = getattr(self.env, "batch", None)
        return b if b is not None else getattr(self.env, "_batch")

    def predict(self, *args, **kwargs):
        b = self._batch()
        if int(b.N) != self.table.N or self.table.device != b.device:
            raise ValueError(f"YawTableAgent: table holds yaws of {self.table.N} turbines on {self.table.device}, the env has {int(b.N)} on {b.device}")
        if self._out is None or self._out.device != b.device or tuple(self._out.shape) != (b.B, b.N):
            self._out = b.torch.zeros((b.B, b.N), dtype=b.torch.float32, device=b.device)
        a = self.table._handle("YawTableAgent").act(b, self._out)
        if not getattr(self.env, "as_torch", False):
            a = a.cpu().numpy()
        return (a if hasattr(self.env, "batch") else a[0]), None
