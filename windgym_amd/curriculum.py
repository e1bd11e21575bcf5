"""Yaw-curriculum reward shaping on the device — the reference's second way of training: PPO on the reward of
``CurriculumWrapper`` with the weight ``CurriculumCallback`` sets (examples/curriculum.py:335-429).

Until ``curriculum_steps`` env steps have been collected the agent is paid mostly for holding yaws close to the Serial-Refine
optimum of its episode's wind, ``1 / (1 + mean |yaw - yaw_opt|)``, less movement and oscillation penalties; the result is blended
with the env's reward by a weight that ramps 0 -> 1 between ``pure_similarity_steps`` and ``curriculum_steps`` and smoothed
exponentially.  The policy never reads the reward while it collects, so the shaping is a POST-PASS over a rollout's buffers, as
GAE is: :meth:`YawCurriculum.rollout` is ``venv.rollout`` (wg_rollout / wg_rollout_multi, untouched) + one Serial-Refine launch
for the episodes that began inside the rollout (k_steady_srf) + one launch of k_curriculum (wg_curriculum_shape).

:func:`shape_numpy` restates the wrapper's arithmetic in float64 numpy; it is to k_curriculum what ``mann.py``'s generator is to
wg_mann.hip, and is itself pinned to the reference class by tests/golden/curriculum_wrapper.npz.  There is no CPU fallback:
:class:`YawCurriculum` needs the built library and a GPU.
"""
from __future__ import annotations

import time

import numpy as np

from .policy import refuse_recurrent

ARGS = ("curriculum_steps", "pure_similarity_steps", "model", "refine_pass_n", "yaw_n", "search_yaw_max", "reward_momentum")


def check_steps(curriculum_steps, pure_similarity_steps):
    """``ValueError`` for schedules the reference cannot evaluate (it would divide by zero) or that make no sense."""
    cs, ps = int(curriculum_steps), int(pure_similarity_steps)
    if cs < 0 or ps < 0:
        raise ValueError("curriculum_steps and pure_similarity_steps must be >= 0")
    if cs <= ps:
        raise ValueError(f"curriculum_steps ({cs}) must exceed pure_similarity_steps ({ps}): the weight ramps between the two")
    return cs, ps


def curriculum_weights(num_timesteps, n_steps, num_envs, curriculum_steps, pure_similarity_steps):
    """``env_reward_weight`` of the ``n_steps`` vector steps that follow ``num_timesteps`` collected env steps, float64 ``[n_steps]``:
    SB3 adds ``num_envs`` to ``num_timesteps`` after every vector step and the callback then calls ``update_curriculum`` with it
    (curriculum.py:409-429), so step ``t`` of the rollout is shaped with ``clip((num_timesteps + t * num_envs - pure) / (curriculum -
    pure), 0, 1)``."""
    cs, ps = check_steps(curriculum_steps, pure_similarity_steps)
    step = int(num_timesteps) + np.arange(int(n_steps), dtype=np.int64) * int(num_envs)
    return np.minimum(1.0, np.maximum(0.0, (step - ps).astype(np.float64) / float(cs - ps)))


def shape_numpy(yaws, rewards, targets, weights, momentum, yaw_max, state=None):
    """``CurriculumWrapper.step`` (curriculum.py:359-407) for ONE env over T steps, in float64: ``yaws [T, N]`` = the agent
    farm's yaws after each step's actuation (before a reset), ``rewards [T]`` the env's, ``targets [T, N]`` the optimal yaws in
    force at each step, ``weights [T]`` -> ``(shaped [T], yaw_diff [T], state)``.  ``state`` (a dict, ``None`` = a fresh wrapper)
    carries what the wrapper keeps — and, like it, never clears: ``previous_yaws`` and the change history survive resets.  The
    unbounded ``yaw_change_history`` is kept in its exact running form: its length ``L``, the integer ``osc = sum |diff(sign)|``,
    ``cum = sum`` of every change, the last signs."""
    yaws, targets = np.asarray(yaws, np.float64), np.asarray(targets, np.float64)
    rewards, weights = np.asarray(rewards, np.float64), np.asarray(weights, np.float64)
    T, N = yaws.shape
    st = dict(yprev=None, sprev=None, L=0, osc=0, cum=0.0, last=0.0) if state is None else dict(state)
    m, yaw_max = float(momentum), float(yaw_max)
    shaped, diff = np.zeros(T), np.zeros(T)
    for t in range(T):
        y = yaws[t]
        d = np.abs(y - targets[t]).mean()
        sim = 1.0 / (1.0 + d)
        pen = 0.0
        if st["yprev"] is not None:
            c = np.abs(y - st["yprev"])
            st["L"] += 1
            csum = c.sum()
            pen += 0.3 * (csum / N / yaw_max)
            st["cum"] += csum
            sg = np.sign(c).astype(np.int64)
            if st["L"] >= 2:
                st["osc"] += int(np.abs(sg - st["sprev"]).sum())
                pen += st["osc"] / ((st["L"] - 1) * N) * 0.2
            if st["L"] >= 5:
                pen += st["cum"] / N / yaw_max * 0.1
            st["sprev"] = sg
        st["yprev"] = y.copy()
        cur = (1.0 - weights[t]) * (sim - pen / 600.0) + weights[t] * rewards[t]
        st["last"] = m * st["last"] + (1.0 - m) * cur
        shaped[t], diff[t] = st["last"], d
    return shaped, diff, st


def targets_per_step(initial, truncated, new_targets):
    """The ``targets [T, N]`` of :func:`shape_numpy` for one env: ``initial [N]`` until the env's first truncation, then, from the
    step AFTER each truncating step, the next row of ``new_targets`` (one per truncation, in order) — the step that truncates is
    still paid against the episode that ended (``CurriculumWrapper.reset`` runs after it)."""
    g, k, out = np.asarray(initial, np.float64), 0, []
    for tr in np.asarray(truncated).astype(bool):
        out.append(g)
        if tr:
            g, k = np.asarray(new_targets[k], np.float64), k + 1
    return np.stack(out)


def lap_ms(t, device, timing, key):
    """Measurement only (``rollout(timing=...)``): synchronise and add the milliseconds since the last lap to ``timing[key]``."""
    if timing is None:
        return
    t.cuda.synchronize(device)
    now = time.perf_counter()
    if key is not None:
        timing[key] = timing.get(key, 0.0) + (now - timing["_t"]) * 1e3
    timing["_t"] = now


def new_episode_targets(t, out, ep_row, optimize, no_targets, lap=lambda key: None, table=None):
    """The new-episode plumbing of a rollout recorded with ``wind_f64`` (:meth:`YawCurriculum.rollout`,
    ``imitation.BehaviorCloning.collect``): the episodes that began inside it get their targets from ONE Serial-Refine launch over
    exactly their C wind conditions.  Fills ``ep_row [T, B]`` (int32: -1, or the row of the step's new episode, numbered in (t, env)
    order) -> ``(C, ep_target [C, N])`` (``no_targets`` when no env truncated).  ``optimize(ws, wd, ti) -> [C, N]`` float64;
    ``lap(key)`` closes a part of the caller's timing split.  Compacting the flags is ONE host synchronisation.

    ``table`` (a ``yaw_table.YawTable``): the targets are the table's — ``ep_row`` becomes the table row of every new episode's wind
    (ONE launch of k_yaw_table_rows) -> ``(table.n_rows, table.yaw)``: no ``nonzero()``, no Serial-Refine launch, no synchronisation."""
    if table is not None:
        table.rows(out["wind_f64"], out["truncated"], out=ep_row)
        return table.n_rows, table.yaw
    idx = out["truncated"].view(-1).nonzero().view(-1)            # the rollout's one host synchronisation; sorted by (t, env)
    n_new = int(idx.numel())
    ep_row.fill_(-1)
    ep_target = no_targets
    if n_new:
        ep_row.view(-1)[idx] = t.arange(n_new, dtype=t.int32, device=ep_row.device)
        wind = out["wind_f64"].view(-1, 3)[idx]                   # recorded after the autoreset: the new episode's wind
        lap("plumbing")
        ep_target = optimize(wind[:, 0], wind[:, 1], wind[:, 2]).contiguous()
        lap("serial_refine")
    return n_new, ep_target


class YawCurriculum:
    """The curriculum of one ``WindFarmVecEnv`` / ``WindFarmVecEnvMulti`` (``as_torch=True``; arguments: the reference's
    ``CurriculumWrapper(env, curriculum_steps, pure_similarity_steps)`` plus the optimiser's — ``model`` ``"blondel_jimenez"`` (the
    reference agent's wake model) or ``"m0"`` (the env's own), ``refine_pass_n`` x ``yaw_n`` candidates within ``search_yaw_max``
    degrees — and ``reward_momentum``).  Construction and :meth:`reset` set every env's running target to the optimum of its
    current wind (``HipBatch.optimal_yaws``); ``targets`` is that table, ``[B, N]`` float64 on the device.  The shaping state (the
    wrapper's ``previous_yaws``, change history and ``last_reward``) is never cleared, as in the reference; :meth:`state` /
    :meth:`load_state` checkpoint it.  ``PPO(..., curriculum=...)`` trains on the shaped reward.

    ``targets=`` a ``yaw_table.YawTable`` of this env's farm and device: every target is the table's row of the episode's wind
    instead.  Construction, :meth:`reset` and :meth:`rollout` then launch no Serial-Refine and synchronise nothing, the optimiser's
    arguments are the table's own, and ``last_n_targets`` is ``None`` (counting the new episodes is the synchronisation this mode
    removes).  The default, ``None``, is the optimiser per rollout."""

    def __init__(self, venv, curriculum_steps, pure_similarity_steps, model="blondel_jimenez", refine_pass_n=8, yaw_n=9,
                 search_yaw_max=30.0, reward_momentum=0.9, targets=None):
        from .binding import Curriculum
        from .steady import MODEL_IDS
        self.curriculum_steps, self.pure_similarity_steps = check_steps(curriculum_steps, pure_similarity_steps)
        if model not in MODEL_IDS:
            raise ValueError(f"model must be one of {sorted(MODEL_IDS)}, not {model!r}")
        if not 0.0 <= float(reward_momentum) < 1.0:
            raise ValueError("reward_momentum must lie in [0, 1)")
        if not (hasattr(venv, "batch") and hasattr(venv, "rollout")):
            raise ValueError("YawCurriculum needs a WindFarmVecEnv or a WindFarmVecEnvMulti")
        if not getattr(venv, "as_torch", True):
            raise ValueError("YawCurriculum works on CUDA tensors: construct the env with as_torch=True")
        self.venv, self.batch, self.torch = venv, venv.batch, venv.batch.torch
        self.table = targets
        if targets is not None:
            if not hasattr(targets, "check_env"):
                raise ValueError("targets must be a yaw_table.YawTable (or None: the optimiser runs for every new episode)")
            targets.check_env(venv, "YawCurriculum(targets=)")
        self.model, self.refine_pass_n, self.yaw_n = model, int(refine_pass_n), int(yaw_n)
        self.search_yaw_max, self.reward_momentum = float(search_yaw_max), float(reward_momentum)
        self._cur = Curriculum(self.batch)
        self._bufs = {}
        self.last_n_targets = 0 if targets is None else None      # Serial-Refine conditions the last rollout() served (a table: not counted)
        self.last_rollout = None                      # the dict the last rollout() returned (valid until the next one)
        t, b = self.torch, self.batch
        self._yaw0 = t.zeros((b.B, b.N), dtype=t.float32, device=b.device)
        self._no_targets = t.zeros((0, b.N), dtype=t.float64, device=b.device)
        self.reset()

    def args(self):
        """The constructor's arguments after ``venv`` (what ``PPO.save`` stores)."""
        return {k: getattr(self, k) for k in ARGS}

    def _optimize(self, ws, wd, ti):
        return self.batch.steady_optimize(ws, wd, ti, model=self.model, refine_pass_n=self.refine_pass_n, yaw_n=self.yaw_n,
                                          yaw_max=self.search_yaw_max)[0]

    def reset(self):
        """``CurriculumWrapper.reset`` for the whole batch: every env's target becomes the optimum of its current wind.  The
        shaping state stays, as in the reference."""
        if self.table is not None:
            self.targets = self.table.targets(self.batch.info("wind_f64"))
            self._cur.set_targets(self.targets)
            return self.targets
        self.targets = self.batch.optimal_yaws(model=self.model, refine_pass_n=self.refine_pass_n, yaw_n=self.yaw_n,
                                               yaw_max=self.search_yaw_max).contiguous()
        self._cur.set_targets(self.targets)
        return self.targets

    def state(self) -> bytes:
        return self._cur.state()

    def load_state(self, blob: bytes):
        self._cur.load_state(blob)
        self.targets = self.torch.from_numpy(self._cur.targets_of(blob)).to(self.batch.device)

    def close(self):
        self._cur.close()

    def weights(self, num_timesteps, n_steps):
        return curriculum_weights(num_timesteps, n_steps, self.venv.num_envs, self.curriculum_steps, self.pure_similarity_steps)

    def _lap(self, timing, key):
        lap_ms(self.torch, self.batch.device, timing, key)

    def rollout(self, policy, n_steps, num_timesteps=0, *, deterministic=False, record=(), values=True, yaw_out=False, timing=None):
        """``venv.rollout(policy, n_steps)`` with the reward shaped: the returned dict has ``reward [T, B]`` replaced by the
        shaped reward and gains ``env_reward`` (the env's own), ``yaw_diff [T, B]`` (mean distance to the target, degrees),
        ``curriculum_weight [T]`` (float64), the records ``yaw_agent`` / ``wind_f64`` and, with ``yaw_out``, ``yaw_held [T, B, N]``:
        the yaws the agent farm held after each step's actuation, before a same-step autoreset.  ``num_timesteps``: env steps
        collected before this rollout (the weight of step t is that of ``num_timesteps + t * num_envs``).

        Episodes that began inside the rollout get their targets from ONE Serial-Refine launch over exactly those C wind
        conditions (none when no env truncated).  Finding them compacts the truncation flags (``nonzero``): ONE host
        synchronisation per rollout, after the closed loop has been enqueued — ``PPO.learn(log_interval=None)`` with a
        curriculum is therefore not free of synchronisation, as it is without one.  With ``targets=`` a ``YawTable`` neither
        happens: the rows come from one k_yaw_table_rows launch and ``learn`` synchronises nothing again.  The buffers are reused like
        ``venv.rollout``'s: valid until the next call.  ``timing``: a dict that receives the milliseconds of the parts
        (``rollout``, ``serial_refine``, ``k_curriculum``, ``plumbing`` = everything else), measured between device
        synchronisations — tools/bench_ppo.py's split; it slows the call."""
        refuse_recurrent(policy, "YawCurriculum.rollout()")
        if getattr(policy, "population", None) is not None:
            raise NotImplementedError("a curriculum for a population is not implemented")
        t, b = self.torch, self.batch
        T, B, N = int(n_steps), b.B, b.N
        w_host = self.weights(num_timesteps, T)
        self._lap(timing, None)
        b.info("yaw_agent", out=self._yaw0)
        rec = tuple(record) + tuple(r for r in ("yaw_agent", "wind_f64") if r not in record)
        out = self.venv.rollout(policy, T, deterministic=deterministic, record=rec, values=values)
        self._lap(timing, "rollout")
        bufs = self._bufs.get((T, bool(yaw_out)))
        if bufs is None:
            f32 = dict(dtype=t.float32, device=b.device)
            bufs = dict(shaped=t.zeros((T, B), **f32), yaw_diff=t.zeros((T, B), **f32),
                        ep_row=t.zeros((T, B), dtype=t.int32, device=b.device),
                        weight=t.zeros((T,), dtype=t.float64, device=b.device),
                        yaw_held=t.zeros((T, B, N), **f32) if yaw_out else None)
            self._bufs[(T, bool(yaw_out))] = bufs
        bufs["weight"].copy_(t.from_numpy(w_host))
        ep_row = bufs["ep_row"]
        n_new, ep_target = new_episode_targets(t, out, ep_row, self._optimize, self._no_targets, lambda key: self._lap(timing, key),
                                               table=self.table)
        self.last_n_targets = n_new if self.table is None else None
        self._lap(timing, "plumbing")
        self._cur.shape(T, self._yaw0, out["actions"], out["yaw_agent"], out["truncated"], ep_row, ep_target, n_new, bufs["weight"],
                        self.reward_momentum, out["reward"], bufs["shaped"], bufs["yaw_diff"], bufs["yaw_held"])
        self._lap(timing, "k_curriculum")
        if self.table is not None:
            # the mirror of the kernel's running targets: an env's target is always the table's row of its episode's wind, and the
            # wind recorded after the last step is that of the episode the env is in now
            self.table.targets(out["wind_f64"][T - 1], out=self.targets)
        elif n_new:
            # the mirror of the kernel's running targets: rows are numbered in step order, so an env's LAST new episode has its largest
            last = ep_row.max(dim=0).values.long()
            self.targets = t.where((last >= 0).unsqueeze(1), ep_target[last.clamp(min=0)], self.targets)
        out["env_reward"], out["reward"], out["yaw_diff"] = out["reward"], bufs["shaped"], bufs["yaw_diff"]
        out["curriculum_weight"] = bufs["weight"]
        if yaw_out:
            out["yaw_held"] = bufs["yaw_held"]
        self._lap(timing, "plumbing")
        self.last_rollout = out
        return out
