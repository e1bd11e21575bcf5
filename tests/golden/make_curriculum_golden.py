"""Records tests/golden/curriculum_wrapper.npz from the reference's own ``CurriculumWrapper`` (examples/curriculum.py:335-419).

Run on a development machine that has the reference checkout (the GPU tests never need it):

    python tests/golden/make_curriculum_golden.py <path to the reference checkout>

Like make_golden.py it stubs the packages the reference file imports and this environment lacks (``gymnasium.Wrapper``,
``stable_baselines3.*``, ``wandb.*``, ``WindGym`` with a ``PyWakeAgent`` that returns scripted targets, ``py_wake ... hornsrev1``),
imports examples/curriculum.py UNMODIFIED and drives ``CurriculumWrapper`` on a scripted env the way SB3 drives it: ``step``, a
``reset`` in the same vector step when the env truncated (DummyVecEnv), ``num_timesteps += num_envs``, then the callback's
``update_curriculum(num_timesteps)``.  Only data is written: per case the scripted inputs (yaws, env rewards, the targets in
force, truncation flags, the schedule) and what the wrapper returned (smoothed reward, ``yaw_diff``, ``curriculum_weight``).

Yaws are float64 arrays holding float32-representable values, so the reference's arithmetic is float64 throughout and the
device kernel — float32 yaws widened to float64 — sees the same numbers.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def install_stubs(script):
    """``script``: a dict the scripted PyWakeAgent reads its targets from (``script["targets"]``, one row per ``optimize()``)."""
    gym = types.ModuleType("gymnasium")

    class Wrapper:
        def __init__(self, env):
            self.env = env
    gym.Wrapper = Wrapper
    sys.modules["gymnasium"] = gym

    def module(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class Base:
        def __init__(self, *a, **k):
            pass
    module("stable_baselines3", PPO=Base)
    module("stable_baselines3.common")
    module("stable_baselines3.common.vec_env", DummyVecEnv=Base)
    module("stable_baselines3.common.callbacks", CallbackList=Base, BaseCallback=Base)
    module("stable_baselines3.common.policies", ActorCriticPolicy=Base)
    module("wandb")
    module("wandb.integration")
    module("wandb.integration.sb3", WandbCallback=Base)

    class PyWakeAgent:
        def __init__(self, x_pos, y_pos):
            self.n = len(x_pos)

        def update_wind(self, ws, wd, ti):
            self.wind = (ws, wd, ti)

        def optimize(self):
            self.optimized_yaws = np.array(script["targets"][script["n_optimized"]], dtype=np.float64)
            script["n_optimized"] += 1
    module("WindGym", WindFarmEnv=Base)
    module("WindGym.Agents", PyWakeAgent=PyWakeAgent)
    module("py_wake")
    module("py_wake.examples")
    module("py_wake.examples.data")
    module("py_wake.examples.data.hornsrev1", V80=Base)


def import_reference(ref_root):
    spec = importlib.util.spec_from_file_location("reference_curriculum", os.path.join(ref_root, "examples", "curriculum.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class ScriptedEnv:
    """What CurriculumWrapper touches of a WindFarmEnv: positions, the wind, yaw_max, reset() and step()'s info."""

    def __init__(self, yaws, rewards, truncated, yaw_max):
        n = yaws.shape[1]
        self.fs = types.SimpleNamespace(windTurbines=types.SimpleNamespace(positions_xyz=(np.arange(n) * 500.0, np.zeros(n))))
        self.ws, self.wd, self.ti, self.yaw_max = 10.0, 270.0, 0.07, yaw_max
        self.yaws, self.rewards, self.truncated, self.t = yaws, rewards, truncated, 0

    def reset(self, **kwargs):
        return np.zeros(1), {}

    def step(self, action):
        t = self.t
        self.t += 1
        return np.zeros(1), float(self.rewards[t]), False, bool(self.truncated[t]), {"yaw angles agent": self.yaws[t].copy()}


def script_yaws(rng, n_steps, n, yaw_max):
    """A yaw trajectory of float32-representable values with every pattern the penalties distinguish: moves, reversals, steps
    on which some turbines rest (sign 0) and steps on which all do."""
    y = np.zeros((n_steps, n), dtype=np.float32)
    cur = rng.uniform(-10, 10, n).astype(np.float32)
    for t in range(n_steps):
        kind = t % 8
        if kind == 3:                       # nobody moves
            step = np.zeros(n, np.float32)
        elif kind == 5:                     # only turbine 0 moves
            step = np.zeros(n, np.float32)
            step[0] = np.float32(rng.uniform(-1, 1))
        elif kind == 6:                     # a reversal of the previous move
            step = -(y[t - 1] - y[t - 2]) if t >= 2 else np.zeros(n, np.float32)
        else:
            step = rng.uniform(-1, 1, n).astype(np.float32)
        cur = np.clip(cur + step, -yaw_max, yaw_max).astype(np.float32)
        y[t] = cur
    return y.astype(np.float64)


def record_case(ref, script, n, n_steps, resets, num_envs, curriculum_steps, pure_similarity_steps, seed, yaw_max=40.0):
    rng = np.random.default_rng(seed)
    yaws = script_yaws(rng, n_steps, n, yaw_max)
    rewards = rng.normal(0.0, 0.5, n_steps)
    truncated = np.zeros(n_steps, dtype=bool)
    truncated[list(resets)] = True
    script["targets"] = np.round(rng.uniform(-25, 25, (len(resets) + 1, n)), 3)
    script["n_optimized"] = 0
    env = ScriptedEnv(yaws, rewards, truncated, yaw_max)
    w = ref.CurriculumWrapper(env, curriculum_steps, pure_similarity_steps)
    w.reset()
    shaped, diff, weight, target = [], [], [], []
    num_timesteps = 0
    for t in range(n_steps):
        target.append(np.array(w.pywake_yaws, dtype=np.float64))
        _, r, _, trunc, info = w.step(None)
        shaped.append(r); diff.append(info["yaw_diff"]); weight.append(info["curriculum_weight"])
        if trunc:
            w.reset()                       # DummyVecEnv resets a finished env inside the same vector step
        num_timesteps += num_envs           # OnPolicyAlgorithm.collect_rollouts, then callback.on_step()
        w.update_curriculum(num_timesteps)
    weight = np.array(weight, dtype=np.float64)
    assert weight[0] == 0.0 and (weight == 1.0).sum() >= 5 and ((weight > 0) & (weight < 1)).sum() >= 5
    return dict(yaws=yaws, rewards=rewards, truncated=truncated, targets=np.array(target), shaped=np.array(shaped, dtype=np.float64),
                yaw_diff=np.array(diff, dtype=np.float64), weight=weight, num_envs=np.int64(num_envs),
                curriculum_steps=np.int64(curriculum_steps), pure_similarity_steps=np.int64(pure_similarity_steps),
                yaw_max=np.float64(yaw_max), momentum=np.float64(w.reward_momentum))


def main(ref_root):
    script = {}
    install_stubs(script)
    ref = import_reference(ref_root)
    out = {}
    cases = {"n2": dict(n=2, n_steps=64, resets=(17, 41), num_envs=4, curriculum_steps=160, pure_similarity_steps=40, seed=1),
             "n4": dict(n=4, n_steps=72, resets=(9, 50), num_envs=3, curriculum_steps=150, pure_similarity_steps=31, seed=2)}
    for name, kw in cases.items():
        for k, v in record_case(ref, script, **kw).items():
            out[f"{name}_{k}"] = v
    path = os.path.join(HERE, "curriculum_wrapper.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
