"""CPU checks of behaviour cloning (windgym_amd/imitation.py): the twins of tests/imitation_twin.py themselves — the autograd twin
of both losses against central finite differences, the label recurrence against the env's float32 actuation rule and against
``BaseAgent.scale_yaw`` — the new-episode plumbing shared with ``YawCurriculum``, the ctypes mirrors, and the refusals that need no
device."""
import ctypes as C
import types

import numpy as np
import pytest

import imitation_twin as tw
from helpers import c_layout


# ---- the autograd twin against finite differences ------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_returns", [False, True], ids=["actor", "critic"])
@pytest.mark.parametrize("loss", ["mse", "nll"])
@pytest.mark.parametrize("shape", [(7, (33,), 1), (8, (16,), 4)], ids=["7-33-1", "8-16-4"])
def test_autograd_twin_vs_finite_differences(shape, loss, with_returns):
    """Central differences with h = 1e-6 of a float64 loss of order 1 carry its rounding, 2^-53 / (2 h) ~ 6e-11 per term, and a
    truncation error of h^2 f''' / 6 ~ 1e-12: 1e-7 * max(1, |g|) has three decades of room and is far below any real mistake."""
    n_in, hidden, n_out = shape
    sd = tw.random_params(n_in, hidden, n_out, seed=5)
    rng = np.random.default_rng(6)
    rows = 12
    obs, target, ret = rng.uniform(-1, 1, (rows, n_in)), rng.uniform(-1, 1, (rows, n_out)), rng.standard_normal(rows)
    ids = np.array([3, 0, 11, 3, -1, 12, 7, 5, 5])                     # repeated rows, one entry below and one above the batch
    args = (obs, target, ret if with_returns else None, ids)
    kw = dict(loss=loss, ent_coef=0.01, vf_coef=0.5)
    total, grads, stats = tw.bc_loss_and_grad(sd, *args, **kw)
    assert stats["loss"] == total and np.isfinite(total)
    fd = tw.finite_difference_grad(sd, *args, **kw)
    for k in sd:
        assert np.all(np.abs(fd[k] - grads[k]) <= 1e-7 * np.maximum(1.0, np.abs(grads[k]))), k
    if loss == "mse":
        assert not grads["log_std"].any() and stats["loss"] == stats["mse"] + (0.5 * stats["v_loss"] if with_returns else 0.0)
    else:
        assert grads["log_std"].all()
    critic = [k for k in sd if "value_net" in k]
    assert all(bool(grads[k].any()) == with_returns for k in critic)
    assert any(grads[k].any() for k in sd if "policy_net" in k or "action_net" in k)


def test_twin_skips_entries_outside_the_batch_and_divides_by_all():
    sd = tw.random_params(5, (8,), 2, seed=1)
    rng = np.random.default_rng(2)
    obs, target = rng.uniform(-1, 1, (6, 5)), rng.uniform(-1, 1, (6, 2))
    a = tw.bc_loss_and_grad(sd, obs, target, None, np.array([0, 1, 2, 3]))[2]
    b = tw.bc_loss_and_grad(sd, obs, target, None, np.array([0, 1, -5, 2, 3, 6, 99, 100]))[2]
    assert abs(b["mse"] - a["mse"] / 2.0) < 1e-15 and abs(b["nll"] - a["nll"] / 2.0) < 1e-15 and b["entropy"] == a["entropy"]


# ---- the label recurrence ------------------------------------------------------------------------------------------------------------
def _ulp32(x):
    return float(np.spacing(np.float32(x)))


@pytest.mark.parametrize("method", [tw.ACT_YAW, tw.ACT_WIND])
def test_label_moves_the_yaw_towards_the_target_as_far_as_the_rule_allows(method):
    """Applied through the float32 actuation rule, the label leaves prev + sign(g - prev) * min(|g - prev|, yaw_step): never further
    from g, and the largest move allowed.  The bar: the label's own rounding and the rule's at most five float32 operations each err
    by half an ulp of a magnitude of at most (yaw_max - yaw_min + yaw_step): 4 ulp of that."""
    rng = np.random.default_rng(17)
    for case in range(40):
        lo = -float(rng.choice([20.0, 30.0, 45.0, 37.5]))
        hi = float(rng.choice([20.0, 30.0, 45.0, 41.25]))
        step = float(rng.choice([0.25, 1.0, 3.0, 7.5, 100.0]))
        B, N = 16, 5
        prev = rng.uniform(lo, hi, (B, N)).astype(np.float32)
        g = rng.uniform(lo, hi, (B, N))
        g[0] = prev[0]                                                   # already there: stay
        g[1] = np.clip(prev[1] + step, lo, hi)                           # exactly one step away
        prev[2, :2], g[2, :2] = (lo, hi), (hi, lo)                       # across the whole range
        zeros = np.zeros((1, B), np.uint8)
        labels, diff, g_after, bad = tw.labels_numpy(prev, np.zeros((1, B, N), np.float32), zeros, zeros.astype(np.int32) - 1,
                                                     np.zeros((0, N)), g, method, lo, hi, step)
        assert bad is None and np.array_equal(g_after, g) and labels.dtype == np.float32 and np.all(np.abs(labels[0]) <= 1.0)
        y1 = tw.adjust_yaw_f32(prev, labels[0], method, lo, hi, step).astype(np.float64)
        p64 = prev.astype(np.float64)
        want = p64 + np.sign(g - p64) * np.minimum(np.abs(g - p64), step)
        tol = 4.0 * _ulp32(hi - lo + step)
        assert np.all(np.abs(y1 - want) <= tol), (case, np.abs(y1 - want).max(), tol)
        assert np.all(np.abs(y1 - g) <= np.abs(p64 - g) + tol)
        assert np.allclose(diff[0], np.abs(p64 - g).mean(axis=1), rtol=1e-6, atol=0.0)


def test_wind_labels_are_scale_yaw_of_the_target_rounded_once():
    from windgym_amd.agents import BaseAgent
    rng = np.random.default_rng(3)
    B, N, T = 6, 4, 3
    g = rng.uniform(-30, 30, (B, N))
    yaw0 = rng.uniform(-45, 45, (B, N)).astype(np.float32)
    after = rng.uniform(-45, 45, (T, B, N)).astype(np.float32)
    none = np.zeros((T, B), np.uint8)
    labels = tw.labels_numpy(yaw0, after, none, none.astype(np.int32) - 1, np.zeros((0, N)), g, tw.ACT_WIND, -45.0, 45.0, 1.0)[0]
    want = BaseAgent(yaw_max=45, yaw_min=-45).scale_yaw(g).astype(np.float32)
    assert all(np.array_equal(labels[t], want) for t in range(T))         # whatever the yaws were


def test_target_switches_only_after_a_truncated_step_and_to_the_row_named():
    T, B, N = 6, 4, 2
    g0 = np.arange(B * N, dtype=np.float64).reshape(B, N) - 3.0
    ep_target = 10.0 + np.arange(3 * N, dtype=np.float64).reshape(3, N)
    tr, row = np.zeros((T, B), np.uint8), np.full((T, B), -1, np.int32)
    tr[1, 0], row[1, 0] = 1, 2                  # env 0: row 2 from step 2 on
    tr[2, 1], row[2, 1] = 1, -1                 # env 1: truncated, no row: keeps its target
    row[3, 2] = 1                               # env 2: a row without a truncation is never read
    tr[0, 3], row[0, 3] = 1, 0                  # env 3: row 0 from step 1, then row 1 from step 5
    tr[4, 3], row[4, 3] = 1, 1
    yaw = np.zeros((T, B, N), np.float32)
    labels, diff, g1, bad = tw.labels_numpy(yaw[0], yaw, tr, row, ep_target, g0, tw.ACT_WIND, -45.0, 45.0, 1.0)
    in_force = (labels.astype(np.float64) + 1.0) / 2.0 * 90.0 - 45.0           # the target a "wind" label encodes
    want = np.broadcast_to(g0, (T, B, N)).copy()
    want[2:, 0], want[1:5, 3], want[5:, 3] = ep_target[2], ep_target[0], ep_target[1]
    assert bad is None and np.allclose(in_force, want, atol=1e-4, rtol=0.0)
    assert np.array_equal(g1[[1, 2]], g0[[1, 2]]) and np.array_equal(g1[0], ep_target[2]) and np.array_equal(g1[3], ep_target[1])
    assert np.allclose(diff, np.abs(want).mean(axis=2), rtol=1e-6)              # (every yaw is 0)
    row[4, 3] = 3                                                              # no such row: skipped and reported
    g2, bad = tw.labels_numpy(yaw[0], yaw, tr, row, ep_target, g0, tw.ACT_WIND, -45.0, 45.0, 1.0)[2:]
    assert bad == (4, 3, 3) and np.array_equal(g2[3], ep_target[0])


# ---- the plumbing shared with YawCurriculum --------------------------------------------------------------------------------------------
def test_new_episode_targets_numbers_the_rows_in_step_order_and_optimises_their_winds_once():
    import torch
    from windgym_amd.curriculum import new_episode_targets
    T, B, N = 4, 3, 2
    tr = torch.zeros((T, B), dtype=torch.uint8)
    tr[0, 2] = tr[2, 0] = tr[2, 2] = 1
    wind = torch.arange(T * B * 3, dtype=torch.float64).reshape(T, B, 3)
    ep_row = torch.full((T, B), 7, dtype=torch.int32)
    calls, laps = [], []

    def optimize(ws, wd, ti):
        calls.append(torch.stack([ws, wd, ti], dim=1))
        return torch.stack([ws, -ws], dim=1)
    none = torch.zeros((0, N), dtype=torch.float64)
    n, target = new_episode_targets(torch, dict(truncated=tr, wind_f64=wind), ep_row, optimize, none, laps.append)
    want = torch.full((T, B), -1, dtype=torch.int32)
    want[0, 2], want[2, 0], want[2, 2] = 0, 1, 2
    assert n == 3 and torch.equal(ep_row, want) and len(calls) == 1 and laps == ["plumbing", "serial_refine"]
    assert torch.equal(calls[0], torch.stack([wind[0, 2], wind[2, 0], wind[2, 2]])) and torch.equal(target[:, 0], calls[0][:, 0])
    n, target = new_episode_targets(torch, dict(truncated=torch.zeros_like(tr), wind_f64=wind), ep_row, optimize, none)
    assert n == 0 and target is none and len(calls) == 1 and bool((ep_row == -1).all())


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirrors_match_the_header(tmp_path):
    from windgym_amd import binding
    for name, cls in (("wg_bc_batch", binding.CBcBatch), ("wg_bc_hyper", binding.CBcHyper)):
        fields = [f[0] for f in cls._fields_]
        out = c_layout(name, fields, tmp_path)
        assert out["sizeof"] == C.sizeof(cls), name
        assert all(out[f] == getattr(cls, f).offset for f in fields), name
    assert c_layout("wg_bc_stats", ["loss", "mse", "nll", "entropy", "v_loss", "mean_abs_err", "reserved"], tmp_path) == dict(
        sizeof=32, loss=0, mse=4, nll=8, entropy=12, v_loss=16, mean_abs_err=20, reserved=24)
    assert binding.BC_STATS[:6] == tw.BC_STATS and binding.BC_LOSS == {"mse": 0, "nll": 1}


def test_the_package_exports_the_trainer():
    import windgym_amd
    from windgym_amd.imitation import BehaviorCloning
    from windgym_amd.ppo import Trainer
    assert windgym_amd.BehaviorCloning is BehaviorCloning and issubclass(BehaviorCloning, Trainer)
    assert "deterministic" in BehaviorCloning.__doc__ and "log_std" in BehaviorCloning.__doc__


def test_refusals_need_no_device():
    from windgym_amd.imitation import BehaviorCloning
    env = dict(batch=types.SimpleNamespace(obs_dim=9), rollout=None, num_envs=4, n_turb=2)
    ok = types.SimpleNamespace(as_torch=True, **env)
    with pytest.raises(NotImplementedError, match="recurrent"):
        BehaviorCloning(types.SimpleNamespace(recurrent=True), ok)
    with pytest.raises(NotImplementedError, match="population"):
        BehaviorCloning("MlpPolicy", types.SimpleNamespace(as_torch=True, population=object(), **env))
    with pytest.raises(NotImplementedError, match="population"):
        BehaviorCloning(types.SimpleNamespace(population=object()), ok)
    with pytest.raises(NotImplementedError, match="split policy"):
        BehaviorCloning(types.SimpleNamespace(split=True, n_in_vf=9), ok)
    with pytest.raises(ValueError, match="as_torch"):
        BehaviorCloning("MlpPolicy", types.SimpleNamespace(as_torch=False, **env))
    with pytest.raises(ValueError, match="WindFarmVecEnv"):
        BehaviorCloning("MlpPolicy", types.SimpleNamespace(as_torch=True))
    with pytest.raises(ValueError, match="loss must be one of"):
        BehaviorCloning("MlpPolicy", ok, loss="huber")
    with pytest.raises(ValueError, match="expert must be one of"):
        BehaviorCloning("MlpPolicy", ok, expert="floris")
    with pytest.raises(ValueError, match="expert must be one of"):
        BehaviorCloning("MlpPolicy", ok, expert=object())
    with pytest.raises(ValueError, match="unknown policy"):
        BehaviorCloning("CnnPolicy", ok)
    with pytest.raises(ValueError, match="batch_size"):
        BehaviorCloning("MlpPolicy", ok, n_steps=2, batch_size=9)
