"""Twins of behaviour cloning (windgym_amd/imitation.py; tests/test_imitation.py checks them on the CPU, tests/test_gpu_imitation.py
holds the kernels against them): the label recurrence of k_expert_labels in float64 numpy, the env's float32 actuation rule, and
both supervised losses of k_bc_grad on float64 torch tensors with gradients from autograd (the forward pass is
oracle/ppo_oracle.py's)."""
import math

import numpy as np

from oracle import ppo_oracle as oo

ACT_WIND, ACT_YAW = "wind", "yaw"
BC_STATS = ("loss", "mse", "nll", "entropy", "v_loss", "mean_abs_err")


def labels_numpy(yaw0, yaw_after, truncated, ep_row, ep_target, targets, action_method, yaw_min, yaw_max, yaw_step):
    """wg_expert_labels in float64 numpy (include/windgym_hip.h states the rule): ``yaw0 [B, N]``, ``yaw_after [T, B, N]``,
    ``truncated`` / ``ep_row [T, B]``, ``ep_target [C, N]``, ``targets [B, N]`` -> ``(labels [T, B, N] float32, yaw_diff [T, B]
    float32, the target table after the rollout [B, N] float64, the first (t, b, row) with row >= C or None)``.  The limits are the
    env's float32 values widened to double, as the kernel holds them."""
    yaw0, yaw_after = np.asarray(yaw0, np.float32), np.asarray(yaw_after, np.float32)
    T, B, N = yaw_after.shape
    ep_target = np.asarray(ep_target, np.float64).reshape(-1, N)
    g = np.array(targets, np.float64).reshape(B, N).copy()
    lo, hi, step = (np.float64(np.float32(v)) for v in (yaw_min, yaw_max, yaw_step))
    labels, diff, bad = np.zeros((T, B, N), np.float32), np.zeros((T, B), np.float32), None
    for t in range(T):
        prev = (yaw0 if t == 0 else yaw_after[t - 1]).astype(np.float64)
        if action_method == ACT_YAW:
            a = np.minimum(np.maximum((g - prev) / step, -1.0), 1.0)
        else:
            a = (g - lo) / (hi - lo) * 2.0 - 1.0
        labels[t] = a.astype(np.float32)
        d = np.zeros(B)
        for i in range(N):                                    # in index order, as the kernel adds
            d = d + np.abs(prev[:, i] - g[:, i])
        diff[t] = (d / np.float64(N)).astype(np.float32)
        for b in np.nonzero(np.asarray(truncated[t]))[0]:
            r = int(ep_row[t][b])
            if r >= len(ep_target):
                bad = bad or (t, int(b), r)
            elif r >= 0:
                g[b] = ep_target[r]
    return labels, diff, g, bad


def adjust_yaw_f32(yaw, a, action_method, yaw_min, yaw_max, yaw_step):
    """WindFarmEnv._adjust_yaws in float32, operation by operation as the step kernels evaluate it (cur_adjust_yaw of
    wg_curriculum.hip restates it): the yaw an actuation step leaves, from the yaw before it and the action."""
    f = np.float32
    yaw, a = np.asarray(yaw, f), np.asarray(a, f)
    lo, hi, step = f(yaw_min), f(yaw_max), f(yaw_step)
    if action_method == ACT_YAW:
        return np.minimum(np.maximum((yaw + (a * step).astype(f)).astype(f), lo), hi)
    tf = (a + f(1.0)).astype(f)
    tf = (tf * f(0.5)).astype(f)
    tf = (tf * f(hi - lo)).astype(f)
    tf = (tf + lo).astype(f)
    ny = np.minimum(np.maximum(tf, (yaw - step).astype(f)), (yaw + step).astype(f))
    return np.minimum(np.maximum(ny, lo), hi)


def bc_loss(tp, obs, target, returns, ids, loss="mse", ent_coef=0.0, vf_coef=0.0, activation="tanh"):
    """The header's loss (wg_bc_grad) on float64 CPU tensors; ``tp`` = {SB3 name: tensor}; ``returns`` may be ``None``.  ``ids``: the
    minibatch's rows (any integers); entries outside ``[0, rows)`` are skipped and every mean still divides by ``len(ids)``.
    -> (loss, dict of the six statistics)."""
    import torch
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    ok = ids[(ids >= 0) & (ids < obs.shape[0])]
    mean = oo._net(tp, "mlp_extractor.policy_net", "action_net", obs[ok], activation)
    ls = tp["log_std"]
    n_out = mean.shape[1]
    e = mean - target[ok]
    z = (target[ok] - mean) / torch.exp(ls)
    logp = (-0.5 * z * z - ls - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)
    mse = (e * e).sum() / n_out / n
    nll = -logp.sum() / n
    H = (0.5 + 0.5 * math.log(2.0 * math.pi) + ls).sum()
    total = mse if loss == "mse" else nll - ent_coef * H
    v_loss = torch.zeros((), dtype=torch.float64)
    if returns is not None:
        V = oo._net(tp, "mlp_extractor.value_net", "value_net", obs[ok], activation)[:, 0]
        v_loss = ((returns[ok] - V) ** 2).sum() / n
        total = total + vf_coef * v_loss
    return total, dict(loss=total, mse=mse, nll=nll, entropy=H, v_loss=v_loss, mean_abs_err=e.abs().sum() / n_out / n)


def _tensors(params, obs, target, returns, requires_grad):
    import torch
    tp = {k: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64, requires_grad=requires_grad) for k, v in params.items()}
    as_t = lambda x: None if x is None else torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)
    return tp, as_t(obs), as_t(target), as_t(returns)


def bc_loss_and_grad(params, obs, target, returns, ids, **kw):
    """numpy in, numpy out -> (loss, {name: d loss / d tensor} from AUTOGRAD, statistics dict)."""
    tp, *args = _tensors(params, obs, target, returns, True)
    total, stats = bc_loss(tp, *args, ids, **kw)
    total.backward()
    grads = {k: (np.zeros(v.shape) if v.grad is None else v.grad.numpy().copy()) for k, v in tp.items()}
    return float(total.detach()), grads, {k: float(v.detach()) for k, v in stats.items()}


def bc_loss_value(params, obs, target, returns, ids, **kw):
    tp, *args = _tensors(params, obs, target, returns, False)
    return float(bc_loss(tp, *args, ids, **kw)[0])


def finite_difference_grad(params, *args, h=1e-6, **kw):
    """Central differences of :func:`bc_loss_value` in every parameter -> {name: array}."""
    out = {}
    for name, a in params.items():
        g = np.zeros(a.shape)
        for i in np.ndindex(*a.shape):
            hi, lo = {k: v.copy() for k, v in params.items()}, {k: v.copy() for k, v in params.items()}
            hi[name][i] += h
            lo[name][i] -= h
            g[i] = (bc_loss_value(hi, *args, **kw) - bc_loss_value(lo, *args, **kw)) / (2.0 * h)
        out[name] = g
    return out


def random_params(n_in, hidden, n_out, seed=0):
    """A float64 state dict under SB3's names (actor and critic of the same hidden stack), every entry away from 0."""
    rng = np.random.default_rng(seed)
    sd = {}
    for net in ("policy_net", "value_net"):
        k = n_in
        for l, m in enumerate(hidden):
            sd[f"mlp_extractor.{net}.{2 * l}.weight"] = rng.standard_normal((m, k)) / np.sqrt(k)
            sd[f"mlp_extractor.{net}.{2 * l}.bias"] = rng.uniform(-0.3, 0.3, m)
            k = m
        head, width = ("action_net", n_out) if net == "policy_net" else ("value_net", 1)
        sd[head + ".weight"] = rng.standard_normal((width, k)) / np.sqrt(k)
        sd[head + ".bias"] = rng.uniform(-0.3, 0.3, width)
    sd["log_std"] = rng.uniform(-0.3, 0.3, n_out)
    return sd
