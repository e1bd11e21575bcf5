"""ORACLE / TEST INFRASTRUCTURE — float64 restatement of the training entries of include/windgym_hip.h (wg_gae, wg_ppo_grad,
wg_ppo_apply), written from the header's formulas and not from windgym_amd/csrc/wg_ppo.hip.

* :func:`gae` is the backward recurrence, :func:`gae_brute` the per-env definition it is checked against;
* :func:`loss` is the minibatch loss as a float64 torch expression on the CPU; :func:`loss_and_grad` takes its gradient from
  AUTOGRAD (the kernel's backward pass is hand-derived: the two share nothing);
* :func:`adam_step` is gradient clipping by the global norm + one Adam step in numpy;
* :func:`tile_rows` is the row tile R of k_ppo_grad as windgym_amd/csrc/wg_ppo.h documents it (the LDS map of one net).

Parameters are dicts under stable-baselines3's state-dict names (weights ``[out][in]``), as in policy_oracle.py.
"""
from __future__ import annotations

import math

import numpy as np


def gae(reward, value, final_value, truncated, gamma, lam):
    """[T, B] float64 (advantage, returns): delta_t = r_t + gamma final_value_t - value_t,
    A_t = delta_t + gamma lam (1 - truncated_t) A_{t+1}, A_T = 0, returns = A + value."""
    r, v, fv = (np.asarray(x, np.float64) for x in (reward, value, final_value))
    cont = 1.0 - np.asarray(truncated).astype(np.float64)
    adv = np.zeros_like(r)
    a = np.zeros(r.shape[1])
    for t in range(r.shape[0] - 1, -1, -1):
        a = r[t] + gamma * fv[t] - v[t] + gamma * lam * cont[t] * a
        adv[t] = a
    return adv, adv + v


def gae_brute(reward, value, final_value, truncated, gamma, lam):
    """The same by definition: A_t = sum_{s >= t} (gamma lam)^(s - t) delta_s over the steps up to and including the first
    truncation at or after t (or the end of the buffer)."""
    r, v, fv = (np.asarray(x, np.float64) for x in (reward, value, final_value))
    tr = np.asarray(truncated).astype(bool)
    T, B = r.shape
    adv = np.zeros((T, B))
    for b in range(B):
        for t in range(T):
            s, w, acc = t, 1.0, 0.0
            while s < T:
                acc += w * (r[s, b] + gamma * fv[s, b] - v[s, b])
                if tr[s, b]:
                    break
                w *= gamma * lam
                s += 1
            adv[t, b] = acc
    return adv, adv + v


def _torch_net(tp, prefix, head, x, activation):
    import torch
    i = 0
    while f"{prefix}.{i}.weight" in tp:
        x = x @ tp[f"{prefix}.{i}.weight"].T + tp[f"{prefix}.{i}.bias"]
        x = torch.tanh(x) if activation == "tanh" else torch.relu(x)
        i += 2
    return x @ tp[head + ".weight"].T + tp[head + ".bias"]


def loss(tp, obs, raw, logp_old, advantage, returns, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, normalize_advantage=True,
         activation="tanh"):
    """The header's loss on float64 CPU tensors; ``tp`` = {name: tensor}.  -> (loss, dict of the statistics, ratio)."""
    import torch
    mean = _torch_net(tp, "mlp_extractor.policy_net", "action_net", obs, activation)
    V = _torch_net(tp, "mlp_extractor.value_net", "value_net", obs, activation)[:, 0]
    ls = tp["log_std"]
    z = (raw - mean) / torch.exp(ls)
    logp = (-0.5 * z * z - ls - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)
    ratio = torch.exp(logp - logp_old)
    A = advantage
    if normalize_advantage and A.numel() > 1:
        A = (A - A.mean()) / (A.std() + 1e-8)
    l_pi = -torch.minimum(ratio * A, torch.clamp(ratio, 1.0 - clip_range, 1.0 + clip_range) * A)
    l_v = (returns - V) ** 2
    H = (0.5 + 0.5 * math.log(2.0 * math.pi) + ls).sum()
    total = l_pi.mean() + vf_coef * l_v.mean() - ent_coef * H
    stats = dict(pi_loss=l_pi.mean(), v_loss=l_v.mean(), entropy=H, approx_kl=((ratio - 1.0) - (logp - logp_old)).mean(),
                 clip_fraction=((ratio - 1.0).abs() > clip_range).double().mean(), loss=total)
    return total, stats, ratio


def loss_and_grad(params, obs, raw, logp_old, advantage, returns, **kw):
    """numpy in, numpy out: -> (loss, {name: d loss / d tensor}, statistics dict, ratio); the gradient is autograd's."""
    import torch
    tp = {k: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    args = [torch.tensor(np.asarray(x, np.float64), dtype=torch.float64) for x in (obs, raw, logp_old, advantage, returns)]
    total, stats, ratio = loss(tp, *args, **kw)
    total.backward()
    grads = {k: (np.zeros(v.shape) if v.grad is None else v.grad.numpy().copy()) for k, v in tp.items()}
    return float(total.detach()), grads, {k: float(v.detach()) for k, v in stats.items()}, ratio.detach().numpy()


def adam_step(params, grad, m, v, step, lr, max_grad_norm, beta1=0.9, beta2=0.999, eps=1e-5):
    """Flat float64 vectors: clip ``grad`` to the global L2 norm ``max_grad_norm`` (scale = min(1, max / (norm + 1e-6))), then
    Adam's bias-corrected step number ``step`` (1-based).  -> (params, m, v)."""
    g = np.asarray(grad, np.float64)
    g = g * min(1.0, max_grad_norm / (math.sqrt(float(np.sum(g * g))) + 1e-6))
    m = beta1 * np.asarray(m, np.float64) + (1.0 - beta1) * g
    v = beta2 * np.asarray(v, np.float64) + (1.0 - beta2) * g * g
    mhat = m / (1.0 - beta1 ** step)
    denom = np.sqrt(v) / math.sqrt(1.0 - beta2 ** step) + eps
    return np.asarray(params, np.float64) - lr * mhat / denom, m, v


def lds_floats(n_in, widths, rows, kc=256):
    """Floats of wg_ppo.h's LDS map (WgPpoLds) of ONE net for tiles of ``rows`` rows; ``widths`` = the M of every layer, head
    included.  S = rows + 1 floats per feature row: xin [min(n_in, kc)][S], act [sum M][S], d [2][max M][S], then rowv [4][32]
    and rid [32]."""
    s = rows + 1
    return (min(n_in, kc) + sum(widths) + 2 * max(widths)) * s + 4 * 32 + 32


def tile_rows(n_in, n_out, hidden_pi, hidden_vf, lds_bytes=65536, kc=256):
    """-> (R, bytes of the larger net's map): the largest R of 32, 16, 8, 4, 2 at which the maps of BOTH nets (actor: hidden_pi +
    [n_out], critic: hidden_vf + [1]) fit ``lds_bytes``; R is None when even R = 2 does not fit."""
    nets = (list(hidden_pi) + [n_out], list(hidden_vf) + [1])
    for rows in (32, 16, 8, 4, 2):
        need = 4 * max(lds_floats(n_in, w, rows, kc) for w in nets)
        if need <= lds_bytes:
            return rows, need
    return None, need
