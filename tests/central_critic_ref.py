"""float64 references of the centralised-critic path (one shared actor per turbine, ONE critic per env on the flat observation),
kept with the tests and written from the definition in include/windgym_hip.h (wg_ppo_grad_shared), not from the kernel.

A minibatch is a list of AGENT rows; entry ``id`` belongs to env row ``e = id // agents``:
  * the actor term uses ``obs[id]``, ``raw[id]``, ``logp_old[id]`` and ``A = advantage[e]``;
  * the advantage normalisation is the mean / unbiased std of ``advantage[id // agents]`` over the minibatch's entries;
  * the critic term is ``(returns[e] - V(obs_vf[e]))**2``, averaged over the ENTRIES (an env row drawn through two of its agents
    counts twice).
Entries outside ``[0, n_agent_rows)`` are skipped: they add nothing to any sum, and every mean still divides by the number of
entries asked for.
"""
import math

import numpy as np

STATS = ("pi_loss", "v_loss", "entropy", "approx_kl", "clip_fraction", "loss", "adv_mean", "adv_std")      # wg_ppo_stats


def _net(tp, prefix, head, x, activation):
    import torch
    i = 0
    while f"{prefix}.{i}.weight" in tp:
        x = x @ tp[f"{prefix}.{i}.weight"].T + tp[f"{prefix}.{i}.bias"]
        x = torch.tanh(x) if activation == "tanh" else torch.relu(x)
        i += 2
    return x @ tp[head + ".weight"].T + tp[head + ".bias"]


def shared_loss(tp, obs, obs_vf, raw, logp_old, advantage, returns, ids, agents, clip_range=0.2, vf_coef=0.5, ent_coef=0.0,
                normalize_advantage=True, activation="tanh"):
    """float64 CPU tensors; ``tp`` = {SB3 name: tensor}; ``ids``: the minibatch's entries (any integers).
    -> (loss, dict of the eight statistics)."""
    import torch
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    ok = ids[(ids >= 0) & (ids < obs.shape[0])]
    e = ok // agents
    mean = _net(tp, "mlp_extractor.policy_net", "action_net", obs[ok], activation)
    V = _net(tp, "mlp_extractor.value_net", "value_net", obs_vf[e], activation)[:, 0]
    ls = tp["log_std"]
    z = (raw[ok] - mean) / torch.exp(ls)
    logp = (-0.5 * z * z - ls - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)
    lr = logp - logp_old[ok]
    ratio = torch.exp(lr)
    A = advantage[e]
    adv_mean, adv_std = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)
    if normalize_advantage and n > 1:
        adv_mean = A.sum() / n
        adv_std = torch.sqrt(((A - adv_mean) ** 2).sum() / (n - 1))
        A = (A - adv_mean) / (adv_std + 1e-8)
    l_pi = -torch.minimum(ratio * A, torch.clamp(ratio, 1.0 - clip_range, 1.0 + clip_range) * A)
    l_v = (returns[e] - V) ** 2
    H = (0.5 + 0.5 * math.log(2.0 * math.pi) + ls).sum()
    total = l_pi.sum() / n + vf_coef * l_v.sum() / n - ent_coef * H
    stats = dict(pi_loss=l_pi.sum() / n, v_loss=l_v.sum() / n, entropy=H, approx_kl=((ratio - 1.0) - lr).sum() / n,
                 clip_fraction=((ratio - 1.0).abs() > clip_range).double().sum() / n, loss=total, adv_mean=adv_mean, adv_std=adv_std)
    return total, stats


def _tensors(params, arrays, requires_grad):
    import torch
    tp = {k: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64, requires_grad=requires_grad) for k, v in params.items()}
    return tp, [torch.tensor(np.asarray(x, np.float64), dtype=torch.float64) for x in arrays]


def shared_loss_and_grad(params, obs, obs_vf, raw, logp_old, advantage, returns, ids, agents, **kw):
    """numpy in, numpy out -> (loss, {name: d loss / d tensor} from AUTOGRAD, statistics dict)."""
    tp, args = _tensors(params, (obs, obs_vf, raw, logp_old, advantage, returns), True)
    total, stats = shared_loss(tp, *args, ids, agents, **kw)
    total.backward()
    grads = {k: (np.zeros(v.shape) if v.grad is None else v.grad.numpy().copy()) for k, v in tp.items()}
    return float(total.detach()), grads, {k: float(v.detach()) for k, v in stats.items()}


def shared_loss_value(params, obs, obs_vf, raw, logp_old, advantage, returns, ids, agents, **kw):
    """The loss alone (what finite differences call)."""
    tp, args = _tensors(params, (obs, obs_vf, raw, logp_old, advantage, returns), False)
    return float(shared_loss(tp, *args, ids, agents, **kw)[0])


def finite_difference_grad(params, *args, h=1e-6, **kw):
    """Central differences of :func:`shared_loss_value` in every parameter -> {name: array}."""
    out = {}
    for name, a in params.items():
        g = np.zeros(a.shape)
        for i in np.ndindex(*a.shape):
            hi, lo = {k: v.copy() for k, v in params.items()}, {k: v.copy() for k, v in params.items()}
            hi[name][i] += h
            lo[name][i] -= h
            g[i] = (shared_loss_value(hi, *args, **kw) - shared_loss_value(lo, *args, **kw)) / (2.0 * h)
        out[name] = g
    return out


def lds_floats(n_in, widths, rows, kc=256):
    """Floats of wg_ppo.h's LDS map of ONE net whose input width is ``n_in``, for tiles of ``rows`` rows (``widths``: the M of every
    layer, head included): xin [min(n_in, kc)][S], act [sum M][S], d [2][max M][S], S = rows + 1, then rowv [4][32] and rid [32]."""
    s = rows + 1
    return (min(n_in, kc) + sum(widths) + 2 * max(widths)) * s + 4 * 32 + 32


def tile_rows(n_in, n_in_vf, n_out, hidden_pi, hidden_vf, lds_bytes=65536):
    """The row tile R of k_ppo_grad for a policy whose critic reads ``n_in_vf`` inputs: the largest of 32, 16, 8, 4, 2 at which the
    maps of both nets — each with its OWN input width — fit ``lds_bytes``.  A restatement for sizing test cases (which minibatch
    lengths are ragged); nothing compares it with the library's R, which is not exposed."""
    for rows in (32, 16, 8, 4, 2):
        need = 4 * max(lds_floats(n_in, list(hidden_pi) + [n_out], rows), lds_floats(n_in_vf, list(hidden_vf) + [1], rows))
        if need <= lds_bytes:
            return rows
    return None
