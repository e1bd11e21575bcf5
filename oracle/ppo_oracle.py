"""ORACLE / TEST INFRASTRUCTURE — float64 restatement of the training entries of include/windgym_hip.h (wg_gae / wg_gae_shared,
wg_ppo_grad / wg_ppo_grad_shared, wg_ppo_apply), written from the header's formulas and not from windgym_amd/csrc/wg_ppo.hip.

* :func:`gae_shared` is the backward recurrence, :func:`gae_shared_brute` the per-row definition it is checked against;
* :func:`shared_loss` is the minibatch loss as a float64 torch expression on the CPU; :func:`shared_loss_and_grad` takes its
  gradient from AUTOGRAD (the kernel's backward pass is hand-derived: the two share nothing), :func:`finite_difference_grad`
  from central differences;
* :func:`gae`, :func:`gae_brute`, :func:`loss` and :func:`loss_and_grad` are those with ONE agent per env, as the header defines
  the plain entries (wg_gae is wg_gae_shared with A = 1, wg_ppo_grad is wg_ppo_grad_shared on ``{batch, batch.obs, 1}``);
* :func:`adam_step` is gradient clipping by the global norm + one Adam step in numpy;
* :func:`tile_rows` is the row tile R of k_ppo_grad as windgym_amd/csrc/wg_ppo.h documents it (the LDS map of one net).

Parameters are dicts under stable-baselines3's state-dict names (weights ``[out][in]``), as in policy_oracle.py.
"""
from __future__ import annotations

import math

import numpy as np

STATS = ("pi_loss", "v_loss", "entropy", "approx_kl", "clip_fraction", "loss", "adv_mean", "adv_std")      # wg_ppo_stats


def gae_shared(reward, value, final_value, truncated, gamma, lam):
    """Shared-reward GAE: reward / truncated [T, B] belong to the env, value / final_value [T, B, A] to its agents.
    delta[t, b, a] = reward[t, b] + gamma final_value[t, b, a] - value[t, b, a],
    A[t, b, a] = delta[t, b, a] + gamma lam (1 - truncated[t, b]) A[t + 1, b, a], A[T] = 0, returns = A + value."""
    r = np.asarray(reward, np.float64)
    v, fv = np.asarray(value, np.float64), np.asarray(final_value, np.float64)
    cont = 1.0 - np.asarray(truncated).astype(np.float64)
    T, B, A = v.shape
    assert r.shape == (T, B) and cont.shape == (T, B) and fv.shape == (T, B, A)
    adv = np.zeros_like(v)
    a = np.zeros((B, A))
    for t in range(T - 1, -1, -1):
        a = r[t][:, None] + gamma * fv[t] - v[t] + gamma * lam * cont[t][:, None] * a
        adv[t] = a
    return adv, adv + v


def gae_shared_brute(reward, value, final_value, truncated, gamma, lam):
    """The same by definition, one agent row at a time: A_t = sum_{s >= t} (gamma lam)^(s - t) delta_s over the steps up to and
    including the env's first truncation at or after t (or the end of the buffer)."""
    r = np.asarray(reward, np.float64)
    v, fv = np.asarray(value, np.float64), np.asarray(final_value, np.float64)
    tr = np.asarray(truncated).astype(bool)
    T, B, A = v.shape
    adv = np.zeros((T, B, A))
    for b in range(B):
        for a in range(A):
            for t in range(T):
                s, w, acc = t, 1.0, 0.0
                while s < T:
                    acc += w * (r[s, b] + gamma * fv[s, b, a] - v[s, b, a])
                    if tr[s, b]:
                        break
                    w *= gamma * lam
                    s += 1
                adv[t, b, a] = acc
    return adv, adv + v


def _one_agent(f, reward, value, final_value, truncated, gamma, lam):
    adv, ret = f(reward, np.asarray(value)[..., None], np.asarray(final_value)[..., None], truncated, gamma, lam)
    return adv[..., 0], ret[..., 0]


def gae(*args):
    """[T, B] float64 (advantage, returns): :func:`gae_shared` with one agent per env."""
    return _one_agent(gae_shared, *args)


def gae_brute(*args):
    """:func:`gae_shared_brute` with one agent per env."""
    return _one_agent(gae_shared_brute, *args)


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
    """The header's loss (wg_ppo_grad_shared) on float64 CPU tensors; ``tp`` = {SB3 name: tensor}.  A minibatch is a list ``ids`` of
    AGENT rows (any integers); entry ``id`` belongs to env row ``e = id // agents``:
      * the actor term uses ``obs[id]``, ``raw[id]``, ``logp_old[id]`` and ``A = advantage[e]``;
      * the advantage normalisation is the mean / unbiased std of ``advantage[id // agents]`` over the minibatch's entries;
      * the critic term is ``(returns[e] - V(obs_vf[e]))**2``, averaged over the ENTRIES (an env row drawn through two of its
        agents counts twice).
    Entries outside ``[0, n_agent_rows)`` are skipped: they add nothing to any sum, and every mean still divides by the number of
    entries asked for.  -> (loss, dict of the eight statistics, ratio of the entries kept)."""
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
    return total, stats, ratio


def loss(tp, obs, raw, logp_old, advantage, returns, **kw):
    """The plain entry's loss (wg_ppo_grad): every row once, one agent per env, the critic on the actor's rows."""
    return shared_loss(tp, obs, obs, raw, logp_old, advantage, returns, np.arange(obs.shape[0]), 1, **kw)


def _tensors(params, arrays, requires_grad):
    import torch
    tp = {k: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64, requires_grad=requires_grad) for k, v in params.items()}
    return tp, [torch.tensor(np.asarray(x, np.float64), dtype=torch.float64) for x in arrays]


def shared_loss_and_grad(params, obs, obs_vf, raw, logp_old, advantage, returns, ids, agents, **kw):
    """numpy in, numpy out -> (loss, {name: d loss / d tensor} from AUTOGRAD, statistics dict, ratio)."""
    tp, args = _tensors(params, (obs, obs_vf, raw, logp_old, advantage, returns), True)
    total, stats, ratio = shared_loss(tp, *args, ids, agents, **kw)
    total.backward()
    grads = {k: (np.zeros(v.shape) if v.grad is None else v.grad.numpy().copy()) for k, v in tp.items()}
    return float(total.detach()), grads, {k: float(v.detach()) for k, v in stats.items()}, ratio.detach().numpy()


def loss_and_grad(params, obs, raw, logp_old, advantage, returns, **kw):
    """:func:`shared_loss_and_grad` of the plain entry (see :func:`loss`)."""
    return shared_loss_and_grad(params, obs, obs, raw, logp_old, advantage, returns, np.arange(len(obs)), 1, **kw)


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
    """Floats of wg_ppo.h's LDS map (WgPpoLds) of ONE net whose input width is ``n_in``, for tiles of ``rows`` rows; ``widths`` = the
    M of every layer, head included.  S = rows + 1 floats per feature row: xin [min(n_in, kc)][S], act [sum M][S],
    d [2][max M][S], then rowv [4][32] and rid [32]."""
    s = rows + 1
    return (min(n_in, kc) + sum(widths) + 2 * max(widths)) * s + 4 * 32 + 32


def tile_rows(n_in, n_out, hidden_pi, hidden_vf, lds_bytes=65536, kc=256, n_in_vf=None):
    """-> (R, bytes of the larger net's map): the largest R of 32, 16, 8, 4, 2 at which the maps of BOTH nets (actor: hidden_pi +
    [n_out] on ``n_in`` inputs, critic: hidden_vf + [1] on ``n_in_vf``, default the actor's) fit ``lds_bytes``; R is None when
    even R = 2 does not fit.  A restatement for sizing test cases (which minibatch lengths are ragged); nothing compares it with
    the library's R, which is not exposed."""
    nets = ((n_in, list(hidden_pi) + [n_out]), (n_in if n_in_vf is None else n_in_vf, list(hidden_vf) + [1]))
    for rows in (32, 16, 8, 4, 2):
        need = 4 * max(lds_floats(k, w, rows, kc) for k, w in nets)
        if need <= lds_bytes:
            return rows, need
    return None, need
