"""TEST INFRASTRUCTURE — the rule of wg_lstm_bc_grad / wg_lstm_bc_update as include/windgym_hip.h states it, in torch (float64 unless
told otherwise, CPU, autograd): ``lstm_bptt_twin.unroll`` in front, then ``imitation_twin.bc_loss``'s two heads on the h rows.  Written
from the header's rule, not from windgym_amd/recurrent_imitation.py or the kernels.

SPEC, FLAT and the parameter layout are lstm_bptt_twin's.  A ROLLOUT is ``dict(obs [T(+1), B, n_in], labels [T, B, n_out], returns
[T, B] or None / absent, episode_start [T(+1), B], lstm_state0 [nets, 2, B, H])``.  For a minibatch of the envs ``envs`` with ALL
``T`` steps of each (row order ``t * len(envs) + j``, ``n = T * len(envs)`` rows)::

    h rows per net = lstm_bptt_twin.unroll(...)            (lstm_state0 is data, episode_start the select: the gradient stops there)
    actor term     = imitation_twin.bc_loss on the ACTOR LSTM's h rows and the labels:  mse,  or  nll - ent_coef * H
    critic term    = vf_coef * v_loss of imitation_twin.bc_loss on the CRITIC LSTM's h rows (shared: the actor's) — only with returns

An entry of ``envs`` outside ``[0, B)`` is a column without an env: its ``T`` rows reach the heads as ``h = 0`` with ``target =
returns = 0``, count in ``n``, and send nothing into the LSTM (``where`` selects a constant).
"""
import numpy as np
import torch

import imitation_twin as it
import lstm_bptt_twin as tw

STATS = it.BC_STATS


def loss(spec, flat, roll, envs, loss="mse", ent_coef=0.0, vf_coef=0.0):
    """-> (loss tensor, stats dict of python floats in the order of STATS).  ``flat``: a torch vector (its dtype is the arithmetic's)."""
    dt = flat.dtype
    lab = tw._t(roll["labels"], dt)
    T, B = lab.shape[:2]
    envs = torch.as_tensor(np.asarray(envs), dtype=torch.long)
    inside = (envs >= 0) & (envs < B)
    safe = torch.where(inside, envs, torch.zeros_like(envs))      # evaluated on env 0, replaced by the constant 0 wherever it is read
    p = tw.views(spec, flat)
    hs, _ = tw.unroll(spec, p, tw._t(roll["obs"], dt)[:T], tw._t(roll["episode_start"], dt)[:T], tw._t(roll["lstm_state0"], dt).detach(), safe)
    col = lambda x: torch.where(inside.reshape((1, -1) + (1,) * (x.ndim - 2)), x, torch.zeros_like(x))
    H, n = spec["H"], T * len(envs)
    ids = np.arange(n)
    h_pi, h_vf = col(hs[0]).reshape(n, H), col(hs[-1]).reshape(n, H)
    target = col(lab[:, safe]).reshape(n, spec["n_out"])
    kw = dict(loss=loss, ent_coef=ent_coef, vf_coef=vf_coef, activation=spec["activation"])
    total, stats = it.bc_loss(p, h_pi, target, None, ids, **kw)
    if roll.get("returns") is not None:
        ret = col(tw._t(roll["returns"], dt)[:, safe]).reshape(n)
        stats["v_loss"] = it.bc_loss(p, h_vf, target, ret, ids, **kw)[1]["v_loss"]
        total = total + vf_coef * stats["v_loss"]
        stats["loss"] = total
    return total, {k: float(torch.as_tensor(stats[k]).detach()) for k in STATS}


def loss_and_grad(spec, flat, roll, envs, dtype=torch.float64, **kw):
    """-> (loss, stats, flat gradient as float64 numpy) by autograd in ``dtype``."""
    w = torch.as_tensor(np.asarray(flat)).to(dtype).clone().requires_grad_(True)
    total, stats = loss(spec, w, roll, envs, **kw)
    total.backward()
    return float(total.detach()), stats, w.grad.detach().double().numpy()


def loss_value(spec, flat, roll, envs, **kw):
    with torch.no_grad():
        return float(loss(spec, torch.as_tensor(np.asarray(flat, np.float64)), roll, envs, **kw)[0])


def finite_difference_grad(spec, flat, roll, envs, index, h=1e-6, **kw):
    """Central differences of the float64 loss in the flat entries ``index`` -> array."""
    flat = np.asarray(flat, np.float64)
    out = np.zeros(len(index))
    for k, i in enumerate(index):
        hi, lo = flat.copy(), flat.copy()
        hi[i] += h
        lo[i] -= h
        out[k] = (loss_value(spec, hi, roll, envs, **kw) - loss_value(spec, lo, roll, envs, **kw)) / (2.0 * h)
    return out


def train(spec, flat, roll, perms, envs_per_mb, lr=1e-3, max_grad_norm=0.5, dtype=torch.float64, **kw):
    """The update: per epoch's permutation and minibatch (``lstm_bptt_twin.minibatches``), gradient -> clipping by the global norm ->
    torch.optim.Adam (betas 0.9 / 0.999, eps 1e-5) on the ONE flat vector.  -> (new flat as float64 numpy, [stats])."""
    w = torch.as_tensor(np.asarray(flat)).to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=lr, eps=1e-5)
    log = []
    for perm in perms:
        for envs in tw.minibatches(perm, envs_per_mb):
            total, stats = loss(spec, w, roll, envs, **kw)
            opt.zero_grad()
            total.backward()
            torch.nn.utils.clip_grad_norm_([w], max_grad_norm)
            opt.step()
            log.append(stats)
    return w.detach().double().numpy(), log


def random_rollout(spec, flat, T, B, seed, starts=None, sigma=0.3):
    """``lstm_bptt_twin.random_rollout``'s buffers with ``labels`` drawn around the actor's mean under ``flat`` with ``sigma`` (as
    test_gpu_imitation.py's ``bc_rows`` draws its targets) and ``returns`` around the critic's value; the PPO keys stay, so the same
    dict also feeds wg_lstm_ppo_grad."""
    roll = tw.random_rollout(spec, flat, T, B, seed, starts=starts)
    rng = np.random.default_rng(seed + 1000)
    w = torch.from_numpy(np.asarray(flat, np.float64))
    p = tw.views(spec, w)
    hs, _ = tw.unroll(spec, p, torch.from_numpy(roll["obs"][:T]).double(), torch.from_numpy(roll["episode_start"][:T]),
                      torch.from_numpy(roll["lstm_state0"]).double(), torch.arange(B))
    mean = tw._mlp(p, "policy_net", "action_net", hs[0].reshape(-1, spec["H"]), spec["activation"]).numpy().reshape(T, B, spec["n_out"])
    roll["labels"] = (mean + sigma * rng.standard_normal(mean.shape)).astype(np.float32)
    return roll
