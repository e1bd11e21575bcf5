"""TEST INFRASTRUCTURE — restatement in torch (float64 unless told otherwise, CPU, autograd) of the recurrent trainer's rule as
include/windgym_hip.h states it for wg_lstm_ppo_grad / wg_lstm_ppo_apply; not written from windgym_amd/recurrent_ppo.py or the kernels.

A SPEC is ``dict(n_in, H, n_out, hidden_pi, hidden_vf, shared, activation)``.  FLAT parameters: per LSTM (the actor's, then the critic's
unless ``shared``) ``weight_ih_l0 [4H, n_in]``, ``weight_hh_l0 [4H, H]``, ``bias_ih_l0``, ``bias_hh_l0 [4H]``, then the MLP's: the actor's hidden
layers (weight, bias), ``action_net``, the critic's hidden layers, ``value_net``, ``log_std`` — sb3-contrib's names.

The rule, for a minibatch of the envs ``envs`` with ALL ``T`` steps of each (row order ``t * len(envs) + j``)::

    per net: (h, c) = lstm_state0[net][:, envs]                        (data: no gradient flows into it)
    for t in 0 .. T-1:  (h, c) <- where(episode_start[t], 0, (h, c));  (h, c) <- cell(x_t, h, c)      (torch.nn.LSTM's cell, i f g o)
    mean = actor MLP(h_actor rows), V = critic MLP(h_critic rows; shared: the actor's)
    loss = wg_ppo_grad's on the T * len(envs) rows (normalize_advantage: mean / unbiased std of those rows)

The gradient stops at an episode start by construction: ``where`` selects a constant there.

An entry of ``envs`` outside ``[0, B)`` is a column without an env: its ``T`` rows enter the heads as ``h = 0`` with ``raw = logp =
advantage = returns = 0``; they count in the ``T * len(envs)`` rows of every mean and of the advantage statistics, and send no gradient
into the LSTM (``where`` selects the constant 0 there too).
"""
import math

import numpy as np
import torch

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
STATS = ("pi_loss", "v_loss", "entropy", "approx_kl", "clip_fraction", "loss", "adv_mean", "adv_std")
NETS = ("lstm_actor", "lstm_critic")


def nets(spec):
    return 1 if spec["shared"] else 2


def layout(spec):
    """[(sb3-contrib name, shape)] in flat order."""
    H, n_in, out = spec["H"], spec["n_in"], []
    for net in NETS[:nets(spec)]:
        out += [(f"{net}.weight_ih_l0", (4 * H, n_in)), (f"{net}.weight_hh_l0", (4 * H, H)), (f"{net}.bias_ih_l0", (4 * H,)),
                (f"{net}.bias_hh_l0", (4 * H,))]
    for stack, head, hidden, m in (("policy_net", "action_net", spec["hidden_pi"], spec["n_out"]), ("value_net", "value_net", spec["hidden_vf"], 1)):
        k = H
        for i, h in enumerate(hidden):
            out += [(f"mlp_extractor.{stack}.{2 * i}.weight", (h, k)), (f"mlp_extractor.{stack}.{2 * i}.bias", (h,))]
            k = h
        out += [(f"{head}.weight", (m, k)), (f"{head}.bias", (m,))]
    return out + [("log_std", (spec["n_out"],))]


def n_params(spec):
    return int(sum(int(np.prod(s)) for _, s in layout(spec)))


def views(spec, flat):
    """flat (tensor or array) -> {name: view}."""
    out, o = {}, 0
    for name, shape in layout(spec):
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    assert o == flat.shape[0]
    return out


def random_params(spec, seed, dtype=np.float32):
    """A flat vector with every tensor away from 0: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) weights, U(-0.3, 0.3) biases and log_std."""
    rng = np.random.default_rng(seed)
    parts = []
    for name, shape in layout(spec):
        k = 1.0 / np.sqrt(shape[1]) if len(shape) == 2 else 0.3
        parts.append(rng.uniform(-k, k, int(np.prod(shape))))
    return np.concatenate(parts).astype(dtype)


def _mlp(p, stack, head, x, activation):
    act = torch.tanh if activation == "tanh" else torch.relu
    i = 0
    while f"mlp_extractor.{stack}.{2 * i}.weight" in p:
        x = act(x @ p[f"mlp_extractor.{stack}.{2 * i}.weight"].T + p[f"mlp_extractor.{stack}.{2 * i}.bias"])
        i += 1
    return x @ p[f"{head}.weight"].T + p[f"{head}.bias"]


def unroll(spec, p, obs, start, state0, envs):
    """-> (h rows per net ``[nets][T, Bm, H]``, final state ``[nets, 2, Bm, H]``) of the envs ``envs`` through all steps of ``obs``."""
    T = obs.shape[0]
    hs, fin = [], []
    for i, net in enumerate(NETS[:nets(spec)]):
        wih, whh = p[f"{net}.weight_ih_l0"], p[f"{net}.weight_hh_l0"]
        b = p[f"{net}.bias_ih_l0"] + p[f"{net}.bias_hh_l0"]
        h, c = state0[i, 0][envs], state0[i, 1][envs]
        out = []
        for t in range(T):
            fresh = (start[t][envs] != 0).reshape(-1, 1)
            h, c = torch.where(fresh, torch.zeros_like(h), h), torch.where(fresh, torch.zeros_like(c), c)      # a select: NaN does not get through
            z = b + obs[t][envs] @ wih.T + h @ whh.T
            zi, zf, zg, zo = z.chunk(4, dim=-1)
            c = torch.sigmoid(zf) * c + torch.sigmoid(zi) * torch.tanh(zg)
            h = torch.sigmoid(zo) * torch.tanh(c)
            out.append(h)
        hs.append(torch.stack(out))
        fin.append(torch.stack([h, c]))
    return hs, torch.stack(fin)


def _t(x, dtype):
    x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return x.to(dtype) if x.is_floating_point() else x


def loss(spec, flat, roll, envs, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, normalize_advantage=True, steps=None):
    """-> (loss tensor, stats dict of python floats, ratio tensor).  ``flat``: a torch vector (its dtype is the arithmetic's);
    ``roll``: dict(obs [T(+1), B, n_in], raw [T, B, n_out], logp, advantage, returns [T, B], episode_start [T(+1), B], lstm_state0
    [nets, 2, B, H]); ``envs``: the minibatch's env ids; ``steps``: None, or the steps t whose rows enter the loss (the mean is then
    over those rows — for the tests of what an episode start cuts)."""
    dt = flat.dtype
    T = roll["raw"].shape[0]
    envs = torch.as_tensor(np.asarray(envs), dtype=torch.long)
    r = {k: _t(v, dt) for k, v in roll.items()}
    inside = (envs >= 0) & (envs < roll["raw"].shape[1])
    if not bool(inside.all()):
        # a column without an env: evaluated on env 0 so that every index is valid, then replaced by the constant 0 where it is read
        envs = torch.where(inside, envs, torch.zeros_like(envs))
    p = views(spec, flat)
    hs, _ = unroll(spec, p, r["obs"][:T], r["episode_start"][:T], r["lstm_state0"].detach(), envs)
    if not bool(inside.all()):
        hs = [torch.where(inside.reshape(1, -1, 1), h, torch.zeros_like(h)) for h in hs]
    H = spec["H"]
    sel = slice(None) if steps is None else torch.as_tensor(list(steps), dtype=torch.long)
    pick = lambda x: x[sel].reshape((-1,) + tuple(x.shape[2:]))
    mean = _mlp(p, "policy_net", "action_net", pick(hs[0]).reshape(-1, H), spec["activation"])
    V = _mlp(p, "value_net", "value_net", pick(hs[-1]).reshape(-1, H), spec["activation"])[:, 0]
    rows = lambda x: torch.where(inside.reshape((1, -1) + (1,) * (x.ndim - 2)), x, torch.zeros_like(x))
    raw, lpo, A, ret = (pick(rows(r[k][:, envs])) for k in ("raw", "logp", "advantage", "returns"))
    ls = p["log_std"]
    z = (raw - mean) / torch.exp(ls)
    logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(1)
    lr = logp - lpo
    ratio = torch.exp(lr)
    mu, sd = torch.zeros((), dtype=dt), torch.ones((), dtype=dt)
    if normalize_advantage and A.numel() > 1:
        mu, sd = A.mean(), A.std()
        A = (A - mu) / (sd + 1e-8)
    l_pi = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - clip_range, 1.0 + clip_range) * A).mean()
    l_v = ((ret - V) ** 2).mean()
    ent = (0.5 + HALF_LOG_2PI + ls).sum()
    total = l_pi + vf_coef * l_v - ent_coef * ent
    vals = (l_pi, l_v, ent, ((ratio - 1.0) - lr).mean(), ((ratio - 1.0).abs() > clip_range).to(dt).mean(), total, mu, sd)
    stats = {k: float(v.detach()) for k, v in zip(STATS, vals)}
    return total, stats, ratio.detach()


def loss_and_grad(spec, flat, roll, envs, dtype=torch.float64, **kw):
    """-> (loss, stats, flat gradient as float64 numpy, ratio as numpy) by autograd in ``dtype``."""
    w = torch.as_tensor(np.asarray(flat)).to(dtype).clone().requires_grad_(True)
    total, stats, ratio = loss(spec, w, roll, envs, **kw)
    total.backward()
    return float(total.detach()), stats, w.grad.detach().double().numpy(), ratio.numpy()


def minibatches(perm, envs_per_batch):
    """The partition rule: minibatch j of an epoch is ``perm[j * Bm : (j + 1) * Bm]``, the last one shorter."""
    perm = np.asarray(perm)
    return [perm[s:s + envs_per_batch] for s in range(0, len(perm), envs_per_batch)]


def envs_per_batch(batch_size, n_steps, num_envs):
    """``batch_size`` (env steps, SB3's meaning) -> envs per minibatch; default ``n_steps * ceil(B / 4)``; not a multiple of
    ``n_steps``: ValueError."""
    if batch_size is None:
        return -(-num_envs // 4)
    batch_size = int(batch_size)
    if batch_size < n_steps or batch_size % n_steps:
        raise ValueError(f"batch_size = {batch_size} must be a multiple of n_steps = {n_steps}: a minibatch is a set of envs with all their steps")
    return batch_size // n_steps


def train(spec, flat, roll, perms, envs_per_mb, lr=3e-4, max_grad_norm=0.5, dtype=torch.float64, adam=None, **kw):
    """The update: per epoch's permutation and minibatch, gradient -> clipping by the global norm -> torch.optim.Adam (betas 0.9 / 0.999,
    eps 1e-5) on the ONE flat vector.  -> (new flat as float64 numpy, [stats])."""
    w = torch.as_tensor(np.asarray(flat)).to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=lr, eps=1e-5) if adam is None else adam(w)
    log = []
    for perm in perms:
        for envs in minibatches(perm, envs_per_mb):
            total, stats, _ = loss(spec, w, roll, envs, **kw)
            opt.zero_grad()
            total.backward()
            torch.nn.utils.clip_grad_norm_([w], max_grad_norm)
            opt.step()
            log.append(stats)
    return w.detach().double().numpy(), log


def random_rollout(spec, flat, T, B, seed, starts=None, state0_scale=0.5):
    """Buffers as ``venv.rollout`` leaves them, drawn at random: ``logp`` = the true log-probability under ``flat`` + N(0, 0.3) so that
    both clip sides occur.  ``starts``: uint8 ``[T + 1, B]`` or None (a few at random, every env fresh at t = 0 with probability 1/2);
    rows that start fresh at t = 0 still carry a nonzero ``lstm_state0`` unless the caller overwrites it."""
    rng = np.random.default_rng(seed)
    n_in, H, n_out = spec["n_in"], spec["H"], spec["n_out"]
    obs = rng.uniform(-1, 1, (T + 1, B, n_in)).astype(np.float32)
    if starts is None:
        starts = (rng.uniform(size=(T + 1, B)) < 0.15).astype(np.uint8)
        starts[0] = rng.uniform(size=B) < 0.5
    state0 = (state0_scale * rng.standard_normal((nets(spec), 2, B, H))).astype(np.float32)
    state0[:, 0] = np.tanh(state0[:, 0])
    w = torch.from_numpy(np.asarray(flat, np.float64))
    p = views(spec, w)
    hs, _ = unroll(spec, p, torch.from_numpy(obs[:T]).double(), torch.from_numpy(starts[:T]), torch.from_numpy(state0).double(), torch.arange(B))
    mean = _mlp(p, "policy_net", "action_net", hs[0].reshape(-1, H), spec["activation"]).numpy().reshape(T, B, n_out)
    value = _mlp(p, "value_net", "value_net", hs[-1].reshape(-1, H), spec["activation"]).numpy().reshape(T, B)
    ls = p["log_std"].numpy()
    raw = (mean + np.exp(ls) * rng.standard_normal((T, B, n_out))).astype(np.float32)
    z = (raw - mean) / np.exp(ls)
    logp = np.sum(-0.5 * z * z - ls - HALF_LOG_2PI, axis=2)
    return dict(obs=obs, raw=raw, logp=(logp + 0.3 * rng.standard_normal((T, B))).astype(np.float32),
                advantage=(rng.standard_normal((T, B)) * 2.0 + 0.5).astype(np.float32),
                returns=(value + rng.standard_normal((T, B))).astype(np.float32), episode_start=starts.astype(np.uint8), lstm_state0=state0)
