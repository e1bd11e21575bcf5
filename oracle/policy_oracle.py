"""ORACLE / TEST INFRASTRUCTURE — numpy restatement of the MLP actor-critic of windgym_amd/csrc/wg_policy.hip.

Written from the formulas of include/windgym_hip.h (wg_policy_act), not from windgym_amd/policy.py: float64 forward of the
actor and the critic, the Philox4x32-10 + Box-Muller noise stream of a stochastic call, the sample and its log-probability.
Parameters are a dict under stable-baselines3's state-dict names (weights ``[out][in]``).
"""
from __future__ import annotations

import numpy as np

NOISE_TAG = 0x50000000
_M32 = np.uint64(0xFFFFFFFF)


def _net(params, prefix, head, obs, activation):
    x = np.asarray(obs, dtype=np.float64)
    i = 0
    while f"{prefix}.{i}.weight" in params:
        x = x @ np.asarray(params[f"{prefix}.{i}.weight"], np.float64).T + np.asarray(params[f"{prefix}.{i}.bias"], np.float64)
        x = np.tanh(x) if activation == "tanh" else np.maximum(x, 0.0)
        i += 2
    return x @ np.asarray(params[head + ".weight"], np.float64).T + np.asarray(params[head + ".bias"], np.float64)


def forward(params, obs, activation="tanh"):
    """-> (mean f64[rows, n_out], value f64[rows] or None)."""
    mean = _net(params, "mlp_extractor.policy_net", "action_net", obs, activation)
    value = _net(params, "mlp_extractor.value_net", "value_net", obs, activation)[..., 0] if "value_net.weight" in params else None
    return mean, value


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) on uint32 arrays: ctr [..., 4], key [..., 2] -> [..., 4]."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = (np.asarray(key[..., i], dtype=np.uint64) for i in range(2))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack(c, axis=-1).astype(np.uint32)


def policy_noise(seed, counter, rows, n_out):
    """eps f32[len(rows), n_out] of a stochastic wg_policy_act: key = (seed lo, seed hi), counter words = (g lo, counter lo,
    counter hi, 0x50000000 | ((g hi) & 0xffff) << 8 | j // 2) for global row g = row + row_offset; output words (o0, o1) ->
    u1 = ((o0 >> 8) + 1) / 2^24, u2 = (o1 >> 8) / 2^24, eps_j = sqrt(-2 ln u1) * (cos | sin)(2 pi u2) for j even | odd,
    in float32 arithmetic like the kernel's."""
    g = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    j = np.arange(n_out, dtype=np.uint64).reshape(1, -1)
    seed, counter = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), np.uint64(int(counter) & 0xFFFFFFFFFFFFFFFF)
    shape = (g.shape[0], n_out)
    ctr = np.zeros(shape + (4,), dtype=np.uint64)
    ctr[..., 0] = np.broadcast_to(g & _M32, shape)
    ctr[..., 1] = counter & _M32
    ctr[..., 2] = counter >> np.uint64(32)
    ctr[..., 3] = np.uint64(NOISE_TAG) | (((g >> np.uint64(32)) & np.uint64(0xFFFF)) << np.uint64(8)) | (j >> np.uint64(1))
    key = np.zeros(shape + (2,), dtype=np.uint64)
    key[..., 0], key[..., 1] = seed & _M32, seed >> np.uint64(32)
    o = philox4x32_10(ctr, key)
    u1 = ((o[..., 0] >> 8).astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)
    u2 = (o[..., 1] >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)
    r = np.sqrt(np.float32(-2.0) * np.log(u1))
    ph = np.float32(6.2831853071795864) * u2
    odd = (np.arange(n_out) & 1).astype(bool).reshape(1, -1)
    return np.where(odd, r * np.sin(ph), r * np.cos(ph)).astype(np.float32)


def sample(params, obs, eps=None, activation="tanh"):
    """-> dict(mean, raw, action, logp, value) in float64; eps None = deterministic (the density at the mean)."""
    mean, value = forward(params, obs, activation)
    log_std = np.asarray(params["log_std"], np.float64) if "log_std" in params else np.zeros(mean.shape[-1])
    e = np.zeros_like(mean) if eps is None else np.asarray(eps, np.float64)
    raw = mean + np.exp(log_std) * e
    logp = np.sum(-0.5 * e * e - log_std - 0.5 * np.log(2.0 * np.pi), axis=-1)
    return dict(mean=mean, raw=raw, action=np.clip(raw, -1.0, 1.0), logp=logp, value=value)
