"""The KL-adaptive learning-rate rule restated in numpy float32 (include/windgym_hip.h: wg_ppo_set_kl_lr) for the tests that replay
it on the host: tests/test_kl_lr_host.py (against the C++ statement of wg_train.h) and tests/test_gpu_kl_lr.py (against the device)."""
import numpy as np

F = np.float32


def np_rule(desired_kl, factor=1.5, lr_min=1e-5, lr_max=1e-2):
    """-> (kl_low, kl_high, up, down, lr_min, lr_max) as float32: the band desired_kl / 2 .. 2 desired_kl, down = 1 / factor rounded once"""
    d, f = F(desired_kl), F(factor)
    return d / F(2), F(2) * d, f, F(1) / f, F(lr_min), F(lr_max)


def np_next(lr, kl, rule):
    """One step: multiplications only; inside the band, kl == 0, kl < 0, NaN: unchanged."""
    kl_low, kl_high, up, down, lr_min, lr_max = rule
    lr, kl = F(lr), F(kl)
    if kl > kl_high:
        return max(lr_min, F(lr * down))
    if kl < kl_low and kl > 0:
        return min(lr_max, F(lr * up))
    return lr


def replay(lr0, kls, rule):
    """The rates of an update's optimiser steps from the minibatches' approx_kl in order: the first minibatch leaves the rate alone."""
    out, lr = [], F(lr0)
    for i, kl in enumerate(np.asarray(kls, F).reshape(-1)):
        if i:
            lr = np_next(lr, kl, rule)
        out.append(lr)
    return np.array(out, F)
