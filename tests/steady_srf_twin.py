"""Host twin of the one-launch Serial-Refine optimiser (k_steady_srf / wg_steady_optimize), written to the contract in
include/windgym_hip.h and to nothing else.  It takes the power function as an argument: on the GPU that is wg_steady_power
(k_steady), and the kernel must equal the twin bit for bit; on the CPU it is the torch evaluation of windgym_amd/steady.py
rounded to float32, which pins the twin's rules against `steady.yaw_optimizer_srf` before the twin judges the kernel.  All
conditions and all candidates of a refine step go through ONE call of the power function.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np


def index_order_sum(p):
    """sum over the last axis in index order, in float64, of float32 values (numpy's own sum is pairwise)"""
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    s = np.zeros(p.shape[:-1])
    for t in range(p.shape[-1]):
        s = s + p[..., t]
    return s


def flow_frame_x(x, y, wd):
    """flow-frame x [C, N] of every turbine about the farm centre, float64 (wd [C] degrees)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    th = np.radians(270.0 - np.asarray(wd, dtype=np.float64))[:, None]
    return (x - x.mean())[None] * np.cos(th) + (y - y.mean())[None] * np.sin(th)


def kernel_order(x, y, wd):
    """k_steady's visiting order [C, N] restated: rank by the float32 flow-frame x, ties by index (wd: what the kernel is handed)"""
    return np.argsort(flow_frame_x(x, y, np.asarray(wd, dtype=np.float32)).astype(np.float32), axis=1, kind="stable")


def check_order(order, x, y, wd, tol=1e-3):
    """`order` [C, N] is a permutation of 0 .. N-1 per condition along which the float64 flow-frame x does not decrease by more
    than `tol` metres (the kernel ranks float32 coordinates of a farm a few km wide)"""
    order = np.asarray(order)
    C, N = order.shape
    assert np.array_equal(np.sort(order, axis=1), np.broadcast_to(np.arange(N), (C, N)))
    xs = np.take_along_axis(flow_frame_x(x, y, wd), order.astype(np.int64), axis=1)
    assert (np.diff(xs, axis=1) >= -tol).all(), float(np.diff(xs, axis=1).min())


def srf_twin(power_fn, order, offsets, yaw_clip):
    """The three steps of the contract.  power_fn(yaw float64 [C, K, N], already rounded to float32) -> per-turbine powers
    [C, K, N] (float32 values); order [C, N]; offsets float64 [passes, yaw_n].  -> (yaw [C, N] float64 clamped, best [C])."""
    order = np.asarray(order, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.float64)
    C, N = order.shape
    K = offsets.shape[1]
    ar, ak = np.arange(C), np.arange(K)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)      # noqa: E731
    yaw = np.zeros((C, N))
    best = index_order_sum(power_fn(f32(yaw[:, None, :])))[:, 0]
    for r in range(offsets.shape[0]):
        for pos in range(N):
            t = order[:, pos]
            cand = np.repeat(yaw[:, None, :], K, axis=1)
            cand[ar[:, None], ak[None, :], t[:, None]] = yaw[ar, t][:, None] + offsets[r][None, :]
            P = index_order_sum(power_fn(f32(cand)))                       # [C, K]
            j = np.argmax(P, axis=1)                                       # the FIRST index of the largest power
            pj = P[ar, j]
            better = pj > best
            yaw[ar[better], t[better]] = cand[ar[better], j[better], t[better]]
            best[better] = pj[better]
    return np.clip(yaw, -yaw_clip, yaw_clip), best
