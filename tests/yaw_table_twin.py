"""Twins of the yaw table (windgym_amd/yaw_table.py; tests/test_yaw_table.py checks them on the CPU, tests/test_gpu_yaw_table.py holds
the kernels against them): the node rule of windgym_amd/csrc/wg_yaw_table.h in float64 numpy — the count of midpoints below the
value, written as a sum over a comparison and not as a search — the row formula, the gather, and the action k_yaw_table_act writes."""
import numpy as np


def axis_index(a, x, wrap=False):
    """The node of every value ``x [...]`` on the axis ``a``: the number of midpoints ``(a_k + a_{k+1}) / 2`` below it (int64).
    ``wrap``: ``x`` is first reduced to ``[a_0, a_0 + 360)`` and a virtual node ``a_0 + 360`` maps to index 0.  NaN -> 0."""
    a, x = np.asarray(a, np.float64), np.asarray(x, np.float64)
    nodes = a
    if wrap:
        with np.errstate(invalid="ignore"):
            r = np.fmod(x - a[0], 360.0)
        r = np.where(r < 0.0, r + 360.0, r)
        x = a[0] + r
        nodes = np.append(a, a[0] + 360.0)
    mid = (nodes[:-1] + nodes[1:]) / 2.0
    i = (mid < x[..., None]).sum(axis=-1)
    return np.where(i == len(a), 0, i) if wrap else i


def rows(ti, ws, wd, wind, mask=None, wrap_wd=False):
    """wg_yaw_table_rows: ``wind [..., 3]`` (ws, wd, ti) -> int32 ``[...]``; -1 where the mask is 0 or a component is not finite."""
    wind = np.asarray(wind, np.float64)
    i_ti = axis_index(ti, wind[..., 2])
    i_ws = axis_index(ws, wind[..., 0])
    i_wd = axis_index(wd, wind[..., 1], wrap_wd)
    r = (i_ti * len(ws) + i_ws) * len(wd) + i_wd
    ok = np.isfinite(wind).all(axis=-1)
    if mask is not None:
        ok = ok & (np.asarray(mask) != 0)
    return np.where(ok, r, -1).astype(np.int32)


def targets(yaw, r, out):
    """wg_yaw_table_targets on rows ``r``: the gathered yaws, ``out``'s row where r is -1"""
    r = np.asarray(r)
    return np.where((r >= 0)[..., None], np.asarray(yaw)[np.maximum(r, 0)], out)


def action(method, g, prev, yaw_min, yaw_max, yaw_step):
    """wg_expert_labels' action in float64, rounded once: ``g`` the target yaws (float64), ``prev`` the current yaws (float32); the
    limits are the env's float32 values widened to double, as the kernels hold them."""
    lo, hi, step = (np.float64(np.float32(v)) for v in (yaw_min, yaw_max, yaw_step))
    g, prev = np.asarray(g, np.float64), np.asarray(prev, np.float32).astype(np.float64)
    if method == "yaw":
        return np.minimum(np.maximum((g - prev) / step, -1.0), 1.0).astype(np.float32)
    return ((g - lo) / (hi - lo) * 2.0 - 1.0).astype(np.float32) + np.zeros_like(prev, np.float32)
