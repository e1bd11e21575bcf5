// wg_yaw_table.h — the node rule of the yaw table (include/windgym_hip.h: wg_yaw_table_*), stated ONCE: the kernels of
// wg_yaw_table.hip compile it for the device, tests/yaw_table_shim.cpp compiles it with g++ alone, tests/yaw_table_twin.py restates
// it in numpy.  No HIP header is needed to include this file.
//
// A table holds the Serial-Refine optimum of every node of a grid over (ti, ws, wd) — ti slowest, wd fastest.  A lookup takes the
// NEAREST node of every axis; it does not interpolate: the optimum is an argmax over discrete candidates and is not continuous in
// the wind (halfway between a +25 deg node and a -25 deg node an interpolated answer is 0 deg, the worst of the three).
//
// One axis with nodes a_0 < ... < a_{n-1} and a value x, all in double:
//     i = the number of midpoints m_k = (a_k + a_{k+1}) / 2, k = 0 .. n-2, with m_k < x
// so a tie goes to the lower node and x below / above the axis goes to the end node.  With `wrap` (the caller's statement that the
// axis covers the full circle, degrees) x is first reduced to [a_0, a_0 + 360) by
//     r = fmod(x - a_0, 360);  if (r < 0) r += 360;  x = a_0 + r
// and the axis gains the virtual node a_n = a_0 + 360, which maps to index 0 (its midpoint m_{n-1} = (a_{n-1} + a_n) / 2 counts like
// the others).  The midpoints ascend with the nodes, so the count is found by bisection.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define WG_YT_HD __host__ __device__
#else
#define WG_YT_HD
#endif

#define WG_YT_MAX_NODES 1024      // nodes of the three axes together: what a workgroup stages in LDS (8 KB)

WG_YT_HD inline int wg_yt_axis(const double* a, const int n, double x, const int wrap) {
    if (wrap) {
        double r = fmod(x - a[0], 360.0);
        if (r < 0.0) r += 360.0;
        x = a[0] + r;
    }
    int lo = 0, hi = wrap ? n : n - 1;      // the count lies in [lo, hi]
    while (lo < hi) {
        const int k = (lo + hi) >> 1;
        const double up = k + 1 < n ? a[k + 1] : a[0] + 360.0;
        if ((a[k] + up) / 2.0 < x) lo = k + 1;
        else hi = k;
    }
    return lo == n ? 0 : lo;
}

WG_YT_HD inline bool wg_yt_finite(const double x) { return fabs(x) <= 1.7976931348623157e308; }

// the row of the wind (ws, wd, ti) — the order WG_INFO_WIND_F64 reports — in a table whose axes lie back to back in `ax`: ti
// [n_ti], ws [n_ws], wd [n_wd]; -1 for a wind with a non-finite component
WG_YT_HD inline int wg_yt_row(const double* ax, const int n_ti, const int n_ws, const int n_wd, const int wrap_wd, const double ws,
                              const double wd, const double ti) {
    if (!(wg_yt_finite(ws) && wg_yt_finite(wd) && wg_yt_finite(ti))) return -1;
    const int i_ti = wg_yt_axis(ax, n_ti, ti, 0);
    const int i_ws = wg_yt_axis(ax + n_ti, n_ws, ws, 0);
    const int i_wd = wg_yt_axis(ax + n_ti + n_ws, n_wd, wd, wrap_wd);
    return (i_ti * n_ws + i_ws) * n_wd + i_wd;
}

#if defined(__HIPCC__)
#include "../../include/windgym_hip.h"
// The expert's action (windgym_hip.h: wg_expert_labels): the action that the env's actuation rule turns into the largest move from
// the yaw `prev` towards the target g — the inverse of the rule, in double; the caller rounds it once.  lo / hi / step: yaw_min /
// yaw_max / yaw_step as the step kernels hold them (floats), widened.  k_expert_labels and k_yaw_table_act both call this.
__device__ __forceinline__ double wg_expert_action(const int action_method, const double g, const double prev, const double lo,
                                                   const double hi, const double step) {
    return action_method == WG_ACT_YAW ? fmin(fmax((g - prev) / step, -1.0), 1.0) : (g - lo) / (hi - lo) * 2.0 - 1.0;
}
#endif
