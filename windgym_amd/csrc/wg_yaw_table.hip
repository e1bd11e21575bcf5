// wg_yaw_table.hip — the yaw table: the Serial-Refine optimiser's yaws on a grid of (ti, ws, wd) nodes, resident on the device, and
// the three small kernels that look it up (include/windgym_hip.h states the contracts, wg_yaw_table.h the node rule).
//
//   k_yaw_table_rows     one thread per wind: the row of its nearest node, -1 where a mask says so or the wind is not finite
//   k_yaw_table_targets  one thread per (wind, turbine): the yaws of the wind's row, gathered
//   k_yaw_table_act      one thread per (env, turbine): the env's CURRENT wind -> row -> the expert's action from the agent farm's
//                        current yaw (wg_expert_action, what k_expert_labels writes) — the table as a scripted agent in the closed loop
//
// Every workgroup stages the three axes in LDS once (at most WG_YT_MAX_NODES doubles) and bisects them there; the threads of an
// env repeat its three bisections (a few dozen LDS reads) instead of sharing them through another barrier.  Loads and stores are
// plain and coalesced over the output index; nothing is allocated after wg_yaw_table_create, nothing is atomic, nothing is summed.
// The launches are latency bound and small next to a step kernel.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "../../include/windgym_hip.h"
#include "wg_host.h"
#include "wg_state.h"
#include "wg_yaw_table.h"

struct wg_yaw_table_s {
    int device = 0, N = 0, n_ti = 0, n_ws = 0, n_wd = 0, wrap_wd = 0;
    long long C = 0;
    WgDevMem mem;                 // one allocation: the axes (ti, ws, wd back to back), then yaw [C][N]
    const double* axes = nullptr;
    const double* yaw = nullptr;
};

namespace {

struct YtP {                      // what the kernels read of a table
    int N, n_ti, n_ws, n_wd, wrap_wd;
    const double* axes;
    const double* yaw;
};

__device__ __forceinline__ void yt_stage(const YtP& t, double* ax) {
    const int n_all = t.n_ti + t.n_ws + t.n_wd;
    for (int k = threadIdx.x; k < n_all; k += blockDim.x) ax[k] = t.axes[k];
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_yaw_table_rows(const YtP t, const int n, const double* __restrict__ wind,
                                                        const uint8_t* __restrict__ mask, int32_t* __restrict__ rows) {
    __shared__ double ax[WG_YT_MAX_NODES];
    yt_stage(t, ax);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int r = -1;
    if (!mask || mask[i]) r = wg_yt_row(ax, t.n_ti, t.n_ws, t.n_wd, t.wrap_wd, wind[(size_t)i * 3], wind[(size_t)i * 3 + 1], wind[(size_t)i * 3 + 2]);
    rows[i] = r;
}

__global__ __launch_bounds__(256) void k_yaw_table_targets(const YtP t, const long long total, const double* __restrict__ wind,
                                                           double* __restrict__ out) {
    __shared__ double ax[WG_YT_MAX_NODES];
    yt_stage(t, ax);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long w = i / t.N;
    const int k = (int)(i - w * t.N);
    const int r = wg_yt_row(ax, t.n_ti, t.n_ws, t.n_wd, t.wrap_wd, wind[w * 3], wind[w * 3 + 1], wind[w * 3 + 2]);
    if (r >= 0) out[i] = t.yaw[(size_t)r * t.N + k];
}

struct YtActP {                   // what k_yaw_table_act reads of the handle: k_info's view of the live episode
    int B, N, F, action_method;
    double lo, hi, step;          // yaw_min / yaw_max / yaw_step as the step kernels hold them, widened
    const WgEnv* env;
    const WgCtx* ctx;
    const float* yaw;
};

__global__ __launch_bounds__(256) void k_yaw_table_act(const YtP t, const YtActP p, float* __restrict__ action) {
    __shared__ double ax[WG_YT_MAX_NODES];
    yt_stage(t, ax);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.B * p.N) return;
    const int e = i / p.N, k = i - e * p.N;
    const int ctx_id = e * 2 + p.env[e].live;                      // (k_info: WG_INFO_WIND_F64 and WG_INFO_YAW_AGENT read these)
    const WgCtx& cx = p.ctx[ctx_id];
    const int r = wg_yt_row(ax, t.n_ti, t.n_ws, t.n_wd, t.wrap_wd, cx.ws, cx.wd, cx.ti);
    float a = 0.0f;                                                // (a non-finite wind, which no env samples, has no row)
    if (r >= 0) {
        const double prev = (double)p.yaw[(size_t)(ctx_id * p.F) * p.N + k];
        a = (float)wg_expert_action(p.action_method, t.yaw[(size_t)r * t.N + k], prev, p.lo, p.hi, p.step);
    }
    action[i] = a;
}

YtP yt_params(const wg_yaw_table_s* t) { return {t->N, t->n_ti, t->n_ws, t->n_wd, t->wrap_wd, t->axes, t->yaw}; }

int yt_axis_check(const char* name, const double* a, int n) {
    const std::string who = std::string("wg_yaw_table_create: ") + name;
    if (!a) return wg_fail(WG_ERR_INVALID, who + " is null");
    if (n < 1) return wg_fail(WG_ERR_INVALID, who + " is empty (n_" + name + " = " + std::to_string(n) + ")");
    for (int k = 0; k < n; ++k) {
        if (!wg_yt_finite(a[k])) return wg_fail(WG_ERR_INVALID, who + "[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(a[k] > a[k - 1])) return wg_fail(WG_ERR_INVALID, who + " is not strictly ascending at index " + std::to_string(k));
    }
    return 0;
}

// a buffer a kernel will touch must be device memory of the table's device
const char* const YT_WHOSE = ", the table's device";

}  // namespace

extern "C" int wg_yaw_table_create(int device, const double* ti, int n_ti, const double* ws, int n_ws, const double* wd, int n_wd,
                                   int wrap_wd, int N, const double* yaw, int on_device, wg_yaw_table* out) {
    if (!out) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_create: out is null");
    if (int rc = yt_axis_check("ti", ti, n_ti)) return rc;
    if (int rc = yt_axis_check("ws", ws, n_ws)) return rc;
    if (int rc = yt_axis_check("wd", wd, n_wd)) return rc;
    const long long n_all = (long long)n_ti + n_ws + n_wd;
    if (n_all > WG_YT_MAX_NODES)
        return wg_fail(WG_ERR_UNSUPPORTED, "wg_yaw_table_create: the three axes have " + std::to_string(n_all) + " nodes together, a workgroup stages at most " +
                                        std::to_string(WG_YT_MAX_NODES));
    if (wrap_wd && !(wd[n_wd - 1] - wd[0] < 360.0))
        return wg_fail(WG_ERR_INVALID, "wg_yaw_table_create: wrap_wd: wd spans " + std::to_string(wd[n_wd - 1] - wd[0]) +
                                        " degrees; an axis that wraps must span less than 360 (its first node returns as wd[0] + 360)");
    if (N < 1) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_create: N must be >= 1, got " + std::to_string(N));
    if (!yaw) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_create: yaw is null");
    const long long C = (long long)n_ti * n_ws * n_wd;
    if (C * N > 0x7fffffffLL) return wg_fail(WG_ERR_UNSUPPORTED, "wg_yaw_table_create: more than 2^31 table entries");
    if (int rc = wg_use_device(device)) return rc;
    if (on_device)
        if (int rc = wg_on_device("wg_yaw_table_create: ", device, yaw, "yaw", YT_WHOSE)) return rc;
    wg_yaw_table_s* t = new (std::nothrow) wg_yaw_table_s;
    if (!t) return wg_fail(WG_ERR_NOMEM, "wg_yaw_table_create: out of memory");
    t->mem.device = t->device = device; t->N = N; t->n_ti = n_ti; t->n_ws = n_ws; t->n_wd = n_wd; t->wrap_wd = wrap_wd != 0; t->C = C;
    const size_t yb = sizeof(double) * (size_t)C * N;
    double* ax = nullptr;
    if (int rc = t->mem.alloc("wg_yaw_table_create", &ax, (size_t)n_all + (size_t)C * N, false)) {
        wg_yaw_table_destroy(t);
        return rc;
    }
    hipError_t e = hipMemcpy(ax, ti, sizeof(double) * n_ti, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ax + n_ti, ws, sizeof(double) * n_ws, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ax + n_ti + n_ws, wd, sizeof(double) * n_wd, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ax + n_all, yaw, yb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        wg_yaw_table_destroy(t);
        return wg_hip_fail("wg_yaw_table_create", e);
    }
    t->axes = ax; t->yaw = ax + n_all;
    *out = t;
    return 0;
}

extern "C" int wg_yaw_table_destroy(wg_yaw_table t) {
    if (!t) return 0;
    t->mem.release();
    delete t;
    return 0;
}

extern "C" int wg_yaw_table_rows(wg_yaw_table t, int n, const double* wind_dev, const uint8_t* mask_dev, int32_t* rows_out, void* stream) {
    if (!t) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_rows: null table");
    if (n < 0) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_rows: n must be >= 0, got " + std::to_string(n));
    if (!wind_dev) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_rows: wind_dev is null");
    if (!rows_out) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_rows: rows_out is null");
    const WgPtrArg args[] = {{wind_dev, "wind_dev", true}, {mask_dev, "mask_dev", false}, {rows_out, "rows_out", true}};
    if (int rc = wg_on_device_all("wg_yaw_table_rows: ", "wg_yaw_table_rows: ", t->device, args, YT_WHOSE)) return rc;
    if (n == 0) return 0;
    if (int rc = wg_use_device(t->device)) return rc;
    hipLaunchKernelGGL(k_yaw_table_rows, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, yt_params(t), n, wind_dev, mask_dev, rows_out);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_yaw_table_targets(wg_yaw_table t, int n, const double* wind_dev, double* targets_out, void* stream) {
    if (!t) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_targets: null table");
    if (n < 0) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_targets: n must be >= 0, got " + std::to_string(n));
    if (!wind_dev) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_targets: wind_dev is null");
    if (!targets_out) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_targets: targets_out is null");
    const WgPtrArg args[] = {{wind_dev, "wind_dev", true}, {targets_out, "targets_out", true}};
    if (int rc = wg_on_device_all("wg_yaw_table_targets: ", "wg_yaw_table_targets: ", t->device, args, YT_WHOSE)) return rc;
    const long long total = (long long)n * t->N;
    if (total > 0x7fffffffLL) return wg_fail(WG_ERR_UNSUPPORTED, "wg_yaw_table_targets: more than 2^31 target entries");
    if (n == 0) return 0;
    if (int rc = wg_use_device(t->device)) return rc;
    hipLaunchKernelGGL(k_yaw_table_targets, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, yt_params(t), total, wind_dev,
                       targets_out);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_yaw_table_geometry_(wg_yaw_table t, int* N, int* device) {
    if (!t) return wg_fail(WG_ERR_INVALID, "null yaw table");
    *N = t->N; *device = t->device;
    return 0;
}

extern "C" void wg_launch_yaw_table_act_(wg_yaw_table t, const WgParams* p, const WgPtrs* d, float* action_out, hipStream_t st) {
    const YtActP a = {p->B, p->N, p->F, p->action_method, (double)p->yaw_min, (double)p->yaw_max, (double)p->yaw_step, d->env, d->ctx, d->yaw};
    hipLaunchKernelGGL(k_yaw_table_act, dim3((p->B * p->N + 255) / 256), dim3(256), 0, st, yt_params(t), a, action_out);
}
