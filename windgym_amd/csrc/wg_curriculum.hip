// wg_curriculum.hip — yaw-curriculum reward shaping on the device: the reference's CurriculumWrapper.step and the weight its
// CurriculumCallback sets (examples/curriculum.py:335-429) as a post-pass over a rollout's buffers (include/windgym_hip.h states
// the recurrence).  The policy never reads the reward while wg_rollout collects, so the shaped reward is computed afterwards,
// exactly as wg_gae computes advantages afterwards: no step kernel, no policy kernel and no part of the closed loop knows of it.
//
// k_curriculum: ONE thread per env walks the env's T steps in order (the recurrence is serial in t: the smoothing, the running
// sums of the change history), the turbines in index order inside a step — every sum has one order, fixed by the shapes alone,
// and shaping T steps in one launch or in several gives the same bits.  Per-turbine state (the previous yaws, the previous
// change signs, the running targets) lives in global memory, [B][N]: N is whatever the handle has (Horns Rev: 80), nothing is
// sized by it at compile time.  A step reads 2 N floats of the rollout and reads / writes 2 N state words, all of which stay
// in the cache between steps; the launch is latency bound and small next to anything else an iteration does.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>

#include "../../include/windgym_hip.h"
#include "wg_host.h"
#include "wg_rules.h"
#include "wg_yaw_table.h"

namespace {

struct CurP {
    int B, N, T, C, action_method;
    float yaw_min, yaw_max, yaw_step;
    double yaw_max_d, momentum;
};

// the per-env state, carved out of one allocation in this order (= the payload of the state blob)
struct CurState {
    double* yprev;      // [B][N] the yaws of the last shaped step (previous_yaws)
    double* g;          // [B][N] the running targets (pywake_yaws)
    double* cum;        // [B]    sum of every change so far (np.sum(yaw_change_history))
    double* last;       // [B]    last_reward
    long long* n;       // [B]    steps shaped so far; the change history holds max(n - 1, 0) entries
    long long* osc;     // [B]    sum of |diff(sign(history))| so far
    int32_t* sprev;     // [B][N] sign of the last change (0 / 1: a change is an absolute value)
};

struct CurHeader {
    uint32_t magic;
    int32_t B, N, reserved;
};
const uint32_t CUR_MAGIC = 0x52554357u;      // "WCUR"

__global__ __launch_bounds__(64) void k_curriculum(const CurP p, const CurState s, int* __restrict__ err, const float* __restrict__ yaw0,
                                                   const float* __restrict__ actions, const float* __restrict__ yaw_after,
                                                   const uint8_t* __restrict__ truncated, const int32_t* __restrict__ ep_row,
                                                   const double* __restrict__ ep_target, const double* __restrict__ weight,
                                                   const float* reward, float* shaped, float* __restrict__ yaw_diff,
                                                   float* __restrict__ yaw_out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    const int N = p.N;
    const size_t sb = (size_t)b * N;
    double* const yprev = s.yprev + sb;
    double* const g = s.g + sb;
    int32_t* const sprev = s.sprev + sb;
    long long n = s.n[b], osc = s.osc[b];
    double cum = s.cum[b], last = s.last[b];
    const double dN = (double)N;
    for (int t = 0; t < p.T; ++t) {
        const size_t row = (size_t)t * p.B + b;
        const float* const prev = t == 0 ? yaw0 + sb : yaw_after + (row - p.B) * N;
        const float* const act = actions + row * N;
        double d = 0.0, csum = 0.0;
        long long dosc = 0;
        for (int i = 0; i < N; ++i) {
            const float yf = wg_rule_adjust_yaw(p.action_method, prev[i], act[i], p.yaw_min, p.yaw_max, p.yaw_step);      // the step kernels' rule
            if (yaw_out) yaw_out[row * N + i] = yf;
            const double y = (double)yf;
            d += fabs(y - g[i]);
            if (n >= 1) {
                const double c = fabs(y - yprev[i]);
                csum += c;
                const int32_t sg = c > 0.0 ? 1 : 0;
                if (n >= 2) dosc += sg > sprev[i] ? sg - sprev[i] : sprev[i] - sg;
                sprev[i] = sg;
            }
            yprev[i] = y;
        }
        d = d / dN;
        const double sim = 1.0 / (1.0 + d);
        double pen = 0.0;
        if (n >= 1) {
            pen += 0.3 * (csum / dN / p.yaw_max_d);
            cum += csum;
            if (n >= 2) {
                osc += dosc;
                pen += (double)osc / ((double)(n - 1) * dN) * 0.2;
            }
            if (n >= 5) pen += cum / dN / p.yaw_max_d * 0.1;
        }
        n += 1;
        const double w = weight[t];
        const double cur = (1.0 - w) * (sim - pen / 600.0) + w * (double)reward[row];
        last = p.momentum * last + (1.0 - p.momentum) * cur;
        shaped[row] = (float)last;
        if (yaw_diff) yaw_diff[row] = (float)d;
        // CurriculumWrapper.reset: the episode that begins after this step brings its own target
        if (truncated[row]) {
            const int r = ep_row[row];
            if (r >= p.C) {
                if (atomicCAS(&err[0], 0, 1) == 0) { err[1] = t; err[2] = b; err[3] = r; }      // the first offender is the one reported
            } else if (r >= 0) {
                const double* const src = ep_target + (size_t)r * N;
                for (int i = 0; i < N; ++i) g[i] = src[i];
            }
        }
    }
    s.n[b] = n; s.osc[b] = osc; s.cum[b] = cum; s.last[b] = last;
}

// The expert's action for every step of a rollout (wg_expert_labels): the action that cur_adjust_yaw turns into the largest move
// from the yaw the step's observation belongs to towards the env's running target — the inverse of the actuation rule, in double,
// rounded once.  One thread per env walks t as k_curriculum does, with its order of target switches; `g` is the caller's table.
__global__ __launch_bounds__(64) void k_expert_labels(const CurP p, double* __restrict__ targets, int* __restrict__ err,
                                                      const float* __restrict__ yaw0, const float* __restrict__ yaw_after,
                                                      const uint8_t* __restrict__ truncated, const int32_t* __restrict__ ep_row,
                                                      const double* __restrict__ ep_target, float* __restrict__ labels,
                                                      float* __restrict__ yaw_diff) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    const int N = p.N;
    const size_t sb = (size_t)b * N;
    double* const g = targets + sb;
    const double dN = (double)N, lo = (double)p.yaw_min, hi = (double)p.yaw_max, step = (double)p.yaw_step;
    for (int t = 0; t < p.T; ++t) {
        const size_t row = (size_t)t * p.B + b;
        const float* const prev = t == 0 ? yaw0 + sb : yaw_after + (row - p.B) * N;
        double d = 0.0;
        for (int i = 0; i < N; ++i) {
            const double y = (double)prev[i], gi = g[i];
            labels[row * N + i] = (float)wg_expert_action(p.action_method, gi, y, lo, hi, step);
            d += fabs(y - gi);
        }
        if (yaw_diff) yaw_diff[row] = (float)(d / dN);
        if (truncated[row]) {
            const int r = ep_row[row];
            if (r >= p.C) {
                if (err && atomicCAS(&err[0], 0, 1) == 0) { err[1] = t; err[2] = b; err[3] = r; }
            } else if (r >= 0) {
                const double* const src = ep_target + (size_t)r * N;
                for (int i = 0; i < N; ++i) g[i] = src[i];
            }
        }
    }
}


}  // namespace

struct wg_curriculum_s {
    WgActuation a;
    WgDevMem mem;               // owns state and err
    char* state = nullptr;      // the state: one allocation, CurState points into it
    size_t bytes = 0;
    CurState s;
    int* err = nullptr;         // device: {latched, t, b, row} of an ep_row entry >= C
};

// the kernels' parameter block for T steps on the batch of `a`
static CurP cur_params(const WgActuation& a, int T, int C, double momentum) {
    CurP p;
    p.B = a.B; p.N = a.N; p.T = T; p.C = C; p.action_method = a.action_method;
    p.yaw_min = a.yaw_min; p.yaw_max = a.yaw_max; p.yaw_step = a.yaw_step;
    p.yaw_max_d = a.yaw_max_d; p.momentum = momentum;
    return p;
}

// the latch of a bad ep_row entry, read on the current, idle device: cleared and reported as `who` when it is set
static int cur_latch_report(const char* who, int* err_dev) {
    int err[4];
    WG_HIPCHK(hipMemcpy(err, err_dev, sizeof(err), hipMemcpyDeviceToHost));
    if (!err[0]) return 0;
    WG_HIPCHK(hipMemset(err_dev, 0, sizeof(err)));
    return wg_fail(WG_ERR_INVALID, std::string(who) + ": ep_row_dev[" + std::to_string(err[1]) + ", " + std::to_string(err[2]) + "] = " +
                                    std::to_string(err[3]) + " is not a row of ep_target_dev (C rows); the entry was skipped");
}

extern "C" int wg_curriculum_create(wg_handle h, wg_curriculum* out) {
    if (!h || !out) return wg_fail(WG_ERR_INVALID, "wg_curriculum_create: null argument");
    wg_curriculum_s* c = new (std::nothrow) wg_curriculum_s;
    if (!c) return wg_fail(WG_ERR_NOMEM, "wg_curriculum_create: out of memory");
    if (int rc = wg_handle_actuation_(h, &c->a)) { delete c; return rc; }
    const size_t B = (size_t)c->a.B, BN = B * (size_t)c->a.N;
    c->bytes = 8 * (2 * BN + 4 * B) + 4 * BN;
    c->mem.device = c->a.device;
    int rc = c->mem.alloc("wg_curriculum_create", &c->state, c->bytes);
    if (!rc) rc = c->mem.alloc("wg_curriculum_create", &c->err, 4);
    if (rc) {
        wg_curriculum_destroy(c);
        return rc;
    }
    char* m = c->state;
    c->s.yprev = (double*)m; m += 8 * BN;
    c->s.g = (double*)m; m += 8 * BN;
    c->s.cum = (double*)m; m += 8 * B;
    c->s.last = (double*)m; m += 8 * B;
    c->s.n = (long long*)m; m += 8 * B;
    c->s.osc = (long long*)m; m += 8 * B;
    c->s.sprev = (int32_t*)m;
    *out = c;
    return 0;
}

extern "C" int wg_curriculum_destroy(wg_curriculum c) {
    if (!c) return 0;
    c->mem.release();
    delete c;
    return 0;
}

static CurHeader cur_header(wg_curriculum c) {
    CurHeader hd;
    hd.magic = CUR_MAGIC; hd.B = c->a.B; hd.N = c->a.N; hd.reserved = 0;
    return hd;
}

extern "C" int wg_curriculum_get_state(wg_curriculum c, void* host, size_t* size) {
    if (!c || !size) return wg_fail(WG_ERR_INVALID, "wg_curriculum_get_state: null argument");
    const size_t total = sizeof(CurHeader) + c->bytes;
    if (int rc = wg_blob_get("wg_curriculum_get_state: ", c->a.device, host, size, total)) return rc;
    if (!host) return 0;
    if (int rc = cur_latch_report("wg_curriculum_shape", c->err)) return rc;
    const CurHeader hd = cur_header(c);
    memcpy(host, &hd, sizeof(hd));
    WG_HIPCHK(hipMemcpy((char*)host + sizeof(hd), c->state, c->bytes, hipMemcpyDeviceToHost));
    *size = total;
    return 0;
}

extern "C" int wg_curriculum_set_state(wg_curriculum c, const void* host, size_t size) {
    if (!c || !host) return wg_fail(WG_ERR_INVALID, "wg_curriculum_set_state: null argument");
    const CurHeader want = cur_header(c);
    const auto geometry = [&](const CurHeader& got) {
        if (!memcmp(&got, &want, sizeof(got)) && size == sizeof(CurHeader) + c->bytes) return 0;
        return wg_fail(WG_ERR_INVALID, "wg_curriculum_set_state: the blob was taken from a curriculum of " + std::to_string(got.B) + " envs x " +
                                        std::to_string(got.N) + " turbines, this one has " + std::to_string(want.B) + " x " + std::to_string(want.N));
    };
    if (int rc = wg_blob_set<CurHeader>("wg_curriculum_set_state: ", c->a.device, host, size, CUR_MAGIC, "not a curriculum state blob", geometry))
        return rc;
    WG_HIPCHK(hipMemcpy(c->state, (const char*)host + sizeof(CurHeader), c->bytes, hipMemcpyHostToDevice));
    return 0;
}

// a buffer the kernel will touch must be device memory of the curriculum's device (the device of the handle it was created on)
static const char* const CUR_WHOSE = ", the device of the handle the curriculum was created on";

extern "C" int wg_curriculum_set_targets(wg_curriculum c, const double* yaw_dev, void* stream) {
    if (!c) return wg_fail(WG_ERR_INVALID, "wg_curriculum_set_targets: null curriculum");
    if (int rc = wg_on_device_all("wg_curriculum_set_targets: ", "wg_curriculum: ", c->a.device, {{yaw_dev, "yaw_dev", true}}, CUR_WHOSE)) return rc;
    if (int rc = wg_use_device(c->a.device)) return rc;
    WG_HIPCHK(hipMemcpyAsync(c->s.g, yaw_dev, sizeof(double) * (size_t)c->a.B * c->a.N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int wg_curriculum_shape(wg_curriculum c, int T, const float* yaw0_dev, const float* actions_dev, const float* yaw_after_dev,
                                   const uint8_t* truncated_dev, const int32_t* ep_row_dev, const double* ep_target_dev, int C,
                                   const double* weight_dev, double momentum, const float* reward_dev, float* shaped_out,
                                   float* yaw_diff_out, float* yaw_out, void* stream) {
    if (!c) return wg_fail(WG_ERR_INVALID, "wg_curriculum_shape: null curriculum");
    if (T < 0) return wg_fail(WG_ERR_INVALID, "wg_curriculum_shape: T must be >= 0, got " + std::to_string(T));
    if (C < 0) return wg_fail(WG_ERR_INVALID, "wg_curriculum_shape: C must be >= 0, got " + std::to_string(C));
    if (!(momentum >= 0.0 && momentum < 1.0))
        return wg_fail(WG_ERR_INVALID, "wg_curriculum_shape: momentum must lie in [0, 1), got " + std::to_string(momentum));
    const WgPtrArg args[] = {
        {yaw0_dev, "yaw0_dev", true}, {actions_dev, "actions_dev", true}, {yaw_after_dev, "yaw_after_dev", true},
        {truncated_dev, "truncated_dev", true}, {ep_row_dev, "ep_row_dev", true}, {ep_target_dev, "ep_target_dev", C > 0},
        {weight_dev, "weight_dev", true}, {reward_dev, "reward_dev", true}, {shaped_out, "shaped_out", true},
        {yaw_diff_out, "yaw_diff_out", false}, {yaw_out, "yaw_out", false}};
    if (int rc = wg_on_device_all("wg_curriculum_shape: ", "wg_curriculum: ", c->a.device, args, CUR_WHOSE)) return rc;
    if (T == 0) return 0;
    if (int rc = wg_use_device(c->a.device)) return rc;
    const CurP p = cur_params(c->a, T, C, momentum);
    hipLaunchKernelGGL(k_curriculum, dim3((p.B + 63) / 64), dim3(64), 0, (hipStream_t)stream, p, c->s, c->err, yaw0_dev, actions_dev,
                       yaw_after_dev, truncated_dev, ep_row_dev, ep_target_dev, weight_dev, reward_dev, shaped_out, yaw_diff_out, yaw_out);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// expert labels (windgym_hip.h: wg_expert_labels) — no handle of its own: the actuation rule is read from `h`, the running
// targets and the latch of a bad ep_row entry are the caller's
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int wg_expert_labels(wg_handle h, int T, const float* yaw0_dev, const float* yaw_after_dev, const uint8_t* truncated_dev,
                                const int32_t* ep_row_dev, const double* ep_target_dev, int C, double* targets_dev, float* labels_out,
                                float* yaw_diff_out, int32_t* err_dev, void* stream) {
    WgActuation a;
    if (!h) return wg_fail(WG_ERR_INVALID, "wg_expert_labels: null handle");
    if (int rc = wg_handle_actuation_(h, &a)) return rc;
    if (T < 0) return wg_fail(WG_ERR_INVALID, "wg_expert_labels: T must be >= 0, got " + std::to_string(T));
    if (C < 0) return wg_fail(WG_ERR_INVALID, "wg_expert_labels: C must be >= 0, got " + std::to_string(C));
    const WgPtrArg args[] = {
        {yaw0_dev, "yaw0_dev", true}, {yaw_after_dev, "yaw_after_dev", true}, {truncated_dev, "truncated_dev", true},
        {ep_row_dev, "ep_row_dev", true}, {ep_target_dev, "ep_target_dev", C > 0}, {targets_dev, "targets_dev", true},
        {labels_out, "labels_out", true}, {yaw_diff_out, "yaw_diff_out", false}, {err_dev, "err_dev", false}};
    if (int rc = wg_on_device_all("wg_expert_labels: ", "wg_expert_labels: ", a.device, args, ", the handle's device")) return rc;
    if (T == 0) return 0;
    if (int rc = wg_use_device(a.device)) return rc;
    const CurP p = cur_params(a, T, C, 0.0);
    hipLaunchKernelGGL(k_expert_labels, dim3((p.B + 63) / 64), dim3(64), 0, (hipStream_t)stream, p, targets_dev, (int*)err_dev, yaw0_dev,
                       yaw_after_dev, truncated_dev, ep_row_dev, ep_target_dev, labels_out, yaw_diff_out);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_expert_labels_check(wg_handle h, int32_t* err_dev) {
    WgActuation a;
    if (!h || !err_dev) return wg_fail(WG_ERR_INVALID, "wg_expert_labels_check: null argument");
    if (int rc = wg_handle_actuation_(h, &a)) return rc;
    if (int rc = wg_on_device("wg_expert_labels: ", a.device, err_dev, "err_dev", ", the handle's device")) return rc;
    if (int rc = wg_use_device(a.device)) return rc;
    WG_HIPCHK(hipDeviceSynchronize());
    return cur_latch_report("wg_expert_labels", (int*)err_dev);
}
