// wg_norm.hip — stable-baselines3's VecNormalize on the device: the running observation statistics inside the closed loop and
// the running return statistics as a post-pass (include/windgym_hip.h restates the rules of common/vec_env/vec_normalize.py and
// common/running_mean_std.py that are pinned here).
//
// The observation half sits between a step kernel and the next launch of k_policy, so it is two small launches and nothing else:
//   k_norm_part   grid (chunks of 64 rows, tiles of 64 features), 4 waves, lane = feature (a row read is coalesced), wave y takes
//                 rows y, y + 4, ... of the chunk.  fp64 chunk moments (mean first, then the squares about it) -> scratch.
//   k_norm_apply  grid (blocks of 64 rows, tiles of 64 features).  EVERY workgroup combines the chunk moments of its 64 features
//                 in chunk order (batch mean = sum n_c mean_c / n, then M2 = sum M2_c + n_c (mean_c - mean)^2: the exact
//                 decomposition, one division instead of one per chunk), merges the batch into the running statistics (Chan) and
//                 normalises its rows of obs and of the final rows.  The workgroups of row block 0 store the new statistics into
//                 the OTHER half of a double-buffered pair: their neighbours still read the old half, the next call reads the
//                 new one (stream order).  No atomics, no waiting between workgroups: every sum has the order the shapes give it.
// The reward half never feeds the policy while it collects, so it is a post-pass over [T, B] like wg_gae: k_ret_scan (one thread
// per env walks t: the discounted returns, fp64, into scratch), k_ret_moments (one workgroup per step: the batch moments),
// k_ret_chain (one thread: T Chan merges in order, the variance after each), k_ret_apply (elementwise).
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>

#include "../../include/windgym_hip.h"
#include "wg_host.h"

namespace {

const int WGN_ROWS = 64;      // rows per chunk of k_norm_part = rows per workgroup of k_norm_apply
const int WGN_Y = 4;          // waves per workgroup; wave y takes rows y, y + 4, ...
const int WGN_PER = WGN_ROWS / WGN_Y;

struct NormHeader {
    uint32_t magic;
    int32_t O, B, reserved;
};
const uint32_t NORM_MAGIC = 0x4d524e57u;      // "WNRM"


// ((a + b) + (c + d)) of the four waves' partial sums of one feature
__device__ __forceinline__ double sum4(const double (*sh)[64], const int lane) {
    return (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

__global__ __launch_bounds__(256) void k_norm_part(const float* __restrict__ obs, const int n_rows, const int O,
                                                   double* __restrict__ pmean, double* __restrict__ pm2) {
    __shared__ double sh[WGN_Y][64];
    const int lane = threadIdx.x, y = threadIdx.y;
    const int f = blockIdx.y * 64 + lane, c = blockIdx.x;
    const int r0 = c * WGN_ROWS;
    const int nr = min(WGN_ROWS, n_rows - r0);
    const bool live = f < O;
    float x[WGN_PER];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < WGN_PER; ++i) {
        const int r = y + i * WGN_Y;
        x[i] = (live && r < nr) ? obs[(size_t)(r0 + r) * O + f] : 0.0f;
        s += (double)x[i];
    }
    sh[y][lane] = s;
    __syncthreads();
    const double mean = sum4(sh, lane) / (double)nr;
    __syncthreads();
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < WGN_PER; ++i) {
        const double d = (double)x[i] - mean;
        if (y + i * WGN_Y < nr) q += d * d;
    }
    sh[y][lane] = q;
    __syncthreads();
    if (y == 0 && live) {
        pmean[(size_t)c * O + f] = mean;
        pm2[(size_t)c * O + f] = sum4(sh, lane);
    }
}

struct NormApplyP {
    const double* sin;        // the statistics to read: mean [O], var [O], count
    double* sout;             // the other half (written when n_upd > 0)
    const double *pmean, *pm2;
    int n_upd;                // rows of the update (0: none); its chunks: (n_upd + 63) / 64
    int n_rows, O, norm;
    double clip, eps;
    const float *obs, *extra;
    float *out, *eout;
};

__global__ __launch_bounds__(256) void k_norm_apply(const NormApplyP p) {
    __shared__ double sh[WGN_Y][64];
    const int lane = threadIdx.x, y = threadIdx.y, O = p.O;
    const int f = blockIdx.y * 64 + lane;
    const bool live = f < O;
    // this thread's rows first: their loads are in flight while the statistics are merged (the kernel is a chain of memory
    // latencies, not of arithmetic: every group of loads below is issued together and waited for once)
    const int r0 = blockIdx.x * WGN_ROWS;
    float a[WGN_PER], b[WGN_PER];
#pragma unroll
    for (int i = 0; i < WGN_PER; ++i) {
        const int r = r0 + y + i * WGN_Y;
        const bool ok = live && r < p.n_rows;
        const size_t at = (size_t)r * O + f;
        a[i] = ok ? p.obs[at] : 0.0f;
        b[i] = ok && p.extra ? p.extra[at] : 0.0f;
    }
    double mean = 0.0, inv = 1.0;
    if (p.norm) {
        double var = 1.0;
        if (live) { mean = p.sin[f]; var = p.sin[O + f]; }
        if (p.n_upd > 0) {
            const double count = p.sin[2 * O];
            const int C = (p.n_upd + WGN_ROWS - 1) / WGN_ROWS;
            const double n = (double)p.n_upd;
            // the chunks c = y, y + 4, ... of this wave, eight loads at a time, summed in chunk order
            double s = 0.0;
            for (int c0 = y; c0 < C; c0 += WGN_Y * 8) {
                double m[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = c0 + j * WGN_Y;
                    m[j] = live && c < C ? p.pmean[(size_t)c * O + f] : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = c0 + j * WGN_Y;
                    if (c < C) s += (double)min(WGN_ROWS, p.n_upd - c * WGN_ROWS) * m[j];
                }
            }
            sh[y][lane] = s;
            __syncthreads();
            const double bm = sum4(sh, lane) / n;
            __syncthreads();
            double q = 0.0;
            for (int c0 = y; c0 < C; c0 += WGN_Y * 8) {
                double m[8], m2[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = c0 + j * WGN_Y;
                    const bool ok = live && c < C;
                    m[j] = ok ? p.pmean[(size_t)c * O + f] : 0.0;
                    m2[j] = ok ? p.pm2[(size_t)c * O + f] : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = c0 + j * WGN_Y;
                    const double d = m[j] - bm;
                    if (c < C) q += m2[j] + (double)min(WGN_ROWS, p.n_upd - c * WGN_ROWS) * (d * d);
                }
            }
            sh[y][lane] = q;
            __syncthreads();
            const double bv = sum4(sh, lane) / n;
            // RunningMeanStd.update_from_moments
            const double delta = bm - mean, tot = count + n;
            mean = mean + delta * n / tot;
            var = (var * count + bv * n + delta * delta * count * n / tot) / tot;
            if (blockIdx.x == 0 && y == 0 && live) {
                p.sout[f] = mean;
                p.sout[O + f] = var;
                if (f == 0) p.sout[2 * O] = tot;
            }
        }
        inv = 1.0 / sqrt(var + p.eps);
    }
#pragma unroll
    for (int i = 0; i < WGN_PER; ++i) {
        const int r = r0 + y + i * WGN_Y;
        if (!live || r >= p.n_rows) continue;
        const size_t at = (size_t)r * O + f;
        float oa = a[i], ob = b[i];
        if (p.norm) {
            double v = ((double)oa - mean) * inv;
            v = v < -p.clip ? -p.clip : (v > p.clip ? p.clip : v);
            oa = (float)v;
            double w = ((double)ob - mean) * inv;
            w = w < -p.clip ? -p.clip : (w > p.clip ? p.clip : w);
            ob = (float)w;
        }
        p.out[at] = oa;
        if (p.extra) p.eout[at] = ob;
    }
}

// steps 4 and 7 of the rule list for one env: returns = returns * gamma + r (training), then zero where the step truncated
__global__ void k_ret_scan(const int T, const int B, const int training, const double gamma, const float* __restrict__ reward,
                           const uint8_t* __restrict__ trunc, double* __restrict__ returns, double* __restrict__ scr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double R = returns[b];
    for (int t = 0; t < T; ++t) {
        const size_t at = (size_t)t * B + b;
        if (training) {
            R = R * gamma + (double)reward[at];
            scr[at] = R;
        }
        if (trunc[at]) R = 0.0;
    }
    returns[b] = R;
}

// the tree sum of 256 partial sums (fixed order)
__device__ __forceinline__ double block_sum(double* sh, const int tid, const double v) {
    sh[tid] = v;
    for (int w = 128; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w) sh[tid] += sh[tid + w];
    }
    __syncthreads();
    const double r = sh[0];
    __syncthreads();
    return r;
}

// batch moments of the returns of step t = blockIdx.x: mom[2 t] = mean, mom[2 t + 1] = sum of squares about it
__global__ __launch_bounds__(256) void k_ret_moments(const int B, const double* __restrict__ scr, double* __restrict__ mom) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const double* x = scr + (size_t)blockIdx.x * B;
    double s = 0.0;
    for (int b = tid; b < B; b += 256) s += x[b];
    const double mean = block_sum(sh, tid, s) / (double)B;
    double q = 0.0;
    for (int b = tid; b < B; b += 256) {
        const double d = x[b] - mean;
        q += d * d;
    }
    q = block_sum(sh, tid, q);
    if (tid == 0) {
        mom[2 * (size_t)blockIdx.x] = mean;
        mom[2 * (size_t)blockIdx.x + 1] = q;
    }
}

// ret_rms.update for t = 0 .. T-1 in order; var_t[t] = the variance step t's reward is divided by
__global__ void k_ret_chain(const int T, const int B, const double* __restrict__ mom, double* __restrict__ ret, double* __restrict__ var_t) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double mean = ret[0], var = ret[1], count = ret[2];
    const double n = (double)B;
    for (int t = 0; t < T; ++t) {
        const double bm = mom[2 * t], bv = mom[2 * t + 1] / n;
        const double delta = bm - mean, tot = count + n;
        mean = mean + delta * n / tot;
        var = (var * count + bv * n + delta * delta * count * n / tot) / tot;
        count = tot;
        var_t[t] = var;
    }
    ret[0] = mean; ret[1] = var; ret[2] = count;
}

__global__ void k_ret_apply(const long long n, const int B, const int norm, const double* __restrict__ var_t, const int var_stride,
                            const double clip, const double eps, const float* __restrict__ reward, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r = reward[i];
    if (norm) {
        double v = (double)r / sqrt(var_t[(size_t)(i / B) * var_stride] + eps);
        v = v < -clip ? -clip : (v > clip ? clip : v);
        r = (float)v;
    }
    out[i] = r;
}

__global__ void k_ret_zero(const int B, const uint8_t* __restrict__ mask, double* __restrict__ returns) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && mask[b]) returns[b] = 0.0;
}

}  // namespace

struct wg_norm_s {
    wg_norm_desc d;
    int device = 0, training = 1;
    int cur = 0;                 // which half of stat the next call reads (flips when a call updates: calls go to one stream at a time)
    WgDevMem mem;                // owns all: one allocation for stat[2][2 O + 1], ret[3] (mean, var, count), returns[B], pmean[C][O], pm2[C][O]
    double *stat[2] = {nullptr, nullptr}, *ret = nullptr, *returns = nullptr, *pmean = nullptr, *pm2 = nullptr;
    uint8_t* mask = nullptr;     // [B] wg_norm_reset_returns' mask on the device
    double* scr = nullptr;       // the reward pass: returns [T, B], then mom [T][2], then var_t [T]; grown by wg_norm_reward
    int scr_T = 0;
};

static size_t norm_state_doubles(const wg_norm_s* n) { return 2 * (size_t)n->d.n_obs + 1 + 3 + (size_t)n->d.n_envs; }

// the fresh statistics: mean 0, var 1, count 1e-4; returns 0
static void norm_fresh(const wg_norm_s* n, double* s) {
    const size_t O = n->d.n_obs;
    memset(s, 0, sizeof(double) * norm_state_doubles(n));
    for (size_t i = 0; i < O; ++i) s[O + i] = 1.0;
    s[2 * O] = 1e-4;
    s[2 * O + 2] = 1.0;
    s[2 * O + 3] = 1e-4;
}

// the blob's payload (obs mean / var / count, ret mean / var / count, returns) -> the device, into half 0
static int norm_upload(wg_norm n, const double* s) {
    const size_t O = n->d.n_obs, B = n->d.n_envs;
    WG_HIPCHK(hipMemcpy(n->stat[0], s, sizeof(double) * (2 * O + 1), hipMemcpyHostToDevice));
    WG_HIPCHK(hipMemcpy(n->ret, s + 2 * O + 1, sizeof(double) * (3 + B), hipMemcpyHostToDevice));      // (returns follow ret)
    n->cur = 0;
    return 0;
}

extern "C" int wg_norm_create(const wg_norm_desc* d, int device, wg_norm* out) {
    if (!d || !out) return wg_fail(WG_ERR_INVALID, "wg_norm_create: null argument");
    *out = nullptr;
    if (d->n_obs < 1 || d->n_envs < 1) return wg_fail(WG_ERR_INVALID, "wg_norm_create: n_obs and n_envs must be >= 1");
    if (!(d->clip_obs > 0.0f) || !(d->clip_reward > 0.0f)) return wg_fail(WG_ERR_INVALID, "wg_norm_create: clip_obs and clip_reward must be > 0");
    if (!(d->gamma >= 0.0 && d->gamma <= 1.0)) return wg_fail(WG_ERR_INVALID, "wg_norm_create: gamma must lie in [0, 1]");
    if (!(d->epsilon > 0.0) || !(d->epsilon < 1.0)) return wg_fail(WG_ERR_INVALID, "wg_norm_create: epsilon must lie in (0, 1)");
    wg_norm_s* n = new (std::nothrow) wg_norm_s;
    if (!n) return wg_fail(WG_ERR_NOMEM, "wg_norm_create: out of host memory");
    n->d = *d;
    n->d.norm_obs = d->norm_obs != 0; n->d.norm_reward = d->norm_reward != 0;
    n->mem.device = n->device = device;
    const size_t O = d->n_obs, B = d->n_envs, C = (B + WGN_ROWS - 1) / WGN_ROWS;
    const size_t words = 2 * (2 * O + 1) + 3 + B + 2 * C * O;
    double* m = nullptr;
    int rc = n->mem.alloc("wg_norm_create", &m, words);
    if (!rc) rc = n->mem.alloc("wg_norm_create", &n->mask, B, false);
    if (rc) {
        wg_norm_destroy(n);
        return rc;
    }
    n->stat[0] = m; m += 2 * O + 1;
    n->stat[1] = m; m += 2 * O + 1;
    n->ret = m; m += 3;
    n->returns = m; m += B;
    n->pmean = m; m += C * O;
    n->pm2 = m;
    double* s = new (std::nothrow) double[norm_state_doubles(n)];
    if (!s) { wg_norm_destroy(n); return wg_fail(WG_ERR_NOMEM, "wg_norm_create: out of host memory"); }
    norm_fresh(n, s);
    rc = norm_upload(n, s);
    delete[] s;
    if (rc) { wg_norm_destroy(n); return rc; }
    *out = n;
    return 0;
}

extern "C" int wg_norm_destroy(wg_norm n) {
    if (!n) return 0;
    n->mem.release();
    delete n;
    return 0;
}

extern "C" int wg_norm_geometry_(wg_norm n, int* n_obs, int* n_envs, int* device) {
    if (!n) return wg_fail(WG_ERR_INVALID, "null wg_norm");
    *n_obs = n->d.n_obs; *n_envs = n->d.n_envs; *device = n->device;
    return 0;
}

extern "C" int wg_norm_get_state(wg_norm n, void* host, size_t* size) {
    if (!n || !size) return wg_fail(WG_ERR_INVALID, "wg_norm_get_state: null argument");
    const size_t O = n->d.n_obs, B = n->d.n_envs;
    const size_t total = sizeof(NormHeader) + sizeof(double) * norm_state_doubles(n);
    if (int rc = wg_blob_get("wg_norm_get_state: ", n->device, host, size, total)) return rc;
    if (!host) return 0;
    const NormHeader hd = {NORM_MAGIC, n->d.n_obs, n->d.n_envs, 0};
    memcpy(host, &hd, sizeof(hd));
    char* at = (char*)host + sizeof(hd);
    WG_HIPCHK(hipMemcpy(at, n->stat[n->cur], sizeof(double) * (2 * O + 1), hipMemcpyDeviceToHost));
    WG_HIPCHK(hipMemcpy(at + sizeof(double) * (2 * O + 1), n->ret, sizeof(double) * (3 + B), hipMemcpyDeviceToHost));
    *size = total;
    return 0;
}

extern "C" int wg_norm_set_state(wg_norm n, const void* host, size_t size) {
    if (!n || !host) return wg_fail(WG_ERR_INVALID, "wg_norm_set_state: null argument");
    const auto geometry = [&](const NormHeader& got) {
        if (got.O == n->d.n_obs && got.B == n->d.n_envs && size == sizeof(NormHeader) + sizeof(double) * norm_state_doubles(n)) return 0;
        return wg_fail(WG_ERR_INVALID, "wg_norm_set_state: the blob holds statistics of " + std::to_string(got.O) + " observation entries x " +
                                        std::to_string(got.B) + " envs, this wg_norm has " + std::to_string(n->d.n_obs) + " x " +
                                        std::to_string(n->d.n_envs));
    };
    if (int rc = wg_blob_set<NormHeader>("wg_norm_set_state: ", n->device, host, size, NORM_MAGIC, "not a wg_norm state blob", geometry)) return rc;
    // (the payload is copied out first: a blob inside a Python bytes object need not be aligned for doubles)
    const size_t nd = norm_state_doubles(n);
    double* s = new (std::nothrow) double[nd];
    if (!s) return wg_fail(WG_ERR_NOMEM, "wg_norm_set_state: out of host memory");
    memcpy(s, (const char*)host + sizeof(NormHeader), sizeof(double) * nd);
    const int rc = norm_upload(n, s);
    delete[] s;
    return rc;
}

extern "C" int wg_norm_set_training(wg_norm n, int training) {
    if (!n) return wg_fail(WG_ERR_INVALID, "wg_norm_set_training: null wg_norm");
    n->training = training != 0;
    return 0;
}

extern "C" int wg_norm_reset_returns(wg_norm n, const uint8_t* env_mask_host, void* stream) {
    if (!n) return wg_fail(WG_ERR_INVALID, "wg_norm_reset_returns: null wg_norm");
    if (int rc = wg_use_device(n->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int B = n->d.n_envs;
    if (!env_mask_host) {
        WG_HIPCHK(hipMemsetAsync(n->returns, 0, sizeof(double) * (size_t)B, st));
        return 0;
    }
    WG_HIPCHK(hipMemcpyAsync(n->mask, env_mask_host, (size_t)B, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ret_zero, dim3((B + 255) / 256), dim3(256), 0, st, B, n->mask, n->returns);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_norm_obs(wg_norm n, int n_rows, const float* obs_dev, float* out_dev, const float* extra_dev, float* extra_out_dev,
                           void* stream) {
    if (!n || !obs_dev || !out_dev) return wg_fail(WG_ERR_INVALID, "wg_norm_obs: null argument (obs_dev and out_dev are required)");
    if ((extra_dev == nullptr) != (extra_out_dev == nullptr))
        return wg_fail(WG_ERR_INVALID, "wg_norm_obs: extra_dev and extra_out_dev go together");
    if (n_rows < 0) return wg_fail(WG_ERR_INVALID, "wg_norm_obs: n_rows < 0");
    const bool update = n->training && n->d.norm_obs;
    if (update && n_rows > n->d.n_envs)
        return wg_fail(WG_ERR_INVALID, "wg_norm_obs: an update takes at most n_envs = " + std::to_string(n->d.n_envs) + " rows, got " +
                                        std::to_string(n_rows));
    if (n_rows == 0) return 0;
    if (int rc = wg_use_device(n->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int O = n->d.n_obs;
    const dim3 block(64, WGN_Y), grid((n_rows + WGN_ROWS - 1) / WGN_ROWS, (O + 63) / 64);
    if (update) hipLaunchKernelGGL(k_norm_part, grid, block, 0, st, obs_dev, n_rows, O, n->pmean, n->pm2);
    NormApplyP p;
    p.sin = n->stat[n->cur]; p.sout = n->stat[n->cur ^ 1];
    p.pmean = n->pmean; p.pm2 = n->pm2;
    p.n_upd = update ? n_rows : 0;
    p.n_rows = n_rows; p.O = O; p.norm = n->d.norm_obs;
    p.clip = (double)n->d.clip_obs; p.eps = n->d.epsilon;
    p.obs = obs_dev; p.extra = extra_dev; p.out = out_dev; p.eout = extra_out_dev;
    hipLaunchKernelGGL(k_norm_apply, grid, block, 0, st, p);
    WG_HIPCHK(hipGetLastError());
    if (update) n->cur ^= 1;
    return 0;
}

extern "C" int wg_norm_reward(wg_norm n, int T, const float* reward_dev, const uint8_t* truncated_dev, float* out_dev, void* stream) {
    if (!n || !reward_dev || !truncated_dev || !out_dev)
        return wg_fail(WG_ERR_INVALID, "wg_norm_reward: null argument (reward_dev, truncated_dev and out_dev are required)");
    if (T < 0) return wg_fail(WG_ERR_INVALID, "wg_norm_reward: T < 0");
    if (T == 0) return 0;
    if (int rc = wg_use_device(n->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int B = n->d.n_envs;
    if (n->training && T > n->scr_T) {          // grown here, before anything is enqueued (hipFree waits for what still reads the old one)
        double* const old = n->scr;
        n->scr = nullptr; n->scr_T = 0;
        if (int rc = n->mem.free("wg_norm_reward", old)) return rc;
        if (int rc = n->mem.alloc("wg_norm_reward", &n->scr, (size_t)T * B + 3 * (size_t)T, false)) return rc;
        n->scr_T = T;
    }
    double* const mom = n->scr ? n->scr + (size_t)n->scr_T * B : nullptr;
    double* const var_t = n->scr ? mom + 2 * (size_t)n->scr_T : nullptr;
    hipLaunchKernelGGL(k_ret_scan, dim3((B + 63) / 64), dim3(64), 0, st, T, B, n->training, n->d.gamma, reward_dev, truncated_dev,
                       n->returns, n->scr);
    if (n->training) {
        hipLaunchKernelGGL(k_ret_moments, dim3(T), dim3(256), 0, st, B, n->scr, mom);
        hipLaunchKernelGGL(k_ret_chain, dim3(1), dim3(64), 0, st, T, B, mom, n->ret, var_t);
    }
    const long long total = (long long)T * B;
    hipLaunchKernelGGL(k_ret_apply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, B, n->d.norm_reward,
                       n->training ? var_t : n->ret + 1, n->training ? 1 : 0, (double)n->d.clip_reward, n->d.epsilon, reward_dev, out_dev);
    WG_HIPCHK(hipGetLastError());
    return 0;
}
