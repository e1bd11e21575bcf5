// wg_steady.hip — k_steady: steady-state farm power for a batch of (wind condition, yaw vector) cases on the MI355X.
//
// The inner loop of the reference's PyWakeAgent (WindGym/Agents/PyWakeAgent.py:144-288, yaw_optimizer_srf_vect: every
// refine step evaluates the farm power of yaw_n candidate yaw vectors per wind condition) — SURVEY.md §8 row f4.  The
// Serial-Refine loop of windgym_amd/steady.py runs on the host, each of its steps ONE launch of this kernel over
// [conditions x candidates] cases; k_steady_srf (below) is the whole loop on the device, on the same farm evaluation.
//   model 0: the steady state of the env's own flow model M0 — the deficit evaluation of k_flow /
//            k_windspeed with the chain replaced by its fixed point: every source's frozen record is the record it emits
//            now, the wake centre is the integral of the Hill-vortex deflection speed along the chain;
//   model 1: the reference agent's py_wake model restated from the publications — Blondel & Cathelain (2020)
//            super-Gaussian deficit at the rotor centre + Jimenez deflection (steady.blondel_jimenez_power).
// One single-wave workgroup per case: turbines are visited upstream -> downstream (rank by flow-frame x); lane s evaluates
// source s for the current target (its S rotor points, its deflection quadrature), wave reductions give the target's
// inflow.  fp32; the fp64 torch restatement of windgym_amd/steady.py is the oracle (tests/test_steady_kernel.py).
#include <hip/hip_runtime.h>

#include "wg_device.h"
#include "wg_steady.h"
#include "wg_internal.h"

__device__ __forceinline__ float st_interp(const float* __restrict__ xs, const float* __restrict__ ys, const int n, const float x) {
    if (!(x >= xs[0]) || x > xs[n - 1]) return 0.f;        // 0 outside the table (steady._interp)
    int i = 0;
    while (i < n - 2 && xs[i + 1] <= x) ++i;
    const float f = (x - xs[i]) / (xs[i + 1] - xs[i]);
    return ys[i] + f * (ys[i + 1] - ys[i]);
}
__device__ __forceinline__ float st_cfrac(const float ct, const float sp) {
    const float m = fminf(1.0f / (8.0f * sp * sp), 1.0f);
    return 1.0f - sqrtf(fmaxf(1.0f - ct * m, 0.0f));
}

// ---- the farm evaluation, shared by k_steady and k_steady_srf (both inline it: same lanes, same order, same bits) ----
// flow-frame layout of the farm for wind direction wd: turbines first, first + stride, ...
__device__ __forceinline__ void st_frame(const SteadyP& p, const float wd, const int first, const int stride,
                                         float* __restrict__ xr, float* __restrict__ yr) {
    const double th = (270.0 - (double)wd) * (WG_PI_D / 180.0);
    const double cth = cos(th), sth = sin(th);
    for (int t = first; t < p.N; t += stride) {
        const double dx = p.x_pos[t] - p.cx0, dy = p.y_pos[t] - p.cy0;
        xr[t] = (float)(p.cx0 + dx * cth + dy * sth - p.cx0);      // (relative to the farm centre: fp32 keeps the metres)
        yr[t] = (float)(p.cy0 - dx * sth + dy * cth - p.cy0);
    }
}
__device__ __forceinline__ void st_set_yaw(const float yaw_deg, float& cg, float& sg) {
    const float g = yaw_deg * WG_DEG2RAD_F;
    cg = cosf(g); sg = sinf(g);
}
// upstream -> downstream: rank of turbine t = number of turbines ahead of it (ties by index, like a stable argsort)
__device__ __forceinline__ void st_rank(const int N, const int first, const int stride, const float* __restrict__ xr, int* __restrict__ by_rank) {
    for (int t = first; t < N; t += stride) {
        int r = 0;
        for (int o = 0; o < N; ++o) r += (xr[o] < xr[t] || (xr[o] == xr[t] && o < t)) ? 1 : 0;
        by_rank[r] = t;
    }
}
// one turbine t of the upstream -> downstream visit, by one wave: lane s evaluates source s (s += 64), lane 0 writes t's state.
// Only sources strictly upstream of t are read, so the state of t and of everything behind it may hold anything.
__device__ __forceinline__ void st_visit(const SteadyP& p, const float ws, const float ti, const int t, const int lane,
                                         const float* __restrict__ xr, const float* __restrict__ yr, const float* cg, const float* sg,
                                         float* u, float* til, float* ct, float* hv) {
    const int N = p.N;
    const float inv_D = 1.0f / p.D;
    {
        const float xt = xr[t], yt = yr[t], cgt = cg[t];
        float dsum = 0.f, tia_max = 0.f;
        for (int s = lane; s < N; s += 64) {
            const float dx = xt - xr[s];
            if (!(dx > 1e-9f)) continue;
            const float cts = ct[s];
            if (p.model == 0) {
                const float k = p.ka * til[s] + p.kb;
                const float q = sqrtf(1.0f - cts);
                const float eps = p.eps0 * sqrtf(0.5f * (1.0f + q) / q);
                const float xd = dx * inv_D;
                const float sp = k * xd + eps, sig = sp * p.D;
                // wake-centre deflection: (hv / U) * integral_0^dx C(x') dx' (trapezoid, n_quad points)
                const int Q = p.n_quad;
                const float h = dx / (float)(Q - 1);
                float integ = 0.f;
                for (int i = 0; i < Q; ++i) {
                    const float cq = st_cfrac(cts, k * ((float)i * h * inv_D) + eps);
                    integ += (i == 0 || i == Q - 1) ? 0.5f * cq : cq;
                }
                integ *= h;
                const float yc = yr[s] + hv[s] / ws * integ;
                const float rc2 = (yt - yc) * (yt - yc);
                const float rcut = p.R + 5.0f * sig;
                if (rc2 > rcut * rcut) continue;
                const float amp = u[s] * st_cfrac(cts, sp);
                const float inv2s2 = 1.0f / (2.0f * sig * sig);
                float acc = 0.f;
                for (int i = 0; i < p.S; ++i) {
                    const float dy = yt + p.rotor_dy[i] * cgt - yc, dz = p.rotor_dz[i];
                    acc += amp * expf(-(dy * dy + dz * dz) * inv2s2);
                }
                dsum += acc;
                const float ind = 0.5f * (1.0f - sqrtf(1.0f - cts));
                tia_max = fmaxf(tia_max, p.tia * powf(ind, p.tib) * powf(ti, p.tic) * powf(fmaxf(xd, 1.0f), p.tid) * expf(-rc2 * inv2s2));
            } else {
                // Blondel & Cathelain (2020) at the rotor centre, Jimenez deflection (py_wake defaults: steady.py)
                const float xd = fmaxf(dx, 1e-9f) * inv_D;
                const float q = sqrtf(1.0f - fminf(cts, 0.999f));
                const float beta = 0.5f * (1.0f + q) / q;
                const float sigma = (0.17f * ti + 0.005f) * xd + 0.2f * sqrtf(beta);
                const float n = 3.11f * expf(-0.68f * xd) + 2.41f;
                const float in2 = 2.0f / n;
                const float C = exp2f(in2 - 1.0f) - sqrtf(fmaxf(exp2f(2.0f * in2 - 2.0f) - n * cts / (16.0f * tgammaf(in2) * powf(sigma, 2.0f * in2)), 0.0f));
                const int Q = p.n_quad;
                const float a0 = cg[s] * cg[s] * sg[s] * cts * 0.5f;
                float defl = 0.f, x_prev = 0.f, f_prev = sinf(a0);
                for (int i = 1; i < Q; ++i) {      // points clustered towards the rotor: (10^(1.1 i / (Q - 1)) - 1) / (10^1.1 - 1)
                    const float s01 = (exp10f(1.1f * (float)i / (float)(Q - 1)) - 1.0f) * (1.0f / (12.589254117941675f - 1.0f));
                    const float xq = dx * s01;
                    const float den = 1.0f + 0.1f * xq * inv_D;
                    const float f = sinf(a0 / (den * den));
                    defl += 0.5f * (f + f_prev) * (xq - x_prev);
                    x_prev = xq; f_prev = f;
                }
                const float r = fabsf(yt - (yr[s] - defl)) * inv_D;
                dsum += ws * C * expf(-powf(r, n) / (2.0f * sigma * sigma));
            }
        }
        dsum = wg_wave_sum(dsum);
        tia_max = wg_wave_max(tia_max);
        if (lane == 0) {
            if (p.model == 0) {
                const float ut = ws - dsum / (float)p.S;
                u[t] = ut;
                til[t] = sqrtf(ti * ti + tia_max * tia_max);
                ct[t] = fminf(fmaxf(st_interp(p.tab_ws, p.tab_ct, p.n_tab, fmaxf(ut * cgt, 0.f)) * cgt * cgt, 0.f), 0.96f);
                hv[t] = -p.hill * sg[t] * ut;
            } else {
                const float ut = ws - dsum;
                u[t] = ut;
                ct[t] = fminf(fmaxf(st_interp(p.tab_ws, p.tab_ct, p.n_tab, fmaxf(ut * cgt, 0.f)) * cgt * cgt, 0.f), 0.999f);
            }
        }
    }
}
__device__ __forceinline__ float st_power(const SteadyP& p, const float u, const float cg) {
    return st_interp(p.tab_ws, p.tab_power, p.n_tab, fmaxf(u * cg, 0.f));
}

__global__ void __launch_bounds__(64)
k_steady(const SteadyP p, const float* __restrict__ ws_in, const float* __restrict__ wd_in, const float* __restrict__ ti_in,
         const float* __restrict__ yaw_in, float* __restrict__ power_out) {
    extern __shared__ float st_lds[];
    const int c = blockIdx.x, lane = threadIdx.x, N = p.N;
    if (c >= p.n_cases) return;
    float* xr = st_lds;            // [N] each
    float* yr = xr + N;
    float* cg = yr + N;
    float* sg = cg + N;
    float* u = sg + N;
    float* til = u + N;
    float* ct = til + N;
    float* hv = ct + N;
    int* by_rank = reinterpret_cast<int*>(hv + N);
    const float ws = ws_in[c], ti = ti_in[c];
    st_frame(p, wd_in[c], lane, 64, xr, yr);
    for (int t = lane; t < N; t += 64) {
        st_set_yaw(yaw_in[(size_t)c * N + t], cg[t], sg[t]);
        u[t] = ws; til[t] = ti; ct[t] = 0.f; hv[t] = 0.f;
    }
    __syncthreads();
    st_rank(N, lane, 64, xr, by_rank);
    __syncthreads();
    for (int pos = 0; pos < N; ++pos) {
        st_visit(p, ws, ti, by_rank[pos], lane, xr, yr, cg, sg, u, til, ct, hv);
        __syncthreads();
    }
    for (int t = lane; t < N; t += 64) power_out[(size_t)c * N + t] = st_power(p, u[t], cg[t]);
}

// k_steady_srf: the whole Serial-Refine optimisation (PyWakeAgent.py:144-288) of ONE wind condition in one workgroup, all
// conditions in one launch.  yaw_n waves; wave j evaluates candidate j of the current refine step (turbine t = by_rank[pos]
// moved by offsets[pass][j]) on a state of its own.  A turbine's state depends on the turbines upstream of it only, so a
// candidate recomputes ranks pos .. N-1 and keeps ranks < pos, which every wave holds equal to the committed state.  After the
// step: first-index argmax of the candidates' farm powers (fp64, summed in index order), a strictly better winner is committed
// (yaw, power, its state of ranks >= pos), and every wave takes the committed state of t back.
// LDS: f64 yaw[N] | f64 cand_power[16] | xr[N] yr[N] | i32 by_rank[N] | committed cg sg u til ct hv [N] each |
//      per wave: cg sg u til ct hv pw [N] each                            (44 N + 128 + 28 N yaw_n bytes; 63 104 at the limits)
#define WG_SRF_WAVE_ARRAYS 7
__global__ void __launch_bounds__(1024)
k_steady_srf(const SteadyP p, const float* __restrict__ ws_in, const float* __restrict__ wd_in, const float* __restrict__ ti_in,
             const int refine_pass_n, const int yaw_n, const double* __restrict__ offsets, const double yaw_clip,
             double* __restrict__ yaw_out, double* __restrict__ power_out, int* __restrict__ order_out) {
    extern __shared__ double st_lds_srf[];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = p.N, nthr = yaw_n * 64;
    double* yaw = st_lds_srf;              // [N] committed yaws, degrees
    double* cand_p = yaw + N;              // [16] farm power of every candidate
    float* xr = reinterpret_cast<float*>(cand_p + 16);
    float* yr = xr + N;
    int* by_rank = reinterpret_cast<int*>(yr + N);
    float* com = reinterpret_cast<float*>(by_rank + N);                   // committed state: cg sg u til ct hv
    float* my = com + 6 * N + (size_t)wave * WG_SRF_WAVE_ARRAYS * N;      // this wave's state, same order, then pw
    float *cg = my, *sg = cg + N, *u = sg + N, *til = u + N, *ct = til + N, *hv = ct + N, *pw = hv + N;
    const float ws = ws_in[c], ti = ti_in[c];
    st_frame(p, wd_in[c], tid, nthr, xr, yr);
    for (int t = tid; t < N; t += nthr) yaw[t] = 0.0;
    for (int t = lane; t < N; t += 64) {
        st_set_yaw(0.f, cg[t], sg[t]);
        u[t] = ws; til[t] = ti; ct[t] = 0.f; hv[t] = 0.f;
    }
    __syncthreads();
    st_rank(N, tid, nthr, xr, by_rank);
    __syncthreads();
    // farm power of this wave's state with ranks from .. N-1 evaluated anew -> cand_p[wave] (fp64 sum in index order)
    auto farm_power = [&](const int from) {
        for (int r = from; r < N; ++r) {
            st_visit(p, ws, ti, by_rank[r], lane, xr, yr, cg, sg, u, til, ct, hv);
            __syncthreads();
        }
        for (int s = lane; s < N; s += 64) pw[s] = st_power(p, u[s], cg[s]);
        __syncthreads();
        if (lane == 0) {
            double sum = 0.0;
            for (int s = 0; s < N; ++s) sum += (double)pw[s];
            cand_p[wave] = sum;
        }
        __syncthreads();
    };
    // the farm at zero yaw: every wave evaluates it, so that all states start equal to the committed one (wave 0's copy)
    farm_power(0);
    double best = cand_p[0];
    if (wave == 0)
        for (int i = lane; i < 6 * N; i += 64) com[i] = my[i];
    __syncthreads();
    for (int pass = 0; pass < refine_pass_n; ++pass) {
        for (int pos = 0; pos < N; ++pos) {
            const int t = by_rank[pos];
            if (lane == 0) st_set_yaw((float)(yaw[t] + offsets[pass * yaw_n + wave]), cg[t], sg[t]);
            __syncthreads();
            farm_power(pos);
            int jb = 0;
            double pb = cand_p[0];
            for (int j = 1; j < yaw_n; ++j) {          // first index of the largest power
                const double pj = cand_p[j];
                if (pj > pb) { pb = pj; jb = j; }
            }
            if (pb > best) {          // (uniform over the workgroup: every thread reads the same candidates)
                best = pb;
                const float* win = com + 6 * N + (size_t)jb * WG_SRF_WAVE_ARRAYS * N;
                for (int r = pos + tid; r < N; r += nthr) {
                    const int o = by_rank[r];
                    for (int a = 0; a < 6; ++a) com[a * N + o] = win[a * N + o];
                }
                if (tid == 0) yaw[t] = yaw[t] + offsets[pass * yaw_n + jb];
            }
            __syncthreads();
            // every wave takes t's committed state back (lanes 0 .. 5: one array each); ranks < pos + 1 equal the committed again
            if (lane < 6) my[lane * N + t] = com[lane * N + t];
        }
    }
    __syncthreads();
    for (int t = tid; t < N; t += nthr) {
        yaw_out[(size_t)c * N + t] = fmin(fmax(yaw[t], -yaw_clip), yaw_clip);
        if (order_out) order_out[(size_t)c * N + t] = by_rank[t];
    }
    if (tid == 0 && power_out) power_out[c] = best;
}

extern "C" void wg_launch_steady(const void* sp, const float* ws, const float* wd, const float* ti, const float* yaw, float* power,
                                 hipStream_t st) {
    const SteadyP* p = (const SteadyP*)sp;
    const size_t lds = (size_t)p->N * (8 * sizeof(float) + sizeof(int));
    hipLaunchKernelGGL(k_steady, dim3(p->n_cases), dim3(64), lds, st, *p, ws, wd, ti, yaw, power);
}

extern "C" size_t wg_steady_srf_lds(int N, int yaw_n) {
    return (size_t)N * 44 + 128 + (size_t)N * yaw_n * WG_SRF_WAVE_ARRAYS * sizeof(float);
}
extern "C" void wg_launch_steady_srf(const void* sp, const float* ws, const float* wd, const float* ti, int refine_pass_n, int yaw_n,
                                     const double* offsets, double yaw_clip, double* yaw, double* power, int* order, hipStream_t st) {
    const SteadyP* p = (const SteadyP*)sp;
    hipLaunchKernelGGL(k_steady_srf, dim3(p->n_cases), dim3(64 * yaw_n), wg_steady_srf_lds(p->N, yaw_n), st, *p, ws, wd, ti,
                       refine_pass_n, yaw_n, offsets, yaw_clip, yaw, power, order);
}
