// wg_lstm.hip — recurrent policies on the device: k_lstm advances up to two one-layer LSTMs (sb3-contrib's lstm_actor / lstm_critic)
// by one step on observation rows, k_lstm_pack builds its weight layout, and the wg_lstm_* entries of include/windgym_hip.h wrap
// them (wg_lstm.h states the model and both layouts).
//
// k_lstm: one workgroup of 4 waves owns 32 rows of ONE net.  The step is one GEMM D[4H][row] = Wcat[4H][K] xcat[K][row], K = n_in + H,
// on the tile core of wg_tile.h — the k-ordered f32 fmaf chain of k_policy, so a row's result depends on
// nothing but that row, its state and the weights (no atomics, no cross-row sum, an order fixed by the shapes alone).  The row
// x ‖ select(start, 0, h) streams through LDS as [k][32 rows] in chunks of 256 (conflict-free stores and one ds_read per k-step);
// the weights come packed from L2 as the A operand, output tile 4u + q = gate q of the units 32u .. 32u + 31.  Wave w accumulates
// the eight tiles of its unit blocks w and w + 4 (128 accumulator registers), so it holds z_i, z_f, z_g, z_o of a (unit, row) in
// ONE lane and finishes c' and h' there: no gate array in LDS, no second pass.  LDS: 32 KB static (k_policy: 64 KB).
// k_lstm_pop / k_lstm_pack_pop: the same bodies with one more grid axis = the member of a population (wg_lstm.h: wg_lstm_pop_s).
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "../../include/windgym_hip.h"
#include "wg_lstm.h"
#include "wg_host.h"

// grid (tiles of 32 rows, nets evaluated): net = net0 + blockIdx.y.  state_in / state_out [net][h | c][n_rows][H] (state_out may be
// state_in: a workgroup has read every h it needs before its first store, and a (row, unit)'s c is read and written by one lane;
// null: the new state is discarded), h_out[net] [n_rows][H] (null: not wanted).
// (Two waves per SIMD asked for: without the bound the compiler spreads the accumulators over 145 VGPRs + 144 AGPRs and one workgroup
// fills a CU; with it 202 VGPRs, nothing spilled, and two workgroups of 32 KB LDS share the CU.  One unit block per wave in workgroups
// of 8 waves — 121 VGPRs, occupancy 4 — was measured too and was no faster at 256 envs and 10 % slower at 4096: DESIGN §4.)
// (one workgroup of k_lstm / k_lstm_pop: the 32 rows from blockIdx.x's tile of ONE net on `n_rows` rows; every pointer is the first
// row's, the state's the first net's)
__device__ __forceinline__ void wgl_step(const WgLstmP& P, const float* __restrict__ packed, const float* __restrict__ x,
                                         const uint8_t* __restrict__ start, const float* state_in, float* state_out,
                                         float* __restrict__ h_out0, float* __restrict__ h_out1, const int n_rows, const int net) {
    __shared__ float lds[WGP_KC * WGP_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int row0 = blockIdx.x * WGP_TILE;
    const int H = P.H, n_in = P.n_in, K = P.K;
    const WgLstmNet nt = P.net[net];
    const size_t plane = (size_t)n_rows * H;
    const float* h_in = state_in + (size_t)net * 2 * plane;
    const float* c_in = h_in + plane;
    const int row = row0 + r;
    const bool valid = row < n_rows;
    const bool fresh = valid && start && start[row] != 0;      // the select: a fresh row never reads its incoming state

    f32x16 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int ub = wave + WGP_WAVES * t;
        if (ub < P.nub) {
#pragma unroll
            for (int q = 0; q < 4; ++q) wg_tile_bias(acc[t][q], packed + nt.b_packed + (4 * ub + q) * 32, hh);
        }
    }
    const float* xrow = x + (size_t)row * n_in;
    const float* hrow = h_in + (size_t)row * H;
    const float* xb = lds + hh * WGP_TILE + r;
    for (int k0 = 0; k0 < K; k0 += WGP_KC) {
        const int kc = min(WGP_KC, K - k0), kcp = wg_tile_kpad(kc);
        // x ‖ h -> LDS: rows past n_rows, the pad behind kc and the h of a fresh row are zeros
        wg_tile_stage(lds, tid, kcp, [&](const int k) {
            const int kk = k0 + k;
            float v = 0.0f;
            if (valid && k < kc) {
                if (kk < n_in) v = xrow[kk];
                else if (!fresh) v = hrow[kk - n_in];
            }
            return v;
        });
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int ub = wave + WGP_WAVES * t;
            if (ub < P.nub) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    wg_tile_gemm(acc[t][q], packed + nt.w_packed + ((size_t)(4 * ub + q) * P.nks + (k0 >> 1)) * 64 + lane, xb, kcp >> 1);
            }
        }
    }
    float* h_new = state_out ? state_out + (size_t)net * 2 * plane : nullptr;
    float* c_new = h_new ? h_new + plane : nullptr;
    float* h_out = net == 0 ? h_out0 : h_out1;
    if (!valid) return;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int ub = wave + WGP_WAVES * t;
        if (ub < P.nub) {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int unit = 32 * ub + wg_tile_drow(g, hh);       // of each of the four gates
                if (unit < H) {
                    const size_t o = (size_t)row * H + unit;
                    const float c = fresh ? 0.0f : c_in[o];
                    const float cn = wgl_sigmoid(acc[t][1][g]) * c + wgl_sigmoid(acc[t][0][g]) * tanhf(acc[t][2][g]);
                    const float hn = wgl_sigmoid(acc[t][3][g]) * tanhf(cn);
                    if (c_new) { c_new[o] = cn; h_new[o] = hn; }
                    if (h_out) h_out[o] = hn;
                }
            }
        }
    }
}

__global__ __launch_bounds__(WGP_WAVES * 64, 2) void k_lstm(const WgLstmP P, const float* __restrict__ packed, const float* __restrict__ x,
                                                            const uint8_t* __restrict__ start, const float* state_in, float* state_out,
                                                            float* __restrict__ h_out0, float* __restrict__ h_out1, const int n_rows,
                                                            const int net0) {
    wgl_step(P, packed, x, start, state_in, state_out, h_out0, h_out1, n_rows, net0 + blockIdx.y);
}

// A population's step (wg_lstm_pop): grid (tiles of 32 rows of ONE member, nets evaluated, members).  Member m = blockIdx.z owns the
// rows [m Bm, (m + 1) Bm) of x, start and h_out, its own state [nets][2][Bm][H] at state + m nets 2 Bm H, and its own packed weights;
// a tile never straddles two members.  The member is a function of blockIdx alone, so its pointers are wave-uniform (the packed
// pointers travel as kernel arguments: 16 of them, read by one scalar load), and what a workgroup computes is wgl_step on them — the
// arithmetic of k_lstm on the member's rows alone.
__global__ __launch_bounds__(WGP_WAVES * 64, 2) void k_lstm_pop(const WgLstmP P, const WgLstmPopW W, const float* __restrict__ x,
                                                                const uint8_t* __restrict__ start, const float* state_in, float* state_out,
                                                                float* __restrict__ h_out0, float* __restrict__ h_out1, const int Bm,
                                                                const int net0) {
    const size_t m = blockIdx.z, r0 = m * Bm, s0 = m * P.n_nets * 2 * Bm * P.H;
    wgl_step(P, W.packed[m], x + r0 * P.n_in, start ? start + r0 : nullptr, state_in + s0, state_out ? state_out + s0 : nullptr,
             h_out0 ? h_out0 + r0 * P.H : nullptr, h_out1 ? h_out1 + r0 * P.H : nullptr, Bm, net0 + blockIdx.y);
}

// flat -> packed (wg_lstm.h); one thread per packed float.  b_ih + b_hh is added HERE, once.
__device__ __forceinline__ void wgl_pack(const WgLstmP& P, const float* __restrict__ flat, float* __restrict__ packed) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P.n_packed) return;
    const uint32_t H = P.H, n_in = P.n_in, K = P.K, nks = P.nks;
    const uint32_t wsize = wg_tile_wsize(4 * P.nub, nks), bsize = wg_tile_bsize(4 * P.nub);
    float v = 0.0f;
    for (int net = 0; net < P.n_nets; ++net) {
        const WgLstmNet nt = P.net[net];
        if (idx >= nt.w_packed && idx < nt.w_packed + wsize) {
            const WgTileElem e = wg_tile_decode(idx - nt.w_packed, nks);
            const int32_t i = wgl_tile_row(e.tile, e.j, H);
            if (i >= 0 && e.k < K)
                v = e.k < n_in ? flat[nt.wih_flat + (size_t)i * n_in + e.k] : flat[nt.whh_flat + (size_t)i * H + (e.k - n_in)];
        } else if (idx >= nt.b_packed && idx < nt.b_packed + bsize) {
            const uint32_t e = idx - nt.b_packed;
            const int32_t i = wgl_tile_row(e >> 5, e & 31, H);
            if (i >= 0) v = flat[nt.bih_flat + i] + flat[nt.bhh_flat + i];
        }
    }
    packed[idx] = v;
}

__global__ void k_lstm_pack(const WgLstmP P, const float* __restrict__ flat, float* __restrict__ packed) { wgl_pack(P, flat, packed); }

// every member of a population: blockIdx.y = member, its flat parameters -> its LSTM's packed copy
__global__ void k_lstm_pack_pop(const WgLstmP P, const WgLstmPopW W) { wgl_pack(P, W.flat[blockIdx.y], const_cast<float*>(W.packed[blockIdx.y])); }

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int wg_lstm_create(const wg_lstm_desc* d, int device, wg_lstm* out) {
    if (!d || !out) return wg_fail(WG_ERR_INVALID, "wg_lstm_create: null argument");
    *out = nullptr;
    if (d->n_in < 1 || d->hidden < 1) return wg_fail(WG_ERR_INVALID, "wg_lstm_create: n_in and hidden must be >= 1");
    if (d->n_nets != 1 && d->n_nets != 2) return wg_fail(WG_ERR_INVALID, "wg_lstm_create: n_nets must be 1 (shared) or 2 (actor, critic)");
    if (d->n_in > WGP_MAX_IN) return wg_fail(WG_ERR_UNSUPPORTED, "wg_lstm_create: n_in = " + std::to_string(d->n_in) + " > " + std::to_string(WGP_MAX_IN));
    if (d->hidden > WGL_MAX_H) return wg_fail(WG_ERR_UNSUPPORTED, "wg_lstm_create: hidden = " + std::to_string(d->hidden) + " > " + std::to_string(WGL_MAX_H));
    wg_lstm_s* l = new (std::nothrow) wg_lstm_s();
    if (!l) return wg_fail(WG_ERR_NOMEM, "wg_lstm_create: out of host memory");
    wgl_fill_layout(l->P, d);
    l->mem.device = device;
    if (int rc = wg_packed_alloc_(&l->mem, &l->w, l->P.n_flat, l->P.n_packed, "wg_lstm_create")) {
        wg_lstm_destroy(l);
        return rc;
    }
    *out = l;
    return 0;
}

extern "C" int wg_lstm_destroy(wg_lstm l) {
    if (!l) return 0;
    l->mem.release();
    delete l;
    return 0;
}

extern "C" int wg_lstm_n_params(wg_lstm l, size_t* n) {
    if (!l || !n) return wg_fail(WG_ERR_INVALID, "wg_lstm_n_params: null argument");
    *n = l->P.n_flat;
    return 0;
}

extern "C" int wg_lstm_geometry_(wg_lstm l, int* n_in, int* hidden, int* n_nets, int* device) {
    if (!l) return wg_fail(WG_ERR_INVALID, "wg_lstm: null handle");
    *n_in = l->P.n_in; *hidden = l->P.H; *n_nets = l->P.n_nets; *device = l->w.device;
    return 0;
}

extern "C" int wg_lstm_set_params(wg_lstm l, const float* params, size_t n, int on_device, void* stream) {
    if (!l || !params) return wg_fail(WG_ERR_INVALID, "wg_lstm_set_params: null argument");
    if (n != l->P.n_flat)
        return wg_fail(WG_ERR_INVALID, "wg_lstm_set_params: " + std::to_string(n) + " parameters given, the LSTM has " + std::to_string(l->P.n_flat));
    hipStream_t st = (hipStream_t)stream;
    const float* src;
    if (int rc = wg_packed_source_(&l->w, params, on_device, st, &src)) return rc;
    hipLaunchKernelGGL(k_lstm_pack, dim3((l->P.n_packed + 255) / 256), dim3(256), 0, st, l->P, src, l->w.packed);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_lstm_step(wg_lstm l, int n_rows, const float* x_dev, const uint8_t* episode_start_dev, const float* state_in_dev,
                            float* state_out_dev, float* h_pi_dev, float* h_vf_dev, int net_mask, void* stream) {
    if (!l || !x_dev || !state_in_dev) return wg_fail(WG_ERR_INVALID, "wg_lstm_step: null argument (x_dev and state_in_dev are required)");
    if (n_rows < 0) return wg_fail(WG_ERR_INVALID, "wg_lstm_step: n_rows < 0");
    const int all = l->P.n_nets == 2 ? (WG_LSTM_ACTOR | WG_LSTM_CRITIC) : WG_LSTM_ACTOR;
    if (net_mask == 0) net_mask = all;
    if (net_mask & ~all)
        return wg_fail(WG_ERR_INVALID, "wg_lstm_step: net_mask = " + std::to_string(net_mask) + " names a net this LSTM does not have (n_nets = " +
                                         std::to_string(l->P.n_nets) + ")");
    if (!(net_mask & WG_LSTM_ACTOR) && h_pi_dev) return wg_fail(WG_ERR_INVALID, "wg_lstm_step: h_pi_dev given, but net_mask leaves the actor's LSTM out");
    if (!(net_mask & WG_LSTM_CRITIC) && h_vf_dev)
        return wg_fail(WG_ERR_INVALID, "wg_lstm_step: h_vf_dev given, but net_mask leaves the critic's LSTM out (a shared LSTM has none: the critic reads h_pi)");
    if (n_rows == 0) return 0;
    if (int rc = wg_use_device(l->w.device)) return rc;
    const int net0 = (net_mask & WG_LSTM_ACTOR) ? 0 : 1, nn = net_mask == (WG_LSTM_ACTOR | WG_LSTM_CRITIC) ? 2 : 1;
    hipLaunchKernelGGL(k_lstm, dim3((n_rows + WGP_TILE - 1) / WGP_TILE, nn), dim3(WGP_WAVES * 64), 0, (hipStream_t)stream, l->P, l->w.packed,
                       x_dev, episode_start_dev, state_in_dev, state_out_dev, h_pi_dev, h_vf_dev, n_rows, net0);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("wg_lstm_step: kernel launch failed: ") + hipGetErrorString(le));
    return 0;
}

// The LSTMs' step and the MLP behind them: two launches.  The critic's LSTM runs only when the value is wanted.
extern "C" int wg_lstm_act(wg_lstm l, wg_policy p, int n_rows, const float* x_dev, const uint8_t* episode_start_dev, const float* state_in_dev,
                           float* state_out_dev, float* h_dev, int deterministic, uint64_t seed, uint64_t counter, uint64_t row_offset,
                           float* action_dev, float* raw_dev, float* logp_dev, float* value_dev, void* stream) {
    if (!l || !p || !h_dev) return wg_fail(WG_ERR_INVALID, "wg_lstm_act: null argument (l, p and h_dev are required)");
    if (p->P.n_in != l->P.H || p->P.n_layers[1] == 0 || p->P.n_in_vf != l->P.H)
        return wg_fail(WG_ERR_INVALID, "wg_lstm_act: p must map the LSTM's hidden size (" + std::to_string(l->P.H) + ") with its critic on the same width; it maps " +
                                         std::to_string(p->P.n_in) + " inputs, its critic " + std::to_string(p->P.n_layers[1] ? p->P.n_in_vf : 0));
    if (p->w.device != l->w.device) return wg_fail(WG_ERR_INVALID, "wg_lstm_act: lstm and policy live on different devices");
    if (n_rows < 0) return wg_fail(WG_ERR_INVALID, "wg_lstm_act: n_rows < 0");
    const bool two = l->P.n_nets == 2, critic = two && value_dev;
    float* const h_pi = h_dev;
    float* const h_vf = two ? h_dev + (size_t)n_rows * l->P.H : h_dev;
    if (int rc = wg_lstm_step(l, n_rows, x_dev, episode_start_dev, state_in_dev, state_out_dev, h_pi, critic ? h_vf : nullptr,
                              WG_LSTM_ACTOR | (critic ? WG_LSTM_CRITIC : 0), stream))
        return rc;
    const WgValueRows v = {h_vf, value_dev, n_rows};
    return wg_policy_eval_(p, n_rows, h_pi, deterministic, seed, counter, row_offset, action_dev, raw_dev, logp_dev, &v, value_dev ? 1 : 0, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// populations of recurrent policies: the step and the heads' slot table (wg_lstm_pop_create / _update: wg_lstm_ppo.hip; the closed
// loop: wg_api.hip)
// ---------------------------------------------------------------------------------------------------------------------
static WgLstmPopW lpop_weights(const wg_lstm_pop_s* q, const float* const* params_dev) {
    WgLstmPopW W = {};
    for (int m = 0; m < q->P; ++m) {
        W.packed[m] = q->lstm[m]->w.packed;
        W.flat[m] = params_dev ? params_dev[m] : nullptr;
    }
    return W;
}

// wg_lstm_step for every member in ONE launch of k_lstm_pop: n_rows = P Bm rows, member m on its own rows, state and weights
extern "C" int wg_lstm_pop_step_(wg_lstm_pop q, int n_rows, const float* x_dev, const uint8_t* episode_start_dev, const float* state_in_dev,
                                 float* state_out_dev, float* h_pi_dev, float* h_vf_dev, int net_mask, void* stream) {
    const WgLstmP& P = q->lstm[0]->P;
    const int Bm = n_rows / q->P;
    if (Bm == 0) return 0;
    if (int rc = wg_use_device(q->device)) return rc;
    const int net0 = (net_mask & WG_LSTM_ACTOR) ? 0 : 1, nn = net_mask == (WG_LSTM_ACTOR | WG_LSTM_CRITIC) ? 2 : 1;
    hipLaunchKernelGGL(k_lstm_pop, dim3((Bm + WGP_TILE - 1) / WGP_TILE, nn, q->P), dim3(WGP_WAVES * 64), 0, (hipStream_t)stream, P,
                       lpop_weights(q, nullptr), x_dev, episode_start_dev, state_in_dev, state_out_dev, h_pi_dev, h_vf_dev, Bm, net0);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("wg_lstm_pop: kernel launch failed: ") + hipGetErrorString(le));
    return 0;
}

// k_lstm_pack for every member in ONE launch: params_dev[m] (the member's flat vector, the LSTM's part first) -> its packed copy
extern "C" int wg_lstm_pack_pop_(wg_lstm_pop q, const float* const* params_dev, void* stream) {
    const WgLstmP& P = q->lstm[0]->P;
    hipLaunchKernelGGL(k_lstm_pack_pop, dim3((P.n_packed + 255) / 256, q->P), dim3(256), 0, (hipStream_t)stream, P, lpop_weights(q, params_dev));
    WG_HIPCHK(hipGetLastError());
    return 0;
}

// The heads' slot table (wg_policy.h: WgPopSlot) on the LSTMs' h rows: P actor slots on h_pi (when an actor output is wanted), P
// critic slots on h_vf (value), P critic slots on h_fin (final_value), member m on rows [m Bm, (m + 1) Bm).  The h rows are the
// running step's (no step stride); the outputs are one call's (o->step = 0) or a rollout's [T, B, ..] (o->step = B).
extern "C" int wg_lstm_pop_slots_(wg_lstm_pop q, int n_rows, const uint64_t* seeds, const uint64_t* row_offsets, const float* h_pi,
                                  const float* h_vf, const float* h_fin, const WgPopOuts* o, void* stream) {
    const int H = q->lstm[0]->P.H;
    const WgPopKind kinds[3] = {{h_pi, H, 0}, {h_vf, H, 0}, {h_fin, H, 0}};
    return wg_pop_slots_(&q->heads, n_rows / q->P, kinds, o, seeds, row_offsets, stream);
}

// The members' LSTM steps and the MLPs behind them: two launches.  The critics' LSTMs run only when the value is wanted.
extern "C" int wg_lstm_pop_act(wg_lstm_pop q, int n_rows, const float* x_dev, const uint8_t* episode_start_dev, const float* state_in_dev,
                               float* state_out_dev, float* h_dev, int deterministic, const uint64_t* seeds, uint64_t counter,
                               const uint64_t* row_offsets, float* action_dev, float* raw_dev, float* logp_dev, float* value_dev, void* stream) {
    if (!q || !x_dev || !state_in_dev || !h_dev) return wg_fail(WG_ERR_INVALID, "wg_lstm_pop_act: null argument (q, x_dev, state_in_dev and h_dev are required)");
    if (n_rows < 0) return wg_fail(WG_ERR_INVALID, "wg_lstm_pop_act: n_rows < 0");
    if (int rc = wg_pop_shares("wg_lstm_pop_act", q->P, n_rows, "rows", "", " rows do")) return rc;
    if ((action_dev || raw_dev || logp_dev) && !seeds) return wg_fail(WG_ERR_INVALID, "wg_lstm_pop_act: seeds[P] is required");
    if ((action_dev || raw_dev || logp_dev) && !q->heads.pol[0]->P.has_log_std && (!deterministic || logp_dev))
        return wg_fail(WG_ERR_INVALID, "wg_lstm_pop_act: a stochastic action / a log-probability needs policies with log_std");
    const WgLstmP& L = q->lstm[0]->P;
    const bool two = L.n_nets == 2, critic = two && value_dev;
    float* const h_pi = h_dev;
    float* const h_vf = two ? h_dev + (size_t)n_rows * L.H : h_dev;
    const WgPopOuts o = {action_dev, raw_dev, logp_dev, value_dev, nullptr, 0};
    if (int rc = wg_lstm_pop_slots_(q, n_rows, seeds, row_offsets, h_pi, h_vf, nullptr, &o, stream)) return rc;
    if (int rc = wg_lstm_pop_step_(q, n_rows, x_dev, episode_start_dev, state_in_dev, state_out_dev, h_pi, critic ? h_vf : nullptr,
                                   WG_LSTM_ACTOR | (critic ? WG_LSTM_CRITIC : 0), stream))
        return rc;
    return wg_pop_launch_(&q->heads, 1, 0, 0, deterministic, counter, stream);
}
