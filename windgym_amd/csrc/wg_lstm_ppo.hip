// wg_lstm_ppo.hip — training recurrent policies on the device: backpropagation through time over one rollout of wg_rollout_lstm, for
// the LSTMs of wg_lstm.hip in front of the MLP heads of wg_policy.hip, and the wg_lstm_ppo_* entries of include/windgym_hip.h
// (wg_lstm_ppo.h states the stash and the transposed packed block); the wg_lstm_bc_* entries, the supervised head on the same handle,
// are above the populations' host side.
//
// THE RULE.  A minibatch is Bm envs with all T steps of each; row (t, j) is env envs[j] at step t, n = T Bm rows.
//   forward    per net, (h, c)_{-1} = lstm_state0[net][., env] — data, not a function of the parameters; for t = 0 .. T-1:
//                  (h, c) <- (0, 0) where episode_start[t][env] != 0            (wg_lstm.h's SELECT: such a row reads no state)
//                  z = (b_ih + b_hh) + [W_ih | W_hh] (x_t ‖ h),  c_t = s(z_f) c + s(z_i) tanh(z_g),  h_t = s(z_o) tanh(c_t)
//   heads      k_ppo_grad's loss, unchanged, on the n rows with obs[0] = the actor LSTM's h rows and obs[1] = the critic LSTM's (the
//              same rows when the LSTM is shared), normalize_advantage over the minibatch's n rows; it returns the MLP's gradient,
//              the 8-float stats record and dH = W0^T dZ0 per head and row (k_ppo_grad_dh)
//   backward   for t = T-1 .. 0:   dh_t = dH[t] (shared LSTM: the actor head's + the critic head's, in that order) + W_hh^T dz_{t+1},
//                  the recurrent term and the carried dc dropped where episode_start[t+1] != 0: the gradient stops there;
//                  do = dh tanh(c_t),  dc = dc_carry + dh o (1 - tanh^2 c_t),  di = dc g,  dg = dc i,  df = dc c_{t-1},  dc_carry = dc f,
//                  dz = (di i (1 - i), df f (1 - f), dg (1 - g^2), do o (1 - o))
//   weights    dWcat[4H][n_in + H] = sum over rows in the order t, j of dz ⊗ (x_t ‖ select(start_t, 0, h_{t-1})),  db_ih = db_hh = sum dz
//   no env     a column whose envs[j] is outside [0, B): its rows reach the heads as h = 0 with raw = logp = advantage = returns = 0
//              (k_lstm_seq_fwd stores the zeros, k_lstm_ppo_gather the rest), count in n, and have dz = 0 at every step
//   gradient   flat: the LSTM tensors, then the MLP's (the entropy constant on log_std included), recurrent.param_layout's order.
// Every sum has an order fixed by T, Bm and the shapes: no atomics, the same bits from run to run.
//
// k_lstm_seq_fwd / k_lstm_seq_bwd: one workgroup of 4 waves owns 32 env columns of ONE net (blockIdx.y) for the WHOLE sequence — the
// time loop is inside the kernel.  Forward is k_lstm's step (one GEMM on wg_tile.h, the four gates of a unit in one lane) with h in
// LDS and c in registers between steps.  Backward keeps dc in registers and the recurrent term in LDS, does the cell's backward
// element-wise, and runs W_hh^T dz as a GEMM over the transposed packed block with dz staged through LDS in chunks of 256 (dz of a
// tile is 128 KB at H = 256).  Both: 64 KB of LDS.  k_lstm_wgrad: output-stationary, a workgroup owns 128 rows x 32 columns of dWcat
// and walks the blocks of its split in index order; at most WGLP_SPLIT rows of partials, added in order by k_lstm_wgrad_reduce.
//
// POPULATIONS (wg_lstm_pop_update): every kernel here has a sibling k_*_pop with one more grid axis = member that runs the same
// __device__ body on the member's row of a device table — P small runs in the launches of one, each bit-identical to its own update.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "../../include/windgym_hip.h"
#include "wg_lstm_ppo.h"
#include "wg_host.h"

// the env of minibatch column j, -1: none (j >= Bm or an entry outside the rollout)
__device__ __forceinline__ int wglp_env(const WgLstmSeq& q, const int j) {
    if (j >= q.Bm) return -1;
    const int e = q.envs[j];
    return (e < 0 || e >= q.B) ? -1 : e;
}

// The bodies below are shared by the single-policy kernels and the population's (k_*_pop, behind them): POP only selects the plane of
// state0, q.sB rows (a member's own state) instead of q.B — with POP = false the code is what it was before the flag.
template <bool POP>
__device__ __forceinline__ int wglp_plane(const WgLstmSeq& q) { return POP ? q.sB : q.B; }

// grid (NT, nets)
template <bool POP>
__device__ __forceinline__ void lstm_seq_fwd(const WgLstmP& P, const float* __restrict__ packed, const WgLstmSeq& q) {
    __shared__ float lds[WGP_KC * WGP_TILE];
    __shared__ float hbuf[WGL_MAX_H * WGP_TILE];           // h_{t-1} as [unit][32 columns]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int net = blockIdx.y, tile = blockIdx.x;
    const int H = P.H, n_in = P.n_in, K = P.K, H4 = 4 * P.H;
    const WgLstmNet nt = P.net[net];
    const int j = tile * WGP_TILE + r, env = wglp_env(q, j);
    const bool valid = env >= 0;
    const float* h0 = q.state0 + (size_t)net * 2 * wglp_plane<POP>(q) * H;
    const float* c0 = h0 + (size_t)wglp_plane<POP>(q) * H;
    for (int unit = tid >> 5; unit < H; unit += 2 * WGP_WAVES) hbuf[unit * WGP_TILE + r] = valid ? h0[(size_t)env * H + unit] : 0.0f;
    float creg[2][16];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
        const int ub = wave + WGP_WAVES * t2;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int unit = 32 * ub + wg_tile_drow(g, hh);
            creg[t2][g] = (valid && unit < H) ? c0[(size_t)env * H + unit] : 0.0f;
        }
    }
    const float* xb = lds + hh * WGP_TILE + r;
    float* gates = q.gates + (size_t)net * q.net_gates;
    float* cst = q.c + (size_t)net * q.net_c;
    float* hst = q.h + (size_t)net * q.net_h;

    for (int t = 0; t < q.T; ++t) {
        const bool fresh = valid && q.start[(size_t)t * q.B + env] != 0;
        const float* xrow = q.obs + ((size_t)t * q.B + (valid ? env : 0)) * n_in;
        f32x16 acc[2][4];
        // (the offset is opaque per step, so that the 128 bias loads stay inside the step instead of being hoisted out of the time
        // loop and held in registers across it)
        uint32_t b_off = nt.b_packed;
        asm volatile("" : "+v"(b_off));
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            const int ub = wave + WGP_WAVES * t2;
            if (ub < P.nub) {
#pragma unroll
                for (int g = 0; g < 4; ++g) wg_tile_bias(acc[t2][g], packed + b_off + (4 * ub + g) * 32, hh);
            }
        }
        for (int k0 = 0; k0 < K; k0 += WGP_KC) {
            const int kc = min(WGP_KC, K - k0), kcp = wg_tile_kpad(kc);
            // x_t ‖ h_{t-1} -> LDS: columns without an env, the pad behind kc and the h of a fresh row are zeros
            wg_tile_stage(lds, tid, kcp, [&](const int k) {
                const int kk = k0 + k;
                float v = 0.0f;
                if (valid && k < kc) {
                    if (kk < n_in) v = xrow[kk];
                    else if (!fresh) v = hbuf[(kk - n_in) * WGP_TILE + r];
                }
                return v;
            });
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                const int ub = wave + WGP_WAVES * t2;
                if (ub < P.nub) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        wg_tile_gemm(acc[t2][g], packed + nt.w_packed + ((size_t)(4 * ub + g) * P.nks + (k0 >> 1)) * 64 + lane, xb, kcp >> 1);
                }
            }
        }
        // the cell, in the lane that holds the unit's four gates; every column of the tile is written (one without an env ran on zeros).
        // (The lane's column is made opaque per step and every address is a uniform base + a 32-bit offset: left to itself the compiler
        // keeps one 64-bit pointer per store of the unrolled loop alive across the time loop, about 200 of them, and spills.)
        const size_t blk = (size_t)t * q.NT + tile;
        float* G = gates + blk * H4 * WGP_TILE;
        float* Cs = cst + blk * H * WGP_TILE;
        float* hr = hst + (size_t)t * q.Bm * H;
        uint32_t ro = r;
        asm volatile("" : "+v"(ro));
        const uint32_t jo = (uint32_t)tile * WGP_TILE + ro, HT = (uint32_t)H * WGP_TILE;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            const int ub = wave + WGP_WAVES * t2;
            if (ub < P.nub) {
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int unit = 32 * ub + wg_tile_drow(g, hh);
                    if (unit < H) {
                        const float c = fresh ? 0.0f : creg[t2][g];
                        const float gi = wgl_sigmoid(acc[t2][0][g]), gf = wgl_sigmoid(acc[t2][1][g]), gg = tanhf(acc[t2][2][g]),
                                    go = wgl_sigmoid(acc[t2][3][g]);
                        const float cn = gf * c + gi * gg;
                        const float hn = go * tanhf(cn);
                        const uint32_t o = (uint32_t)unit * WGP_TILE + ro;
                        G[o] = gi;
                        G[HT + o] = gf;
                        G[2 * HT + o] = gg;
                        G[3 * HT + o] = go;
                        Cs[o] = cn;
                        // (the heads read all T Bm rows: a column whose entry is outside the rollout is a row of zeros, not the stash's past)
                        if (jo < (uint32_t)q.Bm) hr[jo * (uint32_t)H + unit] = valid ? hn : 0.0f;
                        hbuf[o] = hn;                          // (read again only behind the next step's barrier)
                        creg[t2][g] = cn;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(WGP_WAVES * 64) void k_lstm_seq_fwd(const WgLstmP P, const float* __restrict__ packed, const WgLstmSeq q) {
    lstm_seq_fwd<false>(P, packed, q);
}

// grid (NT, nets).  Thread (r = tid & 31, u = tid >> 5) owns the units u, u + 8, ... of column r at every step: its dc never leaves
// its registers.
template <bool POP>
__device__ __forceinline__ void lstm_seq_bwd(const WgLstmP& P, const WgLstmSeq& q) {
    __shared__ float lds[WGP_KC * WGP_TILE];
    __shared__ float rec[WGL_MAX_H * WGP_TILE];            // W_hh^T dz_{t+1} as [unit][32 columns]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5, u0 = tid >> 5;
    const int net = blockIdx.y, tile = blockIdx.x;
    const int H = P.H, H4 = 4 * P.H;
    const int j = tile * WGP_TILE + r, env = wglp_env(q, j);
    const bool valid = env >= 0;
    const float* c0 = q.state0 + ((size_t)net * 2 + 1) * wglp_plane<POP>(q) * H;
    float* gates = q.gates + (size_t)net * q.net_gates;
    const float* cst = q.c + (size_t)net * q.net_c;
    // (a member's q is a copy in registers: no index by `net` there)
    const float* dh0 = POP ? (net ? q.dh[1] : q.dh[0]) : q.dh[net];
    const float* dh1 = q.shared ? q.dh[1] : nullptr;
    const float* wT = q.whhT + (size_t)net * q.whhT_net;
    const float* xb = lds + hh * WGP_TILE + r;
    float dc[WGL_MAX_H / 8];
#pragma unroll
    for (int m = 0; m < WGL_MAX_H / 8; ++m) dc[m] = 0.0f;
    bool cut = true;                                       // no recurrent term reaches this step (the last step; a fresh step behind it)

    for (int t = q.T - 1; t >= 0; --t) {
        const bool fresh = valid && q.start[(size_t)t * q.B + env] != 0;
        const size_t blk = (size_t)t * q.NT + tile;
        float* G = gates + blk * H4 * WGP_TILE;
        const float* Cs = cst + blk * H * WGP_TILE;
        const float* Cp = t > 0 ? cst + (blk - q.NT) * H * WGP_TILE : Cs;   // c_{t-1} (t = 0: c0 instead)
        const size_t row = (size_t)t * q.Bm + j;
        __syncthreads();                                   // rec of step t + 1 is complete
#pragma unroll
        for (int m = 0; m < WGL_MAX_H / 8; ++m) {
            const int unit = u0 + 8 * m;
            if (unit < H) {
                const size_t o = (size_t)unit * WGP_TILE + r;
                float zi = 0.0f, zf = 0.0f, zg = 0.0f, zo = 0.0f;
                if (valid) {
                    float dh = dh0[row * H + unit];
                    if (dh1) dh += dh1[row * H + unit];
                    if (!cut) dh += rec[o];
                    const float gi = G[o], gf = G[(size_t)H * WGP_TILE + o], gg = G[(size_t)2 * H * WGP_TILE + o], go = G[(size_t)3 * H * WGP_TILE + o];
                    const float cp = fresh ? 0.0f : (t > 0 ? Cp[o] : c0[(size_t)env * H + unit]);
                    const float tc = tanhf(Cs[o]);
                    const float d_o = dh * tc;
                    const float dct = dc[m] + dh * go * (1.0f - tc * tc);
                    zi = dct * gg * gi * (1.0f - gi);
                    zf = dct * cp * gf * (1.0f - gf);
                    zg = dct * gi * (1.0f - gg * gg);
                    zo = d_o * go * (1.0f - go);
                    dc[m] = fresh ? 0.0f : dct * gf;
                }
                G[o] = zi; G[(size_t)H * WGP_TILE + o] = zf; G[(size_t)2 * H * WGP_TILE + o] = zg; G[(size_t)3 * H * WGP_TILE + o] = zo;
            }
        }
        cut = fresh;
        if (t == 0) break;
        // rec = W_hh^T dz_t: M = H (wave w: unit tiles w and w + 4), K = 4H through LDS in chunks (the stage's barrier orders the
        // block's stores above before its loads)
        f32x16 acc[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[t2][g] = 0.0f;
        for (int k0 = 0; k0 < H4; k0 += WGP_KC) {
            const int kc = min(WGP_KC, H4 - k0), kcp = wg_tile_kpad(kc);
            wg_tile_stage(lds, tid, kcp, [&](const int k) { return k < kc ? G[(size_t)(k0 + k) * WGP_TILE + r] : 0.0f; });
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                const int ot = wave + WGP_WAVES * t2;
                if (ot < P.nub) wg_tile_gemm(acc[t2], wT + ((size_t)ot * q.nksT + (k0 >> 1)) * 64 + lane, xb, kcp >> 1);
            }
        }
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            const int ot = wave + WGP_WAVES * t2;
            if (ot < P.nub) {
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int unit = 32 * ot + wg_tile_drow(g, hh);
                    if (unit < H) rec[unit * WGP_TILE + r] = acc[t2][g];
                }
            }
        }
    }
}

__global__ __launch_bounds__(WGP_WAVES * 64) void k_lstm_seq_bwd(const WgLstmP P, const WgLstmSeq q) { lstm_seq_bwd<false>(P, q); }

// grid (ceil(K / 32), ceil(4H / 128), nets * S): wave w of workgroup (kt, it) owns rows 128 it + 32 w .. + 31, columns 32 kt .. + 31
// of dWcat and sums over its SPLIT's blocks in index order, 32 rows per block on v_mfma_f32_32x32x2_f32 (A = dz, B = xcat, both from
// LDS with a row stride of 33 floats).  The workgroups kt = 0 also sum the biases.  Split sp of S = min(WGLP_SPLIT, T NT) takes the
// blocks [sp per, (sp + 1) per), per = ceil(T NT / S), and writes row sp of part[S][n_lstm] (the LSTM's flat layout);
// k_lstm_wgrad_reduce adds the rows in index order.  S and per are functions of T and NT alone: the order of every sum is fixed.  One
// workgroup per output tile alone is latency-bound — two barriers and one round of global loads per 16 MFMAs — and leaves CUs idle;
// the split is there for workgroups per CU, not for the arithmetic.
#define WGLP_WI 128
#define WGLP_S 33
// (`z`: the workgroup's index along (net, split), blockIdx.z of the single-policy grid)
template <bool POP>
__device__ __forceinline__ void lstm_wgrad(const WgLstmP& P, const WgLstmSeq& q, float* __restrict__ part, const int S, const int z) {
    __shared__ float ds[WGLP_WI * WGLP_S];
    __shared__ float xs[32 * WGLP_S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int kt = blockIdx.x, i0 = blockIdx.y * WGLP_WI, net = z / S, sp = z - net * S;
    const int H = P.H, n_in = P.n_in, K = P.K, H4 = 4 * P.H;
    const WgLstmNet nt = P.net[net];
    float* __restrict__ grad = part + (size_t)sp * P.n_flat;
    const float* gates = q.gates + (size_t)net * q.net_gates;
    const float* hst = q.h + (size_t)net * q.net_h;
    const float* h0 = q.state0 + (size_t)net * 2 * wglp_plane<POP>(q) * H;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    float db = 0.0f;
    const int nblk = q.T * q.NT, per = (nblk + S - 1) / S;
    const int blk1 = min(nblk, (sp + 1) * per);
    for (int blk = sp * per; blk < blk1; ++blk) {
        const int t = blk / q.NT, tile = blk - t * q.NT;
        const float* G = gates + (size_t)blk * H4 * WGP_TILE;
        __syncthreads();
        for (int idx = tid; idx < WGLP_WI * 32; idx += WGP_WAVES * 64) {
            const int il = idx >> 5, row = idx & 31, i = i0 + il;
            ds[il * WGLP_S + row] = i < H4 ? G[(size_t)i * WGP_TILE + row] : 0.0f;
        }
        for (int idx = tid; idx < 32 * 32; idx += WGP_WAVES * 64) {     // consecutive threads: consecutive inputs of a row
            const int row = idx >> 5, kl = idx & 31, kk = kt * 32 + kl, j = tile * WGP_TILE + row;
            const int env = wglp_env(q, j);
            float v = 0.0f;
            if (env >= 0 && kk < K) {
                if (kk < n_in) v = q.obs[((size_t)t * q.B + env) * n_in + kk];
                else if (q.start[(size_t)t * q.B + env] == 0)
                    v = t > 0 ? hst[((size_t)(t - 1) * q.Bm + j) * H + (kk - n_in)] : h0[(size_t)env * H + (kk - n_in)];
            }
            xs[kl * WGLP_S + row] = v;
        }
        __syncthreads();
        if (kt == 0 && tid < WGLP_WI) {
            for (int row = 0; row < 32; ++row) db += ds[tid * WGLP_S + row];
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int row = 2 * s + hh;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[(wave * 32 + r) * WGLP_S + row], xs[r * WGLP_S + row], acc, 0, 0, 0);
        }
    }
    const int k = kt * 32 + r;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i = i0 + wave * 32 + wg_tile_drow(e, hh);
        if (i < H4 && k < K) {
            if (k < n_in) grad[nt.wih_flat + (size_t)i * n_in + k] = acc[e];
            else grad[nt.whh_flat + (size_t)i * H + (k - n_in)] = acc[e];
        }
    }
    if (kt == 0 && tid < WGLP_WI && i0 + tid < H4) {
        grad[nt.bih_flat + i0 + tid] = db;
        grad[nt.bhh_flat + i0 + tid] = db;
    }
}

__global__ __launch_bounds__(WGP_WAVES * 64) void k_lstm_wgrad(const WgLstmP P, const WgLstmSeq q, float* __restrict__ part, const int S) {
    lstm_wgrad<false>(P, q, part, S, blockIdx.z);
}

// the splits' rows -> the LSTM's entries of the flat gradient, added in index order
__device__ __forceinline__ void lstm_wgrad_reduce(const float* __restrict__ part, const uint32_t n, const int S, float* __restrict__ grad) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    float s = part[p];
    for (int g = 1; g < S; ++g) s += part[(size_t)g * n + p];
    grad[p] = s;
}

__global__ void k_lstm_wgrad_reduce(const float* __restrict__ part, const uint32_t n, const int S, float* __restrict__ grad) {
    lstm_wgrad_reduce(part, n, S, grad);
}

// flat -> the transposed packed blocks (wg_lstm_ppo.h); one thread per float, the slack included
__device__ __forceinline__ void lstm_ppo_pack(const WgLstmP& P, const float* __restrict__ flat, float* __restrict__ whhT, const uint32_t per_net,
                                              const uint32_t total, const uint32_t nksT) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint32_t net = idx / per_net;
    float v = 0.0f;
    if (net < (uint32_t)P.n_nets) {
        const WgTileElem e = wg_tile_decode(idx - net * per_net, nksT);
        const uint32_t unit = 32 * e.tile + e.j;
        if (unit < (uint32_t)P.H && e.k < 4u * P.H) v = flat[P.net[net].whh_flat + (size_t)e.k * P.H + unit];
    }
    whhT[idx] = v;
}

__global__ void k_lstm_ppo_pack(const WgLstmP P, const float* __restrict__ flat, float* __restrict__ whhT, const uint32_t per_net,
                                const uint32_t total, const uint32_t nksT) {
    lstm_ppo_pack(P, flat, whhT, per_net, total, nksT);
}

// the minibatch's rows of raw / logp / advantage / returns [T, B] -> row order t Bm + j (a column without an env: zeros)
__device__ __forceinline__ void lstm_ppo_gather(const WgLstmSeq& q, const int n_out, const float* __restrict__ raw, const float* __restrict__ logp,
                                                const float* __restrict__ adv, const float* __restrict__ ret, float* __restrict__ raw_o,
                                                float* __restrict__ logp_o, float* __restrict__ adv_o, float* __restrict__ ret_o) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= q.T * q.Bm) return;
    const int t = row / q.Bm, j = row - t * q.Bm, env = wglp_env(q, j);
    const size_t src = (size_t)t * q.B + (env >= 0 ? env : 0);
    logp_o[row] = env >= 0 ? logp[src] : 0.0f;
    adv_o[row] = env >= 0 ? adv[src] : 0.0f;
    ret_o[row] = env >= 0 ? ret[src] : 0.0f;
    for (int a = 0; a < n_out; ++a) raw_o[(size_t)row * n_out + a] = env >= 0 ? raw[src * n_out + a] : 0.0f;
}

__global__ void k_lstm_ppo_gather(const WgLstmSeq q, const int n_out, const float* __restrict__ raw, const float* __restrict__ logp,
                                  const float* __restrict__ adv, const float* __restrict__ ret, float* __restrict__ raw_o,
                                  float* __restrict__ logp_o, float* __restrict__ adv_o, float* __restrict__ ret_o) {
    lstm_ppo_gather(q, n_out, raw, logp, adv, ret, raw_o, logp_o, adv_o, ret_o);
}

// The supervised head's rows (wg_lstm_bc_grad): the expert's actions [T, B, n_out], and the returns [T, B] when given, -> row order
// t Bm + j (a column without an env: zeros).  ret = null: ret_o is not touched.
__global__ void k_lstm_bc_gather(const WgLstmSeq q, const int n_out, const float* __restrict__ target, const float* __restrict__ ret,
                                 float* __restrict__ target_o, float* __restrict__ ret_o) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= q.T * q.Bm) return;
    const int t = row / q.Bm, j = row - t * q.Bm, env = wglp_env(q, j);
    const size_t src = (size_t)t * q.B + (env >= 0 ? env : 0);
    if (ret) ret_o[row] = env >= 0 ? ret[src] : 0.0f;
    for (int a = 0; a < n_out; ++a) target_o[(size_t)row * n_out + a] = env >= 0 ? target[src * n_out + a] : 0.0f;
}

// k_lstm_wgrad_reduce when only the nets in front of the flat vector ran (wg_lstm_bc_grad without returns: the actor's LSTM alone):
// the entries [0, n_live) are the splits' sums, the entries [n_live, n) — the nets that were not launched — are 0.0f, and their
// columns of `part`, which hold what an earlier call left there, are not read.
__global__ void k_lstm_wgrad_reduce_live(const float* __restrict__ part, const uint32_t n, const uint32_t n_live, const int S,
                                         float* __restrict__ grad) {
    if (blockIdx.x * blockDim.x + threadIdx.x < n_live) lstm_wgrad_reduce(part, n, S, grad);
    else if (blockIdx.x * blockDim.x + threadIdx.x < n) grad[blockIdx.x * blockDim.x + threadIdx.x] = 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------
// The population's kernels: one more grid axis = member, whose row of the member table (wg_lstm_ppo.h: WgLstmPopMember) holds what
// the single-policy kernel takes as arguments.  The member is a function of blockIdx alone, so the row is read by scalar loads into
// the registers the kernel arguments would occupy: nothing per-member is live across a time loop that was not live before.  `off`
// is the running minibatch's offset into every member's permutations, Bm / NT its size.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ WgLstmSeq wglp_member(const WgLstmPopMember* __restrict__ M, const int64_t off, const int Bm, const int NT) {
    WgLstmSeq q = M->q;
    q.envs += off; q.Bm = Bm; q.NT = NT;
    return q;
}

// grid (ceil(whhT_all / 256), P)
__global__ void k_lstm_ppo_pack_pop(const WgLstmP P, const WgLstmPopMember* __restrict__ mt, const uint32_t per_net, const uint32_t total,
                                    const uint32_t nksT) {
    const WgLstmPopMember* __restrict__ M = mt + blockIdx.y;
    lstm_ppo_pack(P, M->params, M->whhT, per_net, total, nksT);
}

// grid (ceil(T Bm / 256), P); raw / logp / adv / ret: the whole rollout's [T, B]
__global__ void k_lstm_ppo_gather_pop(const WgLstmPopMember* __restrict__ mt, const int64_t off, const int Bm, const int NT, const int n_out,
                                      const float* __restrict__ raw, const float* __restrict__ logp, const float* __restrict__ adv,
                                      const float* __restrict__ ret) {
    const WgLstmPopMember* __restrict__ M = mt + blockIdx.y;
    lstm_ppo_gather(wglp_member(M, off, Bm, NT), n_out, raw, logp, adv, ret, M->raw, M->logp, M->adv, M->ret);
}

// grid (NT, nets, P)
__global__ __launch_bounds__(WGP_WAVES * 64) void k_lstm_seq_fwd_pop(const WgLstmP P, const WgLstmPopMember* __restrict__ mt, const int64_t off,
                                                                     const int Bm, const int NT) {
    const WgLstmPopMember* __restrict__ M = mt + blockIdx.z;
    lstm_seq_fwd<true>(P, M->packed, wglp_member(M, off, Bm, NT));
}

__global__ __launch_bounds__(WGP_WAVES * 64) void k_lstm_seq_bwd_pop(const WgLstmP P, const WgLstmPopMember* __restrict__ mt, const int64_t off,
                                                                     const int Bm, const int NT) {
    lstm_seq_bwd<true>(P, wglp_member(mt + blockIdx.z, off, Bm, NT));
}

// grid (ceil(K / 32), ceil(4H / 128), P * nets * S): member = blockIdx.z / (nets S)
__global__ __launch_bounds__(WGP_WAVES * 64) void k_lstm_wgrad_pop(const WgLstmP P, const WgLstmPopMember* __restrict__ mt, const int64_t off,
                                                                   const int Bm, const int NT, const int S) {
    const int per = P.n_nets * S, m = blockIdx.z / per;
    const WgLstmPopMember* __restrict__ M = mt + m;
    lstm_wgrad<true>(P, wglp_member(M, off, Bm, NT), M->wpart, S, blockIdx.z - m * per);
}

// grid (ceil(n_lstm / 256), P)
__global__ void k_lstm_wgrad_reduce_pop(const WgLstmPopMember* __restrict__ mt, const uint32_t n, const int S) {
    const WgLstmPopMember* __restrict__ M = mt + blockIdx.y;
    lstm_wgrad_reduce(M->wpart, n, S, M->grad);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int wg_lstm_ppo_create(wg_lstm l, wg_policy p, int T_max, int Bm_max, wg_lstm_ppo* out) {
    if (!l || !p || !out) return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_create: null argument");
    *out = nullptr;
    const WgLstmP& L = l->P;
    if (p->P.n_in != L.H || p->P.n_layers[1] == 0 || p->P.n_in_vf != L.H)
        return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_create: p must map the LSTM's hidden size (" + std::to_string(L.H) +
                                         ") with its critic on the same width; it maps " + std::to_string(p->P.n_in) + " inputs, its critic " +
                                         std::to_string(p->P.n_layers[1] ? p->P.n_in_vf : 0));
    if (p->w.device != l->w.device) return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_create: lstm and policy live on different devices");
    if (T_max < 1 || Bm_max < 1) return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_create: T_max and Bm_max must be >= 1");
    const size_t NT = ((size_t)Bm_max + WGP_TILE - 1) / WGP_TILE, n_max = (size_t)T_max * Bm_max, npad = (size_t)T_max * NT * WGP_TILE;
    const size_t H = L.H, nets = L.n_nets, n_out = p->P.n_out;
    const size_t f_gates = nets * npad * 4 * H, f_c = nets * npad * H, f_h = nets * n_max * H, f_dh = 2 * n_max * H, f_rows = n_max * (n_out + 3);
    if ((size_t)T_max > WGLP_ROWS_MAX || (size_t)Bm_max > WGLP_ROWS_MAX || n_max > WGLP_ROWS_MAX ||
        sizeof(float) * (f_gates + f_c + f_h + f_dh + f_rows) > WGLP_STASH_BYTES)
        return wg_fail(WG_ERR_UNSUPPORTED, "wg_lstm_ppo_create: T_max = " + std::to_string(T_max) + " steps of Bm_max = " + std::to_string(Bm_max) +
                                             " envs need a stash of " + std::to_string(sizeof(float) * (f_gates + f_c + f_h + f_dh + f_rows)) +
                                             " bytes; the limits are " + std::to_string(WGLP_STASH_BYTES) + " bytes and " +
                                             std::to_string(WGLP_ROWS_MAX) + " rows per minibatch");
    wg_lstm_ppo_s* o = new (std::nothrow) wg_lstm_ppo_s();
    if (!o) return wg_fail(WG_ERR_NOMEM, "wg_lstm_ppo_create: out of host memory");
    o->lstm = l; o->pol = p;
    o->mem.device = o->adam.device = l->w.device; o->T_max = T_max; o->Bm_max = Bm_max; o->NT_max = (int)NT;
    o->n_lstm = L.n_flat;
    const char* const who = "wg_lstm_ppo_create";
    if (int rc = wg_ppo_grad_init_(&o->mem, &o->heads, p, who)) {
        wg_lstm_ppo_destroy(o);
        return rc;
    }
    o->nksT = wg_tile_nks(4 * L.H);
    o->whhT_net = wg_tile_wsize(L.nub, o->nksT);
    o->whhT_all = o->whhT_net * L.n_nets + WGP_SLACK;
    const uint32_t n_flat = L.n_flat + p->P.n_flat;
    int rc = wg_adam_alloc_(&o->mem, &o->adam, n_flat, who);
    const struct { float** out; size_t n; } bufs[] = {{&o->grad, n_flat}, {&o->stats, WGT_NSTAT}, {&o->gates, f_gates}, {&o->c, f_c}, {&o->h, f_h},
                                                      {&o->dh, f_dh}, {&o->rows, f_rows}, {&o->whhT, o->whhT_all},
                                                      {&o->wpart, (size_t)WGLP_SPLIT * o->n_lstm}};
    for (const auto& b : bufs)
        if (!rc) rc = o->mem.alloc(who, b.out, b.n, false);
    if (rc) {
        wg_lstm_ppo_destroy(o);
        return rc;
    }
    *out = o;
    return 0;
}

extern "C" int wg_lstm_ppo_destroy(wg_lstm_ppo o) {
    if (!o) return 0;
    o->mem.release();
    delete o;
    return 0;
}

extern "C" int wg_lstm_ppo_n_params(wg_lstm_ppo o, size_t* n) {
    if (!o || !n) return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_n_params: null argument");
    *n = o->adam.n_flat;
    return 0;
}

extern "C" int wg_lstm_ppo_get_state(wg_lstm_ppo o, float* mv_host, size_t n, uint64_t* step) {
    return wg_adam_get_state_(o ? &o->adam : nullptr, "wg_lstm_ppo_get_state", mv_host, n, step);
}

extern "C" int wg_lstm_ppo_set_state(wg_lstm_ppo o, const float* mv_host, size_t n, uint64_t step) {
    return wg_adam_set_state_(o ? &o->adam : nullptr, "wg_lstm_ppo_set_state", mv_host, n, step);
}

// what grad and update check of a batch and the hyper-parameters; `who` names the entry
// (the sizes: what the PPO and the supervised entries check alike)
static int lp_check_sizes(const std::string& who, wg_lstm_ppo o, int T, int B, int n_envs) {
    if (T < 1 || B < 1) return wg_fail(WG_ERR_INVALID, who + ": T and B must be >= 1");
    if (n_envs < 1) return wg_fail(WG_ERR_INVALID, who + ": a minibatch has at least one env");
    if (T > o->T_max)
        return wg_fail(WG_ERR_UNSUPPORTED, who + ": T = " + std::to_string(T) + " > the T_max = " + std::to_string(o->T_max) + " the handle was created for");
    if (n_envs > o->Bm_max)
        return wg_fail(WG_ERR_UNSUPPORTED, who + ": " + std::to_string(n_envs) + " envs in a minibatch > the Bm_max = " + std::to_string(o->Bm_max) +
                                             " the handle was created for");
    if ((long long)T * B > 0x7fffffffLL) return wg_fail(WG_ERR_UNSUPPORTED, who + ": more than 2^31 rows T * B");
    return 0;
}

static int lp_check(const std::string& who, wg_lstm_ppo o, const wg_lstm_ppo_batch* b, const wg_ppo_hyper* hp, int n_envs) {
    if (!b->obs || !b->raw || !b->logp || !b->advantage || !b->returns || !b->episode_start || !b->lstm_state0)
        return wg_fail(WG_ERR_INVALID, who + ": a batch pointer is null");
    if (int rc = lp_check_sizes(who, o, b->T, b->B, n_envs)) return rc;
    if (!(hp->clip_range >= 0.0f)) return wg_fail(WG_ERR_INVALID, who + ": clip_range < 0");
    return 0;
}

// the launches of one gradient, no argument checks
static int lp_grad(wg_lstm_ppo o, const float* params_dev, const wg_lstm_ppo_batch* b, const int32_t* envs_dev, int Bm, const wg_ppo_hyper* hp,
                   float* grad_out, float* stats_out, hipStream_t st) {
    const WgLstmP& L = o->lstm->P;
    const int T = b->T, n = T * Bm, n_out = o->pol->P.n_out;
    const WgLstmStash s = wglp_stash(o);
    WgLstmSeq q = s.q;
    q.obs = b->obs; q.start = b->episode_start; q.state0 = b->lstm_state0; q.envs = envs_dev;
    q.T = T; q.B = b->B; q.Bm = Bm; q.NT = (Bm + WGP_TILE - 1) / WGP_TILE;
    hipLaunchKernelGGL(k_lstm_ppo_pack, dim3((o->whhT_all + 255) / 256), dim3(256), 0, st, L, params_dev, o->whhT, o->whhT_net, o->whhT_all,
                       (uint32_t)o->nksT);
    hipLaunchKernelGGL(k_lstm_ppo_gather, dim3((n + 255) / 256), dim3(256), 0, st, q, n_out, b->raw, b->logp, b->advantage, b->returns, s.raw, s.logp,
                       s.adv, s.ret);
    hipLaunchKernelGGL(k_lstm_seq_fwd, dim3(q.NT, L.n_nets), dim3(WGP_WAVES * 64), 0, st, L, o->lstm->w.packed, q);
    WG_HIPCHK(hipGetLastError());
    if (int rc = wg_ppo_heads_grad_(&o->heads, params_dev + o->n_lstm, s.h[0], s.h[1], s.raw, s.logp, s.adv, s.ret, n, hp, s.dh[0], s.dh[1],
                                    grad_out + o->n_lstm, stats_out ? stats_out : o->stats, (void*)st))
        return rc;
    hipLaunchKernelGGL(k_lstm_seq_bwd, dim3(q.NT, L.n_nets), dim3(WGP_WAVES * 64), 0, st, L, q);
    const int nblk = T * q.NT, S = nblk < WGLP_SPLIT ? nblk : WGLP_SPLIT;
    hipLaunchKernelGGL(k_lstm_wgrad, dim3((L.K + 31) / 32, (4 * L.H + WGLP_WI - 1) / WGLP_WI, L.n_nets * S), dim3(WGP_WAVES * 64), 0, st, L, q,
                       o->wpart, S);
    hipLaunchKernelGGL(k_lstm_wgrad_reduce, dim3((o->n_lstm + 255) / 256), dim3(256), 0, st, o->wpart, o->n_lstm, S, grad_out);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

static int lp_apply(wg_lstm_ppo o, float* params_dev, const float* grad_dev, float lr, float max_grad_norm, hipStream_t st) {
    if (int rc = wg_adam_apply_(&o->adam, params_dev, grad_dev, lr, max_grad_norm, st)) return rc;
    if (int rc = wg_lstm_set_params(o->lstm, params_dev, o->n_lstm, 1, (void*)st)) return rc;
    return wg_policy_set_params(o->pol, params_dev + o->n_lstm, o->adam.n_flat - o->n_lstm, 1, (void*)st);
}

// ... of minibatch mb of an update under the handle's KL rule (wg_adam_apply_kl_)
static int lp_apply_kl(wg_lstm_ppo o, float* params_dev, const float* grad_dev, const float* stats_dev, int mb, int last, float max_grad_norm,
                       hipStream_t st) {
    if (int rc = wg_adam_apply_kl_(&o->adam, params_dev, grad_dev, stats_dev, mb, last, max_grad_norm, st)) return rc;
    if (int rc = wg_lstm_set_params(o->lstm, params_dev, o->n_lstm, 1, (void*)st)) return rc;
    return wg_policy_set_params(o->pol, params_dev + o->n_lstm, o->adam.n_flat - o->n_lstm, 1, (void*)st);
}

extern "C" int wg_lstm_ppo_set_kl_lr(wg_lstm_ppo o, const wg_kl_lr* rule, float* lr_dev) {
    return wg_adam_set_kl_lr_(o ? &o->mem : nullptr, o ? &o->adam : nullptr, "wg_lstm_ppo_set_kl_lr", rule, lr_dev);
}

extern "C" int wg_lstm_ppo_grad(wg_lstm_ppo o, const float* params_dev, const wg_lstm_ppo_batch* b, const int32_t* envs_dev, int n_envs,
                                const wg_ppo_hyper* hp, float* grad_out, wg_ppo_stats* stats_out, void* stream) {
    if (!o || !params_dev || !b || !envs_dev || !hp || !grad_out) return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_grad: null argument");
    if (int rc = lp_check("wg_lstm_ppo_grad", o, b, hp, n_envs)) return rc;
    if (int rc = wg_use_device(o->adam.device)) return rc;
    return lp_grad(o, params_dev, b, envs_dev, n_envs, hp, grad_out, (float*)stats_out, (hipStream_t)stream);
}

extern "C" int wg_lstm_ppo_apply(wg_lstm_ppo o, float* params_dev, const float* grad_dev, float lr, float max_grad_norm, void* stream) {
    if (!o || !params_dev || !grad_dev) return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_apply: null argument");
    if (!(max_grad_norm > 0.0f)) return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_apply: max_grad_norm must be > 0");
    if (int rc = wg_use_device(o->adam.device)) return rc;
    return lp_apply(o, params_dev, grad_dev, lr, max_grad_norm, (hipStream_t)stream);
}

extern "C" int wg_lstm_ppo_update(wg_lstm_ppo o, float* params_dev, const wg_lstm_ppo_batch* b, const int32_t* perm_dev, int n_epochs,
                                  int envs_per_batch, const wg_ppo_hyper* hp, float lr, float max_grad_norm, wg_ppo_stats* stats_out,
                                  void* stream) {
    if (!o || !params_dev || !b || !perm_dev || !hp) return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_update: null argument");
    if (n_epochs < 1) return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_update: n_epochs must be >= 1");
    if (int rc = lp_check("wg_lstm_ppo_update", o, b, hp, envs_per_batch)) return rc;
    if (!(max_grad_norm > 0.0f)) return wg_fail(WG_ERR_INVALID, "wg_lstm_ppo_update: max_grad_norm must be > 0");
    if (int rc = wg_use_device(o->adam.device)) return rc;
    const bool kl = o->adam.lr_dev != nullptr;                  // wg_lstm_ppo_set_kl_lr: the rate is the handle's device word, `lr` is ignored
    const int n_all = n_epochs * wg_n_minibatches(b->B, envs_per_batch);
    return wg_each_minibatch(b->B, n_epochs, envs_per_batch, [&](int mb, int64_t off, int Bm) {
        float* so = stats_out ? (float*)(stats_out + mb) : nullptr;
        if (int rc = lp_grad(o, params_dev, b, perm_dev + off, Bm, hp, o->grad, so, (hipStream_t)stream)) return rc;
        if (kl) return lp_apply_kl(o, params_dev, o->grad, so ? so : o->stats, mb, mb == n_all - 1, max_grad_norm, (hipStream_t)stream);
        return lp_apply(o, params_dev, o->grad, lr, max_grad_norm, (hipStream_t)stream);
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// behaviour cloning into a recurrent policy (windgym_hip.h: wg_lstm_bc_*): the supervised head on the wg_lstm_ppo handle — its
// stash, its Adam, wg_lstm_ppo_apply.  THE RULE is the one at the head of this file with wg_bc_grad's loss in place of k_ppo_grad's
// (k_bc_grad_dh) and `target` in place of raw / logp / advantage.  WITHOUT RETURNS the critic gets no gradient, so nothing of its
// side runs: the heads launch the actor's workgroups alone (dh[1] is not written), and with two LSTMs the three sequence kernels run
// on grid nets = 1 — the actor's LSTM is net 0 and leads the flat vector — while k_lstm_wgrad_reduce_live writes the critic LSTM's
// block as 0.0f.  With a shared LSTM the one net runs with dh_t = the actor head's term alone (q.shared = 0: lstm_seq_bwd then does
// not read dh[1]).  So no dh[1] row, wpart column or spart slot that an earlier call left on the handle is ever read.
// ---------------------------------------------------------------------------------------------------------------------
static int lb_check(const std::string& who, wg_lstm_ppo o, const wg_lstm_bc_batch* b, const wg_bc_hyper* hp, int n_envs) {
    const char* null_is = !b->obs ? "obs" : !b->target ? "target" : !b->episode_start ? "episode_start" : !b->lstm_state0 ? "lstm_state0" : nullptr;
    if (null_is) return wg_fail(WG_ERR_INVALID, who + ": the batch's " + null_is + " is null (only returns may be)");
    if (int rc = lp_check_sizes(who, o, b->T, b->B, n_envs)) return rc;
    if (hp->loss != WG_BC_MSE && hp->loss != WG_BC_NLL)
        return wg_fail(WG_ERR_INVALID, who + ": loss must be WG_BC_MSE or WG_BC_NLL, got " + std::to_string(hp->loss));
    if (!(hp->vf_coef >= 0.0f) || !(hp->ent_coef >= 0.0f)) return wg_fail(WG_ERR_INVALID, who + ": vf_coef and ent_coef must be >= 0");
    return 0;
}

// the launches of one supervised gradient, no argument checks
static int lb_grad(wg_lstm_ppo o, const float* params_dev, const wg_lstm_bc_batch* b, const int32_t* envs_dev, int Bm, const wg_bc_hyper* hp,
                   float* grad_out, float* stats_out, hipStream_t st) {
    const WgLstmP& L = o->lstm->P;
    const int T = b->T, n = T * Bm, n_out = o->pol->P.n_out;
    const bool has_ret = b->returns != nullptr;
    const int nets = has_ret ? L.n_nets : 1;               // the nets that run: without returns the actor's (net 0) alone
    const WgLstmStash s = wglp_stash(o);
    WgLstmSeq q = s.q;
    q.obs = b->obs; q.start = b->episode_start; q.state0 = b->lstm_state0; q.envs = envs_dev;
    q.T = T; q.B = b->B; q.Bm = Bm; q.NT = (Bm + WGP_TILE - 1) / WGP_TILE;
    if (!has_ret) q.shared = 0;                            // dh_t is the actor head's term alone
    // (the pack stays whole, the skipped critic net's W_hh^T block included, on purpose: one element-wise launch over at most 2 x 4H x H
    // floats, and what lies behind the actor's block is then this call's packed data, as the layout of wg_lstm_ppo.h says — not an
    // earlier call's, which a cut-off pack would leave where the GEMM loop's last prefetch reads one group past its tile: wg_tile.h,
    // invariant 3)
    hipLaunchKernelGGL(k_lstm_ppo_pack, dim3((o->whhT_all + 255) / 256), dim3(256), 0, st, L, params_dev, o->whhT, o->whhT_net, o->whhT_all,
                       (uint32_t)o->nksT);
    hipLaunchKernelGGL(k_lstm_bc_gather, dim3((n + 255) / 256), dim3(256), 0, st, q, n_out, b->target, b->returns, s.raw, s.ret);
    hipLaunchKernelGGL(k_lstm_seq_fwd, dim3(q.NT, nets), dim3(WGP_WAVES * 64), 0, st, L, o->lstm->w.packed, q);
    WG_HIPCHK(hipGetLastError());
    // (without returns the critic's head is not launched: the h plane it would read may hold an earlier call's rows)
    if (int rc = wg_ppo_heads_bc_grad_(&o->heads, params_dev + o->n_lstm, s.h[0], s.h[1], s.raw, has_ret ? s.ret : nullptr, n, hp, s.dh[0], s.dh[1],
                                       grad_out + o->n_lstm, stats_out ? stats_out : o->stats, (void*)st))
        return rc;
    hipLaunchKernelGGL(k_lstm_seq_bwd, dim3(q.NT, nets), dim3(WGP_WAVES * 64), 0, st, L, q);
    const int nblk = T * q.NT, S = nblk < WGLP_SPLIT ? nblk : WGLP_SPLIT;
    hipLaunchKernelGGL(k_lstm_wgrad, dim3((L.K + 31) / 32, (4 * L.H + WGLP_WI - 1) / WGLP_WI, nets * S), dim3(WGP_WAVES * 64), 0, st, L, q, o->wpart,
                       S);
    const uint32_t n_live = nets == L.n_nets ? o->n_lstm : L.net[1].wih_flat;
    hipLaunchKernelGGL(k_lstm_wgrad_reduce_live, dim3((o->n_lstm + 255) / 256), dim3(256), 0, st, o->wpart, o->n_lstm, n_live, S, grad_out);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_lstm_bc_grad(wg_lstm_ppo o, const float* params_dev, const wg_lstm_bc_batch* b, const int32_t* envs_dev, int n_envs,
                               const wg_bc_hyper* hp, float* grad_out, wg_bc_stats* stats_out, void* stream) {
    if (!o || !params_dev || !b || !envs_dev || !hp || !grad_out) return wg_fail(WG_ERR_INVALID, "wg_lstm_bc_grad: null argument");
    if (int rc = lb_check("wg_lstm_bc_grad", o, b, hp, n_envs)) return rc;
    if (int rc = wg_use_device(o->adam.device)) return rc;
    return lb_grad(o, params_dev, b, envs_dev, n_envs, hp, grad_out, (float*)stats_out, (hipStream_t)stream);
}

extern "C" int wg_lstm_bc_update(wg_lstm_ppo o, float* params_dev, const wg_lstm_bc_batch* b, const int32_t* perm_dev, int n_epochs,
                                 int envs_per_batch, const wg_bc_hyper* hp, float lr, float max_grad_norm, wg_bc_stats* stats_out,
                                 void* stream) {
    if (!o || !params_dev || !b || !perm_dev || !hp) return wg_fail(WG_ERR_INVALID, "wg_lstm_bc_update: null argument");
    if (n_epochs < 1) return wg_fail(WG_ERR_INVALID, "wg_lstm_bc_update: n_epochs must be >= 1");
    if (int rc = lb_check("wg_lstm_bc_update", o, b, hp, envs_per_batch)) return rc;
    if (!(max_grad_norm > 0.0f)) return wg_fail(WG_ERR_INVALID, "wg_lstm_bc_update: max_grad_norm must be > 0");
    if (int rc = wg_use_device(o->adam.device)) return rc;
    return wg_each_minibatch(b->B, n_epochs, envs_per_batch, [&](int mb, int64_t off, int Bm) {
        float* so = stats_out ? (float*)(stats_out + mb) : nullptr;
        if (int rc = lb_grad(o, params_dev, b, perm_dev + off, Bm, hp, o->grad, so, (hipStream_t)stream)) return rc;
        return lp_apply(o, params_dev, o->grad, lr, max_grad_norm, (hipStream_t)stream);
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// populations of recurrent policies (windgym_hip.h: wg_lstm_pop_*; the step and the heads' slot table: wg_lstm.hip)
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int wg_lstm_pop_create(const wg_lstm* lstms, const wg_policy* heads, const wg_lstm_ppo* opts, int P, wg_lstm_pop* out) {
    if (!lstms || !heads || !out) return wg_fail(WG_ERR_INVALID, "wg_lstm_pop_create: null argument");
    *out = nullptr;
    if (int rc = wg_pop_count("wg_lstm_pop_create", P)) return rc;
    for (int m = 0; m < P; ++m) {
        const std::string who = "wg_lstm_pop_create: member " + std::to_string(m);
        if (!lstms[m] || !heads[m]) return wg_fail(WG_ERR_INVALID, who + " is null");
        const WgLstmP &L0 = lstms[0]->P, &L = lstms[m]->P;
        const WgPolicyP& Q = heads[m]->P;
        if (Q.n_in != L.H || Q.n_layers[1] == 0 || Q.n_in_vf != L.H)
            return wg_fail(WG_ERR_INVALID, who + ": its head must map the LSTM's hidden size (" + std::to_string(L.H) + ") with its critic on the same width; it maps " +
                                             std::to_string(Q.n_in) + " inputs, its critic " + std::to_string(Q.n_layers[1] ? Q.n_in_vf : 0));
        if (L.n_in != L0.n_in || L.H != L0.H || L.n_nets != L0.n_nets)
            return wg_fail(WG_ERR_INVALID, who + "'s LSTM maps " + std::to_string(L.n_in) + " -> " + std::to_string(L.H) + " with " + std::to_string(L.n_nets) +
                                             " net(s), member 0's " + std::to_string(L0.n_in) + " -> " + std::to_string(L0.H) + " with " +
                                             std::to_string(L0.n_nets) + ": the members of a population share one n_in, hidden size and number of nets");
        if (!wgp_same_arch(heads[0]->P, Q, false))      // (the widths: both are H, above)
            return wg_fail(WG_ERR_INVALID, who + "'s head has another architecture than member 0's: the members of a population share one");
        if (int rc = wg_pop_same_device(who, lstms[0]->w.device, " (LSTM / head)", lstms[m]->w.device, heads[m]->w.device)) return rc;
        if (int rc = wg_pop_given_twice(who, m, " holds the same handle as member ", lstms, heads)) return rc;
        if (opts) {
            if (!opts[m]) return wg_fail(WG_ERR_INVALID, who + ": its wg_lstm_ppo is null (opts = NULL makes a population that only acts)");
            if (opts[m]->lstm != lstms[m] || opts[m]->pol != heads[m])
                return wg_fail(WG_ERR_INVALID, who + ": opts[" + std::to_string(m) + "] was created for another pair");
        }
    }
    wg_lstm_pop_s* q = new (std::nothrow) wg_lstm_pop_s();
    if (!q) return wg_fail(WG_ERR_NOMEM, "wg_lstm_pop_create: out of host memory");
    q->P = q->heads.P = P;
    q->device = q->heads.device = lstms[0]->w.device;
    for (int m = 0; m < P; ++m) { q->lstm[m] = lstms[m]; q->heads.pol[m] = heads[m]; q->opt[m] = opts ? opts[m] : nullptr; }
    q->mem.device = q->device;
    const char* const who = "wg_lstm_pop_create";
    int rc = q->mem.alloc(who, &q->heads.slots_dev, WGP_POP_SLOTS, false);
    if (!rc) rc = q->mem.alloc_bytes(who, &q->seq_dev, sizeof(WgLstmPopMember) * WGP_POP_MAX, false);
    if (!rc) rc = q->mem.alloc_bytes(who, &q->upd_dev, sizeof(WgPopMember) * 2 * WGP_POP_MAX, false);
    if (!rc) rc = q->mem.alloc_bytes(who, &q->rows_dev, sizeof(WgPopHeadRows) * WGP_POP_MAX, false);
    if (rc) {
        wg_lstm_pop_destroy(q);
        return rc;
    }
    *out = q;
    return 0;
}

extern "C" int wg_lstm_pop_destroy(wg_lstm_pop q) {
    if (!q) return 0;
    q->mem.release();
    delete q;
    return 0;
}

extern "C" int wg_lstm_pop_update(wg_lstm_pop q, float* const* params_dev, const wg_lstm_ppo_batch* b, const int32_t* perm_dev, int n_epochs,
                                  int envs_per_batch, const wg_ppo_hyper* hp, const float* lr, const float* max_grad_norm,
                                  wg_ppo_stats* stats_out, void* stream) {
    if (!q || !params_dev || !b || !perm_dev || !hp || !lr || !max_grad_norm) return wg_fail(WG_ERR_INVALID, "wg_lstm_pop_update: null argument");
    const int P = q->P;
    if (int rc = wg_pop_update_check("wg_lstm_pop_update", q->opt[0], n_epochs >= 1, "n_epochs", P, params_dev, max_grad_norm)) return rc;
    for (int m = 0; m < P; ++m)
        if (int rc = lp_check("wg_lstm_pop_update: member " + std::to_string(m), q->opt[m], b, &hp[m], envs_per_batch)) return rc;
    if (int rc = wg_pop_shares("wg_lstm_pop_update", P, b->B, "envs", "B = ", " does")) return rc;
    if (int rc = wg_use_device(q->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const WgLstmP& L = q->lstm[0]->P;
    const WgPpoGrad* g0 = &q->opt[0]->heads;
    const WgPolicyP& PP = g0->pol->P;
    const int T = b->T, sB = b->B / P, n_out = PP.n_out, n_mb = wg_n_minibatches(sB, envs_per_batch);
    const size_t H = L.H;
    // the three member tables: the sequence kernels', and for the heads and Adam two views of the member as the plain population's
    // kernels see one — the MLP part of its vectors with the heads' scratch, and its whole flat vector
    WgLstmPopMember seq[WGP_POP_MAX] = {};
    WgPopMember upd[2 * WGP_POP_MAX] = {};
    WgPopHeadRows rows[WGP_POP_MAX] = {};
    WgAdam* adam[WGP_POP_MAX];
    for (int m = 0; m < P; ++m) adam[m] = &q->opt[m]->adam;
    int kl = 0;                                                 // the members' rates are their device words (every member or none), `lr` is ignored
    if (int rc = wg_pop_kl_lr_("wg_lstm_pop_update", P, adam, &kl)) return rc;
    bool any_norm = false;
    for (int m = 0; m < P; ++m) {
        wg_lstm_ppo_s* o = q->opt[m];
        const WgLstmStash s = wglp_stash(o);
        WgLstmPopMember& S = seq[m];
        S.q = s.q;
        S.q.obs = b->obs; S.q.start = b->episode_start; S.q.envs = perm_dev + (size_t)m * n_epochs * sB;
        S.q.state0 = b->lstm_state0 + (size_t)m * L.n_nets * 2 * sB * H - (size_t)m * sB * H;
        S.q.T = T; S.q.B = b->B; S.q.sB = sB;
        S.packed = o->lstm->w.packed; S.params = params_dev[m]; S.whhT = o->whhT; S.wpart = o->wpart; S.grad = o->grad;
        S.raw = s.raw; S.logp = s.logp; S.adv = s.adv; S.ret = s.ret;
        rows[m] = {{s.h[0], s.h[1]}, s.raw, s.logp, s.adv, s.ret, {s.dh[0], s.dh[1]}};
        WgPopMember& M = upd[m];
        M.packed = o->pol->w.packed; M.params = params_dev[m] + o->n_lstm; M.grad = o->grad + o->n_lstm;
        M.part = o->heads.part; M.spart = o->heads.spart; M.advstat = o->heads.advstat;
        any_norm = wgt_pop_member(M, hp, stats_out, m, n_epochs, n_mb, o->stats) || any_norm;
        WgPopMember& A = upd[WGP_POP_MAX + m];
        A.params = params_dev[m]; A.grad = o->grad; A.m = o->adam.m; A.v = o->adam.v; A.blocksq = o->adam.blocksq; A.max_norm = max_grad_norm[m];
        A.stats = M.stats; A.stats_step = M.stats_step;           // (the record the heads' reduce writes: what a KL-adaptive rate reads)
        wgt_pop_member_kl(A, o->adam);
    }
    const WgLstmPopMember* mt = (const WgLstmPopMember*)q->seq_dev;
    const WgPopMember* ht = (const WgPopMember*)q->upd_dev;
    const WgPopHeadRows* rt = (const WgPopHeadRows*)q->rows_dev;
    if (int rc = wg_pop_store_(q->seq_dev, seq, sizeof(WgLstmPopMember) * P, stream)) return rc;
    if (int rc = wg_pop_store_(q->upd_dev, upd, sizeof(upd), stream)) return rc;
    if (int rc = wg_pop_store_(q->rows_dev, rows, sizeof(WgPopHeadRows) * P, stream)) return rc;
    const wg_lstm_ppo_s* o0 = q->opt[0];
    // every member has the architecture of member 0: per minibatch the launches of lp_grad and lp_apply, each with the member axis
    return wg_each_minibatch(sB, n_epochs, envs_per_batch, [&](int mb, int64_t off, int Bm) {
        const int n = T * Bm, NT = (Bm + WGP_TILE - 1) / WGP_TILE;
        hipLaunchKernelGGL(k_lstm_ppo_pack_pop, dim3((o0->whhT_all + 255) / 256, P), dim3(256), 0, st, L, mt, o0->whhT_net, o0->whhT_all,
                           (uint32_t)o0->nksT);
        hipLaunchKernelGGL(k_lstm_ppo_gather_pop, dim3((n + 255) / 256, P), dim3(256), 0, st, mt, off, Bm, NT, n_out, b->raw, b->logp,
                           b->advantage, b->returns);
        hipLaunchKernelGGL(k_lstm_seq_fwd_pop, dim3(NT, L.n_nets, P), dim3(WGP_WAVES * 64), 0, st, L, mt, off, Bm, NT);
        WG_HIPCHK(hipGetLastError());
        if (int rc = wg_ppo_heads_grad_pop_(g0, ht, rt, P, any_norm, n, mb, stream)) return rc;
        hipLaunchKernelGGL(k_lstm_seq_bwd_pop, dim3(NT, L.n_nets, P), dim3(WGP_WAVES * 64), 0, st, L, mt, off, Bm, NT);
        const int nblk = T * NT, S = nblk < WGLP_SPLIT ? nblk : WGLP_SPLIT;
        hipLaunchKernelGGL(k_lstm_wgrad_pop, dim3((L.K + 31) / 32, (4 * L.H + WGLP_WI - 1) / WGLP_WI, P * L.n_nets * S), dim3(WGP_WAVES * 64), 0,
                           st, L, mt, off, Bm, NT, S);
        hipLaunchKernelGGL(k_lstm_wgrad_reduce_pop, dim3((o0->n_lstm + 255) / 256, P), dim3(256), 0, st, mt, o0->n_lstm, S);
        WG_HIPCHK(hipGetLastError());
        if (int rc = kl ? wg_adam_apply_kl_pop_(ht + WGP_POP_MAX, P, adam, mb, mb == n_epochs * n_mb - 1, stream)
                        : wg_adam_apply_pop_(ht + WGP_POP_MAX, P, adam, lr, stream))
            return rc;
        if (int rc = wg_lstm_pack_pop_(q, params_dev, stream)) return rc;
        wg_policy_pack_pop_(&PP, ht, P, stream);
        WG_HIPCHK(hipGetLastError());
        return 0;
    });
}
