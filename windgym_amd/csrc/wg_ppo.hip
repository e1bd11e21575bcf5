// wg_ppo.hip — training on the device: what `PPO("MlpPolicy", env).learn(...)` of stable-baselines3 does between two rollouts
// (examples/longer_steps_example.py:212-240, examples/curriculum.py:544-560), for the MlpPolicy of wg_policy.hip.
//
//   k_gae          advantages and returns of a [T, B, A] rollout (wg_rollout's recurrence), one thread per agent row.
//   k_ppo_advstat  mean and unbiased std of a minibatch's advantages, ONE workgroup, fixed-order sums.
//   k_ppo_grad     one minibatch: gather, forward of actor / critic, PPO loss, backward, per-workgroup gradient partials.
//                  A minibatch entry is an AGENT row; with a centralised critic (wg_ppo_batch_shared: agents > 1 or a critic
//                  of another input width) the critic gathers the entry's ENV row = entry / agents from a stream of its own, and
//                  advantage / returns are indexed by env row.  agents = 1 on one stream is the plain batch.
//   k_ppo_reduce   partials -> flat gradient + statistics record, summed in workgroup order.
//   k_bc_grad      k_ppo_grad with the supervised loss head (behaviour cloning: MSE or -logp of the expert's actions) in place of
//                  the clipped surrogate — the same forward, dW and dX, instantiated from the same body; k_bc_reduce is its reduce.
//                  k_bc_grad_dh: the same with the gradients of the input rows, for the LSTMs of a recurrent policy.
//   k_ppo_sumsq / k_ppo_adam   global L2 norm, clipping, Adam on the caller's flat parameters in place.
//
// k_ppo_grad: a workgroup of 4 waves owns ONE net (blockIdx.y: actor / critic — the two gradients share nothing but the
// rows) and walks its tiles of R rows (wg_ppo.h).  All products run on v_mfma_f32_32x32x2_f32 with the tile's rows as the
// 32 columns (forward, dX) or as the summation index (dW):
//     forward   Z[i][row]  = b[i] + sum_k W[i][k] X[k][row]      A = k_policy's packed weights, B = X from LDS — the same
//                                                                k-ordered fmaf chain as k_policy: bit-identical mean / V;
//     dW        dW[i][k]  += sum_row dZ[i][row] X[k][row]        A = dZ, B = X, both from LDS; the accumulator starts from the
//                                                                workgroup's own partial (no atomics: nobody else writes it);
//     dX        dY[k][row] = sum_i W[i][k] dZ[i][row]            A = the caller's flat W[i][.] rows (coalesced), B = dZ from LDS.
// Activations of every layer stay in LDS between forward and backward; the first layer streams the observations through LDS
// in chunks of 256 inputs, once forward and once more for dW.  fp32 throughout.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>

#include "../../include/windgym_hip.h"
#include "wg_ppo.h"
#include "wg_host.h"

#define WGT_HALF_LOG_2PI 0.91893853320467274f

// ---------------------------------------------------------------------------------------------------------------------
// GAE
// ---------------------------------------------------------------------------------------------------------------------
// One thread per AGENT row of a [T, B, A] rollout whose reward and truncation flag belong to the env (a farm's turbines share
// the farm reward; A = 1: one row per env, wg_gae): consecutive threads walk consecutive agent rows, the two [B] arrays are
// read once per thread (the A threads of an env fetch the same word: one transaction).
__device__ __forceinline__ void gae_row(const int T, const int B, const int A, const int r, const float* __restrict__ reward,
                                        const float* __restrict__ value, const float* __restrict__ final_value,
                                        const uint8_t* __restrict__ truncated, const float gamma, const float lambda,
                                        float* __restrict__ adv, float* __restrict__ ret) {
    const int R = B * A;
    const int b = r / A;
    float a = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        const size_t o = (size_t)t * R + r, e = (size_t)t * B + b;
        const float v = value[o];
        const float delta = reward[e] + gamma * final_value[o] - v;
        a = delta + gamma * lambda * (truncated[e] ? 0.0f : 1.0f) * a;
        adv[o] = a;
        ret[o] = a + v;
    }
}

__global__ void k_gae(const int T, const int B, const int A, const float* __restrict__ reward, const float* __restrict__ value,
                      const float* __restrict__ final_value, const uint8_t* __restrict__ truncated, const float gamma,
                      const float lambda, float* __restrict__ adv, float* __restrict__ ret) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B * A) return;
    gae_row(T, B, A, r, reward, value, final_value, truncated, gamma, lambda, adv, ret);
}

// a population's [T, B]: column r belongs to member r / Bm and runs the recurrence with that member's gamma and lambda
struct WgPopGae { float gamma[WGP_POP_MAX], lambda[WGP_POP_MAX]; };
__global__ void k_gae_pop(const int T, const int B, const int Bm, const float* __restrict__ reward, const float* __restrict__ value,
                          const float* __restrict__ final_value, const uint8_t* __restrict__ truncated, const WgPopGae hy,
                          float* __restrict__ adv, float* __restrict__ ret) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B) return;
    const int m = r / Bm;
    gae_row(T, B, 1, r, reward, value, final_value, truncated, hy.gamma[m], hy.lambda[m], adv, ret);
}

// ---------------------------------------------------------------------------------------------------------------------
// fixed-order block reductions (tree over threadIdx, the same shape on every device)
// ---------------------------------------------------------------------------------------------------------------------
template <int NT>
__device__ inline float block_sum(float v, float* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    return sh[0];
}

__device__ inline int ppo_row(const int32_t* index, int64_t first, int n, int64_t n_total, int i) {
    if (i >= n) return -1;
    const int64_t id = index ? (int64_t)index[i] : first + i;
    return (id < 0 || id >= n_total) ? -1 : (int)id;
}

// advstat[0] = mean, advstat[1] = unbiased std (torch.std) of the minibatch's advantages; entry id (an agent row) carries the
// advantage of its env row id / agents (agents = 1: its own)
__device__ __forceinline__ void ppo_advstat(const float* __restrict__ adv, const int32_t* __restrict__ index, const int64_t first,
                                            const int n, const int64_t n_total, const int agents, float* __restrict__ advstat) {
    __shared__ float sh[1024];
    float s = 0.0f;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int id = ppo_row(index, first, n, n_total, i);
        if (id >= 0) s += adv[id / agents];
    }
    const float mean = block_sum<1024>(s, sh) / (float)n;
    float q = 0.0f;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int id = ppo_row(index, first, n, n_total, i);
        if (id >= 0) { const float d = adv[id / agents] - mean; q += d * d; }
    }
    const float var = block_sum<1024>(q, sh) / (float)(n - 1);
    if (threadIdx.x == 0) { advstat[0] = mean; advstat[1] = sqrtf(var); }
}

__global__ __launch_bounds__(1024) void k_ppo_advstat(const float* __restrict__ adv, const int32_t* __restrict__ index,
                                                      const int64_t first, const int n, const int64_t n_total, const int agents,
                                                      float* __restrict__ advstat) {
    ppo_advstat(adv, index, first, n, n_total, agents, advstat);
}

// The population's kernels (k_*_pop): one more grid axis = member, whose row of the member table (wg_policy.h: WgPopMember) gives
// the pointers and hyper-parameters that the single-policy kernel takes as arguments; the arithmetic is the shared body's.  The
// minibatch of member m is perm[off .. off + n) of ITS permutations; `mb` is the minibatch's ordinal e * n_mb + k.
__global__ __launch_bounds__(1024) void k_ppo_advstat_pop(const WgPopMember* __restrict__ mt, const float* __restrict__ adv,
                                                          const int64_t off, const int n, const int64_t n_total) {
    const WgPopMember* __restrict__ M = mt + blockIdx.x;
    if (!(M->normalize && n > 1)) return;
    ppo_advstat(adv, M->perm + off, 0, n, n_total, 1, M->advstat);
}

// ---------------------------------------------------------------------------------------------------------------------
// k_ppo_grad
// ---------------------------------------------------------------------------------------------------------------------
struct WgPpoArgs {
    const float* packed;       // the policy's packed weights (forward)
    const float* flat;         // the caller's flat parameters (dX, log_std)
    const float* obs[2];       // what each net gathers: [n_total, n_in] agent rows (actor), [n_total / agents, n_in_vf] env rows (critic)
    const float* raw;          // [n_total, n_out]
    const float* logp_old;     // [n_total]
    const float* adv;          // [n_total / agents]
    const float* ret;          // [n_total / agents]
    const int32_t* index;      // [n] or null
    int64_t first, n_total;    // (n_total: AGENT rows)
    int32_t n, G, normalize, agents;
    float clip, vf_coef;
    const float* advstat;
    float* part;               // [G][n_flat]
    float* spart;              // [G][4]
    float* dh[2];              // k_ppo_grad_dh only: per net [n_total][the net's input width] d loss / d obs rows (wg_lstm_ppo.hip)
    int32_t bc_loss;           // k_bc_grad only: WG_BC_MSE / WG_BC_NLL (there `raw` holds the expert's actions)
};

// (`a`: what the launch's workgroups share; the remaining arguments are `a`'s own for one policy, the member's for a population)
// DH: also the gradient with respect to the net's INPUT rows, dX[row][k] = sum_i W0[i][k] dZ0[i][row], into a.dh[net] — what the
// LSTMs in front of a recurrent policy's heads backpropagate (each gathered row is written once, by the one tile that holds it).
// With DH = false the code is what it was before the flag: the same instructions, the same bits.
// `rw`: the rows a workgroup reads and the dh rows it writes (obs, raw, logp_old, adv, ret, dh) — `a` itself, or the member's row of
// a recurrent population's table (WgPopHeadRows), read where it lies: the nets index obs and dh by blockIdx.y.
// HEAD: the actor's loss head (wg_ppo.h) — WGT_HEAD_PPO the clipped surrogate, WGT_HEAD_BC the supervised loss of k_bc_grad, which
// reads the expert's actions where PPO reads `raw` and needs neither logp_old nor the advantages.  A compile-time choice as DH is
// one: with WGT_HEAD_PPO the code is what it was before the parameter.  The critic's head, forward, dW and dX are the same for both.
template <bool DH, int HEAD, class Rows>
__device__ __forceinline__ void ppo_grad(const WgPolicyP& P, const WgPpoK& K, const WgPpoArgs& a, const Rows& rw, const float* a_packed,
                                         const float* a_flat, const int32_t* a_index, const int a_normalize, const float a_clip,
                                         const float a_vf_coef, const float* a_advstat, float* a_part, float* a_spart) {
    extern __shared__ float lds[];
    const int net = blockIdx.y, g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int R = K.R, S = R + 1;
    const WgPpoLds& M = K.lds[net];
    const int L = P.n_layers[net];
    const float* __restrict__ xsrc = rw.obs[net];
    float* xin = lds + M.xin;
    float* rowv = lds + M.rowv;
    int* rid = (int*)(lds + M.rid);
    float* part = a_part + (size_t)g * P.n_flat;
    const int ntile = (a.n + R - 1) / R;
    const float inv_n = 1.0f / (float)a.n;
    const bool tanh_act = P.activation != WG_ACTV_RELU;
    float st0 = 0.0f, st1 = 0.0f, st2 = 0.0f;             // thread 0: running sums of the statistics

    for (int tile = g; tile < ntile; tile += a.G) {
        const bool first = tile == g;
        const int row0 = tile * R;
        __syncthreads();                                   // the previous tile's readers are done with LDS
        // rid = the row THIS net gathers: the minibatch entry (an agent row) for the actor, its env row for the critic — the one
        // division per tile row; the gather loops below only multiply
        if (tid < 32) {
            int id = tid < R ? ppo_row(a_index, a.first, a.n, a.n_total, row0 + tid) : -1;
            if (net == 1 && id >= 0) id /= a.agents;
            rid[tid] = id;
        }

        // ---- forward --------------------------------------------------------------------------------------------
        for (int l = 0; l < L; ++l) {
            const WgPolicyLayer ly = P.layer[net][l];
            f32x16 acc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int ot = wave + WGT_WAVES * t;
                if (ot < ly.ntiles) wg_tile_bias(acc[t], a_packed + ly.b_packed + ot * 32, h);
            }
            const int nchunk = l == 0 ? (ly.K + WGP_KC - 1) / WGP_KC : 1;
            for (int c = 0; c < nchunk; ++c) {
                const int k0 = c * WGP_KC, kc = min(WGP_KC, ly.K - k0);
                if (l == 0) {
                    __syncthreads();
                    for (int idx = tid; idx < kc * R; idx += WGT_WAVES * 64) {      // consecutive threads: consecutive inputs of a row
                        const int row = idx / kc, k = idx - row * kc, id = rid[row];
                        xin[k * S + row] = id >= 0 ? xsrc[(size_t)id * ly.K + k0 + k] : 0.0f;
                    }
                    __syncthreads();
                }
                const float* xb = l == 0 ? xin : lds + M.act[l - 1];
                const int nks = (kc + 1) >> 1;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int ot = wave + WGT_WAVES * t;
                    if (ot < ly.ntiles) {
                        const float* wp = a_packed + ly.w_packed + ((size_t)ot * ly.nks + (k0 >> 1)) * 64 + lane;
                        for (int ks = 0; ks < nks; ++ks) {
                            const int k = 2 * ks + h;
                            const float av = wp[(size_t)ks * 64];
                            const float bv = (k < kc && r < R) ? xb[k * S + r] : 0.0f;
                            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
                        }
                    }
                }
            }
            float* dst = lds + M.act[l];
            const bool head = l == L - 1;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int ot = wave + WGT_WAVES * t;
                if (ot < ly.ntiles) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int i = ot * 32 + wg_tile_drow(q, h);
                        float v = acc[t][q];
                        if (!head) v = tanh_act ? tanhf(v) : fmaxf(v, 0.0f);
                        if (i < ly.M && r < R) dst[i * S + r] = v;
                    }
                }
            }
            __syncthreads();
        }

        // ---- loss head: dZ of the head into d[0], per-row statistics into rowv ------------------------------------------
        float* hb = lds + M.act[L - 1];                    // [output][row]
        float* d0 = lds + M.d[0];
        if (HEAD == WGT_HEAD_BC && net == 0) {
            // L = mean_rows(sum_j (mean_j - target_j)^2 / n_out)  or  -mean_rows(logp(target)): the row's thread writes dZ itself;
            // rowv = the row's weight 1/n (0: no row), its squared error / n_out, its -logp, its absolute error / n_out
            const int n_out = P.n_out;
            const bool nll = a.bc_loss == WG_BC_NLL;
            const float inv_no = 1.0f / (float)n_out;
            if (tid < R) {
                const int id = rid[tid];
                float w = 0.0f, sq = 0.0f, nl = 0.0f, ab = 0.0f;
                if (id >= 0) {
                    w = inv_n;
                    for (int j = 0; j < n_out; ++j) {
                        const float ls = a_flat[P.log_std_flat + j];
                        const float sd = expf(ls);
                        const float e = hb[j * S + tid] - rw.raw[(size_t)id * n_out + j];
                        const float z = -e / sd;
                        sq += e * e;
                        ab += fabsf(e);
                        nl += 0.5f * z * z + ls + WGT_HALF_LOG_2PI;
                        hb[j * S + tid] = z;
                        d0[j * S + tid] = nll ? -(z / sd) * inv_n : 2.0f * e * inv_no * inv_n;
                    }
                } else {
                    for (int j = 0; j < n_out; ++j) { hb[j * S + tid] = 0.0f; d0[j * S + tid] = 0.0f; }
                }
                rowv[tid] = w; rowv[32 + tid] = sq * inv_no; rowv[64 + tid] = nl; rowv[96 + tid] = ab * inv_no;
            }
            __syncthreads();
            if (tid < n_out) {                              // d(-logp) / d log_std_j: sum_row (1 - z^2) / n; under MSE exactly 0, WRITTEN
                float s = 0.0f;                             // all the same: the slot may hold what an earlier call left there
                if (nll)
                    for (int row = 0; row < R; ++row) { const float z = hb[tid * S + row]; s += rowv[row] * (1.0f - z * z); }
                float* o = part + P.log_std_flat + tid;
                *o = first ? s : *o + s;
            }
            if (tid == 0)
                for (int row = 0; row < R; ++row) { st0 += rowv[32 + row]; st1 += rowv[64 + row]; st2 += rowv[96 + row]; }
        } else if (net == 0) {
            const int n_out = P.n_out;
            if (tid < R) {
                const int id = rid[tid];
                float dlogp = 0.0f, lpi = 0.0f, kl = 0.0f, cf = 0.0f;
                if (id >= 0) {
                    float lp = 0.0f;
                    for (int j = 0; j < n_out; ++j) {
                        const float ls = a_flat[P.log_std_flat + j];
                        const float z = (rw.raw[(size_t)id * n_out + j] - hb[j * S + tid]) / expf(ls);
                        hb[j * S + tid] = z;
                        lp += -0.5f * z * z - ls - WGT_HALF_LOG_2PI;
                    }
                    const float lr = lp - rw.logp_old[id];
                    const float ratio = expf(lr);
                    float A = rw.adv[id / a.agents];       // the env row's advantage, shared by its agents
                    if (a_normalize) A = (A - a_advstat[0]) / (a_advstat[1] + 1e-8f);
                    const float rc = fminf(fmaxf(ratio, 1.0f - a_clip), 1.0f + a_clip);
                    const float s1 = ratio * A, s2 = rc * A;
                    lpi = -fminf(s1, s2);
                    kl = expm1f(lr) - lr;                   // (ratio - 1) - log ratio without the cancellation at ratio = 1
                    cf = fabsf(ratio - 1.0f) > a_clip ? 1.0f : 0.0f;
                    dlogp = (ratio == rc || s1 < s2) ? -A * ratio * inv_n : 0.0f;
                } else {
                    for (int j = 0; j < n_out; ++j) hb[j * S + tid] = 0.0f;
                }
                rowv[tid] = dlogp; rowv[32 + tid] = lpi; rowv[64 + tid] = kl; rowv[96 + tid] = cf;
            }
            __syncthreads();
            for (int idx = tid; idx < n_out * R; idx += WGT_WAVES * 64) {
                const int j = idx / R, row = idx - j * R;
                d0[j * S + row] = rowv[row] * hb[j * S + row] / expf(a_flat[P.log_std_flat + j]);
            }
            if (tid < n_out) {                              // d loss / d log_std_j through logp: sum_row dlogp (z^2 - 1)
                float s = 0.0f;
                for (int row = 0; row < R; ++row) { const float z = hb[tid * S + row]; s += rowv[row] * (z * z - 1.0f); }
                float* o = part + P.log_std_flat + tid;
                *o = first ? s : *o + s;
            }
            if (tid == 0)
                for (int row = 0; row < R; ++row) { st0 += rowv[32 + row]; st1 += rowv[64 + row]; st2 += rowv[96 + row]; }
        } else {
            if (tid < R) {
                const int id = rid[tid];
                float dv = 0.0f, lv = 0.0f;
                if (id >= 0) {
                    const float e = hb[tid] - rw.ret[id];
                    lv = e * e;
                    dv = a_vf_coef * 2.0f * e * inv_n;
                }
                d0[tid] = dv;
                rowv[tid] = lv;
            }
            __syncthreads();
            if (tid == 0)
                for (int row = 0; row < R; ++row) st0 += rowv[row];
        }
        __syncthreads();

        // ---- backward ---------------------------------------------------------------------------------------------
        int cur = 0;
        for (int l = L - 1; l >= 0; --l) {
            const WgPolicyLayer ly = P.layer[net][l];
            const float* dz = lds + M.d[cur];
            const int ntm = ly.ntiles;
            // db[i] += sum_row dZ[i][row]
            for (int i = tid; i < ly.M; i += WGT_WAVES * 64) {
                float s = 0.0f;
                for (int row = 0; row < R; ++row) s += dz[i * S + row];
                float* o = part + ly.b_flat + i;
                *o = first ? s : *o + s;
            }
            // dW[i][k] += sum_row dZ[i][row] X[k][row]
            const int nchunk = l == 0 ? (ly.K + WGP_KC - 1) / WGP_KC : 1;
            for (int c = 0; c < nchunk; ++c) {
                const int k0 = c * WGP_KC, kc = min(WGP_KC, ly.K - k0);
                if (l == 0 && nchunk > 1) {                 // (a single chunk is still in LDS from the forward pass)
                    __syncthreads();
                    for (int idx = tid; idx < kc * R; idx += WGT_WAVES * 64) {
                        const int row = idx / kc, k = idx - row * kc, id = rid[row];
                        xin[k * S + row] = id >= 0 ? xsrc[(size_t)id * ly.K + k0 + k] : 0.0f;
                    }
                    __syncthreads();
                }
                const float* xb = l == 0 ? xin : lds + M.act[l - 1];
                const int nkt = (kc + 31) >> 5;
                for (int q = wave; q < ntm * nkt; q += WGT_WAVES) {
                    const int ot = q / nkt, kt = q - ot * nkt;
                    const int kk = kt * 32 + r;             // this lane's column of the output tile (input index within the chunk)
                    float* wo = part + ly.w_flat + k0 + kk;
                    f32x16 acc;
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int i = ot * 32 + wg_tile_drow(e, h);
                        acc[e] = (!first && i < ly.M && kk < kc) ? wo[(size_t)i * ly.K] : 0.0f;
                    }
                    const int ia = ot * 32 + r;
                    for (int s = 0; s < (R >> 1); ++s) {
                        const int row = 2 * s + h;
                        const float av = ia < ly.M ? dz[ia * S + row] : 0.0f;
                        const float bv = kk < kc ? xb[kk * S + row] : 0.0f;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int i = ot * 32 + wg_tile_drow(e, h);
                        if (i < ly.M && kk < kc) wo[(size_t)i * ly.K] = acc[e];
                    }
                }
            }
            // dZ of the layer before: (W^T dZ) * act'(Y); DH: at the first layer W^T dZ itself, the gradient of the gathered rows
            if (l > 0 || DH) {
                float* dp = lds + M.d[cur ^ 1];
                const float* y = lds + M.act[l > 0 ? l - 1 : 0];
                const float* wf = a_flat + ly.w_flat;
                const int nkt = (ly.K + 31) >> 5, nis = (ly.M + 1) >> 1;
                for (int kt = wave; kt < nkt; kt += WGT_WAVES) {
                    const int kk = kt * 32 + r;
                    f32x16 acc;
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
                    for (int s = 0; s < nis; ++s) {
                        const int i = 2 * s + h;
                        const float av = (i < ly.M && kk < ly.K) ? wf[(size_t)i * ly.K + kk] : 0.0f;
                        const float bv = (i < ly.M && r < R) ? dz[i * S + r] : 0.0f;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int k = kt * 32 + wg_tile_drow(e, h);
                        if (k < ly.K && r < R) {
                            if (!DH || l > 0) {
                                const float yv = y[k * S + r];
                                dp[k * S + r] = acc[e] * (tanh_act ? 1.0f - yv * yv : (yv > 0.0f ? 1.0f : 0.0f));
                            } else if (rid[r] >= 0) {
                                rw.dh[net][(size_t)rid[r] * ly.K + k] = acc[e];
                            }
                        }
                    }
                }
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    if (tid == 0) {
        float* sp = a_spart + (size_t)g * 4;
        if (net == 0) { sp[0] = st0; sp[1] = st1; sp[2] = st2; }
        else sp[3] = st0;
    }
}

__global__ __launch_bounds__(WGT_WAVES * 64) void k_ppo_grad(const WgPolicyP P, const WgPpoK K, const WgPpoArgs a) {
    ppo_grad<false, WGT_HEAD_PPO>(P, K, a, a, a.packed, a.flat, a.index, a.normalize, a.clip, a.vf_coef, a.advstat, a.part, a.spart);
}

// k_ppo_grad with the input-row gradients (a.dh) as well: the heads of a recurrent policy on the LSTMs' h rows
__global__ __launch_bounds__(WGT_WAVES * 64) void k_ppo_grad_dh(const WgPolicyP P, const WgPpoK K, const WgPpoArgs a) {
    ppo_grad<true, WGT_HEAD_PPO>(P, K, a, a, a.packed, a.flat, a.index, a.normalize, a.clip, a.vf_coef, a.advstat, a.part, a.spart);
}

// The supervised gradient (wg_bc_grad): the BC head on the expert's actions a.raw; grid (G, 2) with returns, (G, 1) — the actor's
// workgroups alone — without.  a.logp_old, a.adv, a.advstat and the clip are not read.
__global__ __launch_bounds__(WGT_WAVES * 64) void k_bc_grad(const WgPolicyP P, const WgPpoK K, const WgPpoArgs a) {
    ppo_grad<false, WGT_HEAD_BC>(P, K, a, a, a.packed, a.flat, a.index, 0, 0.0f, a.vf_coef, nullptr, a.part, a.spart);
}

// k_bc_grad with the input-row gradients (a.dh) as well: the supervised head on the LSTMs' h rows (wg_lstm_bc_grad).  The same grid
// rule: without returns the critic's workgroups are not launched and a.dh[1] is not written.
__global__ __launch_bounds__(WGT_WAVES * 64) void k_bc_grad_dh(const WgPolicyP P, const WgPpoK K, const WgPpoArgs a) {
    ppo_grad<true, WGT_HEAD_BC>(P, K, a, a, a.packed, a.flat, a.index, 0, 0.0f, a.vf_coef, nullptr, a.part, a.spart);
}

// grid (G, 2, P); `c` carries what the members share (the batch, n, G), the member's row the rest
__global__ __launch_bounds__(WGT_WAVES * 64) void k_ppo_grad_pop(const WgPolicyP P, const WgPpoK K, const WgPpoArgs c,
                                                                 const WgPopMember* __restrict__ mt, const int64_t off) {
    const WgPopMember* __restrict__ M = mt + blockIdx.z;
    ppo_grad<false, WGT_HEAD_PPO>(P, K, c, c, M->packed, M->params, M->perm + off, M->normalize && c.n > 1, M->clip, M->vf_coef, M->advstat, M->part, M->spart);
}

// The heads of a recurrent population: grid (G, 2, P); member blockIdx.z reads ITS rows (row m of `rt`: the h rows of its LSTMs and
// its gathered raw / logp / advantage / returns, n rows in order, no index) and `c` carries what the members share (n, G)
__global__ __launch_bounds__(WGT_WAVES * 64) void k_ppo_grad_dh_pop(const WgPolicyP P, const WgPpoK K, const WgPpoArgs c,
                                                                    const WgPopMember* __restrict__ mt,
                                                                    const WgPopHeadRows* __restrict__ rt) {
    const WgPopMember* __restrict__ M = mt + blockIdx.z;
    ppo_grad<true, WGT_HEAD_PPO>(P, K, c, rt[blockIdx.z], M->packed, M->params, nullptr, M->normalize && c.n > 1, M->clip, M->vf_coef, M->advstat, M->part, M->spart);
}

__global__ __launch_bounds__(1024) void k_ppo_advstat_rows_pop(const WgPopMember* __restrict__ mt, const WgPopHeadRows* __restrict__ rt,
                                                               const int n) {
    const WgPopMember* __restrict__ M = mt + blockIdx.x;
    if (!(M->normalize && n > 1)) return;
    ppo_advstat(rt[blockIdx.x].adv, nullptr, 0, n, n, 1, M->advstat);
}

// entry p of the partials' rows 0 .. G-1, added in index order
__device__ __forceinline__ float ppo_part_sum(const float* __restrict__ part, const int G, const uint32_t n_flat, const uint32_t p) {
    float s = 0.0f;
    int g = 0;
    for (; g + 8 <= G; g += 8) {                           // eight loads in flight, added in index order
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = part[(size_t)(g + u) * n_flat + p];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += x[u];
    }
    for (; g < G; ++g) s += part[(size_t)g * n_flat + p];
    return s;
}

// partials -> flat gradient (+ the entropy term's constant gradient on log_std) and the statistics record
__device__ __forceinline__ void ppo_reduce(const WgPolicyP& P, const float* __restrict__ part, const float* __restrict__ spart,
                                           const int G, const int n, const float vf_coef, const float ent_coef, const int normalize,
                                           const float* __restrict__ advstat, const float* __restrict__ flat,
                                           float* __restrict__ grad, float* __restrict__ stats) {
    const uint32_t p = blockIdx.x * WGT_BLOCK + threadIdx.x;
    if (p < P.n_flat) {
        float s = ppo_part_sum(part, G, P.n_flat, p);
        if (p >= P.log_std_flat) s -= ent_coef;
        grad[p] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int g = 0; g < G; ++g)
            for (int k = 0; k < 4; ++k) s[k] += spart[(size_t)g * 4 + k];
        float H = 0.0f;
        for (int j = 0; j < P.n_out; ++j) H += 0.5f + WGT_HALF_LOG_2PI + flat[P.log_std_flat + j];
        const float inv_n = 1.0f / (float)n;
        const float lpi = s[0] * inv_n, lv = s[3] * inv_n;
        stats[0] = lpi; stats[1] = lv; stats[2] = H; stats[3] = s[1] * inv_n; stats[4] = s[2] * inv_n;
        stats[5] = lpi + vf_coef * lv - ent_coef * H;
        stats[6] = normalize ? advstat[0] : 0.0f;
        stats[7] = normalize ? advstat[1] : 1.0f;
    }
}

__global__ __launch_bounds__(WGT_BLOCK) void k_ppo_reduce(const WgPolicyP P, const float* __restrict__ part,
                                                           const float* __restrict__ spart, const int G, const int n,
                                                           const float vf_coef, const float ent_coef, const int normalize,
                                                           const float* __restrict__ advstat, const float* __restrict__ flat,
                                                           float* __restrict__ grad, float* __restrict__ stats) {
    ppo_reduce(P, part, spart, G, n, vf_coef, ent_coef, normalize, advstat, flat, grad, stats);
}

__global__ __launch_bounds__(WGT_BLOCK) void k_ppo_reduce_pop(const WgPolicyP P, const WgPopMember* __restrict__ mt, const int G,
                                                               const int n, const int mb) {
    const WgPopMember* __restrict__ M = mt + blockIdx.y;
    ppo_reduce(P, M->part, M->spart, G, n, M->vf_coef, M->ent_coef, M->normalize && n > 1, M->advstat, M->params, M->grad,
               M->stats + (size_t)mb * M->stats_step);
}

// k_bc_grad's partials -> flat gradient and the wg_bc_stats record.  A reduce of its own: the four spart slots of a workgroup hold
// BC's sums (actor: squared error, -logp, absolute error; critic: L_v), and what no workgroup wrote in THIS call is never read —
// without returns the critic's workgroups were not launched, their rows of `part` and slot 3 hold an earlier call's values, and
// the critic's entries [critic_from, log_std_flat) are 0.0f.  Under MSE log_std gets the sum of the G zeros the actor wrote.
__global__ __launch_bounds__(WGT_BLOCK) void k_bc_reduce(const WgPolicyP P, const float* __restrict__ part,
                                                          const float* __restrict__ spart, const int G, const int n,
                                                          const uint32_t critic_from, const int has_ret, const int nll,
                                                          const float vf_coef, const float ent_coef, const float* __restrict__ flat,
                                                          float* __restrict__ grad, float* __restrict__ stats) {
    const uint32_t p = blockIdx.x * WGT_BLOCK + threadIdx.x;
    if (p < P.n_flat) {
        float s = 0.0f;
        if (has_ret || p < critic_from || p >= P.log_std_flat) s = ppo_part_sum(part, G, P.n_flat, p);
        if (nll && p >= P.log_std_flat) s -= ent_coef;
        grad[p] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int g = 0; g < G; ++g)
            for (int k = 0; k < (has_ret ? 4 : 3); ++k) s[k] += spart[(size_t)g * 4 + k];
        float H = 0.0f;
        for (int j = 0; j < P.n_out; ++j) H += 0.5f + WGT_HALF_LOG_2PI + flat[P.log_std_flat + j];
        const float inv_n = 1.0f / (float)n;
        const float mse = s[0] * inv_n, nl = s[1] * inv_n, lv = s[3] * inv_n;
        float loss = nll ? nl - ent_coef * H : mse;
        if (has_ret) loss += vf_coef * lv;
        stats[0] = loss; stats[1] = mse; stats[2] = nl; stats[3] = H; stats[4] = lv; stats[5] = s[2] * inv_n;
        stats[6] = 0.0f; stats[7] = 0.0f;
    }
}

// blocksq[b] = sum of squares of block b's 256 gradient entries (fixed tree)
__device__ __forceinline__ void ppo_sumsq(const float* __restrict__ grad, const uint32_t n_flat, float* __restrict__ blocksq) {
    __shared__ float sh[WGT_BLOCK];
    const uint32_t p = blockIdx.x * WGT_BLOCK + threadIdx.x;
    const float gv = p < n_flat ? grad[p] : 0.0f;
    const float s = block_sum<WGT_BLOCK>(gv * gv, sh);
    if (threadIdx.x == 0) blocksq[blockIdx.x] = s;
}

__global__ __launch_bounds__(WGT_BLOCK) void k_ppo_sumsq(const float* __restrict__ grad, const uint32_t n_flat,
                                                          float* __restrict__ blocksq) {
    ppo_sumsq(grad, n_flat, blocksq);
}

__global__ __launch_bounds__(WGT_BLOCK) void k_ppo_sumsq_pop(const WgPopMember* __restrict__ mt, const uint32_t n_flat) {
    const WgPopMember* __restrict__ M = mt + blockIdx.y;
    ppo_sumsq(M->grad, n_flat, M->blocksq);
}

// clip by the global norm, then torch.optim.Adam's step (no weight decay, no amsgrad) on params in place
__device__ __forceinline__ void ppo_adam(float* __restrict__ params, const float* __restrict__ grad, float* __restrict__ m,
                                         float* __restrict__ v, const uint32_t n_flat, const float* __restrict__ blocksq,
                                         const uint32_t n_blocks, const float max_norm, const float step_size, const float bc2_sqrt,
                                         const float omb1, const float beta2, const float omb2, const float eps) {
    __shared__ float sh[WGT_BLOCK];
    float s = 0.0f;
    for (uint32_t b = threadIdx.x; b < n_blocks; b += WGT_BLOCK) s += blocksq[b];
    const float norm = sqrtf(block_sum<WGT_BLOCK>(s, sh));
    const float scale = fminf(1.0f, max_norm / (norm + 1e-6f));
    const uint32_t p = blockIdx.x * WGT_BLOCK + threadIdx.x;
    if (p >= n_flat) return;
    const float gv = grad[p] * scale;
    const float mv = m[p] + (gv - m[p]) * omb1;
    const float vv = v[p] * beta2 + omb2 * (gv * gv);
    m[p] = mv; v[p] = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    params[p] = params[p] - step_size * (mv / denom);
}

__global__ __launch_bounds__(WGT_BLOCK) void k_ppo_adam(float* __restrict__ params, const float* __restrict__ grad,
                                                         float* __restrict__ m, float* __restrict__ v, const uint32_t n_flat,
                                                         const float* __restrict__ blocksq, const uint32_t n_blocks,
                                                         const float max_norm, const float step_size, const float bc2_sqrt,
                                                         const float omb1, const float beta2, const float omb2, const float eps) {
    ppo_adam(params, grad, m, v, n_flat, blocksq, n_blocks, max_norm, step_size, bc2_sqrt, omb1, beta2, omb2, eps);
}

// (step size and bias correction depend on the member's own step count and learning rate: computed by the host, as for one policy)
struct WgPopAdam { float step_size[WGP_POP_MAX], bc2_sqrt[WGP_POP_MAX]; };
__global__ __launch_bounds__(WGT_BLOCK) void k_ppo_adam_pop(const WgPopMember* __restrict__ mt, const uint32_t n_flat,
                                                             const uint32_t n_blocks, const WgPopAdam A, const float omb1,
                                                             const float beta2, const float omb2, const float eps) {
    const WgPopMember* __restrict__ M = mt + blockIdx.y;
    ppo_adam(M->params, M->grad, M->m, M->v, n_flat, M->blocksq, n_blocks, M->max_norm, A.step_size[blockIdx.y], A.bc2_sqrt[blockIdx.y],
             omb1, beta2, omb2, eps);
}

// The same step with the KL-adaptive rate (wg_train.h: wg_kl_lr_next, wg_kl_lr_words) — no launch of its own: EVERY block reads the
// rate of the step before from *lr_in and the minibatch's approx_kl from *kl (null: the update's first minibatch, whose KL is
// rounding noise — the rate stays) and forms the same new rate; block 0's first thread stores it to *lr_out (null: nothing to
// store), a word no block reads in this launch.  step_size is wg_adam_scalars' expression on the rate read here.
__device__ __forceinline__ float ppo_kl_lr(const float* lr_in, float* lr_out, const float* kl, const WgKlLr& rule, const bool writes) {
    float lr = *lr_in;
    if (kl) lr = wg_kl_lr_next(lr, *kl, rule);
    if (writes && lr_out) *lr_out = lr;
    return lr;
}

__global__ __launch_bounds__(WGT_BLOCK) void k_ppo_adam_kl(float* __restrict__ params, const float* __restrict__ grad,
                                                            float* __restrict__ m, float* __restrict__ v, const uint32_t n_flat,
                                                            const float* __restrict__ blocksq, const uint32_t n_blocks,
                                                            const float max_norm, const float* lr_in, float* lr_out, const float* kl,
                                                            const WgKlLr rule, const double bc1, const float bc2_sqrt, const float omb1,
                                                            const float beta2, const float omb2, const float eps) {
    const float lr = ppo_kl_lr(lr_in, lr_out, kl, rule, blockIdx.x == 0 && threadIdx.x == 0);
    ppo_adam(params, grad, m, v, n_flat, blocksq, n_blocks, max_norm, (float)((double)lr / bc1), bc2_sqrt, omb1, beta2, omb2, eps);
}

// (member m's words and rule are its row's; mb: the minibatch's ordinal in the update = its stats slot, last: the update's final one)
struct WgPopAdamKl { double bc1[WGP_POP_MAX]; float bc2_sqrt[WGP_POP_MAX]; };
__global__ __launch_bounds__(WGT_BLOCK) void k_ppo_adam_kl_pop(const WgPopMember* __restrict__ mt, const uint32_t n_flat,
                                                                const uint32_t n_blocks, const WgPopAdamKl A, const int mb, const int last,
                                                                const float omb1, const float beta2, const float omb2, const float eps) {
    const WgPopMember* __restrict__ M = mt + blockIdx.y;
    const float* lr_in;
    float* lr_out;
    wg_kl_lr_words(M->lr_dev, M->lr_slots, mb, last, &lr_in, &lr_out);
    const float* kl = mb == 0 ? nullptr : M->stats + (size_t)mb * M->stats_step + WGT_STAT_KL;
    const float lr = ppo_kl_lr(lr_in, lr_out, kl, M->rule, blockIdx.x == 0 && threadIdx.x == 0);
    ppo_adam(M->params, M->grad, M->m, M->v, n_flat, M->blocksq, n_blocks, M->max_norm, (float)((double)lr / A.bc1[blockIdx.y]),
             A.bc2_sqrt[blockIdx.y], omb1, beta2, omb2, eps);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// The argument checks of every wg_gae* entry.  `who`, `dims` and `rows` name the caller, its sizes and its B * A rows in the
// messages; `all_there`: no pointer argument is null; P: the members the B envs divide among (1: one policy, always passes).
static int gae_check(const char* who, const char* dims, const char* rows, bool all_there, int T, int B, int A, int P) {
    const std::string w = who;
    if (!all_there) return wg_fail(WG_ERR_INVALID, w + ": null argument");
    if (T < 1 || B < 1 || A < 1) return wg_fail(WG_ERR_INVALID, w + ": " + dims + " must be >= 1");
    if (P < 1 || P > WG_POP_MAX || B % P != 0)
        return wg_fail(WG_ERR_INVALID, w + ": P = " + std::to_string(P) + " must lie in 1 .. " + std::to_string(WG_POP_MAX) +
                                         " and divide B = " + std::to_string(B));
    if ((long long)B * A > 0x7fffffffLL - 256) return wg_fail(WG_ERR_UNSUPPORTED, w + ": more than 2^31 " + rows);
    return 0;
}

// wg_gae (A = 1) and wg_gae_shared
static int gae_launch(const char* who, const char* dims, int T, int B, int A, const float* reward_dev, const float* value_dev,
                      const float* final_value_dev, const uint8_t* truncated_dev, float gamma, float lambda, float* advantage_out,
                      float* returns_out, void* stream) {
    if (int rc = gae_check(who, dims, "agent rows", reward_dev && value_dev && final_value_dev && truncated_dev && advantage_out && returns_out,
                           T, B, A, 1))
        return rc;
    hipLaunchKernelGGL(k_gae, dim3((B * A + 255) / 256), dim3(256), 0, (hipStream_t)stream, T, B, A, reward_dev, value_dev,
                       final_value_dev, truncated_dev, gamma, lambda, advantage_out, returns_out);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_gae(int T, int B, const float* reward_dev, const float* value_dev, const float* final_value_dev,
                      const uint8_t* truncated_dev, float gamma, float lambda, float* advantage_out, float* returns_out,
                      void* stream) {
    return gae_launch("wg_gae", "T and B", T, B, 1, reward_dev, value_dev, final_value_dev, truncated_dev, gamma, lambda,
                      advantage_out, returns_out, stream);
}

extern "C" int wg_gae_shared(int T, int B, int A, const float* reward_dev, const float* value_dev, const float* final_value_dev,
                             const uint8_t* truncated_dev, float gamma, float lambda, float* advantage_out, float* returns_out,
                             void* stream) {
    return gae_launch("wg_gae_shared", "T, B and A", T, B, A, reward_dev, value_dev, final_value_dev, truncated_dev, gamma, lambda,
                      advantage_out, returns_out, stream);
}

// LDS map of both nets for tiles of R rows -> bytes of the larger one
static size_t t_lds_map(const WgPolicyP& P, int R, WgPpoK* K) {
    const int S = R + 1;
    size_t most = 0;
    K->R = R;
    for (int net = 0; net < 2; ++net) {
        WgPpoLds& m = K->lds[net];
        int o = 0, maxw = 1;
        const int n_in = net == 0 ? P.n_in : P.n_in_vf;          // each net's own input width
        m.xin = o; o += (n_in < WGP_KC ? n_in : WGP_KC) * S;
        for (int l = 0; l < WGP_MAX_LAYERS; ++l) {
            m.act[l] = o;
            if (l < P.n_layers[net]) {
                o += P.layer[net][l].M * S;
                if (P.layer[net][l].M > maxw) maxw = P.layer[net][l].M;
            }
        }
        m.d[0] = o; o += maxw * S;
        m.d[1] = o; o += maxw * S;
        m.rowv = o; o += 4 * 32;
        m.rid = o; o += 32;
        m.total = o;
        if ((size_t)o * sizeof(float) > most) most = (size_t)o * sizeof(float);
    }
    return most;
}

// WgAdam (wg_train.h) and WgPpoGrad (wg_ppo.h): wg_internal.h states what each function does
extern "C" int wg_adam_alloc_(WgDevMem* mem, WgAdam* a, uint32_t n_flat, const char* who) {
    *a = {mem->device, n_flat, (n_flat + WGT_BLOCK - 1) / WGT_BLOCK, 0, nullptr, nullptr, nullptr, nullptr, nullptr, {}};
    if (int rc = mem->alloc(who, &a->m, n_flat)) return rc;
    if (int rc = mem->alloc(who, &a->v, n_flat)) return rc;
    return mem->alloc(who, &a->blocksq, a->n_blocks, false);
}

extern "C" int wg_adam_set_kl_lr_(WgDevMem* mem, WgAdam* a, const char* who, const wg_kl_lr* rule, float* lr_dev) {
    const std::string w = who;
    if (!a || !mem) return wg_fail(WG_ERR_INVALID, w + ": null argument");
    if (!rule && !lr_dev) {
        a->lr_dev = nullptr;
        return 0;
    }
    if (!rule) return wg_fail(WG_ERR_INVALID, w + ": rule is null (with lr_dev given; both null turn the rule off)");
    if (!lr_dev) return wg_fail(WG_ERR_INVALID, w + ": lr_dev is null (with a rule given; both null turn the rule off)");
    if (const char* bad = wg_kl_lr_refusal(rule->desired_kl, rule->factor, rule->lr_min, rule->lr_max)) return wg_fail(WG_ERR_INVALID, w + ": " + bad);
    if (int rc = wg_use_device(a->device)) return rc;
    if (int rc = wg_on_device(w + ": ", a->device, lr_dev, "lr_dev", ", the handle's device")) return rc;
    float lr0 = 0.0f;
    WG_HIPCHK(hipDeviceSynchronize());
    WG_HIPCHK(hipMemcpy(&lr0, lr_dev, sizeof(float), hipMemcpyDeviceToHost));
    if (!(lr0 >= rule->lr_min && lr0 <= rule->lr_max)) {
        char says[128];
        snprintf(says, sizeof(says), ": the starting rate *lr_dev = %g lies outside [lr_min, lr_max] = [%g, %g]", lr0, rule->lr_min, rule->lr_max);
        return wg_fail(WG_ERR_INVALID, w + says);
    }
    if (!a->lr_slots)                                           // the first rule set on this handle: a handle that never takes one allocates nothing
        if (int rc = mem->alloc(who, &a->lr_slots, 2, false)) return rc;
    a->rule = wg_kl_lr_rule(rule->desired_kl, rule->factor, rule->lr_min, rule->lr_max);
    a->lr_dev = lr_dev;
    return 0;
}

// what get_state / set_state check before they copy: the arguments, the size, the device idle
static int adam_state_ready(const WgAdam* a, const std::string& who, bool all_there, size_t n) {
    if (!a || !all_there) return wg_fail(WG_ERR_INVALID, who + ": null argument");
    if (n != 2 * (size_t)a->n_flat) return wg_fail(WG_ERR_INVALID, who + ": the state has " + std::to_string(2 * (size_t)a->n_flat) + " floats");
    if (int rc = wg_use_device(a->device)) return rc;
    WG_HIPCHK(hipDeviceSynchronize());
    return 0;
}

extern "C" int wg_adam_get_state_(WgAdam* a, const char* who, float* mv_host, size_t n, uint64_t* step) {
    if (int rc = adam_state_ready(a, who, mv_host && step, n)) return rc;
    WG_HIPCHK(hipMemcpy(mv_host, a->m, sizeof(float) * a->n_flat, hipMemcpyDeviceToHost));
    WG_HIPCHK(hipMemcpy(mv_host + a->n_flat, a->v, sizeof(float) * a->n_flat, hipMemcpyDeviceToHost));
    *step = a->step;
    return 0;
}

extern "C" int wg_adam_set_state_(WgAdam* a, const char* who, const float* mv_host, size_t n, uint64_t step) {
    if (int rc = adam_state_ready(a, who, mv_host, n)) return rc;
    WG_HIPCHK(hipMemcpy(a->m, mv_host, sizeof(float) * a->n_flat, hipMemcpyHostToDevice));
    WG_HIPCHK(hipMemcpy(a->v, mv_host + a->n_flat, sizeof(float) * a->n_flat, hipMemcpyHostToDevice));
    a->step = step;
    return 0;
}

extern "C" int wg_adam_apply_(WgAdam* a, float* params_dev, const float* grad_dev, float lr, float max_grad_norm, hipStream_t st) {
    const WgAdamStep s = wg_adam_count(a, lr);
    hipLaunchKernelGGL(k_ppo_sumsq, dim3(a->n_blocks), dim3(WGT_BLOCK), 0, st, grad_dev, a->n_flat, a->blocksq);
    hipLaunchKernelGGL(k_ppo_adam, dim3(a->n_blocks), dim3(WGT_BLOCK), 0, st, params_dev, grad_dev, a->m, a->v, a->n_flat,
                       a->blocksq, a->n_blocks, max_grad_norm, s.step_size, s.bc2_sqrt, (float)(1.0 - ADAM_B1), (float)ADAM_B2, (float)(1.0 - ADAM_B2), ADAM_EPS);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_adam_apply_kl_(WgAdam* a, float* params_dev, const float* grad_dev, const float* stats_dev, int mb, int last,
                                 float max_grad_norm, hipStream_t st) {
    const WgAdamKlStep s = wg_adam_kl_scalars(++a->step);
    const float* lr_in;
    float* lr_out;
    wg_kl_lr_words(a->lr_dev, a->lr_slots, mb, last, &lr_in, &lr_out);
    hipLaunchKernelGGL(k_ppo_sumsq, dim3(a->n_blocks), dim3(WGT_BLOCK), 0, st, grad_dev, a->n_flat, a->blocksq);
    hipLaunchKernelGGL(k_ppo_adam_kl, dim3(a->n_blocks), dim3(WGT_BLOCK), 0, st, params_dev, grad_dev, a->m, a->v, a->n_flat, a->blocksq,
                       a->n_blocks, max_grad_norm, lr_in, lr_out, mb == 0 ? nullptr : stats_dev + WGT_STAT_KL, a->rule, s.bc1, s.bc2_sqrt,
                       (float)(1.0 - ADAM_B1), (float)ADAM_B2, (float)(1.0 - ADAM_B2), ADAM_EPS);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_ppo_grad_init_(WgDevMem* mem, WgPpoGrad* g, wg_policy p, const char* who) {
    const WgPolicyP& P = p->P;
    if (P.n_layers[1] == 0) return wg_fail(WG_ERR_INVALID, "wg_ppo_create: training needs a policy with a critic");
    if (!P.has_log_std) return wg_fail(WG_ERR_INVALID, "wg_ppo_create: training needs a policy with log_std");
    g->pol = p;
    g->n_blocks = (P.n_flat + WGT_BLOCK - 1) / WGT_BLOCK;
    int R = 32;
    while ((g->lds_bytes = t_lds_map(P, R, &g->K)) > WGT_LDS_BYTES && R > 2) R >>= 1;
    if (g->lds_bytes > WGT_LDS_BYTES)
        return wg_fail(WG_ERR_UNSUPPORTED, "wg_ppo_create: the architecture's activations do not fit the workgroup's LDS");
    size_t gm = WGT_PART_BYTES / (sizeof(float) * (size_t)P.n_flat);
    g->g_max = (int)(gm < 1 ? 1 : gm > WGT_G_MAX ? WGT_G_MAX : gm);
    if (int rc = mem->alloc(who, &g->part, (size_t)P.n_flat * g->g_max, false)) return rc;
    if (int rc = mem->alloc(who, &g->spart, (size_t)4 * g->g_max)) return rc;
    if (int rc = mem->alloc(who, &g->advstat, 2)) return rc;
    return mem->alloc(who, &g->stats, WGT_NSTAT, false);
}

extern "C" int wg_ppo_create(wg_policy p, wg_ppo* out) {
    if (!p || !out) return wg_fail(WG_ERR_INVALID, "wg_ppo_create: null argument");
    *out = nullptr;
    wg_ppo_s* o = new (std::nothrow) wg_ppo_s();
    if (!o) return wg_fail(WG_ERR_NOMEM, "wg_ppo_create: out of host memory");
    o->mem.device = o->adam.device = p->w.device;
    int rc = wg_ppo_grad_init_(&o->mem, &o->g, p, "wg_ppo_create");
    if (!rc) rc = wg_adam_alloc_(&o->mem, &o->adam, p->P.n_flat, "wg_ppo_create");
    if (!rc) rc = o->mem.alloc("wg_ppo_create", &o->grad, p->P.n_flat, false);
    if (rc) {
        wg_ppo_destroy(o);
        return rc;
    }
    *out = o;
    return 0;
}

extern "C" int wg_ppo_destroy(wg_ppo o) {
    if (!o) return 0;
    o->mem.release();
    delete o;
    return 0;
}

extern "C" int wg_ppo_get_state(wg_ppo o, float* mv_host, size_t n, uint64_t* step) {
    return wg_adam_get_state_(o ? &o->adam : nullptr, "wg_ppo_get_state", mv_host, n, step);
}

extern "C" int wg_ppo_set_state(wg_ppo o, const float* mv_host, size_t n, uint64_t step) {
    return wg_adam_set_state_(o ? &o->adam : nullptr, "wg_ppo_set_state", mv_host, n, step);
}

// the rows of a batch and the critic's stream (a plain batch: its obs), for every entry that takes one
static int t_check_rows(const char* who, const wg_ppo_batch* b, const float* obs_vf) {
    if (!b->obs || !b->raw || !b->logp || !b->advantage || !b->returns || !obs_vf)
        return wg_fail(WG_ERR_INVALID, std::string(who) + ": a batch pointer is null");
    if (b->n_rows < 1 || b->n_rows > 0x7fffffff) return wg_fail(WG_ERR_INVALID, std::string(who) + ": n_rows out of range");
    return 0;
}

// (`who` is the entry the CALLER used: wg_ppo_grad is wg_ppo_grad_shared on {*batch, batch->obs, 1} and reports under its own name)
static int t_check_batch(const char* who, const wg_ppo_batch_shared* sb, const wg_ppo_hyper* hp) {
    if (!sb || !hp) return wg_fail(WG_ERR_INVALID, std::string(who) + ": null argument");
    const wg_ppo_batch* b = &sb->rows;
    if (int rc = t_check_rows(who, b, sb->obs_vf)) return rc;
    if (sb->agents < 1 || b->n_rows % sb->agents != 0)
        return wg_fail(WG_ERR_INVALID, std::string(who) + ": agents must be >= 1 and divide n_rows (" + std::to_string(b->n_rows) + ")");
    if (!(hp->clip_range >= 0.0f)) return wg_fail(WG_ERR_INVALID, std::string(who) + ": clip_range < 0");
    return 0;
}

// workgroups per net of a gradient launch on n rows: one per tile of R rows, at most as many as the partial sums have room for
static int t_grid(const WgPpoGrad* g, int n) {
    const int R = g->K.R, ntile = (n + R - 1) / R;
    return ntile < g->g_max ? ntile : g->g_max;
}

// the launches of one gradient, no argument checks
// (dh_pi / dh_vf both given: k_ppo_grad_dh, which also writes the gradients of the gathered rows — wg_ppo_heads_grad_)
static int t_grad(WgPpoGrad* o, const float* params_dev, const wg_ppo_batch_shared* sb, const int32_t* index_dev, int64_t first, int n,
                  const wg_ppo_hyper* hp, float* grad_out, float* stats_out, hipStream_t st, float* dh_pi = nullptr, float* dh_vf = nullptr) {
    const WgPolicyP& P = o->pol->P;
    const wg_ppo_batch* b = &sb->rows;
    const int G = t_grid(o, n);
    const int normalize = hp->normalize_advantage && n > 1;
    if (normalize) hipLaunchKernelGGL(k_ppo_advstat, dim3(1), dim3(1024), 0, st, b->advantage, index_dev, first, n, b->n_rows, sb->agents, o->advstat);
    WgPpoArgs a;
    a.packed = o->pol->w.packed; a.flat = params_dev; a.obs[0] = b->obs; a.obs[1] = sb->obs_vf; a.agents = sb->agents; a.raw = b->raw; a.logp_old = b->logp; a.adv = b->advantage;
    a.ret = b->returns; a.index = index_dev; a.first = first; a.n_total = b->n_rows; a.n = n; a.G = G; a.normalize = normalize;
    a.clip = hp->clip_range; a.vf_coef = hp->vf_coef; a.advstat = o->advstat; a.part = o->part; a.spart = o->spart;
    a.dh[0] = dh_pi; a.dh[1] = dh_vf; a.bc_loss = 0;
    if (dh_pi && dh_vf) hipLaunchKernelGGL(k_ppo_grad_dh, dim3(G, 2), dim3(WGT_WAVES * 64), o->lds_bytes, st, P, o->K, a);
    else hipLaunchKernelGGL(k_ppo_grad, dim3(G, 2), dim3(WGT_WAVES * 64), o->lds_bytes, st, P, o->K, a);
    hipLaunchKernelGGL(k_ppo_reduce, dim3(o->n_blocks), dim3(WGT_BLOCK), 0, st, P, o->part, o->spart, G, n, hp->vf_coef,
                       hp->ent_coef, normalize, o->advstat, params_dev, grad_out, stats_out ? stats_out : o->stats);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

static int t_apply(wg_ppo o, float* params_dev, const float* grad_dev, float lr, float max_grad_norm, hipStream_t st) {
    if (int rc = wg_adam_apply_(&o->adam, params_dev, grad_dev, lr, max_grad_norm, st)) return rc;
    return wg_policy_set_params(o->g.pol, params_dev, o->adam.n_flat, 1, (void*)st);
}

// ... of minibatch mb of an update under the handle's KL rule: the rate from device memory, stepped by the record at stats_dev
static int t_apply_kl(wg_ppo o, float* params_dev, const float* grad_dev, const float* stats_dev, int mb, int last, float max_grad_norm,
                      hipStream_t st) {
    if (int rc = wg_adam_apply_kl_(&o->adam, params_dev, grad_dev, stats_dev, mb, last, max_grad_norm, st)) return rc;
    return wg_policy_set_params(o->g.pol, params_dev, o->adam.n_flat, 1, (void*)st);
}

// wg_internal.h: the heads of a recurrent policy (wg_lstm_ppo.hip)
extern "C" int wg_ppo_heads_grad_(WgPpoGrad* g, const float* mlp_params_dev, const float* h_pi, const float* h_vf, const float* raw,
                                  const float* logp, const float* adv, const float* ret, int n, const wg_ppo_hyper* hp, float* dh_pi,
                                  float* dh_vf, float* grad_out, float* stats_out, void* stream) {
    const wg_ppo_batch_shared sb = {{h_pi, raw, logp, adv, ret, n}, h_vf, 1};
    return t_grad(g, mlp_params_dev, &sb, nullptr, 0, n, hp, grad_out, stats_out, (hipStream_t)stream, dh_pi, dh_vf);
}

// wg_internal.h: the heads of a recurrent population (wg_lstm_ppo.hip) — t_grad's three launches with the member axis
extern "C" int wg_ppo_heads_grad_pop_(const WgPpoGrad* g0, const WgPopMember* mt, const WgPopHeadRows* rt, int n_members, int any_norm,
                                      int n, int mb, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const WgPolicyP& P = g0->pol->P;
    const int G = t_grid(g0, n);
    if (any_norm && n > 1) hipLaunchKernelGGL(k_ppo_advstat_rows_pop, dim3(n_members), dim3(1024), 0, st, mt, rt, n);
    WgPpoArgs a = {};
    a.agents = 1; a.first = 0; a.n_total = n; a.n = n; a.G = G;
    hipLaunchKernelGGL(k_ppo_grad_dh_pop, dim3(G, 2, n_members), dim3(WGT_WAVES * 64), g0->lds_bytes, st, P, g0->K, a, mt, rt);
    hipLaunchKernelGGL(k_ppo_reduce_pop, dim3(g0->n_blocks, n_members), dim3(WGT_BLOCK), 0, st, P, mt, G, n, mb);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_adam_apply_pop_(const WgPopMember* mt, int n_members, WgAdam* const* adam, const float* lr, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_flat = adam[0]->n_flat, n_blocks = (n_flat + WGT_BLOCK - 1) / WGT_BLOCK;
    WgPopAdam A = {};
    for (int m = 0; m < n_members; ++m) {
        const WgAdamStep s = wg_adam_count(adam[m], lr[m]);
        A.step_size[m] = s.step_size; A.bc2_sqrt[m] = s.bc2_sqrt;
    }
    hipLaunchKernelGGL(k_ppo_sumsq_pop, dim3(n_blocks, n_members), dim3(WGT_BLOCK), 0, st, mt, n_flat);
    hipLaunchKernelGGL(k_ppo_adam_pop, dim3(n_blocks, n_members), dim3(WGT_BLOCK), 0, st, mt, n_flat, n_blocks, A, (float)(1.0 - ADAM_B1),
                       (float)ADAM_B2, (float)(1.0 - ADAM_B2), ADAM_EPS);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_pop_kl_lr_(const char* who, int n_members, WgAdam* const* adam, int* on) {
    *on = adam[0]->lr_dev != nullptr;
    for (int m = 1; m < n_members; ++m) {
        const std::string w = std::string(who) + ": member " + std::to_string(m);
        if ((adam[m]->lr_dev != nullptr) != (*on != 0))
            return wg_fail(WG_ERR_INVALID, w + (*on ? " has no KL-adaptive rate set while member 0 has one"
                                                    : " has a KL-adaptive rate set while member 0 has none") +
                                             ": the members' launches run in lockstep, so every member is set (*_set_kl_lr) or none");
        for (int k = 0; *on && k < m; ++k)
            if (adam[k]->lr_dev == adam[m]->lr_dev) return wg_fail(WG_ERR_INVALID, w + ": its lr_dev is member " + std::to_string(k) + "'s");
    }
    return 0;
}

extern "C" int wg_adam_apply_kl_pop_(const WgPopMember* mt, int n_members, WgAdam* const* adam, int mb, int last, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_flat = adam[0]->n_flat, n_blocks = (n_flat + WGT_BLOCK - 1) / WGT_BLOCK;
    WgPopAdamKl A = {};
    for (int m = 0; m < n_members; ++m) {
        const WgAdamKlStep s = wg_adam_kl_scalars(++adam[m]->step);
        A.bc1[m] = s.bc1; A.bc2_sqrt[m] = s.bc2_sqrt;
    }
    hipLaunchKernelGGL(k_ppo_sumsq_pop, dim3(n_blocks, n_members), dim3(WGT_BLOCK), 0, st, mt, n_flat);
    hipLaunchKernelGGL(k_ppo_adam_kl_pop, dim3(n_blocks, n_members), dim3(WGT_BLOCK), 0, st, mt, n_flat, n_blocks, A, mb, last,
                       (float)(1.0 - ADAM_B1), (float)ADAM_B2, (float)(1.0 - ADAM_B2), ADAM_EPS);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

// the handle's device becomes the current one; the parameters and the batch's observation streams must live on it
static int t_use_device(const std::string& w, wg_ppo o, const float* params_dev, const wg_ppo_batch_shared* b) {
    if (int rc = wg_use_device(o->adam.device)) return rc;
    if (int rc = wg_on_device_all(w + ": ", w + ": ", o->adam.device, {{params_dev, "params_dev", true}, {b->rows.obs, "obs", true}}, "")) return rc;
    if (b->obs_vf != b->rows.obs) return wg_on_device(w + ": ", o->adam.device, b->obs_vf, "obs_vf", "");
    return 0;
}

static int grad_entry(const char* who, wg_ppo o, const float* params_dev, const wg_ppo_batch_shared* b, const int32_t* index_dev,
                      int64_t first, int n, const wg_ppo_hyper* hp, float* grad_out, wg_ppo_stats* stats_out, void* stream) {
    const std::string w = who;
    if (!o || !params_dev || !grad_out) return wg_fail(WG_ERR_INVALID, w + ": null argument");
    if (int rc = t_check_batch(who, b, hp)) return rc;
    if (n < 1) return wg_fail(WG_ERR_INVALID, w + ": n < 1");
    if (!index_dev && (first < 0 || first + n > b->rows.n_rows)) return wg_fail(WG_ERR_INVALID, w + ": rows first .. first + n - 1 leave the batch");
    if (int rc = t_use_device(w, o, params_dev, b)) return rc;
    return t_grad(&o->g, params_dev, b, index_dev, first, n, hp, grad_out, (float*)stats_out, (hipStream_t)stream);
}

extern "C" int wg_ppo_grad_shared(wg_ppo o, const float* params_dev, const wg_ppo_batch_shared* b, const int32_t* index_dev,
                                  int64_t first, int n, const wg_ppo_hyper* hp, float* grad_out, wg_ppo_stats* stats_out, void* stream) {
    return grad_entry("wg_ppo_grad_shared", o, params_dev, b, index_dev, first, n, hp, grad_out, stats_out, stream);
}

// A plain wg_ppo_batch has ONE observation stream of n_in inputs per row: the critic of a split policy cannot read it (it would
// gather rows of n_in_vf from a buffer of rows of n_in).  Refused here, before anything is enqueued.
static int t_refuse_split(const char* who, wg_ppo o) {
    const WgPolicyP& P = o->g.pol->P;
    if (P.n_in_vf == P.n_in) return 0;
    return wg_fail(WG_ERR_INVALID, std::string(who) + ": the policy's critic reads rows of " + std::to_string(P.n_in_vf) + " inputs, its actor rows of " +
                                     std::to_string(P.n_in) + ", and a wg_ppo_batch has one obs stream of the actor's width: use " + who +
                                     "_shared with the critic's rows as obs_vf");
}

extern "C" int wg_ppo_grad(wg_ppo o, const float* params_dev, const wg_ppo_batch* b, const int32_t* index_dev, int64_t first,
                           int n, const wg_ppo_hyper* hp, float* grad_out, wg_ppo_stats* stats_out, void* stream) {
    if (!o || !b) return wg_fail(WG_ERR_INVALID, "wg_ppo_grad: null argument");
    if (int rc = t_refuse_split("wg_ppo_grad", o)) return rc;
    const wg_ppo_batch_shared sb = {*b, b->obs, 1};
    return grad_entry("wg_ppo_grad", o, params_dev, &sb, index_dev, first, n, hp, grad_out, stats_out, stream);
}

extern "C" int wg_ppo_apply(wg_ppo o, float* params_dev, const float* grad_dev, float lr, float max_grad_norm, void* stream) {
    if (!o || !params_dev || !grad_dev) return wg_fail(WG_ERR_INVALID, "wg_ppo_apply: null argument");
    if (!(max_grad_norm > 0.0f)) return wg_fail(WG_ERR_INVALID, "wg_ppo_apply: max_grad_norm must be > 0");
    if (int rc = wg_use_device(o->adam.device)) return rc;
    if (int rc = wg_on_device_all("wg_ppo_apply: ", "wg_ppo_apply: ", o->adam.device, {{params_dev, "params_dev", true}, {grad_dev, "grad_dev", true}}, ""))
        return rc;
    return t_apply(o, params_dev, grad_dev, lr, max_grad_norm, (hipStream_t)stream);
}

static int update_entry(const char* who, wg_ppo o, float* params_dev, const wg_ppo_batch_shared* b, const int32_t* perm_dev, int n_epochs,
                        int batch_size, const wg_ppo_hyper* hp, float lr, float max_grad_norm, wg_ppo_stats* stats_out, void* stream) {
    const std::string w = who;
    if (!o || !params_dev || !perm_dev) return wg_fail(WG_ERR_INVALID, w + ": null argument");
    if (int rc = t_check_batch(who, b, hp)) return rc;
    if (n_epochs < 1 || batch_size < 1) return wg_fail(WG_ERR_INVALID, w + ": n_epochs and batch_size must be >= 1");
    if (!(max_grad_norm > 0.0f)) return wg_fail(WG_ERR_INVALID, w + ": max_grad_norm must be > 0");
    if (int rc = t_use_device(w, o, params_dev, b)) return rc;
    if (int rc = wg_on_device(w + ": ", o->adam.device, perm_dev, "perm_dev", "")) return rc;
    const bool kl = o->adam.lr_dev != nullptr;                  // wg_ppo_set_kl_lr: the rate is the handle's device word, `lr` is ignored
    const int n_all = n_epochs * wg_n_minibatches(b->rows.n_rows, batch_size);
    return wg_each_minibatch(b->rows.n_rows, n_epochs, batch_size, [&](int mb, int64_t off, int n) {
        float* so = stats_out ? (float*)(stats_out + mb) : nullptr;
        if (int rc = t_grad(&o->g, params_dev, b, perm_dev + off, 0, n, hp, o->grad, so, (hipStream_t)stream)) return rc;
        if (kl) return t_apply_kl(o, params_dev, o->grad, so ? so : o->g.stats, mb, mb == n_all - 1, max_grad_norm, (hipStream_t)stream);
        return t_apply(o, params_dev, o->grad, lr, max_grad_norm, (hipStream_t)stream);
    });
}

extern "C" int wg_ppo_set_kl_lr(wg_ppo o, const wg_kl_lr* rule, float* lr_dev) {
    return wg_adam_set_kl_lr_(o ? &o->mem : nullptr, o ? &o->adam : nullptr, "wg_ppo_set_kl_lr", rule, lr_dev);
}

extern "C" int wg_ppo_update_shared(wg_ppo o, float* params_dev, const wg_ppo_batch_shared* b, const int32_t* perm_dev, int n_epochs,
                                    int batch_size, const wg_ppo_hyper* hp, float lr, float max_grad_norm, wg_ppo_stats* stats_out,
                                    void* stream) {
    return update_entry("wg_ppo_update_shared", o, params_dev, b, perm_dev, n_epochs, batch_size, hp, lr, max_grad_norm, stats_out, stream);
}

extern "C" int wg_ppo_update(wg_ppo o, float* params_dev, const wg_ppo_batch* b, const int32_t* perm_dev, int n_epochs,
                             int batch_size, const wg_ppo_hyper* hp, float lr, float max_grad_norm, wg_ppo_stats* stats_out,
                             void* stream) {
    if (!o || !b) return wg_fail(WG_ERR_INVALID, "wg_ppo_update: null argument");
    if (int rc = t_refuse_split("wg_ppo_update", o)) return rc;
    const wg_ppo_batch_shared sb = {*b, b->obs, 1};
    return update_entry("wg_ppo_update", o, params_dev, &sb, perm_dev, n_epochs, batch_size, hp, lr, max_grad_norm, stats_out, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// behaviour cloning (windgym_hip.h: wg_bc_*): the supervised gradient on the wg_ppo handle — its scratch, its Adam, wg_ppo_apply
// ---------------------------------------------------------------------------------------------------------------------
static int bc_check(const std::string& w, wg_ppo o, const float* params_dev, const wg_bc_batch* b, const wg_bc_hyper* hp) {
    if (!o || !params_dev || !b || !hp) return wg_fail(WG_ERR_INVALID, w + ": null argument");
    const WgPolicyP& P = o->g.pol->P;
    if (P.n_in_vf != P.n_in)             // as wg_ppo_grad refuses it: one obs stream of the actor's width, which the critic cannot read
        return wg_fail(WG_ERR_INVALID, w + ": the policy's critic reads rows of " + std::to_string(P.n_in_vf) + " inputs, its actor rows of " +
                                         std::to_string(P.n_in) + ": cloning a split policy (wg_policy_create_vf) is not implemented");
    if (!b->obs || !b->target) return wg_fail(WG_ERR_INVALID, w + ": a batch pointer is null (only returns may be)");
    if (b->n_rows < 1 || b->n_rows > 0x7fffffff) return wg_fail(WG_ERR_INVALID, w + ": n_rows out of range");
    if (hp->loss != WG_BC_MSE && hp->loss != WG_BC_NLL)
        return wg_fail(WG_ERR_INVALID, w + ": loss must be WG_BC_MSE or WG_BC_NLL, got " + std::to_string(hp->loss));
    if (int rc = wg_use_device(o->adam.device)) return rc;
    return wg_on_device_all(w + ": ", w + ": ", o->adam.device, {{params_dev, "params_dev", true}, {b->obs, "obs", true}, {b->target, "target", true}}, "");
}

// the launches of one supervised gradient, no argument checks
// (obs_vf: the rows the critic reads — b->obs for a plain batch; dh_pi / dh_vf both given: k_bc_grad_dh, which also writes the
// gradients of the gathered rows — wg_ppo_heads_bc_grad_)
static int t_bc_grad(WgPpoGrad* o, const float* params_dev, const wg_bc_batch* b, const float* obs_vf, const int32_t* index_dev, int64_t first,
                     int n, const wg_bc_hyper* hp, float* grad_out, float* stats_out, hipStream_t st, float* dh_pi = nullptr,
                     float* dh_vf = nullptr) {
    const WgPolicyP& P = o->pol->P;
    const int G = t_grid(o, n);
    const int has_ret = b->returns != nullptr, nll = hp->loss == WG_BC_NLL;
    WgPpoArgs a = {};
    a.packed = o->pol->w.packed; a.flat = params_dev; a.obs[0] = b->obs; a.obs[1] = obs_vf; a.agents = 1; a.raw = b->target;
    a.ret = b->returns; a.index = index_dev; a.first = first; a.n_total = b->n_rows; a.n = n; a.G = G;
    a.vf_coef = hp->vf_coef; a.part = o->part; a.spart = o->spart; a.bc_loss = hp->loss;
    a.dh[0] = dh_pi; a.dh[1] = dh_vf;
    if (dh_pi && dh_vf) hipLaunchKernelGGL(k_bc_grad_dh, dim3(G, has_ret ? 2 : 1), dim3(WGT_WAVES * 64), o->lds_bytes, st, P, o->K, a);
    else hipLaunchKernelGGL(k_bc_grad, dim3(G, has_ret ? 2 : 1), dim3(WGT_WAVES * 64), o->lds_bytes, st, P, o->K, a);
    hipLaunchKernelGGL(k_bc_reduce, dim3(o->n_blocks), dim3(WGT_BLOCK), 0, st, P, o->part, o->spart, G, n, P.layer[1][0].w_flat,
                       has_ret, nll, hp->vf_coef, hp->ent_coef, params_dev, grad_out, stats_out ? stats_out : o->stats);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_bc_grad(wg_ppo o, const float* params_dev, const wg_bc_batch* b, const int32_t* index_dev, int64_t first, int n,
                          const wg_bc_hyper* hp, float* grad_out, wg_bc_stats* stats_out, void* stream) {
    const std::string w = "wg_bc_grad";
    if (!grad_out) return wg_fail(WG_ERR_INVALID, w + ": null argument");
    if (int rc = bc_check(w, o, params_dev, b, hp)) return rc;
    if (n < 1) return wg_fail(WG_ERR_INVALID, w + ": n < 1");
    if (!index_dev && (first < 0 || first + n > b->n_rows)) return wg_fail(WG_ERR_INVALID, w + ": rows first .. first + n - 1 leave the batch");
    return t_bc_grad(&o->g, params_dev, b, b->obs, index_dev, first, n, hp, grad_out, (float*)stats_out, (hipStream_t)stream);
}

extern "C" int wg_bc_update(wg_ppo o, float* params_dev, const wg_bc_batch* b, const int32_t* perm_dev, int n_epochs, int batch_size,
                            const wg_bc_hyper* hp, float lr, float max_grad_norm, wg_bc_stats* stats_out, void* stream) {
    const std::string w = "wg_bc_update";
    if (!perm_dev) return wg_fail(WG_ERR_INVALID, w + ": null argument");
    if (int rc = bc_check(w, o, params_dev, b, hp)) return rc;
    if (n_epochs < 1 || batch_size < 1) return wg_fail(WG_ERR_INVALID, w + ": n_epochs and batch_size must be >= 1");
    if (!(max_grad_norm > 0.0f)) return wg_fail(WG_ERR_INVALID, w + ": max_grad_norm must be > 0");
    if (int rc = wg_on_device(w + ": ", o->adam.device, perm_dev, "perm_dev", "")) return rc;
    return wg_each_minibatch(b->n_rows, n_epochs, batch_size, [&](int mb, int64_t off, int n) {
        float* so = stats_out ? (float*)(stats_out + mb) : nullptr;
        if (int rc = t_bc_grad(&o->g, params_dev, b, b->obs, perm_dev + off, 0, n, hp, o->grad, so, (hipStream_t)stream)) return rc;
        return t_apply(o, params_dev, o->grad, lr, max_grad_norm, (hipStream_t)stream);
    });
}

// wg_internal.h: the supervised heads of a recurrent policy (wg_lstm_ppo.hip)
extern "C" int wg_ppo_heads_bc_grad_(WgPpoGrad* g, const float* mlp_params_dev, const float* h_pi, const float* h_vf, const float* target,
                                     const float* ret, int n, const wg_bc_hyper* hp, float* dh_pi, float* dh_vf, float* grad_out,
                                     float* stats_out, void* stream) {
    const wg_bc_batch b = {h_pi, target, ret, n};
    return t_bc_grad(g, mlp_params_dev, &b, h_vf, nullptr, 0, n, hp, grad_out, stats_out, (hipStream_t)stream, dh_pi, dh_vf);
}

// ---------------------------------------------------------------------------------------------------------------------
// populations (windgym_hip.h: wg_pop_*; the slot table and the launches of the policy kernel: wg_policy.hip)
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int wg_pop_create(const wg_policy* members, const wg_ppo* opts, int P, wg_pop* out) {
    if (!members || !out) return wg_fail(WG_ERR_INVALID, "wg_pop_create: null argument");
    *out = nullptr;
    if (int rc = wg_pop_count("wg_pop_create", P)) return rc;
    for (int m = 0; m < P; ++m) {
        const std::string who = "wg_pop_create: member " + std::to_string(m);
        if (!members[m]) return wg_fail(WG_ERR_INVALID, who + " is null");
        const WgPolicyP& Q = members[m]->P;
        if (Q.n_layers[1] != 0 && Q.n_in_vf != Q.n_in)
            return wg_fail(WG_ERR_INVALID, who + " is a split policy (its critic reads " + std::to_string(Q.n_in_vf) + " inputs, its actor " +
                                             std::to_string(Q.n_in) + "): populations take policies whose nets read the same rows");
        if (int rc = wg_pop_same_device(who, members[0]->w.device, "", members[m]->w.device)) return rc;
        if (!wgp_same_arch(members[0]->P, Q, true))
            return wg_fail(WG_ERR_INVALID, who + " has another architecture than member 0: the members of a population share one");
        if (int rc = wg_pop_given_twice(who, m, " is the same policy as member ", members)) return rc;
        if (opts) {
            if (!opts[m]) return wg_fail(WG_ERR_INVALID, who + ": its wg_ppo is null (opts = NULL makes a population that only acts)");
            if (opts[m]->g.pol != members[m]) return wg_fail(WG_ERR_INVALID, who + ": opts[" + std::to_string(m) + "] was created for another policy");
        }
    }
    wg_pop_s* q = new (std::nothrow) wg_pop_s();
    if (!q) return wg_fail(WG_ERR_NOMEM, "wg_pop_create: out of host memory");
    q->P = P;
    q->device = members[0]->w.device;
    for (int m = 0; m < P; ++m) { q->pol[m] = members[m]; q->opt[m] = opts ? opts[m] : nullptr; }
    q->mem.device = q->device;
    int rc = q->mem.alloc("wg_pop_create", &q->slots_dev, WGP_POP_SLOTS, false);
    if (!rc) rc = q->mem.alloc_bytes("wg_pop_create", &q->upd_dev, sizeof(WgPopMember) * WGP_POP_MAX, false);
    if (rc) {
        wg_pop_destroy(q);
        return rc;
    }
    *out = q;
    return 0;
}

extern "C" int wg_pop_destroy(wg_pop q) {
    if (!q) return 0;
    q->mem.release();
    delete q;
    return 0;
}

extern "C" int wg_gae_pop(int T, int B, int P, const float* reward_dev, const float* value_dev, const float* final_value_dev,
                          const uint8_t* truncated_dev, const float* gamma, const float* lambda, float* advantage_out,
                          float* returns_out, void* stream) {
    if (int rc = gae_check("wg_gae_pop", "T and B", "rows", reward_dev && value_dev && final_value_dev && truncated_dev && gamma && lambda &&
                           advantage_out && returns_out, T, B, 1, P))
        return rc;
    WgPopGae hy = {};
    for (int m = 0; m < P; ++m) { hy.gamma[m] = gamma[m]; hy.lambda[m] = lambda[m]; }
    hipLaunchKernelGGL(k_gae_pop, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, T, B, B / P, reward_dev, value_dev,
                       final_value_dev, truncated_dev, hy, advantage_out, returns_out);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_pop_update(wg_pop q, float* const* params_dev, const wg_ppo_batch* b, const int32_t* perm_dev, int n_epochs,
                             int batch_size, const wg_ppo_hyper* hp, const float* lr, const float* max_grad_norm,
                             wg_ppo_stats* stats_out, void* stream) {
    if (!q || !params_dev || !b || !perm_dev || !hp || !lr || !max_grad_norm) return wg_fail(WG_ERR_INVALID, "wg_pop_update: null argument");
    const int P = q->P;
    if (int rc = wg_pop_update_check("wg_pop_update", q->opt[0], n_epochs >= 1 && batch_size >= 1, "n_epochs and batch_size", P, params_dev, max_grad_norm))
        return rc;
    if (int rc = t_check_rows("wg_pop_update", b, b->obs)) return rc;
    if (int rc = wg_pop_shares("wg_pop_update", P, b->n_rows, "batch", "", " rows do")) return rc;
    if (int rc = wg_use_device(q->device)) return rc;
    for (int m = 0; m < P; ++m) {
        const std::string who = "wg_pop_update: member " + std::to_string(m);
        if (!(hp[m].clip_range >= 0.0f)) return wg_fail(WG_ERR_INVALID, who + ": clip_range < 0");
        if (int rc = wg_on_device(who + ": ", q->device, params_dev[m], "params_dev", "")) return rc;
    }
    if (int rc = wg_on_device_all("wg_pop_update: ", "wg_pop_update: ", q->device, {{b->obs, "obs", true}, {perm_dev, "perm_dev", true}}, "")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows_m = b->n_rows / P;
    const int n_mb = wg_n_minibatches(rows_m, batch_size);
    WgPopMember tab[WGP_POP_MAX] = {};
    WgAdam* adam[WGP_POP_MAX];
    for (int m = 0; m < P; ++m) adam[m] = &q->opt[m]->adam;
    int kl = 0;                                                 // the members' rates are their device words (every member or none), `lr` is ignored
    if (int rc = wg_pop_kl_lr_("wg_pop_update", P, adam, &kl)) return rc;
    bool any_norm = false;
    for (int m = 0; m < P; ++m) {
        wg_ppo_s* o = q->opt[m];
        WgPopMember& M = tab[m];
        wgt_pop_member_kl(M, o->adam);
        M.packed = o->g.pol->w.packed; M.params = params_dev[m];
        M.m = o->adam.m; M.v = o->adam.v; M.grad = o->grad; M.part = o->g.part; M.spart = o->g.spart; M.advstat = o->g.advstat; M.blocksq = o->adam.blocksq;
        M.perm = perm_dev + (size_t)m * n_epochs * rows_m;
        M.max_norm = max_grad_norm[m];
        any_norm = wgt_pop_member(M, hp, stats_out, m, n_epochs, n_mb, o->g.stats) || any_norm;
    }
    const WgPopMember* mt = (const WgPopMember*)q->upd_dev;
    if (int rc = wg_pop_store_(q->upd_dev, tab, sizeof(WgPopMember) * P, stream)) return rc;
    // every member has the architecture of member 0: one layer table, one LDS map, one G per minibatch size
    const WgPpoGrad* g0 = &q->opt[0]->g;
    const WgPolicyP& PP = g0->pol->P;
    return wg_each_minibatch(rows_m, n_epochs, batch_size, [&](int mb, int64_t off, int n) {
        const int G = t_grid(g0, n);
        if (any_norm && n > 1) hipLaunchKernelGGL(k_ppo_advstat_pop, dim3(P), dim3(1024), 0, st, mt, b->advantage, off, n, b->n_rows);
        WgPpoArgs a = {};
        a.obs[0] = b->obs; a.obs[1] = b->obs; a.agents = 1; a.raw = b->raw; a.logp_old = b->logp; a.adv = b->advantage; a.ret = b->returns;
        a.first = 0; a.n_total = b->n_rows; a.n = n; a.G = G;
        hipLaunchKernelGGL(k_ppo_grad_pop, dim3(G, 2, P), dim3(WGT_WAVES * 64), g0->lds_bytes, st, PP, g0->K, a, mt, off);
        hipLaunchKernelGGL(k_ppo_reduce_pop, dim3(g0->n_blocks, P), dim3(WGT_BLOCK), 0, st, PP, mt, G, n, mb);
        if (int rc = kl ? wg_adam_apply_kl_pop_(mt, P, adam, mb, mb == n_epochs * n_mb - 1, stream) : wg_adam_apply_pop_(mt, P, adam, lr, stream))
            return rc;
        wg_policy_pack_pop_(&PP, mt, P, stream);
        WG_HIPCHK(hipGetLastError());
        return 0;
    });
}
