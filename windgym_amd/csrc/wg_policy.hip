// wg_policy.hip — learned policies on the device: k_policy evaluates an MLP actor(-critic) on observation rows
// (what `model.predict(obs, deterministic=...)` of a stable-baselines3 MlpPolicy computes, WindGym/AgentEval.py:179-190),
// k_policy_pack builds the kernel's weight layout, and the wg_policy_* entries of include/windgym_hip.h wrap them.
//
// k_policy: one workgroup of 4 waves owns 32 observation rows of ONE net (a launch is up to three slots of (net, rows)).  A layer is
// D[neuron][row] = sum_k W[neuron][k] X[k][row] on the tile core of wg_tile.h — an exact k-ordered f32 fmaf chain, so a row's
// outputs depend on nothing but that row and the weights (bitwise: no atomics, no cross-row reduction, fixed order).
// X lives in LDS as [k][32 rows], the weights come packed from L2 as the A operand,
// the 32 x 32 result tile of wave w (tiles w and w + 4) gets bias (accumulator init) and activation
// and goes to the other LDS buffer: hidden activations never leave the CU.  The first layer streams the observations
// through LDS in chunks of 256 inputs (n_in <= 2048).  The head's tile is the action mean / the value.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>

#include "../../include/windgym_hip.h"
#include "wg_policy.h"
#include "wg_host.h"

// Philox4x32-10 (the generator of wg_device.h's sensor noise) -> the first two output words
__device__ inline void wgp_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t& o0,
                                  uint32_t& o1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o0 = c0; o1 = c1;
}

// eps_j of global row g (wg_policy.h: NOISE)
__device__ inline float wgp_noise(uint64_t seed, uint64_t counter, uint64_t g, int j) {
    uint32_t a, b;
    wgp_philox((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)g, (uint32_t)counter, (uint32_t)(counter >> 32),
               WGP_NOISE_TAG | ((uint32_t)(g >> 32) & 0xffffu) << 8 | (uint32_t)(j >> 1), a, b);
    const float u1 = ((float)(a >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    const float ph = 6.2831853071795864f * u2;
    return r * ((j & 1) ? sinf(ph) : cosf(ph));
}

// One workgroup of k_policy / k_policy_pop: 32 rows (from row0) of ONE net on `n_rows` rows of `obs`.  The actor's outputs and the
// noise rows are relative to the slot: action / raw / logp point at the slot's first row, row_offset is that row's global index.
__device__ __forceinline__ void wgp_tile(const WgPolicyP& P, const float* __restrict__ packed, const float* __restrict__ obs,
                                         float* __restrict__ value, const int net, const int n_rows, const int row0,
                                         const int deterministic, const uint64_t seed, const uint64_t counter, const uint64_t row_offset,
                                         float* __restrict__ action, float* __restrict__ raw, float* __restrict__ logp) {
    __shared__ float lds[2][WGP_KC * WGP_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int L = P.n_layers[net];
    int cur = 0;                                  // LDS buffer that holds the running layer's input
    for (int l = 0; l < L; ++l) {
        const WgPolicyLayer ly = P.layer[net][l];
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int ot = wave + WGP_WAVES * t;
            if (ot < ly.ntiles) wg_tile_bias(acc[t], packed + ly.b_packed + ot * 32, h);
        }
        const int nchunk = l == 0 ? (ly.K + WGP_KC - 1) / WGP_KC : 1;
        for (int c = 0; c < nchunk; ++c) {
            const int k0 = c * WGP_KC;
            const int kc = min(WGP_KC, ly.K - k0), kcp = wg_tile_kpad(kc);
            if (l == 0) {
                // observations -> LDS (the 32 rows' cache lines are re-used from L1 by the following passes); rows past n_rows read as 0
                const int row = row0 + r;
                const float* orow = obs + (size_t)row * ly.K + k0;      // (a net's row stride is its first layer's K)
                wg_tile_stage(lds[0], tid, kcp, [&](const int k) { return (row < n_rows && k < kc) ? orow[k] : 0.0f; });
            }
            const float* xb = lds[cur] + h * WGP_TILE + r;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int ot = wave + WGP_WAVES * t;
                if (ot < ly.ntiles)
                    wg_tile_gemm(acc[t], packed + ly.w_packed + ((size_t)ot * ly.nks + (k0 >> 1)) * 64 + lane, xb, kcp >> 1);
            }
        }
        float* dst = lds[cur ^ 1];
        const bool head = l == L - 1;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int ot = wave + WGP_WAVES * t;
            if (ot < ly.ntiles) {
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    float v = acc[t][g];
                    if (!head) v = P.activation == WG_ACTV_RELU ? fmaxf(v, 0.0f) : tanhf(v);
                    dst[(ot * 32 + wg_tile_drow(g, h)) * WGP_TILE + r] = v;
                }
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    float* mb = lds[cur];                         // [output][row]: action means / the value
    const int nvalid = min(WGP_TILE, n_rows - row0);
    if (net == 1) {
        if (tid < nvalid) value[row0 + tid] = mb[tid];
        return;
    }
    const int n_out = P.n_out;
    for (int idx = tid; idx < nvalid * n_out; idx += WGP_WAVES * 64) {      // idx = row * n_out + j: coalesced stores
        const int row = idx / n_out, j = idx - row * n_out;
        const float mean = mb[j * WGP_TILE + row];
        const float ls = P.has_log_std ? packed[P.log_std_packed + j] : 0.0f;
        const float eps = deterministic ? 0.0f : wgp_noise(seed, counter, row_offset + (uint64_t)(row0 + row), j);
        const float rw = mean + expf(ls) * eps;
        const size_t o = (size_t)row0 * n_out + idx;
        if (raw) raw[o] = rw;
        if (action) action[o] = fminf(fmaxf(rw, -1.0f), 1.0f);
        mb[j * WGP_TILE + row] = -0.5f * eps * eps - ls - 0.91893853320467274f;
    }
    if (logp) {                                   // sum over j in index order by ONE thread per row
        __syncthreads();
        if (tid < nvalid) {
            float s = 0.0f;
            for (int j = 0; j < n_out; ++j) s += mb[j * WGP_TILE + tid];
            logp[row0 + tid] = s;
        }
    }
}

__global__ __launch_bounds__(WGP_WAVES * 64) void k_policy(const WgPolicyP P, const float* __restrict__ packed,
                                                           const WgPolicySlots S, const int deterministic, const uint64_t seed,
                                                           const uint64_t counter, const uint64_t row_offset,
                                                           float* __restrict__ action, float* __restrict__ raw,
                                                           float* __restrict__ logp) {
    // blockIdx.x -> (slot, tile of 32 rows): slot s owns the workgroups [end[s - 1], end[s]) (wg_policy.h: WgPolicySlots; an unused
    // slot has end[s] = end[s - 1]).  A 1-D grid of exactly the tiles each slot has: the slots of the closed loop differ by a factor
    // n_turb in rows (the actor on B * N agent rows, the critic on B env rows, wg_rollout_multi's central mode), so a 2-D grid
    // (tiles of the largest slot) x slots would launch mostly workgroups that have nothing to do.
    const int bid = blockIdx.x;
    const int slot = (bid >= S.end[0] ? 1 : 0) + (bid >= S.end[1] ? 1 : 0);
    const int row0 = (bid - (slot ? S.end[slot - 1] : 0)) * WGP_TILE;
    wgp_tile(P, packed, S.obs[slot], S.value[slot], S.net[slot], S.n_rows[slot], row0, deterministic, seed, counter, row_offset, action,
             raw, logp);
}

// The population's launch: slots [first_slot, first_slot + gridDim.x / tiles) of the table, each a member's net on ITS n_rows rows
// with ITS weights, seed and row offset (wg_policy.h: WgPopSlot).  The slot is a function of blockIdx.x alone, so the table is
// read through scalar loads; what a workgroup then computes is wgp_tile on the member's pointers — the arithmetic of k_policy.
__global__ __launch_bounds__(WGP_WAVES * 64) void k_policy_pop(const WgPolicyP P, const WgPopSlot* __restrict__ slots,
                                                               const int first_slot, const int tiles, const int n_rows, const int t,
                                                               const int deterministic, const uint64_t counter) {
    const int bid = blockIdx.x, sl = bid / tiles;
    const WgPopSlot* __restrict__ s = slots + first_slot + sl;
    const int64_t tt = (int64_t)t + s->t_shift;
    float* const value = s->value ? s->value + tt * s->row_step : nullptr;
    float* const action = s->action ? s->action + tt * s->act_step : nullptr;
    float* const raw = s->raw ? s->raw + tt * s->act_step : nullptr;
    float* const logp = s->logp ? s->logp + tt * s->row_step : nullptr;
    wgp_tile(P, s->packed, s->obs + tt * s->obs_step, value, s->net, n_rows, (bid - sl * tiles) * WGP_TILE, deterministic, s->seed,
             counter, s->row_offset, action, raw, logp);
}

// flat -> packed (wg_policy.h); one thread per packed float
__device__ __forceinline__ void wgp_pack(const WgPolicyP& P, const float* __restrict__ flat, float* __restrict__ packed) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P.n_packed) return;
    float v = 0.0f;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < P.n_layers[net]; ++l) {
            const WgPolicyLayer ly = P.layer[net][l];
            if (idx >= ly.w_packed && idx < ly.w_packed + wg_tile_wsize(ly.ntiles, ly.nks)) {
                const WgTileElem e = wg_tile_decode(idx - ly.w_packed, ly.nks);
                const uint32_t i = e.tile * 32 + e.j;
                if (i < (uint32_t)ly.M && e.k < (uint32_t)ly.K) v = flat[ly.w_flat + (size_t)i * ly.K + e.k];
            } else if (idx >= ly.b_packed && idx < ly.b_packed + wg_tile_bsize(ly.ntiles)) {
                const uint32_t i = idx - ly.b_packed;
                if (i < (uint32_t)ly.M) v = flat[ly.b_flat + i];
            }
        }
    if (P.has_log_std && idx >= P.log_std_packed && idx < P.log_std_packed + (uint32_t)P.n_out)
        v = flat[P.log_std_flat + (idx - P.log_std_packed)];
    packed[idx] = v;
}

__global__ void k_policy_pack(const WgPolicyP P, const float* __restrict__ flat, float* __restrict__ packed) { wgp_pack(P, flat, packed); }

// every member of a population: blockIdx.y = member, params -> its policy's packed copy
__global__ void k_policy_pack_pop(const WgPolicyP P, const WgPopMember* __restrict__ mt) {
    const WgPopMember* __restrict__ M = mt + blockIdx.y;
    wgp_pack(P, M->params, const_cast<float*>(M->packed));
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// A handle's device copies (wg_tile.h: WgPacked): the zeroed packed vector and the staging copy, on mem's device
extern "C" int wg_packed_alloc_(WgDevMem* mem, WgPacked* w, uint32_t n_flat, uint32_t n_packed, const char* who) {
    *w = WgPacked{mem->device, nullptr, nullptr, n_flat, n_packed};
    if (int rc = mem->alloc(who, &w->packed, n_packed)) return rc;
    return mem->alloc(who, &w->flat_stage, n_flat, false);
}

// what the pack kernel of a set_params reads: a device pointer itself, a host pointer's copy in the stage (in stream order)
extern "C" int wg_packed_source_(WgPacked* w, const float* params, int on_device, hipStream_t st, const float** src) {
    if (int rc = wg_use_device(w->device)) return rc;
    *src = params;
    if (on_device) return 0;
    WG_HIPCHK(hipMemcpyAsync(w->flat_stage, params, sizeof(float) * w->n_flat, hipMemcpyHostToDevice, st));
    *src = w->flat_stage;
    return 0;
}

extern "C" int wg_policy_create_vf(const wg_policy_desc* d, int32_t n_in_vf, int device, wg_policy* out) {
    if (!d || !out) return wg_fail(WG_ERR_INVALID, "wg_policy_create: null argument");
    *out = nullptr;
    if (d->n_in < 1 || d->n_out < 1) return wg_fail(WG_ERR_INVALID, "wg_policy_create: n_in and n_out must be >= 1");
    if (d->n_in > WGP_MAX_IN) return wg_fail(WG_ERR_UNSUPPORTED, "wg_policy_create: n_in = " + std::to_string(d->n_in) + " > " + std::to_string(WGP_MAX_IN));
    if (d->n_out > WGP_MAX_OUT) return wg_fail(WG_ERR_UNSUPPORTED, "wg_policy_create: n_out = " + std::to_string(d->n_out) + " > " + std::to_string(WGP_MAX_OUT));
    if (d->activation != WG_ACTV_TANH && d->activation != WG_ACTV_RELU) return wg_fail(WG_ERR_INVALID, "wg_policy_create: unknown activation");
    if (d->n_hidden_pi < 0) return wg_fail(WG_ERR_INVALID, "wg_policy_create: n_hidden_pi < 0");
    if (d->n_hidden_vf < 0 && n_in_vf != d->n_in)
        return wg_fail(WG_ERR_INVALID, "wg_policy_create_vf: n_in_vf is the input width of the critic, and this policy has none (n_hidden_vf < 0)");
    if (n_in_vf < 1) return wg_fail(WG_ERR_INVALID, "wg_policy_create_vf: n_in_vf must be >= 1");
    if (n_in_vf > WGP_MAX_IN) return wg_fail(WG_ERR_UNSUPPORTED, "wg_policy_create_vf: n_in_vf = " + std::to_string(n_in_vf) + " > " + std::to_string(WGP_MAX_IN));
    const int nh[2] = {d->n_hidden_pi, d->n_hidden_vf};
    const int32_t* hid[2] = {d->hidden_pi, d->hidden_vf};
    for (int net = 0; net < 2; ++net) {
        if (nh[net] > WG_POLICY_MAX_HIDDEN)
            return wg_fail(WG_ERR_UNSUPPORTED, "wg_policy_create: " + std::to_string(nh[net]) + " hidden layers > " + std::to_string(WG_POLICY_MAX_HIDDEN));
        for (int l = 0; l < nh[net]; ++l) {
            if (hid[net][l] < 1) return wg_fail(WG_ERR_INVALID, "wg_policy_create: hidden width < 1");
            if (hid[net][l] > WGP_MAX_WIDTH)
                return wg_fail(WG_ERR_UNSUPPORTED, "wg_policy_create: hidden width " + std::to_string(hid[net][l]) + " > " + std::to_string(WGP_MAX_WIDTH));
        }
    }
    wg_policy_s* p = new (std::nothrow) wg_policy_s();
    if (!p) return wg_fail(WG_ERR_NOMEM, "wg_policy_create: out of host memory");
    wgp_fill_layout(p->P, d, n_in_vf);
    p->mem.device = device;
    if (int rc = wg_packed_alloc_(&p->mem, &p->w, p->P.n_flat, p->P.n_packed, "wg_policy_create")) {
        wg_policy_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

extern "C" int wg_policy_create(const wg_policy_desc* d, int device, wg_policy* out) {
    if (!d || !out) return wg_fail(WG_ERR_INVALID, "wg_policy_create: null argument");
    return wg_policy_create_vf(d, d->n_in, device, out);
}

extern "C" int wg_policy_destroy(wg_policy p) {
    if (!p) return 0;
    p->mem.release();
    delete p;
    return 0;
}

extern "C" int wg_policy_n_params(wg_policy p, size_t* n) {
    if (!p || !n) return wg_fail(WG_ERR_INVALID, "wg_policy_n_params: null argument");
    *n = p->P.n_flat;
    return 0;
}

extern "C" int wg_policy_set_params(wg_policy p, const float* params, size_t n, int on_device, void* stream) {
    if (!p || !params) return wg_fail(WG_ERR_INVALID, "wg_policy_set_params: null argument");
    if (n != p->P.n_flat)
        return wg_fail(WG_ERR_INVALID, "wg_policy_set_params: " + std::to_string(n) + " parameters given, the policy has " + std::to_string(p->P.n_flat));
    hipStream_t st = (hipStream_t)stream;
    const float* src;
    if (int rc = wg_packed_source_(&p->w, params, on_device, st, &src)) return rc;
    hipLaunchKernelGGL(k_policy_pack, dim3((p->P.n_packed + 255) / 256), dim3(256), 0, st, p->P, src, p->w.packed);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

// One launch of k_policy: the actor on n_rows rows of n_in (when one of its outputs is wanted) and the critic on each of the
// n_v <= 2 row sets of v (rows of n_in_vf).  What wg_policy_act checks about the policy is checked here.
extern "C" int wg_policy_eval_(wg_policy p, int n_rows, const float* obs_dev, int deterministic, uint64_t seed, uint64_t counter,
                               uint64_t row_offset, float* action_dev, float* raw_dev, float* logp_dev, const WgValueRows* v, int n_v,
                               void* stream) {
    if (!p) return wg_fail(WG_ERR_INVALID, "wg_policy_act: null argument");
    if (n_v < 0 || n_v > WGP_MAX_SLOTS - 1 || (n_v > 0 && !v))
        return wg_fail(WG_ERR_INVALID, "wg_policy_act: a launch takes at most " + std::to_string(WGP_MAX_SLOTS - 1) + " row sets for the critic");
    const bool actor = action_dev || raw_dev || logp_dev;
    if (n_v > 0 && p->P.n_layers[1] == 0) return wg_fail(WG_ERR_INVALID, "wg_policy_act: value requested from a policy without a critic");
    if (actor && !p->P.has_log_std && (!deterministic || logp_dev))
        return wg_fail(WG_ERR_INVALID, "wg_policy_act: a stochastic action / a log-probability needs a policy with log_std");
    WgPolicySlots S = {};
    int ns = 0, end = 0;
    if (actor && n_rows > 0) {
        S.obs[ns] = obs_dev; S.n_rows[ns] = n_rows; S.net[ns] = 0;
        S.end[ns++] = end += (n_rows + WGP_TILE - 1) / WGP_TILE;
    }
    for (int i = 0; i < n_v; ++i) {
        if (v[i].n_rows <= 0) continue;
        S.obs[ns] = v[i].obs; S.value[ns] = v[i].value; S.n_rows[ns] = v[i].n_rows; S.net[ns] = 1;
        S.end[ns++] = end += (v[i].n_rows + WGP_TILE - 1) / WGP_TILE;
    }
    if (ns == 0) return 0;
    for (int i = ns; i < WGP_MAX_SLOTS; ++i) S.end[i] = end;
    if (int rc = wg_use_device(p->w.device)) return rc;
    hipLaunchKernelGGL(k_policy, dim3(end), dim3(WGP_WAVES * 64), 0, (hipStream_t)stream, p->P, p->w.packed, S, deterministic ? 1 : 0,
                       seed, counter, row_offset, action_dev, raw_dev, logp_dev);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("wg_policy_act: kernel launch failed: ") + hipGetErrorString(le));
    return 0;
}

extern "C" int wg_policy_act(wg_policy p, int n_rows, const float* obs_dev, int deterministic, uint64_t seed, uint64_t counter,
                             uint64_t row_offset, float* action_dev, float* raw_dev, float* logp_dev, float* value_dev,
                             void* stream) {
    if (!p || !obs_dev) return wg_fail(WG_ERR_INVALID, "wg_policy_act: null argument");
    if (n_rows < 0) return wg_fail(WG_ERR_INVALID, "wg_policy_act: n_rows < 0");
    if (value_dev && (action_dev || raw_dev || logp_dev) && p->P.n_layers[1] != 0 && p->P.n_in_vf != p->P.n_in)
        return wg_fail(WG_ERR_INVALID, "wg_policy_act: the actor of this policy reads rows of " + std::to_string(p->P.n_in) +
                                         " inputs and its critic rows of " + std::to_string(p->P.n_in_vf) +
                                         ", so one obs_dev cannot serve both: ask for the value in a call of its own");
    const WgValueRows v = {obs_dev, value_dev, n_rows};
    return wg_policy_eval_(p, n_rows, obs_dev, deterministic, seed, counter, row_offset, action_dev, raw_dev, logp_dev, &v,
                           value_dev ? 1 : 0, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// populations: the slot table of k_policy_pop and its launches (wg_pop_create / wg_pop_destroy: wg_ppo.hip)
// ---------------------------------------------------------------------------------------------------------------------
// A host table -> device memory in stream order WITHOUT a copy engine or a host synchronisation (a hipMemcpyAsync from pageable
// memory waits for the stream): the bytes travel as kernel arguments, 2 KB per launch, and one thread per word stores them.
struct WgPopWords { uint32_t w[512]; };
__global__ void k_pop_store(const WgPopWords c, uint32_t* __restrict__ dst, const int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = c.w[i];
}

extern "C" int wg_pop_store_(void* dst_dev, const void* src_host, size_t bytes, void* stream) {
    for (size_t o = 0; o < bytes; o += sizeof(WgPopWords)) {
        WgPopWords c;
        const size_t nb = bytes - o < sizeof(WgPopWords) ? bytes - o : sizeof(WgPopWords);
        memcpy(c.w, (const char*)src_host + o, nb);
        hipLaunchKernelGGL(k_pop_store, dim3(2), dim3(256), 0, (hipStream_t)stream, c, (uint32_t*)((char*)dst_dev + o), (int)((nb + 3) / 4));
    }
    WG_HIPCHK(hipGetLastError());
    return 0;
}

// k_policy_pack for every member of the table (wg_pop_update: after Adam's step)
extern "C" void wg_policy_pack_pop_(const WgPolicyP* P, const WgPopMember* mt, int n_members, void* stream) {
    hipLaunchKernelGGL(k_policy_pack_pop, dim3((P->n_packed + 255) / 256, n_members), dim3(256), 0, (hipStream_t)stream, *P, mt);
}

// Write the slot table for `n_rows` rows of observations split evenly among the members: P actor slots (when an actor output is
// wanted), P critic slots (o->value), P critic slots on the final rows (o->final_value), in this order, stored in stream order
// (launches enqueued before on the same stream still read the old table: a population is used on one stream at a time).
extern "C" int wg_pop_prepare_(wg_pop q, const char* who, int n_rows, const uint64_t* seeds, const uint64_t* row_offsets, const float* obs,
                               const float* final_obs, const WgPopOuts* o, void* stream) {
    const std::string w = who;
    const WgPolicyP& P = q->pol[0]->P;
    if (n_rows < 0) return wg_fail(WG_ERR_INVALID, w + ": n_rows < 0");
    if (int rc = wg_pop_shares(w, q->P, n_rows, "rows", "", " rows do")) return rc;
    const bool actor = o->action || o->raw || o->logp;
    if ((o->value || o->final_value) && P.n_layers[1] == 0) return wg_fail(WG_ERR_INVALID, w + ": value requested from policies without a critic");
    if (actor && !seeds) return wg_fail(WG_ERR_INVALID, w + ": seeds[P] is required");
    const WgPopKind kinds[3] = {{obs, P.n_in, o->step * P.n_in}, {obs, P.n_in_vf, o->step * P.n_in_vf}, {final_obs, P.n_in_vf, o->step * P.n_in_vf}};
    return wg_pop_slots_(q, n_rows / q->P, kinds, o, seeds, row_offsets, stream);
}

// wgp_pop_slots (wg_policy.h) for the members of q on Bm rows each: the table's shape into q, the table into q->slots_dev
extern "C" int wg_pop_slots_(wg_pop q, int Bm, const WgPopKind* kinds, const WgPopOuts* o, const uint64_t* seeds, const uint64_t* row_offsets,
                             void* stream) {
    const float* packed[WGP_POP_MAX];
    for (int m = 0; m < q->P; ++m) packed[m] = q->pol[m]->w.packed;
    WgPopSlot tab[WGP_POP_SLOTS] = {};
    const WgPopShape s = wgp_pop_slots(tab, q->P, Bm, q->pol[0]->P.n_out, packed, kinds, *o, seeds, row_offsets);
    q->n_head = s.n_head; q->has_final = s.has_final; q->Bm = s.Bm;
    if (s.ns == 0 || Bm == 0) return 0;
    if (int rc = wg_use_device(q->device)) return rc;
    return wg_pop_store_(q->slots_dev, tab, sizeof(WgPopSlot) * s.ns, stream);
}

// ONE launch of k_policy_pop on the prepared table: the kinds of step t's own rows (`head`: actor and / or critic) and / or the
// critic on the final rows of step t - 1 (`fin`)
extern "C" int wg_pop_launch_(wg_pop q, int head, int fin, int t, int deterministic, uint64_t counter, void* stream) {
    const int kinds = (head ? q->n_head : 0) + (fin ? q->has_final : 0);
    if (kinds == 0 || q->Bm == 0) return 0;
    const int first = head ? 0 : q->n_head * q->P, tiles = (q->Bm + WGP_TILE - 1) / WGP_TILE;
    if (int rc = wg_use_device(q->device)) return rc;
    hipLaunchKernelGGL(k_policy_pop, dim3(kinds * q->P * tiles), dim3(WGP_WAVES * 64), 0, (hipStream_t)stream, q->pol[0]->P, q->slots_dev,
                       first, tiles, q->Bm, t, deterministic ? 1 : 0, counter);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("wg_pop: kernel launch failed: ") + hipGetErrorString(le));
    return 0;
}

extern "C" int wg_pop_act(wg_pop q, int n_rows, const float* obs_dev, int deterministic, const uint64_t* seeds, uint64_t counter,
                          const uint64_t* row_offsets, float* action_dev, float* raw_dev, float* logp_dev, float* value_dev, void* stream) {
    if (!q || !obs_dev) return wg_fail(WG_ERR_INVALID, "wg_pop_act: null argument");
    const WgPolicyP& P = q->pol[0]->P;
    if ((action_dev || raw_dev || logp_dev) && !P.has_log_std && (!deterministic || logp_dev))
        return wg_fail(WG_ERR_INVALID, "wg_pop_act: a stochastic action / a log-probability needs policies with log_std");
    const WgPopOuts o = {action_dev, raw_dev, logp_dev, value_dev, nullptr, 0};
    if (int rc = wg_pop_prepare_(q, "wg_pop_act", n_rows, seeds, row_offsets, obs_dev, nullptr, &o, stream)) return rc;
    return wg_pop_launch_(q, 1, 0, 0, deterministic, counter, stream);
}
