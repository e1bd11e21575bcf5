// wg_tile.h — the MFMA tile core of k_policy, k_lstm and ppo_grad's forward pass: the packed weight layout and the GEMM over it,
// stated once.  The layout half is plain C++ (g++ alone compiles it: tests/test_tile_layout.py); the device half needs hipcc.
//
// A GEMM D[M][32 rows] = W[M][K] X[K][32 rows] runs on v_mfma_f32_32x32x2_f32 in output tiles of 32 rows of W, two k per step.
// A BLOCK is the packed copy of `ntiles` such tiles over nks k-steps:
//     Wp[tile][ks][lane] = W[row(tile, lane & 31)][2 ks + (lane >> 5)]          (0 where W has no such row or k: padding)
//         — the A operand of output tile `tile`, k-step `ks`: one coalesced 256-byte load per wave;
//     bp[tile][j]        = b[row(tile, j)]                                       (0 for padding rows),
// with row(tile, j) = 32 tile + j for an MLP layer; the LSTM has its own map (wg_lstm.h).  A packed vector is blocks back to
// back and WGP_SLACK zeros behind the last.
//
// THE THREE PADDING INVARIANTS of wg_tile_gemm, which has no bounds test:
//   1. nks = ceil(K / 2) rounded up to PAIRS of groups of WGP_GROUP k-steps, the k-steps behind K holding zero weights
//      (wg_tile_nks; the pack kernels write the zeros);
//   2. the staged rows [k][32] behind a chunk's kc inputs, up to wg_tile_kpad(kc), hold zeros (whoever stages writes them);
//   3. the packed vector ends in one group of slack (WGP_SLACK floats): the loop's last prefetch reads one group past its tile.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define WG_TILE_HD __host__ __device__ __forceinline__
#else
#define WG_TILE_HD inline
#endif

#define WGP_TILE 32          // rows of a workgroup's batch tile = columns of one MFMA; output rows per MFMA tile
#define WGP_KC 256           // inputs staged per chunk = widest hidden layer
#define WGP_WAVES 4          // waves per workgroup; wave w computes output tiles (unit blocks) w and w + 4
#define WGP_GROUP 8          // k-steps per software-pipeline group of the MFMA loop
#define WGP_SLACK (WGP_GROUP * 64)   // invariant 3

WG_TILE_HD int32_t wg_tile_nks(int32_t K) { return ((K + 1) / 2 + 2 * WGP_GROUP - 1) / (2 * WGP_GROUP) * (2 * WGP_GROUP); }
WG_TILE_HD int32_t wg_tile_count(int32_t M) { return (M + 31) / 32; }
WG_TILE_HD uint32_t wg_tile_wsize(int32_t ntiles, int32_t nks) { return (uint32_t)ntiles * (uint32_t)nks * 64; }
WG_TILE_HD uint32_t wg_tile_bsize(int32_t ntiles) { return (uint32_t)ntiles * 32; }
// inputs of a staged chunk of kc, padding included: whole pairs of groups of k-steps (invariant 2)
WG_TILE_HD int32_t wg_tile_kpad(int32_t kc) { return (kc + 4 * WGP_GROUP - 1) & ~(4 * WGP_GROUP - 1); }

// packed element e of a weight block of nks k-steps -> its tile, its row j within the tile and its k.  The caller maps
// (tile, j) to a row of W and reads 0 where there is no such row or k >= K.
struct WgTileElem { uint32_t tile, j, k; };
WG_TILE_HD WgTileElem wg_tile_decode(uint32_t e, uint32_t nks) {
    const uint32_t lane = e & 63, ks = (e >> 6) % nks;
    return {(e >> 6) / nks, lane & 31, 2 * ks + (lane >> 5)};
}

// A handle's device copies of its parameters (wg_policy_s, wg_lstm_s; wg_internal.h: wg_packed_*_)
struct WgPacked {
    int device;
    float* packed;             // [n_packed] what the kernels read, zero wherever the pack kernel has not written
    float* flat_stage;         // [n_flat] staging copy for a set_params from a host pointer
    uint32_t n_flat, n_packed;
};

#ifdef __HIPCC__
typedef float f32x16 __attribute__((ext_vector_type(16)));

// D: lane = (batch row lane & 31, half h = lane >> 5); its register g holds row wg_tile_drow(g, h) of the output tile
__device__ __forceinline__ int wg_tile_drow(const int g, const int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

// the accumulator of one output tile starts from the tile's bias (bp: its 32 packed biases)
__device__ __forceinline__ void wg_tile_bias(f32x16& acc, const float* __restrict__ bp, const int h) {
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = bp[wg_tile_drow(g, h)];
}

// Stage one chunk into LDS as [k][32 rows] (B operand: one conflict-free ds_read per k-step): a wave covers 32 rows x 2 inputs
// per pass with conflict-free stores.  src(k) is the value of this thread's row at input k of the chunk — and 0 for k >= kc, for
// rows that do not exist: invariant 2 is the callable's.
template <class Src>
__device__ __forceinline__ void wg_tile_stage(float* __restrict__ lds, const int tid, const int kcp, Src src) {
    __syncthreads();
    for (int k = tid >> 5; k < kcp; k += WGP_WAVES * 2) lds[k * WGP_TILE + (tid & 31)] = src(k);
    __syncthreads();
}

// One output tile over one staged chunk: nks k-steps (a multiple of 2 WGP_GROUP) of A operands from wp (this lane's element of
// the tile's first k-step), B operands from xb (this lane's: staged chunk + (lane >> 5) * WGP_TILE + (lane & 31)).  An exact
// k-ordered f32 fmaf chain.  k-steps in groups of WGP_GROUP: the A operands of group g + 1 (global loads, L2 latency) are requested
// before the MFMAs of group g issue; the B operands are LDS reads of the group itself.  The roles of a0 / a1 are fixed, so that no
// register copy waits for the prefetch.  No bounds tests: the three invariants above.
__device__ __forceinline__ void wg_tile_gemm(f32x16& acc, const float* __restrict__ wp, const float* __restrict__ xb, const int nks) {
    float a0[WGP_GROUP], a1[WGP_GROUP], b[WGP_GROUP];
#pragma unroll
    for (int i = 0; i < WGP_GROUP; ++i) a0[i] = wp[i * 64];
    for (int ks0 = 0; ks0 < nks; ks0 += 2 * WGP_GROUP) {
#pragma unroll
        for (int i = 0; i < WGP_GROUP; ++i) {
            a1[i] = wp[(size_t)(ks0 + WGP_GROUP + i) * 64];
            b[i] = xb[(ks0 + i) * 2 * WGP_TILE];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < WGP_GROUP; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i], b[i], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < WGP_GROUP; ++i) {
            a0[i] = wp[(size_t)(ks0 + 2 * WGP_GROUP + i) * 64];
            b[i] = xb[(ks0 + WGP_GROUP + i) * 2 * WGP_TILE];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < WGP_GROUP; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[i], b[i], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}
#endif
