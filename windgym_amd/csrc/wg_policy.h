// wg_policy.h — parameter block of k_policy (wg_policy.hip) and the host object behind the `wg_policy` handle.
//
// A policy is up to two independent MLPs ("nets"): 0 = actor (n_in -> hidden_pi... -> n_out), 1 = critic
// (n_in_vf -> hidden_vf... -> 1; n_in_vf = n_in unless the policy was built by wg_policy_create_vf: a "split" policy, whose
// critic reads other rows than its actor).  Layer l of a net maps K inputs to M outputs; PyTorch's Linear.weight orientation
// W[M][K] in the caller's flat vector.  A net's input width — the stride of the rows it reads — is its first layer's K.
//
// FLAT parameter vector (what wg_policy_set_params takes; windgym_amd/policy.py and oracle/policy_oracle.py restate it):
//     actor hidden layers in order, each W [M][K] row-major then b [M]; actor head W [n_out][K], b [n_out];
//     critic hidden layers, critic head W [1][K], b [1] (only with a critic); log_std [n_out] (only with has_log_std).
//
// PACKED copy (what the kernel reads; owned by the policy object, written by k_policy_pack): per layer
//     Wp[tile][ks][lane]  = W[32 tile + (lane & 31)][2 ks + (lane >> 5)]   (0 outside M x K; ks < nks, 16 k-steps at a time)
//         — the A operand of v_mfma_f32_32x32x2_f32 for output tile `tile`, k-step `ks`: one coalesced 256-byte load;
//     bp[i], i < 32 n_tiles = b[i]                                              (0 from M on),
// then log_std [n_out] and one k-group of zeros.  Padding lives here, never in the caller's tensors.
//
// NOISE of a stochastic call (restated in oracle/policy_oracle.py: policy_noise): Philox4x32-10 with
//     key     = (seed lo, seed hi)
//     counter = (g lo, counter lo, counter hi, 0x50000000 | ((g hi) & 0xffff) << 8 | (j >> 1)),   g = row + row_offset,
// words (o0, o1) of the output give u1 = ((o0 >> 8) + 1) / 2^24 in (0, 1], u2 = (o1 >> 8) / 2^24 in [0, 1) and
//     eps_j = sqrt(-2 ln u1) * (j even ? cos(2 pi u2) : sin(2 pi u2))                         (float32 arithmetic).
#ifndef WG_POLICY_H
#define WG_POLICY_H
#include <stdint.h>

#define WGP_TILE 32          // rows of a workgroup's batch tile = columns of one MFMA; output neurons per MFMA tile
#define WGP_KC 256           // inputs staged per chunk of the first layer = widest hidden layer
#define WGP_WAVES 4          // waves per workgroup; wave w computes output tiles w and w + 4
#define WGP_GROUP 8          // k-steps per software-pipeline group of the MFMA loop
#define WGP_MAX_LAYERS 5     // WG_POLICY_MAX_HIDDEN + the head
#define WGP_MAX_IN 2048
#define WGP_MAX_OUT 128
#define WGP_MAX_WIDTH 256
#define WGP_NOISE_TAG 0x50000000u
#define WGP_MAX_SLOTS 3      // row sets of one k_policy launch: the actor's, the critic's, the critic's on a second set

struct WgPolicyLayer {
    int32_t K, M;              // inputs, outputs
    int32_t nks, ntiles;       // k-steps = ceil(K / 2) rounded up to PAIRS of groups of WGP_GROUP, output tiles = ceil(M / 32)
    uint32_t w_flat, b_flat;   // offsets (floats) into the flat vector
    uint32_t w_packed, b_packed;
};

struct WgPolicyP {
    int32_t n_in, n_out, activation, has_log_std;
    int32_t n_in_vf;           // the critic's input width (= layer[1][0].K; n_in where there is no critic)
    int32_t n_layers[2];       // per net, head included; 0 = the net does not exist
    WgPolicyLayer layer[2][WGP_MAX_LAYERS];
    uint32_t log_std_flat, log_std_packed;
    uint32_t n_flat, n_packed;
};

// One launch of k_policy = up to WGP_MAX_SLOTS slots, each ONE net on its own rows: slot s owns the workgroups
// [end[s - 1], end[s]) of a 1-D grid (end[-1] = 0), ceil(n_rows[s] / 32) of them, so no workgroup is launched past a slot's rows.
// Only the actor has outputs besides `value`, and a launch holds at most one actor slot: those pointers are kernel arguments.
struct WgPolicySlots {
    const float* obs[WGP_MAX_SLOTS];     // [n_rows][the net's input width]
    float* value[WGP_MAX_SLOTS];         // [n_rows] (critic slots)
    int32_t n_rows[WGP_MAX_SLOTS], net[WGP_MAX_SLOTS], end[WGP_MAX_SLOTS];
};

struct wg_policy_s {
    WgPolicyP P;
    int device;
    float* packed;             // [P.n_packed]
    float* flat_stage;         // [P.n_flat] staging copy for host-pointer wg_policy_set_params
};

#endif
