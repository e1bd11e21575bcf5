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
// PACKED copy (what the kernel reads; owned by the policy object, written by k_policy_pack): per layer one weight block and one
// bias block of wg_tile.h (row(tile, j) = neuron 32 tile + j, ceil(M / 32) tiles), then log_std [n_out] and the slack.  Padding
// lives here, never in the caller's tensors.
//
// NOISE of a stochastic call (restated in oracle/policy_oracle.py: policy_noise): Philox4x32-10 with
//     key     = (seed lo, seed hi)
//     counter = (g lo, counter lo, counter hi, 0x50000000 | ((g hi) & 0xffff) << 8 | (j >> 1)),   g = row + row_offset,
// words (o0, o1) of the output give u1 = ((o0 >> 8) + 1) / 2^24 in (0, 1], u2 = (o1 >> 8) / 2^24 in [0, 1) and
//     eps_j = sqrt(-2 ln u1) * (j even ? cos(2 pi u2) : sin(2 pi u2))                         (float32 arithmetic).
#ifndef WG_POLICY_H
#define WG_POLICY_H
#include <stdint.h>

#include "../../include/windgym_hip.h"
#include "wg_devmem.h"
#include "wg_tile.h"         // the tile constants WGP_TILE, WGP_KC, WGP_WAVES, WGP_GROUP and the packed layout
#include "wg_train.h"        // WgKlLr: a member's learning-rate rule travels in its row of the member table

#define WGP_MAX_LAYERS 5     // WG_POLICY_MAX_HIDDEN + the head
#define WGP_MAX_IN 2048
#define WGP_MAX_OUT 128
#define WGP_MAX_WIDTH 256
#define WGP_NOISE_TAG 0x50000000u
#define WGP_MAX_SLOTS 3      // row sets of one k_policy launch: the actor's, the critic's, the critic's on a second set

struct WgPolicyLayer {
    int32_t K, M;              // inputs, outputs
    int32_t nks, ntiles;       // wg_tile_nks(K), wg_tile_count(M)
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

// Both layouts of a (validated) architecture: the walk of the flat order above, a block pair per layer in the packed vector
inline void wgp_fill_layout(WgPolicyP& P, const wg_policy_desc* d, int32_t n_in_vf) {
    const int nh[2] = {d->n_hidden_pi, d->n_hidden_vf};
    const int32_t* hid[2] = {d->hidden_pi, d->hidden_vf};
    P.n_in = d->n_in; P.n_out = d->n_out; P.activation = d->activation; P.has_log_std = d->has_log_std != 0;
    P.n_in_vf = n_in_vf;
    uint32_t flat = 0, packed = 0;
    for (int net = 0; net < 2; ++net) {
        if (nh[net] < 0) { P.n_layers[net] = 0; continue; }        // (critic only: n_hidden_vf < 0 = none)
        P.n_layers[net] = nh[net] + 1;
        int K = net == 0 ? d->n_in : n_in_vf;
        for (int l = 0; l <= nh[net]; ++l) {
            WgPolicyLayer& ly = P.layer[net][l];
            ly.K = K;
            ly.M = l < nh[net] ? hid[net][l] : (net == 0 ? d->n_out : 1);
            ly.nks = wg_tile_nks(ly.K);
            ly.ntiles = wg_tile_count(ly.M);
            ly.w_flat = flat; flat += (uint32_t)ly.M * ly.K;
            ly.b_flat = flat; flat += (uint32_t)ly.M;
            ly.w_packed = packed; packed += wg_tile_wsize(ly.ntiles, ly.nks);
            ly.b_packed = packed; packed += wg_tile_bsize(ly.ntiles);
            K = ly.M;
        }
    }
    P.log_std_flat = flat; P.log_std_packed = packed;
    if (P.has_log_std) { flat += d->n_out; packed += d->n_out; }
    P.n_flat = flat; P.n_packed = packed + WGP_SLACK;
}

struct wg_policy_s {
    WgPolicyP P;
    WgPacked w;                // [P.n_flat] / [P.n_packed]
    WgDevMem mem;              // owns them
};

// ---------------------------------------------------------------------------------------------------------------------
// Populations (wg_pop): P policies of ONE architecture (one WgPolicyP for all), member m on rows [m Bm, (m + 1) Bm) of every buffer.
// ---------------------------------------------------------------------------------------------------------------------
#define WGP_POP_MAX 16       // = WG_POP_MAX of windgym_hip.h
#define WGP_POP_SLOTS (3 * WGP_POP_MAX)

// One slot of a k_policy_pop launch: ONE net of ONE member on that member's Bm rows.  The table lives in device memory (48
// slots by value would be 4.5 KB of kernel arguments) and is written once per wg_pop_act / wg_pop_rollout; the pointers are those
// of step 0, a step t of a rollout reads / writes at pointer + (t + t_shift) * step.  Every slot of a launch has the same number
// of rows, so blockIdx.x -> (slot, tile) is one scalar division: slot s owns exactly ceil(Bm / 32) workgroups.
struct WgPopSlot {
    const float* packed;       // the member's packed weights
    const float* obs;          // [Bm][the net's input width]
    float* value;              // [Bm] (critic slots)
    float *action, *raw, *logp;   // actor slots: the member's first row of the shared [.., B, ..] arrays (null: not wanted)
    int64_t obs_step, act_step, row_step;   // floats from one step to the next of obs / action, raw / logp, value (0: one call)
    uint64_t seed, row_offset; // the member's noise key and the global row of its first row
    int32_t net, t_shift;      // t_shift = -1: the critic on the final rows of the step before
};

// One member of the training kernels' table (wg_ppo.hip: k_ppo_*_pop, k_policy_pack_pop), written per wg_pop_update
struct WgPopMember {
    const float* packed;       // (k_policy_pack_pop writes it)
    float* params;             // the caller's flat parameters of this member
    float *m, *v, *grad, *part, *spart, *advstat, *blocksq;   // the member's own wg_ppo buffers
    const int32_t* perm;       // [n_epochs][rows_m] GLOBAL row ids of the batch
    float* stats;              // [n_epochs][n_mb][WGT_NSTAT], or the wg_ppo's scratch record with stats_step = 0
    float *lr_dev, *lr_slots;  // with a KL-adaptive rate (all members or none): the caller's rate word, the member's two slots
    float clip, vf_coef, ent_coef, max_norm;
    int32_t normalize, stats_step;
    WgKlLr rule;               // ... and the member's rule (k_ppo_adam_kl_pop)
};

// What the heads of one member of a RECURRENT population read and write in k_ppo_grad_dh_pop (wg_lstm_ppo.hip fills the table): the
// member's own stash rows in minibatch row order — in a plain population these are the one batch all members share
struct WgPopHeadRows {
    const float* obs[2];       // [n][H] the h rows of the actor's / the critic's LSTM
    const float *raw, *logp_old, *adv, *ret;
    float* dh[2];              // [n][H] d loss / d h rows per head
};

struct wg_ppo_s;
struct wg_pop_s {
    int P, device;
    wg_policy_s* pol[WGP_POP_MAX];
    wg_ppo_s* opt[WGP_POP_MAX];    // all null: a population that only acts
    WgPopSlot* slots_dev;          // [WGP_POP_SLOTS]
    // the slot table's current shape: kinds in the order actor, critic, critic on the final rows; P slots of Bm rows per kind
    int n_head, has_final, Bm;     // n_head = kinds of a step's own rows (actor and / or critic)
    void* upd_dev;                 // [WGP_POP_MAX] WgPopMember: the member table of the running wg_pop_update
    WgDevMem mem;                  // owns the two tables (a recurrent population's `heads`: empty, wg_lstm_pop_s::mem owns them)
};

// The slot table, stated once for the plain population (rows = observations) and the recurrent one (rows = the LSTMs' h rows).
// What one KIND of slot reads: member 0's first row, the rows' width, and the floats from one step of a rollout to the next (0: the
// rows stay where they are); kinds in the order actor, critic, critic on the final rows
struct WgPopKind { const float* rows; int width; int64_t step; };
// what the slots write: member 0's first row of each array (null: not wanted; a kind with no output wanted has no slots) and the
// ROWS from one step to the next of all of them (a rollout's [T, B, ..]: B; one call: 0)
struct WgPopOuts { float *action, *raw, *logp, *value, *final_value; int64_t step; };
struct WgPopShape { int ns, n_head, has_final, Bm; };     // slots written; wg_pop_s's three fields

// tab[0 .. ns): per wanted kind P slots, member m on rows [m Bm, (m + 1) Bm) of every array with its own weights packed[m], noise
// key seeds[m] and first global row row_offsets[m] (null: 0; both are read for actor slots only)
inline WgPopShape wgp_pop_slots(WgPopSlot* tab, int P, int Bm, int n_out, const float* const* packed, const WgPopKind kinds[3],
                                const WgPopOuts& o, const uint64_t* seeds, const uint64_t* row_offsets) {
    const bool actor = o.action || o.raw || o.logp;
    int ns = 0;
    for (int kind = 0; kind < 3; ++kind) {
        if (kind == 0 ? !actor : kind == 1 ? !o.value : !o.final_value) continue;
        for (int m = 0; m < P; ++m) {
            WgPopSlot& s = tab[ns++];
            const size_t row = (size_t)m * Bm;
            s.packed = packed[m];
            s.obs = kinds[kind].rows + row * kinds[kind].width;
            s.obs_step = kinds[kind].step; s.act_step = o.step * n_out; s.row_step = o.step;
            s.net = kind == 0 ? 0 : 1;
            s.t_shift = kind == 2 ? -1 : 0;
            if (kind == 0) {
                s.action = o.action ? o.action + row * n_out : nullptr;
                s.raw = o.raw ? o.raw + row * n_out : nullptr;
                s.logp = o.logp ? o.logp + row : nullptr;
                s.seed = seeds[m];
                s.row_offset = row_offsets ? row_offsets[m] : 0;
            } else {
                s.value = (kind == 1 ? o.value : o.final_value) + row;
            }
        }
    }
    return {ns, (actor ? 1 : 0) + (o.value ? 1 : 0), o.final_value ? 1 : 0, Bm};
}

// Two policies of one population have ONE architecture.  The layer table is a function of the wg_policy_desc alone (equal descs <=>
// equal tables, and with them equal n_flat).  `widths`: the input widths n_in / n_in_vf take part — not for the heads of a recurrent
// population, whose widths the check against their LSTMs covers.
inline bool wgp_same_arch(const WgPolicyP& A, const WgPolicyP& Q, bool widths) {
    bool same = Q.n_out == A.n_out && Q.activation == A.activation && Q.has_log_std == A.has_log_std && Q.n_layers[0] == A.n_layers[0] &&
                Q.n_layers[1] == A.n_layers[1] && (!widths || (Q.n_in == A.n_in && Q.n_in_vf == A.n_in_vf));
    for (int net = 0; net < 2 && same; ++net)
        for (int l = 0; l < Q.n_layers[net]; ++l)
            same = same && ((l == 0 && !widths) || Q.layer[net][l].K == A.layer[net][l].K) && Q.layer[net][l].M == A.layer[net][l].M;
    return same;
}

#endif
