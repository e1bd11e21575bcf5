// wg_ppo.h — the host objects behind the `wg_ppo` handle (the gradient kernel's side, WgPpoGrad, and the optimiser's: wg_train.h's
// WgAdam and the gradient vector) and the constants of the training kernels (wg_ppo.hip).
//
// k_ppo_grad works on tiles of R rows (R = 32 when a net's activations fit the workgroup's LDS, else 16, 8, 4 or 2: a
// function of the architecture alone — each net's map with its own input width, n_in / n_in_vf).  Minibatch rows 0 .. n-1 form ceil(n / R) tiles; G = min(tiles, g_max) workgroups
// per net, workgroup g takes tiles g, g + G, g + 2 G ... in that order and owns row g of the partials:
//     part[g][n_flat]   the gradient of the SUM over its rows, in the flat parameter layout of wg_policy.h
//                       (actor workgroup g writes the actor's entries and log_std, critic workgroup g the critic's),
//     spart[g][4]       sums of L_pi, (ratio - 1) - log ratio, [|ratio - 1| > eps] (actor) and of L_v (critic).
// k_ppo_reduce adds the rows g = 0 .. G-1 in index order.  n, R and g_max fix every summation order: results are
// bit-identical from run to run and from device to device.
#ifndef WG_PPO_H
#define WG_PPO_H
#include <stdint.h>

#include "wg_policy.h"
#include "wg_train.h"

#define WGT_WAVES 4               // waves per workgroup of k_ppo_grad
#define WGT_LDS_BYTES 65536       // LDS budget of one workgroup
#define WGT_G_MAX 512             // most workgroups per net
#define WGT_PART_BYTES (256u << 20)   // most bytes of gradient partials (bounds g_max for very large nets)
#define WGT_NSTAT 8               // floats of a wg_ppo_stats record
#define WGT_STAT_KL 3             // ... of which approx_kl is this one (what the KL-adaptive rate reads)
#define WGT_BLOCK 256             // threads of the element-wise kernels (reduce, sum of squares, Adam)
// the actor's loss head, a compile-time choice of the gradient kernel's body: PPO's clipped surrogate (k_ppo_grad*), or the
// supervised loss of k_bc_grad, whose spart[g] holds the sums of the rows' squared error / n_out, -logp(target) and absolute error /
// n_out (actor) and of L_v (critic, only with returns) and is read by k_bc_reduce alone
#define WGT_HEAD_PPO 0
#define WGT_HEAD_BC 1

// LDS map of one net (offsets in floats; S = R + 1 floats per feature row, conflict-free for row- and feature-major reads)
struct WgPpoLds {
    int32_t xin;                          // [min(the net's input width, 256)][S]   observation chunk
    int32_t act[WGP_MAX_LAYERS];          // [M_l][S]              activations of hidden layer l; the head's output at act[L-1]
    int32_t d[2];                         // [max M][S]            dZ of the running layer / of the one before it
    int32_t rowv;                         // [4][32]               per-row scalars of the loss head
    int32_t rid;                          // [32] int              the row this net gathers for each tile row (actor: agent row,
                                          //                       critic: its env row), -1 = none
    int32_t total;
};

struct WgPpoK {                           // by-value kernel argument next to WgPolicyP
    int32_t R;                            // rows per tile
    WgPpoLds lds[2];
};

// the gradient kernel's side of a policy: its LDS map, its grid limit and its scratch — all k_ppo_grad* needs on the host.  The
// recurrent trainer holds one by value for its heads (wg_lstm_ppo.h); wg_ppo_grad_init_ of wg_internal.h
struct WgPpoGrad {
    wg_policy_s* pol;
    WgPpoK K;
    size_t lds_bytes;
    int g_max;
    uint32_t n_blocks;                    // ceil(the policy's n_flat / WGT_BLOCK): k_ppo_reduce's grid
    float *part, *spart;                  // [g_max][n_flat], [g_max][4]
    float *advstat;                       // [2] mean and unbiased std of the minibatch's advantages
    float *stats;                         // [WGT_NSTAT] scratch record when the caller wants none
};

// The hyper-parameter and statistics fields of member m's row of an update's member table (wg_pop_update, wg_lstm_pop_update): the
// member's [n_epochs][n_mb] records of stats_out, or the one `fallback` record written over and over -> the member normalises
inline bool wgt_pop_member(WgPopMember& M, const wg_ppo_hyper* hp, wg_ppo_stats* stats_out, int m, int n_epochs, int n_mb, float* fallback) {
    M.stats = stats_out ? (float*)(stats_out + (size_t)m * n_epochs * n_mb) : fallback;
    M.stats_step = stats_out ? WGT_NSTAT : 0;
    M.clip = hp[m].clip_range; M.vf_coef = hp[m].vf_coef; M.ent_coef = hp[m].ent_coef;
    M.normalize = hp[m].normalize_advantage != 0;
    return M.normalize;
}

// ... and what the row Adam's kernel reads holds of the member's KL-adaptive rate (wg_ppo_set_kl_lr; lr_dev null: none)
inline void wgt_pop_member_kl(WgPopMember& M, const WgAdam& a) {
    M.lr_dev = a.lr_dev; M.lr_slots = a.lr_slots; M.rule = a.rule;
}

struct wg_ppo_s {
    WgPpoGrad g;
    WgAdam adam;                          // over the policy's flat vector, on the policy's device
    float* grad;                          // [n_flat] gradient of wg_ppo_update's running minibatch
    WgDevMem mem;                         // owns the scratch of g, the moments of adam and grad
};

#endif
