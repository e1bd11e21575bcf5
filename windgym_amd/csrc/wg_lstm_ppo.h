// wg_lstm_ppo.h — the host object behind the `wg_lstm_ppo` handle and the buffers of the BPTT kernels (wg_lstm_ppo.hip), next to
// wg_lstm.h, whose model, flat order and packed layout they build on.
//
// A minibatch is Bm ENVS, each with all T steps.  Minibatch row (t, j) is env envs[j] at step t; the env tile `tile` holds the rows
// j = 32 tile .. 32 tile + 31 and NT = ceil(Bm / 32).  BLOCK (t, tile) = t NT + tile.
//
// THE STASH (device memory of the handle, sized for the T_max and Bm_max it was created with; NTm = ceil(Bm_max / 32)):
//     gates [net][T_max NTm][4H][32]   block-major, a block's 32 rows minor: the post-activation gates i, f, g, o of the forward pass
//                                      at feature q H + unit (torch's row order of [4H]); the backward pass overwrites a block IN
//                                      PLACE with dz, the gradient of the pre-activations, and with zeros for rows j >= Bm — so the
//                                      weight-gradient GEMM reads whole blocks with no row mask;
//     c     [net][T_max NTm][H][32]    c_t, same block layout;
//     h     [net][T_max Bm_max][H]     h_t row-major, row t Bm + j: the input rows of the heads, and h_{t-1} of the weight gradient;
//     dh    [2][T_max Bm_max][H]       d loss / d h rows from the actor's and the critic's head (k_ppo_grad_dh);
//     raw, logp, adv, ret              the minibatch's rows of the rollout gathered into row order t Bm + j.
// Floats: nets (5 H) 32 T_max NTm + (nets + 2) H T_max Bm_max + (n_out + 3) T_max Bm_max; with T = 128, Bm = 1024, H = 256 and two nets
// that is 1.9 GB.  A handle whose stash would exceed WGLP_STASH_BYTES is refused by name.
//
// THE TRANSPOSED PACKED BLOCK (written by k_lstm_ppo_pack from the flat parameters at the head of every gradient): the recurrent
// term W_hh^T dz is a GEMM with M = H, K = 4H, so its A operand is a weight block of wg_tile.h over nksT = wg_tile_nks(4H) k-steps
// with row(tile, j) = hidden unit 32 tile + j and k = the row i of W_hh in torch's order:
//     WhhT[net][tile][ks][lane] = W_hh[2 ks + (lane >> 5)][32 tile + (lane & 31)]         (0 for units >= H and rows >= 4H),
// nets back to back, WGP_SLACK zeros behind the last.
#ifndef WG_LSTM_PPO_H
#define WG_LSTM_PPO_H
#include <stdint.h>

#include "wg_lstm.h"
#include "wg_ppo.h"

#define WGLP_STASH_BYTES (16ull << 30)     // most bytes of stash a handle may ask for
#define WGLP_ROWS_MAX (1 << 24)            // most rows T_max * Bm_max of a minibatch
#define WGLP_SPLIT 8                       // most splits of the weight gradient's sum over the blocks: part[WGLP_SPLIT][n_lstm] floats, at
                                           // the policy's limits (two nets, n_in = 2048, H = 256) 151 MB — under wg_ppo.h's WGT_PART_BYTES

// what the three sequence kernels share (by value)
struct WgLstmSeq {
    const float* obs;          // [T][B][n_in]
    const uint8_t* start;      // [T (+ 1)][B]
    const float* state0;       // [nets][2][B][H]
    const int32_t* envs;       // [Bm] env of minibatch column j; an entry outside [0, B) is a column of zeros
    int32_t T, B, Bm, NT, shared;
    int32_t sB;                // populations only (wg_lstm_pop_update): envs of ONE member = rows of a plane of ITS state0
    float *gates, *c, *h;      // the stash
    size_t net_gates, net_c, net_h;        // floats from one net to the next
    const float* dh[2];        // [T Bm][H] from the actor's / the critic's head
    const float* whhT;         // the transposed packed blocks
    uint32_t whhT_net;         // floats of one net's block
    int32_t nksT;
};

// One member of the sequence kernels' table of a population (k_lstm_*_pop; written once per wg_lstm_pop_update, device memory).
// `q` is the WgLstmSeq the member's own wg_lstm_ppo_update would pass, on the WHOLE rollout [T, B] and with
//     q.envs   = the member's permutations [n_epochs][sB] of GLOBAL env ids (the kernels add the minibatch's offset; Bm and NT of
//                the running minibatch are kernel arguments: the members run in lockstep),
//     q.state0 = the member's own [nets][2][sB][H] MINUS m sB H floats, so that the global env id indexes a plane of sB rows,
// and the rest is what the single-policy launches take as arguments.
struct WgLstmPopMember {
    WgLstmSeq q;
    const float* packed;       // the member's LSTM, packed (k_lstm_seq_fwd)
    const float* params;       // the caller's flat vector of the member (k_lstm_ppo_pack reads the LSTM part)
    float* whhT;               // = q.whhT, to write
    float *wpart, *grad;       // the weight gradient's partial sums; the member's flat gradient
    float *raw, *logp, *adv, *ret;   // the gathered rows
};

struct wg_lstm_ppo_s {
    wg_lstm_s* lstm;
    wg_policy_s* pol;
    WgPpoGrad heads;           // the MLP's gradient kernel and its scratch
    WgAdam adam;               // over the policy's one flat vector: the LSTM's n_lstm floats, then the MLP's
    int T_max, Bm_max, NT_max;
    uint32_t n_lstm;
    float *grad, *stats;       // [n_flat] gradient of wg_lstm_ppo_update's running minibatch; scratch stats record
    float *gates, *c, *h, *dh, *rows;      // the stash; rows = raw | logp | adv | ret
    float* whhT;
    float* wpart;              // [WGLP_SPLIT][n_lstm] the weight gradient's partial sums
    uint32_t whhT_net, whhT_all;
    int32_t nksT;
    WgDevMem mem;              // owns every device buffer above, the scratch of heads and the moments of adam included
};

// THE STASH of a handle as the kernels are handed it — the one place that knows the layout above.  q: gates / c / h with their net
// strides, dh, whhT with whhT_net and nksT, `shared`; the batch and the minibatch are the caller's to add.
struct WgLstmStash {
    WgLstmSeq q;
    float *raw, *logp, *adv, *ret;         // the split of `rows`
    const float* h[2];                     // the h plane the actor's / the critic's head reads (a shared LSTM: the one it has)
    float* dh[2];                          // = q.dh, for the heads to write
};
inline WgLstmStash wglp_stash(const wg_lstm_ppo_s* o) {
    const WgLstmP& L = o->lstm->P;
    const size_t n_max = (size_t)o->T_max * o->Bm_max, npad = (size_t)o->T_max * o->NT_max * WGP_TILE, H = L.H;
    WgLstmStash s = {};
    s.q.shared = L.n_nets == 1;
    s.q.gates = o->gates; s.q.c = o->c; s.q.h = o->h;
    s.q.net_gates = npad * 4 * H; s.q.net_c = npad * H; s.q.net_h = n_max * H;
    s.q.dh[0] = s.dh[0] = o->dh; s.q.dh[1] = s.dh[1] = o->dh + n_max * H;
    s.q.whhT = o->whhT; s.q.whhT_net = o->whhT_net; s.q.nksT = o->nksT;
    s.raw = o->rows; s.logp = s.raw + n_max * o->pol->P.n_out; s.adv = s.logp + n_max; s.ret = s.adv + n_max;
    s.h[0] = o->h; s.h[1] = o->h + (size_t)(L.n_nets - 1) * s.q.net_h;
    return s;
}

#endif
