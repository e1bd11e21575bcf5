// wg_lstm.h — parameter block of k_lstm (wg_lstm.hip) and the host object behind the `wg_lstm` handle.
//
// A wg_lstm is one or two independent one-layer LSTMs ("nets": 0 = actor, 1 = critic) of one shape n_in -> H: the recurrent front
// of sb3-contrib's MlpLstmPolicy (lstm_actor / lstm_critic; shared_lstm = one net).  The cell is torch.nn.LSTM's, gate order
// i, f, g, o:
//     (h, c) <- (0, 0) for rows with episode_start != 0          — a SELECT: such a row does not read its incoming state at all
//     z  = (b_ih + b_hh) + sum_k Wcat[.][k] xcat[k],   Wcat = [W_ih | W_hh]  [4H][n_in + H],  xcat = x ‖ h,  k ascending
//     c' = sigmoid(z_f) c + sigmoid(z_i) tanh(z_g),    h' = sigmoid(z_o) tanh(c')
// (sb3-contrib multiplies the state by 1 - episode_start instead; for finite states that is the same arithmetic.)
//
// FLAT parameter vector (wg_lstm_set_params; windgym_amd/recurrent.py and tests/lstm_twin.py restate it): per net, actor first,
//     weight_ih [4H][n_in], weight_hh [4H][H], bias_ih [4H], bias_hh [4H]                    (torch's weight_ih_l0 ... names).
//
// PACKED copy (what the kernel reads; owned by the handle, written by k_lstm_pack): the step is ONE GEMM per net with K = n_in + H
// and M = 4H, whose output tile 4u + q holds gate q of the hidden units 32u .. 32u + 31 — so the wave that owns the tiles
// 4u .. 4u + 3 holds all four gates of its units in registers and finishes the cell there.  Per net
//     weight block (wg_tile.h) with row(tile, j) = wgl_tile_row: row q H + 32 u + j of Wcat, padding for units 32 u + j >= H,
//     bias block     bp[tile][j] = b_ih[row] + b_hh[row]: the two biases are added ONCE, here, in this order, and the sum
//         initialises the accumulator,
// then the slack behind the last net.  Padding lives here, never in the caller's tensors.
#ifndef WG_LSTM_H
#define WG_LSTM_H
#include <stdint.h>

#include "wg_policy.h"       // WGP_MAX_IN; wg_tile.h: the tile constants and the packed layout

#define WGL_MAX_H 256        // = 8 unit blocks of 32: wave w owns the blocks w and w + 4

struct WgLstmNet {
    uint32_t wih_flat, whh_flat, bih_flat, bhh_flat;   // offsets (floats) into the flat vector
    uint32_t w_packed, b_packed;
};

struct WgLstmP {
    int32_t n_in, H, n_nets;
    int32_t K;                 // n_in + H
    int32_t nks;               // wg_tile_nks(K)
    int32_t nub;               // unit blocks = ceil(H / 32); a net has 4 nub output tiles
    WgLstmNet net[2];
    uint32_t n_flat, n_packed;
};

// the gate-to-tile map: element j of output tile 4u + q is row q H + 32 u + j of [4H] (gate q of unit 32 u + j); -1: padding
WG_TILE_HD int32_t wgl_tile_row(uint32_t tile, uint32_t j, int32_t H) {
    const int32_t unit = 32 * (int32_t)(tile >> 2) + (int32_t)j;
    return unit < H ? (int32_t)(tile & 3) * H + unit : -1;
}

// Both layouts of a (validated) shape: the flat order above, a block pair per net in the packed vector
inline void wgl_fill_layout(WgLstmP& P, const wg_lstm_desc* d) {
    P.n_in = d->n_in; P.H = d->hidden; P.n_nets = d->n_nets;
    P.K = P.n_in + P.H;
    P.nks = wg_tile_nks(P.K);
    P.nub = wg_tile_count(P.H);
    uint32_t flat = 0, packed = 0;
    const uint32_t H4 = 4u * P.H;
    for (int net = 0; net < P.n_nets; ++net) {
        WgLstmNet& nt = P.net[net];
        nt.wih_flat = flat; flat += H4 * P.n_in;
        nt.whh_flat = flat; flat += H4 * P.H;
        nt.bih_flat = flat; flat += H4;
        nt.bhh_flat = flat; flat += H4;
        nt.w_packed = packed; packed += wg_tile_wsize(4 * P.nub, P.nks);
        nt.b_packed = packed; packed += wg_tile_bsize(4 * P.nub);
    }
    P.n_flat = flat; P.n_packed = packed + WGP_SLACK;
}

#ifdef __HIPCC__
// the cell's sigmoid, one statement of it for k_lstm and the sequence kernels of wg_lstm_ppo.hip
__device__ __forceinline__ float wgl_sigmoid(const float z) { return 1.0f / (1.0f + expf(-z)); }
#endif

struct wg_lstm_s {
    WgLstmP P;
    WgPacked w;                // [P.n_flat] / [P.n_packed]
    WgDevMem mem;              // owns them
};

// ---------------------------------------------------------------------------------------------------------------------
// Populations of recurrent policies (wg_lstm_pop): P pairs (wg_lstm, wg_policy) of ONE architecture, member m on rows
// [m Bm, (m + 1) Bm) of every buffer and with a state of its own, [P][nets][2][Bm][H]: state[m] is the member's state alone.
// ---------------------------------------------------------------------------------------------------------------------
// the members' weights for k_lstm_pop / k_lstm_pack_pop, a kernel argument by value (256 bytes): the member's packed copy and,
// for the pack, the flat LSTM parameters it is built from
struct WgLstmPopW {
    const float* packed[WGP_POP_MAX];
    const float* flat[WGP_POP_MAX];
};

struct wg_lstm_ppo_s;
struct wg_lstm_pop_s {
    int P, device;
    wg_lstm_s* lstm[WGP_POP_MAX];
    wg_lstm_ppo_s* opt[WGP_POP_MAX];     // all null: a population that only acts
    wg_pop_s heads;                       // the members' MLPs (heads.pol[]) as k_policy_pop sees them: its slot table on the LSTMs' h rows (no optimisers)
    void* seq_dev;                        // [WGP_POP_MAX] WgLstmPopMember: the sequence kernels' member table of the running update
    void* upd_dev;                        // [2][WGP_POP_MAX] WgPopMember of that update: the heads' view (MLP part), Adam's (whole vector)
    void* rows_dev;                       // [WGP_POP_MAX] WgPopHeadRows
    WgDevMem mem;                         // owns the four tables
};

#endif
