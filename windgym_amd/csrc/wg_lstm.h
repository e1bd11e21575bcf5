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
//     Wp[tile][ks][lane] = Wcat[q H + 32 u + (lane & 31)][2 ks + (lane >> 5)]     (0 for units >= H and k >= K; ks < nks)
//         — the A operand of v_mfma_f32_32x32x2_f32, as wg_policy.h's,
//     bp[tile][j]        = b_ih[q H + 32 u + j] + b_hh[q H + 32 u + j]            (0 for units >= H): the two biases are added
//         ONCE, here, in this order, and the sum initialises the accumulator,
// then one k-group of zeros behind the last net.  Padding lives here, never in the caller's tensors.
#ifndef WG_LSTM_H
#define WG_LSTM_H
#include <stdint.h>

#include "wg_policy.h"       // the tile constants: WGP_TILE, WGP_KC, WGP_WAVES, WGP_GROUP, WGP_MAX_IN

#define WGL_MAX_H 256        // = 8 unit blocks of 32: wave w owns the blocks w and w + 4

struct WgLstmNet {
    uint32_t wih_flat, whh_flat, bih_flat, bhh_flat;   // offsets (floats) into the flat vector
    uint32_t w_packed, b_packed;
};

struct WgLstmP {
    int32_t n_in, H, n_nets;
    int32_t K;                 // n_in + H
    int32_t nks;               // k-steps = ceil(K / 2) rounded up to PAIRS of groups of WGP_GROUP
    int32_t nub;               // unit blocks = ceil(H / 32); a net has 4 nub output tiles
    WgLstmNet net[2];
    uint32_t n_flat, n_packed;
};

struct wg_lstm_s {
    WgLstmP P;
    int device;
    float* packed;             // [P.n_packed]
    float* flat_stage;         // [P.n_flat] staging copy for host-pointer wg_lstm_set_params
};

#endif
