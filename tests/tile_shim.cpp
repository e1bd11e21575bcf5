// tile_shim.cpp — hands the packed-layout half of windgym_amd/csrc/wg_tile.h (and the layout walks of wg_policy.h / wg_lstm.h) to
// tests/test_tile_layout.py.  Host C++ only:
//   g++ -std=c++17 -shared -fPIC -I include -I windgym_amd/csrc tests/tile_shim.cpp
#include "wg_lstm.h"

extern "C" void tile_consts(int* out) {
    out[0] = WGP_TILE; out[1] = WGP_KC; out[2] = WGP_WAVES; out[3] = WGP_GROUP; out[4] = WGP_SLACK;
}
extern "C" int tile_nks(int K) { return wg_tile_nks(K); }
extern "C" int tile_count(int M) { return wg_tile_count(M); }
extern "C" int tile_kpad(int kc) { return wg_tile_kpad(kc); }
extern "C" unsigned tile_wsize(int ntiles, int nks) { return wg_tile_wsize(ntiles, nks); }
extern "C" unsigned tile_bsize(int ntiles) { return wg_tile_bsize(ntiles); }
extern "C" int lstm_tile_row(unsigned tile, unsigned j, int H) { return wgl_tile_row(tile, j, H); }

// every element of the weight block of an MLP layer W[M][K] -> row * K + k of its source, -1: padding (as k_policy_pack reads it)
extern "C" void decode_mlp(int M, int K, int* out) {
    const int nks = wg_tile_nks(K);
    const unsigned n = wg_tile_wsize(wg_tile_count(M), nks);
    for (unsigned e = 0; e < n; ++e) {
        const WgTileElem t = wg_tile_decode(e, nks);
        const unsigned i = t.tile * 32 + t.j;
        out[e] = (i < (unsigned)M && t.k < (unsigned)K) ? (int)(i * K + t.k) : -1;
    }
}

// the same of an LSTM net: Wcat [4H][n_in + H] (as k_lstm_pack reads it)
extern "C" void decode_lstm(int n_in, int H, int* out) {
    const int K = n_in + H, nks = wg_tile_nks(K);
    const unsigned n = wg_tile_wsize(4 * wg_tile_count(H), nks);
    for (unsigned e = 0; e < n; ++e) {
        const WgTileElem t = wg_tile_decode(e, nks);
        const int i = wgl_tile_row(t.tile, t.j, H);
        out[e] = (i >= 0 && t.k < (unsigned)K) ? i * K + (int)t.k : -1;
    }
}

// what wg_policy_create_vf / wg_lstm_create allocate: out = n_flat, n_packed, then (w_packed, b_packed) per layer / per net
extern "C" void policy_layout(const wg_policy_desc* d, int n_in_vf, unsigned* out) {
    WgPolicyP P = {};
    wgp_fill_layout(P, d, n_in_vf);
    *out++ = P.n_flat; *out++ = P.n_packed;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < P.n_layers[net]; ++l) { *out++ = P.layer[net][l].w_packed; *out++ = P.layer[net][l].b_packed; }
}
extern "C" void lstm_layout(const wg_lstm_desc* d, unsigned* out) {
    WgLstmP P = {};
    wgl_fill_layout(P, d);
    *out++ = P.n_flat; *out++ = P.n_packed;
    for (int net = 0; net < P.n_nets; ++net) { *out++ = P.net[net].w_packed; *out++ = P.net[net].b_packed; }
}
