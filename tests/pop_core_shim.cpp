// pop_core_shim.cpp — hands the populations' shared host code to tests/test_pop_core_host.py: the slot-table builder and the
// architecture comparison of windgym_amd/csrc/wg_policy.h, the member-table prologue of wg_ppo.h.  Host C++ only:
//   g++ -std=c++17 -shared -fPIC -I windgym_amd/csrc tests/pop_core_shim.cpp
#include "wg_ppo.h"

// the arrays a table points into (never read: the builder only does pointer arithmetic, which stays inside them)
static float g_rows[3][1 << 14], g_out[5][1 << 14], g_packed[WGP_POP_MAX][4];

// want: bit 0 action, 1 raw, 2 logp, 3 value, 4 final_value.  head[4] = ns, n_head, has_final, Bm; slot[s][13] = obs - rows of its
// kind, obs_step, act_step, row_step, net, t_shift, action / raw / logp / value offsets (-1: null; value against value or final_value
// by t_shift), seed, row_offset, member whose weights it reads
extern "C" void pop_slots(int P, int Bm, int n_out, const int32_t* width, const int64_t* step, int want, int64_t out_step, const uint64_t* seeds,
                          const uint64_t* row_offsets, int64_t* head, int64_t* slot) {
    const float* packed[WGP_POP_MAX];
    for (int m = 0; m < P; ++m) packed[m] = g_packed[m];
    const WgPopKind kinds[3] = {{g_rows[0], width[0], step[0]}, {g_rows[1], width[1], step[1]}, {g_rows[2], width[2], step[2]}};
    WgPopOuts o = {};
    float** outs[5] = {&o.action, &o.raw, &o.logp, &o.value, &o.final_value};
    for (int i = 0; i < 5; ++i)
        if (want >> i & 1) *outs[i] = g_out[i];
    o.step = out_step;
    WgPopSlot tab[WGP_POP_SLOTS] = {};
    const WgPopShape sh = wgp_pop_slots(tab, P, Bm, n_out, packed, kinds, o, seeds, row_offsets);
    head[0] = sh.ns; head[1] = sh.n_head; head[2] = sh.has_final; head[3] = sh.Bm;
    auto off = [](const float* p, const float* base) { return p ? (int64_t)(p - base) : (int64_t)-1; };
    for (int s = 0; s < sh.ns; ++s) {
        const WgPopSlot& t = tab[s];
        const int kind = t.net == 0 ? 0 : t.t_shift == 0 ? 1 : 2;
        const int64_t v[13] = {off(t.obs, g_rows[kind]), t.obs_step, t.act_step, t.row_step, t.net, t.t_shift, off(t.action, g_out[0]),
                               off(t.raw, g_out[1]), off(t.logp, g_out[2]), off(t.value, g_out[kind == 2 ? 4 : 3]), (int64_t)t.seed,
                               (int64_t)t.row_offset, (int64_t)((const float(*)[4])t.packed - g_packed)};
        for (int i = 0; i < 13; ++i) slot[13 * s + i] = v[i];
    }
}

// hp[P][4] = clip, vf_coef, ent_coef, normalize.  out[m][7] = stats - stats_out in records (-1: the fallback pointer, -2: neither),
// stats_step, clip, vf_coef, ent_coef, normalize, what the call returned; -> the members' returns folded with `or`
extern "C" int pop_members(int P, int n_epochs, int n_mb, int with_stats, const float* hp, double* out) {
    static wg_ppo_stats stats[WGP_POP_MAX * 64];
    static float fallback[WGT_NSTAT];
    wg_ppo_hyper h[WGP_POP_MAX];
    for (int m = 0; m < P; ++m) h[m] = {hp[4 * m], hp[4 * m + 1], hp[4 * m + 2], (int32_t)hp[4 * m + 3]};
    bool any = false;
    for (int m = 0; m < P; ++m) {
        WgPopMember M = {};
        const bool norm = wgt_pop_member(M, h, with_stats ? stats : nullptr, m, n_epochs, n_mb, fallback);
        any = any || norm;
        const double rec = M.stats == fallback ? -1.0 : with_stats ? (double)((wg_ppo_stats*)M.stats - stats) : -2.0;
        const double v[7] = {rec, (double)M.stats_step, M.clip, M.vf_coef, M.ent_coef, (double)M.normalize, (double)norm};
        for (int i = 0; i < 7; ++i) out[7 * m + i] = v[i];
    }
    return any;
}

// d[15] = n_in, n_out, activation, has_log_std, n_hidden_pi, hidden_pi[4], n_hidden_vf, hidden_vf[4], n_in_vf
static WgPolicyP layout(const int32_t* d) {
    const wg_policy_desc desc = {d[0], d[1], d[2], d[4], {d[5], d[6], d[7], d[8]}, d[9], {d[10], d[11], d[12], d[13]}, d[3]};
    WgPolicyP P = {};
    wgp_fill_layout(P, &desc, d[14]);
    return P;
}

extern "C" int same_arch(const int32_t* a, const int32_t* b, int widths) { return wgp_same_arch(layout(a), layout(b), widths != 0); }

extern "C" int n_stat(void) { return WGT_NSTAT; }
