// env_hot_shim.cpp — hands k_flow_env's hot parameter block (wg_plan_env_hot, windgym_amd/csrc/wg_plan.h) to
// tests/test_env_hot_block.py as text, word by word, each next to the member of FlowP / FlowPtrs / WgParams / WgPtrs it copies —
// this table is the second statement of "which word is a copy of what".  Host C++ only:
//   g++ -std=c++17 -shared -fPIC -I include -I windgym_amd/csrc tests/env_hot_shim.cpp
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "wg_plan.h"

namespace {
struct Out {
    char* buf; int cap, n;
    void line(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        va_list ap;
        va_start(ap, fmt);
        if (n < cap) n += vsnprintf(buf + n, cap - n, fmt, ap);
        va_end(ap);
    }
};
template <typename A, typename B>
void word(Out& o, const EnvHotP& h, const char* group, const char* name, const A& got, const B& src) {
    static_assert(sizeof(A) == sizeof(B), "a word of the block has the size of the member it copies");
    unsigned long long g = 0, s = 0;
    memcpy(&g, &got, sizeof(A)); memcpy(&s, &src, sizeof(B));
    o.line("word %s %s %d %d %llx %llx\n", group, name, (int)((const char*)&got - (const char*)&h), (int)sizeof(A), g, s);
}
}      // namespace

// Every pointer member of the two pointer blocks gets an address of its own (base + 64 x its index in the block), so that a word
// copied from the wrong member cannot compare equal.  hooks: (set, value) pairs flow_block .. pstride_pad, as plan_shim.cpp.
extern "C" int env_hot_dump(const wg_config* c, const int* hooks, int lds_limit, char* out, int cap) {
    WgHooks hk;
    WgHookInt* slot[10] = {&hk.flow_block, &hk.flow_res, &hk.flow_env, &hk.env_wpe, &hk.env_split, &hk.step_fused, &hk.sums, &hk.lds_pad, &hk.lf_cap,
                           &hk.pstride_pad};
    for (int i = 0; i < 10; ++i) { slot[i]->set = hooks[2 * i] != 0; slot[i]->v = hooks[2 * i + 1]; }
    std::string err;
    WgPlan plan;
    int rc = wg_validate_config(c, &err);
    if (!rc) rc = wg_plan_create(c, hk, lds_limit, &plan, &err);
    if (rc) return snprintf(out, cap, "rc %d\nerr %s\n", rc, err.c_str()), rc;
    const FlowP& f = plan.f;
    const WgParams& p = plan.p;
    FlowPtrs d;
    WgPtrs gd;
    static_assert(sizeof(FlowPtrs) % sizeof(void*) == 0 && sizeof(WgPtrs) % sizeof(void*) == 0, "the pointer blocks hold pointers only");
    for (size_t i = 0; i < sizeof(FlowPtrs) / sizeof(void*); ++i) { const uintptr_t v = 0x100000000ull + 64 * i; memcpy((char*)&d + i * sizeof(void*), &v, sizeof(v)); }
    for (size_t i = 0; i < sizeof(WgPtrs) / sizeof(void*); ++i) { const uintptr_t v = 0x200000000ull + 64 * i; memcpy((char*)&gd + i * sizeof(void*), &v, sizeof(v)); }
    const EnvHotP h = wg_plan_env_hot(f, d, p, gd);

    Out o{out, cap, 0};
    o.line("rc 0\nsize %d\nasserted %d\nenvw %d\nN %d\nF %d\nK %d\nnoise %d\npower_avg %d\nenv_inc %d\n", (int)sizeof(EnvHotP), WG_ENV_HOT_BYTES, f.envw, f.N,
           f.F, f.K, f.noise, f.power_avg, f.env_inc);
    o.line("group pro %d %d\ngroup set %d %d\ngroup req %d %d\ngroup tail %d %d\ngroup farm %d %d\n", (int)offsetof(EnvHotP, pro), (int)sizeof(EnvHotPro),
           (int)offsetof(EnvHotP, set), (int)sizeof(EnvHotSet), (int)offsetof(EnvHotP, req), (int)sizeof(EnvHotReq), (int)offsetof(EnvHotP, tail),
           (int)sizeof(EnvHotTail), (int)offsetof(EnvHotP, farm), (int)sizeof(EnvHotFarm));
    const unsigned char* raw = (const unsigned char*)&h;
    o.line("raw ");
    for (size_t i = 0; i < sizeof(h); ++i) o.line("%02x", raw[i]);
    o.line("\n");
#define W(grp, m, src) word(o, h, #grp, #m, h.grp.m, src)
#define WCH(grp, m, src) for (int i = 0; i < WG_N_CH; ++i) word(o, h, #grp, (std::string(#m "[") + std::to_string(i) + "]").c_str(), h.grp.m[i], src[i])
    // prologue
    W(pro, env, d.env); W(pro, slot, d.slot); W(pro, ctx, d.ctx); W(pro, roff, d.roff); W(pro, xr, d.xr); W(pro, yr, d.yr); W(pro, yaw, d.yaw); W(pro, u, d.u);
    W(pro, ti_loc, d.ti_loc); W(pro, bnd, d.bnd); W(pro, tab_power, d.tab_power); W(pro, tab_ct, d.tab_ct); W(pro, rotor_dy, d.rotor_dy);
    W(pro, rotor_dz, d.rotor_dz);
    W(pro, N, f.N); W(pro, F, f.F); W(pro, inv_N, f.inv_N); W(pro, autoreset, f.autoreset); W(pro, K, f.K); W(pro, n_tab, f.n_tab); W(pro, S, f.S);
    W(pro, env_inc, f.env_inc); W(pro, env_share, f.env_share);
    // state into LDS, the action
    W(set, tab_power, d.tab_power); W(set, tab_ct, d.tab_ct); W(set, rotor_dy, d.rotor_dy); W(set, rotor_dz, d.rotor_dz);
    W(set, env_off_tab, f.env_off_tab); W(set, action_method, f.action_method); W(set, yaw_min, f.yaw_min); W(set, yaw_max, f.yaw_max);
    W(set, yaw_step, f.yaw_step); W(set, hill, f.hill); W(set, dt, f.dt); W(set, tic, f.tic); W(set, hub, f.hub);
    // the glue's early request: WgParams / WgPtrs
    W(req, wsum, gd.wsum); W(req, ring, gd.ring); W(req, farm_pow, gd.farm_pow); W(req, base_pow, gd.base_pow); W(req, metrics, gd.metrics);
    W(req, N, p.N); W(req, power_avg, p.power_avg); W(req, ring_stride, p.ring_stride); W(req, sum_mask_t, p.sum_mask_t); W(req, cur_mask_t, p.cur_mask_t);
    WCH(req, ring_off, p.ring_off); WCH(req, sum_w, p.sum_w); WCH(req, ring_cap, p.ring_cap); WCH(req, ring_magic, p.ring_magic);
    // per-turbine tail
    W(tail, ring, d.ring); W(tail, cur_ws, d.cur_ws); W(tail, cur_wd, d.cur_wd); W(tail, env, d.env);
    W(tail, n_tab, f.n_tab); W(tail, tab_x0, f.tab_x0); W(tail, tab_inv_dx, f.tab_inv_dx); W(tail, env_off_tab, f.env_off_tab); W(tail, ring_stride, f.ring_stride);
    WCH(tail, hlen, f.hlen); WCH(tail, ring_off, f.ring_off); WCH(tail, inv_hlen, f.inv_hlen); WCH(tail, noise_sigma, f.noise_sigma);
    // farm-level pushes
    W(farm, fring, d.fring); W(farm, step_farm_pow, d.step_farm_pow); W(farm, step_base_pow, d.step_base_pow); W(farm, pend_farm, d.pend_farm);
    W(farm, pend_base, d.pend_base); W(farm, fring_stride, f.fring_stride); W(farm, power_avg, f.power_avg); W(farm, pavg_magic, f.pavg_magic);
    W(farm, inv_N, f.inv_N);
    WCH(farm, hlen, f.hlen); WCH(farm, fring_off, f.fring_off); WCH(farm, hmagic, f.hmagic);
#undef WCH
#undef W
    return o.n < cap ? 0 : -1;
}
