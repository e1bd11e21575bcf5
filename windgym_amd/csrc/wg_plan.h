// wg_plan.h — what wg_create decides before it touches the device: the parameter blocks of the kernels (WgParams, FlowP), which
// kernel variant a handle runs and how that variant carves its LDS.  Pure host code: a function of the configuration, the
// measurement hooks (as values: WgHooks, filled by wg_hooks_read in wg_api.hip) and the device's LDS limit — no HIP header, no
// environment, no handle — so the choices are pinned by CPU tests (tests/test_plan.py).  One function per decision; every
// threshold sits next to the measurement that set it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#ifndef __HIPCC__
struct float4;      // FlowPtrs (wg_flow.h) only points at HIP's float4
#endif
#include "wg_flow.h"

// Measurement / test hooks (WG_* environment variables, honoured with WG_DEBUG_HOOKS=1 only), read once per wg_create
struct WgHookInt {
    bool set = false;
    int v = 0;      // atoi of the variable's text
};
struct WgHooks {
    WgHookInt flow_block, flow_res, flow_env, env_wpe, env_split, step_fused, sums, lds_pad, lf_cap, pstride_pad, step_graph, share_dev;
    bool first_obs_gl_only = false, no_box8 = false, debug = false, timeline = false;
    std::string timeline_out;
};

struct WgPlan {
    WgParams p;             // what wg_create copies into the handle's parameter blocks (the setters change the copies, not the plan)
    FlowP f;
    int envw_eligible;      // this handle may run the one-launch env kernel / its fused step: the wg_create decision, kept apart from
    int fused_eligible;     // what the boxes set later allow (wg_plan_step_path)
    int first_obs;          // the flow kernel builds the first observation of a background episode (WgPtrs::next_obs)
    double tab_x0, tab_dx;  // uniform grid of the turbine table (FlowP::n_tab points, wg_uniform_table)
    int reset_chunk, reset_launches;      // RESET-mode flow launches that develop any episode (upper bound)
    double alg_bytes;       // algorithmic bytes of one step()
};

inline double wg_defd(double v, double dflt) { return v == 0.0 ? dflt : v; }

inline int wg_plan_fail(std::string* err, int code, const std::string& msg) {
    if (err) *err = msg;
    return code;
}

inline int wg_validate_config(const wg_config* c, std::string* err) {
    if (!c) return wg_plan_fail(err, WG_ERR_INVALID, "null argument");
    if (c->abi_version != WG_ABI_VERSION) return wg_plan_fail(err, WG_ERR_INVALID, "abi_version mismatch");
    if (c->n_envs < 1 || c->n_turb < 1) return wg_plan_fail(err, WG_ERR_INVALID, "n_envs and n_turb must be >= 1");
    if (c->n_farms != 1 && c->n_farms != 2) return wg_plan_fail(err, WG_ERR_INVALID, "n_farms must be 1 or 2");
    if (c->k_sub < 1) return wg_plan_fail(err, WG_ERR_INVALID, "dt_env must be a multiple of dt_sim");
    if (c->n_particles < 8 || c->n_particles % 4) return wg_plan_fail(err, WG_ERR_INVALID, "n_particles must be a multiple of 4 (>= 8)");
    if (c->n_rotor_pts < 1 || c->n_rotor_pts > 64) return wg_plan_fail(err, WG_ERR_INVALID, "n_rotor_pts must be in [1, 64]");
    if (c->n_turb > 32 * WG_MASK_WORDS) return wg_plan_fail(err, WG_ERR_UNSUPPORTED, "n_turb > 128 is not supported by this build");
    if ((long long)c->n_turb * c->n_particles >= (1ll << 22) || c->n_particles > 16384)
        return wg_plan_fail(err, WG_ERR_UNSUPPORTED, "n_turb * n_particles must stay below 2^22 (and n_particles <= 16384)");
    if (!c->x_pos || !c->y_pos || !c->rotor_dy || !c->rotor_dz || !c->tab_ws || !c->tab_power || !c->tab_ct || c->n_tab < 2)
        return wg_plan_fail(err, WG_ERR_INVALID, "layout / rotor points / turbine table missing");
    if (c->action_method != WG_ACT_YAW && c->action_method != WG_ACT_WIND)
        return wg_plan_fail(err, WG_ERR_UNSUPPORTED, "The ActionMethod must be yaw or wind (absolute is not implemented)");
    if (c->reward_mode < 0 || c->reward_mode > 3)
        return wg_plan_fail(err, WG_ERR_INVALID, "The Power_reward must be either Baseline, Power_avg, None or Power_diff");
    if (c->reward_mode == WG_REW_POWER_DIFF && c->power_avg < 40)
        return wg_plan_fail(err, WG_ERR_INVALID, "The Power_avg must be larger then 40 for the Power_diff reward");
    if (c->reward_mode == WG_REW_BASELINE && c->n_farms != 2)
        return wg_plan_fail(err, WG_ERR_INVALID, "Baseline reward needs the baseline farm (n_farms = 2)");
    if (c->power_avg < 1) return wg_plan_fail(err, WG_ERR_INVALID, "Power_avg must be >= 1");
    if (c->turb_mode < WG_TURB_NONE || c->turb_mode > WG_TURB_BOX_POOL) return wg_plan_fail(err, WG_ERR_INVALID, "Invalid turbulence type specified");
    for (int i = 0; i < WG_N_CH; ++i)
        if (c->ch[i].history_len < 1 || c->ch[i].window_len < 1 || c->ch[i].history_n < 1)
            return wg_plan_fail(err, WG_ERR_INVALID, "sensor history/window lengths must be >= 1");
    {
        // the 16-bit emission record (wg_flow.hip): k = ka TI_loc + kb <= 0.25 and |hv| <= |hill| u <= 16 m/s must hold
        // over the sampling ranges (TI_loc^2 <= ti_max^2 + 0.34^2, the Crespo-Hernandez bound at Ct = 0.96); the
        // kernel also flags any violation at run time (wind overrides): WG_ERR_RANGE
        const double ka = wg_defd(c->m0_ka, 0.38), kb = wg_defd(c->m0_kb, 0.004), hill = wg_defd(c->m0_hill, 0.4);
        const double tia = c->no_ti_fold ? 0.0 : 0.466 * wg_defd(c->m0_ti_a, 0.73);
        const double k_hi = ka * std::sqrt(c->ti_max * c->ti_max + tia * tia) + kb;
        if (k_hi > 0.25 || std::fabs(hill) * c->ws_max > 16.0)
            return wg_plan_fail(err, WG_ERR_INVALID, "wind ranges exceed the 16-bit emission record: need ka*sqrt(TI_max^2 + 0.34^2) + kb <= 0.25 "
                                                     "(TI_max <= 0.55 with the default constants) and |hill| * ws_max <= 16 m/s");
    }
    if (c->deficit_model < 0 || c->deficit_model > 2)
        return wg_plan_fail(err, WG_ERR_INVALID, "deficit_model must be 0 (Gaussian), 1 (super-Gaussian) or 2 (tabulated eddy-viscosity deficit)");
    return 0;
}

// ---- WgParams: scalars, observation layout, sums mode --------------------------------------------------------------------------
inline int wg_plan_ch_count(const wg_channel& c, int on) { return (c.current && on) + (c.rolling_mean && on) * c.history_n; }

inline void wg_plan_scalars(const wg_config* c, WgParams& p) {
    p.B = c->n_envs; p.N = c->n_turb; p.F = c->n_farms; p.K = c->k_sub; p.P = c->n_particles; p.S = c->n_rotor_pts;
    p.NP = p.N * p.P;
    p.dt = (float)c->dt_sim; p.dt_d = c->dt_sim;
    p.D = (float)c->rotor_diameter; p.D_d = c->rotor_diameter; p.inv_D = 1.0f / (float)c->rotor_diameter;
    p.hub = (float)c->hub_height; p.hub_d = c->hub_height;
    p.dpart = c->d_particle * c->rotor_diameter;
    p.yaw_min = (float)c->yaw_min; p.yaw_max = (float)c->yaw_max; p.yaw_step = (float)c->yaw_step;
    p.yaw_min_d = c->yaw_min; p.yaw_max_d = c->yaw_max; p.yaw_step_d = c->yaw_step; p.yaw_start = c->yaw_start;
    p.action_method = c->action_method; p.base_controller = c->base_controller; p.yaw_init = c->yaw_init;
    p.has_yaw_defined = c->yaw_defined != nullptr;
    p.ws_min = c->ws_min; p.ws_max = c->ws_max; p.ti_min = c->ti_min; p.ti_max = c->ti_max;
    p.wd_min = c->wd_min; p.wd_max = c->wd_max; p.n_passthrough = c->n_passthrough;
    p.never_truncate = c->never_truncate;
    p.full_chains = c->full_chains;
    for (int i = 0; i < WG_N_CH; ++i) p.ch[i] = c->ch[i];
    p.turb_on[WG_CH_WS] = c->turb_ws; p.turb_on[WG_CH_WD] = c->turb_wd; p.turb_on[WG_CH_YAW] = 1;
    p.turb_on[WG_CH_POWER] = c->turb_power;
    p.farm_on[WG_CH_WS] = c->farm_ws; p.farm_on[WG_CH_WD] = c->farm_wd; p.farm_on[WG_CH_YAW] = 0;
    p.farm_on[WG_CH_POWER] = c->farm_power;
    p.turb_ti = c->turb_ti; p.farm_ti = c->farm_ti;
    const double mn[WG_N_CH] = {c->ws_scale_min, c->wd_scale_min, c->yaw_min, 0.0};
    const double mx[WG_N_CH] = {c->ws_scale_max, c->wd_scale_max, c->yaw_max, c->power_max};
    for (int i = 0; i < WG_N_CH; ++i) { p.sc_min[i] = (float)mn[i]; p.sc_rng[i] = (float)(mx[i] - mn[i]); }
    p.sc_rng_farm_power = (float)(c->power_max * c->n_turb);
    p.ti_min_f = (float)c->ti_scale_min; p.ti_rng_f = (float)(c->ti_scale_max - c->ti_scale_min);
    p.noise = c->noise;
    for (int i = 0; i < WG_N_CH; ++i) p.noise_sigma[i] = (float)c->noise_sigma[i];
    p.reward_mode = c->reward_mode; p.power_avg = c->power_avg; p.power_scaling = c->power_scaling;
    p.action_penalty = c->action_penalty; p.penalty_type = c->penalty_type;
    p.fill_a = c->fill_steps_agent; p.fill_b = c->fill_steps_base; p.autoreset = c->autoreset;
    p.extra_inc = c->extra_timestep_inc; p.turb_mode = c->turb_mode;
    p.ka = (float)wg_defd(c->m0_ka, 0.38); p.kb = (float)wg_defd(c->m0_kb, 0.004); p.eps0 = (float)wg_defd(c->m0_eps, 0.2);
    p.hill = (float)wg_defd(c->m0_hill, 0.4);
    p.tia = (float)wg_defd(c->m0_ti_a, 0.73); p.tib = (float)wg_defd(c->m0_ti_b, 0.8325);
    p.tic = (float)wg_defd(c->m0_ti_c, 0.0325); p.tid = (float)wg_defd(c->m0_ti_d, -0.32);
    p.fc_scale = wg_defd(c->m0_fc_scale, 2.0);
    p.n_tab = c->n_tab;
    double sx = 0, sy = 0;          // farm centre, summed in layout order like the oracle does
    for (int t = 0; t < p.N; ++t) { sx += c->x_pos[t]; sy += c->y_pos[t]; }
    p.cx0 = sx / p.N; p.cy0 = sy / p.N;
}

inline void wg_plan_obs_layout(const wg_config* c, WgParams& p) {
    p.turb_obs = wg_plan_ch_count(c->ch[WG_CH_WS], c->turb_ws) + wg_plan_ch_count(c->ch[WG_CH_WD], c->turb_wd) +
                 wg_plan_ch_count(c->ch[WG_CH_YAW], 1) + (c->turb_ti ? 1 : 0) + wg_plan_ch_count(c->ch[WG_CH_POWER], c->turb_power);
    p.farm_obs = wg_plan_ch_count(c->ch[WG_CH_WS], c->farm_ws) + wg_plan_ch_count(c->ch[WG_CH_WD], c->farm_wd) +
                 (c->farm_ti ? 1 : 0) + wg_plan_ch_count(c->ch[WG_CH_POWER], c->farm_power);
    p.obs_dim = p.turb_obs * p.N + p.farm_obs;
    p.obs_dim_multi = p.turb_obs + p.farm_obs;
    p.hist_max = std::max(c->ch[WG_CH_WS].history_len, std::max(c->ch[WG_CH_WD].history_len, c->ch[WG_CH_YAW].history_len));
    // what k_glue stages of the turbine rings (the farm rings are tiny and always staged): a channel read through
    // windows (rolling means) or through the TI of its whole deque needs the whole ring, a channel read through its
    // `current` value only needs the newest sample, anything else is not part of the observation.  The per-agent
    // observation (PettingZoo facade) reads the same turbine-level channels.
    for (int i = 0; i < WG_N_CH; ++i) {
        const bool on = p.turb_on[i] != 0;
        int st = 0;
        if (on && c->ch[i].current) st = 1;
        if (on && c->ch[i].rolling_mean) st = 2;
        if (i == WG_CH_WS && (c->turb_ti || c->farm_ti)) st = 2;
        p.stage_ch[i] = st;
    }
}

// Sums mode: every rolling mean the observation reads has history_N = 1, i.e. it is the mean of the newest
// min(window, history, pushed) samples (Mes.get_measurements' first window, MesClass.py:85-91) — a window that
// slides by exactly one sample per push.  The lean glue kernel (k_glue_lean) then keeps the window sums of the live
// episode (and the ws deque's sum / sum of squares for calc_TI) as running sums, S += newest - leaving in exact double
// arithmetic, instead of staging and re-summing the rings every step (Env1.yaml: 4 ring samples per turbine instead of
// 35).  The flow kernels are untouched: they push into rings that hold ONE sample more than the deque (ring_cap = H +
// 1), so that the sample leaving a window as long as the deque is still there when the glue runs.  Configurations with
// several windows per channel (2turb.yaml: history_N = 100) keep the ring-staging kernel.  WG_SUMS=0 forces that path
// (tests compare the two).
inline void wg_plan_sums(const wg_config* c, const WgHooks& hk, WgParams& p) {
    bool ok = true;
    for (int i = 0; i < WG_N_CH; ++i) {
        const bool used = p.turb_on[i] || (i != WG_CH_YAW && p.farm_on[i]);
        if (used && c->ch[i].rolling_mean && c->ch[i].history_n != 1) ok = false;
    }
    if (hk.sums.set && hk.sums.v == 0) ok = false;
    p.sums_mode = ok ? 1 : 0;
    for (int i = 0; i < WG_N_CH; ++i) {
        p.ring_cap[i] = c->ch[i].history_len + (ok ? 1 : 0);
        p.ring_magic[i] = (unsigned)((1ull << 32) / (unsigned long long)p.ring_cap[i]) + 1u;
    }
    if (ok) {
        for (int i = 0; i < WG_N_CH; ++i) {
            p.sum_w[i] = std::min(c->ch[i].window_len, c->ch[i].history_len);
            if (p.turb_on[i] && c->ch[i].rolling_mean) p.sum_mask_t |= 1u << i;
            if (p.turb_on[i] && c->ch[i].current) p.cur_mask_t |= 1u << i;
            if (i != WG_CH_YAW && p.farm_on[i] && c->ch[i].rolling_mean) p.sum_mask_f |= 1u << i;
            if (i != WG_CH_YAW && p.farm_on[i] && c->ch[i].current) p.cur_mask_f |= 1u << i;
        }
        p.sum_w[WG_SUM_TI1] = p.sum_w[WG_SUM_TI2] = c->ch[WG_CH_WS].history_len;
        if (c->turb_ti || c->farm_ti) p.sum_mask_t |= (1u << WG_SUM_TI1) | (1u << WG_SUM_TI2);
        if (c->farm_ti) p.sum_mask_f |= (1u << WG_SUM_TI1) | (1u << WG_SUM_TI2);
    }
    // one turbine's block of the observation (wg_obs_turbine)
    WgObsCfg& oc = p.oc;
    oc.cur_mask = p.cur_mask_t; oc.rol_mask = p.sum_mask_t & 0xfu;
    oc.turb_ti = c->turb_ti; oc.turb_obs = p.turb_obs; oc.obs_dim = p.obs_dim; oc.obs_dim_multi = p.obs_dim_multi;
    for (int i = 0; i < WG_N_CH; ++i) {
        oc.hlen[i] = c->ch[i].history_len; oc.wlen[i] = c->ch[i].window_len;
        oc.mn[i] = p.sc_min[i]; oc.inv_rng[i] = 1.0f / p.sc_rng[i];
        oc.inv_w[i] = 1.0 / (double)std::min(c->ch[i].window_len, c->ch[i].history_len);
    }
    oc.ti_mn = p.ti_min_f; oc.inv_ti_rng = 1.0f / p.ti_rng_f;
    int off = 0, foff = 0;
    for (int i = 0; i < WG_N_CH; ++i) {
        p.ring_off[i] = off; off += p.N * p.ring_cap[i];
        p.fring_off[i] = foff; foff += p.ring_cap[i];
    }
    p.ring_stride = off; p.fring_stride = foff;
}

// Particle blocks of consecutive farm slots are `pstride` floats apart: N x P rounded up to an ODD multiple of
// 256 bytes.  The compact rings of a farm use only the front of its block; an odd multiple of the 256-byte granule
// keeps the touched parts from aliasing onto the same residues of the HBM channel interleave (measured: no
// difference on cfg2 either way; kept as the safe choice).
inline int wg_plan_pstride(int NP, const WgHooks& hk) {
    size_t pstride = ((size_t)NP + 63) / 64;      // in 256-byte granules
    if (pstride % 2 == 0) pstride += 1;
    pstride *= 64;
    if (hk.pstride_pad.set) pstride = (size_t)NP + (size_t)hk.pstride_pad.v;
    return (int)pstride;
}

// ---- turbine table on a uniform grid (O(1) lookup in the kernel) -------------------------------------------------------------
// tables that are already uniform (V80: 1 m/s; as_tabular: 0.5 m/s) are used as they are, others are resampled on 1024 points
inline bool wg_uniform_grid(const wg_config* c, int* n, double* x0, double* dx) {
    bool uniform = true;
    const double dx0 = c->tab_ws[1] - c->tab_ws[0];
    for (int i = 2; i < c->n_tab; ++i)
        if (std::fabs((c->tab_ws[i] - c->tab_ws[i - 1]) - dx0) > 1e-9 * std::fabs(dx0)) uniform = false;
    *n = uniform ? c->n_tab : 1024;
    *x0 = c->tab_ws[0];
    *dx = uniform ? dx0 : (c->tab_ws[c->n_tab - 1] - c->tab_ws[0]) / (*n - 1);
    return uniform;
}
inline void wg_uniform_table(const wg_config* c, std::vector<float>* power, std::vector<float>* ct, double* x0, double* dx) {
    int nu = 0;
    const bool uniform = wg_uniform_grid(c, &nu, x0, dx);
    power->clear(); ct->clear();
    if (uniform) {
        for (int i = 0; i < nu; ++i) { power->push_back((float)c->tab_power[i]); ct->push_back((float)c->tab_ct[i]); }
        return;
    }
    int k = 0;
    for (int i = 0; i < nu; ++i) {
        const double x = std::min(*x0 + i * *dx, c->tab_ws[c->n_tab - 1]);
        while (k + 2 < c->n_tab && c->tab_ws[k + 1] <= x) ++k;
        const double f = (x - c->tab_ws[k]) / (c->tab_ws[k + 1] - c->tab_ws[k]);
        power->push_back((float)(c->tab_power[k] + f * (c->tab_power[k + 1] - c->tab_power[k])));
        ct->push_back((float)(c->tab_ct[k] + f * (c->tab_ct[k + 1] - c->tab_ct[k])));
    }
}

// ---- k_flow: variant and LDS carve ---------------------------------------------------------------------------------------------
struct WgFlowVariant {
    bool small;             // N <= 32: all N x N pairs are staged at once
    int res, block;
    int tc0;                // targets per chunk before the compact carve widens it
    int ql_shift, ql_lpt_shift;
};

// Kernel variant: one of the three rows of wg_flow.hip's launch table, (res, block) = (1, 64), (1, 256) or (0, 256) — no hook
// names anything else (tests/test_plan.py).  Small farms (N <= 32: all N x N pairs are staged at once): compact per-turbine
// rings + pair-major deficit phases, single-wave workgroups.  Large farms: the same at 256 threads for steady inflow, else
// uniform P-slot rings with predicate pruning, (target, sample)-major deficit phases, 256 threads.
inline WgFlowVariant wg_plan_flow_variant(const WgParams& p, const WgHooks& hk) {
    WgFlowVariant v;
    int tc = 1024 / p.N; if (tc < 1) tc = 1; if (tc > p.N) tc = p.N;
    // phase B maps one thread per (target, sample): keep a chunk's items a multiple of the sample group
    v.tc0 = tc;
    v.small = p.N <= 32 && tc == p.N;
    v.res = v.small ? 1 : 0;
    v.block = v.small ? 64 : 256;        // small farms: single-wave workgroups (no s_barrier at all): cfg2 80 vs 91 us at 128 threads (no longer built)
    // large farms with steady inflow: the compact / pair-major variant at 256 threads, pairs staged per chunk of
    // targets (cfg3: 206 vs 224 us once the candidate pre-check is tight — the compacted candidate list then holds
    // ~520 of the 6400 pairs, which the sample-major phases walk in full); turbulent large farms keep the legacy one
    if (!v.small && p.N <= 255 && p.turb_mode == WG_TURB_NONE) v.res = 1;
    // tests: WG_FLOW_BLOCK=256 / WG_FLOW_RES=0 force the uniform-ring kernel.  WG_FLOW_BLOCK=64 is what a small farm runs anyway
    // (set, it only switches the env kernels off: wg_plan_step_kernels); any other value names no kernel that is built: ignored.
    if ((hk.flow_block.set && hk.flow_block.v == 256) || (hk.flow_res.set && hk.flow_res.v == 0)) { v.res = 0; v.block = 256; }
    // the compact steady advection lists (turbine, quad-in-ring) in 16 bits: both must fit, whatever the hooks ask for
    v.ql_shift = 0;
    while ((1 << v.ql_shift) < p.P / 4) ++v.ql_shift;
    if (((long)p.N << v.ql_shift) > 65536) { v.res = 0; v.block = 256; }
    v.ql_lpt_shift = 0;
    while (v.ql_lpt_shift < 3 && (p.N << (v.ql_lpt_shift + 1)) <= v.block) ++v.ql_lpt_shift;
    return v;
}

struct WgFlowCarve {
    int target_chunk, lf_cap, gl, lds_off_ql, lds_off_gat, lds_off_turb, lds_off_tab;
    size_t bytes;
};

// LDS carve of k_flow<block, res>.  The staging region of the deficit phases doubles as the quad list of the compact steady
// advection pass (one 16-bit entry per quad of the farm's rings: at most NP / 2 bytes).
// Compact variant: the staging of a chunk of targets is 10 bytes per (target, source) pair (16-bit candidate
// list, deficit, added TI) and the per-pair added-TI array of the sample-major phases is not needed — large farms
// (compact for steady inflow only: no wake-added field there) spend that room on more targets per chunk (cfg3: 27
// instead of 12 -> 3 chunks instead of 7, same LDS).
inline WgFlowCarve wg_plan_flow_carve(const WgParams& p, const WgHooks& hk, const WgFlowVariant& v, int res, int block, int n_tab_u, int S_shift,
                                      int added) {
    WgFlowCarve k;
    int tc = v.tc0;
    k.lf_cap = 0; k.gl = 0; k.lds_off_ql = 0; k.lds_off_gat = 0;
    size_t off = sizeof(float) * 4 * (size_t)tc * p.N;
    if (res) {
        const size_t ql = ((size_t)p.NP / 2 + 15) & ~(size_t)15;
        if (!v.small) {
            const size_t budget = std::max(ql, off) + sizeof(float) * (size_t)tc * p.N;
            const int fit = (int)((budget - 16) / (10 * (size_t)p.N));
            tc = std::max(tc, std::min(p.N, fit));
        }
        // (+ 12 bytes per pair for the added-turbulence contributions when that model is on: small turbulent farms)
        off = std::max(ql, ((size_t)(added ? 22 : 10) * tc * p.N + 16 + 15) & ~(size_t)15);
        if (block == 256) {
            // large-farm steady variant (LF, the one compact kernel at 256 threads): results staged per candidate (layout:
            // wg_flow.h, WG_LF_OFF_*); at least 512 candidates at once, whatever the chunked carve would have taken otherwise
            const size_t fixed = WG_LF_OFF_DEF(p.N);
            off = std::max(off, (fixed + 8 * 512 + 15) & ~(size_t)15);
            k.lf_cap = (int)((off - fixed) / 8);
            // (tests: a small staging capacity, so that the candidates of one flow step take several rounds)
            if (hk.lf_cap.set) k.lf_cap = std::max(64, std::min(k.lf_cap, hk.lf_cap.v));
        }
        // single-wave steady variant: the deficit phase's gathers are LDS-DMA requests issued before the record /
        // quad-list phases, so the candidate list and the quad list are alive together (no aliasing) and the
        // gathers need a landing zone
        if (block == 64 && p.turb_mode == WG_TURB_NONE) {
            k.gl = 1;
            off = ((size_t)10 * tc * p.N + 16 + 15) & ~(size_t)15;
            k.lds_off_ql = (int)off; off += ql;
            k.lds_off_gat = (int)off; off += WG_GAT_BYTES;
        }
    }
    k.target_chunk = tc;
    k.lds_off_turb = (int)off; off += (size_t)WG_TURB_LDS_BYTES * p.N;
    off = (off + 15) & ~(size_t)15;
    k.lds_off_tab = (int)off;
    off += sizeof(float) * (2 * (size_t)n_tab_u + 2 * (size_t)p.S) + (k.gl ? 0 : sizeof(unsigned) * WG_MASK_WORDS * (size_t)tc) +
           (res ? 0 : sizeof(float) * (size_t)tc * p.N);
    off += sizeof(int) * (4 * (size_t)p.N + 4);      // chain-pruning ages + the particle counter + the candidate counter + the quad counter (+ pad) + the yaws before the action + float positions
    if (added && res) off += sizeof(float) * 3 * ((size_t)p.N << S_shift) + sizeof(int) * (size_t)tc;   // gadd: isotropic field at the rotor points + per-target flags
    k.bytes = (off + 15) & ~(size_t)15;
    return k;
}

// ---- the one-launch env kernels ------------------------------------------------------------------------------------------------
// upper bound of a farm's ring quads whatever the wind direction: turbine t keeps roundup4(floor(dx_max / d) + 3)
// particles, dx_max <= its distance to the farthest turbine (wg_ctx_init)
inline size_t wg_plan_farm_quads(const wg_config* c, const WgParams& p) {
    size_t qf = 0;
    for (int t = 0; t < p.N; ++t) {
        double dm = 0;
        for (int j = 0; j < p.N; ++j) dm = std::max(dm, std::hypot(c->x_pos[j] - c->x_pos[t], c->y_pos[j] - c->y_pos[t]));
        // (+ 4, not + 3: the device takes floor((xmax - xr_t) / d) after a cos / sin rotation, which rounding can make one
        // particle longer than this host bound — one more quad after rounding up; the list has no other slack)
        long len = (((long)(dm / p.dpart) + 4) + 3) & ~3L;
        if (len > p.P || p.full_chains) len = p.P;
        qf += (size_t)len / 4;
    }
    return qf;
}

// k_flow_env (wg_env.hip): ONE wave per env, lane = slot * N + turbine over the env's 2 F farm slots — the default for
// steady inflow wherever the slots fit a wave (cfg2: 4 x 16 lanes, cfg4: 4 x 9).  It runs on the GL variant's state
// layout (interleaved record + 16-byte gather copy), so the two are interchangeable launch by launch.
// Its carve (env_off_tab, env_lds) is written for every handle; `ok` says whether the kernel may run.
inline bool wg_plan_env(const WgParams& p, FlowP& f, bool small, size_t qf, int lds_limit) {
    const int NSl = 2 * p.F, NL = NSl * p.N;
    const size_t clb = ((size_t)2 * NL * (p.N > 1 ? p.N - 1 : 1) + 15) & ~(size_t)15;      // candidate list: every ordered pair of a slot
    const size_t stage = std::max((size_t)8 * WG_ENV_CAP + clb, ((size_t)2 * NSl * qf + 15) & ~(size_t)15);
    f.env_off_tab = (int)((WG_ENV_FIXED_LDS_BYTES + stage + 15) & ~(size_t)15);
    const size_t o = (size_t)f.env_off_tab + sizeof(float) * (2 * (size_t)f.n_tab + 2 * (size_t)p.S);      // power | ct | rotor points (float2)
    f.env_lds = (int)((o + 15) & ~(size_t)15);
    return f.res && small && f.block == 64 && f.gl && p.turb_mode == WG_TURB_NONE && NL <= 64 && p.N <= 32 && p.P <= 4096 && !f.added &&
           f.deficit_model == 0 && f.env_lds <= 32768 && f.env_lds <= lds_limit;
}

struct WgEnvbCarve {
    int env_cap, off_cl, off_tab;
    size_t bytes;       // per wave
};
inline WgEnvbCarve wg_plan_envb_carve(const WgParams& p, int n_tab_u, int wpe) {
    WgEnvbCarve k;
    const int nlp = wpe == 4 ? 16 : 64;
    const int nl_w = (wpe == 4 ? 1 : (wpe == 2 ? p.F : 2 * p.F)) * p.N;      // lanes a wave serves
    k.env_cap = wpe == 4 ? 128 : 256;
    size_t ob = WG_ENVB_FIXED_LDS_BYTES(nlp) + (size_t)20 * k.env_cap;
    k.off_cl = (int)ob;
    ob = (ob + (size_t)2 * nl_w * (p.N > 1 ? p.N - 1 : 1) + 15) & ~(size_t)15;      // candidate list: every ordered pair of a slot
    k.off_tab = (int)ob;
    ob += sizeof(float) * (2 * (size_t)n_tab_u + 2 * (size_t)p.S);
    k.bytes = (ob + 15) & ~(size_t)15;
    return k;
}

// k_flow_envb (wg_envb.hip): the same pattern for frozen-box inflow (cfg5) on the turbulent small-farm layout (SoA
// record, what k_flow<64, BOX> runs on: the two are interchangeable).  Gaussian deficit; rotor points in rows
// of S_pad <= 16 lanes; the wake-added field and TI folding are run-time options.
// Returns whether the kernel may run; *wpe = its waves per env.  A candidate handle gets its carve written over k_flow_env's.
inline bool wg_plan_envb(const WgParams& p, const WgHooks& hk, FlowP& f, bool small, int lds_limit, int* wpe) {
    const int NL = 2 * p.F * p.N;
    // waves per env of k_flow_envb: four (one per farm slot; two farms of at most 16 turbines) while every env's four waves are
    // resident at once (1024 envs = the chip's 4096 wave slots), else two (one per context) up to 2048 envs, else one
    // (four waves per env — one per farm slot, WG_ENV_WPE=4 — is built and tested but NOT the default: measured 104.3 vs 101.7 us
    // per step on cfg5 x 1024, the launch is bound by the bytes it moves, not by a wave's chain of trips)
    *wpe = (p.B <= 2048) ? 2 : 1;
    if (hk.env_wpe.set) {
        const int w = hk.env_wpe.v;
        *wpe = (w == 4 && p.F == 2 && p.N <= 16) ? 4 : (w == 2 ? 2 : (w == 4 ? 2 : 1));
    }
    if (!(f.res && small && f.block == 64 && !f.gl && p.turb_mode >= WG_TURB_BOX && NL <= 64 && p.N <= 32 && p.P <= 4096 && f.S_pad <= 16 &&
          f.deficit_model == 0))
        return false;
    // fewer waves per env where a workgroup's regions do not fit the LDS
    WgEnvbCarve k = wg_plan_envb_carve(p, f.n_tab, *wpe);
    while (*wpe > 1 && *wpe * k.bytes + 64 > (size_t)lds_limit) {
        *wpe /= 2;
        k = wg_plan_envb_carve(p, f.n_tab, *wpe);
    }
    f.env_cap = k.env_cap; f.envb_off_cl = k.off_cl; f.env_off_tab = k.off_tab; f.env_lds = (int)k.bytes;
    return f.env_lds <= 32768 && f.env_lds <= lds_limit;
}

// Which step path the handle runs: k_flow_env / k_flow_envb or the per-slot k_flow, waves per env, pass waves, one-launch step.
inline void wg_plan_step_kernels(const wg_config* c, const WgHooks& hk, const WgParams& p, FlowP& f, bool small, int lds_limit) {
    const size_t qf = wg_plan_farm_quads(c, p);
    const bool env_ok = wg_plan_env(p, f, small, qf, lds_limit);
    int envb_wpe = 1;
    const bool envb_ok = wg_plan_envb(p, hk, f, small, lds_limit, &envb_wpe);
    f.env_inc = 1 + (p.extra_inc ? 1 : 0);
    f.env_eps_max = std::min(1.0f, (float)(p.eps0 * std::sqrt(3.0))) + 2.0f / 65535.0f;
    // WG_FLOW_BLOCK / WG_FLOW_RES, set to any value, ask for a per-slot k_flow and switch the env kernels off; WG_FLOW_ENV=0 / 1
    // forces them off / on where eligible (tests run all of them).
    f.envw = ((env_ok || envb_ok) && !hk.flow_block.set && !hk.flow_res.set) ? 1 : 0;
    if (hk.flow_env.set) f.envw = ((env_ok || envb_ok) && hk.flow_env.v != 0) ? 1 : 0;
    // waves per env: two (one per context, side by side, meeting only when the env truncates) while every env's pair of
    // waves is resident at once — 2048 envs fill the chip's 4096 wave slots; beyond that one wave per env (cfg2 ms per
    // step, two waves / one wave / per-slot kernels + k_glue_lean: 256 envs 0.0231 / 0.0294 / 0.0260, 1024: 0.0276 /
    // 0.0360 / 0.0322, 2048: 0.0340 / 0.0411 / 0.0435, 4096: 0.0643 / 0.0624 / 0.0682)
    f.env_wpe = (p.B <= 2048 && 2 * f.env_lds <= lds_limit) ? 2 : 1;
    if (hk.env_wpe.set) f.env_wpe = (hk.env_wpe.v == 2 && 2 * f.env_lds <= lds_limit) ? 2 : 1;
    // small batches: a pass wave for the running episode's context (wg_env.hip, SPLIT: three waves per env) while they sit at
    // most three to a SIMD (1024 envs) and a farm's pass is four trips or more (cfg2 x 256 / 512 / 1024: +19 / +18 / +10 %; x 2048:
    // -21 %, more than one dispatch round; cfg4's 3 x 3 farm: two trips, -3 to -6 %: the wave costs more than it takes over)
    const bool split_ok = env_ok && f.env_wpe == 2 && p.K == 1 && 4 * f.env_lds + 4096 <= lds_limit;
    f.env_split = (split_ok && p.B <= 1024 && qf >= 256) ? (p.B <= 512 ? 2 : 1) : 0;
    if (hk.env_split.set) f.env_split = (hk.env_split.v != 0 && split_ok && p.B <= 2048) ? (hk.env_split.v == 2 ? 2 : 1) : 0;
    if (envb_ok) f.env_wpe = envb_wpe;
    // Shared development (wg_env.hip): until a background episode goes live its baseline farm is a bit-for-bit twin of its agent
    // farm (same wind, the agent's initial yaws, no controller during development), so k_flow_env develops the agent slot alone
    // and clones it — 14 % of cfg2's farm flow-steps.  Only that kernel knows how (k_flow_envb and the per-slot kernels develop
    // both farms), and only a handle with a baseline farm has anything to share; a flow script never reaches the env kernels
    // (wg_launch_flow).  WG_ENV_SHARE_DEV=0: both farms develop, for A/B runs and the tests that compare the two.
    f.env_share = (f.envw && env_ok && p.F == 2) ? 1 : 0;
    if (hk.share_dev.set && hk.share_dev.v == 0) f.env_share = 0;
    // one launch per step where the env kernel runs and the lean glue's specialised instantiation applies
    const bool gen = p.turb_ti || p.farm_ti || p.farm_obs > 0 || (p.sum_mask_f | p.cur_mask_f) != 0;
    f.env_fused = (f.envw && p.sums_mode && !gen && p.power_avg <= 64) ? 1 : 0;
    if (hk.step_fused.set) f.env_fused = (f.env_fused && hk.step_fused.v != 0) ? 1 : 0;
}

// ---- the rest of FlowP: copies and reciprocals of WgParams ---------------------------------------------------------------------
inline void wg_plan_flow_scalars(const wg_config* c, const WgParams& p, double tab_x0, double tab_dx, FlowP& f) {
    f.B = p.B; f.N = p.N; f.F = p.F; f.K = p.K; f.P = p.P; f.S = p.S; f.NP = p.NP;
    f.S_pad = 1; f.S_shift = 0;
    while (f.S_pad < p.S) { f.S_pad <<= 1; f.S_shift++; }
    f.autoreset = p.autoreset; f.action_method = p.action_method; f.base_controller = p.base_controller;
    f.power_avg = p.power_avg; f.script_rows = 0; f.noise = (p.noise == WG_NOISE_NORMAL);
    f.dt = p.dt; f.D = p.D; f.inv_D = p.inv_D; f.hub = p.hub; f.dpart_f = (float)p.dpart; f.R_rot = 0.5f * p.D;
    f.inv_N = 1.0f / (float)p.N; f.inv_S = 1.0f / (float)p.S; f.inv_P = 1.0f / (float)p.P;
    f.inv_power_avg = 1.0f / (float)(p.power_avg > 0 ? p.power_avg : 1);
    f.pavg_magic = (unsigned)((1ull << 32) / (unsigned long long)(p.power_avg > 0 ? p.power_avg : 1)) + 1u;
    f.dt_d = p.dt_d; f.dpart = p.dpart; f.inv_dpart = 1.0 / p.dpart;
    f.yaw_min = p.yaw_min; f.yaw_max = p.yaw_max; f.yaw_step = p.yaw_step;
    f.ka = p.ka; f.kb = p.kb; f.eps0 = p.eps0; f.hill = p.hill; f.tia = p.tia; f.tib = p.tib; f.tic = p.tic; f.tid = p.tid;
    f.tab_x0 = (float)tab_x0; f.tab_inv_dx = (float)(1.0 / tab_dx);
    f.ue_scale = p.turb_mode == WG_TURB_NONE ? 1.0f : 2.0f;
    for (int i = 0; i < WG_N_CH; ++i) {
        // (the flow kernels only push: what they call the history length is the rings' physical capacity)
        f.hlen[i] = p.ring_cap[i]; f.ring_off[i] = p.ring_off[i]; f.fring_off[i] = p.fring_off[i];
        f.inv_hlen[i] = 1.0f / (float)p.ring_cap[i];
        f.hmagic[i] = (unsigned)((1ull << 32) / (unsigned long long)p.ring_cap[i]) + 1u;
        f.noise_sigma[i] = p.noise_sigma[i];
    }
    f.ring_stride = p.ring_stride; f.fring_stride = p.fring_stride;
    f.turb_mode = p.turb_mode; f.fc_scale = p.fc_scale; f.D_d = p.D_d; f.hub_d = p.hub_d;
    f.inv_sqrt_S = 1.0f / std::sqrt((float)p.S);
    f.added = (c->added_turbulence != 0 && c->turb_mode != WG_TURB_NONE) ? 1 : 0;
    f.no_ti_fold = c->no_ti_fold != 0; f.deficit_model = c->deficit_model;
    f.km1 = (float)wg_defd(c->m0_km1, 0.6); f.km2r = (float)(2.0 * wg_defd(c->m0_km2, 0.35) * 0.5 * p.D_d);
    f.sg_af = (float)wg_defd(c->m0_sg_af, 3.11); f.sg_bf = (float)wg_defd(c->m0_sg_bf, -0.68); f.sg_cf = (float)wg_defd(c->m0_sg_cf, 2.41);
    f.an_inv_ka = (float)(1.0 / wg_defd(c->m0_ka, 0.38));
}

// ---- k_flow_env's hot parameter block: copies, word for word, of what its common STEP path reads (EnvHotP, wg_flow.h) ------------
// A function of the four blocks a launch passes and of nothing else: env_launch (wg_env.hip) calls it on its own arguments.  `gp` /
// `gd` are the glue's blocks (all zeros for a launch without a glue tail, which never reads the request group).
inline EnvHotP wg_plan_env_hot(const FlowP& f, const FlowPtrs& d, const WgParams& gp, const WgPtrs& gd) {
    EnvHotP h;
    memset(&h, 0, sizeof(h));
    EnvHotPro& a = h.pro;
    a.env = d.env; a.slot = d.slot; a.ctx = d.ctx; a.roff = d.roff; a.xr = d.xr; a.yr = d.yr; a.yaw = d.yaw; a.u = d.u;
    a.ti_loc = d.ti_loc; a.bnd = d.bnd; a.tab_power = d.tab_power; a.tab_ct = d.tab_ct; a.rotor_dy = d.rotor_dy; a.rotor_dz = d.rotor_dz;
    a.N = f.N; a.F = f.F; a.inv_N = f.inv_N; a.autoreset = f.autoreset; a.K = f.K; a.n_tab = f.n_tab; a.S = f.S; a.env_inc = f.env_inc;
    a.env_share = f.env_share;
    EnvHotSet& s = h.set;
    s.tab_power = d.tab_power; s.tab_ct = d.tab_ct; s.rotor_dy = d.rotor_dy; s.rotor_dz = d.rotor_dz;
    s.env_off_tab = f.env_off_tab; s.action_method = f.action_method; s.yaw_min = f.yaw_min; s.yaw_max = f.yaw_max; s.yaw_step = f.yaw_step;
    s.hill = f.hill; s.dt = f.dt; s.tic = f.tic; s.hub = f.hub;
    EnvHotReq& r = h.req;
    r.wsum = gd.wsum; r.ring = gd.ring; r.farm_pow = gd.farm_pow; r.base_pow = gd.base_pow; r.metrics = gd.metrics;
    r.N = gp.N; r.power_avg = gp.power_avg; r.ring_stride = gp.ring_stride; r.sum_mask_t = gp.sum_mask_t; r.cur_mask_t = gp.cur_mask_t;
    EnvHotTail& t = h.tail;
    t.ring = d.ring; t.cur_ws = d.cur_ws; t.cur_wd = d.cur_wd; t.env = d.env;
    t.n_tab = f.n_tab; t.tab_x0 = f.tab_x0; t.tab_inv_dx = f.tab_inv_dx; t.env_off_tab = f.env_off_tab; t.ring_stride = f.ring_stride;
    EnvHotFarm& m = h.farm;
    m.fring = d.fring; m.step_farm_pow = d.step_farm_pow; m.step_base_pow = d.step_base_pow; m.pend_farm = d.pend_farm; m.pend_base = d.pend_base;
    m.fring_stride = f.fring_stride; m.power_avg = f.power_avg; m.pavg_magic = f.pavg_magic; m.inv_N = f.inv_N;
    for (int i = 0; i < WG_N_CH; ++i) {
        r.ring_off[i] = gp.ring_off[i]; r.sum_w[i] = gp.sum_w[i]; r.ring_cap[i] = gp.ring_cap[i]; r.ring_magic[i] = gp.ring_magic[i];
        t.hlen[i] = f.hlen[i]; t.ring_off[i] = f.ring_off[i]; t.inv_hlen[i] = f.inv_hlen[i]; t.noise_sigma[i] = f.noise_sigma[i];
        m.hlen[i] = f.hlen[i]; m.fring_off[i] = f.fring_off[i]; m.hmagic[i] = f.hmagic[i];
    }
    return h;
}

// how many RESET-mode launches develop the slowest possible episode: the chain needs
// int(2 * dist / ws) steps (dist <= layout diagonal, ws >= ws_min) plus the window fill
inline int wg_plan_reset_launches(const wg_config* c, const WgParams& p, int reset_chunk) {
    double xmn = 1e300, xmx = -1e300, ymn = 1e300, ymx = -1e300;
    for (int t = 0; t < p.N; ++t) {
        xmn = std::min(xmn, c->x_pos[t]); xmx = std::max(xmx, c->x_pos[t]);
        ymn = std::min(ymn, c->y_pos[t]); ymx = std::max(ymx, c->y_pos[t]);
    }
    const double ext_x = xmx - xmn, ext_y = ymx - ymn;
    const double diag = std::sqrt(ext_x * ext_x + ext_y * ext_y);
    const double ws_lo = std::max(1e-3, std::min(c->ws_min, c->ws_max));
    const long max_dev = (long)std::ceil(2.0 * diag / ws_lo / c->dt_sim) + 2;
    const long max_work = max_dev + (long)p.K * (std::max(p.fill_a, p.fill_b) + 1);
    return (int)((max_work + reset_chunk - 1) / reset_chunk) + 1;
}

// algorithmic bytes of one step(): advection streams py r/w + 4 record floats per particle;
// per turbine 7 floats r/w (+ positions); glue: rings, obs, actions, reward/flag
// inflow None: py r/w + 4 record floats; turbulent: + pz, vlp, wlp r/w (24) and, for the box, 8 corners x
// 2 components gathered per particle (64) and 8 x 3 per rotor point (96)
inline double wg_plan_alg_bytes(const WgParams& p) {
    const bool turb = p.turb_mode != WG_TURB_NONE, boxm = p.turb_mode >= WG_TURB_BOX;
    // record: 2 x 32-bit packed words per particle (8 B)
    const double per_farm_step = (double)p.NP * (4 + 4 + 8 + (turb ? 24 : 0) + (boxm ? 64 : 0)) +
                                 (double)p.N * (7 * 4 * 2 + 16) + (boxm ? (double)p.N * p.S * 96 : 0.0);
    return (double)p.B * ((double)p.K * p.F * per_farm_step + 20.0 * p.N + 12.0 * p.obs_dim + 20.0);
}

// The plan of a handle.  `c` has passed wg_validate_config; lds_limit = bytes of LDS a workgroup may allocate on the device.
// A configuration no kernel variant can run is refused here, before anything is allocated.
inline int wg_plan_create(const wg_config* c, const WgHooks& hk, int lds_limit, WgPlan* out, std::string* err) {
    memset(out, 0, sizeof(*out));
    WgParams& p = out->p;
    FlowP& f = out->f;
    wg_plan_scalars(c, p);
    wg_plan_obs_layout(c, p);
    wg_plan_sums(c, hk, p);
    wg_uniform_grid(c, &f.n_tab, &out->tab_x0, &out->tab_dx);
    wg_plan_flow_scalars(c, p, out->tab_x0, out->tab_dx, f);
    f.pstride = wg_plan_pstride(p.NP, hk);

    const WgFlowVariant v = wg_plan_flow_variant(p, hk);
    f.res = v.res; f.block = v.block; f.ql_shift = v.ql_shift; f.ql_lpt_shift = v.ql_lpt_shift;
    // The compact variant's quad list grows with N * P (NP / 2 bytes): a configuration whose carve exceeds what a
    // workgroup may allocate falls back to the uniform-ring variant (LDS independent of P), and one that fits
    // neither is refused here — not at the first launch, where the failure would be silent.
    WgFlowCarve k = wg_plan_flow_carve(p, hk, v, f.res, f.block, f.n_tab, f.S_shift, f.added);
    if (f.res && k.bytes > (size_t)lds_limit) {
        f.res = 0; f.block = 256;
        k = wg_plan_flow_carve(p, hk, v, f.res, f.block, f.n_tab, f.S_shift, f.added);
    }
    if (k.bytes > (size_t)lds_limit)
        return wg_plan_fail(err, WG_ERR_UNSUPPORTED, "wg_create: k_flow needs " + std::to_string(k.bytes) + " bytes of LDS per workgroup (limit " +
                                                     std::to_string(lds_limit) + "): too many turbines for one workgroup");
    if (f.deficit_model != 0 && !f.res)
        return wg_plan_fail(err, WG_ERR_UNSUPPORTED, "deficit_model 1 / 2 (super-Gaussian, eddy-viscosity table) are built into the compact k_flow variants only "
                                                     "(farms of up to 32 turbines, larger ones with steady inflow)");
    p.compact = f.res;
    f.target_chunk = k.target_chunk; f.lf_cap = k.lf_cap; f.gl = k.gl; f.lds_off_ql = k.lds_off_ql; f.lds_off_gat = k.lds_off_gat;
    f.lds_off_turb = k.lds_off_turb; f.lds_off_tab = k.lds_off_tab;
    f.lds_bytes = (int)k.bytes;
    if (hk.lds_pad.set) f.lds_bytes = std::min(lds_limit, f.lds_bytes + hk.lds_pad.v);      // (measurement: what a workgroup's LDS size alone costs)
    // packed emission record: two arrays, or one interleaved (ct|k, u_e|hv) array where the handle is compact and steady — the
    // variants whose deficit phase gathers bracket pairs from it (GL / k_flow_env: 64 threads; LF: 256 threads)
    f.rec_il = (f.res && p.turb_mode == WG_TURB_NONE) ? 1 : 0;

    wg_plan_step_kernels(c, hk, p, f, v.small, lds_limit);
    out->envw_eligible = f.envw; out->fused_eligible = f.env_fused;
    // The first observation of a background episode is built inside k_flow only by the single-wave steady variant (small
    // farms: one wave reads 35 floats per turbine; measured on the multi-wave variants — cfg3, cfg5 — the building
    // workgroup became the flow kernel's tail: -5 % / -1.3 %).  Other handles keep the glue's own second build.
    // (sums mode: wg_first_obs prepares the episode's window sums as well, in WgPtrs::wsum)
    // (round 4, sums mode: the glue's own rebuild sums every window of the new episode — 14-15 us of k_glue_lean on cfg3 /
    // cfg5 against 10 with prepared sums — so every compact variant prepares them now; WG_FIRST_OBS_GL_ONLY=1 for A/B runs)
    out->first_obs = (f.gl || (f.res && p.sums_mode && !hk.first_obs_gl_only)) ? 1 : 0;
    out->reset_chunk = 32;
    out->reset_launches = wg_plan_reset_launches(c, p, out->reset_chunk);
    out->alg_bytes = wg_plan_alg_bytes(p);
    return 0;
}

// The step path a handle runs with the boxes set at the moment (cells of one box of the pool / of the wake-added box; 0 = none):
// k_flow_envb addresses the cells of a box with 32-bit offsets, so a handle with a larger box runs on the per-slot kernel +
// k_glue_lean, which share its state layout — until a smaller box is set again.
inline void wg_plan_step_path(const WgPlan& plan, long long box_cells, long long abox_cells, int* envw, int* env_fused) {
    const bool big = plan.f.turb_mode != WG_TURB_NONE && (box_cells >= (1ll << 28) || abox_cells >= (1ll << 28));
    *envw = (plan.envw_eligible && !big) ? 1 : 0;
    *env_fused = (plan.fused_eligible && *envw) ? 1 : 0;
}
