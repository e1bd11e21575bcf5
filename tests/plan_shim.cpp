// plan_shim.cpp — hands the kernel plan of windgym_amd/csrc/wg_plan.h to tests/test_plan.py as text.  Host C++ only:
//   g++ -std=c++17 -shared -fPIC -I include -I windgym_amd/csrc tests/plan_shim.cpp
#include <cstdio>

#include "wg_plan.h"

// hooks: (set, value) pairs in the order flow_block, flow_res, flow_env, env_wpe, env_split, step_fused, sums, lds_pad, lf_cap,
// pstride_pad, then first_obs_gl_only (set only).  Writes "key value" lines; returns the plan's return code.
extern "C" int plan_dump(const wg_config* c, const int* hooks, int lds_limit, long long box_cells, long long abox_cells, char* out, int cap) {
    WgHooks hk;
    WgHookInt* slot[10] = {&hk.flow_block, &hk.flow_res, &hk.flow_env, &hk.env_wpe, &hk.env_split, &hk.step_fused, &hk.sums, &hk.lds_pad, &hk.lf_cap,
                           &hk.pstride_pad};
    for (int i = 0; i < 10; ++i) { slot[i]->set = hooks[2 * i] != 0; slot[i]->v = hooks[2 * i + 1]; }
    hk.first_obs_gl_only = hooks[20] != 0;
    std::string err;
    WgPlan plan;
    int rc = wg_validate_config(c, &err);
    if (!rc) rc = wg_plan_create(c, hk, lds_limit, &plan, &err);
    if (rc) return snprintf(out, cap, "rc %d\nerr %s\n", rc, err.c_str()), rc;
    const FlowP& f = plan.f;
    const WgParams& p = plan.p;
    int envw = 0, fused = 0;
    wg_plan_step_path(plan, box_cells, abox_cells, &envw, &fused);
    snprintf(out, cap,
             "rc 0\nN %d\nNP %d\nres %d\nblock %d\ngl %d\nrec_il %d\ntarget_chunk %d\nlf_cap %d\nlds_bytes %d\nlds_off_turb %d\nlds_off_tab %d\n"
             "lds_off_ql %d\nlds_off_gat %d\npstride %d\nenvw %d\nenv_wpe %d\nenv_split %d\nenv_fused %d\nenv_lds %d\nenv_off_tab %d\nenv_cap %d\n"
             "envb_off_cl %d\nn_tab %d\ncompact %d\nsums_mode %d\nenvw_eligible %d\nfused_eligible %d\nfirst_obs %d\npath_envw %d\npath_fused %d\n"
             "reset_launches %d\nalg_bytes %.17g\ntab_x0 %.17g\ntab_dx %.17g\nobs_dim %d\nLEAN_PRE_BYTES %d\n",
             f.N, f.NP, f.res, f.block, f.gl, f.rec_il, f.target_chunk, f.lf_cap, f.lds_bytes, f.lds_off_turb, f.lds_off_tab, f.lds_off_ql, f.lds_off_gat,
             f.pstride, f.envw, f.env_wpe, f.env_split, f.env_fused, f.env_lds, f.env_off_tab, f.env_cap, f.envb_off_cl, f.n_tab, p.compact,
             p.sums_mode, plan.envw_eligible, plan.fused_eligible, plan.first_obs, envw, fused, plan.reset_launches, plan.alg_bytes, plan.tab_x0,
             plan.tab_dx, p.obs_dim, LEAN_PRE_BYTES);
    return 0;
}

// the turbine table on the plan's uniform grid; returns its length (power / ct hold at least 1024 floats)
extern "C" int plan_table(const wg_config* c, float* power, float* ct, double* x0, double* dx) {
    std::vector<float> pu, cu;
    wg_uniform_table(c, &pu, &cu, x0, dx);
    for (size_t i = 0; i < pu.size(); ++i) { power[i] = pu[i]; ct[i] = cu[i]; }
    return (int)pu.size();
}
