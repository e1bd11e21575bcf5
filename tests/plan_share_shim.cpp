// plan_share_shim.cpp — the shared-development flag of the kernel plan (FlowP::env_share, windgym_amd/csrc/wg_plan.h) for
// tests/test_plan_share_dev.py.  Host C++ only:
//   g++ -std=c++17 -shared -fPIC -I include -I windgym_amd/csrc tests/plan_share_shim.cpp
#include <cstddef>

#include "wg_plan.h"

// hooks: (set, value) pairs in the order flow_env, flow_block, env_wpe, env_split, share_dev.
// out: env_share, envw, env_wpe, env_split, reset_launches, F, turb_mode.  Returns the plan's return code.
extern "C" int plan_share(const wg_config* c, const int* hooks, int lds_limit, int* out) {
    WgHooks hk;
    WgHookInt* slot[5] = {&hk.flow_env, &hk.flow_block, &hk.env_wpe, &hk.env_split, &hk.share_dev};
    for (int i = 0; i < 5; ++i) { slot[i]->set = hooks[2 * i] != 0; slot[i]->v = hooks[2 * i + 1]; }
    std::string err;
    WgPlan plan;
    int rc = wg_validate_config(c, &err);
    if (!rc) rc = wg_plan_create(c, hk, lds_limit, &plan, &err);
    if (rc) return rc;
    const FlowP& f = plan.f;
    out[0] = f.env_share; out[1] = f.envw; out[2] = f.env_wpe; out[3] = f.env_split; out[4] = plan.reset_launches;
    out[5] = f.F; out[6] = f.turb_mode;
    return 0;
}

// the flag lives in what used to be padding in front of FlowP's doubles: no other member moves, so the kernels that do not read
// it (k_flow_envb, the per-slot k_flow variants) see the block they have always seen
extern "C" int plan_share_layout(int* out) {
    out[0] = (int)offsetof(FlowP, inv_P); out[1] = (int)offsetof(FlowP, env_share); out[2] = (int)offsetof(FlowP, dt_d);
    out[3] = (int)sizeof(FlowP);
    return 0;
}
