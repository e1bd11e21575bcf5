// rules_shim.cpp — hands the value rules of windgym_amd/csrc/wg_rules.h (the functions every step path calls) to
// tests/test_rules_host.py.  Host C++ only:
//   g++ -std=c++17 -shared -fPIC -I windgym_amd/csrc tests/rules_shim.cpp
#include "wg_rules.h"

extern "C" float rule_adjust_yaw(int method, float yaw, float a, float ymin, float ymax, float ystep) {
    return wg_rule_adjust_yaw(method, yaw, a, ymin, ymax, ystep);
}
extern "C" float rule_ctrl_local(float yaw, float wdir, float ystep) { return wg_rule_ctrl_local(yaw, wdir, ystep); }
extern "C" float rule_ctrl_global(float yaw, float ystep) { return wg_rule_ctrl_global(yaw, ystep); }

// the penalty of N turbines (old[N], yaw[N]): the terms summed in float in index order, as one lane would
extern "C" double rule_penalty(double action_penalty, int type, const float* old_yaw, const float* yaw, int N, double yaw_max_d) {
    float s = 0.f;
    for (int t = 0; t < N; ++t) s += wg_rule_penalty_term(type, old_yaw[t], yaw[t]);
    return wg_rule_penalty(action_penalty, type, s, N, yaw_max_d);
}
extern "C" float rule_reward(double pr, double power_scaling, double pen) { return wg_rule_reward(pr, power_scaling, pen); }
extern "C" float rule_metric_add(int lane, float reward, float pnow, float pbase, int truncated, float ep_return, int ep_len,
                                 float ep_power_sum) {
    return wg_rule_metric_add(lane, reward, pnow, pbase, truncated != 0, ep_return, ep_len, ep_power_sum);
}
extern "C" long rule_episode_steps(int time_max, int extra_inc) { return wg_rule_episode_steps(time_max, extra_inc); }
extern "C" long rule_episode_steps_inc(int time_max, int inc) { return wg_rule_episode_steps_inc(time_max, inc); }
