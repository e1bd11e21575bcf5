// wg_rules.h — the task's value rules, stated ONCE: the turbine rules (action, base controller), the reward's penalty head, the
// episode metrics and the steps of an episode.  Every step path (k_flow, k_flow_env, k_flow_envb, k_glue,
// k_glue_lean, k_curriculum) calls these; tests/rules_shim.cpp compiles them with g++ alone and tests/test_rules_host.py holds
// them to numpy restatements of the reference's lines.  Values in, values out: no pointer to device memory, no wait, no shuffle,
// no parameter block — a call site reads its parameters through its own kernarg pointer and passes scalars.  No HIP include.
#pragma once
#include <math.h>

#include "../../include/windgym_hip.h"

#ifdef __HIPCC__
#define WG_RULE __host__ __device__ __forceinline__
#else
#define WG_RULE static inline
#endif

// WindFarmEnv._adjust_yaws (Wind_Farm_Env.py:822-864) in float32, as numpy evaluates it on a float32 action: the yaw an actuation
// step leaves, from the yaw before it and the action.  (One statement per numpy operation: each rounds once.)
WG_RULE float wg_rule_adjust_yaw(const int method, float yaw, const float a, const float ymin, const float ymax, const float ystep) {
    if (method == WG_ACT_YAW) {
        yaw = fminf(fmaxf(yaw + a * ystep, ymin), ymax);
    } else {
        float tf = a + 1.0f;
        tf = tf * 0.5f;
        tf = tf * (ymax - ymin);
        tf = tf + ymin;
        const float ny = fminf(fmaxf(tf, yaw - ystep), yaw + ystep);
        yaw = fminf(fmaxf(ny, ymin), ymax);
    }
    return yaw;
}

// BasicControllers.local_yaw_controller / global_yaw_controller (BasicControllers.py:10-73): one step of the baseline farm's
// controller, not clipped.  wdir: the local wind direction in degrees, formed at the call site.  (numpy's bits, a zero's sign included.)
WG_RULE float wg_rule_ctrl_local(const float yaw, const float wdir, const float ystep) {
    const float off = wdir - yaw;
    const float sgn = (float)((off > 0.f) - (off < 0.f));
    return yaw + sgn * fminf(fabsf(off), ystep);
}
WG_RULE float wg_rule_ctrl_global(const float yaw, const float ystep) {
    const float sgn = (float)((yaw > 0.f) - (yaw < 0.f));
    return yaw - sgn * fminf(fabsf(yaw), ystep);
}

// WindFarmEnv._action_penalty (:804-820): below the switch there is no penalty; one turbine's term of the mean; the penalty from
// the terms' sum over the N turbines
#define WG_PENALTY_SWITCH 0.001
WG_RULE float wg_rule_penalty_term(const int type, const float old_yaw, const float yaw) {
    return type == WG_PEN_CHANGE ? fabsf(old_yaw - yaw) : fabsf(yaw);
}
WG_RULE double wg_rule_penalty(const double action_penalty, const int type, const float pen_sum, const int N, const double yaw_max_d) {
    double pen = 0.0;
    if (action_penalty >= WG_PENALTY_SWITCH)
        pen = type == WG_PEN_CHANGE ? action_penalty * ((double)pen_sum / N) : action_penalty * ((double)pen_sum / N / yaw_max_d);
    return pen;
}
// the step's reward (:989-996) from the power reward pr of the handle's reward mode
WG_RULE float wg_rule_reward(const double pr, const double power_scaling, const double pen) {
    return (float)(pr * power_scaling + 0.0 - pen);
}

// what a step adds to episode metric `lane` (recordEpisodeVals.py:31-64; lane m owns metric m), from the episode's running values
// after this step.  A select chain on purpose: a switch became a scratch table.
WG_RULE float wg_rule_metric_add(const int lane, const float reward, const float pnow, const float pbase, const bool truncated,
                                 const float ep_return, const int ep_len, const float ep_power_sum) {
    const float trf = truncated ? 1.f : 0.f;
    float add = 0.f;
    add = lane == WG_MET_STEP_REWARD_SUM ? reward : add;
    add = lane == WG_MET_FARM_POWER_SUM ? pnow : add;
    add = lane == WG_MET_BASE_POWER_SUM ? pbase : add;
    add = lane == WG_MET_N_STEPS ? 1.f : add;
    add = lane == WG_MET_EP_RETURN_SUM ? trf * ep_return : add;
    add = lane == WG_MET_EP_LENGTH_SUM ? trf * (float)ep_len : add;
    add = lane == WG_MET_EP_MEAN_POWER_SUM ? (truncated ? ep_power_sum / (float)ep_len : 0.f) : add;
    add = lane == WG_MET_N_EPISODES ? trf : add;
    return add;
}

// the step() calls of an episode as the background plans count them: the timestep grows by inc = 1 + extra_inc per step (:1027) and
// the episode truncates at the first step that reaches time_max (:1003).  (..._inc: for a caller that holds inc, FlowP::env_inc.)
WG_RULE long wg_rule_episode_steps_inc(const int time_max, const int inc) { return (long)((time_max + inc - 1) / inc) + 1; }
WG_RULE long wg_rule_episode_steps(const int time_max, const int extra_inc) {
    return wg_rule_episode_steps_inc(time_max, 1 + (extra_inc ? 1 : 0));
}
