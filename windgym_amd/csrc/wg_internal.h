// wg_internal.h — the library's internal functions that cross translation units: the launch wrappers of the kernels and two
// helpers.  They have C linkage, so a caller's prototype that disagrees with the definition would still link; this is the one
// declaration of each, included by the file that defines it and by every file that calls it, so that the compiler checks both.
// (include after <hip/hip_runtime.h>; the parameter blocks are passed by pointer and need no definition here)
#pragma once
#include <stdint.h>

#include "../../include/windgym_hip.h"

struct FlowP;
struct FlowPtrs;
struct WgParams;
struct WgPtrs;
struct WgPopKind;
struct WgPopOuts;
struct WgPolicyP;
struct WgPopMember;
struct WgPopHeadRows;
struct WgPacked;
struct WgAdam;
struct WgPpoGrad;
struct WgDevMem;
struct WgValueRows {           // the critic on n_rows rows: obs [n_rows][critic's input width] -> value [n_rows]
    const float* obs;
    float* value;
    int n_rows;
};

struct WgActuation {           // what a wg_curriculum copies from the handle it is created on: the batch and the yaw actuation rule
    int B, N, action_method, device;
    float yaw_min, yaw_max, yaw_step;      // as the step kernels hold them
    double yaw_max_d;                      // wg_config.yaw_max
};

extern "C" {
// wg_api.hip: the thread-local message behind wg_last_error; returns `code`
int wg_set_last_error_(int code, const char* msg);
// wg_api.hip: the handle's batch geometry, device and yaw actuation (wg_curriculum.hip)
int wg_handle_actuation_(wg_handle h, WgActuation* out);
// wg_norm.hip: the widths a wg_norm was created for and its device (wg_rollout_norm's checks)
int wg_norm_geometry_(wg_norm n, int* n_obs, int* n_envs, int* device);
// wg_lstm.hip: the shape a wg_lstm was created for and its device (wg_rollout_lstm's checks)
int wg_lstm_geometry_(wg_lstm l, int* n_in, int* hidden, int* n_nets, int* device);
// The three allocators below have one shape: the memory is `mem`'s (wg_host.h: WgDevMem, on mem->device), a failure is reported as
// `who` and leaves what was allocated to the handle's destroy, which releases `mem`.
// wg_policy.hip: a handle's device copies of its parameters (wg_tile.h: WgPacked; the packed copy zeroed), and the pointer a
// set_params' pack kernel reads: `params` itself, or the stage after an asynchronous copy of a host pointer
int wg_packed_alloc_(WgDevMem* mem, WgPacked* w, uint32_t n_flat, uint32_t n_packed, const char* who);
int wg_packed_source_(WgPacked* w, const float* params, int on_device, hipStream_t st, const float** src);
// wg_policy.hip: ONE launch of k_policy — the actor on n_rows rows of obs_dev (when action / raw / logp is wanted) and the critic on
// each of n_v <= 2 row sets of its own (rows of the critic's input width -> value); a set of no rows is skipped
int wg_policy_eval_(wg_policy p, int n_rows, const float* obs_dev, int deterministic, uint64_t seed, uint64_t counter, uint64_t row_offset,
                    float* action_dev, float* raw_dev, float* logp_dev, const WgValueRows* v, int n_v, void* stream);
// wg_policy.hip, populations (wg_policy.h): `bytes` (a multiple of 4) of a host table -> device memory by kernel launches in stream
// order; the slot table of k_policy_pop (wg_policy.h: wgp_pop_slots) for Bm rows per member of the rows `kinds` describes, no
// refusals; that table on n_rows rows of observations shared out among the members (refusals reported as `who`); one launch on it
int wg_pop_store_(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int wg_pop_prepare_(wg_pop q, const char* who, int n_rows, const uint64_t* seeds, const uint64_t* row_offsets, const float* obs,
                    const float* final_obs, const WgPopOuts* o, void* stream);
int wg_pop_slots_(wg_pop q, int Bm, const WgPopKind* kinds, const WgPopOuts* o, const uint64_t* seeds, const uint64_t* row_offsets, void* stream);
int wg_pop_launch_(wg_pop q, int head, int fin, int t, int deterministic, uint64_t counter, void* stream);
// wg_ppo.hip: Adam over one flat vector (wg_train.h: WgAdam).  alloc: moments zeroed, step 0; get / set_state: the public
// *_get_state / *_set_state entries, reported as `who`, a null `a` included; apply: counts one step, then clipping by the global norm
// of grad_dev [n_flat] and that step of Adam on params_dev in place (k_ppo_sumsq + k_ppo_adam)
int wg_adam_alloc_(WgDevMem* mem, WgAdam* a, uint32_t n_flat, const char* who);
int wg_adam_get_state_(WgAdam* a, const char* who, float* mv_host, size_t n, uint64_t* step);
int wg_adam_set_state_(WgAdam* a, const char* who, const float* mv_host, size_t n, uint64_t step);
int wg_adam_apply_(WgAdam* a, float* params_dev, const float* grad_dev, float lr, float max_grad_norm, hipStream_t st);
// wg_ppo.hip, the KL-adaptive rate (wg_train.h: WgKlLr).  set_kl_lr: the public *_set_kl_lr entries, reported as `who`, a null `a`
// included; the first rule set on a handle allocates its two slots from `mem`, the handle's owner (none is ever set: nothing);
// apply_kl: wg_adam_apply_ for minibatch mb (`last`: the final one) of an update while a rule is set — the rate comes from the
// handle's device words and is stepped by approx_kl of the record at stats_dev first, mb = 0 excepted (k_ppo_sumsq + k_ppo_adam_kl)
int wg_adam_set_kl_lr_(WgDevMem* mem, WgAdam* a, const char* who, const wg_kl_lr* rule, float* lr_dev);
int wg_adam_apply_kl_(WgAdam* a, float* params_dev, const float* grad_dev, const float* stats_dev, int mb, int last, float max_grad_norm,
                      hipStream_t st);
// wg_ppo.hip: the gradient kernel's side of policy p (wg_ppo.h: WgPpoGrad) — the first half of wg_ppo_create; what it refuses about
// the policy is reported under that name.  heads_grad, the heads of a recurrent policy (wg_lstm_ppo.hip): k_ppo_grad's loss on n rows whose actor reads h_pi [n][H] and
// whose critic reads h_vf [n][H], raw / logp / adv / ret indexed by the same row -> the MLP's flat gradient, the stats record and the
// gradients of the rows, dh_pi / dh_vf [n][H] (k_ppo_grad_dh)
int wg_ppo_grad_init_(WgDevMem* mem, WgPpoGrad* g, wg_policy p, const char* who);
int wg_ppo_heads_grad_(WgPpoGrad* g, const float* mlp_params_dev, const float* h_pi, const float* h_vf, const float* raw, const float* logp,
                       const float* adv, const float* ret, int n, const wg_ppo_hyper* hp, float* dh_pi, float* dh_vf, float* grad_out,
                       float* stats_out, void* stream);
// wg_ppo.hip: wg_ppo_heads_grad_ with k_bc_grad's loss (k_bc_grad_dh + k_bc_reduce) on the expert's actions target [n][n_out]; ret
// [n] or null: no critic term — then the critic's workgroups are not launched, dh_vf is NOT written and the critic's entries of
// grad_out are 0.0f
int wg_ppo_heads_bc_grad_(WgPpoGrad* g, const float* mlp_params_dev, const float* h_pi, const float* h_vf, const float* target,
                          const float* ret, int n, const wg_bc_hyper* hp, float* dh_pi, float* dh_vf, float* grad_out, float* stats_out,
                          void* stream);
// k_policy_pack for each of the n_members rows of a member table (device)
void wg_policy_pack_pop_(const WgPolicyP* P, const WgPopMember* mt, int n_members, void* stream);
// wg_ppo.hip: wg_ppo_heads_grad_ for the n_members heads of a recurrent population in the launches of one — member m's scratch, flat
// MLP parameters, gradient and stats slot are row m of `mt` (device), the rows it reads and the dh rows it writes row m of `rt`
// (device), n rows each; `g0`: the gradient side of member 0's heads (one architecture: one LDS map, one grid); `mb`: the
// minibatch's ordinal (its stats slot); any_norm: some member normalises its advantages
int wg_ppo_heads_grad_pop_(const WgPpoGrad* g0, const WgPopMember* mt, const WgPopHeadRows* rt, int n_members, int any_norm, int n, int mb,
                           void* stream);
// Adam over each of the n_members rows of a member table (device): counts one step of adam[m], then clipping by the member's own
// norm and that step with the member's own lr[m] (k_ppo_sumsq_pop + k_ppo_adam_pop) on vectors of adam[0]->n_flat floats
int wg_adam_apply_pop_(const WgPopMember* mt, int n_members, WgAdam* const* adam, const float* lr, void* stream);
// ... with KL-adaptive rates: *on = every member has a rule set, or none has — anything else is refused as `who`, naming the member
// (so is a rate word two members share); apply_kl_pop: wg_adam_apply_kl_ per member, whose words, rule and stats records are its row's
// (k_ppo_sumsq_pop + k_ppo_adam_kl_pop)
int wg_pop_kl_lr_(const char* who, int n_members, WgAdam* const* adam, int* on);
int wg_adam_apply_kl_pop_(const WgPopMember* mt, int n_members, WgAdam* const* adam, int mb, int last, void* stream);
// wg_lstm.hip, populations of recurrent policies (wg_lstm.h): wg_lstm_step for every member in ONE launch of k_lstm_pop on n_rows =
// P Bm rows; k_lstm_pack for every member in one launch (params_dev[m]: host array of the members' flat vectors); the heads' slot
// table on the h rows of the running step (the outputs: wg_policy.h, WgPopOuts)
int wg_lstm_pop_step_(wg_lstm_pop q, int n_rows, const float* x_dev, const uint8_t* episode_start_dev, const float* state_in_dev,
                      float* state_out_dev, float* h_pi_dev, float* h_vf_dev, int net_mask, void* stream);
int wg_lstm_pack_pop_(wg_lstm_pop q, const float* const* params_dev, void* stream);
int wg_lstm_pop_slots_(wg_lstm_pop q, int n_rows, const uint64_t* seeds, const uint64_t* row_offsets, const float* h_pi, const float* h_vf,
                       const float* h_fin, const WgPopOuts* o, void* stream);
// wg_yaw_table.hip: the turbine count a wg_yaw_table was created for and its device (wg_yaw_table_act's and wg_rollout_table's
// checks); ONE launch of k_yaw_table_act — the table's action for every env's current wind and yaws -> action_out f32[B, N]
int wg_yaw_table_geometry_(wg_yaw_table t, int* N, int* device);
void wg_launch_yaw_table_act_(wg_yaw_table t, const WgParams* p, const WgPtrs* d, float* action_out, hipStream_t st);
// wg_flow.hip
void wg_launch_flow(const FlowP* p, const FlowPtrs* d, int mode, const float* actions, const uint8_t* mask, int chunk, hipStream_t st);
void wg_launch_windspeed(const FlowP* p, const FlowPtrs* d, int e, int farm, const float* xs, int nx, const float* ys, int ny, float z,
                         int include_wakes, float* out, hipStream_t st);
// wg_env.hip, wg_envb.hip
void wg_launch_flow_env(const FlowP* p, const FlowPtrs* d, int mode, const float* actions, const uint8_t* mask, int chunk, hipStream_t st);
void wg_launch_flow_envb(const FlowP* p, const FlowPtrs* d, int mode, const float* actions, const uint8_t* mask, int chunk, hipStream_t st);
void wg_launch_step_env(const FlowP* p, const FlowPtrs* d, const WgParams* gp, const WgPtrs* gd, const float* actions, float* obs, float* reward,
                        uint8_t* trunc, float* final_obs, hipStream_t st);
void wg_launch_step_envb(const FlowP* p, const FlowPtrs* d, const WgParams* gp, const WgPtrs* gd, const float* actions, float* obs, float* reward,
                         uint8_t* trunc, float* final_obs, hipStream_t st);
// wg_kernels.hip
void wg_launch_glue(const WgParams* p, const WgPtrs* d, int phase, const uint8_t* mask, float* obs, float* reward, uint8_t* trunc,
                    float* final_obs, hipStream_t st, const WgParams* gp, const WgPtrs* gd);
void wg_launch_init(const WgParams* p, const WgPtrs* d, const uint8_t* mask, const uint64_t* seeds, hipStream_t st);
void wg_launch_create(const WgParams* p, const WgPtrs* d, hipStream_t st);
void wg_launch_obs_multi(const WgParams* p, const WgPtrs* d, float* out, hipStream_t st);
void wg_launch_info(const WgParams* p, const WgPtrs* d, int field, void* out, hipStream_t st);
void wg_launch_metrics(const WgParams* p, const WgPtrs* d, float* out, int reset_after, hipStream_t st);
void wg_launch_measurements(const WgParams* p, const WgPtrs* d, float* out, hipStream_t st);
void wg_launch_unready(const WgParams* p, const WgPtrs* d, const uint8_t* mask, int* out, hipStream_t st);
void wg_launch_box_repack(const float* planar, void* out, int nx, int ny, int nz, hipStream_t st);
void wg_launch_box_coarsen(const void* fine, void* out, int nx, int ny, int nz, hipStream_t st);
void wg_launch_box_stencil(const void* fine, void* out, int nx, int ny, int nz, hipStream_t st);
// wg_steady.hip (sp: SteadyP, wg_steady.h)
void wg_launch_steady(const void* sp, const float* ws, const float* wd, const float* ti, const float* yaw, float* power, hipStream_t st);
size_t wg_steady_srf_lds(int N, int yaw_n);      // bytes of LDS a k_steady_srf workgroup takes
void wg_launch_steady_srf(const void* sp, const float* ws, const float* wd, const float* ti, int refine_pass_n, int yaw_n,
                          const double* offsets, double yaw_clip, double* yaw, double* power, int* order, hipStream_t st);
}
