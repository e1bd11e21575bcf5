"""ctypes binding of libwindgym_hip.so (C ABI in include/windgym_hip.h) on PyTorch-ROCm tensors.

PyTorch is plumbing here: it owns the I/O device buffers and the HIP stream; all compute happens in the
hand-written kernels behind the C ABI.  There is NO CPU fallback: constructing a :class:`HipBatch` without
the built library or without a GPU raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import sys

import numpy as np

from .config import INFO, INFO_INT, WG_N_METRICS, CConfig, EnvConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
# Measurement hooks, honoured ONLY with WG_DEBUG_HOOKS=1 (tools/ab.sh sets it) and announced on stderr when active:
#   WG_LIB      alternative build of the same library (same-box A/B measurements of kernel variants)
#   WG_NOCHECK  HipBatch.check() only synchronises (profiling builds that ablate parts of the kernels)
_HOOKS = os.environ.get("WG_DEBUG_HOOKS") == "1"
LIB_PATH = os.path.join(_HERE, "libwindgym_hip.so")
if _HOOKS and os.environ.get("WG_LIB"):
    LIB_PATH = os.environ["WG_LIB"]
    print(f"[windgym] WG_DEBUG_HOOKS: loading {LIB_PATH} instead of the in-tree library", file=sys.stderr)
_NOCHECK = bool(_HOOKS and os.environ.get("WG_NOCHECK"))
if _NOCHECK:
    print("[windgym] WG_DEBUG_HOOKS: WG_NOCHECK set — HipBatch.check() does not read the device error word", file=sys.stderr)
# The library's own hooks (wg_api.hip: wg_hooks_read), by the name of the WgHooks field each one fills: what selects a kernel
# variant or a step path.  The first ten are the plan's integer hooks in the order of tests/plan_shim.cpp's array.
HOOK_ENV = {
    "flow_block": "WG_FLOW_BLOCK", "flow_res": "WG_FLOW_RES", "flow_env": "WG_FLOW_ENV", "env_wpe": "WG_ENV_WPE",
    "env_split": "WG_ENV_SPLIT", "step_fused": "WG_STEP_FUSED", "sums": "WG_SUMS", "lds_pad": "WG_LDS_PAD", "lf_cap": "WG_LF_CAP",
    "pstride_pad": "WG_PSTRIDE_PAD", "step_graph": "WG_STEP_GRAPH", "share_dev": "WG_ENV_SHARE_DEV",
    "first_obs_gl_only": "WG_FIRST_OBS_GL_ONLY", "no_box8": "WG_NO_BOX8",
}
# ... and the two that select nothing: WG_DEBUG prints the plan of a handle, WG_TIMELINE_OUT names the file of a -DWG_TIMELINE build
HOOK_ENV_DIAGNOSTIC = {"debug": "WG_DEBUG", "timeline_out": "WG_TIMELINE_OUT"}


@contextlib.contextmanager
def debug_hooks(mapping):
    """The given WG_* variables for the length of the block (the library reads them at wg_create, WG_NO_BOX8 again in the box
    setters); afterwards every one is what it was before — its old value or unset — whatever happened inside.  Refuses where
    WG_DEBUG_HOOKS is not "1": the library would ignore the hooks and the caller would measure or test the default kernel."""
    if mapping and os.environ.get("WG_DEBUG_HOOKS") != "1":
        raise WindGymHipError(f"debug_hooks({sorted(mapping)}): WG_DEBUG_HOOKS is not 1 in the environment, the library ignores its hooks")
    before = {k: os.environ.get(k) for k in mapping}
    os.environ.update({k: str(v) for k, v in mapping.items()})
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


UINT64_MAX = 0xFFFFFFFFFFFFFFFF

# every symbol include/windgym_hip.h declares (tests check the built library exports all of them)
ABI_SYMBOLS = (
    "wg_last_error", "wg_abi_version", "wg_create", "wg_destroy", "wg_obs_dim", "wg_hist_max",
    "wg_set_turbulence_box", "wg_set_turbulence_boxes", "wg_set_added_turbulence_box", "wg_set_deficit_table", "wg_set_box_ids", "wg_set_wind", "wg_set_wind_device", "wg_set_flow_script", "wg_reset", "wg_step", "wg_set_step_graph", "wg_check", "wg_obs_multi", "wg_set_obs_multi_buffer",
    "wg_set_final_obs_multi_buffer", "wg_rollout_multi", "wg_gae_shared",
    "wg_get_info", "wg_get_measurements", "wg_get_windspeed", "wg_metrics", "wg_get_state", "wg_set_state", "wg_generate_mann_box", "wg_mann_beta_table", "wg_steady_power", "wg_steady_optimize", "wg_kernel_timing", "wg_added_lookups", "wg_algorithmic_bytes", "wg_flow_variant",
    "wg_policy_create", "wg_policy_destroy", "wg_policy_set_params", "wg_policy_n_params", "wg_policy_act", "wg_rollout",
    "wg_gae", "wg_ppo_create", "wg_ppo_destroy", "wg_ppo_get_state", "wg_ppo_set_state", "wg_ppo_grad", "wg_ppo_apply", "wg_ppo_update",
    "wg_policy_create_vf", "wg_ppo_grad_shared", "wg_ppo_update_shared", "wg_ppo_set_kl_lr", "wg_lstm_ppo_set_kl_lr",
    "wg_pop_create", "wg_pop_destroy", "wg_pop_act", "wg_pop_rollout", "wg_gae_pop", "wg_pop_update",
    "wg_curriculum_create", "wg_curriculum_destroy", "wg_curriculum_get_state", "wg_curriculum_set_state", "wg_curriculum_set_targets",
    "wg_curriculum_shape",
    "wg_bc_grad", "wg_bc_update", "wg_expert_labels", "wg_expert_labels_check",
    "wg_yaw_table_create", "wg_yaw_table_destroy", "wg_yaw_table_rows", "wg_yaw_table_targets", "wg_yaw_table_act", "wg_rollout_table",
    "wg_norm_create", "wg_norm_destroy", "wg_norm_get_state", "wg_norm_set_state", "wg_norm_set_training", "wg_norm_reset_returns",
    "wg_norm_obs", "wg_norm_reward", "wg_rollout_norm",
    "wg_lstm_create", "wg_lstm_destroy", "wg_lstm_n_params", "wg_lstm_set_params", "wg_lstm_step", "wg_lstm_act", "wg_rollout_lstm",
    "wg_lstm_ppo_create", "wg_lstm_ppo_destroy", "wg_lstm_ppo_n_params", "wg_lstm_ppo_get_state", "wg_lstm_ppo_set_state",
    "wg_lstm_ppo_grad", "wg_lstm_ppo_apply", "wg_lstm_ppo_update", "wg_lstm_bc_grad", "wg_lstm_bc_update",
    "wg_lstm_pop_create", "wg_lstm_pop_destroy", "wg_lstm_pop_act", "wg_lstm_pop_rollout", "wg_lstm_pop_update",
)

_lib = None

WG_POLICY_MAX_HIDDEN = 4
WG_POP_MAX = 16
ACTV = {"tanh": 0, "relu": 1}


class CPolicyDesc(C.Structure):
    """wg_policy_desc"""
    _fields_ = [("n_in", C.c_int32), ("n_out", C.c_int32), ("activation", C.c_int32),
                ("n_hidden_pi", C.c_int32), ("hidden_pi", C.c_int32 * WG_POLICY_MAX_HIDDEN),
                ("n_hidden_vf", C.c_int32), ("hidden_vf", C.c_int32 * WG_POLICY_MAX_HIDDEN),
                ("has_log_std", C.c_int32)]


class CRolloutBufs(C.Structure):
    """wg_rollout_bufs"""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("raw", C.c_void_p), ("logp", C.c_void_p),
                ("value", C.c_void_p), ("final_obs", C.c_void_p), ("final_value", C.c_void_p), ("reward", C.c_void_p),
                ("truncated", C.c_void_p), ("n_info", C.c_int32), ("info_fields", C.POINTER(C.c_int32)),
                ("info_out", C.POINTER(C.c_void_p))]


class CRolloutMultiBufs(C.Structure):
    """wg_rollout_multi_bufs"""
    _fields_ = [("obs_multi", C.c_void_p), ("actions", C.c_void_p), ("raw", C.c_void_p), ("logp", C.c_void_p),
                ("value", C.c_void_p), ("final_obs_multi", C.c_void_p), ("final_value", C.c_void_p), ("reward", C.c_void_p),
                ("truncated", C.c_void_p), ("obs", C.c_void_p), ("final_obs", C.c_void_p), ("n_info", C.c_int32),
                ("info_fields", C.POINTER(C.c_int32)), ("info_out", C.POINTER(C.c_void_p))]


class CPpoBatch(C.Structure):
    """wg_ppo_batch"""
    _fields_ = [("obs", C.c_void_p), ("raw", C.c_void_p), ("logp", C.c_void_p), ("advantage", C.c_void_p),
                ("returns", C.c_void_p), ("n_rows", C.c_int64)]


class CPpoBatchShared(C.Structure):
    """wg_ppo_batch_shared"""
    _fields_ = [("rows", CPpoBatch), ("obs_vf", C.c_void_p), ("agents", C.c_int32)]


class CPpoHyper(C.Structure):
    """wg_ppo_hyper"""
    _fields_ = [("clip_range", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float), ("normalize_advantage", C.c_int32)]


class CKlLr(C.Structure):
    """wg_kl_lr"""
    _fields_ = [("desired_kl", C.c_float), ("factor", C.c_float), ("lr_min", C.c_float), ("lr_max", C.c_float)]


class CNormDesc(C.Structure):
    """wg_norm_desc"""
    _fields_ = [("n_obs", C.c_int32), ("n_envs", C.c_int32), ("norm_obs", C.c_int32), ("norm_reward", C.c_int32),
                ("clip_obs", C.c_float), ("clip_reward", C.c_float), ("gamma", C.c_double), ("epsilon", C.c_double)]


class CLstmDesc(C.Structure):
    """wg_lstm_desc"""
    _fields_ = [("n_in", C.c_int32), ("hidden", C.c_int32), ("n_nets", C.c_int32)]


class CRolloutLstmBufs(C.Structure):
    """wg_rollout_lstm_bufs"""
    _fields_ = [("state", C.c_void_p), ("state0", C.c_void_p), ("episode_start", C.c_void_p), ("scratch", C.c_void_p)]


LSTM_ACTOR, LSTM_CRITIC = 1, 2          # WG_LSTM_ACTOR / WG_LSTM_CRITIC
class CLstmPpoBatch(C.Structure):
    """wg_lstm_ppo_batch"""
    _fields_ = [("obs", C.c_void_p), ("raw", C.c_void_p), ("logp", C.c_void_p), ("advantage", C.c_void_p), ("returns", C.c_void_p),
                ("episode_start", C.c_void_p), ("lstm_state0", C.c_void_p), ("T", C.c_int32), ("B", C.c_int32)]


class CLstmBcBatch(C.Structure):
    """wg_lstm_bc_batch"""
    _fields_ = [("obs", C.c_void_p), ("target", C.c_void_p), ("returns", C.c_void_p), ("episode_start", C.c_void_p),
                ("lstm_state0", C.c_void_p), ("T", C.c_int32), ("B", C.c_int32)]


class CBcBatch(C.Structure):
    """wg_bc_batch"""
    _fields_ = [("obs", C.c_void_p), ("target", C.c_void_p), ("returns", C.c_void_p), ("n_rows", C.c_int64)]


class CBcHyper(C.Structure):
    """wg_bc_hyper"""
    _fields_ = [("loss", C.c_int32), ("ent_coef", C.c_float), ("vf_coef", C.c_float)]


BC_LOSS = {"mse": 0, "nll": 1}          # WG_BC_MSE / WG_BC_NLL
BC_STATS = ("loss", "mse", "nll", "entropy", "v_loss", "mean_abs_err", "reserved0", "reserved1")   # wg_bc_stats
PPO_STATS = ("pi_loss", "v_loss", "entropy", "approx_kl", "clip_fraction", "loss", "adv_mean", "adv_std")   # wg_ppo_stats


class WindGymHipError(RuntimeError):
    pass


def load_library():
    """Load libwindgym_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WindGymHipError(
            f"{LIB_PATH} is missing: build it with `python -m windgym_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the step() path.")
    # torch first: its bundled HIP runtime must be the one the process initialises — loading ours against the
    # system libamdhip64 before `import torch` leaves two runtimes in the process and hipSetDevice then fails with
    # "no ROCm-capable device is detected"
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    L.wg_last_error.restype = C.c_char_p
    L.wg_create.argtypes = [C.POINTER(CConfig), C.c_int, C.POINTER(C.c_void_p)]
    L.wg_destroy.argtypes = [C.c_void_p]
    L.wg_obs_dim.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.wg_hist_max.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.wg_set_turbulence_box.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                        C.c_double, C.c_double]
    L.wg_set_box_ids.argtypes = [C.c_void_p, C.c_void_p]
    L.wg_set_deficit_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                       C.c_int, C.c_double, C.c_int, C.c_double]
    L.wg_set_added_turbulence_box.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                              C.c_double, C.c_double]
    L.wg_set_turbulence_boxes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_double, C.c_double, C.c_double]
    L.wg_set_flow_script.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.wg_set_wind.argtypes = [C.c_void_p, C.c_void_p]
    L.wg_set_wind_device.argtypes = [C.c_void_p, C.c_void_p]
    L.wg_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_step.argtypes = [C.c_void_p] + [C.c_void_p] * 6
    L.wg_set_step_graph.argtypes = [C.c_void_p, C.c_int]
    L.wg_check.argtypes = [C.c_void_p, C.c_void_p]
    L.wg_obs_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_set_obs_multi_buffer.argtypes = [C.c_void_p, C.c_void_p]
    L.wg_get_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.wg_get_measurements.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_get_windspeed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                   C.c_int, C.c_void_p, C.c_void_p]
    L.wg_metrics.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.wg_get_state.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    L.wg_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.wg_kernel_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.wg_added_lookups.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.wg_generate_mann_box.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                       C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_void_p, C.c_void_p]
    L.wg_steady_power.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    L.wg_steady_optimize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                     C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_mann_beta_table.argtypes = [C.c_double, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double)]
    L.wg_algorithmic_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.wg_flow_variant.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.wg_policy_create.argtypes = [C.POINTER(CPolicyDesc), C.c_int, C.POINTER(C.c_void_p)]
    L.wg_policy_create_vf.argtypes = [C.POINTER(CPolicyDesc), C.c_int32, C.c_int, C.POINTER(C.c_void_p)]
    L.wg_policy_destroy.argtypes = [C.c_void_p]
    L.wg_policy_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.wg_policy_n_params.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.wg_policy_act.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_rollout.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                             C.POINTER(CRolloutBufs), C.c_void_p]
    L.wg_set_final_obs_multi_buffer.argtypes = [C.c_void_p, C.c_void_p]
    L.wg_rollout_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                   C.POINTER(CRolloutMultiBufs), C.c_void_p]
    L.wg_gae_shared.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_gae.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p,
                         C.c_void_p, C.c_void_p]
    L.wg_ppo_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    for fam in ("wg_ppo", "wg_lstm_ppo"):                       # what the two optimiser handles share (ppo.HandleOptimizer)
        getattr(L, fam + "_destroy").argtypes = [C.c_void_p]
        getattr(L, fam + "_get_state").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
        getattr(L, fam + "_set_state").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]
        getattr(L, fam + "_apply").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
        getattr(L, fam + "_set_kl_lr").argtypes = [C.c_void_p, C.POINTER(CKlLr), C.c_void_p]
    L.wg_ppo_grad.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CPpoBatch), C.c_void_p, C.c_int64, C.c_int,
                              C.POINTER(CPpoHyper), C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_ppo_update.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CPpoBatch), C.c_void_p, C.c_int, C.c_int,
                                C.POINTER(CPpoHyper), C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.wg_ppo_grad_shared.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CPpoBatchShared)] + L.wg_ppo_grad.argtypes[3:]
    L.wg_ppo_update_shared.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CPpoBatchShared)] + L.wg_ppo_update.argtypes[3:]
    L.wg_bc_grad.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CBcBatch), C.c_void_p, C.c_int64, C.c_int,
                             C.POINTER(CBcHyper), C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_bc_update.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CBcBatch), C.c_void_p, C.c_int, C.c_int,
                               C.POINTER(CBcHyper), C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.wg_expert_labels.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5
    L.wg_expert_labels_check.argtypes = [C.c_void_p, C.c_void_p]
    L.wg_yaw_table_create.argtypes = [C.c_int] + [C.c_void_p, C.c_int] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.wg_yaw_table_destroy.argtypes = [C.c_void_p]
    L.wg_yaw_table_rows.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    L.wg_yaw_table_targets.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
    L.wg_yaw_table_act.argtypes = [C.c_void_p] * 4
    L.wg_rollout_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(CRolloutBufs), C.c_void_p]
    L.wg_pop_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
    L.wg_pop_destroy.argtypes = [C.c_void_p]
    L.wg_pop_act.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64),
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_pop_rollout.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64),
                                 C.POINTER(CRolloutBufs), C.c_void_p]
    L.wg_gae_pop.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float),
                             C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_pop_update.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(CPpoBatch), C.c_void_p, C.c_int, C.c_int,
                                C.POINTER(CPpoHyper), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    L.wg_curriculum_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.wg_curriculum_destroy.argtypes = [C.c_void_p]
    L.wg_curriculum_get_state.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    L.wg_curriculum_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.wg_curriculum_set_targets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_curriculum_shape.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_double] + [C.c_void_p] * 5
    L.wg_norm_create.argtypes = [C.POINTER(CNormDesc), C.c_int, C.POINTER(C.c_void_p)]
    L.wg_norm_destroy.argtypes = [C.c_void_p]
    L.wg_norm_get_state.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    L.wg_norm_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.wg_norm_set_training.argtypes = [C.c_void_p, C.c_int]
    L.wg_norm_reset_returns.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_norm_obs.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    L.wg_norm_reward.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    L.wg_rollout_norm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                  C.POINTER(CRolloutBufs), C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_lstm_create.argtypes = [C.POINTER(CLstmDesc), C.c_int, C.POINTER(C.c_void_p)]
    L.wg_lstm_destroy.argtypes = [C.c_void_p]
    L.wg_lstm_n_params.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.wg_lstm_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.wg_lstm_step.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    L.wg_lstm_act.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64] + [C.c_void_p] * 5
    L.wg_rollout_lstm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                  C.POINTER(CRolloutBufs), C.POINTER(CRolloutLstmBufs), C.c_void_p]
    L.wg_lstm_ppo_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.wg_lstm_ppo_n_params.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.wg_lstm_ppo_grad.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CLstmPpoBatch), C.c_void_p, C.c_int, C.POINTER(CPpoHyper),
                                   C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_lstm_ppo_update.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CLstmPpoBatch), C.c_void_p, C.c_int, C.c_int,
                                     C.POINTER(CPpoHyper), C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.wg_lstm_bc_grad.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CLstmBcBatch), C.c_void_p, C.c_int, C.POINTER(CBcHyper),
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.wg_lstm_bc_update.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CLstmBcBatch), C.c_void_p, C.c_int, C.c_int,
                                    C.POINTER(CBcHyper), C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.wg_lstm_pop_create.argtypes = [C.POINTER(C.c_void_p)] * 3 + [C.c_int, C.POINTER(C.c_void_p)]
    L.wg_lstm_pop_destroy.argtypes = [C.c_void_p]
    L.wg_lstm_pop_act.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64)] + [C.c_void_p] * 5
    L.wg_lstm_pop_rollout.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64),
                                      C.POINTER(CRolloutBufs), C.POINTER(CRolloutLstmBufs), C.c_void_p]
    L.wg_lstm_pop_update.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(CLstmPpoBatch), C.c_void_p, C.c_int, C.c_int,
                                     C.POINTER(CPpoHyper), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    _lib = L
    return L


def _chk(rc, what):
    if rc != 0:
        msg = load_library().wg_last_error().decode(errors="replace")
        if rc == -4:
            raise Exception("NaN Power")                       # Wind_Farm_Env.py:980-981
        if rc == -2:
            raise NotImplementedError(msg)
        if rc == -1:
            raise ValueError(msg)
        raise WindGymHipError(f"{what} failed (rc={rc}): {msg}")


def device_tensor(x, dtype):
    """What every tensor handed to the library must be: a contiguous CUDA tensor of ``dtype`` (its size is the caller's to check)."""
    import torch
    return isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dtype and x.is_contiguous()


def tensor_ptr(x, dtype, message, numel=None, at_least=None, shape=None, device=None):
    """``x.data_ptr()`` of a :func:`device_tensor` — where given: of ``numel`` elements, of ``at_least`` that many, of ``shape``, on
    ``device`` — or ``ValueError(message)``."""
    if not (device_tensor(x, dtype) and (numel is None or x.numel() == numel) and (at_least is None or x.numel() >= at_least)
            and (shape is None or tuple(x.shape) == tuple(shape)) and (device is None or x.device == device)):
        raise ValueError(message)
    return x.data_ptr()


class Handle:
    """What every wrapper of a handle of the library is: ``L`` the library, the raw handle in ``_h`` (``handle_attr``; None once
    closed) and ``destroy``, the entry that frees it.  ``_stream`` wants ``torch`` and ``device`` of the subclass."""

    destroy, handle_attr = None, "_h"

    def close(self):
        """``<destroy>(handle)``, once: a closed or never opened wrapper has nothing to free."""
        h = getattr(self, self.handle_attr, None)
        if h:
            setattr(self, self.handle_attr, None)
            getattr(self.L, self.destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _blob(self, get_entry):
        """The handle's state blob by the two calls of ``get_entry``: the size, then the bytes."""
        get, n = getattr(self.L, get_entry), C.c_size_t(0)
        _chk(get(self._h, None, C.byref(n)), get_entry)
        buf = (C.c_char * n.value)()
        _chk(get(self._h, buf, C.byref(n)), get_entry)
        return bytes(buf)


class HipBatch(Handle):
    """A batch of ``cfg.n_envs`` farms resident on one MI355X."""

    destroy = "wg_destroy"

    def __init__(self, cfg: EnvConfig, device: int | None = None):
        import torch
        if not torch.cuda.is_available():
            raise WindGymHipError("no HIP device visible: the step() path only runs on the GPU "
                                  "(no CPU fallback; the CPU restatement under oracle/ is test-only)")
        self.torch = torch
        self.L = load_library()
        self.cfg = cfg
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self._c = cfg.to_c()
        h = C.c_void_p()
        _chk(self.L.wg_create(C.byref(self._c), self.device_index, C.byref(h)), "wg_create")
        self._h = h
        o, om = C.c_int(), C.c_int()
        self.L.wg_obs_dim(self._h, C.byref(o), C.byref(om))
        self.obs_dim, self.obs_dim_multi = o.value, om.value
        self.B, self.N = cfg.n_envs, cfg.n_turb
        f32 = dict(dtype=torch.float32, device=self.device)
        self.obs = torch.zeros((self.B, self.obs_dim), **f32)
        self.final_obs = torch.zeros((self.B, self.obs_dim), **f32)
        self.reward = torch.zeros(self.B, **f32)
        self.truncated = torch.zeros(self.B, dtype=torch.uint8, device=self.device)
        self._metrics = torch.zeros(WG_N_METRICS, **f32)
        # step() hot path: the persistent output pointers and the bound C function, prepared once
        self._out_ptrs = (self.obs.data_ptr(), self.reward.data_ptr(), self.truncated.data_ptr(),
                          self.final_obs.data_ptr())
        self._wg_step = self.L.wg_step
        self._cur_stream = torch.cuda.current_stream
        self._script = None
        self._box = None

    # -- API ----------------------------------------------------------------------------------------
    def reset(self, seeds=None, mask=None):
        sp = mp = None
        if seeds is not None:
            s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(self.B))
            sp = s.ctypes.data_as(C.c_void_p)
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint8).reshape(self.B))
            mp = m.ctypes.data_as(C.c_void_p)
        if self._c.added_turbulence and not getattr(self, "_abox_set", False):
            from .mann import default_added_box
            self.set_added_turbulence_box(*default_added_box())
        if self._c.deficit_model == 2 and getattr(self, "_dtab", None) is None:
            from .ainslie import deficit_table
            self.set_deficit_table(*deficit_table())
        _chk(self.L.wg_reset(self._h, mp, sp, C.c_void_p(self.obs.data_ptr()), self._stream()), "wg_reset")
        return self.obs

    def step(self, actions):
        """actions: float32 CUDA tensor [B, N].  Returns views of the persistent output tensors."""
        if not (actions.is_cuda and actions.dtype == self.torch.float32 and actions.is_contiguous()
                and actions.numel() == self.B * self.N):
            raise ValueError("step(): actions must be a contiguous float32 CUDA tensor [B, N]")
        o, r, t, f = self._out_ptrs
        rc = self._wg_step(self._h, actions.data_ptr(), o, r, t, f, self._cur_stream(self.device).cuda_stream)
        if rc:
            _chk(rc, "wg_step")
        return self.obs, self.reward, self.truncated, self.final_obs

    # a rollout's ``bufs`` are keyed by the field names of wg_rollout_bufs; these fields go by another key
    MULTI_KEYS = {"obs_multi": "obs", "final_obs_multi": "final_obs", "obs": "flat_obs", "final_obs": "flat_final_obs"}   # wg_rollout_multi_bufs
    LSTM_KEYS = {"state": "lstm_state", "state0": "lstm_state0", "scratch": "lstm_scratch"}                             # wg_rollout_lstm_bufs

    def rollout(self, entry, handles, n_steps, bufs, record, noise=None, members=None, tail=()):
        """The closed-loop entry ``entry`` (windgym_hip.h: wg_rollout, wg_rollout_multi, wg_rollout_norm, wg_rollout_table,
        wg_pop_rollout, wg_rollout_lstm, wg_lstm_pop_rollout) on ``handles``, the raw handles its signature names after the env's.
        ``bufs``: contiguous CUDA tensors, one per pointer field of the buffer structs the entry takes, in the order of their
        ``_fields_`` (a missing one of wg_rollout_bufs / wg_rollout_multi_bufs is NULL = not wanted), one per info name in
        ``record``, and one per key in ``tail``, the pointers that end the signature.  ``noise``: ``(deterministic, seed, counter0,
        row_offset)``, or None for an entry that samples nothing; with ``members = P`` the per-member arrays of a population that
        samples as ONE policy on the whole batch would: every member the one seed, member ``m``'s rows from ``row_offset + m * B / P``."""
        fn = getattr(self.L, entry)
        multi = C.POINTER(CRolloutMultiBufs) in fn.argtypes
        cls, n = CRolloutMultiBufs if multi else CRolloutBufs, len(record)
        keys = [self.MULTI_KEYS.get(f, f) if multi else f for f, ty in cls._fields_ if ty is C.c_void_p]
        structs = [cls(*[bufs[k].data_ptr() if k in bufs else None for k in keys], n, (C.c_int32 * max(1, n))(*[INFO[r] for r in record]),
                       (C.c_void_p * max(1, n))(*[bufs[r].data_ptr() for r in record]))]
        if C.POINTER(CRolloutLstmBufs) in fn.argtypes:
            structs.append(CRolloutLstmBufs(*[bufs[self.LSTM_KEYS.get(f, f)].data_ptr() for f, _ in CRolloutLstmBufs._fields_]))
        if noise is not None:
            deterministic, seed, counter0, row_offset = noise
            if members:
                P = int(members)
                seed, row_offset = (C.c_uint64 * P)(*[int(seed)] * P), (C.c_uint64 * P)(*[int(row_offset) + m * (self.B // P) for m in range(P)])
            noise = (int(bool(deterministic)), seed, counter0, row_offset)
        _chk(fn(self._h, *handles, int(n_steps), *(noise or ()), *[C.byref(x) for x in structs], *[bufs[k].data_ptr() for k in tail],
                self._stream()), entry)

    def set_step_graph(self, enable=True):
        """step() as one hipGraphLaunch (captured per distinct set of I/O pointers) instead of direct launches."""
        _chk(self.L.wg_set_step_graph(self._h, int(bool(enable))), "wg_set_step_graph")

    def check(self):
        if _NOCHECK:          # profiling builds that ablate parts of the kernels (tools/ab.sh)
            self.torch.cuda.synchronize()
            return
        _chk(self.L.wg_check(self._h, self._stream()), "wg_check")

    def obs_multi(self):
        out = self.torch.zeros((self.B, self.N, self.obs_dim_multi), dtype=self.torch.float32, device=self.device)
        _chk(self.L.wg_obs_multi(self._h, C.c_void_p(out.data_ptr()), self._stream()), "wg_obs_multi")
        return out

    def fuse_obs_multi(self, enable=True):
        """Let every following step() / reset() also write the per-agent observations (PettingZoo facade) into a
        persistent tensor [B, N, obs_dim_multi] — returned here, updated in place — instead of a separate
        obs_multi() launch per step."""
        if not enable:
            _chk(self.L.wg_set_obs_multi_buffer(self._h, None), "wg_set_obs_multi_buffer")
            self._multi_buf = self._multi_fin = None      # (the library drops the final buffer with it)
            return None
        t = self.torch
        self._multi_buf = t.zeros((self.B, self.N, self.obs_dim_multi), dtype=t.float32, device=self.device)
        _chk(self.L.wg_set_obs_multi_buffer(self._h, C.c_void_p(self._multi_buf.data_ptr())), "wg_set_obs_multi_buffer")
        return self._multi_buf

    def fuse_final_obs_multi(self, enable=True):
        """After ``fuse_obs_multi()``: let every following step() also write the per-agent observation of the state the step
        ENDED in — a truncating env's finished episode, every other env's rows of the per-agent buffer — into a persistent
        tensor [B, N, obs_dim_multi], returned here and updated in place (wg_set_final_obs_multi_buffer)."""
        if not enable:
            _chk(self.L.wg_set_final_obs_multi_buffer(self._h, None), "wg_set_final_obs_multi_buffer")
            self._multi_fin = None
            return None
        t = self.torch
        buf = t.zeros((self.B, self.N, self.obs_dim_multi), dtype=t.float32, device=self.device)
        _chk(self.L.wg_set_final_obs_multi_buffer(self._h, C.c_void_p(buf.data_ptr())), "wg_set_final_obs_multi_buffer")
        self._multi_fin = buf
        return buf

    def measurements(self):
        """Unscaled sensor values in the layout of the observation, f32[B, O]."""
        out = self.torch.zeros((self.B, self.obs_dim), dtype=self.torch.float32, device=self.device)
        _chk(self.L.wg_get_measurements(self._h, C.c_void_p(out.data_ptr()), self._stream()), "wg_get_measurements")
        return out

    def windspeed(self, env, x, y, z=None, farm=0, include_wakes=True):
        """(u, v, w) of one farm of one env on the grid x[nx] x y[ny] at height z (default: hub height), flow frame:
        f32[3, nx, ny] — fs.get_windspeed(XYView(...)) of the reference (Wind_Farm_Env.py:1040-1083)."""
        t = self.torch
        xs = t.as_tensor(x, dtype=t.float32, device=self.device).contiguous()
        ys = t.as_tensor(y, dtype=t.float32, device=self.device).contiguous()
        out = t.empty((3, xs.numel(), ys.numel()), dtype=t.float32, device=self.device)
        zz = float(self.cfg.tab.hub_height() if z is None else z)
        _chk(self.L.wg_get_windspeed(self._h, C.c_int(int(env)), C.c_int(int(farm)), C.c_void_p(xs.data_ptr()),
                                     C.c_int(xs.numel()), C.c_void_p(ys.data_ptr()), C.c_int(ys.numel()),
                                     C.c_float(zz), C.c_int(1 if include_wakes else 0), C.c_void_p(out.data_ptr()),
                                     self._stream()), "wg_get_windspeed")
        return out

    def info_shape(self, name):
        """(shape, torch dtype) of ``info(name)``."""
        t = self.torch
        per_turb = name in ("yaw_agent", "yaw_base", "ws_turb", "wd_turb", "power_turb_agent",
                            "power_turb_base", "ws_turb_base", "turb_x", "turb_y")
        if name == "wind_f64":
            return (self.B, 3), t.float64
        if name.startswith("rotor_uvw"):
            shape = (self.B, self.N, 3)
        elif per_turb:
            shape = (self.B, self.N)
        else:
            shape = (self.B,)
        return shape, (t.int32 if name in INFO_INT else t.float32)

    def info(self, name, out=None):
        """One field of the lazy info dict as a new CUDA tensor, or written into ``out`` (a contiguous CUDA tensor of
        ``info_shape(name)``, e.g. row 0 of a recording) and returned."""
        t = self.torch
        shape, dtype = self.info_shape(name)
        if out is None:
            out = t.zeros(shape, dtype=dtype, device=self.device)
        else:
            tensor_ptr(out, dtype, f"info({name!r}, out=): out must be a contiguous CUDA tensor of shape {shape} and dtype {dtype}", shape=shape)
        _chk(self.L.wg_get_info(self._h, INFO[name], C.c_void_p(out.data_ptr()), self._stream()), "wg_get_info")
        return out

    def metrics(self, reset_after=False):
        _chk(self.L.wg_metrics(self._h, C.c_void_p(self._metrics.data_ptr()), int(reset_after), self._stream()),
             "wg_metrics")
        return self._metrics

    def set_wind(self, ws=None, wd=None, ti=None):
        """Fix the wind conditions per env (arrays of length B or scalars; None keeps the sampled value)."""
        if ws is None and wd is None and ti is None:
            _chk(self.L.wg_set_wind(self._h, None), "wg_set_wind")
            return
        w = np.full((self.B, 3), np.nan)
        for k, v in enumerate((ws, wd, ti)):
            if v is not None:
                w[:, k] = np.broadcast_to(np.asarray(v, dtype=np.float64), (self.B,))
        w = np.ascontiguousarray(w)
        _chk(self.L.wg_set_wind(self._h, w.ctypes.data_as(C.c_void_p)), "wg_set_wind")

    def set_box_ids(self, ids):
        """Box of the pool each env uses from the next reset on (FarmEval.update_tf per env); None = draw again."""
        if ids is None:
            _chk(self.L.wg_set_box_ids(self._h, None), "wg_set_box_ids")
            return
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(ids, dtype=np.int32), (self.B,)))
        _chk(self.L.wg_set_box_ids(self._h, a.ctypes.data_as(C.c_void_p)), "wg_set_box_ids")

    def set_wind_device(self, wind):
        """Borrow a CUDA float64 tensor [B, 3] = (ws, wd, ti; NaN = keep the sampled value) as the per-env wind
        override; the caller may rewrite it between steps (stream-ordered).  None removes it."""
        if wind is None:
            self._wind_dev = None
            _chk(self.L.wg_set_wind_device(self._h, None), "wg_set_wind_device")
            return
        t = self.torch
        assert device_tensor(wind, t.float64) and tuple(wind.shape) == (self.B, 3)
        self._wind_dev = wind                                   # keep it alive
        _chk(self.L.wg_set_wind_device(self._h, C.c_void_p(wind.data_ptr())), "wg_set_wind_device")

    def set_flow_script(self, uvw, power):
        """Replay mode (test hook).  uvw [F,T,B,N,3], power [F,T,B,N] (array-likes)."""
        t = self.torch
        if uvw is None:
            self._script = None
            _chk(self.L.wg_set_flow_script(self._h, None, None, 0), "wg_set_flow_script")
            return
        u = t.as_tensor(np.ascontiguousarray(uvw, dtype=np.float32), device=self.device).contiguous()
        p = t.as_tensor(np.ascontiguousarray(power, dtype=np.float32), device=self.device).contiguous()
        self._script = (u, p)
        _chk(self.L.wg_set_flow_script(self._h, C.c_void_p(u.data_ptr()), C.c_void_p(p.data_ptr()),
                                       int(u.shape[1])), "wg_set_flow_script")

    def set_turbulence_box(self, box, spacing):
        t = self.torch
        b = box if isinstance(box, t.Tensor) else t.as_tensor(np.ascontiguousarray(box, dtype=np.float32))
        b = b.to(self.device, dtype=t.float32).contiguous()
        assert b.ndim == 4 and b.shape[0] == 3
        self._box = b
        _chk(self.L.wg_set_turbulence_box(self._h, C.c_void_p(b.data_ptr()), int(b.shape[1]), int(b.shape[2]),
                                          int(b.shape[3]), float(spacing[0]), float(spacing[1]),
                                          float(spacing[2])), "wg_set_turbulence_box")

    def set_added_turbulence_box(self, box, spacing):
        """Isotropic unit-variance box of the wake-added turbulence (wg_config.added_turbulence); default:
        ``mann.default_added_box()`` installed at the first reset."""
        t = self.torch
        b = box if isinstance(box, t.Tensor) else t.as_tensor(np.ascontiguousarray(box, dtype=np.float32))
        b = b.to(self.device, dtype=t.float32).contiguous()
        assert b.ndim == 4 and b.shape[0] == 3
        _chk(self.L.wg_set_added_turbulence_box(self._h, C.c_void_p(b.data_ptr()), int(b.shape[1]), int(b.shape[2]),
                                                int(b.shape[3]), float(spacing[0]), float(spacing[1]),
                                                float(spacing[2])), "wg_set_added_turbulence_box")
        self._abox_set = True

    def set_deficit_table(self, table, spec):
        """Deficit table of ``deficit_model`` 2 (``ainslie.deficit_table()`` is installed at the first reset by default):
        table [n_ct, n_ti, n_x, n_r] of 1 - U / U0, ``spec`` its axes (ainslie.TABLE_SPEC)."""
        t = self.torch
        tb = t.as_tensor(np.ascontiguousarray(table, dtype=np.float32)).to(self.device).contiguous()
        assert tb.ndim == 4 and tb.shape[2] == spec["n_x"] and tb.shape[3] == spec["n_r"]
        _chk(self.L.wg_set_deficit_table(self._h, C.c_void_p(tb.data_ptr()), int(tb.shape[0]), float(spec["ct"][0]),
                                         float(spec["ct"][-1]), int(tb.shape[1]), float(spec["ti"][0]), float(spec["ti"][-1]),
                                         int(spec["n_x"]), float(spec["x_max_D"]), int(spec["n_r"]), float(spec["r_max_R"])),
             "wg_set_deficit_table")
        self._dtab = tb              # borrowed by the handle

    def set_turbulence_boxes(self, boxes, spacing):
        """Pool of K boxes of equal shape (turbtype "MannLoad": one TF_* file drawn per reset, :611-618)."""
        t = self.torch
        bs = []
        for box in boxes:
            b = box if isinstance(box, t.Tensor) else t.as_tensor(np.ascontiguousarray(box, dtype=np.float32))
            b = b.to(self.device, dtype=t.float32).contiguous()
            assert b.ndim == 4 and b.shape[0] == 3 and (not bs or b.shape == bs[0].shape)
            bs.append(b)
        ptrs = (C.c_void_p * len(bs))(*[b.data_ptr() for b in bs])
        _chk(self.L.wg_set_turbulence_boxes(self._h, ptrs, len(bs), int(bs[0].shape[1]), int(bs[0].shape[2]),
                                            int(bs[0].shape[3]), float(spacing[0]), float(spacing[1]),
                                            float(spacing[2])), "wg_set_turbulence_boxes")
        self._box = bs[0]      # (the library keeps its own copies; the caller's tensors may go)

    def get_state(self) -> bytes:
        return self._blob("wg_get_state")

    def set_state(self, blob: bytes):
        _chk(self.L.wg_set_state(self._h, blob, len(blob)), "wg_set_state")

    def kernel_timing(self, enable=True):
        """-> (flow kernel ms/launch, glue kernel ms/launch, launches timed, farm flow-steps per launch, wake particles
        streamed per launch).  enable: False/0 = stop, True/1 = time every step(), n > 1 = time every n-th step()."""
        f, g, n, fs, pt = C.c_double(), C.c_double(), C.c_int(), C.c_double(), C.c_double()
        _chk(self.L.wg_kernel_timing(self._h, int(enable), C.byref(f), C.byref(g), C.byref(n), C.byref(fs),
                                     C.byref(pt)), "wg_kernel_timing")
        return f.value, g.value, n.value, fs.value, pt.value

    def steady_power(self, ws, wd, ti, yaw, model="m0"):
        """Steady-state power per turbine [n_cases, N] (W) for the wind conditions ws / wd / ti [n_cases] and yaw vectors
        [n_cases, N] (degrees): ONE launch of k_steady (wg_steady_power).  model "m0" = the env's own flow model,
        "blondel_jimenez" = the reference PyWakeAgent's model."""
        t = self.torch
        f = lambda a: t.as_tensor(np.array(a, dtype=np.float32) if not isinstance(a, t.Tensor) else a, dtype=t.float32,
                                  device=self.device).contiguous()          # noqa: E731
        yaw = f(yaw).reshape(-1, self.cfg.n_turb)
        n = yaw.shape[0]
        ws, wd, ti = (f(a).reshape(-1).expand(n).contiguous() for a in (ws, wd, ti))
        out = t.empty((n, self.cfg.n_turb), dtype=t.float32, device=self.device)
        _chk(self.L.wg_steady_power(self._h, {"m0": 0, "blondel_jimenez": 1}[model], n, ws.data_ptr(), wd.data_ptr(),
                                    ti.data_ptr(), yaw.data_ptr(), out.data_ptr(), self._stream()), "wg_steady_power")
        return out

    def steady_optimize(self, ws, wd, ti, model="m0", refine_pass_n=8, yaw_n=9, yaw_max=30.0, return_order=False):
        """Serial-Refine optimal yaws for the wind conditions ws / wd / ti [C] (host arrays or CUDA tensors) in ONE launch of
        k_steady_srf (wg_steady_optimize), enqueued on the current stream: -> (yaw [C, N] float64 degrees, farm power [C]
        float64) CUDA tensors, and the visiting order [C, N] int32 with ``return_order``.  The result is what
        ``steady.yaw_optimizer_srf(..., batch=self)`` computes with one launch of k_steady per refine step; like it, this
        adds 1e-3 deg to wd (the tie of perfectly aligned rows)."""
        from .steady import MODEL_IDS, srf_offsets
        t = self.torch
        f = lambda a: (a.to(self.device, t.float64) if isinstance(a, t.Tensor) else                    # noqa: E731
                       t.as_tensor(np.array(a, dtype=np.float64), device=self.device)).reshape(-1)
        ws, wd, ti = f(ws), f(wd), f(ti)
        n = max(ws.numel(), wd.numel(), ti.numel())
        ws, wd, ti = (a.expand(n).to(t.float32).contiguous() for a in (ws, wd + 1e-3, ti))
        offs = srf_offsets(refine_pass_n, yaw_n, yaw_max).to(self.device)
        N = self.cfg.n_turb
        yaw = t.empty((n, N), dtype=t.float64, device=self.device)
        power = t.empty((n,), dtype=t.float64, device=self.device)
        order = t.empty((n, N), dtype=t.int32, device=self.device) if return_order else None
        _chk(self.L.wg_steady_optimize(self._h, MODEL_IDS[model], n, ws.data_ptr(), wd.data_ptr(), ti.data_ptr(), int(refine_pass_n),
                                       int(yaw_n), offs.data_ptr(), float(yaw_max), yaw.data_ptr(), power.data_ptr(),
                                       order.data_ptr() if return_order else None, self._stream()), "wg_steady_optimize")
        return (yaw, power, order) if return_order else (yaw, power)

    def optimal_yaws(self, model="m0", refine_pass_n=8, yaw_n=9, yaw_max=30.0):
        """Serial-Refine optimal yaws [B, N] (float64 degrees, CUDA) for the CURRENT wind of every env of this handle: the winds
        are read on the device (info "wind_f64"), no host copy, one launch (``steady_optimize``)."""
        w = self.info("wind_f64")
        return self.steady_optimize(w[:, 0], w[:, 1], w[:, 2], model=model, refine_pass_n=refine_pass_n, yaw_n=yaw_n,
                                    yaw_max=yaw_max)[0]

    def added_lookups(self):
        """Rotor points per flow launch at which the wake-added turbulence box was looked up (window of the last
        kernel_timing call)."""
        v = C.c_double()
        _chk(self.L.wg_added_lookups(self._h, C.byref(v)), "wg_added_lookups")
        return v.value

    def algorithmic_bytes(self):
        v = C.c_double()
        _chk(self.L.wg_algorithmic_bytes(self._h, C.byref(v)), "wg_algorithmic_bytes")
        return v.value

    def flow_variant(self):
        """(threads per k_flow workgroup, compact rings / pair-major phases?, farm slots per wave: 0 = one (k_flow),
        2 = every slot of an env or of one of its contexts (k_flow_env / k_flow_envb: one or two waves per env))"""
        b, r, d = C.c_int(), C.c_int(), C.c_int()
        _chk(self.L.wg_flow_variant(self._h, C.byref(b), C.byref(r), C.byref(d)), "wg_flow_variant")
        return b.value, bool(r.value), d.value


class Curriculum(Handle):
    """The ``wg_curriculum`` handle of one :class:`HipBatch`: the per-env state of the yaw-curriculum reward shaping and its one
    kernel, k_curriculum (include/windgym_hip.h states the recurrence; ``windgym_amd.curriculum.YawCurriculum`` is the user-facing
    class).  ``set_targets`` and ``shape`` enqueue on torch's current stream and synchronise nothing."""

    HEADER_BYTES = 16        # the state blob: (magic, B, N, reserved) int32, then yprev f64[B, N], the targets g f64[B, N], ...
    destroy = "wg_curriculum_destroy"

    def __init__(self, batch: HipBatch):
        self.batch, self.L, self.torch = batch, batch.L, batch.torch
        self.B, self.N = batch.B, batch.N
        h = C.c_void_p()
        _chk(self.L.wg_curriculum_create(batch._h, C.byref(h)), "wg_curriculum_create")
        self._h = h

    def state(self) -> bytes:
        """The state blob (synchronises).  ``ValueError`` once, naming ``ep_row_dev``, when an earlier :meth:`shape` met an
        ``ep_row`` entry that was no row of ``ep_target`` (the kernel skipped it)."""
        return self._blob("wg_curriculum_get_state")

    def load_state(self, blob: bytes):
        _chk(self.L.wg_curriculum_set_state(self._h, blob, len(blob)), "wg_curriculum_set_state")

    def targets_of(self, blob: bytes):
        """The running targets ``[B, N]`` (float64 numpy) a state blob of this geometry holds."""
        n = self.B * self.N
        return np.frombuffer(blob, dtype=np.float64, count=n, offset=self.HEADER_BYTES + 8 * n).reshape(self.B, self.N).copy()

    def set_targets(self, yaw):
        """wg_curriculum_set_targets: ``yaw`` float64 CUDA ``[B, N]``."""
        ptr = tensor_ptr(yaw, self.torch.float64, f"set_targets(): yaw must be a contiguous float64 CUDA tensor [{self.B}, {self.N}]",
                         shape=(self.B, self.N))
        _chk(self.L.wg_curriculum_set_targets(self._h, ptr, self.batch._stream()), "wg_curriculum_set_targets")

    def shape(self, T, yaw0, actions, yaw_after, truncated, ep_row, ep_target, n_targets, weight, momentum, reward, shaped,
              yaw_diff=None, yaw_out=None):
        """wg_curriculum_shape on contiguous CUDA tensors (``None`` = NULL); their sizes are checked here, their values by the
        library."""
        t, B, N, T = self.torch, self.B, self.N, int(T)
        ptrs = []
        for name, x, dtype, numel in (("yaw0", yaw0, t.float32, B * N), ("actions", actions, t.float32, T * B * N),
                                      ("yaw_after", yaw_after, t.float32, T * B * N), ("truncated", truncated, t.uint8, T * B),
                                      ("ep_row", ep_row, t.int32, T * B), ("ep_target", ep_target, t.float64, int(n_targets) * N),
                                      ("weight", weight, t.float64, T), ("reward", reward, t.float32, T * B),
                                      ("shaped", shaped, t.float32, T * B), ("yaw_diff", yaw_diff, t.float32, T * B),
                                      ("yaw_out", yaw_out, t.float32, T * B * N)):
            ptrs.append(None if x is None else tensor_ptr(
                x, dtype, f"shape(): {name} must be a contiguous {dtype} CUDA tensor of at least {numel} elements", at_least=max(numel, 0)))
        _chk(self.L.wg_curriculum_shape(self._h, T, *ptrs[:6], int(n_targets), ptrs[6], float(momentum), *ptrs[7:], self.batch._stream()),
             "wg_curriculum_shape")


class ExpertLabels:
    """wg_expert_labels on one :class:`HipBatch`: the expert's action for every step of a rollout, from the yaws the rollout
    recorded and the Serial-Refine targets of its episodes (include/windgym_hip.h states the rule;
    ``windgym_amd.imitation.BehaviorCloning`` is the user-facing class).  It owns the latch of a bad ``ep_row`` entry; the running
    target table is the caller's.  ``labels`` enqueues on torch's current stream and synchronises nothing; ``check`` synchronises."""

    def __init__(self, batch: HipBatch):
        self.batch, self.L, self.torch = batch, batch.L, batch.torch
        self.B, self.N = batch.B, batch.N
        self._err = self.torch.zeros(4, dtype=self.torch.int32, device=batch.device)

    def labels(self, T, yaw0, yaw_after, truncated, ep_row, ep_target, n_targets, targets, labels, yaw_diff=None):
        """``targets`` float64 ``[B, N]`` is read and updated in place; ``labels`` float32 ``[T, B, N]`` and ``yaw_diff [T, B]``
        (``None`` = NULL) are written.  Sizes are checked here, values by the library."""
        t, B, N, T = self.torch, self.B, self.N, int(T)
        ptrs = []
        for name, x, dtype, numel in (("yaw0", yaw0, t.float32, B * N), ("yaw_after", yaw_after, t.float32, T * B * N),
                                      ("truncated", truncated, t.uint8, T * B), ("ep_row", ep_row, t.int32, T * B),
                                      ("ep_target", ep_target, t.float64, int(n_targets) * N), ("targets", targets, t.float64, B * N),
                                      ("labels", labels, t.float32, T * B * N), ("yaw_diff", yaw_diff, t.float32, T * B)):
            ptrs.append(None if x is None else tensor_ptr(
                x, dtype, f"labels(): {name} must be a contiguous {dtype} CUDA tensor of at least {numel} elements", at_least=max(numel, 0)))
        _chk(self.L.wg_expert_labels(self.batch._h, T, *ptrs[:5], int(n_targets), *ptrs[5:], self._err.data_ptr(), self.batch._stream()),
             "wg_expert_labels")
        return labels

    def check(self):
        """``ValueError`` once, naming ``ep_row_dev``, when an earlier :meth:`labels` met an ``ep_row`` entry that was no row of
        ``ep_target`` (the kernel skipped it).  Synchronises."""
        _chk(self.L.wg_expert_labels_check(self.batch._h, self._err.data_ptr()), "wg_expert_labels_check")


class YawTableHandle(Handle):
    """A ``wg_yaw_table`` handle: the axes and the yaws ``[C, N]`` of a yaw table on one device and its lookup kernels
    (include/windgym_hip.h states the node rule; ``windgym_amd.yaw_table.YawTable`` is the user-facing class).  ``rows``, ``targets``
    and ``act`` enqueue on torch's current stream and synchronise nothing."""

    destroy = "wg_yaw_table_destroy"

    def __init__(self, torch, device, ti, ws, wd, wrap_wd, yaw):
        self.torch, self.L, self.device = torch, load_library(), device
        ax = [np.ascontiguousarray(a, dtype=np.float64) for a in (ti, ws, wd)]
        if not (device_tensor(yaw, torch.float64) and yaw.dim() == 2):
            raise ValueError("yaw must be a contiguous float64 CUDA tensor [C, N]")
        self.N = int(yaw.shape[1])
        args = [x for a in ax for x in (a.ctypes.data_as(C.c_void_p), len(a))]
        h = C.c_void_p()
        _chk(self.L.wg_yaw_table_create(device.index, *args, int(bool(wrap_wd)), self.N, yaw.data_ptr(), 1, C.byref(h)), "wg_yaw_table_create")
        self._h = h

    def _wind(self, who, wind):
        if not (device_tensor(wind, self.torch.float64) and wind.dim() >= 1 and wind.shape[-1] == 3):
            raise ValueError(f"{who}: wind must be a contiguous float64 CUDA tensor [..., 3] (ws, wd, ti)")
        return wind.numel() // 3

    def rows(self, wind, mask=None, out=None):
        """wg_yaw_table_rows: ``wind [..., 3]`` float64, ``mask [...]`` uint8 or ``None`` -> int32 ``[...]``."""
        t = self.torch
        n = self._wind("rows()", wind)
        mp = None if mask is None else tensor_ptr(mask, t.uint8, f"rows(): mask must be a contiguous uint8 CUDA tensor of {n} elements", numel=n)
        if out is None:
            out = t.empty(tuple(wind.shape[:-1]), dtype=t.int32, device=wind.device)
        op = tensor_ptr(out, t.int32, f"rows(): out must be a contiguous int32 CUDA tensor of {n} elements", numel=n)
        _chk(self.L.wg_yaw_table_rows(self._h, n, wind.data_ptr(), mp, op, self._stream()), "wg_yaw_table_rows")
        return out

    def targets(self, wind, out=None):
        """wg_yaw_table_targets: ``wind [..., 3]`` float64 -> float64 ``[..., N]``; a row of ``out`` whose wind has no row stays."""
        t = self.torch
        n = self._wind("targets()", wind)
        if out is None:
            out = t.zeros(tuple(wind.shape[:-1]) + (self.N,), dtype=t.float64, device=wind.device)
        op = tensor_ptr(out, t.float64, f"targets(): out must be a contiguous float64 CUDA tensor of {n * self.N} elements", numel=n * self.N)
        _chk(self.L.wg_yaw_table_targets(self._h, n, wind.data_ptr(), op, self._stream()), "wg_yaw_table_targets")
        return out

    def act(self, batch, out):
        """wg_yaw_table_act on ``batch`` (a :class:`HipBatch`): ``out`` float32 ``[B, N]``."""
        op = tensor_ptr(out, self.torch.float32, f"act(): out must be a contiguous float32 CUDA tensor [{batch.B}, {batch.N}]",
                        numel=batch.B * batch.N)
        _chk(self.L.wg_yaw_table_act(batch._h, self._h, op, batch._stream()), "wg_yaw_table_act")
        return out


class Norm(Handle):
    """A ``wg_norm`` handle: SB3's VecNormalize statistics on the device (include/windgym_hip.h restates the rules;
    ``windgym_amd.normalize.VecNormalize`` is the user-facing class).  ``obs``, ``reward`` and ``reset_returns`` enqueue on torch's
    current stream and synchronise nothing; ``state`` / ``load_state`` synchronise."""

    HEADER_BYTES = 16        # the state blob: (magic, O, B, 0) int32, then float64 obs mean [O], var [O], count, ret mean, var, count, returns [B]
    destroy = "wg_norm_destroy"

    def __init__(self, n_obs, n_envs, device, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99,
                 epsilon=1e-8):
        import torch
        self.torch, self.L = torch, load_library()
        self.O, self.B = int(n_obs), int(n_envs)
        self.device = torch.device("cuda", int(device))
        d = CNormDesc(self.O, self.B, int(bool(norm_obs)), int(bool(norm_reward)), float(clip_obs), float(clip_reward), float(gamma),
                      float(epsilon))
        h = C.c_void_p()
        _chk(self.L.wg_norm_create(C.byref(d), int(device), C.byref(h)), "wg_norm_create")
        self._h = h

    def state(self) -> bytes:
        return self._blob("wg_norm_get_state")

    def load_state(self, blob: bytes):
        _chk(self.L.wg_norm_set_state(self._h, blob, len(blob)), "wg_norm_set_state")

    def stats(self):
        """The state blob's float64 payload as a dict of numpy arrays: ``obs_mean`` / ``obs_var`` ``[O]``, ``obs_count``,
        ``ret_mean``, ``ret_var``, ``ret_count`` and ``returns`` ``[B]`` (synchronises)."""
        return unpack_norm_state(self.state(), self.O, self.B)

    def set_training(self, training):
        _chk(self.L.wg_norm_set_training(self._h, int(bool(training))), "wg_norm_set_training")

    def reset_returns(self, mask=None):
        mp = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint8).reshape(self.B))
            mp = m.ctypes.data_as(C.c_void_p)
        _chk(self.L.wg_norm_reset_returns(self._h, mp, self._stream()), "wg_norm_reset_returns")

    def _rows(self, name, x, dtype, numel=None):
        return tensor_ptr(x, dtype, f"{name} must be a contiguous {dtype} CUDA tensor on {self.device}"
                          + ("" if numel is None else f" of {numel} elements"), numel=numel, device=self.device)

    def obs(self, obs, out, extra=None, extra_out=None):
        """wg_norm_obs on ``[n_rows, O]`` float32 tensors (``extra`` / ``extra_out``: the final rows, or both ``None``)."""
        t = self.torch
        if obs.numel() % self.O:
            raise ValueError(f"obs must hold rows of {self.O} entries")
        n = obs.numel() // self.O
        ptrs = [self._rows("obs", obs, t.float32), self._rows("out", out, t.float32, n * self.O),
                None if extra is None else self._rows("extra", extra, t.float32, n * self.O),
                None if extra_out is None else self._rows("extra_out", extra_out, t.float32, n * self.O)]
        _chk(self.L.wg_norm_obs(self._h, n, *ptrs, self._stream()), "wg_norm_obs")
        return out

    def reward(self, reward, truncated, out):
        """wg_norm_reward on ``[T, B]`` tensors (``reward`` / ``out`` float32, ``truncated`` uint8); ``out`` may be ``reward``."""
        t = self.torch
        if reward.numel() % self.B:
            raise ValueError(f"reward must be [T, {self.B}]")
        T = reward.numel() // self.B
        ptrs = [self._rows("reward", reward, t.float32), self._rows("truncated", truncated, t.uint8, T * self.B),
                self._rows("out", out, t.float32, T * self.B)]
        _chk(self.L.wg_norm_reward(self._h, T, *ptrs, self._stream()), "wg_norm_reward")
        return out


def unpack_norm_state(blob, n_obs, n_envs):
    """The float64 payload of a ``wg_norm`` state blob of these widths as a dict of numpy arrays (copies)."""
    O, B = int(n_obs), int(n_envs)
    a = np.frombuffer(blob, dtype=np.float64, count=2 * O + 4 + B, offset=Norm.HEADER_BYTES).copy()
    return dict(obs_mean=a[:O], obs_var=a[O:2 * O], obs_count=a[2 * O], ret_mean=a[2 * O + 1], ret_var=a[2 * O + 2],
                ret_count=a[2 * O + 3], returns=a[2 * O + 4:])


def pack_norm_state(n_obs, n_envs, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count, returns):
    """The inverse of :func:`unpack_norm_state`: a blob ``wg_norm_set_state`` accepts."""
    O, B = int(n_obs), int(n_envs)
    a = np.concatenate([np.asarray(obs_mean, np.float64).reshape(-1), np.asarray(obs_var, np.float64).reshape(-1),
                        np.array([obs_count, ret_mean, ret_var, ret_count], np.float64), np.asarray(returns, np.float64).reshape(-1)])
    if a.size != 2 * O + 4 + B:
        raise ValueError(f"statistics of the wrong width: obs_mean / obs_var must hold {O} entries and returns {B}")
    return np.array([0x4d524e57, O, B, 0], np.uint32).tobytes() + a.tobytes()
