"""k_flow_env reads the words of its common STEP path — the prologue's pointers and shape, the LDS set-up's constants, the glue's
early request, the per-turbine tail's ring words, the farm-level pushes — out of a hot parameter block (EnvHotP, wg_flow.h) that
env_launch builds from the blocks it passes, one wide scalar trip per phase; the rare paths (episode set-up, clone, first
observation, swap, the truncating step) keep reading the big blocks word by word.  Nothing a caller can see may change.  Method of
tests/test_gpu_glue_early_loads.py: the one-launch step against the two-launch step (flow launch + k_glue_lean, WG_STEP_FUSED=0,
whose glue reads its parameters from the handle's device copies and everything else back from memory) on the same configuration,
seeds and actions, BIT for bit — observation, reward, truncation flag, final observation, the per-agent buffer where there is one,
every step, and the whole state blob at the end.  6 envs, 150 steps; every env is asserted to truncate at least twice, so set-up,
clone, first observation and swap run beside the new reads.

Cases — each word group of the block takes values the cfg2 preset does not give it:
  * window1_local_yaw / window2_global_wind: windows of 1 and 2 samples (ring_cap 2 / 3: the request's and the tail's ring words),
    the baseline farm under the local / the global controller, the action as a yaw step / as a wind-relative set point;
  * deque1: Power_avg 1 under the Baseline reward; power_diff: Power_diff at Power_avg 40 (power_avg, pavg_magic);
  * substeps3: K = 3 flow rounds per launch (the tail's and the farm group's copies are taken every round);
  * noise4: sensor noise on all four channels (the NOISE instantiations read noise_sigma and the env's noise key from the tail group);
  * multi_extra_inc: the 3 x 3 multi-agent preset with extra_timestep_inc (env_inc 2, glue 2, N = 9: slots are not DPP rows);
  * two_turb_one_farm: F = 1, N = 2.
Hooks: one and two waves per env and the two pass-wave settings (a pass wave for the running context / for both) on every case —
the pass wave takes the prologue's and the request's group at the head of the launch (K = 3: the plan runs such a step unsplit).  The two-launch trajectory of a case is computed
once per waves-per-env setting and shared (a pass-wave run is compared with the two-launch run of two waves per env: without a glue
tail there is no pass wave, and the kernels are interchangeable launch by launch, tests/test_gpu_variant_ab.py).

Handle reuse after a parameter-changing call: no wg_set_* call writes a word the block copies (the box and script setters write
FlowP / WgParams words of the turbulent and replay paths, which k_flow_env does not serve); wg_set_wind is the nearest — it changes
a member of WgPtrs, one of the four blocks every launch rebuilds the hot block from — so `reuse_set_wind` fixes the wind of half
the envs after 60 steps and goes on stepping the same handle, on both sides.

One control: a single changed action shows in its env from its step on and nowhere else — the comparison can fail."""
import numpy as np
import pytest

from helpers import hip, make_batch  # noqa: F401  (hip: the fixture)
from variant_census import AllChannelNoiseConfig, _yaml

pytestmark = pytest.mark.gpu

B, STEPS, SET_WIND_AT = 6, 150, 60
HOOKS = {"wpe1": {"WG_ENV_WPE": "1"}, "wpe2": {"WG_ENV_WPE": "2", "WG_ENV_SPLIT": "0"},
         "pass1": {"WG_ENV_WPE": "2", "WG_ENV_SPLIT": "1"}, "pass2": {"WG_ENV_WPE": "2", "WG_ENV_SPLIT": "2"}}
CASES = ["window1_local_yaw", "window2_global_wind", "deque1", "power_diff", "substeps3", "noise4", "multi_extra_inc", "two_turb_one_farm"]
RUNS = [(c, h) for c in CASES for h in HOOKS]
RUNS += [("reuse_set_wind", "wpe1")]


def _cfg(case):
    """-> (EnvConfig, per-agent buffer).  Episodes of time_max + 1 = int(n_passthrough * dist / ws) + 1 timesteps, dist the farm's
    extent along the wind (at most its diagonal), ws >= 7 m/s: at most ~50 env steps each."""
    from windgym_amd import presets
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    common = dict(turbine=V80(), turbtype="None", n_envs=B, autoreset=True, n_rotor_pts=16)
    cfg2 = presets.bench_cfg2_config()         # 4 x 4, two farms: the wave is full; <= 45 steps (diagonal 1570 m)
    if case in ("window1_local_yaw", "window2_global_wind", "reuse_set_wind"):
        w, ctrl, act = (2, "Global", "wind") if case == "window2_global_wind" else (1, "Local", "yaw")
        d = presets._upd(cfg2, ws_mes=dict(ws_history_length=w, ws_window_length=w), yaw_mes=dict(yaw_history_length=w, yaw_window_length=w),
                         BaseController=ctrl, ActionMethod=act)
        return EnvConfig(yaml_dict=d, n_passthrough=0.2, n_particles=128, **common), False
    if case == "deque1":
        d = presets._upd(cfg2, power_def=dict(Power_reward="Baseline", Power_avg=1))
        return EnvConfig(yaml_dict=d, n_passthrough=0.2, n_particles=128, **common), False
    if case == "power_diff":
        d = presets._upd(cfg2, power_def=dict(Power_reward="Power_diff", Power_avg=40))
        return EnvConfig(yaml_dict=d, n_passthrough=0.2, n_particles=128, **common), False
    if case == "substeps3":                    # K = 3; <= 47 steps (1090 m)
        return EnvConfig(yaml_dict=_yaml(False, 3, 2), n_passthrough=0.3, dt_env=3, dt_sim=1, **common), False
    if case == "noise4":                       # <= 39 steps
        return AllChannelNoiseConfig(yaml_dict=_yaml(True, 3, 2, False, True), n_passthrough=0.25, **common), False
    if case == "multi_extra_inc":              # the timestep advances by 2 per env step: <= 25 steps (1357 m)
        return EnvConfig(yaml_dict=presets.multi_3x3_config(), n_passthrough=0.25, n_particles=96, extra_timestep_inc=True, **common), True
    if case == "two_turb_one_farm":            # <= 37 steps (640 m)
        d = presets._upd(presets.env1_config(), ActionMethod="yaw", farm=dict(nx=2, ny=1), power_def=dict(Power_reward="Power_avg"))
        return EnvConfig(yaml_dict=d, n_passthrough=0.4, **common), False
    raise KeyError(case)


def _actions(cfg):
    import torch
    g = torch.Generator(device="cpu").manual_seed(36)
    return torch.rand((STEPS, B, cfg.n_turb), generator=g) * 2 - 1


def _run(hip, case, hooks, fused, acts=None):
    """150 steps of one handle -> per step (obs, reward, truncated, final_obs[, per-agent buffer]) as numpy arrays, state blob"""
    cfg, multi = _cfg(case)
    hk = {"WG_FLOW_ENV": "1", "WG_STEP_FUSED": "1" if fused else "0", **HOOKS[hooks]}
    env = make_batch(hip, cfg, hk, variant=(None, None, 2), multi=multi)      # an env kernel, not the per-slot one
    acts = (_actions(cfg) if acts is None else acts).cuda()
    out = [[env.reset(seeds=3600 + np.arange(B)).cpu().numpy().copy()]]
    for s in range(STEPS):
        if case == "reuse_set_wind" and s == SET_WIND_AT:      # (takes effect at each env's next episode set-up)
            env.set_wind(ws=np.where(np.arange(B) % 2 == 0, 9.0, np.nan), wd=np.where(np.arange(B) % 2 == 0, 262.0, np.nan))
        r = [x.cpu().numpy().copy() for x in env.step(acts[s])]
        if multi:
            r.append(env._multi_buf.cpu().numpy().copy())
        out.append(r)
    env.check()
    blob = np.frombuffer(env.get_state(), np.uint8).copy()
    env.close()
    return out, blob


_TWO_LAUNCH = {}


def _two_launch(hip, case, hooks="wpe1"):
    """the two-launch trajectory of a case, with one or with two waves per env (the state blob holds the background plan's
    words, which the two settings keep differently; a pass-wave setting is compared with the two-wave one): computed once,
    shared, never modified"""
    wpe = "wpe1" if hooks == "wpe1" else "wpe2"
    if (case, wpe) not in _TWO_LAUNCH:
        _TWO_LAUNCH[case, wpe] = _run(hip, case, wpe, fused=False)
    return _TWO_LAUNCH[case, wpe]


WHAT = ("obs", "reward", "truncated", "final_obs", "per-agent buffer")


@pytest.mark.parametrize("case, hooks", RUNS)
def test_hot_block_step_equals_two_launches_bit_for_bit(hip, case, hooks):
    ref, ref_blob = _two_launch(hip, case, hooks)
    got, got_blob = _run(hip, case, hooks, fused=True)
    n_tr = np.zeros(B, int)
    assert np.array_equal(got[0][0], ref[0][0]), "reset obs"
    for s in range(1, STEPS + 1):
        assert len(got[s]) == len(ref[s])
        for x, y, what in zip(got[s], ref[s], WHAT):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what} differs at step {s - 1}"
        n_tr += ref[s][2].astype(bool)
    print(f"{case} {hooks}: truncations per env {n_tr.tolist()}")
    assert (n_tr >= 2).all(), n_tr                  # every env crossed two truncating steps (and what follows them)
    assert np.array_equal(got_blob, ref_blob), "state blobs differ"


def test_set_wind_changed_the_reused_handle(hip):
    """the parameter-changing call of `reuse_set_wind` is not a no-op: from some step after it the trajectory leaves that of the
    same configuration without the call (window1_local_yaw), in an env whose wind was fixed"""
    a, _ = _two_launch(hip, "reuse_set_wind")
    b, _ = _two_launch(hip, "window1_local_yaw")
    first = next((s for s in range(1, STEPS + 1) if not np.array_equal(a[s][0], b[s][0])), None)
    assert first is not None and first - 1 >= SET_WIND_AT, first
    assert all(np.array_equal(a[s][0][1::2], b[s][0][1::2]) for s in range(1, STEPS + 1)), "an env whose wind was left alone changed"


def test_control_one_changed_action_shows_in_its_env_only(hip):
    """The comparison can fail, and envs do not leak into each other: the one-launch run with ONE action of ONE env changed at ONE
    step differs from the unchanged two-launch run in that env — from that step on, not before — and in no other env."""
    case, hooks, e0, s0 = "window1_local_yaw", "wpe1", 2, 70
    cfg, _ = _cfg(case)
    acts = _actions(cfg)
    acts[s0, e0, 5] = -acts[s0, e0, 5] + (0.5 if abs(float(acts[s0, e0, 5])) < 0.05 else 0.0)
    ref, _ = _two_launch(hip, case)
    got, _ = _run(hip, case, hooks, fused=True, acts=acts)
    others = np.arange(B) != e0
    differs = False
    for s in range(1, STEPS + 1):
        for x, y, what in zip(got[s], ref[s], WHAT):
            assert np.array_equal(x[others].view(np.uint8), y[others].view(np.uint8)), f"{what} of an untouched env differs at step {s - 1}"
            same = np.array_equal(x[e0:e0 + 1].view(np.uint8), y[e0:e0 + 1].view(np.uint8))
            if s - 1 < s0:
                assert same, f"{what} of env {e0} differs at step {s - 1}, before the change"
            differs |= not same
    assert differs, "the changed action left no trace"
