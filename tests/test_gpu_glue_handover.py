"""k_flow_env without a pass wave hands the step's own values to its glue tail in registers (newest ring samples, yaw before /
after, powers: LeanFused::regs) and no longer waits for the flow part's stores before the glue's remaining loads — except on a
truncating step, where the swap reads what the launch stored.  Nothing a caller can see may change: the one-launch step against
the two-launch step (flow launch + k_glue_lean, WG_STEP_FUSED=0, whose glue reads everything back from memory) on the same handle
configuration, seeds and actions, BIT for bit — observation, reward, truncation flag, final observation, the per-agent buffer
where there is one, every step, and the whole state blob at the end.

6 envs, both waves-per-env settings without a pass wave, episodes of at most ~50 steps: in 150 steps every env truncates at least
twice (asserted), so each run crosses truncating steps (barrier kept, swap), the deferred episode set-up, the first-observation
launch of a completed background episode and the clone of a parked baseline farm — the paths that keep their own barriers —
between stretches of ordinary steps, the path that lost its barrier."""
import numpy as np
import pytest

from helpers import hip, make_batch  # noqa: F401  (hip: the fixture)
from variant_census import AllChannelNoiseConfig, _yaml

pytestmark = pytest.mark.gpu

B, STEPS = 6, 150
WPE_HOOKS = {"wpe1": {"WG_ENV_WPE": "1"}, "wpe2": {"WG_ENV_WPE": "2", "WG_ENV_SPLIT": "0"}}


def _cfg(case):
    """-> (EnvConfig, per-agent buffer).  Episode lengths are time_max + 1 = int(n_passthrough * dist / ws) + 1 steps, dist the
    farm's extent along the wind (at most its diagonal), ws >= 7 m/s."""
    from windgym_amd import presets
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    common = dict(turbine=V80(), turbtype="None", n_envs=B, autoreset=True, n_rotor_pts=16)
    if case == "cfg2_4x4":                 # two farms of 16 turbines: the wave is full; <= 45 steps (diagonal 1570 m)
        return EnvConfig(yaml_dict=presets.bench_cfg2_config(), n_passthrough=0.2, n_particles=128, **common), False
    if case == "multi_3x3":                # glue 2: the per-agent buffer of the PettingZoo facade; <= 49 steps (1357 m)
        return EnvConfig(yaml_dict=presets.multi_3x3_config(), n_passthrough=0.25, n_particles=96, **common), True
    if case == "two_turb_one_farm":        # F = 1 (no baseline farm), N = 2; <= 37 steps (640 m)
        d = presets._upd(presets.env1_config(), ActionMethod="yaw", farm=dict(nx=2, ny=1), power_def=dict(Power_reward="Power_avg"))
        return EnvConfig(yaml_dict=d, n_passthrough=0.4, **common), False
    if case == "substeps3":                # K = 3 flow sub-steps per env step: the pushed samples are averages; <= 47 steps (1090 m)
        return EnvConfig(yaml_dict=_yaml(False, 3, 2), n_passthrough=0.3, dt_env=3, dt_sim=1, **common), False
    if case == "noise4":                   # sensor noise on ws, wd, yaw and power, all four observed; <= 39 steps
        return AllChannelNoiseConfig(yaml_dict=_yaml(True, 3, 2, False, True), n_passthrough=0.25, **common), False
    raise KeyError(case)


def _actions(cfg):
    import torch
    g = torch.Generator(device="cpu").manual_seed(23)
    return torch.rand((STEPS, B, cfg.n_turb), generator=g) * 2 - 1


def _run(hip, case, wpe, fused, acts=None):
    """150 steps of one handle -> per step (obs, reward, truncated, final_obs[, per-agent buffer]) as numpy arrays, state blob"""
    cfg, multi = _cfg(case)
    hooks = {"WG_FLOW_ENV": "1", "WG_STEP_FUSED": "1" if fused else "0", **WPE_HOOKS[wpe]}
    env = make_batch(hip, cfg, hooks, variant=(None, None, 2), multi=multi)      # an env kernel, not the per-slot one
    acts = (_actions(cfg) if acts is None else acts).cuda()
    out = [[env.reset(seeds=3100 + np.arange(B)).cpu().numpy().copy()]]
    for s in range(STEPS):
        r = [x.cpu().numpy().copy() for x in env.step(acts[s])]
        if multi:
            r.append(env._multi_buf.cpu().numpy().copy())
        out.append(r)
    env.check()
    blob = np.frombuffer(env.get_state(), np.uint8).copy()
    env.close()
    return out, blob


_TWO_LAUNCH = {}


def _two_launch(hip, case, wpe):
    """the two-launch trajectory of a case: computed once, shared (the control reads it too), never modified"""
    if (case, wpe) not in _TWO_LAUNCH:
        _TWO_LAUNCH[case, wpe] = _run(hip, case, wpe, fused=False)
    return _TWO_LAUNCH[case, wpe]


WHAT = ("obs", "reward", "truncated", "final_obs", "per-agent buffer")


@pytest.mark.parametrize("wpe", list(WPE_HOOKS))
@pytest.mark.parametrize("case", ["cfg2_4x4", "multi_3x3", "two_turb_one_farm", "substeps3", "noise4"])
def test_one_launch_step_equals_two_launches_bit_for_bit(hip, case, wpe):
    ref, ref_blob = _two_launch(hip, case, wpe)
    got, got_blob = _run(hip, case, wpe, fused=True)
    n_tr = np.zeros(B, int)
    assert np.array_equal(got[0][0], ref[0][0]), "reset obs"
    for s in range(1, STEPS + 1):
        for x, y, what in zip(got[s], ref[s], WHAT):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what} differs at step {s - 1}"
        n_tr += ref[s][2].astype(bool)
    print(f"{case} {wpe}: truncations per env {n_tr.tolist()}")
    assert (n_tr >= 2).all(), n_tr                  # every env crossed two truncating steps (and what follows them)
    assert np.array_equal(got_blob, ref_blob), "state blobs differ"


def test_control_one_changed_action_shows_in_its_env_only(hip):
    """The comparison can fail, and envs do not leak into each other: the one-launch run with ONE action of ONE env changed at ONE
    step differs from the unchanged two-launch run in that env — from that step on, not before — and in no other env."""
    case, wpe, e0, s0 = "cfg2_4x4", "wpe1", 3, 60
    cfg, _ = _cfg(case)
    acts = _actions(cfg)
    acts[s0, e0, 5] = -acts[s0, e0, 5] + (0.5 if abs(float(acts[s0, e0, 5])) < 0.05 else 0.0)
    ref, _ = _two_launch(hip, case, wpe)
    got, _ = _run(hip, case, wpe, fused=True, acts=acts)
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
