"""k_flow_env without a pass wave requests its glue's step-independent inputs — the old window sums and the leaving ring samples
of the glue lane's turbine, the oldest power-deque entries, the metrics — at the head of its per-turbine tail and hands them to
the glue by value (LeanFused::early): the loads now sit IN FRONT of the tail's ring / farm-ring pushes, the epilogue's state
stores and the stores of the rare paths behind it.  Nothing a caller can see may change.  Same method as
tests/test_gpu_glue_handover.py — the one-launch step against the two-launch step (flow launch + k_glue_lean, WG_STEP_FUSED=0,
whose glue loads everything after the flow launch has ended) on the same configuration, seeds and actions, BIT for bit:
observation, reward, truncation flag, final observation, the per-agent buffer where there is one, every step, and the whole
state blob at the end — at the shapes where moving a load ahead of a store could show:

  * tight windows: window == history == 1 and 2 for the ws / yaw rolling means — the ring has 2 or 3 rows, the leaving row is
    the pushed row's neighbour and the ring wraps every step;
  * the shortest power deques, Power_avg 1 and 2 under the Baseline reward: the oldest entry is the slot the glue overwrites in
    the same step;
  * the Power_diff reward (the glue still loads the whole deque itself) at Power_avg 40, the smallest value the configuration
    check accepts for it;
  * several flow rounds per launch (the request repeats): K = 3 on 3 x 2, and the 3 x 3 multi-agent preset with
    extra_timestep_inc — episodes half as long in env steps, background slots take two flow steps in a launch, glue 2;
  * F = 1, N = 2: no baseline deque.

6 envs, 150 steps, both waves-per-env settings without a pass wave; every env is asserted to truncate at least twice.  One
control: a single changed action shows in its env from its step on and nowhere else — the comparison can fail."""
import numpy as np
import pytest

from helpers import hip, make_batch  # noqa: F401  (hip: the fixture)
from variant_census import _yaml

pytestmark = pytest.mark.gpu

B, STEPS = 6, 150
WPE_HOOKS = {"wpe1": {"WG_ENV_WPE": "1"}, "wpe2": {"WG_ENV_WPE": "2", "WG_ENV_SPLIT": "0"}}
CASES = ["window1", "window2", "deque1", "deque2", "power_diff", "substeps3", "multi_extra_inc", "two_turb_one_farm"]


def _cfg(case):
    """-> (EnvConfig, per-agent buffer).  Episodes of time_max + 1 = int(n_passthrough * dist / ws) + 1 timesteps, dist the farm's
    extent along the wind (at most its diagonal), ws >= 7 m/s: at most ~50 env steps each."""
    from windgym_amd import presets
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    common = dict(turbine=V80(), turbtype="None", n_envs=B, autoreset=True, n_rotor_pts=16)
    cfg2 = presets.bench_cfg2_config()         # 4 x 4, two farms: the wave is full; <= 45 steps (diagonal 1570 m)
    if case in ("window1", "window2"):
        w = int(case[-1])
        d = presets._upd(cfg2, ws_mes=dict(ws_history_length=w, ws_window_length=w), yaw_mes=dict(yaw_history_length=w, yaw_window_length=w))
        return EnvConfig(yaml_dict=d, n_passthrough=0.2, n_particles=128, **common), False
    if case in ("deque1", "deque2"):
        d = presets._upd(cfg2, power_def=dict(Power_reward="Baseline", Power_avg=int(case[-1])))
        return EnvConfig(yaml_dict=d, n_passthrough=0.2, n_particles=128, **common), False
    if case == "power_diff":
        d = presets._upd(cfg2, power_def=dict(Power_reward="Power_diff", Power_avg=40))
        return EnvConfig(yaml_dict=d, n_passthrough=0.2, n_particles=128, **common), False
    if case == "substeps3":                    # K = 3 flow rounds per launch; <= 47 steps (1090 m)
        return EnvConfig(yaml_dict=_yaml(False, 3, 2), n_passthrough=0.3, dt_env=3, dt_sim=1, **common), False
    if case == "multi_extra_inc":              # glue 2; the timestep advances by 2 per env step: <= 25 steps (1357 m), so the
        # background episode's development and fill (25 samples) are spread over fewer env steps than they have flow steps
        return EnvConfig(yaml_dict=presets.multi_3x3_config(), n_passthrough=0.25, n_particles=96, extra_timestep_inc=True, **common), True
    if case == "two_turb_one_farm":            # F = 1 (no baseline farm, no base_pow), N = 2; <= 37 steps (640 m)
        d = presets._upd(presets.env1_config(), ActionMethod="yaw", farm=dict(nx=2, ny=1), power_def=dict(Power_reward="Power_avg"))
        return EnvConfig(yaml_dict=d, n_passthrough=0.4, **common), False
    raise KeyError(case)


def _actions(cfg):
    import torch
    g = torch.Generator(device="cpu").manual_seed(29)
    return torch.rand((STEPS, B, cfg.n_turb), generator=g) * 2 - 1


def _run(hip, case, wpe, fused, acts=None):
    """150 steps of one handle -> per step (obs, reward, truncated, final_obs[, per-agent buffer]) as numpy arrays, state blob"""
    cfg, multi = _cfg(case)
    hooks = {"WG_FLOW_ENV": "1", "WG_STEP_FUSED": "1" if fused else "0", **WPE_HOOKS[wpe]}
    env = make_batch(hip, cfg, hooks, variant=(None, None, 2), multi=multi)      # an env kernel, not the per-slot one
    acts = (_actions(cfg) if acts is None else acts).cuda()
    out = [[env.reset(seeds=4100 + np.arange(B)).cpu().numpy().copy()]]
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
@pytest.mark.parametrize("case", CASES)
def test_early_loads_equal_two_launches_bit_for_bit(hip, case, wpe):
    ref, ref_blob = _two_launch(hip, case, wpe)
    got, got_blob = _run(hip, case, wpe, fused=True)
    n_tr = np.zeros(B, int)
    assert np.array_equal(got[0][0], ref[0][0]), "reset obs"
    for s in range(1, STEPS + 1):
        assert len(got[s]) == len(ref[s])
        for x, y, what in zip(got[s], ref[s], WHAT):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what} differs at step {s - 1}"
        n_tr += ref[s][2].astype(bool)
    print(f"{case} {wpe}: truncations per env {n_tr.tolist()}")
    assert (n_tr >= 2).all(), n_tr                  # every env crossed two truncating steps (and what follows them)
    assert np.array_equal(got_blob, ref_blob), "state blobs differ"


def test_control_one_changed_action_shows_in_its_env_only(hip):
    """The comparison can fail, and envs do not leak into each other: the one-launch run with ONE action of ONE env changed at ONE
    step differs from the unchanged two-launch run in that env — from that step on, not before — and in no other env.  On the
    tightest window: the changed yaw is in the observation's rolling mean at once."""
    case, wpe, e0, s0 = "window1", "wpe1", 2, 70
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
