"""The value rules of windgym_amd/csrc/wg_rules.h (plain C++, the functions every step path calls), decided on the CPU: each rule
against a numpy restatement of the reference's own lines, at its edges.  tests/rules_shim.cpp hands the header's functions over.
This checks the one statement; the kernels that call it are held to the oracle by test_gpu_rule_cases.py and
test_gpu_sensor_cases.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

from helpers import host_shim

F = np.float32
ACT_YAW, ACT_WIND, PEN_CHANGE, PEN_TOTAL = 0, 1, 0, 1            # include/windgym_hip.h


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = host_shim(tmp_path_factory, "rules")
    lib.rule_adjust_yaw.argtypes = [C.c_int] + [C.c_float] * 5
    lib.rule_ctrl_local.argtypes = [C.c_float] * 3
    lib.rule_ctrl_global.argtypes = [C.c_float] * 2
    lib.rule_penalty.argtypes = [C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double]
    lib.rule_reward.argtypes = [C.c_double] * 3
    lib.rule_metric_add.argtypes = [C.c_int] + [C.c_float] * 3 + [C.c_int, C.c_float, C.c_int, C.c_float]
    lib.rule_episode_steps.argtypes = lib.rule_episode_steps_inc.argtypes = [C.c_int, C.c_int]
    for f in (lib.rule_adjust_yaw, lib.rule_ctrl_local, lib.rule_ctrl_global, lib.rule_reward, lib.rule_metric_add):
        f.restype = C.c_float
    lib.rule_penalty.restype = C.c_double
    lib.rule_episode_steps.restype = lib.rule_episode_steps_inc.restype = C.c_long
    return lib


def bits(x):
    return np.asarray(x, F).view(np.uint32)


def np_adjust_yaws(method, yaw, action, yaw_min, yaw_max, yaw_step):
    """Wind_Farm_Env.py:822-864 on float32 arrays (HTC_path is None)"""
    yaw, action = np.array([yaw], F), np.array([action], F)
    if method == ACT_YAW:
        yaw += action * yaw_step
        yaw = np.clip(yaw, yaw_min, yaw_max)
    else:
        new_yaws = (action + F(1.0)) / F(2.0) * (yaw_max - yaw_min) + yaw_min
        hi = yaw + yaw_step
        lo = yaw - yaw_step
        yaw = np.clip(np.clip(new_yaws, lo, hi), yaw_min, yaw_max)
    assert yaw.dtype == F
    return yaw[0]


@pytest.mark.parametrize("method", [ACT_YAW, ACT_WIND])
@pytest.mark.parametrize("ymin, ymax, ystep", [(-30.0, 30.0, 1.0), (-25.5, 40.25, 2.5), (-45.0, 45.0, 0.3)])
def test_adjust_yaws_bit_for_bit(shim, method, ymin, ymax, ystep):
    ymin, ymax, ystep = F(ymin), F(ymax), F(ystep)
    yaws = [ymin, ymax, ymax - ystep * F(0.5), ymin + ystep * F(0.25), np.nextafter(ymax, F(0)), np.nextafter(ymin, F(0)),
            F(0.0), F(-0.0), F(3.3), F(-17.77)]
    acts = [-1.5, -1.0, 0.0, 1.0, 1.5, 0.3337, -0.71, 1e-8]
    n = 0
    for yaw, a in itertools.product(yaws, acts):
        got = F(shim.rule_adjust_yaw(method, yaw, F(a), ymin, ymax, ystep))
        ref = np_adjust_yaws(method, yaw, F(a), ymin, ymax, ystep)
        assert bits(got) == bits(ref), (method, yaw, a, got, ref)
        assert ymin <= got <= ymax
        n += got != yaw
    assert n > len(yaws)                                         # the cases move the yaw


def np_local(yaw, wdir, yaw_step):
    """BasicControllers.py:10-46 from the local wind direction, float32"""
    yaw_baseline = np.array([yaw], F)
    yaw_offset = np.array([wdir], F) - yaw_baseline
    step_dir = np.sign(yaw_offset)
    step_scale = np.abs(yaw_offset)
    step_scale[step_scale > yaw_step] = yaw_step
    return (yaw_baseline + step_dir * step_scale)[0]


def np_global(yaw, yaw_step):
    """BasicControllers.py:49-73, float32"""
    yaw_offset = np.array([yaw], F)
    step_dir = np.sign(yaw_offset)
    step_scale = np.abs(yaw_offset)
    step_scale[step_scale > yaw_step] = yaw_step
    return (yaw_offset - step_dir * step_scale)[0]


@pytest.mark.parametrize("ystep", [1.0, 0.3, 2.5])
def test_controllers_at_the_step_and_at_zero(shim, ystep):
    """Bit for bit, the sign of a zero included: offsets +0.0 and -0.0, yaws +0.0 and -0.0."""
    ystep = F(ystep)
    offs = [F(0.0), F(-0.0), ystep, -ystep, np.nextafter(ystep, F(0)), np.nextafter(ystep, F(9)), -np.nextafter(ystep, F(0)),
            -np.nextafter(ystep, F(9)), F(0.01), F(-0.01), F(17.3), F(-29.0)]
    for off in offs:
        g, r = F(shim.rule_ctrl_global(off, ystep)), np_global(off, ystep)
        assert bits(g) == bits(r) and abs(g) <= abs(off), (off, g, r)
        assert g == 0 if abs(off) <= ystep else abs(abs(off) - abs(g) - ystep) < 2e-6
        for wdir in (F(0.0), F(-0.0), F(4.25), F(-11.5)):
            yaw = wdir - off
            g, r = F(shim.rule_ctrl_local(yaw, wdir, ystep)), np_local(yaw, wdir, ystep)
            assert bits(g) == bits(r), (yaw, wdir, g, r)
            assert abs(float(g) - float(yaw)) <= float(ystep) + 2e-6          # (half an ulp of a yaw below 32)


@pytest.mark.parametrize("ptype", [PEN_CHANGE, PEN_TOTAL])
@pytest.mark.parametrize("action_penalty", [0.0, 0.0009, 0.001, 0.05])
def test_penalty_on_both_sides_of_the_switch(shim, ptype, action_penalty):
    """Wind_Farm_Env.py:804-820 (yaws in quarter degrees: the float sum of the terms is exact) and the reward's last line (:989-996)"""
    rng = np.random.default_rng(3)
    old = (rng.integers(-120, 121, 7) / 4).astype(F)
    yaw = (rng.integers(-120, 121, 7) / 4).astype(F)
    yaw_max = 30.0
    if action_penalty < 0.001:
        ref = 0
    elif ptype == PEN_CHANGE:
        ref = action_penalty * np.mean(np.abs(old.astype(np.float64) - yaw))
    else:
        ref = action_penalty * (np.mean(np.abs(yaw.astype(np.float64))) / yaw_max)
    got = shim.rule_penalty(action_penalty, ptype, old.ctypes.data_as(C.c_void_p), yaw.ctypes.data_as(C.c_void_p), 7, yaw_max)
    assert got == ref and (got > 0) == (action_penalty >= 0.001)
    for pr, scale in [(0.0137, 1.0), (-0.25, 3.0)]:
        assert bits(F(shim.rule_reward(pr, scale, got))) == bits(F(pr * scale + 0.0 - ref))


def test_metric_add_lane_by_lane(shim):
    """recordEpisodeVals.py:31-64: step sums every step, episode sums on the step that truncates"""
    names = ["ep_return", "ep_length", "ep_mean_power", "n_episodes", "step_reward", "farm_power", "base_power", "n_steps"]
    rew, pnow, pbase, ret, length, psum = F(-0.37), F(1.4e7), F(1.9e7), F(-181.5), 685, F(9.1e9)
    for trunc in (0, 1):
        ref = dict(ep_return=ret * trunc, ep_length=F(length) * trunc, ep_mean_power=F(psum / F(length)) * trunc, n_episodes=F(trunc),
                   step_reward=rew, farm_power=pnow, base_power=pbase, n_steps=F(1))
        for lane, name in enumerate(names):
            assert bits(F(shim.rule_metric_add(lane, rew, pnow, pbase, trunc, ret, length, psum))) == bits(F(ref[name])), (trunc, name)
        assert shim.rule_metric_add(len(names), rew, pnow, pbase, trunc, ret, length, psum) == 0.0


@pytest.mark.parametrize("extra_inc", [0, 1])
@pytest.mark.parametrize("time_max", [1, 2, 25, 26])
def test_episode_steps(shim, time_max, extra_inc):
    """Wind_Farm_Env.py:1003, :1027: the timestep grows by 1 + extra_inc per step and the step that reaches time_max truncates; the
    rule is that count plus one, as the background plan has always taken it."""
    t, steps = 0, 0
    while True:
        t += 1 + extra_inc
        steps += 1
        if t >= time_max:
            break
    assert shim.rule_episode_steps(time_max, extra_inc) == steps + 1
    assert shim.rule_episode_steps_inc(time_max, 1 + extra_inc) == steps + 1
    assert shim.rule_episode_steps(time_max, 7 * extra_inc) == steps + 1          # any non-zero flag is one extra step
