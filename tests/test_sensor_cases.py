"""tests/sensor_cases.py on the CPU: the table reaches every step path with every window geometry and fill (decided from the plan of
tests/plan_shim.cpp), the oracle's trajectories meet the preconditions the device comparison relies on, and the comparison can
fail — the oracle with ONE channel's effective window changed by one sample misses the bar tests/test_gpu_sensor_cases.py applies."""
import numpy as np
import pytest

import sensor_cases as sc
import variant_census as vc
from test_plan import shim  # noqa: F401  (the g++-only plan fixture)

_REF = {}


def ref_of(oracle_lib, cs, *over, fill=None):
    """one oracle trajectory per config, shared and read-only"""
    key = cs.ref_id(*over, fill=fill)
    if key not in _REF:
        _REF[key] = sc.reference(oracle_lib, cs, *over, fill=fill)
    return _REF[key]


def unique_cases():
    seen, out = set(), []
    for cs in sc.CASES:
        if cs.ref_id() not in seen:
            seen.add(cs.ref_id())
            out.append(cs)
    return out


UNIQUE = unique_cases()
FAMILIES = {"k_flow + k_glue_lean": (1, 2, 3, 5, 6), "k_flow_env fused": (7, 8), "k_flow_env fused, pass waves": (9,), "k_flow_envb fused": (12,),
            "glue 2": (11,)}


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def test_table_size_and_sensor_sets():
    assert len(sc.CASES) <= 70 and len({c.name for c in sc.CASES}) == len(sc.CASES)
    s = sc.SETS
    geo = {n: {c: (s[n][c]["current"], s[n][c]["rolling_mean"], s[n][c]["history_N"], s[n][c]["history_length"], s[n][c]["window_length"])
               for c in sc.CHANNELS} for n in s}
    assert geo["short"] == dict(ws=(True, True, 1, 12, 5), wd=(True, True, 1, 8, 1), yaw=(True, True, 1, 9, 4), power=(True, True, 1, 20, 7))
    assert geo["beyond"] == dict(ws=(False, True, 1, 12, 30), wd=(False, True, 1, 1, 1), yaw=(False, True, 1, 2, 3), power=(False, True, 1, 1, 4))
    assert geo["current"] == dict(ws=(True, False, 1, 25, 25), wd=(True, False, 1, 20, 20), yaw=(True, False, 1, 10, 10), power=(True, False, 1, 10, 10))
    assert geo["generic"] == geo["short"]
    assert geo["generic-n"] == dict(geo["short"], ws=(True, True, 3, 12, 5), yaw=(True, True, 2, 9, 4))
    for n in ("short", "beyond", "current"):
        lv = s[n]["mes_level"]
        assert (lv["turb_ws"], lv["turb_wd"], lv["turb_power"]) == (True, True, True) and not any(lv[k] for k in ("turb_TI", "farm_ws", "farm_wd", "farm_TI", "farm_power"))
    for n in ("generic", "generic-n"):
        lv = s[n]["mes_level"]
        assert all(lv[k] for k in ("turb_ws", "turb_wd", "turb_power", "turb_TI", "farm_ws", "farm_TI", "farm_power"))
    assert set(sc.FARMS) == {(3, 2), (4, 4), (5, 4), (6, 6), (13, 5)}      # (no Horns Rev; 65 turbines: the smallest grid on path 6)
    assert {c.fill for c in sc.CASES} == {True, False, 3}


def test_every_path_sees_every_geometry_and_fill(shim):  # noqa: F811
    by_path, plans = {}, {}
    for cs in sc.CASES:
        plan = plans[cs.name] = sc.plan_of(shim, cs)
        assert plan["rc"] == 0, (cs.name, plan)
        assert sc.path_of(cs, plan) == cs.path, (cs.name, sc.path_of(cs, plan), plan)
        by_path.setdefault(cs.path, []).append(cs)
        cfg = cs.cfg()
        c = cfg.to_c()
        assert c.n_farms == 2 and c.autoreset == 1 and (c.fill_steps_agent, c.fill_steps_base) == (cfg.steps_on_reset, cfg.hist_max), cs.name
        assert cfg.steps_on_reset == {True: cfg.hist_max, False: 1, 3: 3}[cs.fill] and cfg.hist_max in (12, 25), cs.name
        assert (c.n_envs, c.n_rotor_pts) == ((2, 8) if c.n_turb >= 36 else ((2, 16) if c.n_turb == 20 else (5, 16))), cs.name
        assert c.noise == int(cs.noise) and (cs.noise or cs.inflow != "None"), cs.name      # steady inflow: always under noise
        if cs.noise:
            assert tuple(c.noise_sigma) == vc.AllChannelNoiseConfig.SIGMA, cs.name
        # sums mode, generic and fused as intended
        generic = cs.set_name.startswith("generic")
        hooks = dict(cs.hooks)
        assert plan["sums_mode"] == int(cs.set_name != "generic-n" and hooks.get("sums") != 0), cs.name
        if generic:
            assert plan["path_fused"] == 0 and cs.path in (1, 2, 3, 4, 5, 6, 10, 13), cs.name
        if cs.path in (7, 8, 9, 11, 12):
            assert plan["path_fused"] == 1 and plan["sums_mode"] == 1, cs.name
        if cs.multi:
            assert plan["path_fused"] == 1, cs.name
    assert set(by_path) == set(sc.PATHS) == set(range(1, 15))
    # every one of paths 1 - 12 sees short and beyond, each with a full and a partial fill
    for path in range(1, 13):
        got = {(c.set_name, c.partial) for c in by_path[path]}
        assert got >= {("short", False), ("short", True), ("beyond", False), ("beyond", True)}, (path, got)
    partial = {c.fill for c in sc.CASES if c.partial and c.set_name in ("short", "beyond")}
    assert partial == {False, 3}
    # `current` on at least one path of each family
    cur = {c.path for c in sc.CASES if c.set_name == "current"}
    for fam, paths in FAMILIES.items():
        assert cur & set(paths), fam
    assert {c.partial for c in sc.CASES if c.set_name == "current"} == {False, True}
    # `generic` on the paths it reaches
    assert {c.path for c in sc.CASES if c.set_name == "generic"} == {1, 2, 3, 4, 5, 6, 10, 13}
    gn = [c for c in sc.CASES if c.set_name == "generic-n"]
    assert [c.path for c in gn] == [4] and all("sums" not in dict(c.hooks) and c.fill is False for c in gn)      # (ring staging by itself)
    # short / False on the ring-staging path with 8, 4, 2 and 1 lanes per turbine
    lanes = {sc.LANES[c.farm] for c in by_path[4] if c.set_name == "short" and c.fill is False and plans[c.name]["sums_mode"] == 0}
    assert lanes == {1, 2, 4, 8}
    for farm, L in sc.LANES.items():      # (build_obs<L>, lean_swap's Lg: the largest power of two up to 8 with N L <= 64)
        N = farm[0] * farm[1]
        assert L == max(l for l in (1, 2, 4, 8) if l == 1 or N * l <= 64), farm
    # the members the paths name
    key = {cs.name: vc.key_of(cs, plans[cs.name]) for cs in sc.CASES}
    assert {key[c.name][4] for c in by_path[9]} == {1, 2}
    assert {key[c.name][3] for c in by_path[12]} == {1, 2, 4} and all(key[c.name][2] == 1 for c in by_path[12])
    assert {key[c.name][:3] for c in by_path[5]} == {("k_flow", 256, True), ("k_flow", 64, True)}
    assert {key[c.name][:3] for c in by_path[6]} == {("k_flow", 256, True)} and all(c.cfg().n_turb > 64 for c in by_path[6])
    assert all(key[c.name][:4] == ("k_flow_env", True, 1, 1) for c in by_path[7])
    assert all(key[c.name][:5] == ("k_flow_env", True, 1, 2, 0) for c in by_path[8])
    assert all(key[c.name][:3] == ("k_flow_env", True, 2) for c in by_path[11])
    assert all(key[c.name][:3] == ("k_flow_env", True, 0) for c in by_path[10])
    assert all(key[c.name][:3] == ("k_flow_envb", True, 0) for c in by_path[13])
    assert all(k in vc.ALL_KEYS for k in key.values())
    # turbulent inflow with and without noise; the NOISE = false instantiations of the fused k_flow_envb see both sets partly filled
    for path in (2, 3, 12):
        assert {c.noise for c in by_path[path]} == {False, True}, path
    assert {c.set_name for c in by_path[12] if not c.noise and c.partial} >= {"short", "beyond"}
    assert {(c.set_name, c.partial) for c in by_path[12] if c.noise} == {("short", False), ("beyond", False)}


def test_extra_cases(shim):  # noqa: F811
    a, b, c = sc.case("x-restore"), sc.case("x-multi-window"), sc.case("x-short-extra-inc")
    for cs in (a, b):      # short / False on the default fused path
        assert (cs.set_name, cs.fill, cs.farm, cs.inflow, cs.multi) == ("short", False, (3, 2), "None", False)
        assert sc.plan_of(shim, cs)["path_fused"] == 1
    assert a.restore_at == (2, 40) and sc.filling_steps(a) >= 2      # step 2 is mid-fill
    assert b.multi_window == (30, 55)
    assert (c.set_name, c.fill, c.multi, c.path) == ("short", 3, True, 11) and c.cfg().to_c().extra_timestep_inc == 1
    # uniform rings: nothing prepares an episode's sums, every swap sums them itself (6 turbines: eight lanes each; 65: two passes)
    for name, n, fill in (("p14-short-f3", 6, 3), ("p14-65-short-f3", 65, 3)):
        cs = sc.case(name)
        plan = sc.plan_of(shim, cs)
        assert (cs.set_name, cs.fill, cs.path, cs.cfg().n_turb) == ("short", fill, 14, n)
        assert (plan["path_envw"], plan["sums_mode"], plan["first_obs"], plan["res"], plan["block"]) == (0, 1, 0, 0, 256)
    assert all(sc.plan_of(shim, x)["first_obs"] == 1 for x in sc.CASES if x.path != 14 and sc.plan_of(shim, x)["sums_mode"])
    assert sum(bool(x.restore_at or x.multi_window or x.extra_inc) for x in sc.CASES) == 3


# ---- preconditions on the reference alone -----------------------------------------------------------------------------------------
CLIP_SHARE_MAX = 0.01      # a condition of the table, not a fit


@pytest.mark.parametrize("name", [c.name for c in UNIQUE])
def test_reference_preconditions(oracle_lib, name):
    cs = sc.case(name)
    ref = ref_of(oracle_lib, cs)
    assert cs.steps <= 100
    tr = ref["tr"]
    assert (tr.sum(axis=0) >= 1).all(), tr.sum(axis=0)
    for k in ("obs0", "obs", "fin", "rew", "multi0", "multi"):
        assert np.isfinite(ref[k]).all(), k
    assert ref["obs"].std(axis=(0, 1)).min() > 0.0      # every observation column varies
    clip = float(np.mean(np.abs(np.concatenate([ref["obs0"][None], ref["obs"]])) >= 1.0))
    assert clip <= CLIP_SHARE_MAX, clip
    # the longest episode pushes 63 samples or more: the longest ring (power of `short`: capacity 21) wraps three times
    longest = 0
    for b in range(tr.shape[1]):
        ends = np.concatenate([[-1], np.flatnonzero(tr[:, b]), [cs.steps - 1]])
        longest = max(longest, int(np.diff(ends).max()))
    assert sc.fill_steps(cs) + longest >= 3 * 21, (longest, sc.fill_steps(cs))
    if cs.partial:
        # the partly filled deques reach the first observation ...
        full = ref_of(oracle_lib, cs, fill=True)
        assert np.abs(full["obs0"] - ref["obs0"]).max() > 10 * vc.obs_atol(cs), name
        # ... and, where there is a rolling mean, at least one step after every reset reads a window that is still filling
        if cs.rolling():
            assert sc.filling_steps(cs) >= 1, name
    else:
        assert sc.filling_steps(cs) == 0, name
    if cs.restore_at:      # the second restore comes after a rollover
        assert tr[:cs.restore_at[-1]].any() and sc.filling_steps(cs) >= cs.restore_at[0]
    if cs.multi_window:    # envs roll over while the per-agent buffer is registered, and after
        on, off = cs.multi_window
        assert tr[on:off].any() and tr[off:].any()


def test_filling_steps_from_the_settings():
    """n_pushed < min(W, H) after a reset, from the settings alone: the reset leaves fill_steps samples and every step pushes one"""
    assert sc.filling_steps(sc.case("p1-short-f1")) == 5        # power: W 7; 2 .. 6 samples after steps 1 .. 5
    assert sc.filling_steps(sc.case("p1-beyond-f3")) == 8       # ws: min(30, 12) = 12; 4 .. 11 samples
    assert sc.filling_steps(sc.case("p9-pass2-short-f3")) == 3  # power: 4 .. 6 samples
    assert sc.filling_steps(sc.case("p1-short-full")) == 0 and sc.filling_steps(sc.case("p1-current-f1")) == 0


# ---- reference-side controls: one window changed by one sample breaks the bar of the device comparison ------------------------------
def share_of_steps(cs, a, b):
    """share of the observations (reset and every step) in which some entry misses the case's observation bar"""
    miss = np.abs(np.concatenate([a["obs0"][None], a["obs"]]) - np.concatenate([b["obs0"][None], b["obs"]])) > vc.obs_atol(cs)
    return float(miss.any(axis=(1, 2)).mean())


@pytest.mark.parametrize("name", [c.name for c in UNIQUE if c.rolling()])
def test_one_window_changed_breaks_the_bar(oracle_lib, name):
    """The GPU comparison can fail: for each case and each channel with a rolling mean, the oracle with that channel's effective
    window changed by one sample (sensor_cases.CONTROLS) misses the observation bar tests/test_gpu_sensor_cases.py applies, on at
    least half of the steps.  The two channels of `beyond` without such a control say why, and what they say is asserted."""
    cs = sc.case(name)
    ref = ref_of(oracle_lib, cs)
    for ch in cs.rolling():
        ctl = cs.control(ch)
        if isinstance(ctl, str):
            assert cs.set_name == "beyond" and ch in ("ws", "wd")
            if ch == "wd":      # a deque of 2 under the window of 1: the same numbers
                other = ref_of(oracle_lib, cs, ("wd", "history_length", 2))
                np.testing.assert_array_equal(other["obs"], ref["obs"])
                np.testing.assert_array_equal(other["obs0"], ref["obs0"])
            else:               # the window length beyond the deque's changes nothing
                other = ref_of(oracle_lib, cs, ("ws", "window_length", 31))
                np.testing.assert_array_equal(other["obs"], ref["obs"])
                assert cs.cfg(("ws", "history_length", 13)).hist_max != cs.cfg().hist_max
            continue
        assert cs.cfg(ctl).hist_max == cs.cfg().hist_max and cs.cfg(ctl).steps_on_reset == cs.cfg().steps_on_reset
        other = ref_of(oracle_lib, cs, ctl)
        np.testing.assert_array_equal(other["tr"], ref["tr"])
        s = share_of_steps(cs, other, ref)
        assert s >= 0.5, (name, ch, ctl, s)
        # ... and only that channel's entries move
        lay = cs.cfg().obs_layout()
        off, n = lay["turb"][ch]
        cols = np.zeros(ref["obs"].shape[-1], bool)
        for t in range(cs.cfg().n_turb):
            cols[t * lay["turb_block"] + off:t * lay["turb_block"] + off + n] = True
        if ch in lay["farm"]:
            cols[lay["farm"][ch][0]:lay["farm"][ch][0] + lay["farm"][ch][1]] = True
        np.testing.assert_array_equal(other["obs"][..., ~cols], ref["obs"][..., ~cols])


@pytest.mark.parametrize("name", [c.name for c in UNIQUE if c.set_name == "current"])
def test_current_is_the_one_sample_rolling_mean(oracle_lib, name):
    """`current` and a rolling mean over one sample are two statements of "the newest sample": the oracle with a channel's `current`
    replaced by a rolling mean of H 2 / W 1 gives the same numbers.  (Where the replacement changes hist_max — ws, whose deque is
    the longest — and with it the fill, the channel is tried on the partial-fill cases only.)"""
    cs = sc.case(name)
    ref = ref_of(oracle_lib, cs)
    tried = []
    for ch in sc.CHANNELS:
        over = ((ch, "current", False), (ch, "rolling_mean", True), (ch, "history_length", 2), (ch, "window_length", 1))
        if cs.cfg(*over).steps_on_reset != cs.cfg().steps_on_reset:
            continue
        other = ref_of(oracle_lib, cs, *over)
        np.testing.assert_array_equal(other["obs0"], ref["obs0"], err_msg=ch)
        np.testing.assert_array_equal(other["obs"], ref["obs"], err_msg=ch)
        tried.append(ch)
    assert tried == list(sc.CHANNELS) if cs.partial else tried == ["wd", "yaw", "power"], tried
