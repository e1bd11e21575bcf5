"""The sensor rules of the observation on every step path: per channel (ws, wd, yaw, power) `current` and / or the mean of the newest
min(window_length, history_length, pushed) samples of a deque history_length long, partly filled after a reset when fill_window is
False or a small integer (Mes.get_measurements, MesClass.py:70-125; Wind_Farm_Env.py:229-240).  The device states the rule at
least five times (build_obs in wg_obs.h; wg_sums_load / wg_sums_apply / wg_sums_mean; the rebuild of the sums at a same-step
autoreset, lean_swap; the flow kernel's prepared first observation, wg_first_obs / env_first_obs; the early loads of the fused step
kernels), and tests/variant_census.py and tests/rule_cases.py fix the geometry at env1_config's: window == history on every channel
and a full fill — where the leaving sample of a window is always the ring slot about to be overwritten, the window never fills
while the episode runs and the swap sums whole deques.  This table varies the geometry: the twelve step paths of rule_cases.PATHS
(and two more, below) times the sensor sets SETS times fill_window True / False / 3, and a few extra cases.
tests/test_sensor_cases.py pins coverage, preconditions and the reference-side controls on the CPU;
tests/test_gpu_sensor_cases.py runs every case by value against the oracle.

The task rules stay at env1_config's (rule_cases.ENV1: Baseline reward, two farms — the baseline farm fills hist_max whatever
fill_window says)."""
from dataclasses import dataclass

import numpy as np

import rule_cases as rc
import variant_census as vc
from windgym_amd import presets
from windgym_amd.config import EnvConfig
from windgym_amd.turbine import V80

CHANNELS = ("ws", "wd", "yaw", "power")
_LEVEL = dict(turb_ws=True, turb_wd=True, turb_TI=False, turb_power=True, farm_ws=False, farm_wd=False, farm_TI=False, farm_power=False)


def _ch(current, rolling, H, W, HN=1):
    return dict(current=current, rolling_mean=rolling, history_N=HN, history_length=H, window_length=W)


# ---- the sensor sets: history_N is 1 wherever a rolling mean is on, no TI, nothing farm-level -> sums mode, fused -------------------------
SETS = {
    # W < H on every channel, W == 1 on wd
    "short": dict(mes_level=_LEVEL, ws=_ch(True, True, 12, 5), wd=_ch(True, True, 8, 1), yaw=_ch(True, True, 9, 4), power=_ch(True, True, 20, 7)),
    # W > H (the window is clamped to the deque), H == 1 (ring capacity 2) and H == 2, W == H == 1 on wd; rolling means only
    "beyond": dict(mes_level=_LEVEL, ws=_ch(False, True, 12, 30), wd=_ch(False, True, 1, 1), yaw=_ch(False, True, 2, 3), power=_ch(False, True, 1, 4)),
    # no running sum at all (sum_mask_t == 0): `current` only, env1_config's lengths
    "current": dict(mes_level=_LEVEL, ws=_ch(True, False, 25, 25), wd=_ch(True, False, 20, 20), yaw=_ch(True, False, 10, 10),
                    power=_ch(True, False, 10, 10)),
}
_GEN_LEVEL = dict(_LEVEL, turb_TI=True, farm_ws=True, farm_TI=True, farm_power=True)
# `short` with TI and farm-level entries: a generic layout (GEN), no fused tail.  TI is computed over the whole ws deque while it fills
SETS["generic"] = dict(SETS["short"], mes_level=_GEN_LEVEL)
# ... and with several windows per channel: not sums mode, the ring-staging k_glue — build_obs' `avail < W`, `spacing < 1` and
# `pos > avail - W` branches, which a full fill never reaches
SETS["generic-n"] = dict(SETS["generic"], ws=_ch(True, True, 12, 5, HN=3), yaw=_ch(True, True, 9, 4, HN=2))
FILLS = (True, False, 3)

# ---- reference-side controls: the oracle with ONE channel's effective window changed by one sample ---------------------------------------
# (set, channel) -> (setting, delta) or a string: why the channel has no control that leaves everything else alone.  Where W < H the
# window length moves; where W >= H the window is the deque and the deque length moves — of yaw (hist_max stays the ws deque's 12)
# and of power (not part of hist_max, MesClass.py:239-246) only: the ws deque's length IS hist_max, so changing it changes the fill
# length of a full fill and of the baseline farm, and with it the noise stream; a shifted stream is not a control.
CONTROLS = {
    ("short", "ws"): ("window_length", +1), ("short", "wd"): ("window_length", +1), ("short", "yaw"): ("window_length", -1),
    ("short", "power"): ("window_length", -1),
    ("beyond", "ws"): "W > H and the ws deque's length is hist_max: changing it changes the fill length and the noise stream",
    ("beyond", "wd"): "W == H == 1: the window is the newest sample whatever the deque's length (asserted: H 2 gives the same numbers)",
    ("beyond", "yaw"): ("history_length", +1), ("beyond", "power"): ("history_length", +1),
}
for _c in CHANNELS:
    CONTROLS[("generic", _c)] = CONTROLS[("generic-n", _c)] = CONTROLS[("short", _c)]

# ---- the farms: (B, rotor points, n_passthrough, steps): rule_cases.FARMS' small ones.  n_passthrough so that every env truncates
# inside `steps` and, on the 3 x 2 and 4 x 4 farms, the longest episode pushes 63 samples or more: the longest ring (power of
# `short`, capacity 21) wraps three times.  13 x 5 = 65 turbines is the smallest grid on path 6 (more than 64 turbines: the sums'
# second trip over the lanes); Horns Rev is not here.
FARMS = {
    (3, 2): (5, 16, 0.52, 80),
    (4, 4): (5, 16, 0.39, 90),
    (5, 4): (2, 16, 0.3, 80),
    (6, 6): (2, 8, 0.26, 100),
    (13, 5): (2, 8, 0.125, 80),
}
LANES = {(3, 2): 8, (4, 4): 4, (5, 4): 2, (6, 6): 1}      # lanes per turbine of build_obs<L> (k_glue) and of the swaps' group sums (Lg)


@dataclass(frozen=True)
class Case:
    name: str
    path: int                   # the step path the case is meant for (PATHS); tests/test_sensor_cases.py checks it against the plan
    farm: tuple                 # (nx, ny)
    inflow: str                 # "None" | "Random" | "box"
    set_name: str               # key of SETS
    fill: object                # fill_window: True | False | 3
    noise: bool                 # sensor noise on all four channels (variant_census.AllChannelNoiseConfig)
    hooks: tuple = ()           # (plan hook name, value) pairs
    multi: bool = False         # the per-agent buffer is registered (fuse_obs_multi())
    steps: int = 80
    extra_inc: bool = False     # extra_timestep_inc=True (the multi-agent facade's double clock)
    restore_at: tuple = ()      # steps before which the handle runs set_state(get_state())
    multi_window: tuple = ()    # (on, off): fuse_obs_multi() is switched on before step `on` and off before step `off`
    script = False              # (no flow script, ever: variant_census.key_of reads this)
    rules = tuple(sorted(rc.ENV1.items()))      # (rule_cases.reward_bar reads these)
    penalty_state = "off"
    n_farms = 2

    def sensors(self, *over):
        """the set's channel settings with (channel, setting, value) triples replaced"""
        s = {k: dict(v) for k, v in SETS[self.set_name].items()}
        for ch, key, val in over:
            s[ch][key] = val
        return s

    def cfg(self, *over):
        s = self.sensors(*over)
        B, S, npt, _ = FARMS[self.farm]
        d = presets._upd(vc._yaml(self.noise, *self.farm), mes_level=s["mes_level"],
                         **{f"{c}_mes": {f"{c}_{k}": v for k, v in s[c].items()} for c in CHANNELS})
        cls = vc.AllChannelNoiseConfig if self.noise else EnvConfig
        # (the double clock halves an episode's steps: twice the passthrough keeps them)
        return cls(turbine=V80(), yaml_dict=d, turbtype={"box": "MannGenerate"}.get(self.inflow, self.inflow), n_envs=B, autoreset=True,
                   n_passthrough=npt * (2 if self.extra_inc else 1), n_rotor_pts=S, fill_window=self.fill, extra_timestep_inc=self.extra_inc)

    def ref_id(self, *over, fill=None):
        """cases with equal ref_id share one oracle trajectory (hooks, the per-agent buffer and what the handle is asked to do on the
        way are the handle's business)"""
        return (self.farm, self.inflow, self.set_name, self.fill if fill is None else fill, self.noise, self.steps, self.extra_inc, tuple(over))

    @property
    def partial(self):
        return self.fill is not True

    def rolling(self):
        return [c for c in CHANNELS if SETS[self.set_name][c]["rolling_mean"]]

    def control(self, ch):
        """the (channel, setting, value) triple of the channel's control, or the reason why there is none"""
        c = CONTROLS[(self.set_name, ch)]
        if isinstance(c, str):
            return c
        return (ch, c[0], SETS[self.set_name][ch][c[0]] + c[1])


# ---- the paths ------------------------------------------------------------------------------------------------------------------------
PATHS = dict(rc.PATHS)
PATHS[13] = "k_flow_envb + unfused k_glue_lean (a generic observation on box inflow)"
PATHS[14] = "k_flow 256 on uniform rings + k_glue_lean, steady (large turbulent farms run on such rings; here by hook)"
_SMALL = (3, 2)
# path -> members (suffix, farm, inflow, hooks, multi); then per member the (set, fill, noise) combinations
_MEMBERS = {
    1: [("", _SMALL, "None", {"flow_env": 0}, False)],
    2: [("", _SMALL, "Random", {}, False)],
    3: [("", _SMALL, "box", {"flow_env": 0}, False)],
    4: [("", _SMALL, "None", {"sums": 0, "flow_env": 0}, False)],
    5: [("-36", (6, 6), "None", {}, False), ("-20", (5, 4), "None", {"flow_env": 0}, False)],
    6: [("", (13, 5), "None", {}, False)],
    7: [("", _SMALL, "None", {"env_wpe": 1}, False)],
    8: [("", _SMALL, "None", {"env_wpe": 2}, False)],
    9: [("-pass1", (4, 4), "None", {"env_split": 1}, False), ("-pass2", (4, 4), "None", {"env_split": 2}, False)],
    10: [("", _SMALL, "None", {"step_fused": 0}, False)],
    11: [("", _SMALL, "None", {}, True)],
    12: [("-w1", _SMALL, "box", {"env_wpe": 1}, False), ("-w2", _SMALL, "box", {"env_wpe": 2}, False), ("-w4", _SMALL, "box", {"env_wpe": 4}, False)],
}
# short and beyond, each with a full and a partial fill, on every path; the partial fill alternates between False and 3 and the
# members of a path take turns.  (member index, set, fill) per path with one / two / three members:
_COMBOS = {1: [(0, "short", True), (0, "short", False), (0, "beyond", True), (0, "beyond", 3)],
           2: [(0, "short", True), (1, "short", 3), (1, "beyond", True), (0, "beyond", False)],
           3: [(0, "short", True), (1, "short", False), (2, "beyond", True), (0, "beyond", 3)]}
# steady inflow: noise on all four channels (without it the ws and wd windows are invisible: the un-noised wd is constant, ws nearly).
# Turbulent inflow: short without noise, beyond with it on paths 2 and 3; on path 12 the full fills with noise and the partial ones
# without, so that the NOISE = false instantiations of k_flow_envb see a partly filled window of both sets.
def _noise_of(path, inflow, set_name, fill):
    if inflow == "None":
        return True
    if path == 12:
        return fill is True
    return set_name == "beyond"


def _mk(name, path, member, set_name, fill, noise=None, steps=None, **kw):
    _, farm, inflow, hooks, multi = member
    noise = _noise_of(path, inflow, set_name, fill) if noise is None else noise
    return Case(name, path, farm, inflow, set_name, fill, noise, tuple(sorted(hooks.items())), multi, FARMS[farm][3] if steps is None else steps, **kw)


def _fill_tag(fill):
    return {True: "full", False: "f1"}.get(fill, f"f{fill}")


def _cases():
    out = []
    for path, members in _MEMBERS.items():
        for mi, s, fill in _COMBOS[len(members)]:
            out.append(_mk(f"p{path}{members[mi][0]}-{s}-{_fill_tag(fill)}", path, members[mi], s, fill))
    # ---- `current` on one path of each family: k_flow + k_glue_lean, k_flow_env fused without and with pass waves, k_flow_envb fused,
    # glue 2 with the per-agent buffer
    for path, mi, fill in ((1, 0, False), (8, 0, True), (9, 1, 3), (12, 1, False), (11, 0, 3)):
        m = _MEMBERS[path][mi]
        out.append(_mk(f"p{path}{m[0]}-current-{_fill_tag(fill)}", path, m, "current", fill))
    # ---- the generic set on the paths it reaches: 1 .. 6, 10 (the default plan: an env kernel with an unfused glue) and 13
    dflt, dflt_box = ("", _SMALL, "None", {}, False), ("", _SMALL, "box", {}, False)
    for path, m, fill in ((1, _MEMBERS[1][0], False), (2, _MEMBERS[2][0], 3), (3, _MEMBERS[3][0], True), (4, _MEMBERS[4][0], 3),
                          (5, _MEMBERS[5][0], False), (6, _MEMBERS[6][0], 3), (10, dflt, False), (13, dflt_box, 3)):
        out.append(_mk(f"p{path}-generic-{_fill_tag(fill)}", path, m, "generic", fill, noise=True))
    # (several windows per channel: not sums mode whatever the hooks say)
    out.append(_mk("p4-generic-n-f1", 4, ("", _SMALL, "None", {"flow_env": 0}, False), "generic-n", False))
    # ---- short / False on the ring-staging path with 8 (p4-short-f1, above), 4, 2 and 1 lanes per turbine
    for farm in ((4, 4), (5, 4), (6, 6)):
        out.append(_mk(f"p4-lanes{LANES[farm]}-short-f1", 4, ("", farm, "None", {"sums": 0, "flow_env": 0}, False), "short", False))
    # ---- extra cases, short / False on the default fused path (two waves per env)
    fused = _MEMBERS[8][0]
    # (a) set_state(get_state()) before step 2 — mid-fill — and before step 40 — after a rollover: the restored handle has no
    # prepared sums; the resting background wave prepares them again in the next launch (env_first_obs)
    out.append(_mk("x-restore", 8, fused, "short", False, restore_at=(2, 40)))
    # ---- path 14, uniform rings: no flow kernel prepares an episode's sums there (the plan's first_obs is 0), so EVERY swap sums the
    # windows itself — lean_swap's fallback, cnt = min(sum_w, n_pushed), which a handle on compact rings never runs (its flow kernel
    # prepares a resting background episode again in every launch, also after set_state).  In one pass over 6 turbines, eight lanes
    # each, and in two passes over 65, one lane each.  Fill 3: after a fill of 1 every window holds the one sample there is, and a
    # swap that summed too many slots of the zeroed ring would still be right
    out.append(_mk("p14-short-f3", 14, ("", _SMALL, "None", {"flow_block": 256}, False), "short", 3))
    out.append(_mk("p14-65-short-f3", 14, ("", (13, 5), "None", {"flow_res": 0}, False), "short", 3))
    # (b) the per-agent buffer switched on before step 30 and off before step 55: glue 1 -> glue 2 -> glue 1 on running sums
    out.append(_mk("x-multi-window", 8, fused, "short", False, multi_window=(30, 55)))
    # (c) the per-agent buffer on the double clock
    out.append(_mk("x-short-extra-inc", 11, _MEMBERS[11][0], "short", 3, extra_inc=True))
    return out


CASES = _cases()
assert len(CASES) <= 70 and len({c.name for c in CASES}) == len(CASES)


def case(name):
    return next(c for c in CASES if c.name == name)


# ---- which path a case runs, from the plan ---------------------------------------------------------------------------------------
def plan_of(shim, cs):
    cfg = cs.cfg()
    return shim(cfg, box_cells=vc.box_cells(cfg), **dict(cs.hooks))


def path_of(cs, plan):
    """rule_cases.path_of, and for what it calls None: 13 on box inflow, k_flow_envb with an unfused k_glue_lean; 14 on steady
    inflow, the per-slot kernel on uniform rings with k_glue_lean"""
    if cs.inflow == "None" and not plan["path_envw"] and plan["sums_mode"] and (plan["block"], plan["res"]) == (256, 0):
        return 14      # (rule_cases.path_of does not look at the rings of a farm of more than 64 turbines)
    p = rc.path_of(cs, plan)
    if p is None and cs.inflow == "box" and plan["path_envw"] and not plan["path_fused"] and plan["sums_mode"]:
        return 13
    return p


def seeds_of(cs):
    return 4100 + np.arange(FARMS[cs.farm][0])


def actions_of(cs):
    return np.random.default_rng(19).uniform(-1, 1, size=(cs.steps, FARMS[cs.farm][0], cs.farm[0] * cs.farm[1])).astype(np.float32)


def fill_steps(cs):
    """samples in the agent farm's deques after a reset (Wind_Farm_Env.py:229-240), from the config"""
    return cs.cfg().steps_on_reset


def filling_steps(cs):
    """steps after a reset whose observation reads a window that is still filling: n_pushed < min(W, H) on some channel with a
    rolling mean.  From the settings alone: a reset leaves fill_steps samples, every step pushes one."""
    s = SETS[cs.set_name]
    need = max((min(s[c]["window_length"], s[c]["history_length"]) for c in cs.rolling()), default=0)
    return max(0, need - fill_steps(cs) - 1)


# ---- bars ---------------------------------------------------------------------------------------------------------------------------
def raw_scale(cs):
    """per observation entry: (minimum, range) of its scaling (MesClass.py:440-444; wg_scale), so that an unclipped entry o holds
    the unscaled sensor value (o + 1) / 2 * range + minimum — what measurements() returns"""
    cfg = cs.cfg()
    c, lay = cfg.to_c(), cfg.obs_layout()
    sc = dict(ws=(c.ws_scale_min, c.ws_scale_max - c.ws_scale_min), wd=(c.wd_scale_min, c.wd_scale_max - c.wd_scale_min),
              yaw=(c.yaw_min, c.yaw_max - c.yaw_min), TI=(c.ti_scale_min, c.ti_scale_max - c.ti_scale_min), power=(0.0, c.power_max))
    mn, rng = np.zeros(cfg.obs_var), np.ones(cfg.obs_var)
    for t in range(cfg.n_turb):
        for name, (off, n) in lay["turb"].items():
            a = t * lay["turb_block"] + off
            mn[a:a + n], rng[a:a + n] = sc[name]
    for name, (off, n) in lay["farm"].items():
        mn[off:off + n], rng[off:off + n] = (0.0, c.power_max * cfg.n_turb) if name == "power" else sc[name]
    return mn, rng


# ---- the oracle's side of a case ---------------------------------------------------------------------------------------------------
def reference(oracle_lib, cs, *over, fill=None):
    """The oracle's trajectory of a case: reset on seeds_of, step on actions_of; every step's observation, per-agent observation,
    reward, flag and final observation.  `over`: (channel, setting, value) triples replacing sensor settings (the CPU controls);
    fill: another fill_window."""
    import dataclasses
    cs = cs if fill is None else dataclasses.replace(cs, fill=fill)
    orc = oracle_lib.Oracle(cs.cfg(*over))
    rc.install(cs, orc)
    acts = actions_of(cs)
    out = {k: [] for k in ("obs", "multi", "rew", "tr", "fin")}
    obs0, multi0 = orc.reset(seeds=seeds_of(cs)), orc.obs_multi()
    for k in range(cs.steps):
        obs, rew, tr, fin = orc.step(acts[k])
        out["obs"].append(obs), out["rew"].append(rew), out["tr"].append(tr), out["fin"].append(fin), out["multi"].append(orc.obs_multi())
    out = {k: np.stack(v) for k, v in out.items()}
    out.update(obs0=obs0, multi0=multi0, actions=acts)
    orc.close()
    for v in out.values():
        v.setflags(write=False)
    return out
