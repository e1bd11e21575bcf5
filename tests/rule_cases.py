"""The task rules of the environment on every step path: how an action moves the yaws (ActionMethod yaw / wind), how the baseline
farm's controller moves its yaws (BaseController Local / Global), the reward (Power_reward Baseline / Power_avg / None / Power_diff,
Power_avg, Power_scaling) and the action penalty (action_penalty, Change / Total, the `>= 0.001` switch).  The device code states
them once, in csrc/wg_rules.h (tests/test_rules_host.py), and calls them on every step path (wg_flow.hip, wg_env.hip, wg_envb.hip:
action rule and base controller; k_glue and lean_step: reward head and penalty sum, lean_step unfused and as the tail of k_flow_env /
k_flow_envb; the reward's switch over Power_reward stays in each glue), and tests/variant_census.py fixes them at env1_config's.
This table varies them: twelve step paths (PATHS, named by what the plan selects) times four rule sets (SETS), and a few extra
cases at the sizes where the glue takes another branch.  tests/test_rule_cases.py pins coverage, preconditions and the
reference-side controls on the CPU; tests/test_gpu_rule_cases.py runs every case by value against the oracle."""
from dataclasses import dataclass

import numpy as np

import variant_census as vc
from windgym_amd import presets
from windgym_amd.config import EnvConfig
from windgym_amd.turbine import V80

# ---- the rule sets -----------------------------------------------------------------------------------------------------------------
# env1_config's rules as the census runs them (its action is "yaw")
ENV1 = dict(ActionMethod="yaw", BaseController="Local", Power_reward="Baseline", Power_avg=10, Power_scaling=1.0, action_penalty=0.0,
            action_penalty_type="Change", Baseline_comp=False)
SETS = {
    "A": dict(ActionMethod="wind", BaseController="Global", Power_reward="Power_avg", Baseline_comp=True, Power_avg=7, Power_scaling=2.5,
              action_penalty=0.05, action_penalty_type="Total"),
    "B": dict(ActionMethod="yaw", BaseController="Local", Power_reward="Power_diff", Power_avg=40, action_penalty=0.05,
              action_penalty_type="Change"),
    "C": dict(ActionMethod="wind", BaseController="Local", Power_reward="None", action_penalty=0.001, action_penalty_type="Change"),
    "D": dict(ActionMethod="yaw", BaseController="Global", Power_reward="Baseline", Power_avg=64, Power_scaling=1.0, action_penalty=0.0009,
              action_penalty_type="Total"),
    # set C with a baseline farm: the Local controller at work (F = 2) where the reward is the penalty alone
    "C2": dict(ActionMethod="wind", BaseController="Local", Power_reward="None", Baseline_comp=True, action_penalty=0.001,
               action_penalty_type="Change"),
}
PENALTY_SWITCH = 0.001      # Wind_Farm_Env.py:808: `if self.action_penalty < 0.001: return 0`

# ---- the farms: (B, rotor points, n_passthrough, steps).  n_passthrough so that every env truncates inside `steps` (time_max =
# int(dist / ws * n_passthrough), ws 7 .. 15 m/s) and the longest episodes pass 30 steps, which a pinned turbine needs to reach a stop
FARMS = {
    (3, 2): (5, 16, 0.4, 80),        # dist 960 .. 1090 m: 25 to 62 steps
    (4, 4): (5, 16, 0.3, 90),        # dist 1280 .. 1570 m: 25 to 66 steps
    (5, 4): (5, 16, 0.2, 80),        # 20 turbines: the wave-sum branch of the penalty and power sums on the 64-thread kernel
    (6, 6): (2, 8, 0.2, 100),        # 36 turbines: the 256-thread compact kernel
    "hr": (2, 8, 0.1, 80),           # Horns Rev 1, 80 turbines: the `t = lane + 64` loop of the sums; episodes of 47 and 71 steps on
}                                    # seeds_of (the oracle's time is the development of each episode, so no step more than needed)
PIN = 1.5       # |action| of the two pinned turbines under "wind": a target beyond the stops (below)


def rules_of(over):
    r = dict(ENV1)
    r.update(over)
    return r


@dataclass(frozen=True)
class Case:
    name: str
    path: int                   # the step path the case is meant for (PATHS); tests/test_rule_cases.py checks it against the plan
    farm: object                # (nx, ny) or "hr"
    inflow: str                 # "None" | "Random" | "box"
    rules: tuple                # the rule settings, sorted (name, value) pairs: every key of ENV1
    set_name: str = ""          # key of SETS, "" for an extra case
    hooks: tuple = ()           # (plan hook name, value) pairs
    multi: bool = False         # the per-agent buffer is registered (fuse_obs_multi())
    steps: int = 80
    extra_inc: bool = False     # extra_timestep_inc=True (the multi-agent facade's double clock)
    script = False              # (no flow script, ever: a script forces the per-slot kernel — variant_census.key_of reads this)

    def rule(self, **override):
        r = dict(self.rules)
        r.update(override)
        return r

    def cfg(self, **override):
        """the case's EnvConfig, with rule settings replaced by `override`"""
        r = self.rule(**override)
        B, S, npt, _ = FARMS[self.farm]
        nx, ny = (10, 8) if self.farm == "hr" else self.farm
        d = presets._upd(vc._yaml(False, nx, ny), ActionMethod=r["ActionMethod"], BaseController=r["BaseController"],
                         act_pen=dict(action_penalty=r["action_penalty"], action_penalty_type=r["action_penalty_type"]),
                         power_def=dict(Power_reward=r["Power_reward"], Power_avg=r["Power_avg"], Power_scaling=r["Power_scaling"]))
        assert d["yaw_init"] == "Random"      # (env1_config's: the base controller has work to do)
        kw = {}
        if self.farm == "hr":
            kw["x_pos"], kw["y_pos"] = presets.horns_rev1_layout()
        # (the double clock halves an episode's steps: twice the passthrough keeps them)
        return EnvConfig(turbine=V80(), yaml_dict=d, turbtype={"box": "MannGenerate"}.get(self.inflow, self.inflow), n_envs=B, autoreset=True,
                         n_passthrough=npt * (2 if self.extra_inc else 1), n_rotor_pts=S, Baseline_comp=bool(r["Baseline_comp"]), extra_timestep_inc=self.extra_inc, **kw)

    def ref_id(self, **override):
        """cases with equal ref_id share one oracle trajectory (hooks and the per-agent buffer are the handle's business)"""
        return (self.farm, self.inflow, tuple(sorted(self.rule(**override).items())), self.steps, self.extra_inc)

    @property
    def n_farms(self):
        r = dict(self.rules)
        return 2 if r["Power_reward"] == "Baseline" or r["Baseline_comp"] else 1

    @property
    def penalty_state(self):
        r = dict(self.rules)
        return "off" if r["action_penalty"] < PENALTY_SWITCH else r["action_penalty_type"]


# ---- the paths: number -> (what the plan selects, farm, inflow, hooks, multi) ------------------------------------------------------------
PATHS = {
    1: "k_flow 64 + k_glue_lean, steady",
    2: "k_flow 64 + k_glue_lean, Random inflow",
    3: "k_flow 64 + k_glue_lean, box inflow",
    4: "k_flow + k_glue (ring staging)",
    5: "k_flow + k_glue_lean, steady, 17 .. 64 turbines (256 threads compact at 36, 64 threads at 20)",
    6: "k_flow 256 + k_glue_lean, steady, more than 64 turbines",
    7: "k_flow_env, one wave per env, fused",
    8: "k_flow_env, two waves, no pass wave, fused",
    9: "k_flow_env, pass waves, fused",
    10: "k_flow_env + unfused k_glue_lean",
    11: "k_flow_env fused with the per-agent buffer (glue 2)",
    12: "k_flow_envb, fused",
}
_SMALL = (3, 2)
# path -> members: (suffix, farm, inflow, hooks, multi, sets)
_MEMBERS = {
    1: [("", _SMALL, "None", {"flow_env": 0}, False, "ABCD")],
    2: [("", _SMALL, "Random", {}, False, ("A", "B", "C", "D", "C2"))],
    3: [("", _SMALL, "box", {"flow_env": 0}, False, ("A", "B", "C", "D", "C2"))],
    4: [("", _SMALL, "None", {"sums": 0, "flow_env": 0}, False, "ABCD")],
    5: [("-36", (6, 6), "None", {}, False, "ABCD"), ("-20", (5, 4), "None", {"flow_env": 0}, False, "A")],
    6: [("", "hr", "None", {}, False, "ABCD")],
    7: [("", _SMALL, "None", {"env_wpe": 1}, False, "ABCD")],
    8: [("", _SMALL, "None", {"env_wpe": 2}, False, "ABCD")],
    9: [("-pass1", (4, 4), "None", {"env_split": 1}, False, "AC"), ("-pass2", (4, 4), "None", {"env_split": 2}, False, "BD")],
    10: [("", _SMALL, "None", {"step_fused": 0}, False, "ABCD")],
    11: [("", _SMALL, "None", {}, True, "ABCD")],
    # (four waves per env exist with two farms only: wg_plan_envb)
    12: [("-w1", _SMALL, "box", {"env_wpe": 1}, False, "B"), ("-w2", _SMALL, "box", {"env_wpe": 2}, False, ("C", "D", "C2")),
         ("-w4", _SMALL, "box", {"env_wpe": 4}, False, "A")],
}


def _mk(name, path, farm, inflow, rules, set_name="", hooks=None, multi=False, steps=None, extra_inc=False):
    return Case(name, path, farm, inflow, tuple(sorted(rules_of(rules).items())), set_name, tuple(sorted((hooks or {}).items())), multi,
                FARMS[farm][3] if steps is None else steps, extra_inc)


def _cases():
    out = []
    for path, members in _MEMBERS.items():
        for suffix, farm, inflow, hooks, multi, sets in members:
            for s in sets:
                out.append(_mk(f"p{path}{suffix}-{s}", path, farm, inflow, SETS[s], s, hooks, multi))
    # ---- extra cases
    # the last fused Power_avg is 64 (set D), the first unfused one 65: the default plan on the small farm
    out.append(_mk("x-baseline-avg65", 10, _SMALL, "None", dict(Power_avg=65)))
    # Power_diff with a deque as long as a wave, fused; and longer than a wave (the deque walk's second trip over the lanes), unfused
    out.append(_mk("x-diff-avg64", 8, _SMALL, "None", dict(Power_reward="Power_diff", Power_avg=64), hooks={"env_wpe": 2}, steps=110))
    out.append(_mk("x-diff-avg100", 10, _SMALL, "None", dict(Power_reward="Power_diff", Power_avg=100), steps=160))
    # Change 0.05 under a reward of order one (set B's is in watts) at 20, 36 and 80 turbines: with set A's Total 0.05 the wave-sum
    # and loop branches of the penalty and power sums
    out.append(_mk("x-change-20", 5, (5, 4), "None", dict(action_penalty=0.05), hooks={"flow_env": 0}))
    out.append(_mk("x-change-36", 5, (6, 6), "None", dict(action_penalty=0.05)))
    out.append(_mk("x-change-80", 6, "hr", "None", dict(action_penalty=0.05)))
    # a deque of one entry, Change 0.05
    out.append(_mk("x-avg1-change", 8, _SMALL, "None", dict(Power_avg=1, action_penalty=0.05), hooks={"env_wpe": 2}))
    # set C on the double clock
    out.append(_mk("x-C-extra-inc", 11, _SMALL, "None", SETS["C"], "C", multi=True, extra_inc=True))
    return out


CASES = _cases()
assert len(CASES) <= 60 and len({c.name for c in CASES}) == len(CASES)


def case(name):
    return next(c for c in CASES if c.name == name)


# ---- which path a case runs, from the plan ---------------------------------------------------------------------------------------
def plan_of(shim, cs):
    cfg = cs.cfg()
    return shim(cfg, box_cells=vc.box_cells(cfg), **dict(cs.hooks))


def path_of(cs, plan):
    """The number of PATHS a case's step() takes (wg_api.hip launch_step), from the config and the plan; None: none of the twelve."""
    c = cs.cfg().to_c()
    inflow, N = vc.inflow_of(c), c.n_turb
    if plan["path_envw"]:
        if inflow == "None":
            if not plan["path_fused"]:
                return 10 if plan["sums_mode"] else None
            if cs.multi:
                return 11
            if plan["env_wpe"] != 2:
                return 7
            return 9 if plan["env_split"] in (1, 2) else 8
        return 12 if plan["path_fused"] and not cs.multi else None
    if not plan["sums_mode"]:
        return 4
    if inflow != "None":
        return {"Random": 2, "box": 3}[inflow] if (plan["block"], plan["res"]) == (64, 1) else None
    if N > 64:
        return 6 if plan["block"] == 256 else None
    if N > 16:
        return 5
    return 1 if (plan["block"], plan["res"]) == (64, 1) else None


def variant_of(plan):
    """what flow_variant() of the handle must say"""
    return (plan["block"], bool(plan["res"]), 2 if plan["path_envw"] else 0)


# ---- bars: the project's own (tests/test_gpu_parity.py, tests/variant_census.py) ---------------------------------------------------
YAW_AGENT_ATOL = 1e-4                       # deg (test_gpu_parity.py)
YAW_BASE_STEADY_ATOL = 2e-4                 # deg (test_hip_glue_matches_reference_golden)
POWER_BAR = dict(rtol=2e-4, atol=20.0)      # W per turbine (_compare_step)
METRICS_BAR = dict(rtol=2e-3, atol=1e-2)    # (test_gpu_parity.py's comparison of metrics() after rollovers)


def yaw_base_bar(cs):
    return dict(rtol=0.0, atol=YAW_BASE_STEADY_ATOL) if cs.inflow == "None" else dict(vc.YAW_BASE_BAR)


def reward_bar(cs, ref):
    """(rtol, atol) of a case's reward against the trajectory `ref` of its own config"""
    r = dict(cs.rules)
    mode, ps = r["Power_reward"], r["Power_scaling"]
    if mode in ("Baseline", "Power_avg"):       # linear in the scaling
        b = dict(rtol=1e-4, atol=2e-4) if cs.inflow == "None" else dict(vc.REWARD_BAR)
        return dict(rtol=b["rtol"], atol=b["atol"] * max(1.0, ps))
    if mode == "None":                          # minus the penalty, a function of the yaws alone
        if cs.penalty_state == "off":
            return dict(rtol=0.0, atol=0.0)
        if cs.penalty_state == "Change":        # two yaws at the yaw bar
            return dict(rtol=0.0, atol=r["action_penalty"] * 2.0 * YAW_AGENT_ATOL)
        return dict(rtol=0.0, atol=r["action_penalty"] * YAW_AGENT_ATOL / float(cs.cfg().yaw_max))
    # Power_diff, in watts: two deque means, each within the power bar per turbine, divided by N
    P = float(np.max(ref["power_turb_agent"]))
    return dict(rtol=0.0, atol=2.0 * (POWER_BAR["rtol"] * P + POWER_BAR["atol"]) * ps)


def misses(got, want, rtol, atol):
    """per entry: |got - want| beyond atol + rtol |want|; an entry that is NaN on one side only misses, NaN on both does not"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
        return np.where(both_nan, False, ~(d <= atol + rtol * np.abs(want)))


# ---- the oracle's side of a case ---------------------------------------------------------------------------------------------------
def seeds_of(cs):
    return 4100 + np.arange(FARMS[cs.farm][0])


def actions_of(cs, **override):
    """The census' action stream (default_rng(19), uniform in [-1, 1)).  Under "wind" the first and the last turbine of every env
    are pinned at +PIN / -PIN: a target of yaw_min + (a + 1) / 2 (yaw_max - yaw_min) beyond the stops.  For an action inside
    [-1, 1] the rate-limited step lies between the old yaw and a target inside the stops, so the [yaw_min, yaw_max] clip of the
    "wind" rule never binds; pinned turbines walk to a stop at yaw_step per step and stay there, where it does."""
    B, N = FARMS[cs.farm][0], cs.cfg().n_turb
    a = np.random.default_rng(19).uniform(-1, 1, size=(cs.steps, B, N)).astype(np.float32)
    if cs.rule(**override)["ActionMethod"] == "wind":
        a[:, :, 0], a[:, :, N - 1] = PIN, -PIN
    return a


def install(cs, side):
    if cs.inflow == "box":
        side.set_turbulence_box(vc.mann_box(), vc.BOX_SPACING)


def reference(oracle_lib, cs, precision="f64", **override):
    """The oracle's trajectory of a case: reset on seeds_of, step on actions_of(cs) — the CASE's actions, also where `override`
    replaces a rule setting (the CPU controls: one rule replaced, everything else as the device will see it).  Every step:
    obs, reward, truncated, final obs, per-agent obs, yaw_agent, power_turb_agent, and yaw_base with two farms; metrics() at the end."""
    cfg = cs.cfg(**override)
    orc = oracle_lib.Oracle(cfg, precision=precision)
    install(cs, orc)
    acts = actions_of(cs)
    two = cfg.to_c().n_farms == 2
    keys = ("obs", "multi", "rew", "tr", "fin", "yaw_agent", "power_turb_agent") + (("yaw_base",) if two else ())
    out = {k: [] for k in keys}
    obs0, multi0 = orc.reset(seeds=seeds_of(cs)), orc.obs_multi()
    for k in range(cs.steps):
        obs, rew, tr, fin = orc.step(acts[k])
        out["obs"].append(obs), out["rew"].append(rew), out["tr"].append(tr), out["fin"].append(fin), out["multi"].append(orc.obs_multi())
        out["yaw_agent"].append(orc.info("yaw_agent")), out["power_turb_agent"].append(orc.info("power_turb_agent"))
        if two:
            out["yaw_base"].append(orc.info("yaw_base"))
    out = {k: np.stack(v) for k, v in out.items()}
    out.update(obs0=obs0, multi0=multi0, metrics=orc.metrics(), actions=acts)
    orc.close()
    for v in out.values():
        v.setflags(write=False)
    return out
