"""Census of the step kernels' instantiations: every kernel the three launch tables build (wg_flow.hip launch_row, wg_env.hip
env_kernel, wg_envb.hip envb_kernel), restated by hand, and a table of small cases that between them make step() launch each
one.  tests/test_variant_census.py pins on the CPU that the cases reach all of ALL_KEYS (through the plan of
tests/plan_shim.cpp); tests/test_gpu_variant_census.py runs every case by value against the oracle.

The cases fix the task rules at env1_config's (Baseline reward, Power_avg 10, Power_scaling 1, no action penalty, Local
controller), with the "yaw" action; tests/rule_cases.py varies them on every step path.

A new template axis of a step kernel adds its values to the key tuples below and a case per new instantiation to CASES."""
import itertools
from dataclasses import dataclass

import numpy as np

from windgym_amd import presets
from windgym_amd.binding import HOOK_ENV  # noqa: F401  (plan hook name -> WG_* variable: Case.hooks)
from windgym_amd.config import EnvConfig
from windgym_amd.turbine import V80

# ---- the 74 instantiations ---------------------------------------------------------------------------------------------------------
# k_flow<NT, TURB, REPLAY, NOISE, RES, SGM>:  ("k_flow", threads, compact, inflow, replay, noise, deficit_model)
#   replay ignores the physics: launch_row builds it on inflow None / deficit model 0 only
INFLOWS = ("None", "Random", "box")
K_FLOW_KEYS = (
    # 64 threads, compact rings: inflow x noise x deficit model, + replay x noise
    [("k_flow", 64, True, i, False, n, dm) for i in INFLOWS for n in (False, True) for dm in (0, 1, 2)]
    + [("k_flow", 64, True, "None", True, n, 0) for n in (False, True)]
    # 256 threads, compact rings (large steady farms): noise x deficit model, + replay x noise
    + [("k_flow", 256, True, "None", False, n, dm) for n in (False, True) for dm in (0, 1, 2)]
    + [("k_flow", 256, True, "None", True, n, 0) for n in (False, True)]
    # 256 threads, uniform rings: inflow x noise, + replay x noise
    + [("k_flow", 256, False, i, False, n, 0) for i in INFLOWS for n in (False, True)]
    + [("k_flow", 256, False, "None", True, n, 0) for n in (False, True)])
# k_flow_env<NOISE, GLUE, WPE, SPLIT>:  ("k_flow_env", noise, glue, waves, pass_waves); pass waves exist with a glue tail and two waves only
K_FLOW_ENV_KEYS = (
    [("k_flow_env", n, 0, w, 0) for n in (False, True) for w in (1, 2)]
    + [("k_flow_env", n, g, w, s) for n in (False, True) for g in (1, 2) for w, s in ((1, 0), (2, 0), (2, 1), (2, 2))])
# k_flow_envb<NOISE, GLUE, WPE>:  ("k_flow_envb", noise, glue, waves)
K_FLOW_ENVB_KEYS = [("k_flow_envb", n, g, w) for n in (False, True) for g in (0, 1, 2) for w in (1, 2, 4)]
ALL_KEYS = K_FLOW_KEYS + K_FLOW_ENV_KEYS + K_FLOW_ENVB_KEYS

# Keys no config and hook brings the plan to select, with the evidence from the shim: none.  (A key listed here is left out of
# the equality test_variant_census.py asserts, nothing else.)
UNREACHABLE = {}

BOX_DIMS, BOX_SPACING, BOX_SEED = (256, 64, 32), (3.0, 3.0, 3.0), 1234      # the Mann box of tests/test_gpu_parity.py


# ---- config builders ---------------------------------------------------------------------------------------------------------------
class AllChannelNoiseConfig(EnvConfig):
    """Sensor noise on all four channels (ws, wd, yaw, power): EnvConfig.to_c() writes the reference's (0, 2, 0, 0) only, the
    kernels unroll over wg_config.noise_sigma[WG_N_CH].  Sigmas of the order of each channel's own step-to-step variation."""
    SIGMA = (0.3, 2.0, 0.5, 2.0e4)      # m/s, deg, deg, W

    def to_c(self):
        c = super().to_c()
        for i, s in enumerate(self.SIGMA):
            c.noise_sigma[i] = s
        return c


def _yaml(noise, nx, ny, ti=False, all_channels=False):
    d = presets._upd(presets.env1_config(), ActionMethod="yaw", noise="Normal" if noise else "None", farm=dict(nx=nx, ny=ny),
                     mes_level=dict(turb_wd=True, turb_TI=ti), wd_mes=dict(wd_current=True, wd_rolling_mean=True))
    if all_channels:
        d = presets._upd(d, mes_level=dict(turb_power=True), ws_mes=dict(ws_current=True), yaw_mes=dict(yaw_current=True),
                         power_mes=dict(power_current=True, power_rolling_mean=True))
    return d


def small(inflow="None", noise=False, ti=False, autoreset=True, all_channels=False):
    """3 x 2 turbines, two farms, B = 5 (odd), 16 rotor points; wd observed as current + rolling mean so that the noised channel
    reaches the observation.  Without TI entries the config stays "non-generic" (sums mode, no farm-level entries): a handle on
    an env kernel runs the fused step.  n_passthrough 0.25: episodes of 16 to 39 steps (dist 960 .. 1090 m, ws 7 .. 15 m/s)."""
    cls = AllChannelNoiseConfig if all_channels else EnvConfig
    return cls(turbine=V80(), yaml_dict=_yaml(noise, 3, 2, ti, all_channels), turbtype={"box": "MannGenerate"}.get(inflow, inflow), n_envs=5,
               autoreset=autoreset, n_passthrough=0.25, n_rotor_pts=16)


def cfg2_farm(noise=False, all_channels=False):
    """The 4 x 4 farm of bench cfg2 at B = 5: a farm's pass is four trips or more, where pass waves make sense.  n_passthrough 0.2:
    episodes of 17 to 44 steps (dist 1280 .. 1570 m)."""
    cls = AllChannelNoiseConfig if all_channels else EnvConfig
    return cls(turbine=V80(), yaml_dict=_yaml(noise, 4, 4, False, all_channels), turbtype="None", n_envs=5, autoreset=True, n_passthrough=0.2,
               n_rotor_pts=16)


def large(noise=False, autoreset=True):
    """6 x 6 = 36 turbines (N > 32), steady, B = 2, 8 rotor points: the 256-thread compact row.  n_passthrough 0.2: episodes of
    25 to 67 steps (dist 1920 .. 2350 m)."""
    return EnvConfig(turbine=V80(), yaml_dict=_yaml(noise, 6, 6), turbtype="None", n_envs=2, autoreset=autoreset, n_passthrough=0.2,
                     n_rotor_pts=8)


def deficit(model, inflow="None", noise=False, nxy=3):
    """The config of tests/test_super_gaussian.py / tests/test_ainslie.py (6 D x 4 D grid, ws 10 m/s, TI 8 %, wd 255 .. 285) with the
    noise switch, wd observed, autoreset on and short episodes: dist 1440 .. 1600 m (3 x 3) / 2880 .. 3280 m (6 x 6) at 10 m/s,
    n_passthrough 0.2 / 0.1 -> 28 .. 32 steps."""
    d = _yaml(noise, nxy, nxy)
    d["farm"].update(xDist=6, yDist=4)
    d["wind"] = dict(ws_min=10.0, ws_max=10.0, wd_min=255.0, wd_max=285.0, TI_min=0.08, TI_max=0.08)
    d["yaw_init"] = "Zeros"
    return EnvConfig(turbine=V80(), yaml_dict=d, turbtype={"box": "MannFixed"}.get(inflow, inflow), n_envs=3 if nxy == 3 else 2, autoreset=True,
                     n_passthrough=0.2 if nxy == 3 else 0.1, n_rotor_pts=16 if nxy == 3 else 8, deficit={1: "super_gaussian", 2: "ainslie"}[model])


BUILDERS = {"small": small, "cfg2_farm": cfg2_farm, "large": large, "deficit": deficit}


@dataclass(frozen=True)
class Case:
    name: str
    builder: str                # key of BUILDERS
    kw: tuple = ()              # its keyword arguments, as sorted (name, value) pairs
    hooks: tuple = ()           # (plan hook name, value) pairs: the WG_* hooks the handle is created under (HOOK_ENV)
    script: bool = False        # a flow script is installed (replay mode)
    multi: bool = False         # the per-agent buffer is registered (fuse_obs_multi())
    steps: int = 80

    def cfg(self):
        return BUILDERS[self.builder](**dict(self.kw))

    @property
    def ref_id(self):
        """cases with equal ref_id share one oracle trajectory (the hooks and the per-agent buffer are the handle's business)"""
        return (self.builder, self.kw, self.script, self.steps)


def _case(name, builder, hooks=None, script=False, multi=False, steps=80, **kw):
    import inspect
    dflt = {k: v.default for k, v in inspect.signature(BUILDERS[builder]).parameters.items()}
    kw = {k: v for k, v in kw.items() if dflt[k] != v}      # (equal configs get equal ref_ids)
    return Case(name, builder, tuple(sorted(kw.items())), tuple(sorted((hooks or {}).items())), script, multi, steps)


def _cases():
    out = []
    nz = {False: "", True: "-noise"}
    for n in (False, True):
        # ---- k_flow, 64 threads compact
        out.append(_case(f"flow64-None{nz[n]}", "small", {"flow_block": 64}, noise=n))
        out.append(_case(f"flow64-Random{nz[n]}", "small", inflow="Random", noise=n))
        out.append(_case(f"flow64-box{nz[n]}", "small", {"flow_block": 64}, inflow="box", noise=n))
        for dm, i in itertools.product((1, 2), INFLOWS):
            out.append(_case(f"flow64-{i}-dm{dm}{nz[n]}", "deficit", steps=66, model=dm, inflow=i, noise=n))
        out.append(_case(f"flow64-replay{nz[n]}", "small", script=True, steps=60, noise=n, autoreset=False))
        # ---- k_flow, 256 threads compact (N > 32, steady)
        out.append(_case(f"flow256c-None{nz[n]}", "large", steps=130, noise=n))
        for dm in (1, 2):
            out.append(_case(f"flow256c-None-dm{dm}{nz[n]}", "deficit", steps=66, model=dm, noise=n, nxy=6))
        out.append(_case(f"flow256c-replay{nz[n]}", "large", script=True, steps=90, noise=n, autoreset=False))
        # ---- k_flow, 256 threads uniform rings (by hook on the small farm)
        for i in INFLOWS:
            out.append(_case(f"flow256u-{i}{nz[n]}", "small", {"flow_block": 256}, inflow=i, noise=n))
        out.append(_case(f"flow256u-replay{nz[n]}", "small", {"flow_block": 256}, script=True, steps=60, noise=n, autoreset=False))
        # ---- k_flow_env: glue 0 through a generic observation (turb_TI), glue 1 fused, glue 2 fused + per-agent buffer
        for w in (1, 2):
            out.append(_case(f"env-g0-w{w}{nz[n]}", "small", {"env_wpe": w}, noise=n, ti=True))
            for g in (1, 2):
                out.append(_case(f"env-g{g}-w{w}{nz[n]}", "small", {"env_wpe": w}, multi=g == 2, noise=n))
        for g, s in itertools.product((1, 2), (1, 2)):
            out.append(_case(f"env-g{g}-w2-pass{s}{nz[n]}", "cfg2_farm", {"env_split": s}, multi=g == 2, steps=90, noise=n))
        # ---- k_flow_envb
        for w in (1, 2, 4):
            out.append(_case(f"envb-g0-w{w}{nz[n]}", "small", {"env_wpe": w}, inflow="box", noise=n, ti=True))
            for g in (1, 2):
                out.append(_case(f"envb-g{g}-w{w}{nz[n]}", "small", {"env_wpe": w}, multi=g == 2, inflow="box", noise=n))
    # ---- noise on all four channels, one case per kernel family
    out.append(_case("flow64-box-noise4", "small", {"flow_block": 64}, inflow="box", noise=True, all_channels=True))
    out.append(_case("env-g1-w2-pass2-noise4", "cfg2_farm", {"env_split": 2}, steps=90, noise=True, all_channels=True))
    out.append(_case("envb-g2-w2-noise4", "small", {"env_wpe": 2}, multi=True, inflow="box", noise=True, all_channels=True))
    return out


CASES = _cases()
# one negative control per kernel family (tests/test_gpu_variant_census.py): the oracle on seeds shifted by one
CONTROLS = ("flow64-box-noise", "env-g1-w2-noise", "envb-g1-w2-noise")


def case(name):
    return next(c for c in CASES if c.name == name)


def inflow_of(c_cfg):
    return "None" if c_cfg.turb_mode == 0 else ("Random" if c_cfg.turb_mode == 1 else "box")


def box_cells(cfg):
    return BOX_DIMS[0] * BOX_DIMS[1] * BOX_DIMS[2] if cfg.to_c().turb_mode >= 2 else 0


def plan_of(shim, cs):
    """the plan tests/plan_shim.cpp returns for the case's config under the case's hooks"""
    cfg = cs.cfg()
    return shim(cfg, box_cells=box_cells(cfg), **dict(cs.hooks))


def key_of(cs, plan):
    """The instantiation a case's step() launches (wg_api.hip launch_step -> wg_launch_flow / wg_launch_step_env[b] -> the launch
    tables), from the config and the plan."""
    c = cs.cfg().to_c()
    noise, inflow = c.noise == 1, inflow_of(c)
    if plan["path_envw"] and not cs.script:      # (a script forces the per-slot kernel: wg_launch_flow)
        glue = 0 if not plan["path_fused"] else (2 if cs.multi else 1)
        if inflow == "None":
            wpe = 2 if plan["env_wpe"] == 2 else 1
            split = plan["env_split"] if glue != 0 and wpe == 2 and plan["env_split"] in (1, 2) else 0
            return ("k_flow_env", noise, glue, wpe, split)
        return ("k_flow_envb", noise, glue, 4 if plan["env_wpe"] == 4 else (2 if plan["env_wpe"] == 2 else 1))
    threads, compact = (plan["block"], True) if plan["res"] else (256, False)
    if cs.script:
        return ("k_flow", threads, compact, "None", True, noise, 0)
    return ("k_flow", threads, compact, inflow, False, noise, c.deficit_model)


# ---- bars: each from the project's test of the nearest un-noised variant (tests/test_gpu_parity.py, test_super_gaussian.py) ----------
OBS_ATOL, DEFICIT_OBS_ATOL, TURB_OBS_ATOL = 2e-4, 3e-4, 5e-4
REWARD_BAR = dict(rtol=1e-3, atol=1e-3)
UVW_BAR = dict(rtol=2e-4, atol=2e-3)
YAW_BASE_BAR = dict(rtol=0.0, atol=2e-2)


def obs_atol(cs):
    c = cs.cfg().to_c()
    if c.noise == 1 or c.turb_mode != 0:
        return TURB_OBS_ATOL
    return DEFICIT_OBS_ATOL if c.deficit_model != 0 else OBS_ATOL


# ---- the oracle's side of a case ---------------------------------------------------------------------------------------------------
_BOX = []


def mann_box():
    if not _BOX:
        from windgym_amd.mann import generate_mann_box
        _BOX.append(generate_mann_box(BOX_DIMS, BOX_SPACING, seed=BOX_SEED))
    return _BOX[0]


def seeds_of(cs):
    return 4100 + np.arange(cs.cfg().n_envs)


def flow_script(cs):
    """Synthetic replay tables uvw [F, T, B, N, 3] / power [F, T, B, N]: random (u, v, w) around the ambient wind and random powers,
    fixed seed.  Long enough that no cursor reaches the last row (an episode consumes its fill, 25 rows, and its steps)."""
    cfg = cs.cfg()
    rng = np.random.default_rng(77)
    T, B, N = 12 * 25 + 2 * cs.steps, cfg.n_envs, cfg.n_turb
    uvw = np.stack([rng.uniform(6.0, 12.0, (2, T, B, N)), rng.normal(0.0, 0.6, (2, T, B, N)), rng.normal(0.0, 0.3, (2, T, B, N))], axis=-1)
    power = rng.uniform(2.0e5, 1.8e6, (2, T, B, N))
    return np.ascontiguousarray(uvw.astype(np.float32)), np.ascontiguousarray(power.astype(np.float32))


def install(cs, side):
    """the same box or flow script on a HipBatch or an Oracle (the deficit table: both install ainslie.deficit_table() themselves)"""
    cfg = cs.cfg()
    if cfg.to_c().turb_mode >= 2:
        side.set_turbulence_box(mann_box(), BOX_SPACING)
    if cs.script:
        side.set_flow_script(*flow_script(cs))


def actions_of(cs):
    cfg = cs.cfg()
    return np.random.default_rng(19).uniform(-1, 1, size=(cs.steps, cfg.n_envs, cfg.n_turb)).astype(np.float32)


FLOW_CHECK_EVERY = 20


def reference(oracle_lib, cs, seed_shift=0, steps=None, noise=None):
    """The oracle's trajectory of a case: reset on seeds_of (+ seed_shift), step on actions_of; every step's observation, per-agent
    observation, reward, flag and final observation, rotor_uvw_agent / yaw_base every FLOW_CHECK_EVERY steps.  A handle without
    autoreset (the replay cases: the device keeps a script cursor per context) resets its truncated envs after the step; their
    rows of the reset's observation replace the step's.  noise=False: the same config with the sensor noise off."""
    kw = dict(cs.kw)
    if noise is not None:
        kw["noise"] = noise
    cfg = BUILDERS[cs.builder](**kw)
    orc = oracle_lib.Oracle(cfg)
    install(cs, orc)
    acts = actions_of(cs)
    out = dict(obs0=orc.reset(seeds=seeds_of(cs) + seed_shift), multi0=orc.obs_multi(), obs=[], multi=[], rew=[], tr=[], fin=[], uvw={}, yaw_base={})
    for k in range(cs.steps if steps is None else steps):
        obs, rew, tr, fin = orc.step(acts[k])
        if not cfg.autoreset and tr.any():
            obs = obs.copy()
            obs[tr] = orc.reset(mask=tr.astype(np.uint8))[tr]
        out["obs"].append(obs), out["rew"].append(rew), out["tr"].append(tr), out["fin"].append(fin), out["multi"].append(orc.obs_multi())
        if k % FLOW_CHECK_EVERY == 0:
            out["uvw"][k], out["yaw_base"][k] = orc.info("rotor_uvw_agent"), orc.info("yaw_base")
    orc.close()
    return out
