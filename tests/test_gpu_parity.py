"""GPU parity tests (run with -m gpu on the MI355X box): the HIP path, called through the C ABI, against
  (a) the golden vectors recorded from the reference's glue (replay mode),
  (b) the fp64 oracle of model M0 on the same seeds and actions.

Stated fp32 tolerances: scaled observations |d| <= 2e-4, reward |d| <= 2e-4 (+1e-4 rel),
yaw |d| <= 1e-4 deg, rotor wind speed rel 1e-4, power rel 2e-4 (+20 W).
"""
import numpy as np
import pytest

from helpers import (BLOCKS, OBS_ATOL, config_from_meta, golden_cases, hip, load_golden, make_batch, make_env, physics_cfg,  # noqa: F401  (hip: the fixture)
                     script_tables, turb_cfg)

pytestmark = pytest.mark.gpu


# "env" = k_flow_env, one or two waves per env with lane = farm slot x turbine (small farms: what cfg2 / cfg4 run);
# "env1" = the same kernel forced to ONE wave per env (WG_ENV_WPE=1: what a batch of more than 2048 envs runs — the headline)
STEADY_BLOCKS = BLOCKS + ["env", "env1"]
# frozen-box inflow: the per-slot instantiations and "envb" = k_flow_envb (wg_envb.hip), the one-launch env kernel cfg5 runs
BOX_BLOCKS = BLOCKS + ["envb4", "envb", "envb1"]      # (four waves per env = one per farm slot: hook only, WG_ENV_WPE=4; two: what cfg5 x 1024 runs; one)


def _t(hip, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


@pytest.mark.parametrize("name", golden_cases())
@pytest.mark.parametrize("n_envs", [1, 5])
def test_hip_glue_matches_reference_golden(hip, name, n_envs):
    g, meta = load_golden(name)
    cfg = config_from_meta(meta, n_envs=n_envs)
    env = hip.HipBatch(cfg)
    uvw, pw = script_tables(g, n_envs)
    env.set_flow_script(uvw, pw)
    n_ep = len(g["ep_start"])
    step = 0
    for ep in range(n_ep):
        obs0 = env.reset(seeds=[meta["seed"]] * n_envs if ep == 0 else None).cpu().numpy()
        env.check()
        assert np.allclose(env.info("ws_global").cpu().numpy(), g["ws"][ep], rtol=1e-7)
        # the sampled (ws, wd, ti) in double precision are BIT-identical to what the reference drew from np_random
        w64 = env.info("wind_f64").cpu().numpy()
        assert w64.dtype == np.float64
        for b in range(n_envs):
            assert w64[b, 0] == g["ws"][ep] and w64[b, 1] == g["wd"][ep] and w64[b, 2] == g["ti"][ep], (w64[b], ep)
        assert np.all(env.info("time_max").cpu().numpy() == int(g["time_max"][ep]))
        np.testing.assert_allclose(env.info("yaw_agent").cpu().numpy()[0], g["yaw_init"][ep], atol=1e-5)
        for b in range(n_envs):
            np.testing.assert_allclose(obs0[b], g["obs0"][ep], rtol=0, atol=OBS_ATOL)
        if meta["multi"]:
            om = env.obs_multi().cpu().numpy()
            np.testing.assert_allclose(om[n_envs - 1], g["obs_multi0"][ep], rtol=0, atol=OBS_ATOL)
        end = g["ep_start"][ep + 1] if ep + 1 < n_ep else len(g["action"])
        while step < end:
            a = np.repeat(g["action"][step][None], n_envs, axis=0)
            obs, rew, tr, _ = env.step(_t(hip, a))
            obs, rew, tr = obs.cpu().numpy(), rew.cpu().numpy(), tr.cpu().numpy()
            b = n_envs - 1
            assert bool(tr[b]) == bool(g["truncated"][step]), step
            np.testing.assert_allclose(rew[b], g["reward"][step], rtol=1e-4, atol=OBS_ATOL, equal_nan=True)
            if meta["multi"]:
                np.testing.assert_allclose(env.obs_multi().cpu().numpy()[b], g["obs_multi"][step], rtol=0, atol=OBS_ATOL)
            else:
                np.testing.assert_allclose(obs[b], g["obs"][step], rtol=0, atol=OBS_ATOL, err_msg=f"step {step}")
            if not g["truncated"][step]:
                np.testing.assert_allclose(env.info("yaw_agent").cpu().numpy()[b], g["yaw"][step], atol=1e-4)
                if meta["two_farms"]:
                    np.testing.assert_allclose(env.info("yaw_base").cpu().numpy()[b], g["yaw_base"][step], atol=2e-4)
            step += 1
    env.check()
    env.close()


def _compare_step(env, orc, a, step, check_flow=True, power_rtol=2e-4):
    import torch
    obs, rew, tr, fin = env.step(torch.as_tensor(a, device="cuda"))
    o_obs, o_rew, o_tr, o_fin = orc.step(a)
    np.testing.assert_array_equal(tr.cpu().numpy().astype(bool), o_tr, err_msg=f"step {step}")
    np.testing.assert_allclose(obs.cpu().numpy(), o_obs, rtol=0, atol=OBS_ATOL, err_msg=f"obs step {step}")
    np.testing.assert_allclose(fin.cpu().numpy(), o_fin, rtol=0, atol=OBS_ATOL, err_msg=f"final obs step {step}")
    np.testing.assert_allclose(rew.cpu().numpy(), o_rew, rtol=1e-4, atol=OBS_ATOL, err_msg=f"reward step {step}")
    if check_flow:
        np.testing.assert_allclose(env.info("yaw_agent").cpu().numpy(), orc.info("yaw_agent"), atol=1e-4)
        np.testing.assert_allclose(env.info("rotor_uvw_agent").cpu().numpy(), orc.info("rotor_uvw_agent"),
                                   rtol=1e-4, atol=1e-4, err_msg=f"rotor wind step {step}")
        np.testing.assert_allclose(env.info("power_turb_agent").cpu().numpy(), orc.info("power_turb_agent"),
                                   rtol=power_rtol, atol=20.0, err_msg=f"power step {step}")
        np.testing.assert_allclose(env.info("rotor_uvw_base").cpu().numpy(), orc.info("rotor_uvw_base"),
                                   rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("block", STEADY_BLOCKS)
def test_hip_physics_matches_oracle_step_for_step(hip, oracle_lib, block):
    """cfg2-shaped farm (4x4, yaw action, two farms), B=6, 300 steps on identical seeds and actions — in each of the
    per-slot instantiations of k_flow a small farm can run (64 threads: the compact single-wave kernel, on whose state cfg2 / cfg4's
    env kernel runs; 256: uniform rings) and in that env kernel at two waves and one wave per env."""
    B = 6
    cfg = physics_cfg(B, autoreset=False, n_passthrough=5)
    env, orc = make_env(hip, cfg, block), oracle_lib.Oracle(cfg)
    seeds = 1234 + np.arange(B)
    obs0 = env.reset(seeds=seeds).cpu().numpy()
    o0 = orc.reset(seeds=seeds)
    env.check()
    for k in ("ws_global", "wd_global", "ti_global"):
        np.testing.assert_allclose(env.info(k).cpu().numpy(), orc.info(k), rtol=1e-7)
    np.testing.assert_array_equal(env.info("time_max").cpu().numpy(), orc.info("time_max").astype(int))
    np.testing.assert_allclose(env.info("turb_x").cpu().numpy(), orc.info("turb_x"), rtol=1e-6, atol=1e-3)
    np.testing.assert_allclose(obs0, o0, rtol=0, atol=OBS_ATOL)
    np.testing.assert_allclose(env.info("rotor_uvw_agent").cpu().numpy(), orc.info("rotor_uvw_agent"), rtol=1e-4, atol=1e-4)
    rng = np.random.default_rng(0)
    for step in range(300):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        _compare_step(env, orc, a, step)
    env.check()
    # downstream rows are waked (the invariant the reference left commented out, tests/test_basics.py:299-311)
    u = env.info("rotor_uvw_agent").cpu().numpy()[..., 0]
    x = env.info("turb_x").cpu().numpy()
    ws = env.info("ws_global").cpu().numpy()
    for b in range(B):
        up = x[b] <= x[b].min() + 1.0
        assert np.allclose(u[b][up], ws[b], rtol=1e-5)
        assert u[b][~up].mean() < ws[b]


EDGE_CASES = {
    # name: (nx, ny, kwargs of EnvConfig, yaml overrides)      -- shapes / code paths the BASELINE configs do not hit
    "single_turbine": (1, 1, dict(n_rotor_pts=16), {}),                          # N = 1: truncates at the first step
    "row_of_3_S1": (3, 1, dict(n_rotor_pts=1), {}),                              # one rotor point, ny = 1 -> y = 0
    "grid_5x3_S7": (5, 3, dict(n_rotor_pts=7), {}),                              # S not a power of two (S_pad = 8)
    "max_128_turbines": (16, 8, dict(n_rotor_pts=4, n_particles=64), {}),        # N = 128: 4 mask words, chunked targets
    "short_ring_P16": (2, 2, dict(n_rotor_pts=16, n_particles=16), {}),          # chain shorter than the farm
    "substeps_dt3": (3, 2, dict(n_rotor_pts=16, dt_sim=1, dt_env=3), {}),        # K = 3 sub-steps per env step
    "half_second_dt": (2, 2, dict(n_rotor_pts=16, dt_sim=0.5, dt_env=1), {}),    # dt_sim = 0.5 s, K = 2
    # single-wave GL variant of k_flow (LDS-DMA gathers): 30 turbines in 5 rows of 6 -> 75 in-row pairs alone, i.e. more
    # than one batch of 64 candidates (the second batch lands in the same LDS words)
    "dense_6x5_two_candidate_batches": (6, 5, dict(n_rotor_pts=16), {"farm": dict(xDist=3, yDist=2)}),
    # turbines 0.1 D apart along the wind: closer than the particle spacing (0.2 D), so the bracketing particles of the pair
    # are released in the very step that evaluates them (the turbine's record in LDS, not in memory yet) and the pair is
    # a candidate before the chain's bounds know the new record
    "near_pair_released_this_step": (3, 1, dict(n_rotor_pts=16), {"farm": dict(xDist=0.1, yDist=3)}),
}


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_edge_shapes_match_oracle(hip, oracle_lib, case):
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    nx, ny, kw, over = EDGE_CASES[case]
    _, meta = load_golden("env1")
    d = meta["cfg"]
    d["farm"].update(nx=nx, ny=ny)
    d["ActionMethod"] = "yaw"
    d["mes_level"].update(turb_wd=True, turb_power=True, farm_ws=True, farm_power=True)
    for k, v in over.items():
        d[k].update(v)
    B = 4
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=B, autoreset=True, n_passthrough=1, **kw)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    seeds = 77 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(5)
    n_tr = 0
    steps = 60 if case == "max_128_turbines" else 160
    for step in range(steps):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        # (6 x 5 at 3 D spacing: rotors sit in up to five superposed wakes at ~60 % of the free stream; the rotor wind speed
        # holds its 1e-4 bar, the power is its cube on the steep part of the curve -> 4e-4, in every kernel variant alike)
        _compare_step(env, orc, a, step, power_rtol=4e-4 if case.startswith("dense_6x5") else 2e-4)
        n_tr += int(orc.info("timestep").min() == 0)
    env.check()
    if case == "single_turbine":
        assert n_tr == steps                         # x_max - x_min = 0 -> time_max = 0 (Wind_Farm_Env.py:723-732)


@pytest.mark.parametrize("block", ["env", "env1"])
def test_one_step_episodes_on_the_env_kernel(hip, oracle_lib, block):
    """episodes of ONE step (N = 1: x_max - x_min = 0 -> time_max = 0) on k_flow_env.  Every step truncates, so the
    context retired by step t must be set up, developed and swapped in by step t + 1's launch: with one wave per env the
    episode set-up may NOT be deferred behind the wave's step when that very step truncates (it was: lean_swap then raised
    WG_STATUS_BIT_STATE and the observation windows were under-filled)."""
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    _, meta = load_golden("env1")
    d = meta["cfg"]
    d["farm"].update(nx=1, ny=1)
    d["ActionMethod"] = "yaw"
    B = 5
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=B, autoreset=True, n_passthrough=1, n_rotor_pts=16)
    env, orc = make_env(hip, cfg, block), oracle_lib.Oracle(cfg)
    seeds = 77 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(5)
    for step in range(60):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        _compare_step(env, orc, a, step)
        assert env.truncated.all()
        env.check()                               # no unready background episode at any swap
    env.close()


def test_lds_fallback_to_uniform_rings_matches_oracle(hip, oracle_lib):
    """A small farm whose compact-variant LDS carve does not fit a workgroup (N = 32, P = 4096: the 16-bit quad list alone
    is 64 KB) must fall back to the uniform-ring variant at wg_create — not fail at the first launch — and still match
    the oracle (the fallback also has to drop the single-wave variant's LDS-DMA layout flags)."""
    B = 2
    cfg = physics_cfg(B, autoreset=True, n_passthrough=0.1, nx=8, ny=4, n_particles=4096)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    block, compact, slots = env.flow_variant()
    assert (block, compact, slots) == (256, False, 0)
    seeds = 5 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(3)
    for step in range(12):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        _compare_step(env, orc, a, step)
    env.check()


def test_nonuniform_turbine_table_matches_oracle(hip, oracle_lib):
    """A power/Ct table on a non-uniform wind-speed grid (the kernel resamples it on 1024 uniform points)."""
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import TabularTurbine, V80
    v = V80()
    ws = np.array([3.0, 3.5, 4.0, 5.0, 6.5, 8.0, 9.0, 10.0, 11.0, 12.5, 14.0, 17.0, 21.0, 25.0])
    turb = TabularTurbine("V80-coarse", v.diameter(), v.hub_height(), ws, v.power(ws), np.interp(ws, v.ws_tab, v.ct_tab))
    _, meta = load_golden("env1")
    d = meta["cfg"]
    d["ActionMethod"] = "yaw"
    B = 3
    cfg = EnvConfig(turbine=turb, yaml_dict=d, turbtype="None", n_envs=B, autoreset=True, n_passthrough=1, n_rotor_pts=16)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    seeds = 9 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(6)
    for step in range(120):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        obs, rew, tr, fin = env.step(__import__("torch").as_tensor(a, device="cuda"))
        o_obs, o_rew, o_tr, o_fin = orc.step(a)
        np.testing.assert_array_equal(tr.cpu().numpy().astype(bool), o_tr)
        # the resampled table differs from the exact piecewise-linear one by O(dx^2) curvature inside a cell: power within
        # 0.5 % of rated, observations within 1e-3
        np.testing.assert_allclose(obs.cpu().numpy(), o_obs, rtol=0, atol=1e-3, err_msg=f"obs step {step}")
        np.testing.assert_allclose(env.info("power_turb_agent").cpu().numpy(), orc.info("power_turb_agent"), rtol=5e-3, atol=1e4)
    env.check()


@pytest.mark.parametrize("block", [None, "env1"])
def test_hip_autoreset_pipeline_matches_oracle(hip, oracle_lib, block):
    """Episodes are short (n_passthrough=1) so every env rolls over several times: the background-developed
    next episode must be identical to the oracle's synchronous reset, at the exact step.  None = the handle's default (two
    waves per env at this batch size); "env1" = ONE wave per env, the variant batches above 2048 envs — the headline — run:
    deferred episode set-up, first observation built a launch later, the swap in the wave's own glue tail."""
    B = 12
    cfg = physics_cfg(B, autoreset=True, n_passthrough=1, nx=3, ny=2)
    env, orc = make_env(hip, cfg, block), oracle_lib.Oracle(cfg)
    seeds = 77 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(1)
    n_trunc = 0
    for step in range(700):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        _compare_step(env, orc, a, step, check_flow=(step % 25 == 0))
        n_trunc += int(env.truncated.sum().item())
    env.check()
    assert n_trunc >= 2 * B
    np.testing.assert_array_equal(env.info("episode").cpu().numpy(), orc.info("episode").astype(int))
    m_gpu, m_cpu = env.metrics().cpu().numpy(), orc.metrics()
    np.testing.assert_allclose(m_gpu, m_cpu, rtol=2e-3, atol=1e-2)


def test_large_odd_batch_with_rollovers_matches_oracle(hip, oracle_lib):
    """B = 389 envs (not a multiple of anything), cfg2-shaped farm, two farms, same-step autoreset with several episode
    rollovers: every batch-size dependent path (block order, context hashing, background scheduling) against the
    oracle, which knows none of them."""
    B = 389
    cfg = physics_cfg(B, autoreset=True, n_passthrough=1)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    seeds = 5000 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(8)
    n_tr = 0
    for step in range(260):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        _compare_step(env, orc, a, step, check_flow=(step % 40 == 0))
        n_tr += int((orc.info("timestep") == 0).sum())
    env.check()
    assert n_tr >= B


def test_partial_reset_and_state_roundtrip(hip, oracle_lib):
    B = 4
    cfg = physics_cfg(B, autoreset=False, n_passthrough=2, nx=2, ny=2)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    seeds = np.array([5, 6, 7, 8], dtype=np.uint64)
    env.reset(seeds=seeds), orc.reset(seeds=seeds)
    rng = np.random.default_rng(2)
    for step in range(40):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        _compare_step(env, orc, a, step, check_flow=False)
    mask = np.array([0, 1, 0, 1], dtype=np.uint8)
    new_seeds = np.array([0, 99, 0, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)   # env 3 keeps its generator
    g_obs = env.reset(seeds=new_seeds, mask=mask).cpu().numpy()
    o_obs = orc.reset(seeds=new_seeds, mask=mask)
    np.testing.assert_allclose(g_obs[mask.astype(bool)], o_obs[mask.astype(bool)], rtol=0, atol=OBS_ATOL)
    blob = env.get_state()
    acts = [rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32) for _ in range(30)]
    ref = []
    for step, a in enumerate(acts):
        _compare_step(env, orc, a, step, check_flow=False)
        ref.append(env.obs.cpu().numpy().copy())
    env.set_state(blob)      # replay from the checkpoint: bit-identical trajectory
    import torch
    for a, r in zip(acts, ref):
        obs, *_ = env.step(torch.as_tensor(a, device="cuda"))
        np.testing.assert_array_equal(obs.cpu().numpy(), r)


def test_step_after_truncation_is_an_error(hip):
    cfg = physics_cfg(1, autoreset=False, n_passthrough=0.05, nx=2, ny=1)
    env = hip.HipBatch(cfg)
    env.reset(seeds=[3])
    import torch
    a = torch.zeros((1, cfg.n_turb), device="cuda")
    for _ in range(200):
        _, _, tr, _ = env.step(a)
        if tr.item():
            break
    assert tr.item()
    env.step(a)
    with pytest.raises(Exception):
        env.check()


@pytest.mark.parametrize("variant", ["uniform_samplemajor", "compact_pairmajor", "compact_pairmajor_small_staging"])
def test_horns_rev_80_turbines_matches_oracle(hip, oracle_lib, variant):
    """BASELINE.json configs[2] at test size: Horns Rev 1 layout (N = 80 > one wave, P = 416, target chunking
    in the deficit phases), B = 3, autoreset on.  "compact_pairmajor" = what bench.py --workload cfg3 runs (compact
    rings, pair-major phases in chunks of targets, 16-byte record gathers, 256 threads: the default for large farms with
    steady inflow); "uniform_samplemajor" = the round-1 large-farm variant (WG_FLOW_RES=0: uniform rings with predicate
    pruning, (target, sample)-major phases), still the one turbulent large farms run.  "..._small_staging": the same
    kernel with room for 96 candidate results at a time (WG_LF_CAP), so that the ~500 candidates of a flow step take six
    rounds through the staging region — same sums in the same order."""
    from windgym_amd.config import EnvConfig
    from windgym_amd.presets import horns_rev1_layout, horns_rev_config
    from windgym_amd.turbine import V80
    x, y = horns_rev1_layout()
    cfg = EnvConfig(turbine=V80(), yaml_dict=horns_rev_config(), turbtype="None", n_envs=3, autoreset=True,
                    n_passthrough=0.2, x_pos=x, y_pos=y)
    assert cfg.n_turb == 80
    hooks = {"WG_FLOW_RES": "1" if variant.startswith("compact_pairmajor") else "0"}
    if variant.endswith("small_staging"):
        hooks["WG_LF_CAP"] = "96"
    env = make_batch(hip, cfg, hooks, variant=(256, variant.startswith("compact_pairmajor"), None))
    orc = oracle_lib.Oracle(cfg)
    seeds = 500 + np.arange(3)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(4)
    n_tr = 0
    for step in range(260):
        a = rng.uniform(-1, 1, size=(3, 80)).astype(np.float32)
        _compare_step(env, orc, a, step, check_flow=(step % 20 == 0))
        n_tr += int(env.truncated.sum().item())
    env.check()
    assert n_tr >= 3
    u = env.info("rotor_uvw_agent").cpu().numpy()[..., 0]
    assert (u.min(axis=1) < env.info("ws_global").cpu().numpy() - 0.3).all()      # downstream rows are waked


def test_multi_agent_3x3_batched_matches_oracle(hip, oracle_lib):
    """BASELINE.json configs[3] at test size: per-turbine-agent packing [B, 9, o_t + o_f] for a batch."""
    from windgym_amd.config import EnvConfig
    from windgym_amd.presets import multi_3x3_config
    from windgym_amd.turbine import V80
    d = multi_3x3_config()
    d["mes_level"].update(turb_wd=True, farm_ws=True, farm_power=True, farm_TI=True, turb_TI=True)
    d["wd_mes"]["wd_rolling_mean"] = True
    d["power_mes"]["power_rolling_mean"] = True
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=7, autoreset=True, n_passthrough=1,
                    extra_timestep_inc=True)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    seeds = 900 + np.arange(7)
    env.reset(seeds=seeds), orc.reset(seeds=seeds)
    np.testing.assert_allclose(env.obs_multi().cpu().numpy(), orc.obs_multi(), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(6)
    for step in range(150):
        a = rng.uniform(-1, 1, size=(7, 9)).astype(np.float32)
        _compare_step(env, orc, a, step, check_flow=False)
        if step % 10 == 0:
            np.testing.assert_allclose(env.obs_multi().cpu().numpy(), orc.obs_multi(), rtol=0, atol=OBS_ATOL)
    env.check()


def test_fused_per_agent_observations_equal_the_explicit_packing(hip, oracle_lib):
    """wg_set_obs_multi_buffer: the per-agent observations written by the step's own glue kernel equal what wg_obs_multi
    returns after the step (to float rounding: the glue sums a window on several lanes, wg_obs_multi sequentially) and
    the oracle's packing, across resets and episode rollovers."""
    import torch
    from windgym_amd import presets
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    B = 6
    cfg = EnvConfig(turbine=V80(), yaml_dict=presets.multi_3x3_config(), turbtype="None", n_envs=B, autoreset=True,
                    n_passthrough=1, extra_timestep_inc=True)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    buf = env.fuse_obs_multi()
    seeds = 31 + np.arange(B)
    env.reset(seeds=seeds), orc.reset(seeds=seeds)
    assert (buf - env.obs_multi()).abs().max().item() <= 2e-6
    np.testing.assert_allclose(buf.cpu().numpy(), orc.obs_multi(), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(2)
    n_tr = 0
    for step in range(260):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        _, _, tr, _ = env.step(torch.as_tensor(a, device="cuda"))
        orc.step(a)
        assert (buf - env.obs_multi()).abs().max().item() <= 2e-6, step
        if step % 13 == 0:
            np.testing.assert_allclose(buf.cpu().numpy(), orc.obs_multi(), rtol=0, atol=OBS_ATOL, err_msg=f"step {step}")
        n_tr += int(tr.sum().item())
    assert n_tr >= B
    env.fuse_obs_multi(False)
    before = buf.clone()
    env.step(torch.zeros((B, cfg.n_turb), device="cuda"))
    assert torch.equal(buf, before)                     # unregistered: no longer written
    env.check()


@pytest.mark.parametrize("block", STEADY_BLOCKS)
def test_noise_normal_matches_oracle_stream(hip, oracle_lib, block):
    """noise: "Normal" (2turb.yaml / 4turb.yaml): the Philox/Box-Muller stream is the same on both sides; the
    kernel evaluates log/cos in fast fp32 -> tolerance 2e-3 deg on the 2-deg wd noise (1e-4 of the wd scale)."""
    from windgym_amd.config import EnvConfig
    from windgym_amd.presets import four_turb_config
    from windgym_amd.turbine import V80
    d = four_turb_config()
    d["mes_level"].update(turb_wd=True)
    d["wd_mes"].update(wd_current=True, wd_rolling_mean=True)
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=5, autoreset=True, n_passthrough=1)
    env, orc = make_env(hip, cfg, block), oracle_lib.Oracle(cfg)
    seeds = 11 + np.arange(5)
    g0, o0 = env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds)
    np.testing.assert_allclose(g0, o0, rtol=0, atol=5e-4)
    assert np.std(g0) > 0
    rng = np.random.default_rng(8)
    import torch
    for step in range(120):
        a = rng.uniform(-1, 1, size=(5, 4)).astype(np.float32)
        obs, rew, tr, _ = env.step(torch.as_tensor(a, device="cuda"))
        o_obs, o_rew, o_tr, _ = orc.step(a)
        np.testing.assert_array_equal(tr.cpu().numpy().astype(bool), o_tr)
        np.testing.assert_allclose(obs.cpu().numpy(), o_obs, rtol=0, atol=5e-4)
    env.check()


def test_midepisode_reset_starts_a_new_noise_stream(hip, oracle_lib):
    """an explicit reset(seed=None) that abandons running episodes starts a new episode index on both sides
    (the sensor-noise stream is keyed by it, so the abandoned episode's noise is not replayed) and the two stay in step.
    autoreset off: with it on, the device has already drawn the look-ahead episode and an explicit reset re-draws both
    contexts — the documented one-episode lead of the generator (include/windgym_hip.h, wg_reset)."""
    import torch
    from windgym_amd.config import EnvConfig
    from windgym_amd.presets import four_turb_config
    from windgym_amd.turbine import V80
    d = four_turb_config()
    d["mes_level"].update(turb_wd=True)
    d["wd_mes"].update(wd_current=True, wd_rolling_mean=True)
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=5, autoreset=False, n_passthrough=2)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    seeds = 11 + np.arange(5)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=5e-4)
    rng = np.random.default_rng(8)
    first = []
    for step in range(12):
        a = rng.uniform(-1, 1, size=(5, 4)).astype(np.float32)
        obs, rew, tr, _ = env.step(torch.as_tensor(a, device="cuda"))
        o_obs, o_rew, o_tr, _ = orc.step(a)
        assert not o_tr.any()
        np.testing.assert_allclose(obs.cpu().numpy(), o_obs, rtol=0, atol=5e-4)
        first.append(o_obs.copy())
    ep_before = env.info("episode").cpu().numpy().copy()
    g1, o1 = env.reset().cpu().numpy(), orc.reset()
    np.testing.assert_allclose(g1, o1, rtol=0, atol=5e-4)
    np.testing.assert_array_equal(env.info("episode").cpu().numpy(), orc.info("episode"))
    np.testing.assert_array_equal(env.info("episode").cpu().numpy(), ep_before + 1)
    for step in range(12):
        a = rng.uniform(-1, 1, size=(5, 4)).astype(np.float32)
        obs, rew, tr, _ = env.step(torch.as_tensor(a, device="cuda"))
        o_obs, o_rew, o_tr, _ = orc.step(a)
        np.testing.assert_allclose(obs.cpu().numpy(), o_obs, rtol=0, atol=5e-4)
    env.check()


@pytest.fixture(scope="module")
def small_mann_box():
    from windgym_amd.mann import generate_mann_box
    return generate_mann_box((256, 64, 32), (3.0, 3.0, 3.0), seed=1234), (3.0, 3.0, 3.0)


# with turbulence the rotor wind speeds fluctuate by O(1 m/s); fast fp32 log/cos in the Box-Muller transform and
# fp32 trilinear weights move individual samples by ~1e-4 relative, hence slightly wider bars than for steady inflow
TURB_OBS_ATOL = 5e-4


def _compare_turb(env, orc, steps, rng, n_turb, B):
    import torch
    n_tr = 0
    for step in range(steps):
        a = rng.uniform(-1, 1, size=(B, n_turb)).astype(np.float32)
        obs, rew, tr, fin = env.step(torch.as_tensor(a, device="cuda"))
        o_obs, o_rew, o_tr, o_fin = orc.step(a)
        np.testing.assert_array_equal(tr.cpu().numpy().astype(bool), o_tr, err_msg=f"step {step}")
        np.testing.assert_allclose(obs.cpu().numpy(), o_obs, rtol=0, atol=TURB_OBS_ATOL, err_msg=f"obs step {step}")
        np.testing.assert_allclose(rew.cpu().numpy(), o_rew, rtol=1e-3, atol=1e-3, err_msg=f"reward step {step}")
        if step % 20 == 0:
            np.testing.assert_allclose(env.info("rotor_uvw_agent").cpu().numpy(), orc.info("rotor_uvw_agent"),
                                       rtol=2e-4, atol=2e-3, err_msg=f"uvw step {step}")
            np.testing.assert_allclose(env.info("yaw_base").cpu().numpy(), orc.info("yaw_base"), atol=2e-2)
        n_tr += int(tr.sum().item())
    return n_tr


@pytest.mark.parametrize("block", BLOCKS)
def test_random_inflow_matches_oracle(hip, oracle_lib, block):
    """turbtype "Random": counter-based gusts at the rotors and at the wake particles (meandering); the two k_flow<NT, RANDOM>
    instantiations without sensor noise and with the Gaussian deficit, <64, compact> and <256, uniform rings> (the other six:
    tests/test_gpu_variant_census.py)."""
    B = 6
    cfg = turb_cfg("Random", B)
    env, orc = make_env(hip, cfg, block), oracle_lib.Oracle(cfg)
    seeds = 300 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=TURB_OBS_ATOL)
    v = env.info("rotor_uvw_agent").cpu().numpy()[..., 1]
    assert np.std(v) > 0.01                      # the lateral component is alive -> wd sensors and controller work
    n_tr = _compare_turb(env, orc, 300, np.random.default_rng(9), cfg.n_turb, B)
    env.check()
    assert n_tr >= B


@pytest.mark.parametrize("block", BOX_BLOCKS)
@pytest.mark.parametrize("turbtype", ["MannFixed", "MannGenerate"])
def test_mann_box_inflow_matches_oracle(hip, oracle_lib, small_mann_box, turbtype, block):
    """BASELINE.json configs[4] at test size: frozen Mann box (trilinear, periodic, Taylor advection), DWM
    meandering of the wake particles through the low-pass filtered transverse inflow; every k_flow<NT, BOX>
    instantiation (256: chain pruning and the 16-byte record copy together with turbulence) and the one-launch env kernel
    k_flow_envb with two waves / one wave per env."""
    box, spacing = small_mann_box
    B = 5
    cfg = turb_cfg(turbtype, B)
    env, orc = make_env(hip, cfg, block), oracle_lib.Oracle(cfg)
    env.set_turbulence_box(box, spacing), orc.set_turbulence_box(box, spacing)
    seeds = 700 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=TURB_OBS_ATOL)
    n_tr = _compare_turb(env, orc, 260, np.random.default_rng(10), cfg.n_turb, B)
    env.check()
    assert n_tr >= B
    # the wake centre lines meander: particle positions leave the hub height / the turbine's y
    u = env.info("rotor_uvw_agent").cpu().numpy()
    assert np.std(u[..., 0]) > 0.05 and np.std(u[..., 2]) > 0.005


@pytest.mark.parametrize("dims,spacing,turbtype", [((256, 64, 32), (3.0, 3.0, 3.0), "MannGenerate"),      # coarse copy 64 x 16 x 8: masks
                                                   ((240, 72, 40), (3.0, 3.0, 3.0), "MannGenerate"),      # coarse copy 60 x 18 x 10: modulo
                                                   ((256, 64, 32), (3.0, 3.0, 3.0), "Random")])
def test_cfg5_shape_runs_the_instantiation_the_bench_runs(hip, oracle_lib, dims, spacing, turbtype):
    """BASELINE.json configs[4] at its real farm shape: 4 x 4 turbines x P = 128 (N P = 2048) selects
    the kernel bench.py --workload cfg5 times (the handle's default) — here against the oracle, with a box whose
    block-averaged meandering copy has power-of-two dims and one whose copy has not (both divisible by 4).  "Random"
    covers k_flow<64, RANDOM> at the same shape (one case: it reads no box)."""
    from windgym_amd.mann import generate_mann_box
    B = 4
    cfg = turb_cfg(turbtype, B, nx=4, ny=4)
    assert cfg.n_turb * cfg.n_particles == 2048
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    if turbtype != "Random":
        box = generate_mann_box(dims, spacing, seed=77)
        env.set_turbulence_box(box, spacing), orc.set_turbulence_box(box, spacing)
    seeds = 500 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=TURB_OBS_ATOL)
    n_tr = _compare_turb(env, orc, 330, np.random.default_rng(14), cfg.n_turb, B)
    env.check()
    assert n_tr >= 1


def test_mann_box_ragged_dims_matches_oracle(hip, oracle_lib):
    """A box whose dims are neither powers of two nor divisible by 4: modulo wrap instead of masks, and the wake
    particles read the fine box (no block-averaged meandering copy)."""
    from windgym_amd.mann import generate_mann_box
    box, spacing = generate_mann_box((90, 30, 18), (4.0, 5.0, 6.0), seed=4), (4.0, 5.0, 6.0)
    B = 3
    cfg = turb_cfg("MannGenerate", B)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    env.set_turbulence_box(box, spacing), orc.set_turbulence_box(box, spacing)
    seeds = 900 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=TURB_OBS_ATOL)
    _compare_turb(env, orc, 120, np.random.default_rng(11), cfg.n_turb, B)
    env.check()


@pytest.mark.parametrize("turbtype", ["None", "MannGenerate"])
def test_flow_field_view_matches_oracle(hip, oracle_lib, small_mann_box, turbtype):
    """wg_get_windspeed (fs.get_windspeed(XYView(...)), Wind_Farm_Env.py:1040-1083): the (u, v, w) field on an XY
    grid, agent and baseline farm, with and without wakes, after the farms were yawed for a while."""
    import torch
    B = 3
    cfg = turb_cfg(turbtype, B)
    cfg.advect_full_chains = True          # the view reaches 1000 m behind the last row: no chain pruning
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    if turbtype != "None":
        box, spacing = small_mann_box
        env.set_turbulence_box(box, spacing), orc.set_turbulence_box(box, spacing)
    seeds = 40 + np.arange(B)
    env.reset(seeds=seeds), orc.reset(seeds=seeds)
    rng = np.random.default_rng(12)
    for _ in range(40):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        env.step(torch.as_tensor(a, device="cuda")), orc.step(a)
    tx = orc.info("turb_x")
    ty = orc.info("turb_y")
    for b in (0, 2):
        xs = np.linspace(tx[b].min() - 200.0, tx[b].max() + 1000.0, 97).astype(np.float32)
        ys = np.linspace(ty[b].min() - 200.0, ty[b].max() + 200.0, 61).astype(np.float32)
        for farm in (0, 1):
            for wakes in (True, False):
                got = env.windspeed(b, xs, ys, farm=farm, include_wakes=wakes).cpu().numpy()
                ref = orc.windspeed(b, xs, ys, farm=farm, include_wakes=wakes)
                assert got.shape == (3, 97, 61)
                np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-3, err_msg=f"env {b} farm {farm} wakes {wakes}")
        # the wakes are there: behind the first row the field drops well below the free stream
        u = env.windspeed(b, xs, ys, farm=0).cpu().numpy()[0]
        u0 = env.windspeed(b, xs, ys, farm=0, include_wakes=False).cpu().numpy()[0]
        assert (u0 - u).max() > 1.0 and (u0 - u).min() > -1e-3
    # a different height: above the rotors the deficit is much weaker than at the hub
    hub_def = (env.windspeed(0, xs, ys, include_wakes=False) - env.windspeed(0, xs, ys))[0].max().item()
    top_def = (env.windspeed(0, xs, ys, z=cfg.tab.hub_height() + 120.0, include_wakes=False)
               - env.windspeed(0, xs, ys, z=cfg.tab.hub_height() + 120.0))[0].max().item()
    assert top_def < 0.5 * hub_def
    with pytest.raises(Exception):
        env.windspeed(B, xs, ys)


def test_chain_pruning_changes_no_output_and_streams_fewer_particles(hip):
    """wg_config.full_chains = 0 (default for batches): particles behind the most downstream turbine are not advected
    (compiled into the 256-thread, large-farm variant of k_flow — selected here with WG_FLOW_BLOCK).  Every output of
    step() must be bit-identical to the run that advects all P slots."""
    import torch
    B = 8
    outs = []
    streamed = []
    for full in (False, True):
        cfg = turb_cfg("None", B)
        cfg.advect_full_chains = full
        env = make_batch(hip, cfg, {"WG_FLOW_BLOCK": "256"}, variant=(256, None, 0))
        env.reset(seeds=60 + np.arange(B))
        env.kernel_timing(1)
        rng = np.random.default_rng(13)
        rec = []
        for _ in range(150):
            a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
            obs, rew, tr, fin = env.step(torch.as_tensor(a, device="cuda"))
            rec.append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), tr.cpu().numpy().copy()))
        rec.append((env.info("rotor_uvw_agent").cpu().numpy(), env.info("power_turb_base").cpu().numpy(),
                    env.info("yaw_base").cpu().numpy()))
        _, _, _, fsteps, parts = env.kernel_timing(False)
        streamed.append(parts / (fsteps * cfg.n_turb * cfg.n_particles))
        outs.append(rec)
        env.check()
    for (a0, a1, a2), (b0, b1, b2) in zip(*outs):
        np.testing.assert_array_equal(a0, b0), np.testing.assert_array_equal(a1, b1), np.testing.assert_array_equal(a2, b2)
    assert streamed[0] < 0.75 * streamed[1] and streamed[1] > 0.3, streamed


@pytest.mark.parametrize("turbtype", ["None", "Random"])
def test_results_do_not_depend_on_batch_composition(hip, turbtype):
    """Multi-GPU correctness by construction: an env's trajectory depends only on its seed, not on which handle /
    which position in the batch it occupies (two shards of 4 envs == one batch of 8, bit for bit; and a second run of
    the same batch reproduces itself)."""
    import torch
    from windgym_amd import presets
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    d = presets.two_turb_config()
    d["noise"] = "Normal"                               # sensor noise is keyed by the env's seed too
    seeds = 4000 + np.arange(8)
    rng = np.random.default_rng(21)
    acts = rng.uniform(-1, 1, size=(300, 8, 2)).astype(np.float32)

    def run(idx):
        cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype=turbtype, n_envs=len(idx), autoreset=True, n_passthrough=1)
        env = hip.HipBatch(cfg)
        out = [env.reset(seeds=seeds[idx]).cpu().numpy().copy()]
        for a in acts:
            obs, rew, tr, _ = env.step(torch.as_tensor(a[idx], device="cuda"))
            out.append(np.concatenate([obs.cpu().numpy(), rew.cpu().numpy()[:, None], tr.cpu().numpy()[:, None].astype(np.float32)], axis=1))
        env.check()
        return out
    full = run(np.arange(8))
    again = run(np.arange(8))
    lo, hi = run(np.arange(0, 4)), run(np.arange(4, 8))
    odd = run(np.array([7, 2, 5]))
    n_tr = 0
    for k in range(len(full)):
        np.testing.assert_array_equal(full[k], again[k])
        np.testing.assert_array_equal(full[k][:4], lo[k]), np.testing.assert_array_equal(full[k][4:], hi[k])
        np.testing.assert_array_equal(full[k][[7, 2, 5]], odd[k])
        if k:
            n_tr += int(full[k][:, -1].sum())
    assert n_tr >= 8                                    # the comparison covers episode rollovers


def test_mann_box_required(hip):
    cfg = turb_cfg("MannFixed", 2)
    env = hip.HipBatch(cfg)
    with pytest.raises(ValueError):
        env.reset(seeds=[1, 2])


def test_soak_many_episode_rollovers_at_bench_scale(hip):
    """Full-size properties (no oracle at this size): 1024 envs x 16 turbines x 2 farms, default n_passthrough,
    2600 steps = 3-6 episode rollovers per env.  The background-developed episode must always be ready (no sticky
    error), observations stay finite and inside [-1, 1], the farm is waked, and the episode count is consistent
    with the per-env episode lengths."""
    import torch
    from windgym_amd.config import EnvConfig
    from windgym_amd.presets import bench_cfg2_config
    from windgym_amd.turbine import V80
    B = 1024
    cfg = EnvConfig(turbine=V80(), yaml_dict=bench_cfg2_config(), turbtype="None", n_envs=B, autoreset=True,
                    n_passthrough=5, n_rotor_pts=16)
    env = hip.HipBatch(cfg)
    env.reset(seeds=1234 + np.arange(B))
    g = torch.Generator(device="cpu").manual_seed(0)
    acts = (torch.rand((32, B, cfg.n_turb), generator=g) * 2 - 1).cuda()
    n_trunc = torch.zeros(B, dtype=torch.int64, device="cuda")
    steps = 2600
    for i in range(steps):
        obs, rew, tr, fin = env.step(acts[i % 32])
        n_trunc += tr.long()
        if i % 200 == 0:
            assert torch.isfinite(obs).all() and torch.isfinite(rew).all() and (obs.abs() <= 1).all()
            assert torch.isfinite(fin).all()
    env.check()                                                   # no NaN power, no unready background episode
    assert int(n_trunc.min()) >= 2 and int(n_trunc.max()) <= 7
    np.testing.assert_array_equal(env.info("episode").cpu().numpy(), n_trunc.cpu().numpy())
    tm = env.info("time_max").cpu().numpy()
    assert tm.min() >= 426 and tm.max() <= 1121                   # int(5 * dist / ws), ws in [7, 15], 1280 m <= dist <= 1568 m
    m = env.metrics().cpu().numpy()
    assert m[7] == steps * B and m[3] == int(n_trunc.sum())
    u = env.info("rotor_uvw_agent").cpu().numpy()[..., 0]
    ws = env.info("ws_global").cpu().numpy()
    assert (u.max(axis=1) <= ws * (1 + 1e-5)).all() and (u.min(axis=1) < ws - 0.02).all()   # every farm is waked


def test_box_pool_draws_like_np_random_choice_and_matches_oracle(hip, oracle_lib):
    """turbtype "MannLoad" with K = 3 boxes (row f2): every reset picks a box with the env's own PCG64 stream exactly
    like tf_file = self.np_random.choice(self.TF_files) (Wind_Farm_Env.py:614), and the flow then reads THAT box —
    checked step for step against the oracle, which holds the same pool on the host."""
    import torch
    from windgym_amd.mann import generate_mann_box
    spacing = (3.0, 3.0, 3.0)
    boxes = [generate_mann_box((128, 64, 32), spacing, seed=s) for s in (1, 2, 3)]
    B = 6
    cfg = turb_cfg("MannLoad", B)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    env.set_turbulence_boxes(boxes, spacing), orc.set_turbulence_boxes(boxes, spacing)
    seeds = 2100 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=TURB_OBS_ATOL)
    # the draw: ws, ti, wd = three uniforms, then choice(3 files) == integers(0, 3) on the same generator
    want = []
    for s in seeds:
        g = np.random.default_rng(int(s))
        g.uniform(), g.uniform(), g.uniform()
        want.append(int(g.choice(np.arange(3))))
    np.testing.assert_array_equal(env.info("box_id").cpu().numpy(), want)
    np.testing.assert_array_equal(orc.info("box_id").astype(int), want)
    n_tr = _compare_turb(env, orc, 200, np.random.default_rng(15), cfg.n_turb, B)
    env.check()
    assert n_tr >= B and len(set(want)) >= 2
    # a pool of one consumes no draw (numpy's bounded integers with range 0), like choice() on a one-file list
    env1, orc1 = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    env1.set_turbulence_boxes(boxes[:1], spacing), orc1.set_turbulence_boxes(boxes[:1], spacing)
    np.testing.assert_allclose(env1.reset(seeds=seeds).cpu().numpy(), orc1.reset(seeds=seeds), rtol=0, atol=TURB_OBS_ATOL)
    g = np.random.default_rng(int(seeds[0]))
    ws = g.uniform(cfg.ws_min, cfg.ws_max)
    assert env1.info("wind_f64").cpu().numpy()[0, 0] == ws


def test_manngenerate_pool_seed_picks_box_and_offset(hip, oracle_lib):
    """turbtype "MannGenerate" with a pool of K = 3 generated realisations (EnvConfig.mann_pool): the episode's seed — the
    reference's integers(0, 100000) draw (Wind_Farm_Env.py:623) — picks the box (seed mod K) AND the offset into it; the flow
    then reads that box, step for step against the oracle across rollovers."""
    from windgym_amd.mann import generate_mann_box
    spacing = (3.0, 3.0, 3.0)
    boxes = [generate_mann_box((128, 64, 32), spacing, seed=s) for s in (11, 12, 13)]
    B = 6
    cfg = turb_cfg("MannGenerate", B)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    env.set_turbulence_boxes(boxes, spacing), orc.set_turbulence_boxes(boxes, spacing)
    seeds = 3100 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=TURB_OBS_ATOL)
    want = []
    for s in seeds:
        g = np.random.default_rng(int(s))
        g.uniform(), g.uniform(), g.uniform()
        want.append(int(g.integers(0, 100000)) % 3)
    np.testing.assert_array_equal(env.info("box_id").cpu().numpy(), want)
    np.testing.assert_array_equal(orc.info("box_id").astype(int), want)
    n_tr = _compare_turb(env, orc, 200, np.random.default_rng(16), cfg.n_turb, B)
    env.check()
    assert n_tr >= B and len(set(want)) >= 2


@pytest.mark.parametrize("case", ["rings_in_global", "current_only_and_farm", "ti_and_windows_l2"])
def test_glue_instantiations_match_oracle(hip, oracle_lib, case):
    """k_glue is instantiated per <per-agent buffer, rings staged in LDS, lanes per turbine>; the observation's window
    sums run on 64/N lanes per turbine and the rings are staged by LDS-DMA requests.  Cases the benchmark configs do not
    reach: rings too large for the wave's LDS region (80 turbines x 100-sample histories: read from global memory, one
    lane per turbine), channels observed through their newest sample only together with farm-level observations and
    TI (partial staging, farm rings), and a 5 x 4 farm (two lanes per turbine) with several windows per channel —
    observations, final observations and rewards against the oracle across an autoreset."""
    from windgym_amd.config import EnvConfig
    from windgym_amd.presets import horns_rev1_layout, horns_rev_config, env1_config
    from windgym_amd.turbine import V80
    import copy
    kw = {}
    if case == "rings_in_global":
        d = horns_rev_config()
        d["ws_mes"].update(ws_current=True, ws_history_N=3, ws_history_length=100, ws_window_length=20)
        d["yaw_mes"].update(yaw_history_N=2, yaw_history_length=60, yaw_window_length=10)
        d["mes_level"].update(turb_TI=True)
        x, y = horns_rev1_layout()
        kw = dict(x_pos=x, y_pos=y)
        B, steps, npt = 2, 40, 0.15
    elif case == "current_only_and_farm":
        d = copy.deepcopy(env1_config())
        d["ActionMethod"] = "yaw"
        d["farm"].update(nx=3, ny=2)
        d["mes_level"].update(turb_ws=True, turb_wd=True, turb_TI=True, turb_power=True, farm_ws=True, farm_wd=True,
                              farm_TI=True, farm_power=True)
        d["ws_mes"].update(ws_current=True, ws_rolling_mean=True, ws_history_N=2, ws_history_length=12, ws_window_length=5)
        d["wd_mes"].update(wd_current=True, wd_rolling_mean=False)
        d["power_mes"].update(power_current=True, power_rolling_mean=False)
        d["yaw_mes"].update(yaw_current=True, yaw_rolling_mean=False)
        B, steps, npt = 5, 120, 0.3
    else:
        d = copy.deepcopy(env1_config())
        d["ActionMethod"] = "yaw"
        d["farm"].update(nx=5, ny=4)
        d["mes_level"].update(turb_TI=True, farm_TI=True)
        d["ws_mes"].update(ws_current=True, ws_history_N=4, ws_history_length=30, ws_window_length=7)
        d["yaw_mes"].update(yaw_history_N=3, yaw_history_length=9, yaw_window_length=4)
        B, steps, npt = 3, 120, 0.3
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=B, autoreset=True, n_passthrough=npt,
                    n_rotor_pts=16, **kw)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    seeds = 400 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(11)
    n_tr = 0
    for step in range(steps):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        _compare_step(env, orc, a, step, check_flow=False)
        n_tr += int(env.truncated.sum().item())
    if case != "rings_in_global":
        assert n_tr >= 1
    env.check()
    env.close()


def test_prepared_first_observation_survives_buffer_switches(hip, oracle_lib):
    """On a handle whose flow kernel prepares the next episode's first observation (single-wave steady variant, 4 x 4
    farm) the glue copies it at truncation; with a per-agent buffer registered the glue builds it itself.  Switching the
    buffer on and off across rollovers (and restoring a state blob, which does not carry the prepared rows) must never
    hand out the first observation of an episode that has since been replaced: every step against the oracle."""
    import torch
    B = 6
    cfg = physics_cfg(B, autoreset=True, n_passthrough=0.25)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    assert env.flow_variant() == (64, True, 2)          # k_flow_env (two waves per env) prepares the first observation too
    seeds = 900 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(5)
    n_tr = [0, 0, 0, 0]
    step = 0
    for phase in range(4):
        if phase == 1:
            env.fuse_obs_multi()
        elif phase == 2:
            env.fuse_obs_multi(False)
        elif phase == 3:
            env.set_state(env.get_state())
        for _ in range(130):
            a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
            _compare_step(env, orc, a, step, check_flow=False)
            n_tr[phase] += int(env.truncated.sum().item())
            step += 1
    assert min(n_tr) >= 1, n_tr
    env.check()
    env.close()


def test_checkpoint_resume_is_bit_identical_across_rollovers(hip):
    """a run restored from a state blob must reproduce the uninterrupted run bit for bit, also through the
    rollovers — the blob does not carry the first observations / window sums the flow kernel prepares for the next
    episodes, so the restored handle rebuilds them at the swap (lean_swap's fallback): both paths use one arithmetic."""
    import torch
    B = 8
    cfg = physics_cfg(B, autoreset=True, n_passthrough=0.25)
    a_env, b_env = hip.HipBatch(cfg), hip.HipBatch(cfg)
    assert a_env.flow_variant() == (64, True, 2)
    seeds = 300 + np.arange(B)
    a_env.reset(seeds=seeds)
    rng = np.random.default_rng(9)
    acts = [torch.as_tensor(rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32), device="cuda") for _ in range(260)]
    for i in range(60):
        a_env.step(acts[i])
    b_env.reset(seeds=seeds)
    b_env.set_state(a_env.get_state())
    n_tr = 0
    for i in range(60, 260):
        oa, ra, ta, fa = (t.clone() for t in a_env.step(acts[i]))
        if i % 40 == 0:
            b_env.set_state(b_env.get_state())          # drops whatever the flow kernel has prepared so far
        ob, rb, tb, fb = b_env.step(acts[i])
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(fa, fb), i
        n_tr += int(ta.sum().item())
    assert n_tr >= B
    a_env.check(); b_env.check()
    a_env.close(); b_env.close()


@pytest.mark.parametrize("case", ["env1_4x4", "generic_ti_farm_current", "per_agent_buffer"])
def test_lean_glue_equals_the_ring_staging_glue(hip, case):
    """k_glue_lean (running window sums, sums mode) against k_glue (rings staged and summed every step, WG_SUMS=0) on the
    same handle configuration, step for step across rollovers: observations, final observations, rewards, truncations —
    two independently written kernels, one answer (to float rounding: exact double sums vs float sums)."""
    import copy
    import torch
    from windgym_amd.config import EnvConfig
    from windgym_amd.presets import env1_config
    from windgym_amd.turbine import V80
    d = copy.deepcopy(env1_config())
    d["ActionMethod"] = "yaw"
    B, multi = 6, False
    if case == "env1_4x4":
        d["farm"].update(nx=4, ny=4)
    elif case == "generic_ti_farm_current":
        d["farm"].update(nx=3, ny=2)
        d["mes_level"].update(turb_ws=True, turb_wd=True, turb_TI=True, turb_power=True, farm_ws=True, farm_wd=True,
                              farm_TI=True, farm_power=True)
        d["ws_mes"].update(ws_current=True, ws_rolling_mean=True, ws_history_N=1, ws_history_length=12, ws_window_length=5)
        d["wd_mes"].update(wd_current=True, wd_rolling_mean=True, wd_history_N=1, wd_history_length=8, wd_window_length=8)
        d["power_mes"].update(power_current=True, power_rolling_mean=True, power_history_N=1, power_history_length=20,
                              power_window_length=30)
        d["yaw_mes"].update(yaw_current=True, yaw_rolling_mean=False)
    else:
        d["farm"].update(nx=3, ny=3)
        d["mes_level"].update(farm_ws=True, farm_TI=True)
        multi = True
    kw = dict(extra_timestep_inc=True) if multi else {}
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=B, autoreset=True, n_passthrough=0.3, n_rotor_pts=16, **kw)
    lean = hip.HipBatch(cfg)
    ring = make_batch(hip, cfg, {"WG_SUMS": "0"})
    ml = lean.fuse_obs_multi() if multi else None
    mr = ring.fuse_obs_multi() if multi else None
    seeds = 70 + np.arange(B)
    assert (lean.reset(seeds=seeds) - ring.reset(seeds=seeds)).abs().max().item() <= 2e-6
    rng = np.random.default_rng(2)
    n_tr = 0
    for step in range(200):
        a = torch.as_tensor(rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32), device="cuda")
        ol, rl, tl, fl = lean.step(a)
        orr, rr, tr, fr = ring.step(a)
        assert torch.equal(tl, tr), step
        assert (ol - orr).abs().max().item() <= 2e-6 and (fl - fr).abs().max().item() <= 2e-6, step
        assert (rl - rr).abs().max().item() <= 2e-6 + 1e-6 * rr.abs().max().item(), step
        if multi:
            assert (ml - mr).abs().max().item() <= 2e-6, step
        n_tr += int(tl.sum().item())
    assert n_tr >= B
    lean.check(); ring.check()
    lean.close(); ring.close()


@pytest.mark.parametrize("nx,ny", [(16, 8), (13, 5), (11, 6)])
def test_large_farm_variant_at_its_size_limits(hip, oracle_lib, nx, ny):
    """The 256-thread compact steady variant (what cfg3 runs) at the edges of its mask / ballot layout: 128 turbines (the
    build's maximum: two full 64-source blocks, four mask words), 65 and 66 (a second source block with one / two sources),
    wind directions that wake the farm along rows and diagonals, same-step autoreset."""
    import torch
    from windgym_amd import presets
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    d = presets.env1_config()
    d["farm"].update(nx=nx, ny=ny, xDist=4, yDist=3)
    d["wind"] = dict(ws_min=9, ws_max=11, wd_min=250, wd_max=290, TI_min=0.05, TI_max=0.1)
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=2, autoreset=True, n_passthrough=0.3, n_rotor_pts=8)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    assert env.flow_variant() == (256, True, False) and cfg.n_turb == nx * ny
    np.testing.assert_allclose(env.reset(seeds=[3, 4]).cpu().numpy(), orc.reset(seeds=[3, 4]), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(0)
    for step in range(60):
        a = rng.uniform(-1, 1, size=(2, cfg.n_turb)).astype(np.float32)
        _compare_step(env, orc, a, step, check_flow=(step % 20 == 0))
    env.check()


def test_never_truncate_long_run_keeps_the_running_ti_sums_on_the_oracle(hip, oracle_lib):
    """in sums mode the lean glue carries the ws deque's sum and sum of squares (calc_TI, MesClass.py:220-237) as
    RUNNING sums for the whole episode; the sum of squares rounds (v * v needs 48 mantissa bits) and the rounding is carried
    along.  An episode that never truncates, 12 000 steps, TI entries at turbine and farm level observed: the observation must
    stay on the oracle's (which recomputes TI from the deque every step) — i.e. the drift of the running sum of squares stays
    orders of magnitude below the observation tolerance."""
    import copy
    import torch
    from windgym_amd.config import EnvConfig
    from windgym_amd.presets import env1_config
    from windgym_amd.turbine import V80
    d = copy.deepcopy(env1_config())
    d["ActionMethod"] = "yaw"
    d["farm"].update(nx=3, ny=2)
    d["mes_level"].update(turb_ws=True, turb_TI=True, farm_ws=True, farm_TI=True)
    B = 3
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=B, autoreset=False, n_passthrough=1, n_rotor_pts=16,
                    never_truncate=True)
    env, orc = hip.HipBatch(cfg), oracle_lib.Oracle(cfg)
    seeds = 41 + np.arange(B)
    np.testing.assert_allclose(env.reset(seeds=seeds).cpu().numpy(), orc.reset(seeds=seeds), rtol=0, atol=OBS_ATOL)
    rng = np.random.default_rng(3)
    worst = 0.0
    for step in range(12000):
        a = rng.uniform(-1, 1, size=(B, cfg.n_turb)).astype(np.float32)
        obs, rew, tr, _ = env.step(torch.as_tensor(a, device="cuda"))
        o_obs, o_rew, o_tr, _ = orc.step(a)
        assert not o_tr.any()
        if step % 100 == 0 or step > 11900:
            assert not tr.any()
            g = obs.cpu().numpy()
            np.testing.assert_allclose(g, o_obs, rtol=0, atol=OBS_ATOL, err_msg=f"obs step {step}")
            worst = max(worst, float(np.abs(g - o_obs).max()))
    env.check()
    assert worst <= OBS_ATOL
    env.close()
