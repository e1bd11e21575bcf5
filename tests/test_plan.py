"""Which kernel a handle runs, decided on the CPU: windgym_amd/csrc/wg_plan.h is host-only C++, so the choices wg_create makes
(variant, threads, waves per env, LDS carve — DESIGN.md §4, §5) are pinned here without a device.  tests/plan_shim.cpp hands
the plan of a wg_config back as text."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import bench
from helpers import host_shim
from windgym_amd import presets
from windgym_amd.binding import HOOK_ENV
from windgym_amd.config import CConfig, EnvConfig
from windgym_amd.turbine import V80

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "windgym_amd", "csrc")
HOOKS = list(HOOK_ENV)[:10]      # the plan's ten integer hooks, flow_block .. pstride_pad: the layout of plan_shim.cpp's array
WG_ERR_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """g++ alone, no ROCm include path: the plan must stay free of HIP headers."""
    lib = host_shim(tmp_path_factory, "plan", include_header_dir=True)
    lib.plan_dump.argtypes = [C.POINTER(CConfig), C.POINTER(C.c_int), C.c_int, C.c_longlong, C.c_longlong, C.c_char_p, C.c_int]
    lib.plan_table.argtypes = [C.POINTER(CConfig), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double)]

    def plan(cfg, lds_limit=65536, box_cells=0, abox_cells=0, first_obs_gl_only=False, **hooks):
        arr = (C.c_int * 21)()
        for k, v in hooks.items():
            i = HOOKS.index(k)
            arr[2 * i], arr[2 * i + 1] = 1, v
        arr[20] = int(first_obs_gl_only)
        buf = C.create_string_buffer(4096)
        cc = cfg.to_c() if isinstance(cfg, EnvConfig) else cfg
        lib.plan_dump(C.byref(cc), arr, lds_limit, box_cells, abox_cells, buf, 4096)
        d = dict(ln.split(" ", 1) for ln in buf.value.decode().splitlines())
        return {k: (v if k == "err" else (float(v) if k in ("alg_bytes", "tab_x0", "tab_dx") else int(v))) for k, v in d.items()}

    plan.lib = lib
    return plan


def grid_cfg(nx, ny, n_envs, turbtype="None", farms2=True, **kw):
    d = presets._upd(presets.env1_config(), ActionMethod="yaw", farm=dict(nx=nx, ny=ny))
    if not farms2:
        d["power_def"]["Power_reward"] = "Power_avg"
    return EnvConfig(turbine=V80(), yaml_dict=d, turbtype=turbtype, n_envs=n_envs, autoreset=True, **kw)


def pick(d, *keys):
    return tuple(d[k] for k in keys)


def test_plan_header_is_host_only(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "wg_plan.h"\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src)], check=True)
    text = open(os.path.join(CSRC, "wg_plan.h")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    for word in ("getenv", "hipMalloc", "hip_runtime", "wg_env_s"):
        assert word not in code, word


# ---- DESIGN.md's table of the step path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_envs, wpe, split", [(8192, 1, 0), (4096, 1, 0), (2048, 2, 0), (1024, 2, 1), (512, 2, 2), (256, 2, 2)])
def test_cfg2_waves_per_env_and_pass_waves(shim, n_envs, wpe, split):
    d = shim(bench.make_cfg(n_envs, workload="cfg2"))
    assert pick(d, "envw", "env_wpe", "env_split", "env_fused", "block", "res", "gl", "rec_il") == (1, wpe, split, 1, 64, 1, 1, 1)
    assert d["compact"] == d["res"] and d["first_obs"] == 1 and d["sums_mode"] == 1


def test_other_bench_workloads(shim):
    d = shim(bench.make_cfg(1024, workload="cfg4"))       # 3 x 3 farm: its pass is two trips (qf < 256) — no pass wave
    assert pick(d, "envw", "env_wpe", "env_split") == (1, 2, 0)
    d = shim(bench.make_cfg(1024, workload="cfg5"))       # frozen box: k_flow_envb on the SoA record
    assert pick(d, "envw", "env_wpe", "env_split", "gl", "rec_il", "block", "res") == (1, 2, 0, 0, 0, 64, 1)
    assert shim(bench.make_cfg(4096, workload="cfg5"))["env_wpe"] == 1
    d = shim(bench.make_cfg(512, workload="cfg3"))        # 80 turbines, steady: the 256-thread compact variant, no env kernel
    assert pick(d, "block", "res", "rec_il", "envw", "env_fused", "gl") == (256, 1, 1, 0, 0, 0) and d["lf_cap"] >= 512


def test_large_turbulent_farm_and_model_options(shim):
    d = shim(grid_cfg(8, 5, 64, "MannGenerate"))          # N > 32, turbulent: uniform rings, sample-major
    assert pick(d, "res", "block", "envw", "compact", "first_obs") == (0, 256, 0, 0, 0)
    d = shim(grid_cfg(4, 4, 1024, "None", farms2=False))  # n_farms = 1
    assert pick(d, "envw", "env_wpe", "block") == (1, 2, 64)
    # k_flow_env is Gaussian, without the wake-added field; k_flow_envb takes the added field but not the other deficits
    assert shim(grid_cfg(4, 4, 1024, deficit="super_gaussian"))["envw"] == 0
    assert shim(grid_cfg(4, 4, 1024, "MannGenerate", added_turbulence="iso"))["envw"] == 1
    assert shim(grid_cfg(4, 4, 1024, "MannGenerate", deficit="super_gaussian"))["envw"] == 0
    r = shim(grid_cfg(8, 5, 64, "MannGenerate", deficit="super_gaussian"))
    assert r["rc"] == WG_ERR_UNSUPPORTED and r["err"].startswith("deficit_model 1 / 2 (super-Gaussian, eddy-viscosity table) are built into the compact")


# ---- the hooks the GPU tests select variants with --------------------------------------------------------------------------------
def test_hooks(shim):
    c2, c3, c5 = (bench.make_cfg(n, workload=w) for n, w in ((1024, "cfg2"), (64, "cfg3"), (1024, "cfg5")))
    assert pick(shim(c2, flow_block=64), "res", "block", "gl", "envw") == (1, 64, 1, 0)
    # (128 threads is not built: the value is ignored like any unknown one — the no-hook variant, the env kernels off as for every set hook)
    assert pick(shim(c2, flow_block=128), "res", "block", "gl", "rec_il", "envw") == pick(shim(c2), "res", "block", "gl", "rec_il") + (0,) == (1, 64, 1, 1, 0)
    assert pick(shim(c2, flow_block=256), "res", "block", "rec_il", "envw") == (0, 256, 0, 0)
    assert pick(shim(c2, flow_block=64, flow_env=1), "block", "envw") == (64, 1)
    assert pick(shim(c2, flow_res=0), "res", "block", "envw") == (0, 256, 0)
    assert pick(shim(c3, flow_res=0), "res", "block", "rec_il", "lf_cap") == (0, 256, 0, 0)
    assert pick(shim(grid_cfg(8, 5, 64, "MannGenerate"), flow_res=1), "res", "block") == (0, 256)      # (no compact kernel for large turbulent farms)
    assert pick(shim(c2, flow_env=0), "envw", "env_fused", "block", "gl") == (0, 0, 64, 1)
    assert pick(shim(c2, flow_env=1), "envw", "env_fused") == (1, 1)
    assert shim(c3, flow_env=1)["envw"] == 0              # (only where eligible)
    assert [shim(c2, env_wpe=w)["env_wpe"] for w in (1, 2, 4)] == [1, 2, 1]
    assert [shim(c5, env_wpe=w)["env_wpe"] for w in (1, 2, 4)] == [1, 2, 4]
    assert shim(grid_cfg(5, 5, 64, "MannGenerate", farms2=False), env_wpe=4)["env_wpe"] == 2      # four waves: two farms of up to 16 turbines
    assert [shim(c2, env_split=s)["env_split"] for s in (0, 1, 2)] == [0, 1, 2]
    assert shim(bench.make_cfg(2048, workload="cfg2"), env_split=1)["env_split"] == 1 and shim(c2, env_split=1, env_wpe=1)["env_split"] == 0
    assert shim(c5, env_split=1)["env_split"] == 0
    assert pick(shim(c2, step_fused=0), "envw", "env_fused") == (1, 0)
    assert pick(shim(c2, sums=0), "sums_mode", "envw", "env_fused", "first_obs") == (0, 1, 0, 1)
    assert shim(c3, first_obs_gl_only=True)["first_obs"] == 0 and shim(c3)["first_obs"] == 1
    assert [shim(c3, lf_cap=v)["lf_cap"] for v in (1, 100, 10 ** 6)] == [64, 100, shim(c3)["lf_cap"]]
    assert shim(c2, pstride_pad=0)["pstride"] == 16 * 128 and shim(c2, pstride_pad=64)["pstride"] == 16 * 128 + 64
    assert shim(c2, lds_pad=4096)["lds_bytes"] == shim(c2)["lds_bytes"] + 4096 and shim(c2, lds_pad=10 ** 6)["lds_bytes"] == 65536


# ---- invariants over a grid ------------------------------------------------------------------------------------------------------
def test_invariants_over_a_grid(shim):
    seen_fallback = seen_refused = seen_envb_stepdown = 0
    layouts = [(1, 1), (2, 2), (4, 4), (5, 5), (6, 5), (8, 5), (10, 8), (12, 10)]
    for (nx, ny), P, S, f2, B, tt, lds in itertools.product(layouts, (None, 128, 8192), (4, 16, 64), (True, False), (24, 1024, 4096),
                                                            ("None", "Random", "MannGenerate"), (65536, 32768)):
        cfg = grid_cfg(nx, ny, B, tt, farms2=f2, n_rotor_pts=S, **({"n_particles": P} if P else {}))
        d = shim(cfg, lds_limit=lds)
        if d["rc"]:
            assert d["rc"] == WG_ERR_UNSUPPORTED and "too many turbines for one workgroup" in d["err"] and f"(limit {lds})" in d["err"]
            seen_refused += 1
            continue
        for k in ("lds_bytes", "env_lds", "lds_off_tab", "env_off_tab"):
            assert d[k] % 16 == 0, (k, d)
        assert d["lds_bytes"] <= lds and d["res"] == d["compact"]
        assert d["pstride"] >= d["NP"] and d["pstride"] % 64 == 0 and (d["pstride"] // 64) % 2 == 1
        assert d["block"] in (64, 256) and (d["res"] or d["block"] == 256)
        if d["envw"]:
            assert d["env_wpe"] * d["env_lds"] <= lds and d["env_lds"] <= 32768
            if d["env_split"]:      # what the pass-wave launch requests: the waves' regions + the pre-fetched glue inputs
                assert (2 + d["env_split"]) * d["env_lds"] + d["LEAN_PRE_BYTES"] <= lds
            assert d["block"] == 64 and d["res"] == 1 and d["N"] * 2 * (2 if f2 else 1) <= 64
        else:
            assert d["env_fused"] == 0 and d["env_split"] == 0
        assert pick(d, "path_envw", "path_fused") == pick(d, "envw", "env_fused") == pick(d, "envw_eligible", "fused_eligible")
        small = nx * ny <= 32
        seen_fallback += small and d["res"] == 0          # res 1 did not fit: the uniform-ring carve
        seen_envb_stepdown += tt == "MannGenerate" and d["envw"] and B <= 2048 and d["env_wpe"] == 1
    assert seen_fallback and seen_refused and seen_envb_stepdown


# wg_flow.hip's launch table: (threads, compact rings, turbulent inflow) of every k_flow that is built
BUILT = {(64, 1, False), (64, 1, True), (256, 1, False), (256, 0, False), (256, 0, True)}


def test_no_hook_names_a_kernel_that_is_not_built(shim):
    """The grid of test_invariants_over_a_grid x WG_FLOW_BLOCK x WG_FLOW_RES: every accepted plan is a row of the launch table."""
    layouts = [(1, 1), (2, 2), (4, 4), (5, 5), (6, 5), (8, 5), (10, 8), (12, 10)]
    n_plans = 0
    for (nx, ny), P, S, f2, B, tt, lds in itertools.product(layouts, (None, 128, 8192), (4, 16, 64), (True, False), (24, 1024, 4096),
                                                            ("None", "Random", "MannGenerate"), (65536, 32768)):
        cfg = grid_cfg(nx, ny, B, tt, farms2=f2, n_rotor_pts=S, **({"n_particles": P} if P else {})).to_c()
        for fb, fr in itertools.product((None, 64, 128, 256), (None, 0, 1)):
            hooks = {k: v for k, v in (("flow_block", fb), ("flow_res", fr)) if v is not None}
            d = shim(cfg, lds_limit=lds, **hooks)
            if d["rc"]:
                continue
            n_plans += 1
            assert (d["block"], d["res"], tt != "None") in BUILT, (nx, ny, P, S, f2, B, tt, lds, hooks, pick(d, "block", "res"))
            assert d["rec_il"] == (d["res"] and tt == "None") and d["gl"] == (d["rec_il"] and d["block"] == 64)
    assert n_plans > 20000


def test_envb_wave_count_steps_down_with_the_lds(shim):
    c5 = bench.make_cfg(1024, workload="cfg5")
    assert [pick(shim(c5, lds_limit=m), "env_wpe", "env_lds") for m in (65536, 32768)] == [(2, 16384), (1, 17344)]
    assert [shim(c5, lds_limit=m, env_wpe=4)["env_wpe"] for m in (65536, 32768, 20000)] == [4, 4, 1]


def test_too_large_farm_is_refused_before_any_allocation(shim):
    r = shim(grid_cfg(12, 10, 64, "MannGenerate"), lds_limit=32768)
    assert r == {"rc": WG_ERR_UNSUPPORTED,
                 "err": "wg_create: k_flow needs 35984 bytes of LDS per workgroup (limit 32768): too many turbines for one workgroup"}


# ---- exact carves of the bench workloads (as the previous, unsplit wg_create computed them) ---------------------------------------
@pytest.mark.parametrize("workload, n_envs, expect", [
    ("cfg2", 4096, (8672, 9152, 8832, 16, 0, 2112)),
    ("cfg3", 512, (33264, 57792, 57472, 27, 1548, 35904)),
    ("cfg4", 2048, (5392, 7808, 7488, 9, 0, 960)),
    ("cfg5", 1024, (11552, 16384, 16064, 16, 0, 2112)),
    ("env1", 4096, (3808, 7328, 7008, 4, 0, 448)),
])
def test_exact_carves(shim, workload, n_envs, expect):
    cfg = (EnvConfig(turbine=V80(), yaml_dict=presets.env1_config(), turbtype="None", n_envs=n_envs, autoreset=True) if workload == "env1"
           else bench.make_cfg(n_envs, workload=workload))
    assert pick(shim(cfg), "lds_bytes", "env_lds", "env_off_tab", "target_chunk", "lf_cap", "pstride") == expect


def test_uniform_table_resamples_like_numpy_interp(shim):
    cfg = bench.make_cfg(4, workload="cfg2")
    cc = cfg.to_c()
    pw, ct = (C.c_float * 1024)(), (C.c_float * 1024)()
    x0, dx = C.c_double(), C.c_double()
    n = shim.lib.plan_table(C.byref(cc), pw, ct, C.byref(x0), C.byref(dx))      # V80: 1 m/s steps — used as it is
    assert n == cc.n_tab and dx.value == 1.0 and np.array_equal(np.array(pw[:n]), np.asarray(cfg.tab.power_tab, np.float32))
    ws = np.array([3.0, 4.0, 6.5, 7.0, 11.0, 12.5, 25.0])
    p_t, c_t = np.array([0.0, 60e3, 400e3, 500e3, 1.9e6, 2e6, 2e6]), np.array([0.0, 0.82, 0.8, 0.79, 0.5, 0.3, 0.05])
    keep = [np.ascontiguousarray(a) for a in (ws, p_t, c_t)]
    cc.n_tab = len(ws)
    cc.tab_ws, cc.tab_power, cc.tab_ct = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in keep)
    n = shim.lib.plan_table(C.byref(cc), pw, ct, C.byref(x0), C.byref(dx))
    assert n == 1024 and x0.value == 3.0 and dx.value == (25.0 - 3.0) / 1023
    x = np.minimum(3.0 + np.arange(1024) * dx.value, 25.0)
    assert np.allclose(np.array(pw[:n]), np.interp(x, ws, p_t), rtol=1e-6) and np.allclose(np.array(ct[:n]), np.interp(x, ws, c_t), rtol=1e-6, atol=1e-7)
    d = shim(cc)
    assert pick(d, "n_tab", "tab_x0") == (1024, 3.0) and d["tab_dx"] == dx.value


# ---- the box rule: a box of 2^28 cells or more runs on the per-slot kernels, a smaller one set later gets the env kernel back --------
def test_step_path_follows_the_boxes_set(shim):
    c5 = bench.make_cfg(1024, workload="cfg5")
    assert pick(shim(c5, box_cells=2048 * 512 * 64), "path_envw", "path_fused") == (1, 1)
    for kw in ({"box_cells": 1 << 28}, {"box_cells": 4096, "abox_cells": 1 << 28}):
        d = shim(c5, **kw)
        assert pick(d, "path_envw", "path_fused", "envw_eligible", "fused_eligible") == (0, 0, 1, 1)
    assert pick(shim(c5, box_cells=(1 << 28) - 1, abox_cells=4096), "path_envw", "path_fused") == (1, 1)
    assert shim(bench.make_cfg(1024, workload="cfg2"), box_cells=1 << 28)["path_envw"] == 1      # steady inflow reads no box
    assert pick(shim(c5, box_cells=64, step_fused=0), "path_envw", "path_fused") == (1, 0)
