"""Shared helpers of the tests: golden fixtures -> EnvConfig and scripted tables; the `hip` fixture and handles under kernel-variant
hooks (make_batch); the case table of the variant A/B tests; the gcc layout probe and the g++ host shims.  (torch is imported where
it is used: the CPU tests import this module too.)"""
import ctypes
import glob
import json
import os
import subprocess

import numpy as np
import pytest

from windgym_amd.binding import debug_hooks
from windgym_amd.config import EnvConfig
from windgym_amd.turbine import V80

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CSRC = os.path.join(ROOT, "windgym_amd", "csrc")
GOLDEN = os.path.join(TESTS, "golden")


# ---- the device ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    """the binding with its library loaded, on a machine with a device (a test file takes it with `from helpers import hip`)"""
    import torch
    from windgym_amd import binding
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    binding.load_library()
    return binding


def make_batch(hip, cfg, hooks=None, variant=None, multi=False):
    """HipBatch of cfg created under the WG_* hooks (read at wg_create).  variant: what flow_variant() of the handle must be —
    (threads, compact rings, 2 for an env kernel / 0 for the per-slot k_flow), None in a place the caller leaves open: the variant
    asked for is the one that runs, a silent fallback would test the wrong kernel.  multi: the per-agent buffer is registered."""
    with debug_hooks(hooks or {}):
        env = hip.HipBatch(cfg)
    if variant is not None:
        got = env.flow_variant()
        assert len(variant) == len(got) and all(w is None or w == g for w, g in zip(variant, got)), (got, variant)
    if multi:
        env.fuse_obs_multi()
    return env


# ---- the oracle parity tests: their bar, their two small configs, a handle on a named flow kernel ------------------------------------------
OBS_ATOL = 2e-4
# every k_flow variant the host can select for a small farm (wg_flow.hip's launch table): one workgroup per farm slot, 64 threads on
# compact rings or 256 threads on uniform rings
BLOCKS = [64, 256]


def make_env(hip, cfg, block=None):
    """HipBatch whose flow kernel is the given instantiation: a thread count of BLOCKS (the per-slot k_flow), "env..." = an env kernel
    with two waves per env, one ("...1") or four ("...4"); None: whatever the plan chooses."""
    if block is None:
        return hip.HipBatch(cfg)
    envk = isinstance(block, str) and block.startswith("env")
    hooks = {"WG_FLOW_BLOCK": "64" if envk else str(block), "WG_FLOW_ENV": "1" if envk else "0"}
    if envk:
        hooks["WG_ENV_WPE"] = block[-1] if block[-1] in "14" else "2"
    return make_batch(hip, cfg, hooks, variant=(64, True, 2) if envk else (block, None, 0))


def physics_cfg(n_envs, autoreset, n_passthrough, nx=4, ny=4, n_particles=None, **over):
    _, meta = load_golden("env1")
    d = meta["cfg"]
    d["farm"].update(nx=nx, ny=ny)
    d["ActionMethod"] = "yaw"
    for k, v in over.items():
        d[k].update(v) if isinstance(v, dict) else d.__setitem__(k, v)
    return EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=n_envs, autoreset=autoreset,
                     n_passthrough=n_passthrough, n_particles=n_particles, n_rotor_pts=16)


def turb_cfg(turbtype, n_envs, autoreset=True, n_passthrough=1.0, nx=3, ny=2):
    from windgym_amd.presets import env1_config
    d = env1_config()
    d["ActionMethod"] = "yaw"
    d["farm"].update(nx=nx, ny=ny)
    d["mes_level"].update(turb_wd=True, turb_TI=True)
    d["wd_mes"].update(wd_rolling_mean=True)
    return EnvConfig(turbine=V80(), yaml_dict=d, turbtype=turbtype, n_envs=n_envs, autoreset=autoreset,
                     n_passthrough=n_passthrough, n_rotor_pts=16)


# ---- the variant A/B tests: one case table, one comparison of the flow fields, one action table -----------------------------------------
FIELDS = ["yaw_agent", "yaw_base", "rotor_uvw_agent", "rotor_uvw_base", "power_turb_agent", "power_turb_base"]


def ab_cases():
    """name -> (yaml dict, EnvConfig keywords, per-agent buffer)"""
    from windgym_amd import presets
    return {
        "cfg2_4x4": (presets.bench_cfg2_config(), dict(n_passthrough=1, n_particles=128), False),
        "cfg4_3x3_per_agent_buffer": (presets.multi_3x3_config(), dict(n_passthrough=0.5, n_particles=96, extra_timestep_inc=True), True),
        "two_turb_noise_K": (presets.two_turb_config(), dict(n_passthrough=1), False),
        "cfg2_one_farm": (presets._upd(presets.bench_cfg2_config(), power_def=dict(Power_reward="Power_avg")),
                          dict(n_passthrough=1, n_particles=128), False),
    }


def make_ab(hip, d, B, hooks, multi=False, variant=None, **kw):
    """-> (cfg, handle) of an A/B case at B envs: steady inflow, autoreset, 16 rotor points"""
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=B, autoreset=True, n_rotor_pts=16, **kw)
    return cfg, make_batch(hip, cfg, hooks, variant=variant, multi=multi)


def _equal(x, y, what, **_):
    import torch
    assert torch.equal(x, y), what


def same_fields(a_env, b_env, tag, same=_equal):
    """every flow field of FIELDS of the two handles through same(x, y, what, atol=) — bit for bit unless the caller brings its own"""
    for f in FIELDS:
        try:
            x, y = a_env.info(f), b_env.info(f)
        except Exception:  # noqa: BLE001  (one-farm configurations have no baseline fields)
            continue
        same(x, y, f"{tag}: {f}", atol=20.0 if f.startswith("power") else 1e-5)


def ab_actions(cfg, B, seed=5, n=64):
    """n action rows [B, n_turb], uniform in [-1, 1) from a seeded CPU generator, on the device"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand((n, B, cfg.n_turb), generator=g) * 2 - 1).cuda()


# ---- host-side C / C++ ------------------------------------------------------------------------------------------------------------------
def c_layout(struct_name, fields, tmp_path):
    """{"sizeof": sizeof(struct_name), field: offsetof(struct_name, field), ...} of a struct of include/windgym_hip.h as gcc sees it"""
    body = "\n".join(f'printf("{f} %zu\\n", offsetof({struct_name}, {f}));' for f in fields)
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/windgym_hip.h"\n'
                   f'int main(void) {{ printf("sizeof %zu\\n", sizeof({struct_name}));\n{body}\nreturn 0; }}\n')
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def host_shim(tmp_path_factory, name, include_header_dir=False):
    """tests/<name>_shim.cpp as a ctypes.CDLL, built by g++ alone with no ROCm include path: what it includes must stay free of HIP
    headers.  include_header_dir: the shim also includes the public header (include/)."""
    so = tmp_path_factory.mktemp(name) / f"{name}_shim.so"
    inc = ["-I", os.path.join(ROOT, "include")] if include_header_dir else []
    subprocess.run(["g++", "-std=c++17", "-shared", "-fPIC", *inc, "-I", CSRC, os.path.join(TESTS, f"{name}_shim.cpp"), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def golden_cases():
    return sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN, "glue_*.npz")))


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, f"glue_{name}.npz"), allow_pickle=False)
    meta = json.loads(str(g["meta"]))
    return g, meta


def config_from_meta(meta, n_envs=1, autoreset=False, **over):
    kw = dict(meta["kwargs"])
    kw.update(over)
    return EnvConfig(turbine=V80(), yaml_dict=meta["cfg"], turbtype="None", n_envs=n_envs, autoreset=autoreset,
                     extra_timestep_inc=bool(meta["multi"]), n_rotor_pts=4, n_particles=32, **kw)


def script_tables(g, n_envs=1):
    """[F,T,B,N,(3)] tables from the golden script; every env of the batch replays the same rows."""
    # the PettingZoo facade resets once inside its constructor (consuming rows) before the recorded reset
    c0, c1 = int(g["cursor0"][0]), int(g["cursor1"][0])
    s0u, s0p, s1u, s1p = g["script0_uvw"][c0:], g["script0_power"][c0:], g["script1_uvw"][c1:], g["script1_power"][c1:]
    T = max(s0u.shape[0], s1u.shape[0])

    def pad(a):
        if a.shape[0] < T:
            a = np.concatenate([a, np.repeat(a[-1:], T - a.shape[0], axis=0)], axis=0)
        return a

    uvw = np.stack([pad(s0u), pad(s1u)])[:, :, None]      # [2,T,1,N,3]
    pw = np.stack([pad(s0p), pad(s1p)])[:, :, None]       # [2,T,1,N]
    uvw = np.repeat(uvw, n_envs, axis=2)
    pw = np.repeat(pw, n_envs, axis=2)
    return np.ascontiguousarray(uvw), np.ascontiguousarray(pw)
