"""Shared development of a background episode (FlowP::env_share): where the plan switches it on.  The flag is a
pure function of the configuration and the WG_ENV_SHARE_DEV hook — k_flow_env's handles with a baseline farm, nothing else —
and it must not move a single member of FlowP or the RESET launch count (tests/plan_share_shim.cpp hands both back)."""
import ctypes as C

import pytest

import bench
from helpers import host_shim
from windgym_amd.config import CConfig

HOOKS = ["flow_env", "flow_block", "env_wpe", "env_split", "share_dev"]
OUT = ["env_share", "envw", "env_wpe", "env_split", "reset_launches", "F", "turb_mode"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = host_shim(tmp_path_factory, "plan_share", include_header_dir=True)
    lib.plan_share.argtypes = [C.POINTER(CConfig), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    lib.plan_share_layout.argtypes = [C.POINTER(C.c_int)]

    def plan(cfg, **hooks):
        arr = (C.c_int * 10)()
        for k, v in hooks.items():
            i = HOOKS.index(k)
            arr[2 * i], arr[2 * i + 1] = 1, v
        out = (C.c_int * len(OUT))()
        cc = cfg.to_c()
        assert lib.plan_share(C.byref(cc), arr, 65536, out) == 0
        return dict(zip(OUT, out))

    plan.lib = lib
    return plan


@pytest.mark.parametrize("n_envs", [64, 512, 1024, 2048, 4096, 8192])
def test_on_by_default_for_every_instantiation_of_the_env_kernel(shim, n_envs):
    for workload in ("cfg2", "cfg4"):
        d = shim(bench.make_cfg(n_envs, workload=workload))
        assert (d["envw"], d["F"], d["env_share"]) == (1, 2, 1), (workload, d)


def test_hook_switches_it_off_and_nothing_else(shim):
    cfg = bench.make_cfg(1024, workload="cfg2")
    on, off, on1 = shim(cfg), shim(cfg, share_dev=0), shim(cfg, share_dev=1)
    assert on["env_share"] == 1 and on1 == on and off["env_share"] == 0
    assert {k: v for k, v in off.items() if k != "env_share"} == {k: v for k, v in on.items() if k != "env_share"}
    # with every wave layout the other hooks select
    for hooks in (dict(env_wpe=1), dict(env_wpe=2, env_split=0), dict(env_wpe=2, env_split=1), dict(env_wpe=2, env_split=2)):
        assert shim(cfg, **hooks)["env_share"] == 1 and shim(cfg, share_dev=0, **hooks)["env_share"] == 0


def test_not_eligible_elsewhere(shim):
    # no baseline farm: nothing to clone
    d = shim(bench.make_cfg(1024, farms2=False, workload="cfg2"))
    assert (d["envw"], d["F"], d["env_share"]) == (1, 1, 0)
    assert shim(bench.make_cfg(1024, farms2=False, workload="cfg2"), share_dev=1)["env_share"] == 0
    # frozen-box inflow (k_flow_envb) and the large steady farm (per-slot kernels) keep developing both farms
    d5 = shim(bench.make_cfg(1024, workload="cfg5"))
    assert d5["envw"] == 1 and d5["turb_mode"] != 0 and d5["env_share"] == 0
    assert shim(bench.make_cfg(1024, workload="cfg5"), share_dev=1)["env_share"] == 0
    d3 = shim(bench.make_cfg(64, workload="cfg3"))
    assert (d3["envw"], d3["env_share"]) == (0, 0)
    # a handle the hooks move to the per-slot kernels
    cfg = bench.make_cfg(1024, workload="cfg2")
    assert shim(cfg, flow_env=0)["env_share"] == 0 and shim(cfg, flow_block=64)["env_share"] == 0
    assert shim(cfg, flow_block=64, flow_env=1)["env_share"] == 1


def test_reset_launch_count_does_not_depend_on_the_flag(shim):
    for workload in ("cfg2", "cfg4"):
        cfg = bench.make_cfg(256, workload=workload)
        assert shim(cfg)["reset_launches"] == shim(cfg, share_dev=0)["reset_launches"]


def test_flag_fills_padding_of_the_parameter_block(shim):
    """FlowP is a by-value argument of every flow kernel: the flag sits in the four bytes that used to pad the block in front of
    its first double, so the kernels that do not read it address every member where they always did."""
    out = (C.c_int * 4)()
    shim.lib.plan_share_layout(out)
    inv_p, share, dt_d, size = out
    assert share == inv_p + 4 and dt_d == share + 4 and dt_d % 8 == 0 and size % 8 == 0
