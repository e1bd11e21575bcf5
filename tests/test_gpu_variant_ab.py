"""Kernel-variant A/Bs on identical seeds and actions (these lived in tools/env_vs_gl.py, which the driver
never runs).  Every pair runs the SAME handle configuration through two kernel variants selected with the debug hooks:

  fused   step() as ONE launch (k_flow_env with the glue as its tail)  vs  flow launch + k_glue_lean      -> bit-identical
  wpe     two waves per env (one per context)                          vs  one wave per env               -> bit-identical
  split   a third wave per env runs the advection pass of the          vs  the same two-wave kernel       -> bit-identical,
          running episode's context and fetches the glue's step-              without it                        state blobs too
          independent inputs ahead (default at 513 .. 1024 envs for
          farms with long chains); split_both: a fourth wave does the
          background context's pass (default at <= 512 envs)
  gl      k_flow_env (lane = farm slot x turbine)                      vs  k_flow GL (one farm slot per workgroup)
          same state layout, arithmetic and summation orders; the compiler contracts a few products differently, so the
          flow values agree to the last bits (held to 1e-5 relative over hundreds of steps), decisions (truncation) exactly

at B = 64 and B = 389 (not a multiple of anything) through several episode rollovers, + one 5000-step run of the fused pair
(the glue's header / deque loads are plain global loads now, wg_glue_lean.h: what used to rest on a register pin)."""
import numpy as np
import pytest

from helpers import FIELDS, ab_actions, ab_cases, hip, make_ab, make_batch, same_fields  # noqa: F401  (hip: the fixture)
from windgym_amd.binding import debug_hooks

pytestmark = pytest.mark.gpu


def _pair(mode):
    """hooks of the (a, b) handles and whether the pair must agree bit for bit"""
    if mode == "fused":
        return {"WG_FLOW_ENV": "1", "WG_STEP_FUSED": "1"}, {"WG_FLOW_ENV": "1", "WG_STEP_FUSED": "0"}, True
    if mode == "wpe":
        return {"WG_FLOW_ENV": "1", "WG_ENV_WPE": "2"}, {"WG_FLOW_ENV": "1", "WG_ENV_WPE": "1"}, True
    if mode in ("split", "split_both"):      # (a pass wave for the running episode's context / for both contexts)
        return ({"WG_FLOW_ENV": "1", "WG_ENV_WPE": "2", "WG_ENV_SPLIT": "1" if mode == "split" else "2"},
                {"WG_FLOW_ENV": "1", "WG_ENV_WPE": "2", "WG_ENV_SPLIT": "0"}, True)
    return {"WG_FLOW_ENV": "1"}, {"WG_FLOW_ENV": "0"}, False


def _ab(hip, mode, case, B, steps):
    import torch
    d, kw, multi = ab_cases()[case]
    ha, hb, exact = _pair(mode)
    cfg, a_env = make_ab(hip, d, B, ha, multi=multi, variant=(None, None, 2), **kw)
    _, b_env = make_ab(hip, d, B, hb, multi=multi, variant=(None, None, 0 if mode == "gl" else 2), **kw)

    def same(x, y, what, rtol=1e-5, atol=1e-5):
        if exact:
            assert torch.equal(x, y), what
        else:
            fx, fy = x.float(), y.float()
            assert ((fx - fy).abs() <= atol + rtol * fy.abs()).all(), (what, float((fx - fy).abs().max()))

    seeds = 900 + np.arange(B)
    same(a_env.reset(seeds=seeds), b_env.reset(seeds=seeds), "reset obs")
    same_fields(a_env, b_env, "after reset", same)
    acts = ab_actions(cfg, B, seed=5)
    n_tr = 0
    for s in range(steps):
        ra, rb = a_env.step(acts[s % 64]), b_env.step(acts[s % 64])
        assert torch.equal(ra[2], rb[2]), f"truncation flags differ at step {s}"
        same(ra[0], rb[0], f"obs step {s}")
        same(ra[1], rb[1], f"reward step {s}", atol=2e-5)
        same(ra[3], rb[3], f"final obs step {s}")
        if multi:
            same(a_env._multi_buf, b_env._multi_buf, f"per-agent buffer step {s}")
        n_tr += int(ra[2].sum())
        if s % 50 == 49:
            same_fields(a_env, b_env, f"step {s}", same)
    a_env.check(); b_env.check()
    if mode in ("fused", "split", "split_both"):
        # particles, rings, headers, window sums: the whole state.  (Not for "wpe": one wave per env defers a retired context's
        # episode set-up behind its step, so the BACKGROUND context's development runs a launch behind the two-wave schedule —
        # every output is equal, the not-yet-live episode's intermediate state is not.)
        sa, sb = a_env.get_state(), b_env.get_state()
        assert np.array_equal(np.frombuffer(sa, np.uint8), np.frombuffer(sb, np.uint8)), "state blobs differ"
    a_env.close(); b_env.close()
    return n_tr


# every case at B = 64; the two bench shapes also at the large odd batch
PAIRS = [(m, c, 64) for m in ("fused", "wpe", "gl") for c in ("cfg2_4x4", "cfg4_3x3_per_agent_buffer", "two_turb_noise_K", "cfg2_one_farm")]
PAIRS += [(m, c, 389) for m in ("fused", "wpe", "gl") for c in ("cfg2_4x4", "cfg4_3x3_per_agent_buffer")]
PAIRS += [(m, c, B) for m in ("split", "split_both") for c in ("cfg2_4x4", "cfg4_3x3_per_agent_buffer", "two_turb_noise_K", "cfg2_one_farm")
          for B in (64, 389)]


@pytest.mark.parametrize("mode,case,B", PAIRS)
def test_variant_pairs_agree(hip, mode, case, B):
    n_tr = _ab(hip, mode, case, B, 400)
    assert n_tr >= B                                   # every env rolled over at least once on average


def test_fused_step_equals_two_launches_over_5000_steps(hip):
    """the fused glue's loads are correct by construction now (no scalar-cache reads of words the launch
    writes) — 5000 steps x 64 envs with ~30 rollovers per env, bit for bit against flow + k_glue_lean."""
    n_tr = _ab(hip, "fused", "cfg2_4x4", 64, 5000)
    assert n_tr >= 20 * 64


@pytest.mark.parametrize("wpe", ["4", "2", "1"])
def test_box_env_kernel_agrees_with_the_per_slot_kernel(hip, wpe):
    """k_flow_envb (wg_envb.hip: one launch per step, lanes turbine-major, sample-major deficit phase) against k_flow<64, BOX>
    (one workgroup per farm slot + k_glue_lean) on the SAME state layout, seeds and actions, frozen Mann box with the
    wake-added field on, through rollovers: decisions (truncations, the box-pool draw) exactly, values to float rounding — the
    two kernels sum the rotor points and the wake-added shares in different orders (held to 2e-5 of the scaled observation;
    both are held to the oracle's bars separately, tests/test_gpu_parity.py)."""
    import torch
    from windgym_amd import presets
    from windgym_amd.config import EnvConfig
    from windgym_amd.mann import generate_mann_box
    from windgym_amd.turbine import V80
    d = presets.bench_cfg2_config()
    B = 48
    box, spacing = generate_mann_box((256, 64, 32), (3.0, 3.0, 3.0), seed=1234), (3.0, 3.0, 3.0)

    def make(hooks, variant):
        cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="MannGenerate", n_envs=B, autoreset=True, n_rotor_pts=16,
                        n_passthrough=1, n_particles=128)
        env = make_batch(hip, cfg, hooks, variant=variant)
        env.set_turbulence_box(box, spacing)
        return cfg, env
    cfg, a_env = make({"WG_FLOW_ENV": "1", "WG_ENV_WPE": wpe}, (64, True, 2))
    _, b_env = make({"WG_FLOW_ENV": "0"}, (64, True, 0))
    seeds = 700 + np.arange(B)
    oa, ob = a_env.reset(seeds=seeds), b_env.reset(seeds=seeds)
    assert (oa - ob).abs().max().item() <= 2e-5
    acts = ab_actions(cfg, B, seed=7)
    n_tr = 0
    for s in range(360):
        ra, rb = a_env.step(acts[s % 64]), b_env.step(acts[s % 64])
        assert torch.equal(ra[2], rb[2]), f"truncation flags differ at step {s}"
        assert (ra[0] - rb[0]).abs().max().item() <= 2e-5, s
        assert (ra[3] - rb[3]).abs().max().item() <= 2e-5, s
        assert ((ra[1] - rb[1]).abs() <= 1e-4 + 1e-4 * rb[1].abs()).all(), s
        n_tr += int(ra[2].sum())
        if s % 60 == 59:
            for f in FIELDS:
                x, y = a_env.info(f).float(), b_env.info(f).float()
                tol = 50.0 if f.startswith("power") else 2e-4
                assert ((x - y).abs() <= tol + 1e-4 * y.abs()).all(), (s, f, float((x - y).abs().max()))
    assert n_tr >= B
    a_env.check(); b_env.check()
    a_env.close(); b_env.close()


def test_stencil_records_equal_the_brick_ordered_box_bit_for_bit(hip):
    """k_flow_envb reads a rotor point's 8 box corners from ONE 128-byte stencil record (FlowPtrs::box8 / abox8: 8 x the box in
    HBM) where the pool is small enough, else cell by cell from the brick-ordered box: the same cells with the same weights
    in the same association — every output and the whole state must be BIT-identical (WG_NO_BOX8 keeps the records from being
    built).  A box whose dimensions are not powers of two: the records wrap their indices in double, the bricks with %."""
    import torch
    from windgym_amd import presets
    from windgym_amd.config import EnvConfig
    from windgym_amd.mann import generate_mann_box
    from windgym_amd.turbine import V80
    d = presets.bench_cfg2_config()
    B = 24
    box, spacing = generate_mann_box((240, 72, 40), (3.0, 3.0, 3.0), seed=77), (3.0, 3.0, 3.0)
    envs = []
    for no8 in (False, True):
        cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="MannGenerate", n_envs=B, autoreset=True, n_rotor_pts=16,
                        n_passthrough=1, n_particles=128)
        env = make_batch(hip, cfg, variant=(64, True, 2))
        with debug_hooks({"WG_NO_BOX8": "1"} if no8 else {}):
            env.set_turbulence_box(box, spacing)
            from windgym_amd.mann import default_added_box
            env.set_added_turbulence_box(*default_added_box())
        envs.append(env)
    a_env, b_env = envs
    seeds = 70 + np.arange(B)
    assert torch.equal(a_env.reset(seeds=seeds), b_env.reset(seeds=seeds))
    acts = ab_actions(cfg, B, seed=9, n=32)
    n_tr = 0
    for s_ in range(260):
        ra, rb = a_env.step(acts[s_ % 32]), b_env.step(acts[s_ % 32])
        for x, y in zip(ra, rb):
            assert torch.equal(x, y), s_
        n_tr += int(ra[2].sum())
    assert n_tr >= B
    assert torch.equal(a_env.info("rotor_uvw_agent"), b_env.info("rotor_uvw_agent"))
    assert a_env.get_state() == b_env.get_state()
    a_env.check(); b_env.check()
    a_env.close(); b_env.close()
