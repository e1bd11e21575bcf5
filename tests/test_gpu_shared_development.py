"""Shared development of a background episode (k_flow_env): while a not-yet-live episode develops, its baseline
farm is an exact twin of its agent farm (same wind, same initial yaws, no controller), so the kernel parks the baseline slot,
develops the agent slot alone and clones it when its development steps are done.  WG_ENV_SHARE_DEV=0 is the kernel that
develops both farms.  Everything a caller can see must be BIT-identical between the two — no tolerance anywhere: the twin is the
same arithmetic on the same bits — for every instantiation (one / two waves per env, pass waves, fused / unfused step), with
different fill lengths of the two farms, across a checkpoint taken while slots are parked, and for the per-slot kernels that
continue from such a checkpoint.  And the work must really be gone: the device's own flow-step counters say so."""
import math

import numpy as np
import pytest

from helpers import ab_actions, ab_cases, hip, make_ab, same_fields  # noqa: F401  (hip: the fixture)

pytestmark = pytest.mark.gpu

# kernel instantiations: one wave per env, two, a pass wave for the running episode's context, pass waves for both
VARIANTS = {
    "wpe1": {"WG_ENV_WPE": "1"},
    "wpe2": {"WG_ENV_WPE": "2", "WG_ENV_SPLIT": "0"},
    "split1": {"WG_ENV_WPE": "2", "WG_ENV_SPLIT": "1"},
    "split2": {"WG_ENV_WPE": "2", "WG_ENV_SPLIT": "2"},
}


ENV_KERNEL = (None, None, 2)      # flow_variant() of a handle on k_flow_env, whatever its threads and rings


def _hooks(variant, fused, share):
    return {"WG_FLOW_ENV": "1", "WG_STEP_FUSED": "1" if fused else "0", "WG_ENV_SHARE_DEV": "1" if share else "0", **VARIANTS[variant]}


def _lockstep(a_env, b_env, acts, s0, s1, multi=False, fields_every=50):
    """steps s0 .. s1 - 1 of both handles on the same actions, every output bit for bit; -> truncations"""
    import torch
    n_tr = 0
    for s in range(s0, s1):
        ra, rb = a_env.step(acts[s % 64]), b_env.step(acts[s % 64])
        assert torch.equal(ra[2], rb[2]), f"truncation flags differ at step {s}"
        assert torch.equal(ra[0], rb[0]), f"obs step {s}"
        assert torch.equal(ra[1], rb[1]), f"reward step {s}"
        assert torch.equal(ra[3], rb[3]), f"final obs step {s}"
        if multi:
            assert torch.equal(a_env._multi_buf, b_env._multi_buf), f"per-agent buffer step {s}"
        n_tr += int(ra[2].sum())
        if s % fields_every == fields_every - 1:
            same_fields(a_env, b_env, f"step {s}")
    return n_tr


def _on_off(hip, case, B, variant, fused, steps, **over):
    import torch
    d, kw, multi = ab_cases()[case]
    kw = {**kw, **over}
    cfg, a_env = make_ab(hip, d, B, _hooks(variant, fused, True), multi=multi, variant=ENV_KERNEL, **kw)
    _, b_env = make_ab(hip, d, B, _hooks(variant, fused, False), multi=multi, variant=ENV_KERNEL, **kw)
    seeds = 900 + np.arange(B)
    assert torch.equal(a_env.reset(seeds=seeds), b_env.reset(seeds=seeds)), "reset obs"
    same_fields(a_env, b_env, "after reset")
    a_env.check(); b_env.check()
    n_tr = _lockstep(a_env, b_env, ab_actions(cfg, B), 0, steps, multi=multi)
    same_fields(a_env, b_env, "end")
    a_env.check(); b_env.check()          # (an episode that is not ready at its swap latches the status word)
    a_env.close(); b_env.close()
    return n_tr


PAIRS = [(c, B, v, f) for c in ("cfg2_4x4", "cfg4_3x3_per_agent_buffer", "two_turb_noise_K", "cfg2_one_farm") for B in (64, 389)
         for v in VARIANTS for f in (True, False)]


@pytest.mark.parametrize("case,B,variant,fused", PAIRS)
def test_sharing_on_equals_off_bit_for_bit(hip, case, B, variant, fused):
    n_tr = _on_off(hip, case, B, variant, fused, 400)
    assert n_tr >= B                                   # every env rolled over at least once on average


@pytest.mark.parametrize("fill_window", [False, 7])
@pytest.mark.parametrize("variant", ["wpe1", "wpe2", "split2"])
def test_farms_with_different_fill_lengths(hip, fill_window, variant):
    """fill_window=False / an integer below hist_max: the agent farm fills 1 / 7 env steps, the baseline farm hist_max — its fill
    only starts at the clone, and the episode must still be ready WG_SHADOW_MARGIN steps before the truncation (check())."""
    d, kw, _ = ab_cases()["cfg2_4x4"]
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    cfg = EnvConfig(turbine=V80(), yaml_dict=d, turbtype="None", n_envs=4, fill_window=fill_window, **kw)
    assert cfg.steps_on_reset < cfg.hist_max
    n_tr = _on_off(hip, "cfg2_4x4", 64, variant, True, 400, fill_window=fill_window)
    assert n_tr >= 64


@pytest.mark.parametrize("variant", ["wpe1", "wpe2", "split2"])
def test_checkpoint_with_parked_slots_replays(hip, variant):
    """get_state() at several offsets inside the episodes (slots are parked for ~40 % of every env's steps; B = 64 envs with
    different winds: every offset catches parked ones), restored into a fresh handle:
    the continuation equals the uninterrupted run bit for bit, through the next rollovers."""
    import torch
    d, kw, _ = ab_cases()["cfg2_4x4"]
    B = 64
    cfg, ref = make_ab(hip, d, B, _hooks(variant, True, True), variant=ENV_KERNEL, **kw)
    seeds = 40 + np.arange(B)
    ref.reset(seeds=seeds)
    acts = ab_actions(cfg, B, seed=11)
    outs, blobs = [], {}
    for s in range(420):
        if s in (30, 95, 170):
            blobs[s] = ref.get_state()
        outs.append([x.clone() for x in ref.step(acts[s % 64])])
    ref.check()
    for s0, blob in blobs.items():
        _, env = make_ab(hip, d, B, _hooks(variant, True, True), variant=ENV_KERNEL, **kw)
        env.reset(seeds=seeds + 1000)              # (another state, overwritten by the blob)
        env.set_state(blob)
        for s in range(s0, 420):
            r = env.step(acts[s % 64])
            for x, y, what in zip(r, outs[s], ("obs", "reward", "truncated", "final obs")):
                assert torch.equal(x, y), f"checkpoint at {s0}: {what} differs at step {s}"
        env.check()
        env.close()
    ref.close()


def test_per_slot_kernels_continue_from_a_parked_checkpoint(hip):
    """A parked baseline slot (never stepped, its agent twin part-way through its development) is a legal state for every
    kernel: the blob goes into a handle that runs the per-slot kernels (WG_FLOW_ENV=0, same layout), which develop the slot
    on their own.  Through the next rollover of every env: check() clean, decisions exact, values within the 1e-5 the
    k_flow_env / k_flow pair is held to (tests/test_gpu_variant_ab.py, "gl")."""
    import torch
    d, kw, _ = ab_cases()["cfg2_4x4"]
    B = 64
    cfg, a_env = make_ab(hip, d, B, _hooks("wpe1", False, True), variant=ENV_KERNEL, **kw)
    _, b_env = make_ab(hip, d, B, {"WG_FLOW_ENV": "0"}, variant=(None, None, 0), **kw)
    seeds = 77 + np.arange(B)
    a_env.reset(seeds=seeds); b_env.reset(seeds=seeds + 5)
    acts = ab_actions(cfg, B, seed=3)
    for s in range(60):
        a_env.step(acts[s % 64])
    b_env.set_state(a_env.get_state())
    n_tr = 0
    for s in range(60, 520):
        ra, rb = a_env.step(acts[s % 64]), b_env.step(acts[s % 64])
        assert torch.equal(ra[2], rb[2]), f"truncation flags differ at step {s}"
        for x, y, what, atol in ((ra[0], rb[0], "obs", 1e-5), (ra[1], rb[1], "reward", 2e-5), (ra[3], rb[3], "final obs", 1e-5)):
            fx, fy = x.float(), y.float()
            assert ((fx - fy).abs() <= atol + 1e-5 * fy.abs()).all(), (what, s, float((fx - fy).abs().max()))
        n_tr += int(ra[2].sum())
    assert n_tr >= B
    a_env.check(); b_env.check()
    a_env.close(); b_env.close()


def _n_dev(cfg, ws, wd):
    """development steps of an episode with wind (ws, wd): the set-up's own formula (wg_ctx_init; Wind_Farm_Env.py:723-729)"""
    x, y = np.asarray(cfg.x_pos, float), np.asarray(cfg.y_pos, float)
    th = (270.0 - wd) * (math.pi / 180.0)
    xr = x.mean() + (x - x.mean()) * math.cos(th) + (y - y.mean()) * math.sin(th)
    t_developed = int((xr.max() - xr.min()) / ws * 2)
    return int(math.ceil(t_developed / float(cfg.dt_sim) - 1e-9))


@pytest.mark.parametrize("variant", ["wpe1", "wpe2"])
def test_the_duplicate_flow_steps_are_gone(hip, variant):
    """Farm flow-steps the DEVICE counted (WgSlot::flow_count through kernel_timing) over a window that starts at reset() — where
    every background context is about to be set up: no partial episode at that end — with sharing on, over those with sharing
    off, background share only (the running episodes take 2 K per env step either way).

    Expectation: sum over the episodes that went live inside the window — their development lies wholly inside it — of
    n_dev + K (fill_a + fill_b), over the sum of 2 n_dev + K (fill_a + fill_b); n_dev from the handle's own wind of each of
    those episodes (info "wind_f64", read after every truncation).

    Slack, computed here and not tuned: the window's far end cuts ONE background episode per env, whose wind is not known yet.
    With C_on / C_off the sums over the complete episodes and p_on <= p_off' the parts of the cut ones inside the window,
    |(C_on + p_on) / (C_off + p_off) - C_on / C_off| <= max(p_on, p_off) / (C_off + p_off) <= w, the weight of the cut episodes:
    B x the largest work an episode of this configuration can have with sharing off (the slowest wind along the layout's
    diagonal, as wg_plan_reset_launches bounds it) over all background flow-steps counted with sharing off.  The run is long
    enough for w < 0.2; the ratio itself is ~0.55 against 1 without the change."""
    import torch
    d, kw, _ = ab_cases()["cfg2_4x4"]
    B, steps = 64, 6000
    cfg, a_env = make_ab(hip, d, B, _hooks(variant, True, True), variant=ENV_KERNEL, **kw)
    _, b_env = make_ab(hip, d, B, _hooks(variant, True, False), variant=ENV_KERNEL, **kw)
    seeds = 300 + np.arange(B)
    a_env.reset(seeds=seeds); b_env.reset(seeds=seeds)
    a_env.kernel_timing(True); b_env.kernel_timing(True)          # (marks the counters: the window starts here)
    acts = ab_actions(cfg, B, seed=21)
    K = cfg.sim_steps_per_env_step
    fills = K * (cfg.steps_on_reset + cfg.hist_max)
    num = den = 0
    for s in range(steps):
        ra, rb = a_env.step(acts[s % 64]), b_env.step(acts[s % 64])
        assert torch.equal(ra[2], rb[2])
        tr = ra[2].bool().cpu().numpy()
        if tr.any():
            wind = a_env.info("wind_f64").cpu().numpy()
            for e in np.nonzero(tr)[0]:
                n = _n_dev(cfg, wind[e, 0], wind[e, 1])
                num += n + fills
                den += 2 * n + fills
    a_env.check(); b_env.check()
    ta, tb = a_env.kernel_timing(False), b_env.kernel_timing(False)
    live = 2 * K * B                                               # the running episodes' two farms, every launch
    bg_on, bg_off = (ta[3] - live) * steps, (tb[3] - live) * steps
    assert den > 0 and bg_off > 0
    expect, ratio = num / den, bg_on / bg_off
    diag = math.hypot(float(np.ptp(cfg.x_pos)), float(np.ptp(cfg.y_pos)))
    n_dev_cap = int(math.ceil(2.0 * diag / min(cfg.ws_min, cfg.ws_max) / float(cfg.dt_sim))) + 2
    w = B * (2 * n_dev_cap + fills) / bg_off
    print(f"background flow-steps on / off: {bg_on:.0f} / {bg_off:.0f} = {ratio:.4f}, expected {expect:.4f} +- {w:.4f} "
          f"(largest possible n_dev {n_dev_cap})")
    assert w < 0.2, "window too short for the bound to mean anything"
    assert abs(ratio - expect) <= w
    assert ratio < 0.75                                            # (and well below 1, whatever the slack)
    # particles the advection passes touched fall with the flow-steps
    assert ta[4] < tb[4]
    a_env.close(); b_env.close()


def test_one_farm_handle_is_untouched(hip):
    """F = 1: no baseline farm, the flag is off whatever the hook says — same flow-step count, same state blob."""
    d, kw, _ = ab_cases()["cfg2_one_farm"]
    B = 64
    cfg, a_env = make_ab(hip, d, B, _hooks("wpe1", True, True), variant=ENV_KERNEL, **kw)
    _, b_env = make_ab(hip, d, B, _hooks("wpe1", True, False), variant=ENV_KERNEL, **kw)
    seeds = 5 + np.arange(B)
    a_env.reset(seeds=seeds); b_env.reset(seeds=seeds)
    a_env.kernel_timing(True); b_env.kernel_timing(True)
    _lockstep(a_env, b_env, ab_actions(cfg, B), 0, 300)
    assert a_env.kernel_timing(False)[3] == b_env.kernel_timing(False)[3]
    assert a_env.get_state() == b_env.get_state()
    a_env.close(); b_env.close()
