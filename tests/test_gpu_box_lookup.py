"""Frozen-box lookups BY VALUE at the box sizes that ship (2^26, 2^27 and 2^28 cells), on WHITE-NOISE boxes.

Every other value-level test of the turbulence boxes runs on a Mann box of at most 2^20 cells.  The reference's boxes are 64 to 256
times larger — record and brick offsets pass 2^31 bytes, the index products of three dimensions pass 2^26, the env kernel hands
over to the per-slot kernels at 2^28 cells — and on a box of independent values per cell a wrong cell, a swapped weight or a missed
wrap is an error of the size of the field (TI U ~ 1 m/s), not a second-order one.  Judges: the float64 numpy reference of
box_reference.py (pinned on the CPU in test_box_reference.py) where the box is read un-shifted ("MannFixed", "MannLoad"), the
float64 C oracle everywhere else.  What is covered, by name: the flow view (k_box_repack + box_lookup_dims: bricks / plain order,
masks / modulo), the rotor points of every box-reading kernel instantiation (stencil records and brick-ordered box of k_flow_envb,
which must also agree bit for bit), the block-averaged meandering copy, the wake-added box, a pool of two boxes, the 2^28 rule.

The big boxes are views of ONE buffer of 3 x 2^28 clipped unit normals drawn on the device (3.2 GB) and copied to the host once
(3.2 GB, the oracle reads it in place): module-scoped, freed when the module ends.
"""
import numpy as np
import pytest

import box_reference as br
from helpers import BLOCKS, hip, make_env, turb_cfg  # noqa: F401  (hip: the fixture)
from windgym_amd.binding import debug_hooks

pytestmark = pytest.mark.gpu

CLIP = 3.0
# Bars of the white-noise comparisons, each with the worst error observed on an MI355X over every test of this module (120-step
# rollouts of 4 to 6 envs; the flow view at 9 coordinate classes x 3072 points).  None is wider than about 4 x its worst case:
FLOW_ATOL = 4e-6        # flow view vs the float64 reference, m/s: worst 1.2e-6 (one float32 ulp of U + TI U g at 8-16 m/s is 9.5e-7)
BARS = dict(
    obs=2e-4,           # scaled observation vs oracle: worst 6.9e-5
    rew=6e-5,           # reward vs oracle: worst 1.6e-5
    uvw=1.5e-3,         # rotor-averaged (u, v, w) vs oracle, m/s: worst 5.1e-4 — the wake deficits in float32 (5e-5 of U), not the
                        # lookups: without wakes the same lookups agree to 1.2e-6 (flow view)
    pow_rtol=5e-4, pow_atol=50.0)      # turbine power vs oracle, W: worst 0.44 of (5e-4 rel + 50 W), 117 W absolute
# The bars IN USE on the Mann box of the parity tests, for the negative control on that box (test_gpu_parity._compare_turb: obs 5e-4,
# reward 1e-3 + 1e-3 rel, rotor wind 2e-3 + 2e-4 rel; test_gpu_spotcheck: power 5e-3 rel + 2000 W), each rounded UP to one absolute
# number (|reward| <= 1, |u| <= 20 m/s): failing these is failing those.  Worst observed on that box with the right cells: obs 9.2e-5,
# reward 1.8e-5, rotor wind 1.73e-3 m/s, power 0.09 of its bar — the rotor-wind bar has no room to tighten there.
MANN_BARS_IN_USE = dict(obs=5e-4, rew=2e-3, uvw=6e-3, pow_rtol=5e-3, pow_atol=2000.0)


@pytest.fixture(scope="module")
def noise(hip):
    """(device tensor, host array) of 3 x 2^28 independent unit normals clipped at 3 sigma, float32"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(2028)
    dev = torch.empty(3 * (1 << 28), dtype=torch.float32, device="cuda")
    dev.normal_(generator=g).clamp_(-CLIP, CLIP)
    host = dev.cpu().numpy()
    yield dev, host
    del dev, host
    torch.cuda.empty_cache()


def _box(noise, shape, k=0):
    """box k of the given shape as views [3, Nx, Ny, Nz] of the noise buffer (device, host): consecutive k do not overlap"""
    n = 3 * int(np.prod(shape))
    assert (k + 1) * n <= noise[1].size
    return noise[0][k * n:(k + 1) * n].view(3, *shape), noise[1][k * n:(k + 1) * n].reshape(3, *shape)


def _set_box(env, orc, box, spacing):
    env.set_turbulence_box(box[0], spacing)
    if orc is not None:
        orc.set_turbulence_box(box[1], spacing)


def _added(seed, shape=(128, 128, 128)):
    """white-noise wake-added box (every handle and oracle of this module gets one: the default is a smooth Mann field)"""
    return br.white_noise_box(shape, seed, clip=CLIP), (3.0, 3.0, 3.0)


class Worst:
    """worst error per quantity of one comparison against `bars`: printed for the record (pytest -rP), asserted by the caller"""

    def __init__(self, bars):
        self.bars = bars
        self.w = dict(obs=0.0, rew=0.0, uvw=0.0, power=0.0, power_abs=0.0)

    def add(self, k, v):
        self.w[k] = max(self.w[k], float(v))

    def ratios(self):
        """worst error / bar per quantity (power: error / (pow_atol + pow_rtol |reference|), the worst over the turbines)"""
        return dict(obs=self.w["obs"] / self.bars["obs"], rew=self.w["rew"] / self.bars["rew"], uvw=self.w["uvw"] / self.bars["uvw"],
                    power=self.w["power"])

    def failing(self):
        return {k: v for k, v in self.ratios().items() if not v <= 1.0}

    def __repr__(self):
        b = self.bars
        return ("worst |obs| %.2e (bar %g)  |reward| %.2e (%g)  |rotor wind| %.2e m/s (%g)  |power| %.1f W, %.3f of (%g rel + %g W)"
                % (self.w["obs"], b["obs"], self.w["rew"], b["rew"], self.w["uvw"], b["uvw"], self.w["power_abs"], self.w["power"],
                   b["pow_rtol"], b["pow_atol"]))


def _compare(env, orc, w):
    """rotor winds of both farms and the turbine powers of the step just taken"""
    for k in ("rotor_uvw_agent", "rotor_uvw_base"):
        w.add("uvw", np.abs(env.info(k).cpu().numpy() - orc.info(k)).max())
    ref = orc.info("power_turb_agent")
    err = np.abs(env.info("power_turb_agent").cpu().numpy() - ref)
    w.add("power_abs", err.max())
    w.add("power", (err / (w.bars["pow_atol"] + w.bars["pow_rtol"] * np.abs(ref))).max())


def _rollout(envs, orc, seeds, steps, act_seed, tag, bars=BARS):
    """reset + `steps` steps of every handle of `envs` and of the oracle on the same seeds and actions; every step compares
    observation, reward, truncation, the rotor winds and the powers of handle 0 with the oracle, and every output of the other handles
    with handle 0 BIT FOR BIT.  Returns the Worst of handle 0 (not yet asserted)."""
    import torch
    B, N = envs[0].B, envs[0].N
    w = Worst(bars)
    obs = [e.reset(seeds=seeds) for e in envs]
    w.add("obs", np.abs(obs[0].cpu().numpy() - orc.reset(seeds=seeds)).max())
    for o in obs[1:]:
        assert torch.equal(o, obs[0]), f"{tag}: reset observation differs between the handles"
    _compare(envs[0], orc, w)
    rng = np.random.default_rng(act_seed)
    for step in range(steps):
        a = rng.uniform(-1, 1, size=(B, N)).astype(np.float32)
        at = torch.as_tensor(a, device="cuda")
        res = [e.step(at) for e in envs]
        o_obs, o_rew, o_tr, o_fin = orc.step(a)
        np.testing.assert_array_equal(res[0][2].cpu().numpy().astype(bool), o_tr, err_msg=f"{tag} step {step}")
        w.add("obs", np.abs(res[0][0].cpu().numpy() - o_obs).max())
        w.add("obs", np.abs(res[0][3].cpu().numpy() - o_fin).max())
        w.add("rew", np.abs(res[0][1].cpu().numpy() - o_rew).max())
        _compare(envs[0], orc, w)
        for r in res[1:]:
            for x, y in zip(r, res[0]):
                assert torch.equal(x, y), f"{tag} step {step}: outputs differ between the handles"
    for e in envs[1:]:
        for k in ("rotor_uvw_agent", "rotor_uvw_base", "power_turb_agent"):
            assert torch.equal(e.info(k), envs[0].info(k)), (tag, k)
    for e in envs:
        e.check()
    print(f"[{tag}] {w!r}")
    return w


def _envb_pair(hip, cfg, block, capfd, set_boxes):
    """two handles on the same env kernel: one reading stencil records, one (WG_NO_BOX8) the brick-ordered box; `set_boxes(env)` installs
    the boxes.  The WG_DEBUG line of build_stencil_records is the witness of which one was built."""
    envs = []
    for no8 in (False, True):
        with debug_hooks({"WG_DEBUG": "1"}):                                # (read at wg_create)
            env = make_env(hip, cfg, block)
        capfd.readouterr()
        with debug_hooks({"WG_NO_BOX8": "1"} if no8 else {}):               # (read by the box setters)
            set_boxes(env)
        err = capfd.readouterr().err
        if no8:
            assert err.count("stencil records not built (WG_NO_BOX8)") == 2, err          # fine box and wake-added box
        else:
            assert "stencil records not built" not in err, err
        envs.append(env)
    return envs


# =====================================================================================================================================
# flow view: k_box_repack + box_lookup_dims<POW2> against the float64 reference
# =====================================================================================================================================
FLOW_SHAPES = [
    pytest.param((256, 64, 32), (3.0, 3.0, 3.0), id="256x64x32-bricks-masks"),
    pytest.param((240, 72, 40), (3.0, 3.0, 3.0), id="240x72x40-bricks-modulo"),
    pytest.param((90, 30, 18), (4.0, 5.0, 6.0), id="90x30x18-plain-modulo"),
    pytest.param((128, 32, 2), (3.0, 3.0, 3.0), id="128x32x2-plain-masks"),
    pytest.param((2048, 512, 64), (3.0, 3.0, 3.0), id="2^26-cells-2048x512x64-bricks-masks"),
    pytest.param((4096, 512, 64), (4.0, 8.0, 8.0), id="2^27-cells-4096x512x64-bricks-masks"),
    pytest.param((2040, 516, 60), (3.0, 3.0, 3.0), id="2^26-cells-2040x516x60-bricks-modulo"),
    pytest.param((2047, 513, 63), (3.0, 3.0, 3.0), id="2^26-cells-2047x513x63-plain-modulo"),
]


def _flow_view_errors(env, e, box_host, spacing, classes):
    """worst |wg_get_windspeed(include_wakes=False) - reference| per coordinate class of env e; the view's grid is x[n] x y[n] at one
    height, so every class is evaluated on the product of its x and y values at three of its heights.  The view takes float32
    coordinates: the reference is given the float32 values the kernel was given."""
    wind = env.info("wind_f64").cpu().numpy()[e]
    ws, ti, t = float(wind[0]), float(wind[2]), float(env.info("fs_time").cpu().numpy()[e])
    worst = {}
    for name, (x, y, z) in classes.items():
        xs, ys = (x + ws * t).astype(np.float32), y.astype(np.float32)
        err = 0.0
        for zz in z[:3]:
            zz = float(np.float32(zz))
            got = env.windspeed(e, xs, ys, z=zz, include_wakes=False).cpu().numpy()
            ref = br.ambient_wind(box_host, spacing, ws, ti, t, xs.astype(np.float64)[:, None], ys.astype(np.float64)[None, :], zz)
            err = max(err, float(np.abs(got - ref).max()))
        worst[name] = err
    return worst


@pytest.mark.parametrize("shape,spacing", FLOW_SHAPES)
def test_flow_view_matches_float64_reference_on_white_noise(hip, noise, shape, spacing):
    """wg_get_windspeed without wakes = U + TI U g(x - U t, y, z) ("MannFixed": un-shifted) at nodes, in the last cell of every axis,
    at negative coordinates and more than ten box lengths away; after the reset and after 300 steps.  Env 0 runs at U = 8 m/s exactly,
    so that its "nodes" are nodes; env 1 at its sampled wind."""
    import torch
    cfg = turb_cfg("MannFixed", 2, nx=2, ny=1)
    env = hip.HipBatch(cfg)
    box = _box(noise, shape)
    _set_box(env, None, box, spacing)
    env.set_added_turbulence_box(*_added(3))
    env.set_wind(ws=np.array([8.0, np.nan]))
    env.reset(seeds=np.array([31, 32]))
    classes = br.coordinate_classes(shape, spacing, np.random.default_rng(1), n=32)
    g = torch.Generator().manual_seed(1)
    worst = {}
    for phase in range(2):
        for e in (0, 1):
            for k, v in _flow_view_errors(env, e, box[1], spacing, classes).items():
                worst[k] = max(worst.get(k, 0.0), v)
        if phase == 0:
            for _ in range(300):
                env.step((torch.rand((2, cfg.n_turb), generator=g) * 2 - 1).cuda())
    assert float(env.info("fs_time")[0]) >= 100.0
    env.check()
    env.close()
    print(f"[flow view {shape}] worst per class (bar {FLOW_ATOL:g}): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= FLOW_ATOL, worst


# =====================================================================================================================================
# rotor points + meandering copy at 2^26 and 2^27 cells: every box-reading instantiation against the float64 oracle
# =====================================================================================================================================
# the reference's own pairs of box and turbtype: MannFixed reads 2048 x 512 x 64 @ 3 m un-shifted, MannGenerate 4096 x 512 x 64 @ (D / 20,
# D / 10, D / 10) at a per-episode offset
BIG = {"2^26-cells": ((2048, 512, 64), (3.0, 3.0, 3.0), "MannFixed"),
       "2^27-cells": ((4096, 512, 64), (4.0, 8.0, 8.0), "MannGenerate")}
STEPS = 120


def _cfg5_shape(turbtype, B):
    cfg = turb_cfg(turbtype, B, nx=4, ny=4)
    assert cfg.n_turb * cfg.n_particles == 2048          # the farm shape bench.py --workload cfg5 runs
    return cfg


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("cells", list(BIG))
def test_rotor_winds_per_slot_kernels_bricks_match_float64_oracle(hip, oracle_lib, noise, cells, block):
    """k_flow<64 / 256, BOX>: rotor points through box_lookup (brick order, 64-bit offsets), particles through the block-averaged
    meandering copy, wake-added turbulence through abox_lookup — 5 envs x 120 steps, every step, on white noise"""
    shape, spacing, turbtype = BIG[cells]
    B = 5
    cfg = _cfg5_shape(turbtype, B)
    env, orc = make_env(hip, cfg, block), oracle_lib.Oracle(cfg)
    _set_box(env, orc, _box(noise, shape), spacing)
    ab = _added(3)
    env.set_added_turbulence_box(*ab), orc.set_added_turbulence_box(*ab)
    w = _rollout([env], orc, 800 + np.arange(B), STEPS, 21, f"{cells} block {block}")
    env.close(), orc.close()
    assert not w.failing(), w


@pytest.mark.parametrize("block", ["envb4", "envb", "envb1"])
@pytest.mark.parametrize("cells", list(BIG))
def test_rotor_winds_env_kernel_records_and_bricks_match_float64_oracle_and_each_other_bit_for_bit(hip, oracle_lib, noise, capfd, cells, block):
    """k_flow_envb with four / two / one wave per env: once reading the stencil records (8.6 GB at 2^26 cells, 17 GB at 2^27: record
    offsets far beyond 2^31 bytes, `ra_ * 8u` close to 2^30), once the brick-ordered box (WG_NO_BOX8) — each against the oracle, and the
    two against each other bit for bit (outputs every step, state at the end)"""
    shape, spacing, turbtype = BIG[cells]
    B = 5
    cfg = _cfg5_shape(turbtype, B)
    box, ab = _box(noise, shape), _added(3)

    def set_boxes(env):
        env.set_turbulence_box(box[0], spacing)
        env.set_added_turbulence_box(*ab)

    envs = _envb_pair(hip, cfg, block, capfd, set_boxes)
    orc = oracle_lib.Oracle(cfg)
    orc.set_turbulence_box(box[1], spacing), orc.set_added_turbulence_box(*ab)
    # the records handle is judged by the oracle, the bricks handle equals it bit for bit: both are judged
    w = _rollout(envs, orc, 800 + np.arange(B), STEPS, 21, f"{cells} {block} records (= bricks)")
    orc.close()
    assert envs[0].get_state() == envs[1].get_state()
    if turbtype == "MannFixed":
        # un-shifted, the rotors sit at x - U t < 0: they read the upper half of the box along x, whose records lie beyond 2^31 bytes
        e = envs[0]
        bx = e.info("turb_x").cpu().numpy().astype(np.float64) - (e.info("wind_f64").cpu().numpy()[:, :1] * e.info("fs_time").cpu().numpy()[:, None])
        i0 = np.mod(np.floor(bx / spacing[0]), shape[0])
        assert (i0 * shape[1] * shape[2] * 128 > 2 ** 31).any() and (i0 * shape[1] * shape[2] * 128 > 2 ** 32).any()
    for e in envs:
        e.close()
    assert not w.failing(), w


@pytest.mark.parametrize("block", [64, "envb4"])
def test_meandering_copy_whose_dims_are_no_powers_of_two_matches_float64_oracle(hip, oracle_lib, noise, block):
    """2040 x 516 x 60 (6.3e7 cells): coarse copy 510 x 129 x 15 — cbox_lookup_vw with modulo, the fine box in bricks with modulo, the
    records wrapped by envb_wrap in double.  The wake centres follow the low-passed transverse inflow: a mis-built or mis-indexed coarse
    copy moves them by metres and the waked rotor winds by several 1e-2 m/s."""
    shape, spacing = (2040, 516, 60), (3.0, 3.0, 3.0)
    B = 5
    cfg = _cfg5_shape("MannGenerate", B)
    env, orc = make_env(hip, cfg, block), oracle_lib.Oracle(cfg)
    _set_box(env, orc, _box(noise, shape), spacing)
    ab = _added(3)
    env.set_added_turbulence_box(*ab), orc.set_added_turbulence_box(*ab)
    w = _rollout([env], orc, 810 + np.arange(B), STEPS, 22, f"meandering 2040x516x60 block {block}")
    # meandering is alive: the wake particles left their turbines' hub height, so the waked rotors see a vertical wind
    assert np.abs(orc.info("rotor_uvw_agent")[..., 2]).max() > 0.01
    env.close(), orc.close()
    assert not w.failing(), w


# =====================================================================================================================================
# wake-added box
# =====================================================================================================================================
@pytest.mark.parametrize("ashape", [pytest.param((160, 144, 132), id="160x144x132-bricks-modulo"),
                                    pytest.param((150, 141, 134), id="150x141x134-plain-modulo")])
def test_wake_added_box_larger_than_the_default_matches_float64_oracle(hip, oracle_lib, capfd, ashape):
    """a white-noise wake-added box of 3.0e6 / 2.8e6 cells (default: 2.1e6) whose dims are no powers of two: abox_lookup of the per-slot
    kernel, abox8 records and the plain / brick-ordered abox4 of k_flow_envb; the added share is first order in the looked-up value"""
    shape, spacing = (256, 64, 32), (3.0, 3.0, 3.0)
    B = 6
    cfg = turb_cfg("MannGenerate", B)
    box = br.white_noise_box(shape, 8, clip=CLIP)
    ab = _added(9, ashape)

    def set_boxes(env):
        env.set_turbulence_box(box, spacing)
        env.set_added_turbulence_box(*ab)

    slot = make_env(hip, cfg, 64)
    set_boxes(slot)
    envs = _envb_pair(hip, cfg, "envb", capfd, set_boxes)
    ws = []
    for hs in ([slot], envs):                # (the brick-ordered handle equals the records handle bit for bit: judged with it)
        orc = oracle_lib.Oracle(cfg)
        orc.set_turbulence_box(box, spacing), orc.set_added_turbulence_box(*ab)
        ws.append(_rollout(hs, orc, 820 + np.arange(B), STEPS, 23, f"added box {ashape} {'per-slot' if hs[0] is slot else 'env kernel'}"))
        orc.close()
    # the added turbulence was looked up: with the added box zeroed the oracle's rotor winds differ
    orc, orc0 = oracle_lib.Oracle(cfg), oracle_lib.Oracle(cfg)
    for o, a in ((orc, ab[0]), (orc0, np.zeros_like(ab[0]))):
        o.set_turbulence_box(box, spacing), o.set_added_turbulence_box(a, ab[1])
        o.reset(seeds=820 + np.arange(B))
    assert np.abs(orc.info("rotor_uvw_agent") - orc0.info("rotor_uvw_agent")).max() > 0.01
    orc.close(), orc0.close()
    for e in [slot] + envs:
        e.close()
    assert not any(w.failing() for w in ws), ws


# =====================================================================================================================================
# box pool: box_cell0 = id x n_cells
# =====================================================================================================================================
def test_pool_of_two_boxes_of_2_26_cells_pinned_to_box_1_matches_reference_and_float64_oracle(hip, oracle_lib, noise, capfd):
    """"MannLoad" with two white-noise boxes of 2^26 cells, every env pinned to box 1 (wg_set_box_ids): box_cell0 = 2^26, the records of
    box 1 start 8.6 GB into the pool's.  Flow view against the reference (the pool is read un-shifted), rotor winds of the per-slot
    kernel, of the records and of the brick-ordered box against the oracle."""
    shape, spacing = (2048, 512, 64), (3.0, 3.0, 3.0)
    B = 5
    cfg = _cfg5_shape("MannLoad", B)
    boxes, ab = [_box(noise, shape, k) for k in (0, 1)], _added(3)
    assert not np.shares_memory(boxes[0][1], boxes[1][1])

    def set_boxes(env):
        env.set_turbulence_boxes([b[0] for b in boxes], spacing)
        env.set_added_turbulence_box(*ab)
        env.set_box_ids(1)

    slot = make_env(hip, cfg, 64)
    set_boxes(slot)
    envs = _envb_pair(hip, cfg, "envb4", capfd, set_boxes)
    seeds = 830 + np.arange(B)
    ws = []
    for hs in ([slot], envs):
        orc = oracle_lib.Oracle(cfg)
        orc.set_turbulence_boxes([b[1] for b in boxes], spacing), orc.set_added_turbulence_box(*ab), orc.set_box_ids(1)
        ws.append(_rollout(hs, orc, seeds, STEPS, 24, f"pool box 1 {'per-slot' if hs[0] is slot else 'env kernel'}"))
        np.testing.assert_array_equal(orc.info("box_id").astype(int), 1)
        orc.close()
    assert envs[0].get_state() == envs[1].get_state()
    classes = br.coordinate_classes(shape, spacing, np.random.default_rng(2), n=24)
    for e in (slot, envs[0]):
        np.testing.assert_array_equal(e.info("box_id").cpu().numpy(), 1)
        worst = _flow_view_errors(e, 2, boxes[1][1], spacing, classes)
        assert max(worst.values()) <= FLOW_ATOL, worst
        # (and it is not box 0 that was read)
        assert max(_flow_view_errors(e, 2, boxes[0][1], spacing, {"interior": classes["interior"]}).values()) > 1e4 * FLOW_ATOL
    for e in [slot] + envs:
        e.close()
    assert not any(w.failing() for w in ws), ws


# =====================================================================================================================================
# the 2^28 rule on the device
# =====================================================================================================================================
def test_box_of_2_28_cells_runs_the_per_slot_kernels_by_value_and_a_smaller_box_restores_the_env_kernel_bit_for_bit(hip, oracle_lib, noise):
    """4096 x 1024 x 64 = 2^28 cells (3.2 GB planar, 4.3 GB interleaved: brick offsets up to 2^32 bytes) on a handle that would run
    k_flow_envb: flow_variant() reports the per-slot kernels, the values match the oracle for 40 steps and the reference in the flow
    view.  Then 256 x 64 x 32: the env kernel is back, and from a common reset the handle equals a fresh handle that only ever saw the
    small box in every output of every step; continued from one state blob, in every byte of the state as well."""
    import torch
    big, big_sp = (4096, 1024, 64), (3.0, 3.0, 3.0)
    B = 4
    cfg = _cfg5_shape("MannFixed", B)
    env, fresh = hip.HipBatch(cfg), hip.HipBatch(cfg)
    assert env.flow_variant() == (64, True, 2)
    box, ab = _box(noise, big), _added(3)
    orc = oracle_lib.Oracle(cfg)
    _set_box(env, orc, box, big_sp)
    env.set_added_turbulence_box(*ab), orc.set_added_turbulence_box(*ab)
    assert env.flow_variant() == (64, True, 0)                       # per-slot kernel + k_glue_lean on the same state layout
    w = _rollout([env], orc, 840 + np.arange(B), 40, 25, "2^28 cells per-slot")
    orc.close()
    classes = br.coordinate_classes(big, big_sp, np.random.default_rng(3), n=24)
    worst = _flow_view_errors(env, 1, box[1], big_sp, classes)
    assert max(worst.values()) <= FLOW_ATOL, worst
    # un-shifted, x - U t < 0 puts the rotors into the upper half of the box along x: brick offsets beyond 2^31 bytes were read
    bx = env.info("turb_x").cpu().numpy().astype(np.float64) - (env.info("wind_f64").cpu().numpy()[:, :1] * env.info("fs_time").cpu().numpy()[:, None])
    assert (np.mod(np.floor(bx / big_sp[0]), big[0]) * big[1] * big[2] * 16 > 2 ** 31).any()
    assert not w.failing(), w
    # a smaller box moves the handle back to the env kernel
    small, sp = br.white_noise_box((256, 64, 32), 8, clip=CLIP), (3.0, 3.0, 3.0)
    for e in (env, fresh):
        e.set_turbulence_box(small, sp)
        e.set_added_turbulence_box(*ab)
        assert e.flow_variant() == (64, True, 2)
        e.metrics(reset_after=True)                                  # (running sums of the steps above: part of the state blob)
    orc = oracle_lib.Oracle(cfg)
    orc.set_turbulence_box(small, sp), orc.set_added_turbulence_box(*ab)
    # from a common reset: every output of every step bit for bit, through at least one rollover of every env
    w = _rollout([env, fresh], orc, 850 + np.arange(B), 200, 26, "after 2^28: small box, env kernel")
    assert int(env.info("episode").min()) >= 1
    # The state blob carries bytes no output depends on: measured here, 4822 of its 878612 bytes (from inside the first particle-ring
    # array onwards) differ between these two handles with different pasts, while every output stayed bit-identical over 420 steps and
    # two rollovers of every env.  So the blobs are compared from ONE blob onwards: both handles continue from the fresh handle's
    # state, and after 200 more steps and another rollover every byte must agree.
    blob = fresh.get_state()
    env.set_state(blob), fresh.set_state(blob)
    g = torch.Generator().manual_seed(4)
    for step in range(200):
        a = (torch.rand((B, cfg.n_turb), generator=g) * 2 - 1).cuda()
        for x, y in zip(env.step(a), fresh.step(a)):
            assert torch.equal(x, y), step
    assert int(env.info("episode").min()) >= 2
    env.check(), fresh.check()
    a, b = np.frombuffer(env.get_state(), np.uint8), np.frombuffer(fresh.get_state(), np.uint8)
    diff = np.flatnonzero(a != b) if a.size == b.size else None
    assert diff is not None and diff.size == 0, (a.size, b.size, None if diff is None else (diff.size, diff[:8], diff[-8:]))
    orc.close(), env.close(), fresh.close()
    assert not w.failing(), w


# =====================================================================================================================================
# negative control: the comparisons above can see a one-cell error
# =====================================================================================================================================
@pytest.mark.parametrize("axis", ["z", "x"])
@pytest.mark.parametrize("field", ["white-noise", "mann"])
def test_negative_control_oracle_box_rolled_by_one_cell_fails_every_bar(hip, oracle_lib, field, axis):
    """The oracle (and the reference of the flow view) is handed the handle's box rolled by ONE cell along z / x; the kernels are
    untouched.  The comparison must then fail at the bars in use — on white noise at this module's bars and, as measured, on the Mann
    box of the parity tests at the wider bars those tests use (that field is rough enough at its 3 m grid to show a cell; its reward
    bar sees it by a factor of 1.3 only)."""
    from windgym_amd.mann import generate_mann_box
    shape, spacing = (256, 64, 32), (3.0, 3.0, 3.0)
    box = br.white_noise_box(shape, 8, clip=CLIP) if field == "white-noise" else generate_mann_box(shape, spacing, seed=1234)
    rolled = np.ascontiguousarray(np.roll(box, 1, axis={"x": 1, "z": 3}[axis]))
    B = 5
    cfg = turb_cfg("MannFixed", B)
    ab = _added(3)
    env = hip.HipBatch(cfg)
    env.set_turbulence_box(box, spacing), env.set_added_turbulence_box(*ab)
    bars = BARS if field == "white-noise" else MANN_BARS_IN_USE
    ws = {}
    for name, b in (("same", box), ("rolled", rolled)):
        orc = oracle_lib.Oracle(cfg)
        orc.set_turbulence_box(b, spacing), orc.set_added_turbulence_box(*ab)
        ws[name] = _rollout([env], orc, 700 + np.arange(B), STEPS, 27, f"negative control {field} {axis} {name}", bars)
        orc.close()
    assert not ws["same"].failing(), ws
    # every quantity misses its bar: on white noise by a factor of 90 to 900, on the Mann box by 1.3 (reward) to 100 (rotor wind)
    r = ws["rolled"].ratios()
    assert min(r.values()) > (50.0 if field == "white-noise" else 1.2), r
    classes = {"interior": br.coordinate_classes(shape, spacing, np.random.default_rng(1), n=24)["interior"]}
    assert max(_flow_view_errors(env, 0, box, spacing, classes).values()) <= FLOW_ATOL
    assert max(_flow_view_errors(env, 0, rolled, spacing, classes).values()) > 1e3 * FLOW_ATOL
    env.close()
