"""The sensor rules — `current`, the rolling mean over min(window, history, pushed) samples, the partly filled deques of
fill_window False / 3 — by value against the fp64 oracle on every step path: tests/sensor_cases.py's table, fourteen paths times
the sensor sets short (W < H, W == 1), beyond (W > H, H == 1, H == 2), current (no running sum) and generic (TI, farm-level
entries, several windows per channel), each with full and partial fills, and three extra cases (a state restored mid-fill and
after a rollover, the per-agent buffer switched on and off on running sums, the double clock).  tests/test_sensor_cases.py pins on
the CPU that the table reaches every path with every geometry and that each comparison made here can fail.  Each case checks that
its handle runs the variant the plan names, then compares at reset and at EVERY step: truncation flags (exact), observations,
final observations, per-agent rows where registered, reward; and measurements() — the unscaled values, build_obs' `raw` path,
scaled here on the host — at reset and every 10th step, on the entries the oracle does not clip.  Bars: the project's own
(variant_census.obs_atol, rule_cases.reward_bar), none fitted to what the kernels give.

The worst error per quantity is printed per case (pytest -s; one run's lines: profiles/sensor_cases_errors.txt) as worst |d| and
as its ratio to the bar, atol + rtol |reference|; a case asserts after its whole run that every ratio is <= 1.

No case found a wrong kernel.  What the table notices, tried once on a library built with deliberate value errors (none moves an
address out of a ring):
  * the leaving sample of wg_sums_load taken at np - Wc + 1: every sums-mode case with a rolling mean fails on obs / final_obs —
    56 of the 70 cases of the table as it stood then, all but the ring-staging cases of path 4 and the `current` cases;
  * wg_sums_mean dividing by min(W, H) while the window fills: every sums-mode case with a rolling mean AND a partial fill fails,
    33 cases (every p*-short-f1 / -f3, p*-beyond-f1 / -f3, the partly filled generic cases, x-restore, x-multi-window,
    x-short-extra-inc), no full-fill case does;
  * lean_swap summing ring_cap samples instead of min(sum_w, n_pushed): at first NO case failed — on compact rings the flow kernel
    prepares a resting background episode's sums again in every launch, also after set_state, so the swap's own sums never run
    there.  They run on uniform rings, where nothing is prepared (the plan's first_obs is 0): path 14 was added for it, and
    p14-short-f3 and p14-65-short-f3 fail (obs, final_obs), the other 68 pass.  (With a fill of 1 the error is invisible: the
    ring is zeroed and every window holds the one sample there is.  Hence fill 3.)
  * the same error in the prepared first observation (wg_first_obs and env_first_obs: cnt = ring_cap): 41 cases fail, among them
    every full-fill short / beyond case of paths 1 - 3 and 5 - 12.
(The first two were run before path 14 replaced two cases of path 12; their lists name classes of cases for that reason.)"""
import time

import numpy as np
import pytest

import rule_cases as rc
import sensor_cases as sc
import variant_census as vc
from helpers import hip, make_batch  # noqa: F401  (hip: the fixture)
from test_gpu_rule_cases import Worst
from test_gpu_variant_census import CASE_TIME_LIMIT_S, _guarded, time_limit
from test_plan import shim  # noqa: F401  (the g++-only plan fixture)

pytestmark = pytest.mark.gpu

MEASURE_EVERY = 10
_REF = {}


def _reference(oracle_lib, cs):
    """one oracle trajectory per config, shared by the cases that differ in what the handle is asked to do only; read-only"""
    if cs.ref_id() not in _REF:
        _REF[cs.ref_id()] = sc.reference(oracle_lib, cs)
    return _REF[cs.ref_id()]


def _run(hip, shim, cs, ref):  # noqa: F811
    import torch
    cfg = cs.cfg()
    plan = sc.plan_of(shim, cs)
    assert plan["rc"] == 0 and sc.path_of(cs, plan) == cs.path
    env = make_batch(hip, cfg, {vc.HOOK_ENV[k]: str(v) for k, v in cs.hooks}, variant=rc.variant_of(plan))
    rc.install(cs, env)
    buf = env.fuse_obs_multi() if cs.multi else None
    atol, w = vc.obs_atol(cs), Worst()
    rbar = rc.reward_bar(cs, ref)
    mn, rng = sc.raw_scale(cs)

    def measured(want):
        """measurements(), scaled on the host, against the oracle's observation where the oracle does not clip"""
        raw = env.measurements().cpu().numpy().astype(np.float64)
        w.add("measured", 2.0 * (raw - mn) / rng - 1.0, want, atol, where=np.abs(want) < 1.0)

    w.add("obs", env.reset(seeds=sc.seeds_of(cs)).cpu().numpy(), ref["obs0"], atol)
    env.check()
    if buf is not None:
        w.add("obs_multi", buf.cpu().numpy(), ref["multi0"], atol)
    measured(ref["obs0"])
    acts = torch.as_tensor(ref["actions"].copy(), device="cuda")
    for k in range(cs.steps):
        if k in cs.restore_at:
            env.set_state(env.get_state())
        if cs.multi_window and k == cs.multi_window[0]:
            buf = env.fuse_obs_multi()
        if cs.multi_window and k == cs.multi_window[1]:
            buf = env.fuse_obs_multi(False)
        obs, rew, tr, fin = env.step(acts[k])
        np.testing.assert_array_equal(tr.cpu().numpy().astype(bool), ref["tr"][k], err_msg=f"{cs.name}: truncation flags, step {k}")
        w.add("obs", obs.cpu().numpy(), ref["obs"][k], atol)
        w.add("final_obs", fin.cpu().numpy(), ref["fin"][k], atol)
        if buf is not None:
            w.add("obs_multi", buf.cpu().numpy(), ref["multi"][k], atol)
        w.add("reward", rew.cpu().numpy(), ref["rew"][k], **rbar)
        if k % MEASURE_EVERY == 0:
            measured(ref["obs"][k])
    env.check()
    env.close()
    return w, rbar


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_sensors_match_oracle_on_every_step_path(hip, oracle_lib, shim, name):  # noqa: F811
    cs = sc.case(name)
    t0 = time.perf_counter()
    with time_limit(CASE_TIME_LIMIT_S):
        ref = _reference(oracle_lib, cs)
        w, rbar = _guarded(_run, hip, shim, cs, ref)
    print(f"\n[sensor cases] {name:22s} path {cs.path:2d} {str(vc.key_of(cs, sc.plan_of(shim, cs))):52s} fill {sc.fill_steps(cs):2d} "
          f"{time.perf_counter() - t0:5.2f} s  {w.row()}")
    assert not w.missed(), (name, w.missed())
