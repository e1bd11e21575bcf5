"""The task rules — action rule, base controller, reward head, action penalty — by value against the fp64 oracle on every step
path: tests/rule_cases.py's table, twelve paths times four rule sets and the extra cases.  tests/test_rule_cases.py pins on the
CPU that the table reaches every path with every rule value and that each comparison made here can fail.  Each case checks that
its handle runs the variant the plan names, then compares at reset and at EVERY step: truncation flags (exact), observations,
final observations, per-agent rows (glue 2), reward, yaw_agent, power_turb_agent, yaw_base where there is a baseline farm; and
metrics() at the end.  Bars: the project's own (rule_cases.py), none fitted to what the kernels give.

The worst error per quantity is printed per case (pytest -s; one run's lines: profiles/rule_cases_errors.txt) as worst |d| and
as its ratio to the bar, atol + rtol |reference|; a case asserts after its whole run that every ratio is <= 1.

No case found a wrong kernel.  What the table notices, tried once on a library built with three deliberate value errors: the sign
of wg_envb.hip's Global branch flipped (p12-w2-D, p12-w4-A fail on yaw_base), lean_step's penalty summed by rows up to N = 32
(p5-20-A, x-change-20 fail on the reward), Power_scaling dropped in the fused tail (p7-A, p8-A, p9-pass1-A, p11-A, p12-w4-A fail on
the reward); the other 52 cases passed."""
import time

import numpy as np
import pytest

import rule_cases as rc
import variant_census as vc
from helpers import hip, make_batch  # noqa: F401  (hip: the fixture)
from test_gpu_variant_census import CASE_TIME_LIMIT_S, _guarded, time_limit
from test_plan import shim  # noqa: F401  (the g++-only plan fixture)

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(oracle_lib, cs):
    """one oracle trajectory per config, shared by the cases that differ in hooks only; read-only"""
    if cs.ref_id() not in _REF:
        _REF[cs.ref_id()] = rc.reference(oracle_lib, cs)
    return _REF[cs.ref_id()]


class Worst:
    """worst |got - want| and worst |got - want| / (atol + rtol |want|) per quantity; NaN must meet NaN (an entry that is NaN on
    one side only counts as infinitely wrong), and a bar of zero admits equality alone"""

    def __init__(self):
        self.q = {}

    def add(self, name, got, want, atol, rtol=0.0, where=None):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        if where is not None:
            got, want = got[where], want[where]
        both_nan = np.isnan(got) & np.isnan(want)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.where(both_nan, 0.0, np.abs(got - want))
            d = np.where(np.isfinite(d), d, np.inf)
            bar = atol + rtol * np.abs(np.where(both_nan, 0.0, want))
            ratio = np.where(d == 0.0, 0.0, d / bar)
        a, r = self.q.get(name, (0.0, 0.0))
        if d.size:
            a, r = max(a, float(d.max())), max(r, float(ratio.max()))
        self.q[name] = (a, r)

    def row(self):
        return "  ".join(f"{k} {a:.2e} ({r:.2f})" for k, (a, r) in self.q.items())

    def missed(self):
        return {k: v for k, v in self.q.items() if not v[1] <= 1.0}


def _run(hip, shim, cs, ref):  # noqa: F811
    import torch
    cfg = cs.cfg()
    plan = rc.plan_of(shim, cs)
    assert plan["rc"] == 0 and rc.path_of(cs, plan) == cs.path
    env = make_batch(hip, cfg, {vc.HOOK_ENV[k]: str(v) for k, v in cs.hooks}, variant=rc.variant_of(plan))
    rc.install(cs, env)
    buf = env.fuse_obs_multi() if cs.multi else None
    atol, w = vc.obs_atol(cs), Worst()
    rbar, ybar = rc.reward_bar(cs, ref), rc.yaw_base_bar(cs)
    w.add("obs", env.reset(seeds=rc.seeds_of(cs)).cpu().numpy(), ref["obs0"], atol)
    env.check()
    if cs.multi:
        w.add("obs_multi", buf.cpu().numpy(), ref["multi0"], atol)
    acts = torch.as_tensor(ref["actions"].copy(), device="cuda")
    for k in range(cs.steps):
        obs, rew, tr, fin = env.step(acts[k])
        np.testing.assert_array_equal(tr.cpu().numpy().astype(bool), ref["tr"][k], err_msg=f"{cs.name}: truncation flags, step {k}")
        w.add("obs", obs.cpu().numpy(), ref["obs"][k], atol)
        w.add("final_obs", fin.cpu().numpy(), ref["fin"][k], atol)
        if cs.multi:
            w.add("obs_multi", buf.cpu().numpy(), ref["multi"][k], atol)
        w.add("reward", rew.cpu().numpy(), ref["rew"][k], **rbar)
        w.add("yaw_agent", env.info("yaw_agent").cpu().numpy(), ref["yaw_agent"][k], rc.YAW_AGENT_ATOL)
        w.add("power_turb", env.info("power_turb_agent").cpu().numpy(), ref["power_turb_agent"][k], **rc.POWER_BAR)
        if cs.n_farms == 2:
            w.add("yaw_base", env.info("yaw_base").cpu().numpy(), ref["yaw_base"][k], **ybar)
    env.check()
    w.add("metrics", env.metrics().cpu().numpy(), ref["metrics"], where=np.isfinite(ref["metrics"]), **rc.METRICS_BAR)
    env.close()
    return w, rbar


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_rules_match_oracle_on_every_step_path(hip, oracle_lib, shim, name):  # noqa: F811
    cs = rc.case(name)
    t0 = time.perf_counter()
    with time_limit(CASE_TIME_LIMIT_S):
        ref = _reference(oracle_lib, cs)
        w, rbar = _guarded(_run, hip, shim, cs, ref)
    print(f"\n[rule cases] {name:18s} path {cs.path:2d} {str(vc.key_of(cs, rc.plan_of(shim, cs))):52s} {time.perf_counter() - t0:5.2f} s  "
          f"reward bar rtol {rbar['rtol']:.0e} atol {rbar['atol']:.2e}  {w.row()}")
    assert not w.missed(), (name, w.missed())
