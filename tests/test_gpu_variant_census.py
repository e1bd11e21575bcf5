"""Every built instantiation of the three step kernels (k_flow, k_flow_env, k_flow_envb: tests/variant_census.py, 74 keys) run by
value against the fp64 oracle: one small case per instantiation, and three with sensor noise on all four channels.
tests/test_variant_census.py pins on the CPU that the cases reach every key; here each case checks that its handle runs the
variant the plan names, then compares truncation flags (exact), observations (the fused per-agent buffer for glue 2), final
observations and rewards at every step and rotor_uvw_agent / yaw_base every 20 steps, over at least one episode rollover of
every env.  Bars: variant_census.py, each from the project's test of the nearest un-noised variant.

The worst error per quantity is printed per case (pytest -s; the committed table: profiles/r17_variant_census_errors.txt) as
worst |d| and as its ratio to the bar, atol + rtol |reference|; a case asserts after its whole run that every ratio is <= 1."""
import contextlib
import faulthandler
import sys
import time

import numpy as np
import pytest

import variant_census as vc
from helpers import hip, make_batch  # noqa: F401  (hip: the fixture)
from test_plan import shim  # noqa: F401  (the g++-only plan fixture)

pytestmark = pytest.mark.gpu

# Per-case time limit, sized from the first clean run on an MI355X host: the slowest case took 0.93 s (it also solves the eddy-viscosity
# table), most take 0.02 .. 0.4 s, the file 13.5 s; a case that runs thirty times as long as the slowest hangs.  A hung kernel cannot
# be interrupted from Python and nothing more may be started on a device after a hang, so the watchdog ends the whole pytest
# process (faulthandler: traceback of every thread on stderr, exit status 1).
CASE_TIME_LIMIT_S = 30


@contextlib.contextmanager
def time_limit(seconds):
    faulthandler.dump_traceback_later(seconds, exit=True, file=sys.stderr)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


_REF = {}


def _reference(oracle_lib, cs, **kw):
    """one oracle trajectory per config, shared by the cases that differ in hooks only; never modified"""
    key = (cs.ref_id, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = vc.reference(oracle_lib, cs, **kw)
    return _REF[key]


def _make_env(hip, cs, plan):
    """HipBatch under the case's hooks (read at wg_create); the variant the plan names is the one that runs — a silent fallback
    would test the wrong kernel"""
    hooks = {vc.HOOK_ENV[k]: str(v) for k, v in cs.hooks}
    return make_batch(hip, cs.cfg(), hooks, variant=(plan["block"], bool(plan["res"]), 2 if plan["path_envw"] else 0))


class Worst:
    """worst |got - want| and worst |got - want| / (atol + rtol |want|) per quantity"""

    def __init__(self):
        self.q = {}

    def add(self, name, got, want, atol, rtol=0.0):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        d = np.abs(got - want)
        d = np.where(np.isfinite(d), d, np.inf)
        a, r = self.q.get(name, (0.0, 0.0))
        self.q[name] = (max(a, float(d.max())), max(r, float((d / (atol + rtol * np.abs(want))).max())))

    def row(self):
        return "  ".join(f"{k} {a:.2e} ({r:.2f})" for k, (a, r) in self.q.items())

    def missed(self):
        return {k: v for k, v in self.q.items() if not v[1] <= 1.0}


def _run(hip, oracle_lib, shim, cs, ref, steps=None):  # noqa: F811
    """the case on the device against the trajectory `ref`: -> Worst, truncations per env"""
    import torch
    cfg = cs.cfg()
    plan = vc.plan_of(shim, cs)
    assert plan["rc"] == 0 and vc.key_of(cs, plan) in vc.ALL_KEYS
    env = _make_env(hip, cs, plan)
    vc.install(cs, env)
    buf = env.fuse_obs_multi() if cs.multi else None
    atol, w = vc.obs_atol(cs), Worst()
    obs0 = env.reset(seeds=vc.seeds_of(cs)).cpu().numpy()
    env.check()
    w.add("obs", obs0, ref["obs0"], atol)
    if cs.multi:
        w.add("obs_multi", buf.cpu().numpy(), ref["multi0"], atol)
    acts = vc.actions_of(cs)
    n_tr = np.zeros(cfg.n_envs, int)
    for k in range(cs.steps if steps is None else steps):
        obs, rew, tr, fin = env.step(torch.as_tensor(acts[k], device="cuda"))
        obs, rew, tr, fin = obs.cpu().numpy().copy(), rew.cpu().numpy(), tr.cpu().numpy().astype(bool), fin.cpu().numpy()
        np.testing.assert_array_equal(tr, ref["tr"][k], err_msg=f"{cs.name}: truncation flags, step {k}")
        n_tr += tr
        if cfg.autoreset:
            w.add("final_obs", fin, ref["fin"][k], atol)
        elif tr.any():      # (replay cases: no autoreset — the truncated envs are reset now, on both sides)
            obs[tr] = env.reset(mask=tr.astype(np.uint8)).cpu().numpy()[tr]
        w.add("obs", obs, ref["obs"][k], atol)
        if cs.multi:
            w.add("obs_multi", buf.cpu().numpy(), ref["multi"][k], atol)
        w.add("reward", rew, ref["rew"][k], **vc.REWARD_BAR)
        if k in ref["uvw"]:
            w.add("rotor_uvw", env.info("rotor_uvw_agent").cpu().numpy(), ref["uvw"][k], **vc.UVW_BAR)
            w.add("yaw_base", env.info("yaw_base").cpu().numpy(), ref["yaw_base"][k], **vc.YAW_BASE_BAR)
    env.check()
    env.close()
    return w, n_tr


def _guarded(fn, *a, **kw):
    """a device fault ends the session: nothing more is started on a device that has faulted"""
    try:
        return fn(*a, **kw)
    except RuntimeError as e:
        if any(t in str(e) for t in ("illegal memory access", "HIP error", "launch failure", "hipError")):
            pytest.exit(f"device fault, the session ends here: {e}", returncode=3)
        raise


@pytest.mark.parametrize("name", [c.name for c in vc.CASES])
def test_instantiation_matches_oracle(hip, oracle_lib, shim, name):  # noqa: F811
    cs = vc.case(name)
    t0 = time.perf_counter()
    with time_limit(CASE_TIME_LIMIT_S):
        ref = _reference(oracle_lib, cs)
        # the oracle alone: every env rolled over at least once (the noise stream is keyed by the episode, the fused tails have a
        # truncating path of their own, a background episode's first observation is built by other code)
        assert (np.sum(ref["tr"], axis=0) >= 1).all(), np.sum(ref["tr"], axis=0)
        w, n_tr = _guarded(_run, hip, oracle_lib, shim, cs, ref)
    key = vc.key_of(cs, vc.plan_of(shim, cs))
    print(f"\n[variant census] {name:26s} {str(key):58s} {time.perf_counter() - t0:5.2f} s  {w.row()}")
    assert (n_tr >= 1).all(), n_tr
    assert not w.missed(), (name, w.missed())


@pytest.mark.parametrize("name", vc.CONTROLS)
def test_oracle_on_shifted_seeds_breaks_the_observation_bar(hip, oracle_lib, shim, name):  # noqa: F811
    """Negative control, one per kernel family: the kernel stays as it is, the oracle is reset on seeds shifted by one — another
    wind and another noise stream.  The comparison must miss the observation bar at the reset and the first steps."""
    cs = vc.case(name)
    with time_limit(CASE_TIME_LIMIT_S):
        wrong = _reference(oracle_lib, cs, seed_shift=1, steps=3)
        # (the flags may differ as well: compare up to the first step only where they agree)
        good = _reference(oracle_lib, cs)
        n = 0
        while n < 3 and np.array_equal(wrong["tr"][n], good["tr"][n]):
            n += 1
        w, _ = _guarded(_run, hip, oracle_lib, shim, cs, wrong, steps=n)
    print(f"\n[variant census control] {name}: oracle on seeds + 1, {n} steps: {w.row()}")
    assert w.q["obs"][1] > 40.0, w.q
