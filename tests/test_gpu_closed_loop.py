"""The closed loop a user calls — ``WindFarmVecEnv.rollout`` (wg_rollout: k_policy and the step kernels alternating on slices of
[T, B, ...] recordings) and ``PPOOptimizer.gae`` on its buffers — BY VALUE against float64 references, on every step path a handle
can take, at the full batch size of that path.  tests/test_gpu_policy.py compares the rollout with the same kernels called one at a
time; tests/test_gpu_spotcheck.py compares the step kernels with the oracle under random actions.  Here the rollout's own buffers
meet the oracles:

* policy outputs  raw / actions / logp / value [t] against oracle/policy_oracle.py on the recorded obs[t], with the noise of
                  (base seed, counter0 + t, GLOBAL row): the counter-per-step and row conventions, pinned from outside;
* final values    final_value[t] against the float64 critic on final_obs[t] (steps 0 .. T-2 ride in the next step's policy launch,
                  step T-1 is a launch of its own);
* step outputs    obs[t+1], reward[t], truncated[t], final_obs[t] and the recorded info fields against oracle/oracle.py, TEACHER-FORCED
                  with the device's own actions[t] (a closed loop cannot drift away from it) on a 16-env twin configuration with the
                  same global seeds: N_SAMPLE envs spread over the batch, as in test_gpu_spotcheck._run;
* advantages      wg_gae on the rollout's buffers against ppo_oracle.gae (whole batch) and gae_brute (the sampled envs).

Each case asserts the kernel variant it claims: ``flow_variant()`` of the live handle and, for what no entry of the ABI reports
(fused step, window-sums mode, waves per env), the host-side plan of windgym_amd/csrc/wg_plan.h for the same configuration
(tests/plan_shim.cpp, as tests/test_plan.py builds it).  The bitwise loop check of test_gpu_policy.py runs on the same rollout."""
import copy
import functools
import ctypes as C
import os

import numpy as np
import pytest

import rl_helpers
from helpers import host_shim
from oracle import policy_oracle as po
from oracle import ppo_oracle as oo
from rl_helpers import (LOGP_ATOL, N_SAMPLE, OBS_ATOL, RAW_ATOL, SMALL_BOX, SMALL_BOX_SPACING, TURB_OBS_ATOL, TURB_POW_ATOL, TURB_POW_RTOL,
                        TURB_REW_ATOL, TURB_REW_RTOL, TURB_UVW_ATOL, TURB_UVW_RTOL, VAL_ATOL, VAL_RTOL, _ti_farm_history_100, _torch,
                        rollout_equals_the_loop)

pytestmark = pytest.mark.gpu
make = functools.partial(rl_helpers.make, draw="normal")        # (test_gpu_policy.py's policies)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = ("power_agent", "yaw_agent", "rotor_uvw_agent", "wind_f64", "timestep")     # one field of every layout of info_shape
# bars of the step outputs per inflow: obs atol, reward (rtol, atol), rotor wind (rtol, atol), power (rtol, atol).  "steady" and "box"
# are test_gpu_spotcheck.py's, "random" test_gpu_parity.py's for counter-based gusts (_compare_turb) with the box's power bar.
BARS = {"steady": (OBS_ATOL, (1e-4, OBS_ATOL), (1e-4, 1e-4), (4e-4, 20.0)),
        "box": (TURB_OBS_ATOL, (TURB_REW_RTOL, TURB_REW_ATOL), (TURB_UVW_RTOL, TURB_UVW_ATOL), (TURB_POW_RTOL, TURB_POW_ATOL)),
        "random": (5e-4, (1e-3, 1e-3), (2e-4, 2e-3), (TURB_POW_RTOL, TURB_POW_ATOL))}


def _case(name):
    """-> dict(yaml, B, T, turbtype, kw of EnvConfig, bars, hidden (pi, vf), graph, what the handle must run)
    variant = flow_variant() of the handle; plan = entries of the host-side plan.  T: at least half of the sampled envs truncate inside
    the rollout (episode lengths at these n_passthrough: cfg2 / cfg5 / Random 98-215 steps, Horns Rev 175-423, the 3 x 2 farm 21-43)."""
    from windgym_amd import presets
    fused_env = dict(envw=1, path_envw=1, path_fused=1, sums_mode=1, block=64)
    c = dict(yaml=presets.bench_cfg2_config(), turbtype="None", kw=dict(n_passthrough=1), bars="steady", hidden=((64, 64), (64, 64)),
             graph=False, T=200, variant=(64, True, 2))
    if name.startswith("cfg2_"):
        B = int(name.split("_")[1])
        wpe, split = {4096: (1, 0), 1024: (2, 1), 389: (2, 2), 256: (2, 2)}[B]       # tests/test_plan.py's table of the step path
        c.update(B=B, plan=dict(fused_env, env_wpe=wpe, env_split=split), graph=name.endswith("graph"))
    elif name == "cfg3_512":
        x, y = presets.horns_rev1_layout()
        c.update(yaml=presets.horns_rev_config(), B=512, T=300, kw=dict(n_passthrough=0.5, x_pos=x, y_pos=y), hidden=((128, 128), (64,)),
                 variant=(256, True, 0), plan=dict(envw=0, path_envw=0, path_fused=0, sums_mode=1, block=256, gl=0))
    elif name == "cfg5_1024":
        c.update(B=1024, turbtype="MannGenerate", bars="box", plan=dict(fused_env, env_wpe=2, env_split=0))
    elif name == "random_256":
        c.update(B=256, turbtype="Random", bars="random", variant=(64, True, 0),
                 plan=dict(envw=0, path_envw=0, path_fused=0, sums_mode=1, block=64, gl=0))
    elif name == "ti_farm_history100_64":
        c.update(yaml=_ti_farm_history_100(), B=64, T=100, kw=dict(n_passthrough=0.3), hidden=((64,), (128, 128)),
                 plan=dict(envw=1, path_envw=1, path_fused=0, sums_mode=0, block=64))
    else:
        raise KeyError(name)
    return c


CASES = ["cfg2_4096", "cfg2_1024", "cfg2_389", "cfg3_512", "cfg5_1024", "random_256", "ti_farm_history100_64", "cfg2_256_graph"]


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    """cfg, box cells -> the plan wg_create makes for it, as a dict of ints (tests/plan_shim.cpp; g++ alone)."""
    from windgym_amd.config import CConfig
    lib = host_shim(tmp_path_factory, "plan", include_header_dir=True)
    lib.plan_dump.argtypes = [C.POINTER(CConfig), C.POINTER(C.c_int), C.c_int, C.c_longlong, C.c_longlong, C.c_char_p, C.c_int]

    def plan(cfg, box_cells=0):
        buf = C.create_string_buffer(4096)
        cc = cfg.to_c()
        assert lib.plan_dump(C.byref(cc), (C.c_int * 21)(), 65536, box_cells, 0, buf, 4096) == 0, buf.value
        d = dict(ln.split(" ", 1) for ln in buf.value.decode().splitlines())
        return {k: int(v) for k, v in d.items() if k not in ("err", "alg_bytes", "tab_x0", "tab_dx")}
    return plan


@pytest.fixture(scope="module")
def small_box():
    from windgym_amd.mann import generate_mann_box
    return generate_mann_box(SMALL_BOX, SMALL_BOX_SPACING, seed=1234)


def _venv(c, n_envs, seed, box=None):
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.turbine import V80
    kw = dict(c["kw"])
    if c["turbtype"].startswith("Mann"):
        kw["turbulence_box"] = (box, SMALL_BOX_SPACING)
    v = WindFarmVecEnv(V80(), n_envs, yaml_dict=copy.deepcopy(c["yaml"]), seed=seed, as_torch=True, turbtype=c["turbtype"], n_rotor_pts=16, **kw)
    return v


def _oracle(oracle_lib, c, box):
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    sub = EnvConfig(turbine=V80(), yaml_dict=copy.deepcopy(c["yaml"]), turbtype=c["turbtype"], n_envs=N_SAMPLE, autoreset=True, n_rotor_pts=16,
                    **c["kw"])
    orc = oracle_lib.Oracle(sub)
    if c["turbtype"].startswith("Mann"):
        orc.set_turbulence_box(box, SMALL_BOX_SPACING)
    return orc


class _Worst(dict):
    """largest absolute errors per quantity, printed for the record as the spot checks do"""

    def see(self, key, got, ref):
        e = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())
        self[key] = max(self.get(key, 0.0), e)
        return e


def check_rollout_by_value(venv, orc, policy, sd, out, T, idx, seed, counter0, bars, activation="tanh", pre_actions=()):
    """The buffers ``out`` of ``venv.rollout(policy, T, record=RECORD)`` at the env rows ``idx`` against the float64 references.
    ``orc`` replays those envs (global seeds ``seed + row0 + idx``); ``pre_actions``: what the envs were stepped with between the
    reset and the rollout.  -> (worst absolute errors, truncations per sampled env)."""
    t = _torch()
    obs_atol, (rew_rtol, rew_atol), (uvw_rtol, uvw_atol), (pow_rtol, pow_atol) = bars
    N = venv.n_turb
    grow = venv._global_offset + idx                                          # global rows: seeds and the noise stream
    it = t.as_tensor(idx, device="cuda")
    h = {k: v.index_select(1, it).cpu().numpy() for k, v in out.items()}      # [T(+1), 16, ...]: only the sampled rows cross PCIe
    worst = _Worst()
    o0 = orc.reset(seeds=seed + grow)
    for a in pre_actions:
        o0 = orc.step(a[idx])[0]
    np.testing.assert_allclose(h["obs"][0], o0, rtol=0, atol=obs_atol, err_msg="obs[0]")
    # ---- policy outputs and final values: one float64 pass over all T x 16 rows ----------------------------------------------------
    eps = np.stack([po.policy_noise(seed, counter0 + s, grow, N) for s in range(T)])
    ref = po.sample(sd, h["obs"][:T], eps=eps, activation=activation)
    for k, rk, atol, rtol in (("raw", "raw", RAW_ATOL, 0.0), ("actions", "action", RAW_ATOL, 0.0), ("logp", "logp", LOGP_ATOL, 0.0),
                              ("value", "value", VAL_ATOL, VAL_RTOL)):
        worst.see(k, h[k], ref[rk])
        np.testing.assert_allclose(h[k], ref[rk], rtol=rtol, atol=atol, err_msg=k)
    assert np.array_equal(h["actions"], np.clip(h["raw"], -1.0, 1.0))
    fv = po.forward(sd, h["final_obs"], activation)[1]
    worst.see("final_value", h["final_value"], fv)
    for s in (0, T - 2, T - 1):                                               # (named: ride-along slots and the separate last launch)
        np.testing.assert_allclose(h["final_value"][s], fv[s], rtol=VAL_RTOL, atol=VAL_ATOL, err_msg=f"final_value step {s}")
    np.testing.assert_allclose(h["final_value"], fv, rtol=VAL_RTOL, atol=VAL_ATOL, err_msg="final_value")
    # ---- step outputs and recorded info: the oracle driven by the device's own actions --------------------------------------------
    n_tr = np.zeros(len(idx), dtype=int)
    for s in range(T):
        o_obs, o_rew, o_tr, o_fin = orc.step(h["actions"][s])
        np.testing.assert_array_equal(h["truncated"][s].astype(bool), o_tr, err_msg=f"truncated step {s}")
        worst.see("obs", h["obs"][s + 1], o_obs), worst.see("final_obs", h["final_obs"][s], o_fin), worst.see("reward", h["reward"][s], o_rew)
        np.testing.assert_allclose(h["obs"][s + 1], o_obs, rtol=0, atol=obs_atol, err_msg=f"obs step {s}")
        np.testing.assert_allclose(h["final_obs"][s], o_fin, rtol=0, atol=obs_atol, err_msg=f"final obs step {s}")
        np.testing.assert_allclose(h["reward"][s], o_rew, rtol=rew_rtol, atol=rew_atol, err_msg=f"reward step {s}")
        n_tr += o_tr.astype(int)
        wind = np.stack([orc.info(k) for k in ("ws_global", "wd_global", "ti_global")], axis=1)
        worst.see("yaw", h["yaw_agent"][s], orc.info("yaw_agent")), worst.see("rotor wind", h["rotor_uvw_agent"][s], orc.info("rotor_uvw_agent"))
        worst.see("farm power", h["power_agent"][s], orc.info("power_agent")), worst.see("wind_f64", h["wind_f64"][s], wind)
        np.testing.assert_array_equal(h["timestep"][s], orc.info("timestep").astype(np.int64), err_msg=f"timestep step {s}")
        np.testing.assert_allclose(h["yaw_agent"][s], orc.info("yaw_agent"), atol=1e-4, err_msg=f"yaw step {s}")
        np.testing.assert_allclose(h["rotor_uvw_agent"][s], orc.info("rotor_uvw_agent"), rtol=uvw_rtol, atol=uvw_atol, err_msg=f"rotor wind step {s}")
        np.testing.assert_allclose(h["power_agent"][s], orc.info("power_agent"), rtol=pow_rtol, atol=pow_atol, err_msg=f"farm power step {s}")
        np.testing.assert_allclose(h["wind_f64"][s], wind, rtol=1e-12, atol=0, err_msg=f"wind_f64 step {s}")
    assert h["wind_f64"].dtype == np.float64 and h["timestep"].dtype == np.int32
    return worst, n_tr


def check_gae(policy, out, idx, worst, gamma=0.99, lam=0.95):
    """wg_gae on the rollout's own buffers: the recurrence on the whole batch, the definition on the sampled envs."""
    from windgym_amd.ppo import PPOOptimizer
    opt = PPOOptimizer(policy)
    adv, ret = (x.cpu().numpy() for x in opt.gae(out["reward"], out["value"], out["final_value"], out["truncated"], gamma, lam))
    r, v, fv, tr = (out[k].cpu().numpy() for k in ("reward", "value", "final_value", "truncated"))
    ra, rr = oo.gae(r, v, fv, tr, gamma, lam)
    ba, br = oo.gae_brute(r[:, idx], v[:, idx], fv[:, idx], tr[:, idx], gamma, lam)
    worst.see("advantage", adv, ra), worst.see("advantage (definition)", adv[:, idx], ba)
    for got, want in ((adv, ra), (ret, rr), (adv[:, idx], ba), (ret[:, idx], br)):         # test_gpu_ppo.py's bars of test_gae_vs_oracle
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-5)
    opt.close()
    return int(tr.sum())


@pytest.mark.parametrize("name", CASES)
def test_rollout_by_value_and_against_the_loop(name, oracle_lib, plan_of, small_box):
    t = _torch()
    c = _case(name)
    B, T, seed = c["B"], c["T"], 1234                                         # bench.py's seeding: env i of the batch has seed 1234 + i
    va, vb = _venv(c, B, seed, small_box), _venv(c, B, seed, small_box)
    # the kernels this case claims
    assert va.batch.flow_variant() == c["variant"], va.batch.flow_variant()
    plan = plan_of(va.cfg, int(np.prod(SMALL_BOX)) if c["turbtype"].startswith("Mann") else 0)
    assert {k: plan[k] for k in c["plan"]} == c["plan"], plan
    O, N = va.batch.obs_dim, va.n_turb
    assert (O, N) == (plan["obs_dim"], plan["N"])
    va.reset(seed=seed); vb.reset(seed=seed)
    pre = []
    if c["graph"]:
        # two steps through the graph first (one cached graph on the persistent buffers), the rollout by direct launches, step() again
        # through the graph (rollout_equals_the_loop's last step): the twin vb runs direct launches throughout
        va.batch.set_step_graph(True)
        g = t.Generator(device="cpu").manual_seed(1)
        for _ in range(2):
            a = (t.rand((B, N), generator=g) * 2 - 1).cuda()
            assert t.equal(va.step(a)[0], vb.step(a)[0])
            pre.append(a.cpu().numpy())
    policy, sd = make(O, c["hidden"][0], N, hidden_vf=c["hidden"][1])
    idx = np.linspace(0, B - 1, N_SAMPLE).round().astype(int)                 # first, last and 14 envs in between
    out = va.rollout(policy, T, record=RECORD)
    orc = _oracle(oracle_lib, c, small_box)
    worst, n_tr = check_rollout_by_value(va, orc, policy, sd, out, T, idx, seed, 0, BARS[c["bars"]], pre_actions=pre)
    assert (n_tr >= 1).sum() >= N_SAMPLE // 2, n_tr
    n_trunc = check_gae(policy, out, idx, worst)                              # (on a rollout with same-step autoresets: n_trunc of them)
    assert n_trunc >= B // 4, n_trunc
    # recorded info of step T-1 == what the handle reports after the rollout (info_bytes against info_shape)
    for k in RECORD:
        assert t.equal(out[k][T - 1], va.batch.info(k)), k
        assert tuple(out[k].shape) == (T,) + tuple(va.batch.info_shape(k)[0])
    print(f"[{name}] T = {T}, {n_trunc} truncations; worst absolute errors: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    # the same rollout against the loop of act + step on the twin, bit for bit; then step() (the graph's, in graph mode) and the state
    rollout_equals_the_loop(va, vb, policy, T, RECORD, out=out, min_trunc=B // 4)
    orc.close(); va.close(); vb.close(); policy.close()


def test_shard_invariance_of_every_rollout_buffer(small_box):
    """One handle of 64 envs == two handles of 32 with .shard(0, 2) / .shard(1, 2) on the same base seed: env seeds and the policy's
    noise follow the GLOBAL row, and nothing else of a row depends on the batch it sits in."""
    t = _torch()
    c = _case("cfg5_1024")
    T, seed = 150, 4321
    whole = _venv(c, 64, seed, small_box)
    halves = [_venv(c, 32, seed, small_box).shard(r, 2) for r in range(2)]
    for v in [whole] + halves:
        assert v.batch.flow_variant() == (64, True, 2)                        # k_flow_envb at every size
        v.reset(seed=seed)
    policy, _ = make(whole.batch.obs_dim, (64, 64), whole.n_turb, hidden_vf=(32,))
    out = {k: x.clone() for k, x in whole.rollout(policy, T, record=RECORD).items()}
    assert int(out["truncated"].sum()) >= 32
    for r, v in enumerate(halves):
        part = v.rollout(policy, T, record=RECORD)
        assert set(part) == set(out)
        for k, x in part.items():
            assert t.equal(x, out[k][:, 32 * r:32 * (r + 1)]), (k, r)
        v.batch.check()
    for v in [whole] + halves:
        v.close()
    policy.close()


def test_rollouts_interleaved_with_steps_equal_the_loop():
    """rollout(T1), step, rollout(T2) with another record tuple, rollout(T1) again (its cached buffers reused) == one twin driven by the
    loop of act + step: the buffer cache's keys and the running count of policy steps that numbers the noise."""
    from rl_helpers import _venv as venv77
    t = _torch()
    va, vb = venv77(48, n_passthrough=0.3), venv77(48, n_passthrough=0.3)      # episodes of 30 to 65 steps
    O, N, B = va.batch.obs_dim, va.n_turb, va.num_envs
    policy, _ = make(O, (64, 64), N)
    raws = []
    for T, rec in ((40, ("power_agent", "yaw_agent")), (25, ("rotor_uvw_agent", "timestep", "wind_f64")), (40, ("power_agent", "yaw_agent")),
                   (40, ())):
        counter0 = va.__dict__.get("_policy_steps", 0)
        assert counter0 == vb.__dict__.get("_policy_steps", 0)
        out = rollout_equals_the_loop(va, vb, policy, T, rec, min_trunc=0)          # (ends with one step() on both)
        assert va._policy_steps == counter0 + T
        raws.append((out["raw"] - policy.torch_forward(out["obs"][:T])[0].detach()).clone())
    assert not t.equal(raws[0], raws[2]) and not t.equal(raws[2], raws[3])            # no noise is reused
    assert int(va.batch.info("episode").sum()) >= B                                    # the 145 + 4 steps crossed autoresets
    va.close(); vb.close(); policy.close()
