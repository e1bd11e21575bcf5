"""The multi-agent path on the device: one agent per turbine, ONE policy shared by the turbines.

* final per-agent observations  ``WindFarmVecEnvMulti.step``'s ``final_obs`` BY VALUE: a float64 oracle without autoreset, one per sampled
                                env, teacher-forced with the device's own actions, gives ``obs_multi()`` of the finished episode at its
                                truncating step; rows of envs that did not truncate equal the per-agent buffer bit for bit; on every step
                                path that writes the per-agent buffer, each asserted through ``flow_variant()`` and the host-side plan;
* NULL final pointer            outputs and ``get_state()`` equal a handle that never registered one, bit for bit;
* wg_rollout_multi              equals its documented loop bit for bit (every buffer, the state, the step after it), meets the float64
                                policy oracle on sampled envs, is shard-invariant and interleaves with ``step()``;
* wg_gae_shared                 against the float64 reference of oracle/ppo_oracle.py and, at A = 1, wg_gae bit for bit;
* PPO on the multi-agent env    one iteration against the torch reference trainer on the flattened agent rows, save / load resume,
                                a 20-iteration run without a NaN."""
import copy
import functools
import os

import numpy as np
import pytest

import rl_helpers
from oracle import policy_oracle as po
from oracle.ppo_oracle import gae_shared
from rl_helpers import (LOGP_ATOL, OBS_ATOL, RAW_ATOL, SMALL_BOX, SMALL_BOX_SPACING, TURB_OBS_ATOL, VAL_ATOL, VAL_RTOL, _ti_farm_history_100,
                        _torch, rollout_equals_the_loop)
from test_gpu_closed_loop import plan_of, small_box  # noqa: F401  (module-scoped fixtures, used by name)

pytestmark = pytest.mark.gpu
make = functools.partial(rl_helpers.make, draw="normal")        # (test_gpu_policy.py's policies)


def _case(name):
    """-> dict(yaml, turbtype, kw of EnvConfig, B, T, obs atol, flow_variant() and plan entries the handle must show)"""
    from windgym_amd import presets
    c = dict(yaml=presets.multi_3x3_config(), turbtype="None", kw=dict(n_passthrough=1), B=64, T=260, atol=OBS_ATOL,
             variant=(64, True, 2), plan=dict(path_envw=1, path_fused=1, sums_mode=1))
    if name == "cfg4_fused":                     # k_flow_env with the glue as its tail
        pass
    elif name == "box_fused":                    # k_flow_envb
        c.update(turbtype="MannGenerate", atol=TURB_OBS_ATOL)
    elif name == "ti_farm_history":              # ring-staging k_glue: TI, farm-level entries (the agents' farm block), 100-sample history
        c.update(yaml=_ti_farm_history_100(), kw=dict(n_passthrough=0.3), T=100, plan=dict(path_envw=1, path_fused=0, sums_mode=0))
    elif name == "horns_rev_lean":               # k_flow + k_glue_lean
        x, y = presets.horns_rev1_layout()
        c.update(yaml=presets.horns_rev_config(), kw=dict(n_passthrough=0.2, x_pos=x, y_pos=y), B=32, T=200, variant=(256, True, 0),
                 plan=dict(path_envw=0, path_fused=0, sums_mode=1))
    else:
        raise KeyError(name)
    return c


def _menv(c, n_envs, seed, box=None, **over):
    from windgym_amd.envs import WindFarmVecEnvMulti
    from windgym_amd.turbine import V80
    kw = dict(c["kw"])
    kw.update(over)
    if c["turbtype"].startswith("Mann"):
        kw["turbulence_box"] = (box, SMALL_BOX_SPACING)
    return WindFarmVecEnvMulti(V80(), n_envs, yaml_dict=copy.deepcopy(c["yaml"]), seed=seed, turbtype=c["turbtype"], n_rotor_pts=16, **kw)


def _assert_path(m, c, plan_of):
    assert m.batch.flow_variant() == c["variant"], m.batch.flow_variant()
    plan = plan_of(m.cfg, int(np.prod(SMALL_BOX)) if c["turbtype"].startswith("Mann") else 0)
    assert {k: plan[k] for k in c["plan"]} == c["plan"], plan


@pytest.mark.parametrize("name", ["cfg4_fused", "box_fused", "ti_farm_history", "horns_rev_lean"])
def test_final_obs_multi_by_value(name, oracle_lib, plan_of, small_box):     # noqa: F811
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    t = _torch()
    c = _case(name)
    B, T, seed = c["B"], c["T"], 1234
    m = _menv(c, B, seed, small_box)
    _assert_path(m, c, plan_of)
    N, Om = m.n_turb, m.obs_len
    obs0 = m.reset(seed=seed).clone()
    assert tuple(obs0.shape) == (B, N, Om)
    assert (obs0 - m.batch.obs_multi()).abs().max().item() <= c["atol"]       # (the explicit launch sums its windows in another order)
    g = t.Generator(device="cpu").manual_seed(7)
    acts, obs_m, fin_m, trunc = [], [], [], []
    for _ in range(T):
        a = (t.rand((B, N), generator=g) * 2 - 1).cuda()
        o, r, term, tr, f = m.step(a if len(acts) % 2 else a.reshape(B, N, 1))
        assert tuple(f.shape) == (B, N, Om) and tr.dtype == t.bool and not term.any()
        acts.append(a.cpu().numpy()); obs_m.append(o.clone()); fin_m.append(f.clone()); trunc.append(tr.clone())
    m.batch.check()
    obs_m, fin_m, trunc = t.stack(obs_m), t.stack(fin_m), t.stack(trunc)
    # rows of envs that did not truncate: the per-agent buffer's, bit for bit; truncating envs: another episode's observation
    assert t.equal(fin_m[~trunc], obs_m[~trunc])
    assert trunc.any(dim=0).float().mean().item() >= 0.5, "episodes must truncate inside the run"
    assert not t.equal(fin_m[trunc], obs_m[trunc])
    # by value: one oracle per sampled env WITHOUT autoreset, driven by the device's actions up to its first truncation
    idx = np.linspace(0, B - 1, 6).round().astype(int)
    first = [int(np.argmax(trunc[:, i].cpu().numpy())) if bool(trunc[:, i].any()) else -1 for i in idx]
    assert sum(f >= 0 for f in first) >= 3, first
    worst = 0.0
    for i, ft in zip(idx, first):
        if ft < 0:
            continue
        cfg1 = EnvConfig(turbine=V80(), yaml_dict=copy.deepcopy(c["yaml"]), turbtype=c["turbtype"], n_envs=1, autoreset=False, n_rotor_pts=16,
                         extra_timestep_inc=True, **c["kw"])
        orc = oracle_lib.Oracle(cfg1)
        if c["turbtype"].startswith("Mann"):
            orc.set_turbulence_box(small_box, SMALL_BOX_SPACING)
        orc.reset(seeds=np.array([seed + i], dtype=np.uint64))
        np.testing.assert_allclose(obs0[i].cpu().numpy(), orc.obs_multi()[0], rtol=0, atol=c["atol"])
        for s in range(ft + 1):
            _, _, o_tr, _ = orc.step(acts[s][i:i + 1])
            assert bool(o_tr[0]) == (s == ft), (i, s, ft)
            ref = orc.obs_multi()[0]                                          # the state step s ended in (no reset: the FINISHED episode)
            got = fin_m[s, i].cpu().numpy()
            worst = max(worst, float(np.abs(got - ref).max()))
            np.testing.assert_allclose(got, ref, rtol=0, atol=c["atol"], err_msg=f"final_obs_multi env {i} step {s} (truncates at {ft})")
        orc.close()
    print(f"[{name}] first truncations at {first}; worst |final_obs_multi - oracle| = {worst:.2e}")
    m.close()


@pytest.mark.parametrize("name", ["cfg4_fused", "ti_farm_history"])
def test_null_final_pointer_is_the_parent_bit_for_bit(name, small_box):       # noqa: F811
    """Three handles on the same seeds and actions: never registered / registered and dropped again / registered throughout.  Flat
    outputs, the per-agent buffer and the state blob are the same bits on all three; so the feature neither reads nor perturbs state."""
    from windgym_amd.binding import HipBatch
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    t = _torch()
    c = _case(name)
    B, T = 48, c["T"] // 2 + 40
    hs, multi = [], []
    for k in range(3):
        cfg = EnvConfig(turbine=V80(), yaml_dict=copy.deepcopy(c["yaml"]), turbtype=c["turbtype"], n_envs=B, autoreset=True, n_rotor_pts=16,
                        extra_timestep_inc=True, **c["kw"])
        h = HipBatch(cfg, device=0)
        multi.append(h.fuse_obs_multi())
        if k >= 1:
            h.fuse_final_obs_multi()
        if k == 1:
            h.fuse_final_obs_multi(False)
        h.reset(seeds=np.arange(B) + 99)
        hs.append(h)
    g = t.Generator(device="cpu").manual_seed(3)
    n_tr = 0
    for s in range(T):
        a = (t.rand((B, hs[0].N), generator=g) * 2 - 1).cuda()
        outs = [[x.clone() for x in h.step(a)] for h in hs]
        n_tr += int(outs[0][2].sum())
        for k in (1, 2):
            for x, y in zip(outs[0], outs[k]):
                assert t.equal(x, y), (k, s)
            assert t.equal(multi[0], multi[k]), (k, s)
    assert n_tr >= B // 2
    s0 = hs[0].get_state()
    assert s0 == hs[1].get_state() and s0 == hs[2].get_state()
    with pytest.raises(ValueError):                                           # the final buffer needs the per-agent buffer
        hs[0].fuse_obs_multi(False)
        hs[0].fuse_final_obs_multi()
    for h in hs:
        h.check(); h.close()


@pytest.mark.parametrize("B", [2048, 389, 64])
def test_rollout_multi_equals_its_loop_and_the_policy_oracle(B, plan_of):     # noqa: F811
    t = _torch()
    c = _case("cfg4_fused")
    T, seed = 220, 1234
    va, vb = _menv(c, B, seed), _menv(c, B, seed)
    _assert_path(va, c, plan_of)
    va.reset(seed=seed); vb.reset(seed=seed)
    N, Om = va.n_turb, va.obs_len
    p, sd = make(Om, (64, 64), 1, hidden_vf=(32, 32))
    out = rollout_equals_the_loop(va, vb, p, T, min_trunc=B // 2)
    # 16 sampled envs (all their agents) against the float64 policy oracle: noise row of agent i of env e = e * N + i
    idx = np.linspace(0, B - 1, 16).round().astype(int)
    it = t.as_tensor(idx, device="cuda")
    h = {k: out[k].index_select(1, it).cpu().numpy() for k in ("obs", "raw", "actions", "logp", "value", "final_obs", "final_value")}
    rows = (idx[:, None] * N + np.arange(N)[None, :]).reshape(-1)
    eps = np.stack([po.policy_noise(seed, s, rows, 1) for s in range(T)])     # [T, 16 N, 1]
    ref = po.sample(sd, h["obs"][:T].reshape(T, 16 * N, Om), eps=eps)
    np.testing.assert_allclose(h["raw"].reshape(T, -1), ref["raw"][..., 0], rtol=0, atol=RAW_ATOL)
    np.testing.assert_allclose(h["actions"].reshape(T, -1), ref["action"][..., 0], rtol=0, atol=RAW_ATOL)
    np.testing.assert_allclose(h["logp"].reshape(T, -1), ref["logp"], rtol=0, atol=LOGP_ATOL)
    np.testing.assert_allclose(h["value"].reshape(T, -1), ref["value"], rtol=VAL_RTOL, atol=VAL_ATOL)
    fv = po.forward(sd, h["final_obs"].reshape(T, 16 * N, Om), "tanh")[1]
    np.testing.assert_allclose(h["final_value"].reshape(T, -1), fv, rtol=VAL_RTOL, atol=VAL_ATOL)
    # the noise of an env's agents differs (a row index of `e` alone would repeat it N times)
    z = (out["raw"] - p.torch_forward(out["obs"][:T])[0].detach()[..., 0])
    assert (z[:, :, 0] != z[:, :, 1]).float().mean().item() > 0.99
    va.close(); vb.close(); p.close()


def test_rollout_multi_without_flat_buffers_through_the_abi():
    """wg_rollout_multi with obs = final_obs = NULL (the handle's own scratch takes the flat observation): every other buffer and the
    state as with them."""
    import ctypes as C
    from windgym_amd.binding import CRolloutMultiBufs, _chk
    t = _torch()
    c = _case("cfg4_fused")
    B, T, seed = 64, 150, 77
    va, vb = _menv(c, B, seed), _menv(c, B, seed)
    va.reset(seed=seed); vb.reset(seed=seed)
    N, Om = va.n_turb, va.obs_len
    p, _ = make(Om, (64,), 1)
    ref = {k: v.clone() for k, v in va.rollout(p, T).items()}
    f32 = dict(dtype=t.float32, device="cuda")
    bufs = dict(obs=t.zeros((T + 1, B, N, Om), **f32), actions=t.zeros((T, B, N), **f32), raw=t.zeros((T, B, N), **f32), logp=t.zeros((T, B, N), **f32),
                value=t.zeros((T, B, N), **f32), final_obs=t.zeros((T, B, N, Om), **f32), final_value=t.zeros((T, B, N), **f32),
                reward=t.zeros((T, B), **f32), truncated=t.zeros((T, B), dtype=t.uint8, device="cuda"))
    bufs["obs"][0].copy_(vb._obs)
    own = (vb._obs.clone(), vb._final_obs.clone())
    cb = CRolloutMultiBufs(*[bufs[k].data_ptr() for k in ("obs", "actions", "raw", "logp", "value", "final_obs", "final_value", "reward", "truncated")],
                           None, None, 0, None, None)
    b = vb.batch
    _chk(b.L.wg_rollout_multi(b._h, p._h, T, 0, seed, 0, 0, C.byref(cb), b._stream()), "wg_rollout_multi")
    b.check()
    for k, v in bufs.items():
        assert t.equal(v, ref[k]), k
    assert t.equal(vb._obs, own[0]) and t.equal(vb._final_obs, own[1])       # the handle's own per-agent buffers were not written
    assert va.batch.get_state() == vb.batch.get_state()
    # refusals: a policy of the single-agent shape, final_value without final_obs_multi
    q, _ = make(va.batch.obs_dim, (64,), N)
    with pytest.raises(ValueError, match="obs_dim_multi"):
        _chk(b.L.wg_rollout_multi(b._h, q._h, T, 0, seed, 0, 0, C.byref(cb), b._stream()), "wg_rollout_multi")
    with pytest.raises(ValueError, match="-> 1"):
        va.rollout(q, 4)
    cb.final_obs_multi = None
    with pytest.raises(ValueError, match="final_obs_multi"):
        _chk(b.L.wg_rollout_multi(b._h, p._h, T, 0, seed, 0, 0, C.byref(cb), b._stream()), "wg_rollout_multi")
    va.close(); vb.close(); p.close(); q.close()


def test_shard_invariance_and_interleaving_with_step(small_box):             # noqa: F811
    t = _torch()
    c = _case("box_fused")
    T, seed = 150, 4321
    whole = _menv(c, 64, seed, small_box)
    halves = [_menv(c, 32, seed, small_box).shard(r, 2) for r in range(2)]
    for v in [whole] + halves:
        assert v.batch.flow_variant() == (64, True, 2)
        v.reset(seed=seed)
    p, _ = make(whole.obs_len, (64, 64), 1, hidden_vf=(32,))
    out = {k: x.clone() for k, x in whole.rollout(p, T, record=("yaw_agent",)).items()}
    assert int(out["truncated"].sum()) >= 32
    for r, v in enumerate(halves):
        part = v.rollout(p, T, record=("yaw_agent",))
        assert set(part) == set(out)
        for k, x in part.items():
            assert t.equal(x, out[k][:, 32 * r:32 * (r + 1)]), (k, r)
        v.batch.check()
    for v in [whole] + halves:
        v.close()
    # rollout, step, rollout with another record tuple, rollout again (cached buffers): a twin driven by the loop
    c = _case("cfg4_fused")
    va, vb = _menv(c, 48, 5, n_passthrough=0.3), _menv(c, 48, 5, n_passthrough=0.3)
    va.reset(seed=5); vb.reset(seed=5)
    q, _ = make(va.obs_len, (64, 64), 1)
    for Ti, rec in ((40, ("power_agent",)), (25, ("timestep", "wind_f64")), (40, ("power_agent",)), (40, ())):
        rollout_equals_the_loop(va, vb, q, Ti, rec, min_trunc=0)
    assert int(va.batch.info("episode").sum()) >= 48
    va.close(); vb.close(); p.close(); q.close()


@pytest.mark.parametrize("T,B,A", [(1, 1, 1), (7, 389, 9), (128, 2048, 9), (64, 33, 80), (128, 4096, 1)])
def test_gae_shared_vs_reference_and_wg_gae(T, B, A):
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    rng = np.random.default_rng(T + B + A)
    r = rng.standard_normal((T, B)).astype(np.float32)
    v, fv = (rng.standard_normal((T, B, A)).astype(np.float32) for _ in range(2))
    tr = (rng.uniform(size=(T, B)) < 0.05).astype(np.uint8)
    p, _ = make(4, (8,), 1)
    opt = PPOOptimizer(p)
    dv = lambda a: t.as_tensor(a, device="cuda")                              # noqa: E731
    adv, ret = opt.gae_shared(dv(r), dv(v), dv(fv), dv(tr), 0.99, 0.95)
    ra, rr = gae_shared(r, v, fv, tr, 0.99, 0.95)
    np.testing.assert_allclose(adv.cpu().numpy(), ra, rtol=1e-5, atol=2e-5)   # test_gpu_ppo.py's bars of test_gae_vs_oracle
    np.testing.assert_allclose(ret.cpu().numpy(), rr, rtol=1e-5, atol=2e-5)
    # every agent column IS wg_gae on that column (A = 1 included): bit for bit
    for i in sorted({0, A - 1}):
        a1, r1 = opt.gae(dv(r), dv(np.ascontiguousarray(v[:, :, i])), dv(np.ascontiguousarray(fv[:, :, i])), dv(tr), 0.99, 0.95)
        assert t.equal(a1, adv[:, :, i]) and t.equal(r1, ret[:, :, i]), i
    with pytest.raises(ValueError):
        opt.gae_shared(dv(r), dv(v[:, :, 0]), dv(fv[:, :, 0]), dv(tr), 0.99, 0.95)
    opt.close(); p.close()


def test_ppo_one_iteration_vs_torch_reference_trainer_on_agent_rows():
    from rl_helpers import _torch_trainer
    from windgym_amd.ppo import PPO
    t = _torch()
    c = _case("cfg4_fused")
    v = _menv(c, 256, 21, n_passthrough=0.3)
    v.reset(seed=21)
    B, N = v.num_envs, v.n_turb
    ppo = PPO("MlpPolicy", v, n_steps=32, n_epochs=2, ent_coef=0.01, seed=3)
    assert (ppo.policy.n_in, ppo.policy.n_out) == (v.obs_len, 1)
    assert ppo.n_rows == 32 * B * N and ppo.batch_size == ppo.n_rows // 4 and tuple(ppo._perm.shape) == (2, ppo.n_rows)
    out = ppo.collect()
    assert tuple(out["advantage"].shape) == (32, B, N) and int(out["truncated"].sum()) > 0
    ra, rr = gae_shared(*(out[k].cpu().numpy() for k in ("reward", "value", "final_value", "truncated")), 0.99, 0.95)
    np.testing.assert_allclose(out["advantage"].cpu().numpy(), ra, rtol=1e-5, atol=2e-5)
    gen_state = ppo._gen.get_state()
    before = ppo.policy.params.clone()
    ppo.train(out, 3e-4, 0.2)
    perm = ppo._perm.clone()
    ppo._gen.set_state(gen_state)
    with t.no_grad():
        after = ppo.policy.params.clone()
        ppo.policy.params.copy_(before)
    ref = _torch_trainer(ppo.policy, out, ppo._adv, ppo._ret, perm, ppo.batch_size, 3e-4, 0.2, 0.5, 0.01, 0.5)
    assert (after - before).abs().max().item() > 1e-4
    err = ((after - ref).abs() / (ref.abs() + 1e-3)).max().item()
    assert err <= 1e-4, err                                                   # test_gpu_ppo.py's trainer bar
    assert (after - ref).abs().max().item() <= 1e-5
    ppo.close(); ppo.policy.close(); v.close()


def test_ppo_learn_save_load_continue_and_twenty_iterations(tmp_path):
    from windgym_amd.ppo import PPO
    t = _torch()
    c = _case("cfg4_fused")
    T, seed = 40, 9
    kw = dict(n_steps=T, n_epochs=2, ent_coef=0.001, seed=11)
    mk = lambda n: _menv(c, n, seed, n_passthrough=0.3)                       # noqa: E731
    va = mk(64); va.reset(seed=seed)
    a = PPO("MlpPolicy", va, **kw)
    a.learn(4 * T * va.num_envs)
    assert a.iteration == 4 and a.num_timesteps == 4 * T * va.num_envs and len(a.log) == 4      # env steps, not agent rows
    vb = mk(64); vb.reset(seed=seed)
    b = PPO("MlpPolicy", vb, **kw)
    b.learn(2 * T * vb.num_envs)
    path = os.path.join(tmp_path, "ppo_multi.zip")
    b.save(path)
    cc = PPO.load(path, vb)
    assert cc.multi and cc.n_rows == a.n_rows
    b.close(); b.policy.close()
    cc.learn(2 * T * vb.num_envs, reset_num_timesteps=False)
    assert cc.num_timesteps == a.num_timesteps and cc.iteration == 4
    assert t.equal(cc.policy.params, a.policy.params)
    ma, sa = a.opt.state()
    mc, sc = cc.opt.state()
    assert sa == sc and np.array_equal(ma, mc)
    for x in (a, cc):
        x.close(); x.policy.close()
    va.close(); vb.close()
    # a smoke, not a learning claim: 20 iterations on 256 envs, nothing in the log is NaN
    v = mk(256); v.reset(seed=seed)
    s = PPO("MlpPolicy", v, n_steps=32, n_epochs=4, seed=1)
    s.learn(20 * 32 * 256)
    assert s.iteration == 20 and len(s.log) == 20
    for rec in s.log:
        assert all(np.isfinite(float(x)) for x in rec.values()), rec
        assert np.isfinite(rec["approx_kl"])
    v.batch.check()
    s.close(); s.policy.close(); v.close()
