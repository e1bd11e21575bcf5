"""GPU tests of populations (wg_pop_*: windgym_amd/csrc/wg_policy.hip, wg_ppo.hip, wg_api.hip; windgym_amd/population.py): every
population entry against the loop of single-policy calls it documents, by BIT equality."""
import functools

import numpy as np
import pytest

import rl_helpers
from population_twin import MemberLoop, twin_rollout, twin_train
from rl_helpers import _torch, _venv, close_all, mlp_members, pop_hyper, rollout_equals_the_loop

pytestmark = pytest.mark.gpu
make = functools.partial(rl_helpers.make, dtype=np.float64)        # (test_gpu_ppo.py's policies)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Bm", [(1, 64), (2, 96), (3, 50), (16, 32), (16, 5)])
@pytest.mark.parametrize("deterministic", [False, True])
def test_act_equals_the_single_calls(P, Bm, deterministic):
    from windgym_amd.population import Population
    t = _torch()
    ms = mlp_members(P)
    pop, loop = Population(ms), MemberLoop(ms)
    obs = t.rand((P * Bm, 32), device="cuda") * 2 - 1
    seeds, offs = [11 + 3 * m for m in range(P)], [1000 * m + 5 for m in range(P)]
    got = [x.clone() for x in pop.act(obs, deterministic, counter=9, seed=seeds, row_offset=offs)]
    want = loop.act(obs, deterministic, counter=9, seed=seeds, row_offset=offs)
    for g, w, k in zip(got, want, ("action", "raw", "logp", "value")):
        assert t.equal(g, w), k
    assert t.equal(pop.value(obs), loop.value(obs))
    if P > 1 and not deterministic:
        assert not t.equal(got[1][:Bm], got[1][Bm:2 * Bm])
    close_all(pop, ms)


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3])
def test_rollout_equals_the_loop_of_single_calls(P):
    from windgym_amd.population import Population
    va, vb = _venv(48), _venv(48)
    ms = mlp_members(P, va.batch.obs_dim, (64, 64), va.n_turb)
    pop, T, rec = Population(ms), 300, ("power_agent", "yaw_agent")
    out = va.rollout(pop, T, record=rec)
    rollout_equals_the_loop(va, vb, MemberLoop(ms), T, rec=rec, out=out)       # buffers, wg_state blob, persistent outputs
    close_all(pop, ms, va, vb)


def test_equal_members_roll_out_what_one_policy_does():
    from windgym_amd.population import Population
    t = _torch()
    va, vb = _venv(64), _venv(64)
    ms = mlp_members(4, va.batch.obs_dim, (64, 64), va.n_turb)
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    pop = Population(ms)
    a, b = va.rollout(pop, 40), vb.rollout(ms[0], 40)
    assert set(a) == set(b)
    for k in a:
        assert t.equal(a[k], b[k]), k
    assert va.batch.get_state() == vb.batch.get_state()
    close_all(pop, ms, va, vb)


# 3, 5, 6, 8 ------------------------------------------------------------------------------------------------------------
def _twin_population(pp, vb):
    """single-policy twins of a PPOPopulation's members (same initial weights), their optimisers and generators"""
    from windgym_amd.policy import MlpPolicy
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    tw = []
    for m in pp.members:
        q = MlpPolicy(m.n_in, m.n_out, m.desc["hidden_pi"], m.desc["hidden_vf"], m.desc["activation"], seed=m.seed)
        q.load_state_dict(m.state_dict())
        tw.append(q)
    gens = []
    for s in pp.seed:
        g = t.Generator(device="cuda")
        g.manual_seed(0 if s is None else int(s))
        gens.append(g)
    return tw, [PPOOptimizer(q) for q in tw], gens


@pytest.mark.parametrize("P,B,T,bs", [(3, 48, 16, None), (4, 64, 12, 50), (1, 32, 16, None)])
def test_learn_equals_the_twin_of_single_policy_entries(P, B, T, bs):
    """THE test of the feature: >= 3 iterations of PPOPopulation.learn == rollout by single calls, wg_gae and wg_ppo_update per
    member on contiguous copies of its columns, with the same local permutations."""
    from windgym_amd.population import PPOPopulation
    t = _torch()
    va, vb = _venv(B), _venv(B)
    E = 3
    pp = PPOPopulation("MlpPolicy", va, n_members=P, n_steps=T, n_epochs=E, batch_size=bs, seed=list(range(5, 5 + P)), **pop_hyper(P))
    tw, opts, gens = _twin_population(pp, vb)
    loop = MemberLoop(tw)
    hyper = [pp.member_hyper(m) for m in range(P)]
    before = [m.params.clone() for m in pp.members]
    for it in range(3):
        pp.learn(T * B // P, log_interval=1, reset_num_timesteps=False)
        ref = twin_rollout(vb, loop, T)
        bufs = next(iter(va._rollout_bufs.values()))                      # (the population's buffers of this iteration are still valid)
        for k, x in ref.items():
            assert t.equal(bufs[k], x), (it, k)
        stats = twin_train(opts, ref, gens, E, pp.batch_size, hyper, [h["learning_rate"] for h in hyper], [h["clip_range"] for h in hyper])
        for m in range(P):
            assert t.equal(pp._stats[m], stats[m]), (it, m)
            assert t.equal(pp.members[m].params, tw[m].params), (it, m)
            (mva, sa), (mvb, sb) = pp.opts[m].state(), opts[m].state()
            assert sa == sb == (it + 1) * E * pp.n_minibatches and np.array_equal(mva, mvb), (it, m)
        vb.batch.metrics(reset_after=True)                                # (a logged iteration consumes the batch's episode sums, as PPO.learn does)
    assert va.batch.get_state() == vb.batch.get_state()
    for m in range(P):                                                    # per-member hyper-parameters act: lr = 0 keeps its params
        moved = not t.equal(pp.members[m].params, before[m])
        assert moved == (hyper[m]["learning_rate"] != 0.0), m
    assert len(pp.log) == 3 and len(pp.log[-1]) == P and pp.log[-1][P - 1]["member"] == P - 1
    assert all(np.isfinite(r["loss"]) and np.isfinite(r["explained_variance"]) for r in pp.log[-1])
    x = t.rand((64, pp.members[0].n_in), device="cuda")
    for m in range(P):                                                    # the packed copies followed (repack after every step)
        assert t.equal(pp.members[m].act(x, deterministic=True)[1], tw[m].act(x, deterministic=True)[1])
    pp.close(); close_all(opts, tw, pp.members, va, vb)


def test_population_of_one_is_ppo():
    from windgym_amd.population import PPOPopulation
    from windgym_amd.ppo import PPO
    t = _torch()
    va, vb = _venv(32), _venv(32)
    kw = dict(n_steps=16, n_epochs=3, gamma=0.97, ent_coef=0.01, learning_rate=1e-3)
    pp = PPOPopulation("MlpPolicy", va, n_members=1, seed=4, **kw).learn(3 * 16 * 32)
    ppo = PPO("MlpPolicy", vb, seed=4, **kw).learn(3 * 16 * 32)
    assert t.equal(pp.members[0].params, ppo.policy.params)
    assert np.array_equal(pp.opts[0].state()[0], ppo.opt.state()[0])
    assert va.batch.get_state() == vb.batch.get_state()
    for k in ("loss", "pi_loss", "v_loss", "approx_kl", "explained_variance"):
        assert pp.log[-1][0][k] == ppo.log[-1][k], k
    pp.close(); ppo.close(); close_all(pp.members, ppo.policy, va, vb)


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_members_are_independent():
    """Other weights, seeds and hyper-parameters in the members != 0 leave member 0's rollout columns and parameters alone."""
    from windgym_amd.population import PPOPopulation
    t = _torch()
    P, B, T = 3, 48, 8
    hy = pop_hyper(3)

    def run(others_changed):
        v = _venv(B)
        kw, sd = dict(hy), [5, 6, 7]
        if others_changed:
            sd = [5, 91, 92]
            kw = {k: [x[0]] + [pop_hyper(4)[k][3]] * 2 for k, x in hy.items()}
        pp = PPOPopulation("MlpPolicy", v, n_members=P, n_steps=T, n_epochs=2, seed=sd, **kw).learn(2 * T * B // P)
        bufs = {k: x.clone() for k, x in next(iter(v._rollout_bufs.values())).items()}
        params = [m.params.clone() for m in pp.members]
        pp.close(); close_all(pp.members, v)
        return bufs, params
    (base, pb), (other, po) = run(False), run(True)
    Bm = B // P
    assert t.equal(pb[0], po[0]) and not t.equal(pb[1], po[1])
    for k in ("obs", "actions", "raw", "logp", "value", "final_value", "reward", "truncated"):
        assert t.equal(base[k][:, :Bm], other[k][:, :Bm]), k
    assert not t.equal(base["actions"][:, Bm:], other["actions"][:, Bm:])


def test_update_is_permuted_with_the_members():
    """wg_pop_update on one batch with the members listed in another order (and their row shares swapped with them) gives each
    member the same parameters: nothing depends on the index m."""
    from windgym_amd.population import Population, global_rows
    from windgym_amd.ppo import PPOOptimizer
    from windgym_amd.binding import CPpoBatch, CPpoHyper
    import ctypes as C
    from rl_helpers import batch, dev
    t = _torch()
    P, Bm, T, E, bs = 2, 40, 5, 2, 64
    B, rows_m = P * Bm, T * Bm
    res = []
    for order in ([0, 1], [1, 0]):
        ms = [make(32, (64, 64), 16, seed=3 + 7 * i) for i in range(P)]
        pol = [ms[i][0] for i in order]
        opts = [PPOOptimizer(p) for p in pol]
        pop = Population(pol, opts)
        parts = [dev(*batch(ms[i][1], 32, 16, rows_m, "tanh", seed=20 + i)) for i in order]      # the member's own rows travel with it
        cols = [t.stack([parts[m][j].view(T, Bm, -1) for m in range(P)], dim=1) for j in range(5)]   # [T, P, Bm, ..] = [T, B, ..]
        d = [c.reshape(T * B, -1).contiguous() for c in cols]
        g = t.Generator(device="cuda"); g.manual_seed(1)
        local = [t.stack([t.randperm(rows_m, generator=g, device="cuda") for _ in range(E)]) for _ in range(P)]
        local = [local[i] for i in order]
        perm = t.stack([global_rows(local[m], m, B, Bm) for m in range(P)]).to(t.int32).contiguous()
        b = CPpoBatch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), T * B)
        hp = (CPpoHyper * P)(*[CPpoHyper(0.2, 0.5, 0.01 * (i + 1), 1) for i in order])
        lr = (C.c_float * P)(*[1e-3 * (i + 1) for i in order])
        mg = (C.c_float * P)(0.5, 0.5)
        params = (C.c_void_p * P)(*[p.params.data_ptr() for p in pol])
        pop._chk(pop.L.wg_pop_update(pop._h, params, C.byref(b), perm.data_ptr(), E, bs, hp, lr, mg, None, pop._stream()), "wg_pop_update")
        out = {i: pol[m].params.clone() for m, i in enumerate(order)}
        res.append(out)
        close_all(pop, opts, pol)
    for i in range(P):
        assert t.equal(res[0][i], res[1][i]), i


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_member_equals_ppo_on_its_shard():
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.population import PPOPopulation
    from windgym_amd.ppo import PPO
    from windgym_amd.turbine import V80
    t = _torch()
    P, B, T = 2, 32, 16
    va = _venv(B)
    hy = {k: x[:P] for k, x in pop_hyper(P).items()}
    pp = PPOPopulation("MlpPolicy", va, n_members=P, n_steps=T, n_epochs=2, seed=[5, 6], **hy).learn(3 * T * B // P)
    for m in range(P):
        vs = WindFarmVecEnv(V80(), B // P, yaml_dict=presets.bench_cfg2_config(), seed=77, as_torch=True, turbtype="None", n_passthrough=1,
                            n_rotor_pts=16).shard(m, P)
        vs.reset(seed=77)
        ppo = PPO("MlpPolicy", vs, seed=5 + m, **pp.member_hyper(m))
        ppo.learn(3 * T * B // P)
        assert t.equal(ppo.policy.params, pp.members[m].params), m
        ppo.close(); close_all(ppo.policy, vs)
    pp.close(); close_all(pp.members, va)


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_widest_layers():
    from windgym_amd.population import Population
    t = _torch()
    ms = mlp_members(2, 2048, (256, 256), 16)
    pop, loop = Population(ms), MemberLoop(ms)
    obs = t.rand((2 * 40, 2048), device="cuda") * 2 - 1
    got = [x.clone() for x in pop.act(obs, counter=2, seed=[1, 2], row_offset=[0, 7])]
    for g, w in zip(got, loop.act(obs, counter=2, seed=[1, 2], row_offset=[0, 7])):
        assert t.equal(g, w)
    close_all(pop, ms)


def test_refusals():
    import ctypes as C
    from windgym_amd.policy import MlpPolicy
    from windgym_amd.population import Population, PPOPopulation
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    a, b = mlp_members(2)
    with pytest.raises(ValueError, match="1 .. 16 members"):
        Population([])
    with pytest.raises(ValueError, match="member 1 is the same policy as member 0"):
        Population([a, a])
    c = make(32, (64, 32), 16)[0]
    with pytest.raises(ValueError, match="member 1 has another architecture"):
        Population([a, c])
    s = MlpPolicy(32, 16, (64, 64), (64, 64), n_in_vf=48)
    with pytest.raises(ValueError, match="member 1 is a split policy"):
        Population([a, s])
    oa, ob = PPOOptimizer(a), PPOOptimizer(b)
    with pytest.raises(ValueError, match="created for another policy"):
        Population([a, b], [ob, oa])
    pop = Population([a, b])
    with pytest.raises(ValueError, match="does not divide by 2"):
        pop.act(t.zeros((7, 32), device="cuda"))
    x = t.zeros((8, 32), device="cuda")
    perm = t.zeros((2, 1, 4), dtype=t.int32, device="cuda")
    from windgym_amd.binding import CPpoBatch, CPpoHyper
    bt = CPpoBatch(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 8)
    hp = (CPpoHyper * 2)(CPpoHyper(0.2, 0.5, 0.0, 1), CPpoHyper(0.2, 0.5, 0.0, 1))
    f = (C.c_float * 2)(0.5, 0.5)
    params = (C.c_void_p * 2)(a.params.data_ptr(), b.params.data_ptr())
    with pytest.raises(ValueError, match="created without optimisers"):
        pop._chk(pop.L.wg_pop_update(pop._h, params, C.byref(bt), perm.data_ptr(), 1, 4, hp, f, f, None, None), "wg_pop_update")
    pop2 = Population([a, b], [oa, ob])
    bt.n_rows = 7
    with pytest.raises(ValueError, match="do not divide by 2"):
        pop2._chk(pop2.L.wg_pop_update(pop2._h, params, C.byref(bt), perm.data_ptr(), 1, 4, hp, f, f, None, None), "wg_pop_update")
    bt.n_rows = 8
    f0 = (C.c_float * 2)(0.5, 0.0)
    with pytest.raises(ValueError, match="member 1: max_grad_norm"):
        pop2._chk(pop2.L.wg_pop_update(pop2._h, params, C.byref(bt), perm.data_ptr(), 1, 4, hp, f, f0, None, None), "wg_pop_update")
    v = _venv(9)
    with pytest.raises(ValueError, match="does not divide by 2"):
        PPOPopulation("MlpPolicy", v, n_members=2)
    pv = Population(mlp_members(2, v.batch.obs_dim, (64, 64), v.n_turb))
    with pytest.raises(ValueError, match="does not divide by 2"):
        v.rollout(pv, 4)
    g = (C.c_float * 2)(0.9, 0.9)
    with pytest.raises(ValueError, match="wg_gae_pop: P = 2"):
        pop._chk(pop.L.wg_gae_pop(2, 7, 2, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), g, g, x.data_ptr(), x.data_ptr(), None), "wg_gae_pop")
    close_all(pop, pop2, pv, oa, ob, a, b, c, s, v)
