"""GPU tests of populations of recurrent policies (wg_lstm_pop_*: windgym_amd/csrc/wg_lstm.hip, wg_lstm_ppo.hip, wg_ppo.hip, wg_api.hip;
windgym_amd/recurrent_population.py): every population entry against the loop of single-policy calls it documents, by BIT equality —
no tolerance anywhere in this file."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from recurrent_population_twin import LstmMemberLoop, pop_update, single_update, twin_rollout
import lstm_bptt_twin as tw
from recurrent_ppo_cases import make_spec
from rl_helpers import _torch, _venv, close_all, dev, lstm_members, lstm_policy, pop_hyper

pytestmark = pytest.mark.gpu

N_IN, H = 7, 40             # H: not a multiple of the 32 units of a tile (the defaults of rl_helpers.lstm_members)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Bm", [(1, 33), (3, 40), (16, 2)])
@pytest.mark.parametrize("shared", [False, True], ids=["two-lstms", "shared-lstm"])
@pytest.mark.parametrize("deterministic", [False, True])
def test_act_equals_the_single_calls(P, Bm, shared, deterministic):
    from windgym_amd.recurrent_population import RecurrentPopulation
    t = _torch()
    ms = lstm_members(P, shared=shared)
    pop, loop = RecurrentPopulation(ms), LstmMemberLoop(ms)
    n = P * Bm
    g = t.Generator(device="cuda"); g.manual_seed(P * 100 + Bm)
    obs = t.rand((n, N_IN), device="cuda", generator=g) * 2 - 1
    state = t.randn((P, ms[0].nets, 2, Bm, H), device="cuda", generator=g) * 0.5
    start = (t.rand(n, device="cuda", generator=g) < 0.3).to(t.uint8)
    start[0], start[n - 1] = 1, 0
    seeds, offs = [11 + 3 * m for m in range(P)], [1000 * m + 5 for m in range(P)]
    for es in (start, None):
        got, new = pop.act(obs, state, es, deterministic, counter=9, seed=seeds, row_offset=offs)
        got = [x.clone() for x in got]
        want, wnew = loop.act(obs, state, es, deterministic, counter=9, seed=seeds, row_offset=offs)
        for a, b, k in zip(got, want, ("action", "raw", "logp", "value")):
            assert t.equal(a, b), k
        assert t.equal(new, wnew) and tuple(new.shape) == (P, ms[0].nets, 2, Bm, H)
    # value=False: the critics' LSTMs do not run
    got, new = pop.act(obs, state, start, deterministic, counter=9, seed=seeds, row_offset=offs, value=False)
    want, wnew = loop.act(obs, state, start, deterministic, counter=9, seed=seeds, row_offset=offs, value=False)
    assert got[3] is None and t.equal(got[1], want[1]) and t.equal(new, wnew)
    if P > 1 and not deterministic:
        assert not t.equal(got[1][:Bm], got[1][Bm:2 * Bm])
    close_all(pop, ms)


# 2 ---------------------------------------------------------------------------------------------------------------------
ROLL_KEYS = ("obs", "actions", "raw", "logp", "value", "final_obs", "final_value", "reward", "truncated", "episode_start")


@pytest.mark.parametrize("P,B,T,shared", [(3, 120, 300, False), (2, 16, 40, True)], ids=["P3-B120", "P2-B16-shared"])
def test_rollout_equals_the_loop_of_single_calls(P, B, T, shared):
    """P = 3, B = 120: a global tile of 32 envs would straddle two members; P = 2, B = 16: fewer envs per member than a tile."""
    from windgym_amd.recurrent_population import RecurrentPopulation
    t = _torch()
    va, vb = _venv(B), _venv(B)
    ms = lstm_members(P, va.batch.obs_dim, va.n_turb, 48, shared, (64, 64))
    pop, loop, rec = RecurrentPopulation(ms), LstmMemberLoop(ms), ("power_agent",)
    out = va.rollout(pop, T, record=rec)
    ref, ref_state = twin_rollout(vb, loop, T, pop.initial_state(B), t.ones(B, dtype=t.uint8, device="cuda"), rec=rec)
    assert set(out) == set(ref) | {"lstm_state", "lstm_state0"}
    for k, x in ref.items():
        assert out[k].shape == x.shape and t.equal(out[k], x), k
    Bm = B // P
    assert tuple(out["lstm_state"].shape) == (P, ms[0].nets, 2, Bm, 48) == tuple(out["lstm_state0"].shape)
    assert t.equal(out["lstm_state"], ref_state) and not bool(out["lstm_state0"].any())
    if T >= 300:
        assert int(out["truncated"].sum()) > 0                           # truncations fall inside the rollout
    assert t.equal(out["episode_start"][1:], out["truncated"]) and bool((out["episode_start"][0] == 1).all())
    va.batch.check(); vb.batch.check()
    assert va.batch.get_state() == vb.batch.get_state() and va._policy_steps == vb._policy_steps == T
    assert t.equal(va.batch.obs, out["obs"][T]) and t.equal(va.batch.final_obs, out["final_obs"][T - 1])
    assert t.equal(va.batch.reward, out["reward"][T - 1]) and t.equal(va.batch.truncated, out["truncated"][T - 1])
    # a second rollout continues the first: the kept state and the pending episode starts
    state_T, es_T = out["lstm_state"].clone(), out["episode_start"][T].clone()
    o1 = {k: v.clone() for k, v in va.rollout(pop, 5).items()}
    assert t.equal(o1["lstm_state0"], state_T) and t.equal(o1["episode_start"][0], es_T)
    r1, s1 = twin_rollout(vb, loop, 5, state_T, es_T)
    for k in r1:
        assert t.equal(o1[k], r1[k]), k
    assert t.equal(o1["lstm_state"], s1) and va.batch.get_state() == vb.batch.get_state()
    # reset() marks every env as an episode start; state= overrides the kept state
    va.reset(seed=5)
    o2 = va.rollout(pop, 2, state=state_T)
    assert bool((o2["episode_start"][0] == 1).all()) and t.equal(o2["lstm_state0"], state_T)
    close_all(pop, ms, va, vb)


def test_equal_members_roll_out_what_one_policy_does():
    from windgym_amd.recurrent_population import RecurrentPopulation
    t = _torch()
    P, B, T = 4, 64, 40
    va, vb = _venv(B), _venv(B)
    ms = lstm_members(P, va.batch.obs_dim, va.n_turb, 48, False, (64, 64))
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    pop = RecurrentPopulation(ms)
    a, b = va.rollout(pop, T), vb.rollout(ms[0], T)
    assert set(a) == set(b)
    for k in ROLL_KEYS:
        assert t.equal(a[k], b[k]), k
    for k in ("lstm_state0", "lstm_state"):                              # [P, nets, 2, Bm, H] against [nets, 2, B, H]
        assert t.equal(a[k].permute(1, 2, 0, 3, 4).reshape(b[k].shape), b[k]), k
    assert va.batch.get_state() == vb.batch.get_state()
    close_all(pop, ms, va, vb)


# 3, 4 ------------------------------------------------------------------------------------------------------------------
P3, BM, EPB, E = 3, 40, 16, 2            # minibatches of 16, 16 and 8 envs


@functools.lru_cache(maxsize=None)
def _shards(shared, T):
    """Per member id 0 .. 3: (flat parameters, its own rollout [T (+ 1), BM, ..] as recurrent_ppo_cases makes them, its local permutations)."""
    spec = make_spec(N_IN, H, shared)
    out = []
    for i in range(4):
        flat = tw.random_params(spec, seed=4 + 10 * i)
        roll = tw.random_rollout(spec, flat, T, BM, seed=5 + 10 * i)
        perms = np.stack([np.random.default_rng(100 + 10 * i + e).permutation(BM) for e in range(E)]).astype(np.int32)
        out.append((flat, roll, perms))
    return spec, out


def _result(p, opt, stats):
    mv, step = opt.state()
    return p.params.clone(), mv, step, stats.clone()


def _same(a, b):
    t = _torch()
    return t.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and t.equal(a[3], b[3])


def _run_pop(shared, T, order, nan=(), bad_ids=None, epb=EPB):
    """wg_lstm_pop_update with the members ``order`` (ids of _shards) in that order, each on its own shard -> {id: result}.  ``nan``: ids
    whose parameters and rollout columns are NaN; ``bad_ids``: (id, [(epoch, position, global env id written there)])."""
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    from windgym_amd.recurrent_population import RecurrentPopulation, global_envs
    t = _torch()
    spec, sh = _shards(shared, T)
    P = len(order)
    flats = [np.full_like(sh[i][0], np.nan) if i in nan else sh[i][0] for i in order]
    rolls = []
    for i in order:
        r = dict(sh[i][1])
        if i in nan:
            r = {k: (np.full_like(v, np.nan) if v.dtype == np.float32 else v) for k, v in r.items()}
        rolls.append(r)
    roll = {k: np.concatenate([r[k] for r in rolls], axis=1) for k in rolls[0] if k != "lstm_state0"}
    roll["lstm_state0"] = np.stack([r["lstm_state0"] for r in rolls])                    # [P, nets, 2, BM, H]
    perm = np.stack([global_envs(sh[i][2], m, BM) for m, i in enumerate(order)]).astype(np.int32)
    if bad_ids is not None:
        for e, pos, val in bad_ids[1]:
            perm[order.index(bad_ids[0]), e, pos] = val
    ps = [lstm_policy(spec, f) for f in flats]
    opts = [RecurrentPPOOptimizer(p, T, epb) for p in ps]
    pop = RecurrentPopulation(ps, opts)
    hy = {k: [pop_hyper(4)[k][i] for i in order] for k in pop_hyper(4)}
    keys = list(roll)
    d = dict(zip(keys, dev(*[roll[k] for k in keys])))
    st = pop_update(pop, d, dev(perm)[0], epb, hy)
    res = {i: _result(ps[m], opts[m], st[m]) for m, i in enumerate(order)}
    close_all(pop, opts, ps)
    return res


@functools.lru_cache(maxsize=None)
def _base(shared, T):
    return _run_pop(shared, T, (0, 1, 2))


@functools.lru_cache(maxsize=None)
def _run_single(shared, T, i, bad=(), epb=EPB):
    """wg_lstm_ppo_update of member ``i`` alone on its shard with local env ids; ``bad``: ((epoch, position, local id), ...)."""
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    spec, sh = _shards(shared, T)
    flat, roll, perms = sh[i]
    perms = perms.copy()
    for e, pos, val in bad:
        perms[e, pos] = val
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, T, epb)
    keys = list(roll)
    d = dict(zip(keys, dev(*[roll[k] for k in keys])))
    st = single_update(opt, d, dev(perms)[0], epb, pop_hyper(4), i)
    res = _result(p, opt, st)
    close_all(opt, p)
    return res


@pytest.mark.parametrize("T", [6, 3])                                    # T NT = 6 and 3 blocks (NT = 1): the weight gradient's split below WGLP_SPLIT
@pytest.mark.parametrize("shared", [False, True], ids=["two-lstms", "shared-lstm"])
def test_update_equals_the_single_updates(shared, T):
    """Parameters, Adam's moments and step counts and the statistics of every member == wg_lstm_ppo_update alone on contiguous copies
    of its columns with local env ids; per-member hyper-parameters: normalize_advantage on and off, lr = 0, a max_grad_norm that clips."""
    t = _torch()
    pop = _base(shared, T)
    spec, sh = _shards(shared, T)
    for i in range(P3):
        one = _run_single(shared, T, i)
        assert one[2] == E * 3 and tuple(one[3].shape) == (E, 3, 8)
        assert t.equal(pop[i][0], one[0]), ("params", i)
        assert np.array_equal(pop[i][1], one[1]) and pop[i][2] == one[2], ("adam", i)
        assert t.equal(pop[i][3], one[3]), ("stats", i)
        moved = not t.equal(one[0].cpu(), t.from_numpy(sh[i][0]))
        assert moved == (pop_hyper(4)["learning_rate"][i] != 0.0) and np.abs(one[1]).max() > 0
    assert float(pop[1][3][..., 7].min()) == 1.0 and float(pop[0][3][..., 7].max()) != 1.0      # adv_std: member 1 does not normalise


def test_update_with_the_full_split_and_two_env_tiles():
    """One minibatch of all 40 envs: NT = 2 tiles (the second one of 8 columns), T NT = 12 blocks in WGLP_SPLIT = 8 splits."""
    pop = _run_pop(True, 6, (0, 1, 2), epb=BM)
    for i in range(P3):
        assert _same(pop[i], _run_single(True, 6, i, epb=BM)), i


@pytest.mark.parametrize("shared", [False, True], ids=["two-lstms", "shared-lstm"])
def test_population_of_one_is_the_single_path(shared):
    assert _same(_run_pop(shared, 6, (3,))[3], _run_single(shared, 6, 3))


def test_members_do_not_depend_on_order_or_population_size():
    base = _base(False, 6)
    other = _run_pop(False, 6, (2, 0, 1))
    for i in range(P3):
        assert _same(base[i], other[i]), i
    two = _run_pop(False, 6, (1, 3))
    assert _same(two[1], base[1]) and _same(two[3], _run_single(False, 6, 3))


def test_members_do_not_depend_on_what_the_others_hold():
    t = _torch()
    base = _base(False, 6)
    poisoned = _run_pop(False, 6, (0, 1, 2), nan=(1,))
    assert bool(t.isnan(poisoned[1][0]).all())
    for i in (0, 2):
        assert _same(base[i], poisoned[i]), i


def test_an_env_outside_the_rollout_is_a_column_of_zeros():
    """-1 and B in member 1's lists: what -1 and Bm do in its own single update; the other members keep every bit."""
    base = _base(False, 6)
    B = P3 * BM
    bad = _run_pop(False, 6, (0, 1, 2), bad_ids=(1, [(0, 3, -1), (1, 20, B), (1, 39, -1)]))
    one = _run_single(False, 6, 1, bad=((0, 3, -1), (1, 20, BM), (1, 39, -1)))
    assert _same(bad[1], one) and not _same(bad[1], base[1])
    for i in (0, 2):
        assert _same(base[i], bad[i]), i


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_learn_equals_the_twin_of_single_policy_entries(tmp_path):
    """THE test of the feature: 3 iterations of RecurrentPPOPopulation.learn == rollout by single calls, wg_gae and wg_lstm_ppo_update
    per member on contiguous copies of its columns with the same local permutations; then save, RecurrentPPO.load of one member's zip
    on a shard env, and one more iteration of both."""
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.recurrent import MlpLstmPolicy
    from windgym_amd.recurrent_population import RecurrentPPOPopulation
    from windgym_amd.recurrent_ppo import RecurrentPPO, RecurrentPPOOptimizer
    from windgym_amd.turbine import V80
    t = _torch()
    P, B, T = 2, 16, 8
    Bm = B // P
    va, vb = _venv(B), _venv(B)
    hy = {k: x[:P] for k, x in pop_hyper(P).items()}
    pp = RecurrentPPOPopulation("MlpLstmPolicy", va, n_members=P, n_steps=T, n_epochs=E, seed=[5, 6],
                                policy_kwargs=dict(lstm_hidden_size=40, net_arch=dict(pi=[16], vf=[16])), **hy)
    assert pp.envs_per_batch == 2 and pp.batch_size == 2 * T and pp.n_minibatches == 4
    twins = []
    for m in pp.members:
        q = MlpLstmPolicy(m.n_in, m.n_out, m.H, m.desc["mlp"]["hidden_pi"], m.desc["mlp"]["hidden_vf"], m.shared_lstm, seed=m.seed)
        q.load_state_dict(m.state_dict())
        twins.append(q)
    opts = [RecurrentPPOOptimizer(q, T, pp.envs_per_batch) for q in twins]
    gens = []
    for s in pp.seed:
        g = t.Generator(device="cuda"); g.manual_seed(int(s))
        gens.append(g)
    loop = LstmMemberLoop(twins)
    hyper = [pp.member_hyper(m) for m in range(P)]
    state, start, actions = pp.population.initial_state(B), t.ones(B, dtype=t.uint8, device="cuda"), []
    for it in range(3):
        pp.learn(T * Bm, reset_num_timesteps=False)
        out = {**next(iter(va._rollout_bufs.values())), **{k: v for k, v in va._lstm_pair(pp.population)[3][T].items() if k != "lstm_scratch"}}
        ref, new_state = twin_rollout(vb, loop, T, state, start)
        for k, x in ref.items():
            assert t.equal(out[k], x), (it, k)
        assert t.equal(out["lstm_state0"], state) and t.equal(out["lstm_state"], new_state), it
        actions.append(ref["actions"].clone())
        ref["lstm_state0"] = state
        for m in range(P):
            h = hyper[m]
            c = slice(m * Bm, (m + 1) * Bm)
            col = {k: ref[k][:, c].contiguous() for k in ("obs", "raw", "logp", "episode_start", "reward", "value", "final_value", "truncated")}
            col["advantage"], col["returns"] = opts[m].gae(col["reward"], col["value"], col["final_value"], col["truncated"], h["gamma"], h["gae_lambda"])
            col["lstm_state0"] = state[m].contiguous()
            perm = t.stack([t.randperm(Bm, generator=gens[m], device="cuda") for _ in range(E)]).to(t.int32).contiguous()
            st = opts[m].update(col, perm, pp.envs_per_batch, clip_range=h["clip_range"], vf_coef=h["vf_coef"], ent_coef=h["ent_coef"],
                                normalize_advantage=h["normalize_advantage"], learning_rate=h["learning_rate"], max_grad_norm=h["max_grad_norm"])
            assert t.equal(pp._stats[m], st), (it, m)
            assert t.equal(pp.members[m].params, twins[m].params), (it, m)
            (mva, sa), (mvb, sb) = pp.opts[m].state(), opts[m].state()
            assert sa == sb == (it + 1) * E * pp.n_minibatches and np.array_equal(mva, mvb), (it, m)
        state, start = new_state, ref["episode_start"][T].clone()
        vb.batch.metrics(reset_after=True)                                # (a logged iteration consumes the batch's episode sums)
        assert va.batch.get_state() == vb.batch.get_state(), it
    assert len(pp.log) == 3 and len(pp.log[-1]) == P and all(np.isfinite(r["loss"]) for r in pp.log[-1])
    # save; member 1 alone on a shard env brought to the shard's state by the recorded actions; one more iteration of both
    paths = pp.save(os.path.join(tmp_path, "pop"))
    assert [os.path.basename(p) for p in paths] == ["member_00.zip", "member_01.zip"]
    m = 1
    vs = WindFarmVecEnv(V80(), Bm, yaml_dict=presets.bench_cfg2_config(), seed=77, as_torch=True, turbtype="None", n_passthrough=1,
                        n_rotor_pts=16).shard(m, P)
    vs.reset(seed=77)
    for a in t.cat(actions):
        vs.batch.step(a[m * Bm:(m + 1) * Bm].contiguous())
    assert t.equal(vs.batch.obs, va.batch.obs[m * Bm:(m + 1) * Bm])
    one = RecurrentPPO.load(paths[m], vs)
    assert t.equal(one.policy.params, pp.members[m].params) and one.envs_per_batch == pp.envs_per_batch
    pp.learn(T * Bm, reset_num_timesteps=False)
    one.learn(T * Bm, reset_num_timesteps=False)
    assert t.equal(one.policy.params, pp.members[m].params) and not t.equal(one.policy.params, twins[m].params)
    (mva, sa), (mvb, sb) = pp.opts[m].state(), one.opt.state()
    assert sa == sb == 4 * E * pp.n_minibatches and np.array_equal(mva, mvb)
    assert t.equal(vs._lstm_pair(one.policy)[1], va._lstm_pair(pp.population)[1][m])
    one.close(); pp.close()
    close_all(one.policy, opts, twins, pp.members, va, vb, vs)


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from windgym_amd.recurrent_population import RecurrentPopulation, RecurrentPPOPopulation
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    from windgym_amd.site import hornsrev1_site
    t = _torch()
    a, b = lstm_members(2)
    arr = lambda hs: (C.c_void_p * len(hs))(*[h.value for h in hs])        # noqa: E731
    L, h = a.L, C.c_void_p()

    def create(ms, opts=None):
        from windgym_amd.binding import _chk
        _chk(L.wg_lstm_pop_create(arr([m._lstm for m in ms]), arr([m.mlp._h for m in ms]), None if opts is None else arr([o._h for o in opts]),
                                  len(ms), C.byref(h)), "wg_lstm_pop_create")
    # the classes refuse on the host, the ABI by name where a caller goes past them
    wide, one_net, heads = lstm_members(1, hidden=48)[0], lstm_members(1, shared=True)[0], lstm_members(1, heads=(16, 16))[0]
    for bad in (wide, one_net, heads):
        with pytest.raises(ValueError, match="member 1 has another architecture"):
            RecurrentPopulation([a, bad])
    with pytest.raises(ValueError, match="hidden size and number of nets"):
        create([a, wide])
    with pytest.raises(ValueError, match="hidden size and number of nets"):
        create([a, one_net])
    with pytest.raises(ValueError, match="member 1's head has another architecture"):
        create([a, heads])
    with pytest.raises(ValueError, match="member 1 is the same policy"):
        RecurrentPopulation([a, a])
    with pytest.raises(ValueError, match="member 1 holds the same handle as member 0"):
        create([a, a])
    with pytest.raises(ValueError, match="1 .. 16 members"):
        RecurrentPopulation([])
    oa, ob = RecurrentPPOOptimizer(a, 4, 4), RecurrentPPOOptimizer(b, 4, 4)
    with pytest.raises(ValueError, match="created for another pair"):
        RecurrentPopulation([a, b], [ob, oa])
    pop, pop2 = RecurrentPopulation([a, b]), RecurrentPopulation([a, b], [oa, ob])
    with pytest.raises(ValueError, match="does not divide by 2"):
        pop.act(t.zeros((7, N_IN), device="cuda"), t.zeros((2, 2, 2, 3, H), device="cuda"))
    # the update: no optimisers, B % P, T > T_max, a minibatch > Bm_max, max_grad_norm — nothing is enqueued
    spec = make_spec(N_IN, H, False)
    roll = tw.random_rollout(spec, tw.random_params(spec, 1), 4, 8, seed=2)
    roll["lstm_state0"] = np.stack([roll["lstm_state0"][:, :, :4], roll["lstm_state0"][:, :, 4:]])
    d = dict(zip(roll, dev(*roll.values())))
    perm = dev(np.stack([np.arange(4, dtype=np.int32)[None], 4 + np.arange(4, dtype=np.int32)[None]]))[0]
    hy = {k: x[:2] for k, x in pop_hyper(2).items()}
    w0 = [a.params.clone(), b.params.clone()]
    with pytest.raises(ValueError, match="created without optimisers"):
        pop_update(pop, d, perm, 4, hy)
    with pytest.raises(NotImplementedError, match="member 0: 5 envs in a minibatch > the Bm_max = 4"):
        pop_update(pop2, d, perm, 5, hy)
    with pytest.raises(ValueError, match="member 1: max_grad_norm"):
        pop_update(pop2, d, perm, 4, dict(hy, max_grad_norm=[0.5, 0.0]))
    d7 = {k: (v[:, :7].contiguous() if k != "lstm_state0" else v) for k, v in d.items()}
    with pytest.raises(ValueError, match="B = 7 does not divide by 2"):
        pop_update(pop2, d7, perm, 4, hy)
    o3 = RecurrentPPOOptimizer(b, 3, 4)
    pop3 = RecurrentPopulation([a, b], [oa, o3])
    with pytest.raises(NotImplementedError, match="member 1: T = 4 > the T_max = 3"):
        pop_update(pop3, d, perm, 4, hy)
    assert t.equal(a.params, w0[0]) and t.equal(b.params, w0[1]) and oa.state()[1] == 0 == ob.state()[1]
    # the closed loop: B % P, sample_site, a multi-agent env; a refused rollout leaves the env as it was
    v = _venv(9)
    blob = v.batch.get_state()
    pv = RecurrentPopulation(lstm_members(2, v.batch.obs_dim, v.n_turb))
    with pytest.raises(ValueError, match="does not divide by 2"):
        v.rollout(pv, 4)
    with pytest.raises(ValueError, match="does not divide by 2"):
        RecurrentPPOPopulation("MlpLstmPolicy", v, n_members=2)
    from windgym_amd.binding import CRolloutBufs, CRolloutLstmBufs, _chk
    z = t.zeros(9 * 4 * 64, device="cuda")
    cb = CRolloutBufs(*[z.data_ptr()] * 9, 0, None, None)
    lb = CRolloutLstmBufs(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr())
    u = (C.c_uint64 * 2)(1, 1)
    with pytest.raises(ValueError, match="n_envs = 9 does not divide by 2"):
        _chk(L.wg_lstm_pop_rollout(v.batch._h, pv._h, 2, 0, u, 0, u, C.byref(cb), C.byref(lb), None), "wg_lstm_pop_rollout")
    assert v.batch.get_state() == blob
    vs = _venv(8, sample_site=hornsrev1_site())
    with pytest.raises(NotImplementedError, match="sample_site"):
        vs.rollout(pv, 2)

    class Multi:
        possible_agents = ["a"]
    with pytest.raises(NotImplementedError, match="WindFarmVecEnvMulti"):
        RecurrentPPOPopulation("MlpLstmPolicy", Multi(), n_members=2)
    for k in ("curriculum", "normalize"):
        with pytest.raises(NotImplementedError, match=k):
            RecurrentPPOPopulation("MlpLstmPolicy", v, n_members=3, **{k: object()})
    with pytest.raises(ValueError, match="multiple of n_steps"):
        RecurrentPPOPopulation("MlpLstmPolicy", v, n_members=3, n_steps=8, batch_size=20)
    close_all(pop, pop2, pop3, pv, oa, ob, o3, a, b, wide, one_net, heads, pv.members, v, vs)


# the tool --------------------------------------------------------------------------------------------------------------
def test_bench_cli_reports_the_members_leg():
    """tools/bench_recurrent_ppo.py --members at a toy size: the population leg runs and the line has the documented keys."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_recurrent_ppo.py"), "--members", "2", "--sizes", "8x16", "--n-steps", "4",
                        "--epochs", "1", "--reps", "1", "--preroll", "0", "--legs", "pop"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-400:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["members"] == 2 and res["envs_per_member"] == 8 and res["hidden"] == 16, res
    assert res["rollout_pop_ms"] > 0 and res["train_pop_ms"] > 0 and len(res["train_pop_ms_all"]) == 1, res
