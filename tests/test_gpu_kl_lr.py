"""The KL-adaptive learning rate on the device (include/windgym_hip.h: wg_ppo_set_kl_lr, wg_lstm_ppo_set_kl_lr): every entry that takes
the rule against the documented loop of grad + apply(lr_k) with lr_k replayed on the host in numpy float32 (tests/kl_lr_cases.py), bit
for bit — one policy, the centralised critic, the recurrent trainer, both populations — and the trainers end to end."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import lstm_bptt_twin as tw
from kl_lr_cases import F, np_rule, replay
from recurrent_population_twin import COLUMNS
from rl_helpers import _torch, _venv, batch, close_all, dev, lstm_members, make, shared_batch

pytestmark = pytest.mark.gpu

KW = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)
E = 3
SHAPES = {"small": (5, (8,), 2, 50, 16), "shipped": (32, (64, 64), 16, 1000, 300)}       # n_in, hidden, n_out, rows, batch_size
# (rule, starting rate): every minibatch but the first steps down and reaches lr_min / up and reaches lr_max, within 12 minibatches
DOWN = (dict(desired_kl=1e-12, factor=1.5, lr_min=1e-3, lr_max=1e-2), 1e-2)
UP = (dict(desired_kl=1e3, factor=1.5, lr_min=1e-5, lr_max=2e-4), 1e-5)


def bits(x):
    return np.asarray(x, F).view(np.uint32)


def rule_of(d):
    return np_rule(d["desired_kl"], d["factor"], d["lr_min"], d["lr_max"])


def blocks(n, bs):
    return [min(bs, n - s) for s in range(0, n, bs)]


@functools.lru_cache(maxsize=None)
def case(shape, agents=1):
    """The rows of a shape (host arrays; ``agents`` > 1: rl_helpers.shared_batch) and E permutations whose minibatches alternate between
    rows collected almost on-policy (logp_old = the true log-probability + N(0, 0.02): approx_kl about 2e-4) and rows far off it
    (+ N(0, 0.6): about 0.2), so that an update meets both sides of a band — even minibatches the former, odd ones the latter."""
    n_in, hidden, n_out, n, bs = SHAPES[shape]
    rng = np.random.default_rng(17)
    from oracle import policy_oracle as po
    if agents == 1:
        p, sd = make(n_in, hidden, n_out)
        rows = list(batch(sd, n_in, n_out, n, "tanh", seed=5))
        lp = 2                                                             # (obs, raw, logp_old, adv, ret)
        mean, _ = po.forward(sd, rows[0], "tanh")
    else:
        n = -(-n // agents) * agents                                       # agent rows: the next multiple of `agents`
        p, sd = make(n_in, hidden, n_out, n_in_vf=n_in + 3)
        rows = list(shared_batch(sd, n_in, n_in + 3, n_out, n // agents, agents, "tanh", seed=5))
        lp = 3                                                             # (obs, obs_vf, raw, logp_old, adv, ret)
        mean = po._net(sd, "mlp_extractor.policy_net", "action_net", rows[0], "tanh")
    p.close()
    sizes = blocks(n, bs)
    n_low = sum(sizes[0::2])
    # the helpers' logp_old is the true log-probability + N(0, 0.3): keep their draw, rescaled per row
    z = (rows[lp - 1] - mean) / np.exp(sd["log_std"])
    logp = np.sum(-0.5 * z * z - sd["log_std"] - 0.5 * np.log(2 * np.pi), axis=1)
    eps = (rows[lp].astype(np.float64) - logp) / 0.3                       # ~ N(0, 1)
    sigma = np.where(np.arange(n) < n_low, 0.02, 0.6)
    rows[lp] = (logp + sigma * eps).astype(F)
    perms = []
    for e in range(E):
        low, high = list(rng.permutation(n_low)), list(n_low + rng.permutation(n - n_low))
        p = []
        for k, s in enumerate(sizes):
            src = low if k % 2 == 0 else high
            p += src[:s]
            del src[:s]
        assert sorted(p) == list(range(n))
        perms.append(p)
    return tuple(rows), np.array(perms, np.int32), n, bs, (n_in, hidden, n_out)


def pair(shape, agents=1):
    """Two equal policies with their optimisers, the device rows as update() / grad() take them and the permutations."""
    from windgym_amd.ppo import PPOOptimizer
    rows, perms, n, bs, (n_in, hidden, n_out) = case(shape, agents)
    vf = {} if agents == 1 else dict(n_in_vf=n_in + 3)
    (pa, _), (pb, _) = make(n_in, hidden, n_out, **vf), make(n_in, hidden, n_out, **vf)
    d = dev(*rows)
    if agents == 1:
        args, kw = d, dict(KW)
    else:
        obs, obs_vf, raw, logp, adv, ret = d
        args, kw = [obs, raw, logp, adv, ret], dict(KW, obs_vf=obs_vf, agents=agents)
    return pa, pb, PPOOptimizer(pa), PPOOptimizer(pb), args, kw, dev(perms)[0], n, bs


def lr_word(x):
    t = _torch()
    return t.full((1,), float(F(x)), dtype=t.float32, device="cuda")


def loop_equals(oa, ob, pa, pb, args, kw, perm, n, bs, sa, lr0, rule, lr_end):
    """Handle B's grad + apply(lr_k), lr_k replayed from A's own approx_kl, == what A's update left: every record, the parameters,
    the packed copies, Adam's state and the final rate.  -> lr_k"""
    t = _torch()
    n_mb = -(-n // bs)
    lrs = replay(lr0, sa[..., 3].cpu().numpy(), rule)
    for e in range(E):
        for k in range(n_mb):
            idx = perm[e, k * bs:min(n, (k + 1) * bs)].contiguous()
            g, st = ob.grad(*args, index=idx, **kw)
            assert t.equal(st, sa[e, k]), (e, k)
            ob.apply(g, learning_rate=float(lrs[e * n_mb + k]), max_grad_norm=0.5)
    assert t.equal(pa.params, pb.params)
    (ma, na), (mb, nb) = oa.state(), ob.state()
    assert na == nb and np.array_equal(ma, mb)
    assert bits(lr_end.cpu().numpy())[0] == bits(lrs[-1])
    return lrs


def mixed_rule(args, kw, perm, bs, shape, agents, lr0):
    """desired_kl from a fixed-rate pilot run on the same data: the geometric mean of the least and the largest approx_kl after the
    first minibatch."""
    from windgym_amd.ppo import PPOOptimizer
    _, _, _, _, (n_in, hidden, n_out) = case(shape, agents)
    p, _ = make(n_in, hidden, n_out, **({} if agents == 1 else dict(n_in_vf=n_in + 3)))
    o = PPOOptimizer(p)
    kl = o.update(*args, perm, bs, learning_rate=lr0, max_grad_norm=0.5, **kw)[..., 3].cpu().numpy().reshape(-1)[1:]
    close_all(o, p)
    assert (kl > 0).all()
    return dict(desired_kl=float(np.sqrt(kl.min() * kl.max())), factor=1.5, lr_min=1e-5, lr_max=1e-2)


# 1, 5 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["down", "up", "mixed"])
@pytest.mark.parametrize("shape, agents", [("small", 1), ("shipped", 1), ("small", 3)], ids=["small", "shipped", "central"])
def test_update_equals_the_documented_loop(shape, agents, regime):
    """wg_ppo_update / wg_ppo_update_shared (agents = 3, n_in_vf = n_in + 3, 51 agent rows: the next multiple of 3) with the rule set."""
    pa, pb, oa, ob, args, kw, perm, n, bs = pair(shape, agents)
    n_mb = -(-n // bs)
    assert n % bs != 0 and E * n_mb == 12
    if regime == "mixed":
        lr0 = 3e-4
        rd = mixed_rule(args, kw, perm, bs, shape, agents, lr0)
    else:
        rd, lr0 = DOWN if regime == "down" else UP
    rule, lr = rule_of(rd), lr_word(lr0)
    oa.set_kl_lr(rd, lr)
    sa = oa.update(*args, perm, bs, learning_rate=7.0, max_grad_norm=0.5, **kw)            # (its own learning_rate is ignored)
    lrs = loop_equals(oa, ob, pa, pb, args, kw, perm, n, bs, sa, lr0, rule, lr)
    print(regime, shape, agents, rd, "approx_kl", sa[..., 3].cpu().numpy().reshape(-1), "lr", lrs)
    down, up = rule[3], rule[2]
    if regime == "down":
        ref = np.array([max(rule[4], F(lr0))] + [0] * 11, F)
        for k in range(1, 12):
            ref[k] = max(rule[4], F(ref[k - 1] * down))
        assert np.array_equal(bits(lrs), bits(ref)) and lrs[-1] == rule[4] and lrs[1] < lrs[0]
    elif regime == "up":
        assert (sa[..., 3] > 0).all()
        ref = np.array([F(lr0)] + [0] * 11, F)
        for k in range(1, 12):
            ref[k] = min(rule[5], F(ref[k - 1] * up))
        assert np.array_equal(bits(lrs), bits(ref)) and lrs[-1] == rule[5] and lrs[1] > lrs[0]
    else:
        steps = np.sign(np.diff(lrs.astype(np.float64)))
        assert (steps > 0).any() and (steps < 0).any()                      # a condition on the inputs, not on the code under test
    close_all(oa, ob, pa, pb)


# 2 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["small", "shipped"])
def test_a_rule_that_never_fires_leaves_the_bits_alone(shape):
    """factor = 1: the device-side step_size expression is the host's."""
    t = _torch()
    pa, pb, oa, ob, args, kw, perm, n, bs = pair(shape)
    lr = lr_word(7.7e-4)
    oa.set_kl_lr(dict(desired_kl=0.01, factor=1.0, lr_min=1e-5, lr_max=1e-2), lr)
    sa = oa.update(*args, perm, bs, learning_rate=0.5, max_grad_norm=0.5, **kw)
    sb = ob.update(*args, perm, bs, learning_rate=float(F(7.7e-4)), max_grad_norm=0.5, **kw)
    assert t.equal(sa, sb) and t.equal(pa.params, pb.params) and bits(lr.cpu().numpy())[0] == bits(7.7e-4)
    (ma, na), (mb, nb) = oa.state(), ob.state()
    assert na == nb == 12 and np.array_equal(ma, mb)
    x = args[0][:32].contiguous()
    assert t.equal(pa.act(x, deterministic=True)[1], pb.act(x, deterministic=True)[1])
    close_all(oa, ob, pa, pb)


def raw_update(o, args, perm, bs, lr, stats_ptr):
    """wg_ppo_update through the ABI (stats_ptr may be None = NULL)"""
    b, rows, shared = o._batch(*args)
    assert not shared
    o._chk(o.L.wg_ppo_update(o._h, o.policy.params.data_ptr(), C.byref(b), perm.data_ptr(), perm.shape[0], int(bs),
                             C.byref(o._hyper(**KW)), float(lr), 0.5, stats_ptr, o.policy._stream()), "wg_ppo_update")


# 3 -------------------------------------------------------------------------------------------------------------------------------------
def test_stats_out_null_with_the_rule_set():
    t = _torch()
    pa, pb, oa, ob, args, kw, perm, n, bs = pair("small")
    rd = mixed_rule(args, kw, perm, bs, "small", 1, 3e-4)
    la, lb = lr_word(3e-4), lr_word(3e-4)
    oa.set_kl_lr(rd, la); ob.set_kl_lr(rd, lb)
    raw_update(oa, args, perm, bs, 0.0, None)
    ob.update(*args, perm, bs, max_grad_norm=0.5, **kw)
    assert t.equal(pa.params, pb.params) and t.equal(la, lb) and float(la) != float(F(3e-4))
    assert oa.state()[1] == ob.state()[1] == 12 and np.array_equal(oa.state()[0], ob.state()[0])
    close_all(oa, ob, pa, pb)


# 4 -------------------------------------------------------------------------------------------------------------------------------------
def test_set_unset_and_reuse_of_a_handle():
    """plain update, rule set at step count 12, rule off again: each leg equals handle B's, which replays the set leg by the loop."""
    t = _torch()
    pa, pb, oa, ob, args, kw, perm, n, bs = pair("small")
    rd = mixed_rule(args, kw, perm, bs, "small", 1, 3e-4)
    for o in (oa, ob):
        o.update(*args, perm, bs, learning_rate=1e-3, max_grad_norm=0.5, **kw)
    assert t.equal(pa.params, pb.params) and oa.state()[1] == 12
    lr = lr_word(3e-4)
    oa.set_kl_lr(rd, lr)
    sa = oa.update(*args, perm, bs, learning_rate=1e-3, max_grad_norm=0.5, **kw)
    lrs = loop_equals(oa, ob, pa, pb, args, kw, perm, n, bs, sa, 3e-4, rule_of(rd), lr)
    assert oa.state()[1] == 24 and len(set(lrs.tolist())) > 1
    # a second update under the rule starts from the rate the first one left
    left = lr.clone()
    sa = oa.update(*args, perm, bs, learning_rate=1e-3, max_grad_norm=0.5, **kw)
    loop_equals(oa, ob, pa, pb, args, kw, perm, n, bs, sa, float(left), rule_of(rd), lr)
    oa.set_kl_lr(None, None)
    left = lr.clone()
    sa = oa.update(*args, perm, bs, learning_rate=2e-3, max_grad_norm=0.5, **kw)
    sb = ob.update(*args, perm, bs, learning_rate=2e-3, max_grad_norm=0.5, **kw)
    assert t.equal(sa, sb) and t.equal(pa.params, pb.params) and t.equal(lr, left) and oa.state()[1] == ob.state()[1] == 48
    close_all(oa, ob, pa, pb)


# 6 -------------------------------------------------------------------------------------------------------------------------------------
LSTM_T, LSTM_B, LSTM_EPB = 4, 6, 4                                        # minibatches of 4 and 2 envs


def lstm_spec(shared):
    return dict(n_in=7, H=40, n_out=2, hidden_pi=(16,), hidden_vf=(16,), shared=shared, activation="tanh")


@functools.lru_cache(maxsize=None)
def lstm_case(shared, seed=0, B=LSTM_B):
    """(flat parameters of rl_helpers.lstm_members' small policy, a random rollout [T, B] on them, E permutations of the envs)"""
    p = lstm_members(1, shared=shared, seed0=3 + seed)[0]
    flat = p.params.detach().cpu().numpy().copy()
    p.close()
    roll = tw.random_rollout(lstm_spec(shared), flat, LSTM_T, B, seed=5 + seed)
    perms = np.stack([np.random.default_rng(100 + 10 * seed + e).permutation(B) for e in range(E)]).astype(np.int32)
    return flat, roll, perms


def lstm_handle(shared, seed=0):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    p = lstm_members(1, shared=shared, seed0=3 + seed)[0]
    return p, RecurrentPPOOptimizer(p, LSTM_T, LSTM_EPB)


@pytest.mark.parametrize("regime", ["down", "up"])
@pytest.mark.parametrize("shared", [False, True], ids=["two-lstms", "shared-lstm"])
def test_recurrent_update_equals_the_documented_loop(shared, regime):
    t = _torch()
    flat, roll, perms = lstm_case(shared)
    (pa, oa), (pb, ob) = lstm_handle(shared), lstm_handle(shared)
    assert np.array_equal(pa.params.cpu().numpy(), flat) and t.equal(pa.params, pb.params)
    d = dict(zip(roll, dev(*roll.values())))
    perm = dev(perms)[0]
    # 6 minibatches, 5 steps: 1e-2 / 1.5^5 = 1.3e-3 reaches lr_min = 2e-3; 1e-5 * 1.5^5 = 7.6e-5 reaches lr_max = 5e-5
    rd, lr0 = (dict(DOWN[0], lr_min=2e-3), DOWN[1]) if regime == "down" else (dict(UP[0], lr_max=5e-5), UP[1])
    rule, lr = rule_of(rd), lr_word(lr0)
    oa.set_kl_lr(rd, lr)
    sa = oa.update(d, perm, LSTM_EPB, learning_rate=7.0, max_grad_norm=0.5, **KW)
    n_mb = 2
    assert tuple(sa.shape) == (E, n_mb, 8)
    lrs = replay(lr0, sa[..., 3].cpu().numpy(), rule)
    for e in range(E):
        for k in range(n_mb):
            envs = perm[e, k * LSTM_EPB:min(LSTM_B, (k + 1) * LSTM_EPB)].contiguous()
            g, st = ob.grad(d, envs, **KW)
            assert t.equal(st, sa[e, k]), (e, k)
            ob.apply(g, learning_rate=float(lrs[e * n_mb + k]), max_grad_norm=0.5)
    print(shared, regime, "approx_kl", sa[..., 3].cpu().numpy().reshape(-1), "lr", lrs)
    assert t.equal(pa.params, pb.params) and bits(lr.cpu().numpy())[0] == bits(lrs[-1])
    (ma, na), (mb, nb) = oa.state(), ob.state()
    assert na == nb == 6 and np.array_equal(ma, mb)
    assert lrs[-1] == (rule[4] if regime == "down" else rule[5]) and lrs[1] != lrs[0]
    close_all(oa, ob, pa, pb)


# 7 -------------------------------------------------------------------------------------------------------------------------------------
# member id -> (rule, starting rate): the rate falls, rises, sits at its lower clamp
POP_RULES = {0: (dict(desired_kl=1e-12, factor=1.5, lr_min=1e-5, lr_max=1e-2), 1e-3),
             1: (dict(desired_kl=1e3, factor=1.5, lr_min=1e-5, lr_max=1e-2), 1e-4),
             2: (dict(desired_kl=1e-12, factor=2.0, lr_min=3e-4, lr_max=1e-2), 3e-4)}
POP_T, POP_BM, POP_BS = 5, 8, 16                                          # 40 rows per member: minibatches of 16, 16, 8


@functools.lru_cache(maxsize=None)
def mlp_shard(i):
    _, sd = make(5, (8,), 2, seed=3 + 7 * i)
    rows = batch(sd, 5, 2, POP_T * POP_BM, "tanh", seed=20 + i)
    perms = np.stack([np.random.default_rng(50 + 10 * i + e).permutation(POP_T * POP_BM) for e in range(E)]).astype(np.int32)
    return rows, perms


def mlp_single(i):
    """wg_ppo_update of member i alone on its rows with its rule -> (params, Adam's moments, step, stats, rate)"""
    from windgym_amd.ppo import PPOOptimizer
    rows, perms = mlp_shard(i)
    p, _ = make(5, (8,), 2, seed=3 + 7 * i)
    o, lr = PPOOptimizer(p), lr_word(POP_RULES[i][1])
    o.set_kl_lr(POP_RULES[i][0], lr)
    st = o.update(*dev(*rows), dev(perms)[0], POP_BS, learning_rate=0.0, max_grad_norm=0.5, **KW)
    res = (p.params.clone(), *o.state(), st.clone(), lr.clone())
    close_all(o, p)
    return res


def mlp_pop(order, rules_on=None, stats=True):
    """wg_pop_update with the members ``order`` -> {id: the same tuple}; ``rules_on``: the ids whose rule is set (default: all)"""
    from windgym_amd.binding import CPpoBatch, CPpoHyper
    from windgym_amd.population import Population, global_rows
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    P, T, Bm = len(order), POP_T, POP_BM
    B = P * Bm
    pol = [make(5, (8,), 2, seed=3 + 7 * i)[0] for i in order]
    opts = [PPOOptimizer(p) for p in pol]
    lrs = t.tensor([float(F(POP_RULES[i][1])) for i in order], dtype=t.float32, device="cuda")
    for m, i in enumerate(order):
        if rules_on is None or i in rules_on:
            opts[m].set_kl_lr(POP_RULES[i][0], lrs[m:m + 1])
    pop = Population(pol, opts)
    parts = [dev(*mlp_shard(i)[0]) for i in order]
    cols = [t.stack([parts[m][j].view(T, Bm, -1) for m in range(P)], dim=1) for j in range(5)]      # [T, P, Bm, ..] = [T, B, ..]
    d = [c.reshape(T * B, -1).contiguous() for c in cols]
    perm = t.stack([global_rows(dev(mlp_shard(i)[1])[0].long(), m, B, Bm) for m, i in enumerate(order)]).to(t.int32).contiguous()
    b = CPpoBatch(*[x.data_ptr() for x in d], T * B)
    hp = (CPpoHyper * P)(*[CPpoHyper(KW["clip_range"], KW["vf_coef"], KW["ent_coef"], 1) for _ in order])
    f = lambda v: (C.c_float * P)(*[v] * P)                                # noqa: E731
    params = (C.c_void_p * P)(*[p.params.data_ptr() for p in pol])
    st = t.zeros((P, E, 3, 8), dtype=t.float32, device="cuda")
    before = [(p.params.clone(), o.state()[1]) for p, o in zip(pol, opts)]
    rc = pop.L.wg_pop_update(pop._h, params, C.byref(b), perm.data_ptr(), E, POP_BS, hp, f(0.0), f(0.5), st.data_ptr() if stats else None,
                             pop._stream())
    msg = pop.L.wg_last_error().decode()
    t.cuda.synchronize()
    res = {i: (pol[m].params.clone(), *opts[m].state(), st[m].clone(), lrs[m:m + 1].clone()) for m, i in enumerate(order)}
    unchanged = all(t.equal(p.params, w) and o.state()[1] == n for (w, n), p, o in zip(before, pol, opts))
    close_all(pop, opts, pol)
    return rc, msg, res, unchanged


def same(a, b, stats=True):
    t = _torch()
    return (t.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and (not stats or t.equal(a[3], b[3]))
            and np.array_equal(bits(a[4].cpu().numpy()), bits(b[4].cpu().numpy())))


def test_population_members_equal_the_single_updates():
    rc, msg, pop, _ = mlp_pop((0, 1, 2))
    assert rc == 0, msg
    singles = {i: mlp_single(i) for i in range(3)}
    for i in range(3):
        assert same(pop[i], singles[i]), i
        assert pop[i][2] == E * 3
    r = {i: float(singles[i][4]) for i in range(3)}
    print("rates", r, [POP_RULES[i][1] for i in range(3)])
    assert r[0] < float(F(1e-3)) and r[0] > float(F(1e-5)) and r[1] > float(F(1e-4)) and r[2] == float(F(3e-4))      # falls, rises, sits at lr_min
    # permuting the members permutes the results; neither P nor the others matter; without statistics the same
    rc, msg, other, _ = mlp_pop((2, 0, 1))
    assert rc == 0 and all(same(other[i], singles[i]) for i in range(3))
    rc, msg, two, _ = mlp_pop((1, 2), stats=False)
    assert rc == 0 and all(same(two[i], singles[i], stats=False) for i in (1, 2))


def test_population_with_the_rule_on_some_members_is_refused():
    for on, says in (((0, 2), "member 1 has no KL-adaptive rate set while member 0 has one"),
                     ((1,), "member 1 has a KL-adaptive rate set while member 0 has none")):
        rc, msg, _, unchanged = mlp_pop((0, 1, 2), rules_on=on)
        assert rc == -1 and msg.startswith("wg_pop_update: " + says) and unchanged, msg


def lstm_pop_run(shared, order, rules_on=None):
    from recurrent_population_twin import pop_update
    from windgym_amd.recurrent_population import RecurrentPopulation, global_envs
    t = _torch()
    P = len(order)
    hs = [lstm_handle(shared, seed=i) for i in order]
    ps, opts = [h[0] for h in hs], [h[1] for h in hs]
    lrs = t.tensor([float(F(POP_RULES[i][1])) for i in order], dtype=t.float32, device="cuda")
    for m, i in enumerate(order):
        if rules_on is None or i in rules_on:
            opts[m].set_kl_lr(POP_RULES[i][0], lrs[m:m + 1])
    pop = RecurrentPopulation(ps, opts)
    rolls = [lstm_case(shared, seed=i)[1] for i in order]
    roll = {k: np.concatenate([r[k] for r in rolls], axis=1) for k in COLUMNS}
    roll["lstm_state0"] = np.stack([r["lstm_state0"] for r in rolls])
    perm = np.stack([global_envs(lstm_case(shared, seed=i)[2], m, LSTM_B) for m, i in enumerate(order)]).astype(np.int32)
    d = dict(zip(roll, dev(*roll.values())))
    hy = dict(clip_range=[0.2] * P, vf_coef=[0.5] * P, ent_coef=[0.01] * P, normalize_advantage=[True] * P, learning_rate=[0.0] * P,
              max_grad_norm=[0.5] * P)
    before = [(p.params.clone(), o.state()[1]) for p, o in zip(ps, opts)]
    err = None
    try:
        st = pop_update(pop, d, dev(perm)[0], LSTM_EPB, hy)
    except ValueError as e:
        err, st = str(e), t.zeros((P, E, 2, 8), device="cuda")
    res = {i: (ps[m].params.clone(), *opts[m].state(), st[m].clone(), lrs[m:m + 1].clone()) for m, i in enumerate(order)}
    unchanged = all(t.equal(p.params, w) and o.state()[1] == n for (w, n), p, o in zip(before, ps, opts))
    close_all(pop, opts, ps)
    return err, res, unchanged


@pytest.mark.parametrize("shared", [False, True], ids=["two-lstms", "shared-lstm"])
def test_recurrent_population_members_equal_the_single_updates(shared):
    err, pop, _ = lstm_pop_run(shared, (0, 1, 2))
    assert err is None
    singles = {}
    for i in range(3):
        flat, roll, perms = lstm_case(shared, seed=i)
        p, o = lstm_handle(shared, seed=i)
        lr = lr_word(POP_RULES[i][1])
        o.set_kl_lr(POP_RULES[i][0], lr)
        st = o.update(dict(zip(roll, dev(*roll.values()))), dev(perms)[0], LSTM_EPB, learning_rate=0.0, max_grad_norm=0.5, **KW)
        singles[i] = (p.params.clone(), *o.state(), st.clone(), lr.clone())
        close_all(o, p)
        assert same(pop[i], singles[i]), i
    r = {i: float(singles[i][4]) for i in range(3)}
    assert float(F(1e-5)) < r[0] < float(F(1e-3)) and r[1] > float(F(1e-4)) and r[2] == float(F(3e-4))
    err, other, _ = lstm_pop_run(shared, (1, 2, 0))
    assert err is None and all(same(other[i], singles[i]) for i in range(3))
    err, _, unchanged = lstm_pop_run(shared, (0, 1, 2), rules_on=(0, 1))
    assert err.startswith("wg_lstm_pop_update: member 2 has no KL-adaptive rate set while member 0 has one") and unchanged


# 8 -------------------------------------------------------------------------------------------------------------------------------------
ADAPT = dict(desired_kl=1e-4, factor=1.5, lr_min=1e-5, lr_max=1e-2)


def learn_and_watch(trainer, n_iter, steps, reset=True):
    """learn() for n_iter iterations; per iteration: the rate on the device afterwards == the log's, and == the replay of the
    iteration's own approx_kl from the rate the iteration before left (the next iteration starts from it).  -> the rates"""
    rule, seen = rule_of(trainer.adaptive_lr), [F(float(trainer.lr))]

    def watch(p):
        now = F(float(p.lr))
        assert bits(p.log[-1]["learning_rate"]) == bits(now)
        assert bits(replay(seen[-1], p._stats[..., 3].cpu().numpy(), rule)[-1]) == bits(now)
        seen.append(now)
    trainer.learn(n_iter * steps, callback=watch, reset_num_timesteps=reset)
    assert len(seen) == n_iter + 1
    return seen


@pytest.mark.parametrize("which", ["ppo", "recurrent"])
def test_learn_save_load_continue(which, tmp_path):
    from windgym_amd.ppo import PPO, read_checkpoint
    from windgym_amd.recurrent_ppo import RecurrentPPO
    t = _torch()
    T = 16
    if which == "ppo":
        mk = lambda v: PPO("MlpPolicy", v, n_steps=T, n_epochs=2, seed=11, learning_rate=3e-4, adaptive_lr=ADAPT)          # noqa: E731
        cls = PPO
    else:
        mk = lambda v: RecurrentPPO("MlpLstmPolicy", v, n_steps=T, n_epochs=2, seed=11, learning_rate=3e-4, adaptive_lr=ADAPT,      # noqa: E731
                                    policy_kwargs=dict(lstm_hidden_size=32, net_arch=dict(pi=[16], vf=[16])))
        cls = RecurrentPPO
    va, vb = _venv(64), _venv(64)
    a = mk(va)
    assert tuple(a.lr.shape) == (1,) and a.lr.dtype == t.float32 and a.lr.is_cuda
    ra = learn_and_watch(a, 3, T * 64)
    assert len(set(float(x) for x in ra)) > 1                              # the rate moved
    b = mk(vb)
    rb = learn_and_watch(b, 2, T * 64)
    assert np.array_equal(bits(rb), bits(ra[:3]))
    path = os.path.join(tmp_path, "a.zip")
    b.save(path)
    meta, members = read_checkpoint(path)
    assert meta["adaptive_lr"] == b.adaptive_lr and bits(members["learning_rate.npy"])[0] == bits(rb[-1])
    assert meta["hyper"]["learning_rate"] == 3e-4
    c = cls.load(path, vb)
    assert c.adaptive_lr == b.adaptive_lr and t.equal(c.lr, b.lr)
    b.close(); b.policy.close()
    rc = learn_and_watch(c, 1, T * 64, reset=False)
    assert c.iteration == 3 and t.equal(c.policy.params, a.policy.params) and t.equal(c.lr, a.lr) and bits(rc[-1]) == bits(ra[-1])
    (ma, sa), (mc, sc) = a.opt.state(), c.opt.state()
    assert sa == sc and np.array_equal(ma, mc)
    # log_interval=None: no record is made, and the rate still follows the iteration's own approx_kl on the device
    before = F(float(a.lr))
    a.learn(T * 64, log_interval=None, reset_num_timesteps=False)
    assert len(a.log) == 3 and a.iteration == 4
    assert bits(float(a.lr)) == bits(replay(before, a._stats[..., 3].cpu().numpy(), rule_of(a.adaptive_lr))[-1])
    for x in (a, c):
        x.close(); x.policy.close()
    va.close(); vb.close()


def test_population_learns_as_its_members_alone(tmp_path):
    """PPOPopulation of 2 members with rules of their own == PPO with the member's rule on the member's shard: parameters, rate, log.
    The population has no load(): a member resumes alone, so save -> load -> continue is 2 iterations of the population, save(),
    one more — against PPO on the shard for 2 iterations, PPO.load(the member's zip) on that shard, one more."""
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.population import PPOPopulation
    from windgym_amd.ppo import PPO, read_checkpoint
    from windgym_amd.turbine import V80
    t = _torch()
    P, B, T = 2, 64, 16
    va = _venv(B)
    ad = dict(desired_kl=[1e-7, 1e3], lr_max=[1e-2, 1e-3])
    pp = PPOPopulation("MlpPolicy", va, n_members=P, n_steps=T, n_epochs=2, seed=[5, 6], learning_rate=[3e-4, 1e-4], adaptive_lr=ad)
    assert tuple(pp.lr.shape) == (P,)
    pp.learn(2 * T * B // P)
    paths = pp.save(os.path.join(tmp_path, "pop"))
    at2 = [(p.params.clone(), pp.lr[m:m + 1].clone()) for m, p in enumerate(pp.members)]
    pp.learn(T * B // P, reset_num_timesteps=False)
    assert pp.iteration == 3 and len(pp.log) == 3
    assert [bits(r["learning_rate"]) for r in pp.log[-1]] == [bits(x) for x in pp.lr.cpu().numpy()]
    assert float(pp.lr[0]) < float(F(3e-4)) and float(pp.lr[1]) > float(F(1e-4))
    for m in range(P):
        vs = WindFarmVecEnv(V80(), B // P, yaml_dict=presets.bench_cfg2_config(), seed=77, as_torch=True, turbtype="None", n_passthrough=1,
                            n_rotor_pts=16).shard(m, P)
        vs.reset(seed=77)
        ppo = PPO("MlpPolicy", vs, seed=5 + m, adaptive_lr=pp.adaptive_lr[m], **pp.member_hyper(m))
        ppo.learn(2 * T * B // P)
        assert t.equal(ppo.policy.params, at2[m][0]) and t.equal(ppo.lr, at2[m][1]), m
        meta, members = read_checkpoint(paths[m])
        assert meta["adaptive_lr"] == pp.adaptive_lr[m] and bits(members["learning_rate.npy"])[0] == bits(float(at2[m][1]))
        c = PPO.load(paths[m], vs)
        assert c.adaptive_lr == pp.adaptive_lr[m] and t.equal(c.lr, at2[m][1]) and t.equal(c.policy.params, at2[m][0])
        ppo.close(); ppo.policy.close()
        c.learn(T * B // P, reset_num_timesteps=False)
        assert c.iteration == 3 and t.equal(c.policy.params, pp.members[m].params) and t.equal(c.lr, pp.lr[m:m + 1]), m
        assert [bits(r["learning_rate"]) for r in c.log] == [bits(recs[m]["learning_rate"]) for recs in pp.log]
        (mc, sc), (mp, sp) = c.opt.state(), pp.opts[m].state()
        assert sc == sp and np.array_equal(mc, mp)
        c.close(); close_all(c.policy, vs)
    pp.close(); close_all(pp.members, va)


# 9 -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_abi():
    from windgym_amd.binding import CKlLr
    t = _torch()
    pa, pb, oa, ob, args, kw, perm, n, bs = pair("small")
    pl, ol = lstm_handle(False)
    good = CKlLr(0.01, 1.5, 1e-5, 1e-2)
    lr = lr_word(3e-4)
    host = np.array([3e-4], F)
    for o, fn, who in ((oa, oa.L.wg_ppo_set_kl_lr, "wg_ppo_set_kl_lr"), (ol, ol.L.wg_lstm_ppo_set_kl_lr, "wg_lstm_ppo_set_kl_lr")):
        def refused(rule, ptr, says):
            rc = fn(o._h, None if rule is None else C.byref(rule), ptr)
            msg = o.L.wg_last_error().decode()
            assert rc == -1 and msg.startswith(who + ": " + says), msg
        refused(good, None, "lr_dev is null")
        refused(None, lr.data_ptr(), "rule is null")
        refused(good, host.ctypes.data, "lr_dev is not")                   # host memory: not a device pointer / not memory of the device
        for bad, says in ((CKlLr(0.0, 1.5, 1e-5, 1e-2), "desired_kl must be > 0"), (CKlLr(float("nan"), 1.5, 1e-5, 1e-2), "desired_kl must be > 0"),
                          (CKlLr(float("inf"), 1.5, 1e-5, 1e-2), "desired_kl must be > 0 and finite"), (CKlLr(0.01, 0.5, 1e-5, 1e-2), "factor must be >= 1"),
                          (CKlLr(0.01, float("inf"), 1e-5, 1e-2), "factor must be >= 1 and finite"), (CKlLr(0.01, 1.5, 0.0, 1e-2), "lr_min must be > 0"),
                          (CKlLr(0.01, 1.5, 1e-2, 1e-3), "lr_min must be <= lr_max"), (CKlLr(0.01, 1.5, 1e-3, 1e-2), "the starting rate *lr_dev = 0.0003 lies outside"),
                          (CKlLr(0.01, 1.5, 1e-5, 1e-4), "the starting rate *lr_dev = 0.0003 lies outside")):
            refused(bad, lr.data_ptr(), says)
        assert fn(None, C.byref(good), lr.data_ptr()) == -1
    if t.cuda.device_count() > 1:
        far = t.full((1,), 3e-4, dtype=t.float32, device="cuda:1")
        assert oa.L.wg_ppo_set_kl_lr(oa._h, C.byref(good), far.data_ptr()) == -1
        assert "lr_dev is not memory of device 0" in oa.L.wg_last_error().decode()
    # nothing above set a rule: the handle still takes its own learning_rate
    sa = oa.update(*args, perm, bs, learning_rate=1e-3, max_grad_norm=0.5, **kw)
    sb = ob.update(*args, perm, bs, learning_rate=1e-3, max_grad_norm=0.5, **kw)
    assert t.equal(sa, sb) and t.equal(pa.params, pb.params)
    # the wrapper: one float32 CUDA element
    with pytest.raises(ValueError, match="lr must be a contiguous float32 CUDA tensor of one element"):
        oa.set_kl_lr(dict(desired_kl=0.01, factor=1.5, lr_min=1e-5, lr_max=1e-2), t.zeros(2, device="cuda"))
    close_all(oa, ob, pa, pb, ol, pl)
