"""GPU tests of the recurrent trainer: the BPTT kernels of windgym_amd/csrc/wg_lstm_ppo.hip through the wg_lstm_ppo_* entries
(RecurrentPPOOptimizer) against the float64 twin tests/lstm_bptt_twin.py, and RecurrentPPO end to end.

THE BAR of the gradient and of the trained parameters follows the project's two precedents.  ``e32`` is the error, against the twin, of
the SAME computation by torch in float32 on the CPU — from the reference side only.  The device's worst absolute gradient error must
be at most ``max(4 e32, 1e-4 |ref|_2 + 1e-6)`` (the second term is test_gpu_ppo.py's own bar); the trained parameters' at most
``4 e32 + 1e-6``.  Each case prints its device error next to e32 and the bar (profiles/r21_lstm_ppo_errors.txt keeps a run's lines)."""
import os

import numpy as np
import pytest

import lstm_bptt_twin as tw
from recurrent_ppo_cases import make_spec
from rl_helpers import _torch, _venv, dev, dev_roll, lstm_policy

pytestmark = pytest.mark.gpu

KW = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)


def _long_starts(T, B):
    """Episode starts at t = 0 for some rows, mid-sequence, on two consecutive steps and on the last step."""
    s = np.zeros((T + 1, B), np.uint8)
    s[0, ::3] = 1
    s[T // 2, 1::4] = 1
    s[10, 2::5] = 1
    s[11, 2::5] = 1
    s[T - 1, ::2] = 1
    return s


CASES = [(3, 1, 1, 1, False), (8, 32, 5, 33, False), (7, 40, 9, 31, False), (7, 40, 9, 31, True), (257, 64, 4, 33, False),
         (20, 256, 3, 32, False), (2048, 256, 2, 2, False), (8, 64, 64, 33, False)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_grad_vs_twin(case):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    n_in, H, T, Bm, shared = case
    spec = make_spec(n_in, H, shared)
    extra = 5
    B = Bm + extra
    flat = tw.random_params(spec, seed=Bm + T)
    roll = tw.random_rollout(spec, flat, T, B, seed=H + T, starts=_long_starts(T, B) if T == 64 else None)
    envs = np.random.default_rng(n_in).permutation(B)[:Bm].astype(np.int32)
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, T, Bm)
    g, st = opt.grad(dev_roll(roll), dev(envs)[0], **KW)
    g, st = g.cpu().numpy().astype(np.float64), st.cpu().numpy()
    _, rs, ref, ratio = tw.loss_and_grad(spec, flat, roll, envs, **KW)
    d32 = np.abs(tw.loss_and_grad(spec, flat, roll, envs, dtype=t.float32, **KW)[2] - ref)
    e32 = d32.max()
    err, bar = np.abs(g - ref).max(), max(4.0 * e32, 1e-4 * np.linalg.norm(ref) + 1e-6)
    # the LSTM tensors on their own, so that the MLP's larger entries do not hide them: the same two terms on that block, without the
    # absolute 1e-6 (the block's entries can be smaller than that)
    n_lstm = (1 if shared else 2) * 4 * H * (n_in + H + 2)
    err_l, bar_l = np.abs(g - ref)[:n_lstm].max(), max(4.0 * d32[:n_lstm].max(), 1e-4 * np.linalg.norm(ref[:n_lstm]))
    print(f"r21 grad case={case} rows={T * Bm} device_err={err:.3e} e32={e32:.3e} bar={bar:.3e} ref_norm={np.linalg.norm(ref):.3e} | "
          f"lstm block: device_err={err_l:.3e} e32={d32[:n_lstm].max():.3e} bar={bar_l:.3e} ref_norm={np.linalg.norm(ref[:n_lstm]):.3e}")
    n = T * Bm
    if n >= 128:
        assert (ratio > 1.2).any() and (ratio < 0.8).any()               # both clip sides are exercised
    if T == 64:
        es = roll["episode_start"][:T, envs]
        assert es[0].any() and not es[0].all() and es[T // 2].any() and (es[10] & es[11]).any() and es[T - 1].any()
        assert np.abs(roll["lstm_state0"][:, :, envs[es[0] == 0]]).min() > 0
    assert np.all(np.isfinite(g)) and np.abs(ref[:n_lstm]).max() > 0
    assert err <= bar, (err, e32, bar)
    assert err_l <= bar_l, (err_l, bar_l)
    for i, k in enumerate(tw.STATS):
        tol = 2.0 / n if k == "clip_fraction" else 1e-5 * max(1.0, abs(rs[k]))
        assert abs(st[i] - rs[k]) <= tol, (k, st[i], rs[k])
    opt.close(); p.close()


def _small(shared=False, T=6, B=40, H=40, n_in=7, seed=0, **kw):
    spec = make_spec(n_in, H, shared)
    flat = tw.random_params(spec, seed=seed)
    return spec, flat, tw.random_rollout(spec, flat, T, B, seed=seed + 1, **kw)


def test_fresh_rows_never_read_their_state():
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    spec, flat, roll = _small(T=5, B=37)
    fresh = roll["episode_start"][0] != 0
    assert fresh.any() and not fresh.all()
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, 5, 37)
    envs = dev(np.random.default_rng(1).permutation(37).astype(np.int32))[0]
    roll["lstm_state0"][:, :, fresh] = 0.0
    g0, s0 = (x.clone() for x in opt.grad(dev_roll(roll), envs, **KW))
    roll["lstm_state0"][:, :, fresh] = np.nan
    g1, s1 = opt.grad(dev_roll(roll), envs, **KW)
    assert bool(t.isfinite(g1).all()) and t.equal(g0, g1) and t.equal(s0, s1)
    opt.close(); p.close()


def test_deterministic_and_independent_of_other_envs():
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    spec, flat, roll = _small(shared=True)
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, 6, 33)
    perm = np.random.default_rng(2).permutation(40)
    inside, outside = perm[:33], perm[33:]
    envs = dev(inside.astype(np.int32))[0]
    g0, s0 = (x.clone() for x in opt.grad(dev_roll(roll), envs, **KW))
    g1, s1 = opt.grad(dev_roll(roll), envs, **KW)
    assert t.equal(g0, g1) and t.equal(s0, s1) and float(g0.abs().max()) > 0
    rng = np.random.default_rng(3)
    for k in ("obs", "raw", "logp", "advantage", "returns"):
        roll[k][:, outside] = rng.uniform(-7, 7, roll[k][:, outside].shape).astype(np.float32)
    roll["lstm_state0"][:, :, outside] = 5.0
    roll["episode_start"][:, outside] ^= 1
    g2, s2 = opt.grad(dev_roll(roll), envs, **KW)
    assert t.equal(g0, g2) and t.equal(s0, s2)
    opt.close(); p.close()


def _update_and_loop(shared, n_epochs=2, B=40, Bm=16, T=6, lr=3e-4):
    """-> (spec, flat, roll, perms, policy after wg_lstm_ppo_update, its optimiser, stats, policy after the documented loop, its optimiser, stats)"""
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    spec, flat, roll = _small(shared=shared, T=T, B=B, seed=4)
    perms = np.stack([np.random.default_rng(10 + e).permutation(B) for e in range(n_epochs)]).astype(np.int32)
    d, perm = dev_roll(roll), dev(perms)[0]
    kw = {k: v for k, v in KW.items()}
    pa, pb = lstm_policy(spec, flat), lstm_policy(spec, flat)
    oa, ob = RecurrentPPOOptimizer(pa, T, Bm), RecurrentPPOOptimizer(pb, T, Bm)
    sa = oa.update(d, perm, Bm, learning_rate=lr, max_grad_norm=0.5, **kw)
    n_mb = -(-B // Bm)
    sb = t.zeros((n_epochs, n_mb, 8), dtype=t.float32, device="cuda")
    for e in range(n_epochs):
        for k in range(n_mb):
            g, _ = ob.grad(d, perm[e, k * Bm:(k + 1) * Bm], stats=sb[e, k], **kw)
            ob.apply(g, learning_rate=lr, max_grad_norm=0.5)
    return spec, flat, roll, perms, pa, oa, sa, pb, ob, sb


def test_update_equals_its_documented_loop():
    t = _torch()
    *_, pa, oa, sa, pb, ob, sb = _update_and_loop(False)
    assert sa.shape == (2, 3, 8) and t.equal(sa, sb) and t.equal(pa.params, pb.params)
    (ma, na), (mb, nb) = oa.state(), ob.state()
    assert na == nb == 6 and np.array_equal(ma, mb) and np.abs(ma).max() > 0
    for x in (oa, ob, pa, pb):
        x.close()


@pytest.mark.parametrize("shared", [False, True], ids=["two-lstms", "shared-lstm"])
def test_adam_state_moves_between_handles(shared):
    """Adam's state through wg_lstm_ppo_get_state / _set_state / _apply: k applies count k steps, and a second handle given that state
    and the same parameters takes the next step to the same bits."""
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    T, Bm, k = 3, 5, 3
    spec, flat, roll = _small(shared=shared, T=T, B=Bm, H=40, n_in=7, seed=6)
    d, envs = dev_roll(roll), dev(np.arange(Bm, dtype=np.int32))[0]
    pa, pb = lstm_policy(spec, flat), lstm_policy(spec, flat)
    oa, ob = RecurrentPPOOptimizer(pa, T, Bm), RecurrentPPOOptimizer(pb, T, Bm)
    n = pa.params.numel()
    mv0, step0 = oa.state()
    assert step0 == 0 and mv0.shape == (2 * n,) and not mv0.any()
    for _ in range(k):
        oa.grad(d, envs, **KW)
        oa.apply(learning_rate=1e-2, max_grad_norm=0.5)
    mv, step = oa.state()
    assert step == k and np.all(np.isfinite(mv)) and np.abs(mv[:n]).max() > 0 and mv[n:].min() >= 0 and mv[n:].max() > 0
    assert float((pa.params - t.from_numpy(np.asarray(flat, np.float32)).cuda()).abs().max()) > 1e-3
    ob.load_state(mv, step)
    with t.no_grad():
        pb.params.copy_(pa.params)
    pb.sync()
    g = oa.grad(d, envs, **KW)[0].clone()
    oa.apply(g, learning_rate=1e-2, max_grad_norm=0.5)
    ob.apply(g, learning_rate=1e-2, max_grad_norm=0.5)
    (ma, na), (mb, nb) = oa.state(), ob.state()
    assert na == nb == k + 1 and np.array_equal(ma.view(np.uint32), mb.view(np.uint32)) and not np.array_equal(ma, mv)
    assert t.equal(pa.params, pb.params)
    with pytest.raises(ValueError, match=f"wg_lstm_ppo_set_state: the state has {2 * n} floats"):
        ob.load_state(mv[:-1], step)
    for x in (oa, ob, pa, pb):
        x.close()


def test_update_vs_reference_trainer():
    t = _torch()
    spec, flat, roll, perms, pa, oa, sa, pb, ob, _ = _update_and_loop(False)
    ref, log = tw.train(spec, flat, roll, perms, 16, lr=3e-4, max_grad_norm=0.5, **KW)
    f32, _ = tw.train(spec, flat, roll, perms, 16, lr=3e-4, max_grad_norm=0.5, dtype=t.float32, **KW)
    e32 = np.abs(f32 - ref).max()
    err = np.abs(pa.params.cpu().numpy().astype(np.float64) - ref).max()
    moved = np.abs(ref - flat).max()
    print(f"r21 train device_err={err:.3e} e32={e32:.3e} bar={4 * e32 + 1e-6:.3e} moved={moved:.3e}")
    assert moved > 1e-4 and err <= 4.0 * e32 + 1e-6, (err, e32)
    got = sa.cpu().numpy().reshape(-1, 8)
    for i, k in enumerate(tw.STATS):
        if k != "clip_fraction":
            assert np.allclose(got[:, i], [s[k] for s in log], rtol=1e-4, atol=1e-4), k
    for x in (oa, ob, pa, pb):
        x.close()


def test_recurrent_ppo_end_to_end(tmp_path):
    from windgym_amd.binding import PPO_STATS
    from windgym_amd.recurrent import MlpLstmPolicy
    from windgym_amd.recurrent_ppo import RecurrentPPO
    t = _torch()
    T, B = 8, 8
    kw = dict(n_steps=T, n_epochs=2, ent_coef=0.001, seed=5, policy_kwargs=dict(lstm_hidden_size=32, net_arch=dict(pi=[16], vf=[16])))
    va = _venv(B)
    a = RecurrentPPO("MlpLstmPolicy", va, **kw)
    assert a.envs_per_batch == 2 and a.batch_size == 2 * T
    w0 = a.policy.params.clone()
    seen = []

    def cb(ppo):
        out = list(ppo.venv._lstm.values())[0][3][T]
        seen.append((out["lstm_state0"].clone(), out["lstm_state"].clone(), out["episode_start"].clone()))
    a.learn(2 * T * B, callback=cb)
    assert a.num_timesteps == 2 * T * B and a.iteration == 2 and len(a.log) == 2
    keys = set(PPO_STATS) | {"explained_variance", "iteration", "num_timesteps", "learning_rate", "clip_range", "n_episodes",
                             "mean_episode_return", "mean_episode_power", "mean_step_reward", "fps"}
    for rec in a.log:
        assert set(rec) == keys and all(np.isfinite(float(x)) for x in rec.values()), rec
    assert not t.equal(a.policy.params, w0) and bool(t.isfinite(a.policy.params).all())
    # iteration 2's rollout began from iteration 1's final LSTM state, with no env marked fresh unless it was truncated
    assert t.equal(seen[1][0], seen[0][1]) and float(seen[0][1].abs().max()) > 0 and bool(seen[0][2][0].all())
    va.batch.check()
    # 1 iteration, save, load on the same env, 1 more
    vb = _venv(B)
    b = RecurrentPPO("MlpLstmPolicy", vb, **kw)
    b.learn(T * B)
    path = os.path.join(tmp_path, "rppo.zip")
    b.save(path)
    q = MlpLstmPolicy.from_sb3_zip(path)
    assert q.desc == b.policy.desc and t.equal(q.params, b.policy.params)
    q.close()
    c = RecurrentPPO.load(path, vb)
    b.close(); b.policy.close()
    c.learn(T * B, reset_num_timesteps=False)
    assert c.num_timesteps == a.num_timesteps and c.iteration == 2
    assert t.equal(c.policy.params, a.policy.params)
    (ma, sa), (mc, sc) = a.opt.state(), c.opt.state()
    assert sa == sc == 2 * 2 * 4 and np.array_equal(ma, mc)
    s, h = c.predict(np.zeros(va.batch.obs_dim, np.float32), deterministic=True)
    assert s.shape == (va.n_turb,) and h[0].shape == (1, 1, 32)
    for x in (a, c):
        x.close(); x.policy.close()
    va.close(); vb.close()


def test_recurrent_ppo_shared_lstm_matches_the_loop():
    from windgym_amd.recurrent_ppo import RecurrentPPO, RecurrentPPOOptimizer
    t = _torch()
    T, B = 8, 8
    kw = dict(n_steps=T, n_epochs=2, seed=6, policy_kwargs=dict(lstm_hidden_size=32, net_arch=[16], shared_lstm=True))
    va, vb = _venv(B), _venv(B)
    a, b = RecurrentPPO("MlpLstmPolicy", va, **kw), RecurrentPPO("MlpLstmPolicy", vb, **kw)
    assert a.policy.nets == 1 and t.equal(a.policy.params, b.policy.params)
    w0 = a.policy.params.clone()
    a.learn(T * B)
    out = b.collect()
    for e in range(b.n_epochs):
        b._perm[e].copy_(t.randperm(B, generator=b._gen, device="cuda"))
    for e in range(b.n_epochs):
        for k in range(4):
            g, _ = b.opt.grad(out, b._perm[e, 2 * k:2 * k + 2], clip_range=0.2, vf_coef=b.vf_coef, ent_coef=b.ent_coef)
            b.opt.apply(g, learning_rate=3e-4, max_grad_norm=b.max_grad_norm)
    assert t.equal(a.policy.params, b.policy.params) and not t.equal(a.policy.params, w0)
    for x in (a, b):
        x.close(); x.policy.close()
    va.close(); vb.close()


def test_refusals():
    from windgym_amd.policy import MlpPolicy
    from windgym_amd.recurrent_ppo import RecurrentPPO, RecurrentPPOOptimizer
    t = _torch()
    v = _venv(8)
    O, N = v.batch.obs_dim, v.n_turb
    mlp = MlpPolicy(O, N, (16,), (16,))
    with pytest.raises(ValueError, match="PPO trains an MlpPolicy"):
        RecurrentPPO(mlp, v)
    with pytest.raises(ValueError, match="only 'MlpLstmPolicy'"):
        RecurrentPPO("MlpPolicy", v)
    for k, val in (("target_kl", 0.01), ("clip_range_vf", 0.2), ("use_sde", True)):
        with pytest.raises(NotImplementedError, match=k):
            RecurrentPPO("MlpLstmPolicy", v, **{k: val})
    with pytest.raises(ValueError, match="multiple of n_steps"):
        RecurrentPPO("MlpLstmPolicy", v, n_steps=8, batch_size=20)

    class Multi:
        possible_agents = ["a"]
    with pytest.raises(NotImplementedError, match="WindFarmVecEnvMulti"):
        RecurrentPPO("MlpLstmPolicy", Multi())
    # the ABI (binding._chk: WG_ERR_INVALID is a ValueError, WG_ERR_UNSUPPORTED a NotImplementedError)
    spec, flat, roll = _small(T=4, B=6, H=8)
    p = lstm_policy(spec, flat)
    with pytest.raises(ValueError, match="T_max and Bm_max must be >= 1"):
        RecurrentPPOOptimizer(p, 0, 4)
    with pytest.raises(NotImplementedError, match=r"T_max = 16777216 steps of Bm_max = 1024 envs"):
        RecurrentPPOOptimizer(p, 1 << 24, 1024)
    opt = RecurrentPPOOptimizer(p, 3, 4)
    d = dev_roll(roll)
    envs = dev(np.arange(6, dtype=np.int32))[0]
    with pytest.raises(NotImplementedError, match="T = 4 > the T_max = 3"):
        opt.grad(d, envs[:4], **KW)
    opt.close()
    opt = RecurrentPPOOptimizer(p, 4, 4)
    with pytest.raises(NotImplementedError, match="6 envs in a minibatch > the Bm_max = 4"):
        opt.grad(d, envs, **KW)
    with pytest.raises(ValueError, match="clip_range < 0"):
        opt.grad(d, envs[:4], clip_range=-1.0)
    with pytest.raises(ValueError, match="max_grad_norm must be > 0"):
        opt.apply(max_grad_norm=0.0)
    with pytest.raises(ValueError, match="the state has"):
        opt.load_state(np.zeros(3, np.float32), 0)
    with pytest.raises(ValueError, match="needs a recurrent policy"):
        RecurrentPPOOptimizer(mlp, 4, 4)
    opt.close(); p.close(); mlp.close(); v.close()
