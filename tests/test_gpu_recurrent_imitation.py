"""GPU tests of behaviour cloning into a recurrent policy: k_bc_grad_dh of wg_ppo.hip in front of the BPTT kernels of wg_lstm_ppo.hip,
through the wg_lstm_bc_* entries (RecurrentPPOOptimizer.bc_grad / bc_update) against the float64 twin tests/lstm_bc_twin.py, and
RecurrentBehaviorCloning end to end.

THE BAR is tests/test_gpu_recurrent_ppo.py's.  ``e32`` is the error, against the float64 twin, of the SAME computation by torch in
float32 on the CPU — from the reference side only.  The device's worst absolute gradient error must be at most ``max(4 e32, 1e-4
|ref|_2 + 1e-6)`` on the whole vector and the same two terms without the 1e-6 on the LSTM block alone; every statistic within ``1e-5
max(1, |ref|)``; the trained parameters within ``4 e32 + 1e-6``.  Each gradient case prints its device error next to e32 and the bar
(profiles/r31_recurrent_imitation_errors.txt keeps a run's lines)."""
import ctypes as C
import os

import numpy as np
import pytest

import imitation_twin as it
import lstm_bc_twin as bt
import lstm_bptt_twin as tw
import rl_helpers
from recurrent_ppo_cases import make_spec
from rl_helpers import _torch, _venv, dev, dev_roll, lstm_policy

pytestmark = pytest.mark.gpu

KW = dict(ent_coef=0.01, vf_coef=0.5)
PPO_KW = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)
COMBOS = [(loss, with_ret) for loss in ("mse", "nll") for with_ret in (True, False)]


def _long_starts(T, B):
    """test_gpu_recurrent_ppo.py's pattern: episode starts at t = 0 for some rows, mid-sequence, on two consecutive steps and on the
    last step."""
    s = np.zeros((T + 1, B), np.uint8)
    s[0, ::3] = 1
    s[T // 2, 1::4] = 1
    s[10, 2::5] = 1
    s[11, 2::5] = 1
    s[T - 1, ::2] = 1
    return s


def bc_roll(roll, with_ret):
    """a twin's rollout as the device tensors wg_lstm_bc_grad / _update take (the twin's own dict without returns: ``with_ret`` False)"""
    keys = ("obs", "labels", "episode_start", "lstm_state0") + (("returns",) if with_ret else ())
    return dict(zip(keys, dev(*[roll[k] for k in keys])))


def twin_roll(roll, with_ret):
    return roll if with_ret else dict(roll, returns=None)


def _slices(spec):
    """{tensor name: slice of the flat vector}"""
    out, o = {}, 0
    for name, shape in tw.layout(spec):
        n = int(np.prod(shape))
        out[name] = slice(o, o + n)
        o += n
    return out


def _entries(spec, pick):
    sl = _slices(spec)
    return np.concatenate([np.arange(s.start, s.stop) for k, s in sl.items() if pick(k)])


def _n_lstm(spec):
    return tw.nets(spec) * 4 * spec["H"] * (spec["n_in"] + spec["H"] + 2)


def _bits(x):
    return x.detach().cpu().numpy().view(np.int32)


def _bars(spec, flat, roll, envs, g, st, tag, **kw):
    """bar 1 of the module docstring on a device gradient ``g`` and statistics ``st`` (numpy); prints the figures, then asserts."""
    t = _torch()
    _, rs, ref = bt.loss_and_grad(spec, flat, roll, envs, **kw)
    d32 = np.abs(bt.loss_and_grad(spec, flat, roll, envs, dtype=t.float32, **kw)[2] - ref)
    nl = _n_lstm(spec)
    diff = np.abs(g - ref)
    err, e32, bar = diff.max(), d32.max(), max(4.0 * d32.max(), 1e-4 * np.linalg.norm(ref) + 1e-6)
    err_l, e32_l, bar_l = diff[:nl].max(), d32[:nl].max(), max(4.0 * d32[:nl].max(), 1e-4 * np.linalg.norm(ref[:nl]))
    print(f"r31 bc grad {tag} device_err={err:.3e} e32={e32:.3e} bar={bar:.3e} ref_norm={np.linalg.norm(ref):.3e} | "
          f"lstm block: device_err={err_l:.3e} e32={e32_l:.3e} bar={bar_l:.3e} ref_norm={np.linalg.norm(ref[:nl]):.3e}")
    assert np.all(np.isfinite(g)) and np.abs(ref[:nl]).max() > 0
    assert err <= bar, (tag, err, e32, bar)
    assert err_l <= bar_l, (tag, err_l, e32_l, bar_l)
    for i, k in enumerate(bt.STATS):
        assert abs(st[i] - rs[k]) <= 1e-5 * max(1.0, abs(rs[k])), (tag, k, st[i], rs[k])
    assert st[6] == 0.0 and st[7] == 0.0
    return ref


# ---- 1. the gradient against the twin -------------------------------------------------------------------------------------------------
CASES = [(3, 1, 1, 1, False), (8, 32, 5, 33, False), (7, 40, 9, 31, False), (7, 40, 9, 31, True), (20, 256, 3, 32, False),
         (8, 64, 64, 33, False)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_grad_vs_twin(case):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    n_in, H, T, Bm, shared = case
    spec = make_spec(n_in, H, shared)
    B = Bm + 5
    flat = tw.random_params(spec, seed=Bm + T)
    roll = bt.random_rollout(spec, flat, T, B, seed=H + T, starts=_long_starts(T, B) if T == 64 else None)
    envs = np.random.default_rng(n_in).permutation(B)[:Bm].astype(np.int32)
    if T == 64:
        es = roll["episode_start"][:T, envs]
        assert es[0].any() and not es[0].all() and es[T // 2].any() and (es[10] & es[11]).any() and es[T - 1].any()
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, T, Bm)
    d_envs = dev(envs)[0]
    for loss, with_ret in COMBOS:
        g, st = opt.bc_grad(bc_roll(roll, with_ret), d_envs, loss=loss, **KW)
        _bars(spec, flat, twin_roll(roll, with_ret), envs, g.cpu().numpy().astype(np.float64), st.cpu().numpy(),
              f"case={case} loss={loss} returns={with_ret} rows={T * Bm}", loss=loss, **KW)
    opt.close(); p.close()


# ---- 2. exact zeros on a used handle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["two-lstms", "shared-lstm"])
def test_exact_zeros_after_a_ppo_gradient_on_the_same_handle(shared):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    n_in, H, T, B, Bm = 7, 40, 6, 40, 33
    spec = make_spec(n_in, H, shared)
    flat = tw.random_params(spec, seed=3)
    other = tw.random_rollout(spec, flat, T, B, seed=21)
    roll = bt.random_rollout(spec, flat, T, B, seed=22)
    perm = np.random.default_rng(5).permutation(B).astype(np.int32)
    envs, envs_other = perm[:Bm], perm[::-1][:Bm].copy()
    critic_mlp = _entries(spec, lambda k: "value_net" in k)
    critic_lstm = _entries(spec, lambda k: k.startswith("lstm_critic")) if not shared else np.zeros(0, np.int64)
    actor_lstm = _entries(spec, lambda k: k.startswith("lstm_actor"))
    log_std = _entries(spec, lambda k: k == "log_std")
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, T, Bm)
    d_other, d_roll = dev_roll(other), bc_roll(roll, False)
    for loss in ("mse", "nll"):
        # the heads' partials and statistics slots, dh[1], the critic net's stash and its columns of the weight gradient's partial sums,
        # and the gradient buffer all hold another batch's PPO values
        g0 = opt.grad(d_other, dev(envs_other)[0], **PPO_KW)[0].cpu().numpy()
        assert g0[critic_mlp].all() and g0[log_std].all() and (shared or g0[critic_lstm].all())
        g, st = opt.bc_grad(d_roll, dev(envs)[0], loss=loss, **KW)
        bits, g, st = _bits(g), g.cpu().numpy().astype(np.float64), st.cpu()
        assert not bits[critic_mlp].any() and not bits[critic_lstm].any() and _bits(st)[4] == 0        # +0.0f, every one, and v_loss
        if loss == "mse":
            assert not bits[log_std].any()
        else:
            assert g[log_std].all()
        assert g[actor_lstm].any()
        # the actor LSTM's block (a shared LSTM: the one block, the actor head's term alone) within bar 1 of the twin
        _bars(spec, flat, twin_roll(roll, False), envs, g, st.numpy(), f"used handle shared={shared} loss={loss}", loss=loss, **KW)
    opt.close(); p.close()


# ---- 3. columns without an env -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,with_ret", [("mse", True), ("nll", False)])
def test_columns_without_an_env(loss, with_ret):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    n_in, H, T, B, Bm = 7, 40, 5, 45, 40
    spec = make_spec(n_in, H, False)
    flat = tw.random_params(spec, seed=8)
    roll = bt.random_rollout(spec, flat, T, B, seed=9)
    envs = np.random.default_rng(10).permutation(B)[:Bm].astype(np.int32)
    envs[1::8] = [-1, -7, -(2 ** 31), -2, -1]                           # a quarter of the columns outside [0, B), on both sides
    envs[5::8] = [B, B + 1, 2 ** 31 - 1, B + 100, B]
    assert ((envs < 0) | (envs >= B)).sum() == Bm // 4 and (envs < 0).any() and (envs >= B).any()
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, T, Bm)
    d_envs = dev(envs)[0]
    g0, s0 = (x.clone() for x in opt.bc_grad(bc_roll(roll, with_ret), d_envs, loss=loss, **KW))
    _bars(spec, flat, twin_roll(roll, with_ret), envs, g0.cpu().numpy().astype(np.float64), s0.cpu().numpy(),
          f"no-env columns loss={loss} returns={with_ret}", loss=loss, **KW)
    # the rows of target / returns that no column reads hold NaN: the same bits
    unread = np.setdiff1d(np.arange(B), envs[(envs >= 0) & (envs < B)])
    assert len(unread) >= 5
    nan = dict(roll, labels=roll["labels"].copy(), returns=roll["returns"].copy())
    nan["labels"][:, unread] = np.nan
    nan["returns"][:, unread] = np.nan
    g1, s1 = opt.bc_grad(bc_roll(nan, with_ret), d_envs, loss=loss, **KW)
    assert bool(t.isfinite(g1).all()) and np.array_equal(_bits(g0), _bits(g1)) and np.array_equal(_bits(s0), _bits(s1))
    opt.close(); p.close()


# ---- 4. determinism and the documented loop -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,with_ret", [("mse", False), ("nll", True)])
def test_update_is_deterministic_and_equals_the_documented_loop(loss, with_ret):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    n_epochs, B, Bm, T, lr = 2, 40, 16, 6, 1e-3
    spec = make_spec(7, 40, False)
    flat = tw.random_params(spec, seed=4)
    roll = bt.random_rollout(spec, flat, T, B, seed=5)
    perms = np.stack([np.random.default_rng(10 + e).permutation(B) for e in range(n_epochs)]).astype(np.int32)
    d, perm = bc_roll(roll, with_ret), dev(perms)[0]
    kw = dict(loss=loss, **KW)
    n_mb = -(-B // Bm)
    assert B % Bm != 0 and n_mb == 3                                     # ragged: 16, 16, 8
    ps = [lstm_policy(spec, flat) for _ in range(3)]
    os_ = [RecurrentPPOOptimizer(q, T, Bm) for q in ps]
    sa = os_[0].bc_update(d, perm, Bm, learning_rate=lr, max_grad_norm=0.5, **kw)
    sb = os_[1].bc_update(d, perm, Bm, learning_rate=lr, max_grad_norm=0.5, **kw)
    sc = t.zeros((n_epochs, n_mb, 8), dtype=t.float32, device="cuda")
    for e in range(n_epochs):
        for k in range(n_mb):
            g, _ = os_[2].bc_grad(d, perm[e, k * Bm:(k + 1) * Bm], stats=sc[e, k], **kw)
            os_[2].apply(g, learning_rate=lr, max_grad_norm=0.5)
    assert sa.shape == (n_epochs, n_mb, 8) and np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(_bits(sa), _bits(sc))
    assert t.equal(ps[0].params, ps[1].params) and t.equal(ps[0].params, ps[2].params)
    assert not t.equal(ps[0].params, t.from_numpy(flat).cuda())
    states = [o.state() for o in os_]
    assert all(s[1] == n_epochs * n_mb for s in states) and np.abs(states[0][0]).max() > 0
    assert all(np.array_equal(states[0][0].view(np.uint32), s[0].view(np.uint32)) for s in states[1:])
    rl_helpers.close_all(os_, ps)


# ---- 5. no contamination the other way ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["two-lstms", "shared-lstm"])
def test_a_ppo_gradient_after_a_supervised_one_is_a_fresh_handles(shared):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    n_in, H, T, B, Bm = 7, 40, 6, 40, 33
    spec = make_spec(n_in, H, shared)
    flat = tw.random_params(spec, seed=13)
    roll = tw.random_rollout(spec, flat, T, B, seed=14)
    other = bt.random_rollout(spec, flat, T, B, seed=15)
    perm = np.random.default_rng(16).permutation(B).astype(np.int32)
    pa, pb = lstm_policy(spec, flat), lstm_policy(spec, flat)
    oa, ob = RecurrentPPOOptimizer(pa, T, Bm), RecurrentPPOOptimizer(pb, T, Bm)
    d, envs = dev_roll(roll), dev(perm[:Bm])[0]
    for loss, with_ret in COMBOS:
        oa.bc_grad(bc_roll(other, with_ret), dev(perm[::-1][:Bm - 3].copy())[0], loss=loss, **KW)
        ga, sa = oa.grad(d, envs, **PPO_KW)
        gb, sb = ob.grad(d, envs, **PPO_KW)
        assert np.array_equal(_bits(ga), _bits(gb)) and np.array_equal(_bits(sa), _bits(sb)) and float(ga.abs().max()) > 0
    rl_helpers.close_all(oa, ob, pa, pb)


# ---- 6. descent on a fixed batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["mse", "nll"])
def test_descent_on_a_fixed_batch(loss):
    """lr = 1e-3, BehaviorCloning's default: Adam moves every parameter by about lr per update, 20 updates move a weight by 0.02 — small
    against weights of 1 / sqrt(fan_in) >= 0.1, so the loss falls steadily; the float64 twin's ``train`` on the same data is asserted to
    descend too, so that a failure tells the reference's behaviour from the kernel's."""
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    T, B, H, lr, n_upd = 8, 64, 32, 1e-3, 20
    spec = make_spec(8, H, False)
    flat = tw.random_params(spec, seed=17)
    roll = bt.random_rollout(spec, flat, T, B, seed=18)
    kw = dict(loss=loss, ent_coef=0.0, vf_coef=0.0)
    perms = np.arange(B, dtype=np.int32)[None]
    key = "mse" if loss == "mse" else "nll"
    falls = ("mse",) if loss == "mse" else ("mse", "nll")               # the final mse, and nll under NLL, is below the first
    ref, log = bt.train(spec, flat, twin_roll(roll, False), np.repeat(perms, n_upd, axis=0), B, lr=lr, **kw)
    for k in falls:
        assert log[-1][k] < log[0][k], (k, log[0][k], log[-1][k])       # the reference descends at this lr
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, T, B)
    d, perm = bc_roll(roll, False), dev(perms)[0]
    after3, st = None, []
    for i in range(n_upd):
        st.append(opt.bc_update(d, perm, B, learning_rate=lr, max_grad_norm=0.5, **kw).cpu().numpy().reshape(8))
        if i == 2:
            after3 = p.params.cpu().numpy().astype(np.float64)
    st = np.stack(st)
    col = bt.STATS.index(key)
    assert np.all(np.isfinite(st))
    for k in falls:
        c = bt.STATS.index(k)
        assert st[-1, c] < st[0, c], (k, st[0, c], st[-1, c])
    assert np.array_equal(st[:, 0], st[:, col])                          # ent_coef = 0, no returns: the loss IS the term
    ref3 = bt.train(spec, flat, twin_roll(roll, False), np.repeat(perms, 3, axis=0), B, lr=lr, **kw)[0]
    f32 = bt.train(spec, flat, twin_roll(roll, False), np.repeat(perms, 3, axis=0), B, lr=lr, dtype=t.float32, **kw)[0]
    e32, err = np.abs(f32 - ref3).max(), np.abs(after3 - ref3).max()
    print(f"r31 bc train loss={loss} device_err={err:.3e} e32={e32:.3e} bar={4 * e32 + 1e-6:.3e} moved={np.abs(ref3 - flat).max():.3e}")
    assert np.abs(ref3 - flat).max() > 1e-4 and err <= 4.0 * e32 + 1e-6, (err, e32)
    if loss == "mse":
        sl = _slices(spec)["log_std"]
        assert np.array_equal(p.params.cpu().numpy()[sl], flat[sl])
    opt.close(); p.close()


# ---- 7. the trainer ----------------------------------------------------------------------------------------------------------------------------
KEYS = ("loss", "mse", "nll", "entropy", "v_loss", "mean_abs_err", "mean_yaw_diff", "mean_episode_power", "mean_episode_return",
        "mean_step_reward", "n_episodes", "fps", "iteration", "num_timesteps", "learning_rate")


def _two_turbine_venv(n_envs, method="yaw"):
    """test_gpu_imitation.py's two-turbine env"""
    from windgym_amd import presets
    d = presets.env1_config()
    d["ActionMethod"] = method
    return _venv(n_envs, yaml_dict=d, n_passthrough=0.5)


def test_learn_save_load_continue_and_fine_tune(tmp_path):
    from windgym_amd import RecurrentBehaviorCloning
    from windgym_amd.curriculum import new_episode_targets
    from windgym_amd.recurrent import MlpLstmPolicy
    from windgym_amd.recurrent_ppo import RecurrentPPO
    from windgym_amd.yaw_table import YawTable
    t = _torch()
    T, B = 40, 32
    kw = dict(n_steps=T, n_epochs=2, seed=11, refine_pass_n=4, yaw_n=5,
              policy_kwargs=dict(lstm_hidden_size=32, net_arch=dict(pi=[16], vf=[16])))
    va, vb = _two_turbine_venv(B), _two_turbine_venv(B)
    a, b = RecurrentBehaviorCloning("MlpLstmPolicy", va, **kw), RecurrentBehaviorCloning("MlpLstmPolicy", vb, **kw)
    assert a.envs_per_batch == 8 and a.batch_size == 8 * T and a.policy.H == 32 and a.policy.nets == 2
    # one collect(): the labels bit for bit against the numpy twin on the rollout's own records
    cfg = va.cfg
    g0, yaw0 = a.targets.cpu().numpy().copy(), va.batch.info("yaw_agent").clone()
    out = a.collect()
    tr = out["truncated"].cpu().numpy()
    assert tr[1:T - 1].any() and out["episode_start"][1:T].any()         # a truncation inside the rollout: starts occur mid-sequence
    ep_row = t.zeros((T, B), dtype=t.int32, device="cuda")
    n_new, ep_target = new_episode_targets(t, out, ep_row, a._optimize, a._no_targets)
    assert n_new == a.last_n_targets == int(tr.sum()) and t.equal(ep_row, a._ep_row)
    rl, rd, rg, bad = it.labels_numpy(yaw0.cpu().numpy(), out["yaw_agent"].cpu().numpy(), tr, ep_row.cpu().numpy(), ep_target.cpu().numpy(),
                                      g0, cfg.ActionMethod, cfg.yaw_min, cfg.yaw_max, cfg.yaw_step)
    assert bad is None and np.array_equal(_bits(out["labels"]), rl.view(np.int32)) and np.array_equal(_bits(out["yaw_diff"]), rd.view(np.int32))
    assert np.array_equal(a.targets.cpu().numpy(), rg) and "returns" not in out
    b.collect()                                                          # (the twin env follows)
    # three iterations then one more == two iterations, save, load, two more
    ls0 = a.policy.state_dict()["log_std"].clone()
    w0 = a.policy.params.clone()
    a.learn(3 * T * B)
    assert len(a.log) == 3 and a.iteration == 3 and a.num_timesteps == 3 * T * B
    for rec in a.log:
        assert set(KEYS) <= set(rec) and all(np.isfinite(float(x)) for x in rec.values()), rec
        assert rec["loss"] == rec["mse"] and rec["v_loss"] == 0.0 and rec["mean_yaw_diff"] >= 0.0
    assert np.array_equal(_bits(a.policy.state_dict()["log_std"]), _bits(ls0)) and not t.equal(a.policy.params, w0)      # MSE: log_std unmoved
    a.learn(T * B, reset_num_timesteps=False)
    b.learn(2 * T * B)
    path = os.path.join(tmp_path, "rbc.zip")
    b.save(path)
    q = MlpLstmPolicy.from_sb3_zip(path)
    assert q.desc == b.policy.desc and t.equal(q.params, b.policy.params)
    q.close()
    c = RecurrentBehaviorCloning.load(path, vb)
    assert t.equal(c.targets, b.targets) and c.args() == b.args() and c.n_epochs == 2 and c.batch_size == b.batch_size
    b.close(); b.policy.close()
    c.learn(2 * T * B, reset_num_timesteps=False)
    assert c.num_timesteps == a.num_timesteps and c.iteration == 4
    assert t.equal(c.policy.params, a.policy.params) and t.equal(c.targets, a.targets)
    (ma, sa), (mc, sc) = a.opt.state(), c.opt.state()
    assert sa == sc == 4 * 2 * 4 and np.array_equal(ma, mc)
    ea, ec = va._lstm_pair(a.policy), vb._lstm_pair(c.policy)
    assert t.equal(ea[1], ec[1]) and t.equal(ea[2], ec[2]) and float(ea[1].abs().max()) > 0      # the pair's LSTM state, the pending starts
    # the two recurrent trainers refuse each other's checkpoints by name
    with pytest.raises(ValueError, match="RecurrentBehaviorCloning wrote it"):
        RecurrentPPO.load(path, vb)
    # fine-tuning: a fresh optimiser on the cloned weights, the pair's LSTM state continues, and an iteration runs
    state = ec[1].clone()
    ppo = RecurrentPPO(c.policy, vb, n_steps=16, n_epochs=1, seed=2)
    assert ppo.opt.state()[1] == 0 and not ppo.opt.state()[0].any() and t.equal(vb._lstm_pair(c.policy)[1], state)
    w = c.policy.params.clone()
    ppo.learn(16 * B)
    assert len(ppo.log) == 1 and np.isfinite(ppo.log[0]["loss"]) and not t.equal(w, c.policy.params)
    assert t.equal(list(vb._lstm_pair(c.policy)[3].values())[-1]["lstm_state0"], state)          # its rollout began from the cloning's state
    other = os.path.join(tmp_path, "rppo.zip")
    ppo.save(other)
    with pytest.raises(ValueError, match="not a windgym_amd RecurrentBehaviorCloning checkpoint"):
        RecurrentBehaviorCloning.load(other, vb)
    # once with a YawTable as the expert: no Serial-Refine launch, nothing counted
    tab = YawTable.build(vb, refine_pass_n=1, yaw_n=3)
    d = RecurrentBehaviorCloning("MlpLstmPolicy", vb, expert=tab, loss="nll", vf_coef=0.5, **dict(kw, n_epochs=1))
    d.learn(T * B)
    assert d.last_n_targets is None and len(d.log) == 1 and np.isfinite(d.log[0]["loss"]) and d.log[0]["v_loss"] > 0.0
    va.batch.check(); vb.batch.check()
    for x in (ppo, a, c, d):
        x.close()
    a.policy.close(); c.policy.close(); d.policy.close(); tab.close()
    va.close(); vb.close()


# ---- 8. refusals on real objects --------------------------------------------------------------------------------------------------------------
def test_refusals():
    from windgym_amd import BehaviorCloning, RecurrentBehaviorCloning
    from windgym_amd.binding import CBcHyper, CLstmBcBatch
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    spec = make_spec(7, 8, False)
    flat = tw.random_params(spec, seed=0)
    roll = bt.random_rollout(spec, flat, 4, 6, seed=1)
    p = lstm_policy(spec, flat)
    d, envs = bc_roll(roll, True), dev(np.arange(6, dtype=np.int32))[0]
    opt = RecurrentPPOOptimizer(p, 3, 4)
    with pytest.raises(NotImplementedError, match="wg_lstm_bc_grad: T = 4 > the T_max = 3"):
        opt.bc_grad(d, envs[:4])
    opt.close()
    opt = RecurrentPPOOptimizer(p, 4, 4)
    with pytest.raises(NotImplementedError, match="wg_lstm_bc_grad: 6 envs in a minibatch > the Bm_max = 4"):
        opt.bc_grad(d, envs)
    perm = envs.reshape(1, 6).contiguous()
    with pytest.raises(NotImplementedError, match="wg_lstm_bc_update: 6 envs in a minibatch > the Bm_max = 4"):
        opt.bc_update(d, perm, 6)
    with pytest.raises(ValueError, match="loss must be one of"):
        opt.bc_grad(d, envs[:4], loss="huber")
    with pytest.raises(ValueError, match="vf_coef and ent_coef must be >= 0"):
        opt.bc_grad(d, envs[:4], vf_coef=-0.5)
    # the ABI itself: an unknown loss and a null target, each named
    g, hp = t.zeros_like(p.params), CBcHyper(7, 0.0, 0.0)
    args = lambda b, h: (opt._h, p.params.data_ptr(), C.byref(b), envs.data_ptr(), 4, C.byref(h), g.data_ptr(), None, p._stream())
    ok = CLstmBcBatch(d["obs"].data_ptr(), d["labels"].data_ptr(), None, d["episode_start"].data_ptr(), d["lstm_state0"].data_ptr(), 4, 6)
    with pytest.raises(ValueError, match="loss must be WG_BC_MSE or WG_BC_NLL, got 7"):
        opt._chk(opt.L.wg_lstm_bc_grad(*args(ok, hp)), "wg_lstm_bc_grad")
    null = CLstmBcBatch(d["obs"].data_ptr(), None, None, d["episode_start"].data_ptr(), d["lstm_state0"].data_ptr(), 4, 6)
    with pytest.raises(ValueError, match="the batch's target is null"):
        opt._chk(opt.L.wg_lstm_bc_grad(*args(null, CBcHyper(0, 0.0, 0.0))), "wg_lstm_bc_grad")
    opt._chk(opt.L.wg_lstm_bc_grad(*args(ok, CBcHyper(0, 0.0, 0.0))), "wg_lstm_bc_grad")          # (and the same call with both in order runs)
    assert bool(t.isfinite(g).all()) and float(g.abs().max()) > 0
    opt.close()
    # the trainers
    v = _two_turbine_venv(4)
    O, N = v.batch.obs_dim, v.n_turb
    lstm = rl_helpers.lstm_members(1, n_in=O, n_out=N)[0]
    with pytest.raises(NotImplementedError, match="recurrent"):
        BehaviorCloning(lstm, v)
    mlp = rl_helpers.make(O, (16,), N)[0]
    with pytest.raises(ValueError, match="needs a recurrent policy"):
        RecurrentBehaviorCloning(mlp, v)
    with pytest.raises(ValueError, match="multiple of n_steps"):
        RecurrentBehaviorCloning(lstm, v, n_steps=8, batch_size=20)
    wrong = rl_helpers.lstm_members(1, n_in=O + 1, n_out=N)[0]
    with pytest.raises(ValueError, match="this env needs"):
        RecurrentBehaviorCloning(wrong, v)
    rl_helpers.close_all(p, lstm, mlp, wrong)
    v.close()
