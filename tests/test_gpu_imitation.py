"""GPU tests of behaviour cloning (windgym_amd/imitation.py; k_bc_grad / k_bc_reduce of wg_ppo.hip, k_expert_labels of
wg_curriculum.hip) against the twins of tests/imitation_twin.py: the supervised gradient against float64 autograd with the bars of
tests/test_gpu_ppo.py, the exact zeros on a handle that PPO has used, determinism and the documented loop of wg_bc_update, descent,
the labels bit for bit, the trainer on the two-turbine env and on the shared per-turbine policy."""
import copy
import functools
import os

import numpy as np
import pytest

import imitation_twin as tw
import rl_helpers
from oracle import policy_oracle as po
from oracle import ppo_oracle as oo
from rl_helpers import _torch, _venv, batch, dev, flat_grad
from windgym_amd.policy import param_layout

pytestmark = pytest.mark.gpu
make = functools.partial(rl_helpers.make, dtype=np.float64)        # (the float64 state dict the twin takes)
SHAPES = [(8, (64, 64), 4), (7, (33,), 1), (32, (), 16), (160, (64, 64), 80)]
STATS = tw.BC_STATS


def bc_rows(sd, n_in, n_out, n, activation, seed=0):
    """Random rows: expert actions around the actor's mean (sigma 0.3: errors of the size a half-trained clone has), returns
    around the critic's value."""
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-1, 1, (n, n_in)).astype(np.float32)
    mean, value = po.forward(sd, obs, activation)
    target = (mean + 0.3 * rng.standard_normal((n, n_out))).astype(np.float32)
    ret = (value + rng.standard_normal(n)).astype(np.float32)
    return obs, target, ret


def _entries(desc, pick):
    """flat indices of the tensors whose SB3 name satisfies ``pick``"""
    out, o = [], 0
    for name, shape in param_layout(desc):
        k = int(np.prod(shape))
        if pick(name):
            out += list(range(o, o + k))
        o += k
    return np.array(out)


def _bits(x):
    return x.detach().cpu().numpy().view(np.int32)


# ---- 1. the gradient against the twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=rl_helpers.shape_id)
def test_grad_vs_autograd_twin(shape, activation):
    """Bars: tests/test_gpu_ppo.py's — max|g - ref| <= 1e-4 ||ref|| + 1e-6 on the gradient, 1e-5 max(1, |ref|) on every statistic."""
    from windgym_amd.ppo import PPOOptimizer
    n_in, hidden, n_out = shape
    p, sd = make(n_in, hidden, n_out, activation)
    opt = PPOOptimizer(p)
    R = oo.tile_rows(n_in, n_out, hidden, hidden)[0]
    extra, worst = 37, [0.0, 0.0]
    for k, n in enumerate([1, 33, 389, R, R + 1, 2 * R - 1]):
        use_index = k % 2 == 1
        obs, target, ret = bc_rows(sd, n_in, n_out, n + extra, activation, seed=n)
        rng = np.random.default_rng(n + 1)
        rows = np.arange(5, 5 + n)
        if use_index:                                      # repeated rows and entries on both sides of the batch
            rows = rng.permutation(n + extra)[:n]
            if n >= 4:
                rows[1], rows[n // 2], rows[n - 1] = rows[0], -1 - int(rng.integers(3)), n + extra + int(rng.integers(3))
        d_obs, d_target, d_ret = dev(obs, target, ret)
        for loss in ("mse", "nll"):
            for with_ret in (False, True):
                kw = dict(loss=loss, ent_coef=0.01, vf_coef=0.5)
                sel = dict(index=dev(rows.astype(np.int32))[0]) if use_index else dict(first=5, n=n)
                g, st = opt.bc_grad(d_obs, d_target, d_ret if with_ret else None, **sel, **kw)
                g, st = g.cpu().numpy().astype(np.float64), st.cpu().numpy()
                _, grads, rs = tw.bc_loss_and_grad(sd, obs, target, ret if with_ret else None, rows, activation=activation, **kw)
                ref = flat_grad(p.desc, grads)
                err = np.abs(g - ref).max()
                worst[0] = max(worst[0], err / (1e-4 * np.linalg.norm(ref) + 1e-6))
                assert err <= 1e-4 * np.linalg.norm(ref) + 1e-6, (n, loss, with_ret, err, np.linalg.norm(ref))
                for i, name in enumerate(STATS):
                    worst[1] = max(worst[1], abs(st[i] - rs[name]) / (1e-5 * max(1.0, abs(rs[name]))))
                    assert abs(st[i] - rs[name]) <= 1e-5 * max(1.0, abs(rs[name])), (n, loss, with_ret, name, st[i], rs[name])
                assert st[6] == 0.0 and st[7] == 0.0
    print(f"worst fraction of the bar: gradient {worst[0]:.3f}, statistics {worst[1]:.3f}")
    opt.close(); p.close()


# ---- 2. exact zeros on a handle PPO has used ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, (64, 64), 4), (32, (), 16)], ids=rl_helpers.shape_id)
def test_exact_zeros_after_a_ppo_gradient_on_the_same_handle(shape):
    from windgym_amd.ppo import PPOOptimizer
    n_in, hidden, n_out = shape
    p, sd = make(n_in, hidden, n_out)
    opt = PPOOptimizer(p)
    critic = _entries(p.desc, lambda k: "value_net" in k)
    log_std = _entries(p.desc, lambda k: k == "log_std")
    actor = _entries(p.desc, lambda k: "value_net" not in k and k != "log_std")
    obs, target, ret = bc_rows(sd, n_in, n_out, 700, "tanh", seed=4)
    d = dev(obs, target, ret)
    for loss, with_ret in (("mse", False), ("nll", False), ("mse", True)):
        # every workgroup's row of the partials, its statistics slots and the gradient buffer hold another batch's PPO values
        g0, _ = opt.grad(*dev(*batch(sd, n_in, n_out, 4096, "tanh", seed=9)), clip_range=0.2, vf_coef=0.5, ent_coef=0.01)
        g0 = g0.cpu().numpy()
        assert g0[critic].all() and g0[log_std].all()
        g, st = opt.bc_grad(d[0], d[1], d[2] if with_ret else None, first=3, n=650, loss=loss, ent_coef=0.01, vf_coef=0.5)
        bits, g = _bits(g), g.cpu().numpy()
        if not with_ret:
            assert not bits[critic].any() and _bits(st)[4] == 0                   # +0.0f, every one, and v_loss
        else:
            assert g[critic].any()
        if loss == "mse":
            assert not bits[log_std].any()
        else:
            assert g[log_std].all()
        assert g[actor].any()
        _, grads, _ = tw.bc_loss_and_grad(sd, obs, target, ret if with_ret else None, np.arange(3, 653), loss=loss, ent_coef=0.01, vf_coef=0.5)
        ref = flat_grad(p.desc, grads)
        assert np.abs(g - ref).max() <= 1e-4 * np.linalg.norm(ref) + 1e-6
    opt.close(); p.close()


# ---- 3. determinism, the documented loop ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,with_ret", [("mse", False), ("nll", True)])
def test_update_equals_the_documented_loop(loss, with_ret):
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    n_in, hidden, n_out, n, bs, epochs = 32, (64, 64), 16, 1000, 300, 3
    (pa, sd), (pb, _) = make(n_in, hidden, n_out), make(n_in, hidden, n_out)
    assert t.equal(pa.params, pb.params)
    oa, ob = PPOOptimizer(pa), PPOOptimizer(pb)
    obs, target, ret = dev(*bc_rows(sd, n_in, n_out, n, "tanh", seed=2))
    ret = ret if with_ret else None
    kw = dict(loss=loss, ent_coef=0.01, vf_coef=0.5)
    g1, s1 = oa.bc_grad(obs, target, ret, first=0, n=n, out=t.zeros_like(pa.params), **kw)
    g2, s2 = oa.bc_grad(obs, target, ret, first=0, n=n, out=t.full_like(pa.params, 7.0), **kw)
    assert t.equal(g1, g2) and t.equal(s1, s2)
    gen = t.Generator(device="cuda")
    gen.manual_seed(5)
    perm = t.stack([t.randperm(n, generator=gen, device="cuda").int() for _ in range(epochs)]).contiguous()
    n_mb = -(-n // bs)
    assert n % bs != 0 and n_mb == 4                                     # ragged: 300, 300, 300, 100
    p0 = pa.params.clone()
    st = oa.bc_update(obs, target, ret, perm, bs, learning_rate=1e-3, max_grad_norm=0.5, **kw)
    ref = t.zeros_like(st)
    for e in range(epochs):
        for k in range(n_mb):
            m = min(bs, n - k * bs)
            g, _ = ob.bc_grad(obs, target, ret, index=perm[e, k * bs:k * bs + m].contiguous(), n=m, stats=ref[e, k], **kw)
            ob.apply(g, learning_rate=1e-3, max_grad_norm=0.5)
    assert t.equal(pa.params, pb.params) and t.equal(st, ref) and not t.equal(pa.params, p0)
    (ma, sa), (mb, sb) = oa.state(), ob.state()
    assert sa == sb == epochs * n_mb and np.array_equal(ma, mb)
    if loss == "mse":
        assert not ma[-n_out:].any() and not ma[-n_out - pa.params.numel():-pa.params.numel()].any()       # Adam never moved log_std
        assert t.equal(pa.state_dict()["log_std"].cpu(), t.from_numpy(sd["log_std"].astype(np.float32)))
    obs2 = t.rand((64, n_in), device="cuda")
    assert all(t.equal(x, y) for x, y in zip(pa.act(obs2, True, 0, seed=1), pb.act(obs2, True, 0, seed=1)))     # the packed copies too
    rl_helpers.close_all(oa, ob, pa, pb)


# ---- 4. descent ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["mse", "nll"])
def test_descent_on_a_fixed_batch(loss):
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    n_in, hidden, n_out, n = 32, (64, 64), 16, 1024
    p, sd = make(n_in, hidden, n_out)
    if loss == "nll":
        sd["log_std"][:] = 0.0
        p.load_state_dict({k: v.astype(np.float32) for k, v in sd.items()})
    opt = PPOOptimizer(p)
    obs, target, ret = dev(*bc_rows(sd, n_in, n_out, n, "tanh", seed=8))
    perm = t.arange(n, dtype=t.int32, device="cuda").repeat(30, 1).contiguous()
    st = opt.bc_update(obs, target, None, perm, n, loss=loss, learning_rate=1e-3, max_grad_norm=0.5).cpu().numpy()
    losses = st[:, 0, 0]
    assert losses.shape == (30,) and np.all(np.isfinite(st)) and losses[-1] < losses[0], (losses[0], losses[-1])
    assert np.array_equal(losses, st[:, 0, 1] if loss == "mse" else st[:, 0, 2])                     # ent_coef = 0: the loss IS the term
    if loss == "nll":
        assert bool((p.state_dict()["log_std"] != 0).all())
    opt.close(); p.close()


# ---- 5. the labels -----------------------------------------------------------------------------------------------------------------------------
def _two_turbine_venv(n_envs, method):
    from windgym_amd import presets
    d = presets.env1_config()
    d["ActionMethod"] = method
    return _venv(n_envs, yaml_dict=d, n_passthrough=0.5)


def _multi_venv(n_envs):
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnvMulti
    from windgym_amd.turbine import V80
    m = WindFarmVecEnvMulti(V80(), n_envs, yaml_dict=copy.deepcopy(presets.multi_3x3_config()), seed=5, turbtype="None", n_rotor_pts=16,
                            n_passthrough=0.3)
    m.reset(seed=5)
    return m


# (env, rollout length): the episodes of a batch differ in length with their wind speed — T lies between the shortest and the longest
LABEL_CASES = {"two_turbine_yaw": (lambda: _two_turbine_venv(8, "yaw"), 30), "two_turbine_wind": (lambda: _two_turbine_venv(8, "wind"), 30),
               "farm_4x4": (lambda: _venv(4, n_passthrough=0.3), 34), "multi_3x3": (lambda: _multi_venv(4), 13)}


def _policy(v):
    multi = hasattr(v, "possible_agents")
    return rl_helpers.make(v.obs_len, (64, 64), 1)[0] if multi else rl_helpers.make(v.batch.obs_dim, (64, 64), v.n_turb)[0]


@pytest.mark.parametrize("case", list(LABEL_CASES))
def test_labels_against_the_numpy_twin(case):
    from windgym_amd.binding import ExpertLabels
    from windgym_amd.curriculum import new_episode_targets
    from windgym_amd.steady import SteadyStateYawVecAgent
    t = _torch()
    mk, T = LABEL_CASES[case]
    v = mk()
    b, c = v.batch, v.cfg
    B, N = b.B, b.N
    p = _policy(v)
    model = "blondel_jimenez"
    search = dict(refine_pass_n=4, yaw_n=5)
    optimize = lambda ws, wd, ti: b.steady_optimize(ws, wd, ti, model=model, yaw_max=30.0, **search)[0]
    agent = SteadyStateYawVecAgent(env=v, model=model, yaw_max=c.yaw_max, yaw_min=c.yaw_min, search_yaw_max=30.0, **search)
    a0 = t.as_tensor(agent.predict()[0]).to(b.device).clone()
    targets = b.optimal_yaws(model=model, yaw_max=30.0, **search).contiguous()
    g0 = targets.cpu().numpy()
    yaw0 = b.info("yaw_agent").clone()
    out = v.rollout(p, T, record=("yaw_agent", "wind_f64"))
    ep_row = t.zeros((T, B), dtype=t.int32, device=b.device)
    n_new, ep_target = new_episode_targets(t, out, ep_row, optimize, t.zeros((0, N), dtype=t.float64, device=b.device))
    tr = out["truncated"].bool()
    ends = tr.any(dim=0)
    print("first truncation per env:", [int(tr[:, e].nonzero()[0]) if bool(ends[e]) else None for e in range(B)])
    assert bool(ends.any()) and not bool(ends.all()), ends                # at least one env truncates inside the rollout, one does not
    lab = ExpertLabels(b)
    labels, diff = t.full((T, B, N), 9.0, device=b.device), t.full((T, B), 9.0, device=b.device)
    lab.labels(T, yaw0, out["yaw_agent"], out["truncated"], ep_row, ep_target, n_new, targets, labels, diff)
    lab.check()
    method = c.ActionMethod
    rl, rd, rg, bad = tw.labels_numpy(yaw0.cpu().numpy(), out["yaw_agent"].cpu().numpy(), out["truncated"].cpu().numpy(),
                                      ep_row.cpu().numpy(), ep_target.cpu().numpy(), g0, method, c.yaw_min, c.yaw_max, c.yaw_step)
    assert bad is None
    assert np.array_equal(_bits(labels), rl.view(np.int32)) and np.array_equal(_bits(diff), rd.view(np.int32))
    assert np.array_equal(targets.cpu().numpy(), rg)
    assert t.equal(targets, b.optimal_yaws(model=model, yaw_max=30.0, **search))          # the table followed the autoresets
    assert float(labels.abs().max()) <= 1.0
    if method == "wind":
        stay = (~ends).nonzero().view(-1)
        assert all(t.equal(labels[s, e], a0[e]) for e in stay.tolist() for s in range(T))
    else:                                                   # one step of the env's own rule moves each yaw as far towards g as it may
        prev = t.cat([yaw0[None], out["yaw_agent"][:-1]]).cpu().numpy()
        y1 = tw.adjust_yaw_f32(prev[0], labels[0].cpu().numpy(), method, c.yaw_min, c.yaw_max, c.yaw_step).astype(np.float64)
        want = prev[0] + np.sign(g0 - prev[0]) * np.minimum(np.abs(g0 - prev[0]), c.yaw_step)
        assert np.all(np.abs(y1 - want) <= 4.0 * np.spacing(np.float32(c.yaw_max - c.yaw_min + c.yaw_step)))
    # an ep_row entry that is no row of ep_target: skipped, latched, reported once
    targets2 = t.from_numpy(g0).to(b.device)
    lab.labels(T, yaw0, out["yaw_agent"], out["truncated"], ep_row, ep_target[:n_new - 1].contiguous(), n_new - 1, targets2, labels, diff)
    with pytest.raises(ValueError, match=rf"ep_row_dev\[\d+, \d+\] = {n_new - 1} is not a row"):
        lab.check()
    lab.check()
    b.check()
    p.close(); v.close()


# ---- 6. the trainer ----------------------------------------------------------------------------------------------------------------------------
KEYS = ("loss", "mse", "nll", "entropy", "v_loss", "mean_abs_err", "mean_yaw_diff", "mean_episode_power", "mean_episode_return",
        "mean_step_reward", "n_episodes", "fps", "iteration", "num_timesteps", "learning_rate")


def test_learn_save_load_continue_and_fine_tune(tmp_path):
    from windgym_amd import BehaviorCloning
    from windgym_amd.policy import MlpPolicy, read_sb3_zip
    from windgym_amd.ppo import PPO
    t = _torch()
    T = 40
    kw = dict(n_steps=T, n_epochs=2, seed=11, refine_pass_n=4, yaw_n=5)
    va = _two_turbine_venv(32, "yaw")
    a = BehaviorCloning("MlpPolicy", va, **kw)
    ls0 = a.policy.state_dict()["log_std"].clone()
    a.learn(3 * T * va.num_envs)
    assert len(a.log) == 3 and a.iteration == 3 and a.num_timesteps == 3 * T * 32
    for rec in a.log:
        assert set(KEYS) <= set(rec) and all(np.isfinite(float(x)) for x in rec.values()), rec
        assert rec["loss"] == rec["mse"] and rec["v_loss"] == 0.0 and rec["mean_yaw_diff"] >= 0.0
    assert t.equal(a.policy.state_dict()["log_std"], ls0)                      # MSE leaves log_std where it was
    a.learn(T * va.num_envs, reset_num_timesteps=False)
    va.batch.check()
    # 2 iterations, save, load on the same env, 2 more == the 4 above
    vb = _two_turbine_venv(32, "yaw")
    b = BehaviorCloning("MlpPolicy", vb, **kw)
    b.learn(2 * T * vb.num_envs)
    path = os.path.join(tmp_path, "bc.zip")
    b.save(path)
    desc, tensors = read_sb3_zip(path)
    assert desc == b.policy.desc and all(np.array_equal(tensors[k], x.cpu().numpy()) for k, x in b.policy.state_dict().items())
    c = BehaviorCloning.load(path, vb)
    assert t.equal(c.targets, b.targets) and c.args() == b.args() and c.n_epochs == 2 and c.batch_size == b.batch_size
    b.close(); b.policy.close()
    c.learn(2 * T * vb.num_envs, reset_num_timesteps=False)
    assert c.num_timesteps == a.num_timesteps and c.iteration == 4
    assert t.equal(c.policy.params, a.policy.params) and t.equal(c.targets, a.targets)
    (ma, sa), (mc, sc) = a.opt.state(), c.opt.state()
    assert sa == sc and np.array_equal(ma, mc)
    q = MlpPolicy.from_sb3_zip(path)
    q.close()
    # fine-tuning: a fresh optimiser on the cloned weights changes nothing about the policy, and an iteration runs
    obs = vb.batch.obs.clone()
    before = [x.clone() for x in c.policy.act(obs, False, 3, seed=1)]
    ppo = PPO(c.policy, vb, n_steps=16, n_epochs=1, seed=2)
    assert all(t.equal(x, y) for x, y in zip(before, c.policy.act(obs, False, 3, seed=1)))
    assert ppo.opt.state()[1] == 0 and not ppo.opt.state()[0].any()
    w = c.policy.params.clone()
    ppo.learn(16 * vb.num_envs)
    assert len(ppo.log) == 1 and np.isfinite(ppo.log[0]["loss"]) and not t.equal(w, c.policy.params)
    other = os.path.join(tmp_path, "ppo.zip")
    ppo.save(other)
    with pytest.raises(ValueError, match="not a windgym_amd BehaviorCloning checkpoint"):
        BehaviorCloning.load(other, vb)
    vb.batch.check()
    for x in (ppo, a, c):
        x.close()
    a.policy.close(); c.policy.close()
    va.close(); vb.close()


def test_refusals_on_real_envs():
    from windgym_amd import BehaviorCloning
    from windgym_amd.population import Population
    v = _two_turbine_venv(4, "yaw")
    O, N = v.batch.obs_dim, v.n_turb
    lstm = rl_helpers.lstm_members(1, n_in=O, n_out=N)[0]
    with pytest.raises(NotImplementedError, match="recurrent"):
        BehaviorCloning(lstm, v)
    members = rl_helpers.mlp_members(2, n_in=O, n_out=N)
    pop = Population(members)
    with pytest.raises(NotImplementedError, match="population"):
        BehaviorCloning(pop, v)
    split = rl_helpers.make(O, (16,), N, n_in_vf=O + 3)[0]
    with pytest.raises(NotImplementedError, match="split policy"):
        BehaviorCloning(split, v)
    with pytest.raises(ValueError, match="loss must be one of"):
        BehaviorCloning("MlpPolicy", v, loss="l1")
    with pytest.raises(ValueError, match="expert must be one of"):
        BehaviorCloning("MlpPolicy", v, expert="gauss")
    wrong = rl_helpers.make(O + 1, (16,), N)[0]
    with pytest.raises(ValueError, match="this env needs"):
        BehaviorCloning(wrong, v)
    vh = _venv(4, as_torch=False)
    with pytest.raises(ValueError, match="as_torch"):
        BehaviorCloning("MlpPolicy", vh)
    pop.close()
    rl_helpers.close_all(lstm, members, split, wrong)
    v.close(); vh.close()


# ---- 7. the shared per-turbine policy --------------------------------------------------------------------------------------------------------
def test_multi_agent_iteration_equals_its_documented_loop():
    from windgym_amd import BehaviorCloning
    from windgym_amd.policy import MlpPolicy
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    T, B = 16, 4
    v = _multi_venv(B)
    N = v.n_turb
    bc = BehaviorCloning("MlpPolicy", v, n_steps=T, n_epochs=2, vf_coef=0.5, loss="nll", ent_coef=0.001, seed=4, refine_pass_n=4, yaw_n=5)
    assert bc.n_rows == T * B * N and bc.batch_size == T * B * N // 4 and bc.critic == "agent"
    d = bc.policy.desc
    twin = MlpPolicy(d["n_in"], d["n_out"], d["hidden_pi"], d["hidden_vf"], d["activation"])
    twin.load_state_dict(bc.policy.state_dict())
    out = bc.collect()
    labels, ret = out["labels"].view(-1, 1), out["returns"].view(-1)
    assert labels.shape[0] == T * B * N == ret.shape[0] and tuple(out["returns"].shape) == (T, B, N) == tuple(out["labels"].shape)
    obs = out["obs"][:T].view(-1, bc.policy.n_in).clone()
    labels, ret = labels.clone(), ret.clone()
    st = bc.train(out, 1e-3).clone()
    opt = PPOOptimizer(twin)
    bs, n = bc.batch_size, bc.n_rows
    for e in range(2):
        for k in range(-(-n // bs)):
            m = min(bs, n - k * bs)
            g, s = opt.bc_grad(obs, labels, ret, index=bc._perm[e, k * bs:k * bs + m].contiguous(), n=m, loss="nll", ent_coef=0.001, vf_coef=0.5)
            assert t.equal(s, st[e, k])
            opt.apply(g, learning_rate=1e-3, max_grad_norm=0.5)
    assert t.equal(twin.params, bc.policy.params) and bool(st[..., 4].min() > 0)
    bc.learn(T * B)
    assert len(bc.log) == 1 and all(np.isfinite(float(x)) for x in bc.log[0].values()) and bc.log[0]["v_loss"] > 0
    v.batch.check()
    opt.close(); twin.close(); bc.close(); bc.policy.close(); v.close()
