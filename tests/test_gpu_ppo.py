"""GPU tests of training on the device (windgym_amd/csrc/wg_ppo.hip, windgym_amd/ppo.py): k_gae, k_ppo_grad, the Adam step,
wg_ppo_update and PPO.learn against oracle/ppo_oracle.py (float64, gradients from autograd) and a torch reference trainer."""
import functools
import os

import numpy as np
import pytest

import rl_helpers
from oracle import ppo_oracle as oo
from rl_helpers import LIMIT_SHAPES, _torch, _torch_trainer, _venv, batch, dev, flat_grad, shape4, shape_id
from windgym_amd.policy import param_layout

pytestmark = pytest.mark.gpu

SHAPES = [(8, (64, 64), 4), (32, (64, 64), 16), (7, (33,), 1), (200, (128, 128, 128), 2), (1600, (256, 256), 16),
          (160, (64, 64), 80), (32, (), 16)]                        # tests/test_gpu_policy.py's
make = functools.partial(rl_helpers.make, dtype=np.float64)        # (the float64 state dict the oracle takes)
STATS = ("pi_loss", "v_loss", "entropy", "approx_kl", "clip_fraction", "loss")


def tile_id(shape):
    """the test id of a shape with the row tile R it must get (wg_ppo.h's LDS map, restated in oracle/ppo_oracle.py: tile_rows)"""
    n_in, hidden, hidden_vf, n_out = shape4(shape)
    return shape_id(shape) if len(shape) == 3 else f"{shape_id(shape)}-R{oo.tile_rows(n_in, n_out, hidden, hidden_vf)[0]}"


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", [(1, 1), (7, 389), (128, 4096), (128, 1), (1, 4096)])
def test_gae_vs_oracle(T, B):
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    p, _ = make(8, (16,), 2)
    opt = PPOOptimizer(p)
    rng = np.random.default_rng(T * 10007 + B)
    r, v, fv = (rng.standard_normal((T, B)).astype(np.float32) for _ in range(3))
    tr = (rng.uniform(size=(T, B)) < 0.1).astype(np.uint8)
    adv, ret = opt.gae(*dev(r, v, fv, tr), 0.99, 0.95)
    ra, rr = oo.gae(r, v, fv, tr, 0.99, 0.95)
    assert np.allclose(adv.cpu().numpy(), ra, rtol=1e-5, atol=2e-5) and np.allclose(ret.cpu().numpy(), rr, rtol=1e-5, atol=2e-5)
    t.cuda.synchronize()
    opt.close(); p.close()


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("shape", SHAPES + LIMIT_SHAPES, ids=tile_id)
def test_grad_vs_autograd_oracle(shape, activation):
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    n_in, hidden, hidden_vf, n_out = shape4(shape)
    p, sd = make(n_in, hidden, n_out, activation, hidden_vf=hidden_vf)
    opt = PPOOptimizer(p)
    R = oo.tile_rows(n_in, n_out, hidden, hidden_vf)[0]
    # (n, index array?, normalise?); 65 536 rows of 1600 inputs would need a gigabyte for the float64 oracle: skipped there and at
    # the limit shapes; a minibatch of exactly one tile, one row more and one row short of two tiles where the tile is smallest
    cases = [(1, False, True), (33, True, True), (389, False, True), (4096, True, False)]
    cases += [(65536, True, True)] if n_in <= 200 and len(shape) == 3 else []
    cases += [(R, False, True), (R + 1, True, True), (2 * R - 1, False, False)] if R == 4 else []
    for n, use_index, norm in cases:
        extra = 37
        obs, raw, lpo, adv, ret = batch(sd, n_in, n_out, n + extra, activation, seed=n)
        rng = np.random.default_rng(n + 1)
        rows = rng.permutation(n + extra)[:n] if use_index else np.arange(5, 5 + n)
        kw = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=norm)
        d = dev(obs, raw, lpo, adv, ret)
        if use_index:
            g, st = opt.grad(*d, index=dev(rows.astype(np.int32))[0], **kw)
        else:
            g, st = opt.grad(*d, first=5, n=n, **kw)
        g, st = g.cpu().numpy().astype(np.float64), st.cpu().numpy()
        _, grads, rs, ratio = oo.loss_and_grad(sd, obs[rows], raw[rows], lpo[rows], adv[rows], ret[rows], activation=activation, **kw)
        if n >= 389:
            assert (ratio > 1.2).any() and (ratio < 0.8).any()           # both clip sides are exercised
        ref = flat_grad(p.desc, grads)
        err = np.abs(g - ref).max()
        assert err <= 1e-4 * np.linalg.norm(ref) + 1e-6, (n, err, np.linalg.norm(ref))
        # At the limit shapes the surrogate's statistics also carry the float32 resolution of the log-probability itself: a sum of up
        # to 128 terms, |logp| up to 200, enters ratio = exp(logp - logp_old) and is weighted by the advantage, and a minibatch of a
        # few rows averages nothing away.  Worst observed on an MI355X: 1.86e-5 on pi_loss at 7 rows of 128 outputs, 4.5 times less
        # than this term there.  The shapes of SHAPES keep their bar as it was.
        A = adv[rows] if not (norm and n > 1) else (adv[rows] - adv[rows].mean()) / (adv[rows].std(ddof=1) + 1e-8)
        res = 2.0 ** -23 * np.abs(lpo[rows]).max() * max(1.0, np.abs(A).max()) if len(shape) == 4 else 0.0
        for i, k in enumerate(STATS):
            # (a ratio within rounding of a clip bound may fall on the other side in float32: two rows of slack there)
            tol = 2.0 / n if k == "clip_fraction" else 1e-5 * max(1.0, abs(rs[k])) + (res if k in ("pi_loss", "loss") else 0.0)
            assert abs(st[i] - rs[k]) <= tol, (n, k, st[i], rs[k])
    opt.close(); p.close()


EDGES = ["clip_0.05", "clip_0.5", "vf_coef_0", "ent_coef_0", "constant_advantage", "saturated_tanh", "dead_relu_layer", "log_std_-3",
         "log_std_+1.5", "repeated_rows"]


@pytest.mark.parametrize("edge", EDGES)
def test_grad_loss_head_edges(edge):
    """k_ppo_grad where the loss head or an activation's derivative degenerates, against the float64 autograd oracle, same bars."""
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    n_in, hidden, n_out, n, total = 32, (64, 64), 16, 1024, 1500
    activation = "relu" if edge == "dead_relu_layer" else "tanh"
    p, sd = make(n_in, hidden, n_out, activation)
    kw = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)
    kw.update({"clip_0.05": dict(clip_range=0.05), "clip_0.5": dict(clip_range=0.5), "vf_coef_0": dict(vf_coef=0.0),
               "ent_coef_0": dict(ent_coef=0.0)}.get(edge, {}))
    pre = "mlp_extractor.policy_net."
    if edge == "saturated_tanh":                                         # |pre-activation| of every hidden unit far beyond tanh's range
        for k in sd:
            if k.startswith("mlp_extractor") and k.endswith("weight"):
                sd[k] = sd[k] * 400.0
    elif edge == "dead_relu_layer":                                      # no unit of either net's first hidden layer ever fires
        sd[pre + "0.bias"][:] = -100.0
        sd["mlp_extractor.value_net.0.bias"][:] = -100.0
        sd[pre + "2.bias"][:] = np.abs(sd[pre + "2.bias"]) + 0.1         # (the layer behind it lives on its biases)
    elif edge.startswith("log_std"):
        sd["log_std"][:] = float(edge.split("_")[-1])
    p.load_state_dict({k: v.astype(np.float32) for k, v in sd.items()})
    opt = PPOOptimizer(p)
    obs, raw, lpo, adv, ret = batch(sd, n_in, n_out, total, activation, seed=21)
    rng = np.random.default_rng(22)
    rows = rng.permutation(total)[:n]
    if edge == "constant_advantage":
        adv[:] = 0.5            # std 0: the divisor is 1e-8.  (0.5: the float32 mean of n copies is exact, as the float64 one is)
    elif edge == "repeated_rows":
        rows = rng.integers(0, 40, n)                                    # every one of 40 rows about 25 times
        assert len(np.unique(rows)) < n
    g, st = opt.grad(*dev(obs, raw, lpo, adv, ret), index=dev(rows.astype(np.int32))[0], **kw)
    g, st = g.cpu().numpy().astype(np.float64), st.cpu().numpy()
    _, grads, rs, ratio = oo.loss_and_grad(sd, obs[rows], raw[rows], lpo[rows], adv[rows], ret[rows], activation=activation, **kw)
    ref = flat_grad(p.desc, grads)
    err = np.abs(g - ref).max()
    assert np.all(np.isfinite(g)) and err <= 1e-4 * np.linalg.norm(ref) + 1e-6, (err, np.linalg.norm(ref))
    for i, k in enumerate(STATS):
        tol = 2.0 / n if k == "clip_fraction" else 1e-5 * max(1.0, abs(rs[k]))
        assert abs(st[i] - rs[k]) <= tol, (k, st[i], rs[k])
    got = dict(zip([name for name, _ in param_layout(p.desc)], np.split(g, np.cumsum([int(np.prod(s)) for _, s in param_layout(p.desc)])[:-1])))
    if edge == "clip_0.05":
        assert rs["clip_fraction"] > 0.5
    elif edge == "clip_0.5":
        assert 0.0 < rs["clip_fraction"] < 0.2
    elif edge == "constant_advantage":
        assert all(np.all(got[k] == 0.0) for k in got if "policy_net" in k or k.startswith("action_net")) and st[0] == 0.0
        assert np.all(got["log_std"] == -np.float32(kw["ent_coef"])) and np.abs(got["value_net.bias"]).max() > 0
    elif edge == "saturated_tanh":
        hid = np.tanh(obs[rows].astype(np.float64) @ sd[pre + "0.weight"].T + sd[pre + "0.bias"])
        assert np.mean(np.abs(hid) > 1 - 1e-7) > 0.9 and np.abs(got["action_net.bias"]).max() > 0
    elif edge == "dead_relu_layer":
        for k in (pre + "0.weight", pre + "0.bias", pre + "2.weight", "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
                  "mlp_extractor.value_net.2.weight"):
            assert np.all(got[k] == 0.0), k                              # exactly 0 upstream of the dead layer
        assert np.abs(got["action_net.bias"]).max() > 0 and np.abs(got[pre + "2.bias"]).max() > 0 and np.abs(got["value_net.bias"]).max() > 0
    opt.close(); p.close()


def test_grad_is_bit_identical_from_run_to_run():
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    p, sd = make(32, (64, 64), 16)
    opt = PPOOptimizer(p)
    n = 20000
    d = dev(*batch(sd, 32, 16, n, "tanh", seed=9))
    idx = dev(np.random.default_rng(1).permutation(n).astype(np.int32))[0]
    outs = []
    for _ in range(3):
        g, st = opt.grad(*d, index=idx, ent_coef=0.01)
        outs.append((g.clone(), st.clone()))
        opt.grad(*d, first=0, n=777)                                      # other work in between leaves no trace
    for g, st in outs[1:]:
        assert t.equal(g, outs[0][0]) and t.equal(st, outs[0][1])
    opt.close(); p.close()


def test_unchanged_parameters_give_ratio_one():
    """The forward recomputation is k_policy's: on a fresh rollout mean and V are the stored ones, so nothing is clipped."""
    from windgym_amd.ppo import PPO
    t = _torch()
    v = _venv(64)
    ppo = PPO("MlpPolicy", v, n_steps=16, seed=2)
    with t.no_grad():
        ppo.policy.params[-v.n_turb:].uniform_(-0.5, 0.2)                # log_std away from 0
    ppo.policy.sync()
    out = ppo.collect()
    O, N = ppo.policy.n_in, ppo.policy.n_out
    g, st = ppo.opt.grad(out["obs"][:16].view(-1, O), out["raw"].view(-1, N), out["logp"].view(-1), out["advantage"].view(-1),
                         out["returns"].view(-1))
    st = st.cpu().numpy()
    assert abs(st[3]) <= 1e-9 and st[4] == 0.0, st
    # the ratios themselves, from the float64 oracle on the same buffers
    sd = {k: x.cpu().numpy().astype(np.float64) for k, x in ppo.policy.state_dict().items()}
    arrs = [out[k].cpu().numpy() for k in ("raw", "logp", "advantage", "returns")]
    _, _, _, ratio = oo.loss_and_grad(sd, out["obs"][:16].reshape(-1, O).cpu().numpy(), arrs[0].reshape(-1, N), arrs[1].reshape(-1),
                                      arrs[2].reshape(-1), arrs[3].reshape(-1))
    assert np.abs(ratio - 1.0).max() <= 1e-5
    # and V: the value loss of the kernel is that of the stored values, to rounding
    lv = float(((out["returns"] - out["value"]).double() ** 2).mean())
    assert abs(st[1] - lv) <= 1e-6 * max(1.0, lv)
    ppo.close(); ppo.policy.close(); v.close()


@pytest.mark.parametrize("max_norm", [0.05, 1e6])
def test_apply_vs_oracle_and_repack(max_norm):
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    p, sd = make(32, (64, 64), 16)
    opt = PPOOptimizer(p)
    rng = np.random.default_rng(4)
    nf = p.params.numel()
    ref, m, v = p.params.cpu().numpy().astype(np.float64), np.zeros(nf), np.zeros(nf)
    x = dev(rng.uniform(-1, 1, (64, 32)).astype(np.float32))[0]
    for step in range(1, 21):
        gnp = (rng.standard_normal(nf) * 0.1).astype(np.float32)
        before = p.act(x, deterministic=True)[1].clone()
        opt.apply(dev(gnp)[0], learning_rate=1e-3, max_grad_norm=max_norm)
        ref, m, v = oo.adam_step(ref, gnp, m, v, step, 1e-3, max_norm)
        assert np.abs(p.params.cpu().numpy() - ref).max() <= 2e-6, step
        after = p.act(x, deterministic=True)[1].clone()
        assert not t.equal(after, before)
        p.sync()                                                          # the repack already happened: sync() changes nothing
        assert t.equal(p.act(x, deterministic=True)[1], after)
    mv, s = opt.state()
    assert s == 20 and np.allclose(mv[:nf], m, atol=1e-6) and np.allclose(mv[nf:], v, atol=1e-7)
    opt.close(); p.close()


def test_update_equals_the_documented_loop():
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    n, bs, E = 1000, 300, 3                                               # ragged: minibatches of 300, 300, 300, 100
    pa, sd = make(32, (64, 64), 16)
    pb, _ = make(32, (64, 64), 16)
    oa, ob = PPOOptimizer(pa), PPOOptimizer(pb)
    d = dev(*batch(sd, 32, 16, n, "tanh", seed=5))
    perm = t.stack([t.randperm(n, device="cuda") for _ in range(E)]).to(t.int32).contiguous()
    kw = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)
    sa = oa.update(*d, perm, bs, learning_rate=1e-3, max_grad_norm=0.5, **kw)
    assert tuple(sa.shape) == (E, 4, 8)
    for e in range(E):
        for k in range(4):
            idx = perm[e, k * bs:min(n, (k + 1) * bs)].contiguous()
            g, st = ob.grad(*d, index=idx, **kw)
            assert t.equal(st, sa[e, k]), (e, k)
            ob.apply(g, learning_rate=1e-3, max_grad_norm=0.5)
    assert t.equal(pa.params, pb.params)
    x = d[0][:64].contiguous()
    assert t.equal(pa.act(x, deterministic=True)[1], pb.act(x, deterministic=True)[1])
    assert oa.state()[1] == ob.state()[1] == 12
    for o in (oa, ob):
        o.close()
    pa.close(); pb.close()


def _small_box():
    from windgym_amd.mann import generate_mann_box
    return generate_mann_box((256, 64, 32), (3.0, 3.0, 3.0), seed=1234), (3.0, 3.0, 3.0)


def _cfg5_venv(n_envs):
    """cfg2's farm in a frozen Mann box (the small box of the spot checks): k_flow_envb"""
    v = _venv(n_envs, turbtype="MannGenerate", turbulence_box=_small_box())
    assert v.batch.flow_variant() == (64, True, 2)
    return v


def _cfg3_venv(n_envs):
    """Horns Rev 1, 80 turbines: k_flow<256> + k_glue_lean, a policy of 160 inputs and 80 outputs"""
    from windgym_amd import presets
    x, y = presets.horns_rev1_layout()
    v = _venv(n_envs, yaml_dict=presets.horns_rev_config(), x_pos=x, y_pos=y, n_passthrough=0.5)
    assert v.batch.flow_variant() == (256, True, 0) and v.n_turb == 80
    return v


def _one_iteration_vs_torch_reference_trainer(v, rel_bar=1e-5 * 10):
    from windgym_amd.ppo import PPO
    t = _torch()
    B = v.num_envs
    ppo = PPO("MlpPolicy", v, n_steps=32, n_epochs=2, batch_size=B * 32 // 4, ent_coef=0.01, seed=3)
    out = ppo.collect()
    gen_state = ppo._gen.get_state()
    before = ppo.policy.params.clone()
    ppo.train(out, 3e-4, 0.2)
    perm = ppo._perm.clone()
    ppo._gen.set_state(gen_state)
    with t.no_grad():
        after = ppo.policy.params.clone()
        ppo.policy.params.copy_(before)
    ref = _torch_trainer(ppo.policy, out, ppo._adv, ppo._ret, perm, ppo.batch_size, 3e-4, 0.2, 0.5, 0.01, 0.5)
    moved = (after - before).abs().max().item()
    assert moved > 1e-4
    err = ((after - ref).abs() / (ref.abs() + 1e-3)).max().item()
    assert err <= rel_bar, err                                           # relative, with a floor of 1e-3 on |w|
    assert (after - ref).abs().max().item() <= 1e-5
    ppo.close(); ppo.policy.close(); v.close()


def test_one_iteration_vs_torch_reference_trainer():
    _one_iteration_vs_torch_reference_trainer(_venv(512))


@pytest.mark.parametrize("which", ["cfg5", "cfg3"])
def test_one_iteration_vs_torch_reference_trainer_on_other_paths(which):
    """the same iteration on the frozen-box kernel (256 envs) and on the large-farm kernels (64 envs, 80 outputs).

    cfg5 keeps every bar.  On cfg3 the absolute bar (1e-5 on every parameter; worst observed on an MI355X 3.03e-6) stays, the relative
    one is 1e-2 against a worst case of 2.53e-3: SB3 initialises the action head with gain 0.01, so its 80 x 64 weights are of the
    order of the 1e-3 floor, and the worst entry (reference value -1.97e-4) is one whose gradient over the 512 rows of a minibatch nearly
    cancels — Adam divides by that |g|, so the float32 summation orders of k_ppo_grad and of torch's autograd differ by 1.25e-3 of the
    entry's movement.  The same fraction was measured at learning rates 3e-4 (clip fractions up to 0.16) and 3e-5 (nothing clipped):
    it is not a row falling on the other side of a clip bound."""
    if which == "cfg5":
        _one_iteration_vs_torch_reference_trainer(_cfg5_venv(256))
    else:
        _one_iteration_vs_torch_reference_trainer(_cfg3_venv(64), rel_bar=1e-2)


def test_descent_on_a_fixed_batch():
    from windgym_amd.ppo import PPOOptimizer
    p, sd = make(32, (64, 64), 16)
    opt = PPOOptimizer(p)
    arrs = batch(sd, 32, 16, 2048, "tanh", seed=12)
    d = dev(*arrs)
    kw = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.0, normalize_advantage=True)
    l0 = oo.loss_and_grad(sd, *arrs, **kw)[0]
    for _ in range(5):
        g, _ = opt.grad(*d, **kw)
        opt.apply(g, learning_rate=1e-4, max_grad_norm=0.5)
    sd1 = {k: x.cpu().numpy().astype(np.float64) for k, x in p.state_dict().items()}
    l1 = oo.loss_and_grad(sd1, *arrs, **kw)[0]
    assert l1 < l0, (l0, l1)
    opt.close(); p.close()


def _two_turbine_venv(n_envs=32):
    from windgym_amd import presets
    d = presets.env1_config()
    d["ActionMethod"] = "yaw"
    return _venv(n_envs, yaml_dict=d)


@pytest.mark.parametrize("which", ["two_turbine", "cfg2", "cfg5"])
def test_learn_save_load_continue(which, tmp_path):
    from windgym_amd.policy import MlpPolicy, read_sb3_zip
    from windgym_amd.ppo import PPO
    t = _torch()
    mk = {"two_turbine": lambda: _two_turbine_venv(32), "cfg2": lambda: _venv(64), "cfg5": lambda: _cfg5_venv(64)}[which]
    T = 40
    kw = dict(n_steps=T, n_epochs=2, ent_coef=0.001, seed=11)
    # uninterrupted: 4 iterations
    va = mk()
    a = PPO("MlpPolicy", va, **kw)
    calls = []
    a.learn(4 * T * va.num_envs, callback=lambda p: calls.append(p.iteration))
    assert calls == [1, 2, 3, 4] and a.num_timesteps == 4 * T * va.num_envs and len(a.log) == 4
    for rec in a.log:
        assert all(np.isfinite(float(x)) for x in rec.values()), rec
    assert sum(r["n_episodes"] for r in a.log) >= 0 and a.log[-1]["fps"] > 0
    va.batch.check()
    # 2 iterations, save, load on the same env, 2 more
    vb = mk()
    b = PPO("MlpPolicy", vb, **kw)
    b.learn(2 * T * vb.num_envs)
    path = os.path.join(tmp_path, "ppo.zip")
    b.save(path)
    desc, tensors = read_sb3_zip(path)
    assert desc == b.policy.desc and all(np.array_equal(tensors[k], x.cpu().numpy()) for k, x in b.policy.state_dict().items())
    c = PPO.load(path, vb)
    b.close(); b.policy.close()
    c.learn(2 * T * vb.num_envs, reset_num_timesteps=False)
    assert c.num_timesteps == a.num_timesteps and c.iteration == 4
    assert t.equal(c.policy.params, a.policy.params)
    ma, sa = a.opt.state()
    mc, sc = c.opt.state()
    assert sa == sc and np.array_equal(ma, mc)
    vb.batch.check()
    q = MlpPolicy.from_sb3_zip(path)
    q.close()
    for x in (a, c):
        x.close(); x.policy.close()
    va.close(); vb.close()


def test_learn_across_same_step_autoresets_and_sample_site():
    from windgym_amd.ppo import PPO
    from windgym_amd.site import hornsrev1_site
    t = _torch()
    v = _venv(32)
    ppo = PPO("MlpPolicy", v, n_steps=64, n_epochs=1, seed=1)
    n_trunc = []
    ppo.learn(6 * 64 * 32, callback=lambda p: n_trunc.append(int(list(p.venv._rollout_bufs.values())[0]["truncated"].sum())))
    assert sum(n_trunc) > 0                                              # episodes ended (and were reset) inside the rollouts
    assert all(np.isfinite(float(x)) for rec in ppo.log for x in rec.values())
    assert sum(r["n_episodes"] for r in ppo.log) > 0
    v.batch.check()
    ppo.close(); ppo.policy.close(); v.close()
    vs = _venv(16, sample_site=hornsrev1_site())
    ps = PPO("MlpPolicy", vs, n_steps=8, n_epochs=1, seed=1)
    ps.learn(2 * 8 * 16)
    assert len(ps.log) == 2 and all(np.isfinite(float(x)) for rec in ps.log for x in rec.values())
    vs.batch.check()
    ps.close(); ps.policy.close(); vs.close()
