"""GPU tests of the recurrent trainer at its limits: wg_lstm_ppo_grad (windgym_amd/csrc/wg_lstm_ppo.hip behind RecurrentPPOOptimizer)
on the cases of tests/recurrent_ppo_cases.py — the architecture that ships, relu and deep / absent / asymmetric head stacks behind
the LSTM, degenerate cells — on a handle that is reused at other (T, Bm) than it was created for, on minibatch entries outside the
rollout, and one iteration of the default RecurrentPPO against the reference trainer.

THE BARS.  test_gpu_recurrent_ppo.py's two stay as they are: the whole gradient's worst absolute error is at most ``max(4 e32, 1e-4
|ref|_2 + 1e-6)`` and the LSTM block's at most ``max(4 e32_block, 1e-4 |ref_block|_2)``.  The same form holds here PER TENSOR k of
lstm_bptt_twin.layout: ``err_k <= max(4 e32_k, 1e-4 |ref_k|_2)`` — a critic LSTM or a W_hh with a fraction of the block's norm is
then held to its own size.  ``e32`` is the float32 twin's error against the float64 twin: it comes from the reference side only.  A
tensor whose reference is exactly zero in both has the bar 0.  Each case prints one line with the worst tensor (its err / bar ratio)
and the worst ratio per tensor class; profiles/r22_lstm_ppo_limits_errors.txt keeps a run's lines."""
import numpy as np
import pytest

import lstm_bptt_twin as tw
import recurrent_ppo_cases as rc
from rl_helpers import _torch, _venv, dev, dev_roll, lstm_policy

pytestmark = pytest.mark.gpu


def _ratio(err, bar):
    return 0.0 if err == 0.0 else (err / bar if bar > 0.0 else float("inf"))


def check_against_twin(tag, g, st, ref):
    """Every bar of the module docstring and the stats record, for the device's (gradient, stats) of the case ``ref`` was computed on."""
    g, st = g.detach().cpu().numpy().astype(np.float64), st.detach().cpu().numpy()
    c = rc.compare(ref, g)
    (err, e32, bar), (err_l, _, bar_l) = c["whole"], c["block"]
    worst, classes, missed = None, {}, []
    for name, e_k, e32_k, bar_k in c["tensors"]:
        r_k = _ratio(e_k, bar_k)
        cls = rc.tensor_class(name)
        classes[cls] = max(classes.get(cls, 0.0), r_k)
        if worst is None or r_k > worst[0]:
            worst = (r_k, name, e_k, e32_k, bar_k)
        if not e_k <= bar_k:
            missed.append((name, e_k, e32_k, bar_k))
    print(f"r22 {tag} rows={ref.rows} whole: err={err:.3e} e32={e32:.3e} bar={bar:.3e} | lstm block: err={err_l:.3e} bar={bar_l:.3e} | "
          f"worst tensor {worst[1]}: err={worst[2]:.3e} e32={worst[3]:.3e} bar={worst[4]:.3e} ratio={worst[0]:.3f} | "
          + " ".join(f"{k}={r:.3f}" for k, r in sorted(classes.items())))
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(st))
    assert err <= bar, (err, e32, bar)
    assert err_l <= bar_l, (err_l, bar_l)
    assert not missed, missed
    for i, k in enumerate(tw.STATS):
        tol = 2.0 / ref.rows if k == "clip_fraction" else 1e-5 * max(1.0, abs(ref.stats[k]))
        assert abs(st[i] - ref.stats[k]) <= tol, (k, st[i], ref.stats[k])
    return g


def _grad(opt, roll, envs, kw):
    """One wg_lstm_ppo_grad -> (gradient, stats), copies of their own."""
    g, st = opt.grad(dev_roll(roll), dev(np.asarray(envs, np.int32))[0], **kw)
    return g.clone(), st.clone()


@pytest.mark.parametrize("i", range(len(rc.ARCH_CASES)), ids=[rc.arch_id(c) for c in rc.ARCH_CASES])
def test_arch_grad_vs_twin(i):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    (spec, flat, roll, envs, kw), ref = rc.arch(i)
    T = roll["raw"].shape[0]
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, T, len(envs))
    g, st = _grad(opt, roll, envs, kw)
    check_against_twin(f"arch {rc.arch_id(rc.ARCH_CASES[i])}", g, st, ref)
    opt.close(); p.close()


@pytest.mark.parametrize("name", list(rc.CELL_EDGES))
def test_cell_edge_grad_vs_twin(name):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    (spec, flat, roll, envs, kw), ref = rc.edge(name)
    T = roll["raw"].shape[0]
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, T, len(envs))
    g, st = _grad(opt, roll, envs, kw)
    got = tw.views(spec, check_against_twin(f"edge {name}", g, st, ref))
    # the exact properties, on the device
    if name == "all_fresh":
        assert all(np.all(got[f"{n}.weight_hh_l0"] == 0.0) for n in tw.NETS)
        assert all(np.abs(got[f"{n}.weight_ih_l0"]).max() > 0 for n in tw.NETS)
        zeroed = dict(roll, lstm_state0=np.zeros_like(roll["lstm_state0"]))
        g0, s0 = _grad(opt, zeroed, envs, kw)
        assert t.equal(g, g0) and t.equal(st, s0)
    elif name == "vf_coef_0":
        for k, v in got.items():
            if k.startswith(("lstm_critic.", "mlp_extractor.value_net.", "value_net.")):
                assert np.all(v == 0.0), k
        assert np.abs(got["lstm_actor.weight_hh_l0"]).max() > 0 and st.cpu().numpy()[1] > 0          # the value loss itself is still reported
    opt.close(); p.close()


REUSE_CALLS = rc.REUSE_CALLS


@pytest.mark.parametrize("shared", [False, True], ids=["two", "shared"])
def test_handle_reuse_is_bit_identical(shared):
    """One handle created at (T_max, Bm_max) = (9, 40) through shorter and narrower calls, a short one after a long one and the same
    shape twice: the stash strides come from the maxima, the kernels index with the call's T and Bm.  Every call equals, bit for bit,
    a fresh handle created at exactly its (T, Bm), and is within the bars of the twin."""
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    spec = rc.make_spec(7, 40, shared)
    flat = tw.random_params(spec, seed=21)
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, 9, 40)
    B = 44
    for call, (T, Bm) in enumerate(REUSE_CALLS):
        roll = tw.random_rollout(spec, flat, T, B, seed=30 + call)
        envs = np.random.default_rng(40 + call).permutation(B)[:Bm].astype(np.int32)
        g, st = _grad(opt, roll, envs, rc.KW)
        fresh = RecurrentPPOOptimizer(p, T, Bm)
        g1, s1 = _grad(fresh, roll, envs, rc.KW)
        fresh.close()
        assert t.equal(g, g1) and t.equal(st, s1), (call, T, Bm)
        check_against_twin(f"reuse {'shared' if shared else 'two'} call {call + 1} T={T} Bm={Bm}", g, st, rc.Reference(spec, flat, roll, envs, rc.KW))
    opt.close(); p.close()


def test_entry_outside_the_rollout():
    """Entries -1 and B in a minibatch (first and last column of env tile 1, first and last of tile 2): rows of zeros by the header's
    rule, whatever the handle computed before — a fresh handle and one that has just been through an all-valid call agree bit for
    bit, and with the twin within the bars."""
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    T, B, Bm = 6, 40, 37
    spec = rc.make_spec(7, 40, False)
    flat = tw.random_params(spec, seed=51)
    roll = tw.random_rollout(spec, flat, T, B, seed=52)
    envs = np.random.default_rng(53).permutation(B)[:Bm].astype(np.int32)
    valid = envs.copy()
    envs[[0, 32]] = -1
    envs[[31, 36]] = B
    p = lstm_policy(spec, flat)
    a = RecurrentPPOOptimizer(p, T, Bm)
    ga, sa = _grad(a, roll, envs, rc.KW)
    b = RecurrentPPOOptimizer(p, T, Bm)
    other = tw.random_rollout(spec, flat, T, B, seed=54)
    gv, _ = _grad(b, other, valid, rc.KW)
    gb, sb = _grad(b, roll, envs, rc.KW)
    assert bool(t.isfinite(ga).all()) and bool(t.isfinite(sa).all()) and bool(t.isfinite(gb).all()) and bool(t.isfinite(sb).all())
    assert not t.equal(gv, gb)
    assert t.equal(ga, gb) and t.equal(sa, sb)
    ref = rc.Reference(spec, flat, roll, envs, rc.KW)
    check_against_twin("entry outside the rollout, fresh handle", ga, sa, ref)
    check_against_twin("entry outside the rollout, used handle", gb, sb, ref)
    a.close(); b.close(); p.close()


def test_default_policy_iteration_vs_reference_trainer():
    """RecurrentPPO("MlpLstmPolicy", env) as it ships — H = 256, [64, 64] heads — in its SECOND iteration: a rollout that starts from a
    nonzero LSTM state, Adam continuing from the first iteration's moments, against lstm_bptt_twin.train on the same rollout."""
    from windgym_amd.recurrent_ppo import RecurrentPPO
    t = _torch()
    T, B, n_epochs = 16, 8, 2
    v = _venv(B)
    a = RecurrentPPO("MlpLstmPolicy", v, n_steps=T, n_epochs=n_epochs, seed=7)
    pol = a.policy
    n_in, H, _, _, shared, hidden_pi, hidden_vf, _, activation = rc.ARCH_CASES[0]
    assert (pol.H, pol.nets, tuple(pol.desc["mlp"]["hidden_pi"]), tuple(pol.desc["mlp"]["hidden_vf"]), pol.desc["mlp"]["activation"]) == \
        (H, 1 if shared else 2, hidden_pi, hidden_vf, activation)
    spec = rc.make_spec(pol.n_in, H, shared, hidden_pi, hidden_vf, pol.n_out, activation)
    a.learn(T * B)
    assert a.iteration == 1
    out = a.collect()
    for e in range(n_epochs):
        a._perm[e].copy_(t.randperm(B, generator=a._gen, device=pol.device))
    keys = ("obs", "raw", "logp", "advantage", "returns", "episode_start", "lstm_state0")
    roll = {k: out[k].detach().cpu().numpy().copy() for k in keys}
    assert np.abs(roll["lstm_state0"]).max() > 0 and np.all(np.isfinite(roll["lstm_state0"]))
    perms = a._perm.cpu().numpy()
    flat = pol.params.detach().cpu().numpy().copy()
    mv, step = a.opt.state()
    n = flat.size
    assert step == n_epochs * 4 and np.abs(mv[:n]).max() > 0

    def adam(w):
        import torch
        o = torch.optim.Adam([w], lr=3e-4, eps=1e-5)
        o.state[w] = dict(step=torch.tensor(float(step)), exp_avg=torch.from_numpy(mv[:n].copy()).to(w.dtype),
                          exp_avg_sq=torch.from_numpy(mv[n:].copy()).to(w.dtype))
        return o
    kw = dict(clip_range=0.2, vf_coef=a.vf_coef, ent_coef=a.ent_coef, normalize_advantage=True)
    ref, log = tw.train(spec, flat, roll, perms, a.envs_per_batch, lr=3e-4, max_grad_norm=a.max_grad_norm, adam=adam, **kw)
    f32, _ = tw.train(spec, flat, roll, perms, a.envs_per_batch, lr=3e-4, max_grad_norm=a.max_grad_norm, adam=adam, dtype=t.float32, **kw)
    st = a.opt.update(out, a._perm, a.envs_per_batch, learning_rate=3e-4, max_grad_norm=a.max_grad_norm, **kw)
    e32 = np.abs(f32 - ref).max()
    err = np.abs(pol.params.detach().cpu().numpy().astype(np.float64) - ref).max()
    moved = np.abs(ref - flat).max()
    print(f"r22 default policy iteration 2: device_err={err:.3e} e32={e32:.3e} bar={4 * e32 + 1e-6:.3e} moved={moved:.3e}")
    assert moved > 1e-4 and err <= 4.0 * e32 + 1e-6, (err, e32, moved)
    got = st.cpu().numpy().reshape(-1, 8)
    assert len(log) == got.shape[0] == n_epochs * 4
    for i, k in enumerate(tw.STATS):
        if k != "clip_fraction":
            assert np.allclose(got[:, i], [s[k] for s in log], rtol=1e-4, atol=1e-4), k
    a.close(); pol.close(); v.close()
