"""GPU tests of behaviour cloning into a recurrent policy at its limits: wg_lstm_bc_grad (k_bc_grad_dh of wg_ppo.hip in front of the BPTT
kernels of wg_lstm_ppo.hip, behind ``RecurrentPPOOptimizer.bc_grad``) on the cases of tests/recurrent_ppo_cases.py under the supervised
head — the architectures (relu, heads directly on h, deep / absent / asymmetric stacks, a shared LSTM, K = H = 255 and 33) and the
degenerate cells, each under both losses with the returns and without — on a handle that is reused at other (T, Bm) and in turn with
PPO, and on minibatch entries outside the rollout with the heads directly on h.

THE BARS are the two recurrent files': the whole gradient's worst absolute error at most ``max(4 e32, 1e-4 |ref|_2 + 1e-6)``, the LSTM
block's and EVERY TENSOR's at most ``max(4 e32, 1e-4 |ref|_2)`` of that part, every statistic within ``1e-5 max(1, |ref|)``.  ``e32``
is the float32 torch run of lstm_bc_twin's rule against its float64 run: it comes from the reference side only.  A tensor whose
reference is exactly zero in both (the critic's side without returns, log_std under MSE) has the bar 0.  Each case prints one line
with the worst tensor and the worst ratio per tensor class; profiles/r32_imitation_limits_errors.txt keeps a run's lines.

``labels_are_the_means`` is the one case whose bar is its ``4 e32`` term on every actor tensor: the labels lie within an ulp of the
means, so the float32 twin's gradient and the device's are both the rounding of a forward pass, 1e-10 in size.  Measured on an MI355X:
0.976 of the bar at worst (``lstm_actor.weight_ih_l0``, error 1.03e-10); every other case stays below 0.02 of its bars."""
import numpy as np
import pytest

import lstm_bc_twin as bt
import lstm_bptt_twin as tw
import recurrent_ppo_cases as rc
import rl_helpers
from rl_helpers import _torch, dev, dev_roll, lstm_policy

pytestmark = pytest.mark.gpu
COMBO_IDS = [f"{loss}-{'returns' if r else 'no_returns'}" for loss, r in rc.BC_COMBOS]


def _ratio(err, bar):
    return 0.0 if err == 0.0 else (err / bar if bar > 0.0 else float("inf"))


def _bits(x):
    return x.detach().cpu().numpy().view(np.int32)


def bc_roll(roll):
    """a built supervised case's rollout as the device tensors wg_lstm_bc_grad takes (``returns`` None: left out)"""
    keys = ("obs", "labels", "episode_start", "lstm_state0") + (("returns",) if roll.get("returns") is not None else ())
    return dict(zip(keys, dev(*[roll[k] for k in keys])))


def check_against_twin(tag, g, st, ref):
    """Every bar of the module docstring, for the device's (gradient, stats) of the case ``ref`` (a BcReference) was computed on."""
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
    s_worst = max(abs(st[i] - ref.stats[k]) / (1e-5 * max(1.0, abs(ref.stats[k]))) for i, k in enumerate(bt.STATS))
    print(f"r32 bc {tag} rows={ref.rows} whole: err={err:.3e} e32={e32:.3e} bar={bar:.3e} | lstm block: err={err_l:.3e} bar={bar_l:.3e} | "
          f"worst tensor {worst[1]}: err={worst[2]:.3e} e32={worst[3]:.3e} bar={worst[4]:.3e} ratio={worst[0]:.3f} | "
          + " ".join(f"{k}={r:.3f}" for k, r in sorted(classes.items())) + f" | statistics={s_worst:.3f}")
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(st))
    assert err <= bar, (err, e32, bar)
    assert err_l <= bar_l, (err_l, bar_l)
    assert not missed, missed
    for i, k in enumerate(bt.STATS):
        assert abs(st[i] - ref.stats[k]) <= 1e-5 * max(1.0, abs(ref.stats[k])), (k, st[i], ref.stats[k])
    assert st[6] == 0.0 and st[7] == 0.0
    return g


def _bc_grad(opt, roll, envs, kw):
    """One wg_lstm_bc_grad -> (gradient, stats), copies of their own."""
    g, st = opt.bc_grad(bc_roll(roll), dev(np.asarray(envs, np.int32))[0], **kw)
    return g.clone(), st.clone()


def _ppo_grad(opt, roll, envs):
    g, st = opt.grad(dev_roll(roll), dev(np.asarray(envs, np.int32))[0], **rc.KW)
    return g.clone(), st.clone()


# ---- a. the architectures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(rc.ARCH_CASES)), ids=[rc.arch_id(c) for c in rc.ARCH_CASES])
def test_arch_grad_vs_twin(i):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    (spec, flat, roll, envs, _), _ = rc.bc_arch(i, *rc.BC_COMBOS[0])
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, roll["labels"].shape[0], len(envs))
    for (loss, with_ret), cid in zip(rc.BC_COMBOS, COMBO_IDS):
        (_, _, roll, _, kw), ref = rc.bc_arch(i, loss, with_ret)
        g, st = _bc_grad(opt, roll, envs, kw)
        check_against_twin(f"arch {rc.arch_id(rc.ARCH_CASES[i])} {cid}", g, st, ref)
    opt.close(); p.close()


# ---- b. the degenerate cells ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.BC_CELL_EDGES)
def test_cell_edge_grad_vs_twin(name):
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    (spec, flat, roll, envs, _), ref0 = rc.bc_edge(name, *rc.BC_COMBOS[0])
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, roll["labels"].shape[0], len(envs))
    critic_lstm = np.concatenate([np.arange(s.start, s.stop) for k, s in ref0.slices if k.startswith("lstm_critic.")])
    for (loss, with_ret), cid in zip(rc.BC_COMBOS, COMBO_IDS):
        (_, _, roll, _, kw), ref = rc.bc_edge(name, loss, with_ret)
        if name == "all_fresh" and not with_ret:
            # the skipped critic net's dh, stash and partial sums hold a PPO call's values on other rows
            other = tw.random_rollout(spec, flat, roll["labels"].shape[0], roll["labels"].shape[1], seed=77)
            g0, _ = _ppo_grad(opt, other, envs[::-1].copy())
            assert np.count_nonzero(g0.cpu().numpy()[critic_lstm]) > critic_lstm.size // 2
        g, st = _bc_grad(opt, roll, envs, kw)
        got = tw.views(spec, check_against_twin(f"edge {name} {cid}", g, st, ref))
        # the exact properties, on the device
        for k, v in got.items():
            if rc.bc_is_zero_tensor(name, k, loss, with_ret):
                assert np.all(v == 0.0), (cid, k)
        if name == "all_fresh":
            assert np.isnan(roll["lstm_state0"]).all()
            assert np.abs(got["lstm_actor.weight_ih_l0"]).max() > 0 and (not with_ret or np.abs(got["lstm_critic.weight_ih_l0"]).max() > 0)
            if not with_ret:
                assert not _bits(g)[critic_lstm].any()                   # +0.0f by bits, next to a NaN state and a used handle
            zeroed = dict(roll, lstm_state0=np.zeros_like(roll["lstm_state0"]))
            g1, s1 = _bc_grad(opt, zeroed, envs, kw)
            assert t.equal(g, g1) and t.equal(st, s1)
        elif name == "vf_coef_0" and with_ret:
            assert np.abs(got["lstm_actor.weight_hh_l0"]).max() > 0 and st.cpu().numpy()[4] > 0        # the value loss itself is still reported
    opt.close(); p.close()


# ---- c. handle reuse ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["two", "shared"])
def test_handle_reuse_is_bit_identical(shared):
    """One handle created at (T_max, Bm_max) = (9, 40) through the sizes of REUSE_CALLS three times over, the calls cycling through a
    PPO gradient, a supervised one with returns and one without (so every size meets every kind, a PPO gradient follows a supervised
    call without returns four times, and the losses alternate).  Every call equals, bit for bit, the same call on a fresh handle
    created at exactly its (T, Bm): the skipped net's dh[1], wpart columns and h plane held another call's rows."""
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    spec = rc.make_spec(7, 40, shared)
    flat = tw.random_params(spec, seed=21)
    p = lstm_policy(spec, flat)
    opt = RecurrentPPOOptimizer(p, *rc.REUSE_CALLS[0])
    B, n_after = 44, 0
    for call in range(3 * len(rc.REUSE_CALLS)):
        T, Bm = rc.REUSE_CALLS[call % len(rc.REUSE_CALLS)]
        kind = call % 3                                                  # 0: PPO, 1: supervised with returns, 2: supervised without
        roll = bt.random_rollout(spec, flat, T, B, seed=30 + call)
        envs = np.random.default_rng(40 + call).permutation(B)[:Bm].astype(np.int32)
        fresh = RecurrentPPOOptimizer(p, T, Bm)
        if kind == 0:
            (g, st), (g1, s1) = _ppo_grad(opt, roll, envs), _ppo_grad(fresh, roll, envs)
            n_after += call > 0
        else:
            kw = dict(rc.BC_KW, loss=("mse", "nll")[(call // 3) % 2])
            roll = roll if kind == 1 else dict(roll, returns=None)
            (g, st), (g1, s1) = _bc_grad(opt, roll, envs, kw), _bc_grad(fresh, roll, envs, kw)
        fresh.close()
        assert np.array_equal(_bits(g), _bits(g1)) and np.array_equal(_bits(st), _bits(s1)), (call, kind, T, Bm)
        assert float(g.abs().max()) > 0
    assert n_after == 4
    opt.close(); p.close()


# ---- d. columns outside the rollout ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,with_ret", rc.BC_COMBOS, ids=COMBO_IDS)
def test_entry_outside_the_rollout(loss, with_ret):
    """test_gpu_recurrent_ppo_limits.py's test of the same name under the supervised head, at the ARCH_CASES shape with the heads directly
    on h (no hidden layers, a shared LSTM, 80 outputs): entries -1 and B in the first and last column of env tile 1 and of tile 2 are
    rows of zeros by the header's rule, whatever the handle computed before — a fresh handle and one that has just been through an
    all-valid call agree bit for bit, and with the twin within the bars."""
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    t = _torch()
    case = rc.ARCH_CASES[2]
    n_in, H, _, _, shared, hidden_pi, hidden_vf, n_out, activation = case
    assert (shared, hidden_pi, hidden_vf, n_out) == (True, (), (), 80)
    T, B, Bm = 6, 40, 37
    spec = rc.make_spec(n_in, H, shared, hidden_pi, hidden_vf, n_out, activation)
    flat = tw.random_params(spec, seed=51)
    twin = lambda r: r if with_ret else dict(r, returns=None)           # noqa: E731
    roll = twin(bt.random_rollout(spec, flat, T, B, seed=52))
    envs = np.random.default_rng(53).permutation(B)[:Bm].astype(np.int32)
    valid = envs.copy()
    envs[[0, 32]] = -1
    envs[[31, 36]] = B
    kw = dict(rc.BC_KW, loss=loss)
    p = lstm_policy(spec, flat)
    a = RecurrentPPOOptimizer(p, T, Bm)
    ga, sa = _bc_grad(a, roll, envs, kw)
    b = RecurrentPPOOptimizer(p, T, Bm)
    other = twin(bt.random_rollout(spec, flat, T, B, seed=54))
    gv, _ = _bc_grad(b, other, valid, kw)
    gb, sb = _bc_grad(b, roll, envs, kw)
    assert bool(t.isfinite(ga).all()) and bool(t.isfinite(sa).all()) and bool(t.isfinite(gb).all()) and bool(t.isfinite(sb).all())
    assert not t.equal(gv, gb)
    assert t.equal(ga, gb) and t.equal(sa, sb)
    ref = rc.BcReference(spec, flat, roll, envs, kw)
    check_against_twin(f"entry outside the rollout {loss} returns={with_ret}, fresh handle", ga, sa, ref)
    check_against_twin(f"entry outside the rollout {loss} returns={with_ret}, used handle", gb, sb, ref)
    rl_helpers.close_all(a, b, p)
