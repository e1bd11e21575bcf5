"""GPU tests of the supervised gradient of an MLP policy at its limits: k_bc_grad / k_bc_reduce of wg_ppo.hip behind
``PPOOptimizer.bc_grad`` against the float64 autograd twin ``imitation_twin.bc_loss_and_grad`` — the policy shapes at the kernel's limits
(``rl_helpers.LIMIT_SHAPES``: four head tiles, a head tile of one row, first-layer chunks, four hidden layers, actor and critic stacks
of different depth), the boundary between the actor's and the critic's entries tensor by tensor, the loss head's edges
(``bc_cases.BC_EDGES``) and a handle that is reused across row counts, losses and PPO.

THE BARS are tests/test_gpu_imitation.py's: ``max|g - ref| <= 1e-4 ||ref|| + 1e-6`` on the gradient (on a tensor alone: with that
tensor's norm), every statistic within ``1e-5 max(1, |ref|)``, ``st[6] == st[7] == 0``.  Every gradient test prints its worst
fraction of the bar; profiles/r32_imitation_limits_errors.txt keeps a run's lines (worst on an MI355X: 0.52 of the gradient's bar at
2048-DEEP-128 with relu, 0.15 at ``saturated_tanh``, below 0.01 everywhere else; 0.053 of a statistic's bar)."""
import functools

import numpy as np
import pytest

import bc_cases as bc
import imitation_twin as tw
import rl_helpers
from oracle import ppo_oracle as oo
from rl_helpers import LIMIT_SHAPES, DEEP, _torch, batch, dev, flat_grad
from test_gpu_imitation import bc_rows
from windgym_amd.policy import param_layout

pytestmark = pytest.mark.gpu
make = functools.partial(rl_helpers.make, dtype=np.float64)        # (the float64 state dict the twin takes)
STATS = tw.BC_STATS
KW = dict(ent_coef=0.01, vf_coef=0.5)


def _bits(x):
    return x.detach().cpu().numpy().view(np.int32)


def _slices(desc):
    """{SB3 name: slice of the flat vector}"""
    out, o = {}, 0
    for name, shape in param_layout(desc):
        k = int(np.prod(shape))
        out[name] = slice(o, o + k)
        o += k
    return out


def _is_critic(name):
    return "value_net" in name


def grad_bar(ref):
    return 1e-4 * np.linalg.norm(ref) + 1e-6


def check(tag, g, st, ref, rs):
    """The module's bars on a device result (numpy) against the twin's flat gradient ``ref`` and statistics ``rs`` -> the fractions
    of the bar (gradient, worst statistic)."""
    err = np.abs(g - ref).max()
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(st)), tag
    assert err <= grad_bar(ref), (tag, err, np.linalg.norm(ref))
    worst = 0.0
    for i, name in enumerate(STATS):
        tol = 1e-5 * max(1.0, abs(rs[name]))
        worst = max(worst, abs(st[i] - rs[name]) / tol)
        assert abs(st[i] - rs[name]) <= tol, (tag, name, st[i], rs[name])
    assert st[6] == 0.0 and st[7] == 0.0, tag
    return err / grad_bar(ref), worst


# ---- a. the limit shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("shape", LIMIT_SHAPES, ids=rl_helpers.shape_id)
def test_limit_shape_grad_vs_twin(shape, activation):
    """tests/test_gpu_imitation.py's first test at the shapes of LIMIT_SHAPES: a minibatch of one row, of 33, of exactly one row
    tile R, one row more, one short of two tiles and 389, as ``first / n`` and as an index array in turn (the index with a repeated
    entry and entries on both sides of the batch), under both losses, with the returns and without."""
    from windgym_amd.ppo import PPOOptimizer
    n_in, hidden, hidden_vf, n_out = shape
    p, sd = make(n_in, hidden, n_out, activation, hidden_vf=hidden_vf)
    opt = PPOOptimizer(p)
    R = oo.tile_rows(n_in, n_out, hidden, hidden_vf)[0]
    extra, worst, at = 37, [0.0, 0.0], None
    for k, n in enumerate([1, 33, R, R + 1, 2 * R - 1, 389]):
        use_index = k % 2 == 1
        obs, target, ret = bc_rows(sd, n_in, n_out, n + extra, activation, seed=n)
        rng = np.random.default_rng(n + 1)
        rows = np.arange(5, 5 + n)
        if use_index:
            rows = rng.permutation(n + extra)[:n]
            if n >= 4:
                rows[1], rows[n // 2], rows[n - 1] = rows[0], -1 - int(rng.integers(3)), n + extra + int(rng.integers(3))
        d_obs, d_target, d_ret = dev(obs, target, ret)
        for loss in ("mse", "nll"):
            for with_ret in (False, True):
                sel = dict(index=dev(rows.astype(np.int32))[0]) if use_index else dict(first=5, n=n)
                g, st = opt.bc_grad(d_obs, d_target, d_ret if with_ret else None, loss=loss, **sel, **KW)
                _, grads, rs = tw.bc_loss_and_grad(sd, obs, target, ret if with_ret else None, rows, activation=activation, loss=loss, **KW)
                f = check((n, use_index, loss, with_ret), g.cpu().numpy().astype(np.float64), st.cpu().numpy(), flat_grad(p.desc, grads), rs)
                at = (n, loss, with_ret) if f[0] > worst[0] else at
                worst = [max(a, b) for a, b in zip(worst, f)]
    print(f"r32 bc limits {rl_helpers.shape_id(shape)} {activation} R={R}: worst fraction of the bar: gradient {worst[0]:.3f} "
          f"(n={at[0]} {at[1]} returns={at[2]}), statistics {worst[1]:.3f}")
    opt.close(); p.close()


# ---- b. the critic boundary, entry by entry --------------------------------------------------------------------------------------------------
UNEQUAL = [(256, (64, 64), DEEP, 16), (256, DEEP, (64, 64), 16), (200, (128, 128, 128), (), 2), (32, (), (33,), 16), (160, (256,), (64, 64), 80)]


@pytest.mark.parametrize("shape", UNEQUAL, ids=rl_helpers.shape_id)
def test_critic_boundary_entry_by_entry(shape):
    """Actor and critic stacks of different depth, without returns, on a handle whose previous call was a PPO gradient of 4096 rows
    (every slot k_bc_reduce must skip holds a foreign value): every critic entry is +0.0f by its bits, every actor tensor (and
    log_std under NLL) is nonzero and within the bar of the twin, each tensor against its own norm."""
    from windgym_amd.ppo import PPOOptimizer
    assert shape in LIMIT_SHAPES and shape[1] != shape[2]
    n_in, hidden, hidden_vf, n_out = shape
    p, sd = make(n_in, hidden, n_out, hidden_vf=hidden_vf)
    opt = PPOOptimizer(p)
    sl = _slices(p.desc)
    critic = np.concatenate([np.arange(s.start, s.stop) for k, s in sl.items() if _is_critic(k)])
    assert len(sl) == 2 * (len(hidden) + len(hidden_vf) + 2) + 1 and critic.size > 0
    assert np.array_equal(critic, np.arange(critic[0], sl["log_std"].start))          # one block, between the actor's entries and log_std
    n, first = 650, 3
    obs, target, ret = bc_rows(sd, n_in, n_out, 700, "tanh", seed=4)
    d = dev(obs, target, ret)
    ppo = dev(*batch(sd, n_in, n_out, 4096, "tanh", seed=9))
    worst = 0.0
    for loss in ("mse", "nll"):
        g0, _ = opt.grad(*ppo, clip_range=0.2, vf_coef=0.5, ent_coef=0.01)
        g0 = g0.cpu().numpy()
        assert g0[critic].all() and g0[sl["log_std"]].all()
        g, st = opt.bc_grad(d[0], d[1], None, first=first, n=n, loss=loss, **KW)
        bits, g, st = _bits(g), g.cpu().numpy().astype(np.float64), st.cpu().numpy()
        assert not bits[critic].any() and st.view(np.int32)[4] == 0              # +0.0f, every one, and v_loss
        _, grads, rs = tw.bc_loss_and_grad(sd, obs, target, None, np.arange(first, first + n), loss=loss, **KW)
        ref = flat_grad(p.desc, grads)
        worst = max(worst, check((loss,), g, st, ref, rs)[0])
        for name, s in sl.items():
            if _is_critic(name):
                continue
            if name == "log_std" and loss == "mse":
                assert not bits[s].any()
                continue
            err = np.abs(g[s] - ref[s]).max()
            worst = max(worst, err / grad_bar(ref[s]))
            assert g[s].any() and (name != "log_std" or g[s].all()), (loss, name)
            assert err <= grad_bar(ref[s]), (loss, name, err, np.linalg.norm(ref[s]))
    print(f"r32 bc critic boundary {rl_helpers.shape_id(shape)}: worst fraction of the bar, whole vector and every tensor: {worst:.3f}")
    opt.close(); p.close()


# ---- c. the loss head's edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge,loss", bc.CASES, ids=[f"{e}-{l}" for e, l in bc.CASES])
def test_loss_head_edges(edge, loss):
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    case, (grads, rs) = bc.edge(edge, loss)
    n_in, hidden, n_out = case.shape
    p, _ = make(n_in, hidden, n_out, case.activation)
    p.load_state_dict({k: v.astype(np.float32) for k, v in case.sd.items()})
    opt = PPOOptimizer(p)
    sl = _slices(p.desc)
    d_obs, d_target, d_ret = dev(case.obs, case.target, case.ret)
    index = dev(case.rows.astype(np.int32))[0]
    if edge == "targets_are_the_means":
        # the device's own unclipped deterministic means of every row (k_policy), in place of the twin's rounded ones
        d_target = p.act(d_obs, deterministic=True)[1].clone().reshape(case.target.shape)
        target = d_target.cpu().numpy()
        assert np.abs(target - case.target).max() <= rl_helpers.RAW_ATOL
        grads, rs = bc.reference(case, target)
    g, st = opt.bc_grad(d_obs, d_target, d_ret, index=index, **case.kw)
    gf, st = g.cpu().numpy(), st.cpu().numpy()
    g = gf.astype(np.float64)
    ref = flat_grad(p.desc, grads)
    f = check((edge, loss), g, st, ref, rs)
    print(f"r32 bc edge {edge} {loss}: worst fraction of the bar: gradient {f[0]:.3f}, statistics {f[1]:.3f}")
    got = {k: g[s] for k, s in sl.items()}
    for k in bc.zero_tensors(edge, loss):
        assert np.all(got[k] == 0.0), k                                  # exactly 0 where the case says so
    actor = [k for k in got if not _is_critic(k) and k != "log_std"]
    if edge == "vf_coef_0":
        assert st[4] > 0 and (loss != "mse" or st[0] == st[1])          # v_loss is reported and is no part of the loss
        assert all(np.abs(got[k]).max() > 0 for k in actor)
    elif edge == "ent_coef_0":
        # the data term alone: the same call with an entropy coefficient differs by that coefficient, subtracted once in float32
        g1, _ = opt.bc_grad(d_obs, d_target, d_ret, index=index, **dict(case.kw, ent_coef=0.01))
        g1 = g1.cpu().numpy()
        assert np.array_equal(g1[sl["log_std"]], gf[sl["log_std"]] - np.float32(0.01)) and gf[sl["log_std"]].all()
        assert np.array_equal(np.delete(g1, np.r_[sl["log_std"]]), np.delete(gf, np.r_[sl["log_std"]]))
    elif edge == "saturated_tanh":
        assert np.abs(got["action_net.bias"]).max() > 0
    elif edge == "dead_relu_layer":
        assert np.abs(got["action_net.bias"]).max() > 0 and np.abs(got[bc.PRE + "2.bias"]).max() > 0 and np.abs(got["value_net.bias"]).max() > 0
    elif edge == "far_targets":
        assert np.abs(got["action_net.bias"]).max() > 1.0 and st[2] > 6400.0                  # |z| > 40 on the rows: a large gradient, finite
    elif edge == "targets_are_the_means":
        # the gradient kernel's forward pass is k_policy's, bit for bit: the error is exactly zero, and with it the actor's whole path
        assert all(np.all(got[k] == 0.0) for k in actor), [k for k in actor if np.any(got[k] != 0.0)]
        assert st[1] == 0.0 and st[5] == 0.0
        if loss == "nll":
            assert np.abs(got["log_std"] - (1.0 - case.kw["ent_coef"])).max() <= grad_bar(ref[sl["log_std"]])
    opt.close(); p.close()


# ---- d. handle reuse -----------------------------------------------------------------------------------------------------------------------------
def test_handle_reuse_is_bit_identical():
    """One handle through a PPO gradient of 4096 rows, then supervised calls of 700 rows with returns, 33 without, 1 under NLL, 389
    under MSE with returns, and the first again: fewer workgroups after more, grid (G, 1) after (G, 2), MSE's written zeros in
    log_std after NLL.  Every supervised result equals, bit for bit, the same call on a fresh handle."""
    from windgym_amd.ppo import PPOOptimizer
    t = _torch()
    n_in, hidden, n_out = 32, (64, 64), 16
    (pa, sd), (pb, _) = make(n_in, hidden, n_out), make(n_in, hidden, n_out)
    assert t.equal(pa.params, pb.params)
    opt = PPOOptimizer(pa)
    obs, target, ret = bc_rows(sd, n_in, n_out, 800, "tanh", seed=6)
    d_obs, d_target, d_ret = dev(obs, target, ret)
    index = dev(np.random.default_rng(7).permutation(800).astype(np.int32))[0]
    calls = [("mse", True, 700), ("mse", False, 33), ("nll", False, 1), ("mse", True, 389), ("mse", True, 700)]
    g0, _ = opt.grad(*dev(*batch(sd, n_in, n_out, 4096, "tanh", seed=9)), clip_range=0.2, vf_coef=0.5, ent_coef=0.01)
    assert bool((g0 != 0).all())
    worst, results = [0.0, 0.0], []
    for loss, with_ret, n in calls:
        args = (d_obs, d_target, d_ret if with_ret else None)
        kw = dict(index=index[:n].contiguous(), loss=loss, **KW)
        g, st = (x.clone() for x in opt.bc_grad(*args, **kw))
        fresh = PPOOptimizer(pb)
        g1, s1 = (x.clone() for x in fresh.bc_grad(*args, **kw))
        fresh.close()
        assert np.array_equal(_bits(g), _bits(g1)) and np.array_equal(_bits(st), _bits(s1)), (loss, with_ret, n)
        _, grads, rs = tw.bc_loss_and_grad(sd, obs, target, ret if with_ret else None, index[:n].cpu().numpy(), loss=loss, **KW)
        f = check((loss, with_ret, n), g.cpu().numpy().astype(np.float64), st.cpu().numpy(), flat_grad(pa.desc, grads), rs)
        worst = [max(a, b) for a, b in zip(worst, f)]
        results.append((g, st))
    assert t.equal(results[0][0], results[-1][0]) and t.equal(results[0][1], results[-1][1])
    print(f"r32 bc handle reuse: worst fraction of the bar: gradient {worst[0]:.3f}, statistics {worst[1]:.3f}")
    rl_helpers.close_all(opt, pa, pb)
