"""CPU tests of tests/lstm_bptt_twin.py, the float64 restatement the recurrent trainer's GPU tests compare with, and of the host-side
rules of windgym_amd/recurrent_ppo.py (the minibatch partition, batch_size)."""
import numpy as np
import pytest
import torch

import lstm_bptt_twin as tw
import lstm_twin

SPEC = dict(n_in=5, H=7, n_out=2, hidden_pi=(6,), hidden_vf=(4, 3), shared=False, activation="tanh")


def _case(spec, T=6, B=5, seed=0, **kw):
    flat = tw.random_params(spec, seed)
    return flat, tw.random_rollout(spec, flat, T, B, seed + 1, **kw)


@pytest.mark.parametrize("shared", [False, True])
def test_forward_equals_lstm_twin_through_time(shared):
    spec = dict(SPEC, shared=shared)
    flat, roll = _case(spec)
    T, B = roll["raw"].shape[:2]
    p64 = tw.views(spec, torch.from_numpy(flat.astype(np.float64)))
    hs, fin = tw.unroll(spec, p64, torch.from_numpy(roll["obs"][:T]).double(), torch.from_numpy(roll["episode_start"][:T]),
                        torch.from_numpy(roll["lstm_state0"]).double(), torch.arange(B))
    params = {k: v.numpy() for k, v in p64.items()}
    state = roll["lstm_state0"].astype(np.float64)
    for t in range(T):
        out, state = lstm_twin.step(params, roll["obs"][t], state, roll["episode_start"][t])
        np.testing.assert_allclose(hs[0][t].numpy(), out["h_pi"], rtol=0, atol=1e-14)
        np.testing.assert_allclose(hs[-1][t].numpy(), out["h_vf"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(fin.numpy(), state, rtol=0, atol=1e-14)
    assert roll["episode_start"][1:T].any() and roll["episode_start"][0].any() and not roll["episode_start"][0].all()


def test_lstm_gradient_equals_torch_nn_lstm():
    spec = dict(SPEC, shared=True)
    T, B = 6, 4
    flat = tw.random_params(spec, 3)
    roll = tw.random_rollout(spec, flat, T, B, 4, starts=np.zeros((T + 1, B), np.uint8))
    roll["lstm_state0"][:] = 0.0
    envs = np.array([2, 0, 3])
    _, _, g, _ = tw.loss_and_grad(spec, flat, roll, envs, ent_coef=0.01)
    # the same loss with torch.nn.LSTM as the recurrence: h rows from the module, heads from the twin
    w = torch.from_numpy(flat.astype(np.float64)).requires_grad_(True)
    p = tw.views(spec, w)
    lstm = torch.nn.LSTM(spec["n_in"], spec["H"], batch_first=False).double()
    names = [("weight_ih_l0", "lstm_actor.weight_ih_l0"), ("weight_hh_l0", "lstm_actor.weight_hh_l0"), ("bias_ih_l0", "lstm_actor.bias_ih_l0"),
             ("bias_hh_l0", "lstm_actor.bias_hh_l0")]
    x = torch.from_numpy(roll["obs"][:T][:, envs]).double()
    h, _ = torch.func.functional_call(lstm, {a: p[b] for a, b in names}, (x,))
    mean = tw._mlp(p, "policy_net", "action_net", h.reshape(-1, spec["H"]), "tanh")
    V = tw._mlp(p, "value_net", "value_net", h.reshape(-1, spec["H"]), "tanh")[:, 0]
    pick = lambda k: torch.from_numpy(roll[k][:, envs]).double().reshape((T * len(envs),) + roll[k].shape[2:])
    ls = p["log_std"]
    z = (pick("raw") - mean) / torch.exp(ls)
    ratio = torch.exp((-0.5 * z * z - ls - tw.HALF_LOG_2PI).sum(1) - pick("logp"))
    A = pick("advantage")
    A = (A - A.mean()) / (A.std() + 1e-8)
    total = (-torch.min(ratio * A, torch.clamp(ratio, 0.8, 1.2) * A).mean() + 0.5 * ((pick("returns") - V) ** 2).mean()
             - 0.01 * (0.5 + tw.HALF_LOG_2PI + ls).sum())
    total.backward()
    ref = w.grad.numpy()
    n_lstm = 4 * spec["H"] * (spec["n_in"] + spec["H"] + 2)
    assert np.abs(ref[:n_lstm]).max() > 1e-4
    np.testing.assert_allclose(g, ref, rtol=0, atol=1e-13)


def test_episode_start_cuts_the_gradient():
    spec = dict(SPEC)
    T, B, cut = 7, 3, 4
    starts = np.zeros((T + 1, B), np.uint8)
    starts[cut] = 1
    flat, roll = _case(spec, T=T, B=B, seed=5, starts=starts)
    envs = np.array([1, 2, 0])
    kw = dict(steps=range(cut, T), normalize_advantage=False)
    l0, _, g0, _ = tw.loss_and_grad(spec, flat, roll, envs, **kw)
    other = {k: v.copy() for k, v in roll.items()}
    other["obs"][:cut] += 3.0
    other["lstm_state0"][:] = -other["lstm_state0"] + 0.25
    l1, _, g1, _ = tw.loss_and_grad(spec, flat, other, envs, **kw)
    assert l0 == l1 and np.array_equal(g0, g1) and np.abs(g0).max() > 0
    # without the start the same perturbation does change it
    for r in (roll, other):
        r["episode_start"][cut] = 0
    assert not np.array_equal(tw.loss_and_grad(spec, flat, roll, envs, **kw)[2], tw.loss_and_grad(spec, flat, other, envs, **kw)[2])


def test_nan_state_of_a_fresh_row_does_not_get_through():
    spec = dict(SPEC)
    flat, roll = _case(spec, seed=7)
    fresh = roll["episode_start"][0] != 0
    zeroed = {k: v.copy() for k, v in roll.items()}
    zeroed["lstm_state0"][:, :, fresh] = 0.0
    roll["lstm_state0"][:, :, fresh] = np.nan
    a, b = tw.loss_and_grad(spec, flat, roll, np.arange(5)), tw.loss_and_grad(spec, flat, zeroed, np.arange(5))
    assert np.isfinite(a[2]).all() and np.array_equal(a[2], b[2]) and a[0] == b[0]


def test_minibatch_partition_and_batch_size():
    from windgym_amd.recurrent_ppo import envs_per_minibatch
    perm = np.random.default_rng(0).permutation(40)
    mbs = tw.minibatches(perm, 16)
    assert [len(m) for m in mbs] == [16, 16, 8] and np.array_equal(np.concatenate(mbs), perm)
    for f in (tw.envs_per_batch, envs_per_minibatch):
        assert f(None, 128, 10) == 3 and f(None, 6, 40) == 10 and f(6 * 16, 6, 40) == 16 and f(128, 128, 4096) == 1
        with pytest.raises(ValueError, match="multiple of n_steps"):
            f(100, 6, 40)
        with pytest.raises(ValueError, match="multiple of n_steps"):
            f(3, 6, 40)


def test_train_clips_by_the_global_norm_and_steps_adam():
    spec = dict(SPEC)
    flat, roll = _case(spec, seed=9)
    perm = np.array([3, 1, 4, 0, 2])
    new, log = tw.train(spec, flat, roll, [perm], 5, lr=1e-3, max_grad_norm=0.01)
    _, _, g, _ = tw.loss_and_grad(spec, flat, roll, perm)
    assert np.linalg.norm(g) > 0.01 and len(log) == 1
    gc = g * (0.01 / (np.linalg.norm(g) + 1e-6))
    m, v = 0.1 * gc, 0.001 * gc * gc
    step = flat.astype(np.float64) - 1e-3 / 0.1 * m / (np.sqrt(v) / np.sqrt(0.001) + 1e-5)
    np.testing.assert_allclose(new, step, rtol=0, atol=1e-12)


def test_twin_layout_is_the_package_layout():
    from windgym_amd import recurrent
    for shared in (False, True):
        spec = dict(SPEC, shared=shared)
        desc = recurrent.make_lstm_desc(spec["n_in"], spec["n_out"], spec["H"], spec["hidden_pi"], spec["hidden_vf"], shared)
        assert [(k, tuple(s)) for k, s in recurrent.param_layout(desc)] == [(k, tuple(s)) for k, s in tw.layout(spec)]
        assert recurrent.n_params(desc) == tw.n_params(spec)
