"""CPU test of tests/recurrent_ppo_cases.py: every case meets, on the twin alone, the conditions that make it a test of the device —
a finite gradient, every LSTM tensor's gradient nonzero (or exactly zero where the case says so, in float64 AND float32), both clip
sides where there are rows enough, and the degeneracy its name promises — and of the twin's rule for an entry outside the rollout."""
import numpy as np
import pytest
import torch

import lstm_bptt_twin as tw
import recurrent_ppo_cases as rc


def _conditions(built, ref, zero=lambda name: False):
    spec, flat, roll, envs, kw = built
    assert np.all(np.isfinite(ref.grad)) and np.all(np.isfinite(ref.grad32))
    assert sum(s.stop - s.start for _, s in ref.slices) == ref.grad.size == tw.n_params(spec)
    for name, sl in ref.slices:
        if zero(name):
            assert np.all(ref.grad[sl] == 0.0) and np.all(ref.grad32[sl] == 0.0), name
        elif name.startswith("lstm_"):
            assert np.abs(ref.grad[sl]).max() > 0, name
    if ref.rows >= 128:
        assert (ref.ratio > 1.0 + kw["clip_range"]).any() and (ref.ratio < 1.0 - kw["clip_range"]).any()


@pytest.mark.parametrize("i", range(len(rc.ARCH_CASES)), ids=[rc.arch_id(c) for c in rc.ARCH_CASES])
def test_arch_case_is_a_test(i):
    built, ref = rc.arch(i)
    spec, flat, roll, envs, kw = built
    n_in, H, T, Bm = rc.ARCH_CASES[i][:4]
    assert roll["raw"].shape == (T, Bm + rc.EXTRA, spec["n_out"]) and len(envs) == Bm == len(set(envs.tolist()))
    es = roll["episode_start"][:T, envs]
    assert es[0].any() and (Bm < 8 or not es[0].all())
    _conditions(built, ref)


def test_the_first_arch_case_is_the_default_policy():
    import inspect
    from windgym_amd.recurrent_ppo import RecurrentPPO
    n_in, H, T, Bm, shared, pi, vf, n_out, act = rc.ARCH_CASES[0]
    assert inspect.signature(RecurrentPPO.__init__).parameters["n_steps"].default == T == 128
    # (the default architecture itself: test_gpu_recurrent_ppo_limits.py builds the default policy and compares its shape with this)
    assert (H, pi, vf, shared, act) == (256, (64, 64), (64, 64), False, "tanh")


def test_the_tensor_bar_catches_what_the_block_bar_lets_through():
    """Negative control of recurrent_ppo_cases.compare on the default architecture: the float32 twin passes every bar; an error in the
    critic's W_hh alone, twice that tensor's bar, passes the whole-gradient and the LSTM-block bar and misses the tensor's own."""
    _, ref = rc.arch(0)
    ok = rc.compare(ref, ref.grad32)
    assert ok["whole"][0] <= ok["whole"][2] and ok["block"][0] <= ok["block"][2] and all(e <= b for _, e, _, b in ok["tensors"])
    (name, sl), = [(k, s) for k, s in ref.slices if k == "lstm_critic.weight_hh_l0"]
    bar_k = dict((k, b) for k, _, _, b in ok["tensors"])[name]
    assert 0 < 2.0 * bar_k < ok["block"][2] < ok["whole"][2]
    wrong = ref.grad32.copy()
    wrong[sl] += 2.0 * bar_k
    bad = rc.compare(ref, wrong)
    assert bad["whole"][0] <= bad["whole"][2] and bad["block"][0] <= bad["block"][2]
    assert [k for k, e, _, b in bad["tensors"] if not e <= b] == [name]


@pytest.mark.parametrize("name", list(rc.CELL_EDGES))
def test_cell_edge_is_a_test(name):
    built, ref = rc.edge(name)
    spec, flat, roll, envs, kw = built
    T = roll["raw"].shape[0]
    es = roll["episode_start"][:T]
    _conditions(built, ref, lambda k: rc.is_zero_tensor(name, k))
    if name == "all_fresh":
        assert es.all() and np.isnan(roll["lstm_state0"]).all()
    elif name == "none_fresh":
        assert not es.any() and np.abs(roll["lstm_state0"]).min() > 0
    elif name == "vf_coef_0":
        assert kw["vf_coef"] == 0.0
    elif name == "saturated_gates":
        assert rc.gate_saturation(spec, flat, roll, envs) >= 0.25
        weak = flat.copy()                                      # at a quarter of the factor the case would be no edge
        for sl in rc._lstm_slices(spec).values():
            weak[sl] *= np.float32(0.25)
        assert rc.gate_saturation(spec, weak, roll, envs) < 0.02
    elif name == "long_carry":
        assert (spec["H"], T, len(envs)) == (64, 128, 3) and not es.any()
        # the forget gates stay open: the carried dc of the last step still reaches step 0
        p = tw.views(spec, flat.astype(np.float64))
        assert all(p[f"{n}.bias_ih_l0"][64:128].min() > 3.5 for n in tw.NETS)
    elif name == "large_c0":
        carried = roll["episode_start"][0] == 0
        assert carried.any() and np.abs(roll["lstm_state0"][:, 1][:, carried]).max() > 10.0
    elif name == "start_on_last_step_only":
        assert not es[:T - 1].any() and es[T - 1].any() and not es[T - 1].all()
    elif name == "constant_advantage":
        assert np.all(roll["advantage"] == roll["advantage"].flat[0]) and ref.stats["adv_std"] == 0.0 and ref.stats["pi_loss"] == 0.0


def test_entry_outside_the_rollout_is_rows_of_zeros():
    """The twin's rule for a column without an env, against the same loss written out on the other columns' rows."""
    spec = rc.make_spec(5, 7, False, (6,), (4, 3))
    flat = tw.random_params(spec, 2)
    T, B = 4, 6
    roll = tw.random_rollout(spec, flat, T, B, 3)
    envs = np.array([-1, 4, 2, B, 0], np.int32)
    w = torch.from_numpy(flat.astype(np.float64)).requires_grad_(True)
    total, stats, _ = tw.loss(spec, w, roll, envs, ent_coef=0.01)
    total.backward()
    # by hand: the valid columns' h rows, zeros for the other two, every buffer zero there
    u = torch.from_numpy(flat.astype(np.float64)).requires_grad_(True)
    p = tw.views(spec, u)
    good = np.array([4, 2, 0])
    r = {k: tw._t(v, torch.float64) for k, v in roll.items()}
    hs, _ = tw.unroll(spec, p, r["obs"][:T], r["episode_start"][:T], r["lstm_state0"], torch.as_tensor(good))
    cols = [None, 0, 1, None, 2]

    def place(x):                                               # [T, 3, ...] -> [T, 5, ...] with zeros in the columns without an env
        z = torch.zeros_like(x[:, 0])
        return torch.stack([z if c is None else x[:, c] for c in cols], dim=1)
    h_pi, h_vf = place(hs[0]).reshape(-1, 7), place(hs[1]).reshape(-1, 7)
    mean = tw._mlp(p, "policy_net", "action_net", h_pi, "tanh")
    V = tw._mlp(p, "value_net", "value_net", h_vf, "tanh")[:, 0]
    raw, lpo, A, ret = (place(r[k][:, good]).reshape((T * 5,) + r[k].shape[2:]) for k in ("raw", "logp", "advantage", "returns"))
    ls = p["log_std"]
    z = (raw - mean) / torch.exp(ls)
    ratio = torch.exp((-0.5 * z * z - ls - tw.HALF_LOG_2PI).sum(1) - lpo)
    assert A.numel() == 20 and int((A == 0).sum()) >= 8
    A = (A - A.mean()) / (A.std() + 1e-8)
    by_hand = (-torch.min(ratio * A, torch.clamp(ratio, 0.8, 1.2) * A).mean() + 0.5 * ((ret - V) ** 2).mean()
               - 0.01 * (0.5 + tw.HALF_LOG_2PI + ls).sum())
    by_hand.backward()
    assert abs(float(total.detach()) - float(by_hand.detach())) < 1e-14
    np.testing.assert_allclose(w.grad.numpy(), u.grad.numpy(), rtol=0, atol=1e-14)
    # the other envs' data and env 0's (which stands in for the index) do not matter to such a column; the valid ones do
    other = {k: v.copy() for k, v in roll.items()}
    for k in ("obs", "raw", "logp", "advantage", "returns"):
        other[k][:, [1, 3, 5]] += 1.0
    g0 = tw.loss_and_grad(spec, flat, roll, envs)[2]
    assert np.array_equal(g0, tw.loss_and_grad(spec, flat, other, envs)[2])
    only_invalid = tw.loss_and_grad(spec, flat, roll, np.array([-1, B], np.int32))[2]
    n_lstm = 2 * 4 * 7 * (5 + 7 + 2)
    assert np.all(only_invalid[:n_lstm] == 0.0) and np.abs(only_invalid[n_lstm:]).max() > 0 and np.all(np.isfinite(only_invalid))
