"""CPU test of the supervised head's limit cases (tests/bc_cases.py for the MLP policy, the bc_* half of tests/recurrent_ppo_cases.py for
the recurrent one): every built case meets, on the twins alone, the conditions that make it a test of the device — a finite reference,
a gradient that is nonzero on every tensor the case does not declare zero (and exactly zero, in float64 and float32, where it does),
e32 > 0, and the degeneracy its name promises."""
import numpy as np
import pytest

import bc_cases as bc
import lstm_bptt_twin as tw
import recurrent_ppo_cases as rc


# ---- the MLP policy's loss-head edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,loss", bc.CASES, ids=[f"{e}-{l}" for e, l in bc.CASES])
def test_mlp_edge_is_a_test(name, loss):
    case, (grads, stats) = bc.edge(name, loss)
    n_in, hidden, n_out = case.shape
    assert len(case.rows) == bc.N_ROWS and case.obs.shape == (bc.TOTAL, n_in) and case.target.shape == (bc.TOTAL, n_out)
    assert all(np.array_equal(v, v.astype(np.float32)) for v in case.sd.values())          # the device can hold these parameters
    assert all(np.isfinite(v) for v in stats.values()) and stats["v_loss"] > 0
    zero = bc.zero_tensors(name, loss)
    assert set(zero) <= set(grads)
    for k, g in grads.items():
        assert np.all(np.isfinite(g)), k
        assert np.all(g == 0.0) if k in zero else np.abs(g).max() > 0, k
    z = bc.z_scores(case)
    if name == "log_std_spread":
        assert len(np.unique(case.sd["log_std"])) == n_out == 16 and case.sd["log_std"].min() == -3.0 and case.sd["log_std"].max() == 1.5
    elif name == "vf_coef_0":
        assert case.kw["vf_coef"] == 0.0 and abs(stats["loss"] - (stats["mse"] if loss == "mse" else stats["nll"] - 0.01 * stats["entropy"])) < 1e-12
    elif name == "ent_coef_0":
        assert case.kw["ent_coef"] == 0.0 and stats["loss"] == stats["nll"] + 0.5 * stats["v_loss"]
    elif name == "saturated_tanh":
        assert np.mean(np.abs(np.tanh(bc.first_hidden(case, bc.PRE))) > 1 - 1e-7) > 0.9
    elif name == "dead_relu_layer":
        assert case.activation == "relu" and bc.first_hidden(case, bc.PRE).max() < 0 and bc.first_hidden(case, bc.PRE_VF).max() < 0
        all_rows = case.obs.astype(np.float64) @ case.sd[bc.PRE + "0.weight"].T + case.sd[bc.PRE + "0.bias"]
        assert all_rows.max() < 0                                        # fires nowhere, on no row of the batch
    elif name == "repeated_rows":
        assert len(np.unique(case.rows)) == 40
    elif name == "far_targets":
        assert np.mean(np.abs(z) > 40.0) > 0.5 and np.abs(z).max() < 60.0 and stats["nll"] > 0.5 * 40.0 ** 2 * n_out * 0.5
    elif name == "n_out_1":
        assert case.shape == (7, (33,), 1)
    elif name == "targets_are_the_means":
        assert np.abs(z * np.exp(case.sd["log_std"])).max() <= 2.0 ** -23 and stats["mse"] < 1e-14      # half an ulp of |mean| < 2
        if loss == "nll":                                                # d(-logp) / d log_std = 1 - z^2 per row: 1 at the mean
            assert np.abs(grads["log_std"] - (1.0 - 0.01)).max() < 1e-10


# ---- the recurrent policy's cases under the supervised head ---------------------------------------------------------------------------
def _bc_conditions(built, ref, zero):
    spec, flat, roll, envs, kw = built
    assert np.all(np.isfinite(ref.grad)) and np.all(np.isfinite(ref.grad32)) and all(np.isfinite(v) for v in ref.stats.values())
    assert sum(s.stop - s.start for _, s in ref.slices) == ref.grad.size == tw.n_params(spec)
    assert ref.d32.max() > 0                                            # e32 > 0: the bar max(4 e32, ...) has its first term
    for name, sl in ref.slices:
        if zero(name):
            assert np.all(ref.grad[sl] == 0.0) and np.all(ref.grad32[sl] == 0.0), name
        else:
            assert np.abs(ref.grad[sl]).max() > 0, name
    assert (roll.get("returns") is None) == (ref.stats["v_loss"] == 0.0)


@pytest.mark.parametrize("loss,with_ret", rc.BC_COMBOS)
@pytest.mark.parametrize("i", range(len(rc.ARCH_CASES)), ids=[rc.arch_id(c) for c in rc.ARCH_CASES])
def test_recurrent_arch_case_is_a_test(i, loss, with_ret):
    built, ref = rc.bc_arch(i, loss, with_ret)
    spec, flat, roll, envs, kw = built
    _, flat0, roll0, envs0, _ = rc.build_arch(rc.ARCH_CASES[i])          # the PPO case's parameters, buffers and minibatch
    assert np.array_equal(flat, flat0) and np.array_equal(envs, envs0) and kw == dict(rc.BC_KW, loss=loss)
    assert all(np.array_equal(roll[k], roll0[k]) for k in roll0 if k != "returns" or with_ret)
    assert roll["labels"].shape == roll["raw"].shape and ref.rows == rc.ARCH_CASES[i][2] * rc.ARCH_CASES[i][3]
    _bc_conditions(built, ref, lambda k: rc.bc_is_zero_tensor(None, k, loss, with_ret))


@pytest.mark.parametrize("loss,with_ret", rc.BC_COMBOS)
@pytest.mark.parametrize("name", rc.BC_CELL_EDGES)
def test_recurrent_cell_edge_is_a_test(name, loss, with_ret):
    built, ref = rc.bc_edge(name, loss, with_ret)
    spec, flat, roll, envs, kw = built
    T = roll["labels"].shape[0]
    es = roll["episode_start"][:T]
    _bc_conditions(built, ref, lambda k: rc.bc_is_zero_tensor(name, k, loss, with_ret))
    if name in rc.CELL_EDGES:                                           # the cell is the PPO case's: same parameters, starts and states
        (_, flat0, roll0, envs0, _), _ = rc.edge(name)
        assert np.array_equal(flat, flat0) and np.array_equal(envs, envs0)
        assert all(np.array_equal(roll[k], roll0[k], equal_nan=True) for k in ("obs", "episode_start", "lstm_state0"))
    if name == "all_fresh":
        assert es.all() and np.isnan(roll["lstm_state0"]).all()
    elif name == "none_fresh":
        assert not es.any() and np.abs(roll["lstm_state0"]).min() > 0
    elif name == "vf_coef_0":
        assert kw["vf_coef"] == 0.0 and (not with_ret or ref.stats["v_loss"] > 0)
    elif name == "saturated_gates":
        assert rc.gate_saturation(spec, flat, roll, envs) >= 0.25
    elif name == "long_carry":
        assert (spec["H"], T, len(envs)) == (64, 128, 3) and not es.any()
    elif name == "large_c0":
        carried = roll["episode_start"][0] == 0
        assert carried.any() and np.abs(roll["lstm_state0"][:, 1][:, carried]).max() > 10.0
    elif name == "start_on_last_step_only":
        assert not es[:T - 1].any() and es[T - 1].any() and not es[T - 1].all()
    elif name == "labels_are_the_means":
        # labels = the twin's means to float32 rounding: the error is below an ulp of the means, the actor's path small and not zero
        assert 0.0 < ref.stats["mean_abs_err"] < 2.0 ** -23 and ref.stats["mse"] < 1e-13
        if loss == "nll":
            sl = dict(ref.slices)["log_std"]
            assert np.abs(ref.grad[sl] - (1.0 - kw["ent_coef"])).max() < 1e-10
