"""CPU checks of behaviour cloning into a recurrent policy (windgym_amd/recurrent_imitation.py): the ctypes mirror and the exports,
the twin tests/lstm_bc_twin.py itself — where its two parents meet, against central differences, the no-env column rule — the
minibatch rule, and the refusals that need no device."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import imitation_twin as it
import lstm_bc_twin as bt
import lstm_bptt_twin as tw
from helpers import c_layout
from recurrent_ppo_cases import make_spec
from windgym_amd.recurrent_imitation import RecurrentBehaviorCloning


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_matches_the_header(tmp_path):
    from windgym_amd import binding
    cls = binding.CLstmBcBatch
    fields = [f[0] for f in cls._fields_]
    assert fields == ["obs", "target", "returns", "episode_start", "lstm_state0", "T", "B"]
    out = c_layout("wg_lstm_bc_batch", fields, tmp_path)
    assert out["sizeof"] == C.sizeof(cls) == 48
    assert all(out[f] == getattr(cls, f).offset for f in fields)
    assert {"wg_lstm_bc_grad", "wg_lstm_bc_update"} <= set(binding.ABI_SYMBOLS)


def test_the_package_exports_the_trainer_and_the_optimiser_has_the_entries():
    import windgym_amd
    from windgym_amd.ppo import Trainer
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    assert windgym_amd.RecurrentBehaviorCloning is RecurrentBehaviorCloning and issubclass(RecurrentBehaviorCloning, Trainer)
    assert callable(RecurrentPPOOptimizer.bc_grad) and callable(RecurrentPPOOptimizer.bc_update)
    assert "log_std" in RecurrentBehaviorCloning.__doc__ and "multiple of ``n_steps``" in RecurrentBehaviorCloning.__doc__


# ---- the twin ----------------------------------------------------------------------------------------------------------------------------
def _case(shared, T=4, B=7, n_in=5, H=6, seed=0):
    spec = make_spec(n_in, H, shared, hidden_pi=(8,), hidden_vf=(8,), n_out=2)
    flat = tw.random_params(spec, seed=seed, dtype=np.float64)
    return spec, flat, bt.random_rollout(spec, flat, T, B, seed=seed + 1)


@pytest.mark.parametrize("with_returns", [False, True], ids=["actor", "critic"])
@pytest.mark.parametrize("loss", ["mse", "nll"])
@pytest.mark.parametrize("shared", [False, True], ids=["two-lstms", "shared-lstm"])
def test_at_one_fresh_step_the_twin_is_bc_loss_on_the_cell_of_zeros(shared, loss, with_returns):
    """T = 1 with every row fresh: h = cell(x, 0, 0) whatever lstm_state0 holds, and the loss over the n = Bm rows is imitation_twin's on
    those h rows — where the two parents must agree.  Both sides are float64 autograd of the same expression up to the order of a few
    sums: 1e-12 relative to max(1, |g|) is four decades above their rounding."""
    spec, flat, roll = _case(shared, T=1)
    roll["episode_start"][0] = 1
    roll["lstm_state0"][:] = np.nan
    if not with_returns:
        roll["returns"] = None
    envs = np.array([4, 0, 6, 2, 5])
    kw = dict(loss=loss, ent_coef=0.01, vf_coef=0.5)
    total, stats, g = bt.loss_and_grad(spec, flat, roll, envs, **kw)
    # the other parent, by hand: the cell on zeros, then imitation_twin.bc_loss_and_grad per head on those rows
    w = torch.tensor(flat, dtype=torch.float64, requires_grad=True)
    p = tw.views(spec, w)
    hs = []
    for net in tw.NETS[:tw.nets(spec)]:
        z = p[f"{net}.bias_ih_l0"] + p[f"{net}.bias_hh_l0"] + torch.from_numpy(roll["obs"][0][envs]).double() @ p[f"{net}.weight_ih_l0"].T
        zi, zf, zg, zo = z.chunk(4, dim=-1)
        hs.append(torch.sigmoid(zo) * torch.tanh(torch.sigmoid(zi) * torch.tanh(zg)))
    mlp = {k: v.detach().numpy() for k, v in p.items() if not k.startswith("lstm_")}
    ids = np.arange(len(envs))
    ref_total, ref_grads, ref_stats = it.bc_loss_and_grad(mlp, hs[0].detach().numpy(), roll["labels"][0][envs], None, ids, **kw)
    if with_returns:
        v = it.bc_loss_and_grad(mlp, hs[-1].detach().numpy(), roll["labels"][0][envs], roll["returns"][0][envs], ids, **kw)
        ref_total += kw["vf_coef"] * v[2]["v_loss"]
        for k in ref_grads:
            if "value_net" in k:
                ref_grads[k] = v[1][k]
        ref_stats.update(v_loss=v[2]["v_loss"], loss=ref_total)
    assert abs(total - ref_total) <= 1e-12 * max(1.0, abs(ref_total))
    for k in bt.STATS:
        assert abs(stats[k] - ref_stats[k]) <= 1e-12 * max(1.0, abs(ref_stats[k])), k
    got = tw.views(spec, g)
    for k, r in ref_grads.items():
        assert np.all(np.abs(got[k] - r) <= 1e-12 * np.maximum(1.0, np.abs(r))), k
    assert not got["lstm_actor.weight_hh_l0"].any() and got["lstm_actor.weight_ih_l0"].any()      # every row fresh: W_hh sees h = 0
    if loss == "mse":
        assert not got["log_std"].any()
    critic = [k for k in got if "value_net" in k or k.startswith("lstm_critic")]
    assert critic and all(bool(got[k].any()) == (with_returns and not k.endswith("lstm_critic.weight_hh_l0")) for k in critic)


@pytest.mark.parametrize("with_returns", [False, True], ids=["actor", "critic"])
@pytest.mark.parametrize("loss", ["mse", "nll"])
@pytest.mark.parametrize("shared", [False, True], ids=["two-lstms", "shared-lstm"])
def test_autograd_twin_vs_finite_differences(shared, loss, with_returns):
    """Central differences with h = 1e-6 of a float64 loss of order 1 (test_imitation.py's reasoning: rounding 6e-11 per term,
    truncation 1e-12): 1e-7 * max(1, |g|), on every eleventh entry of the flat vector and the last (log_std)."""
    spec, flat, roll = _case(shared, T=4)
    roll["episode_start"][:, :] = 0
    roll["episode_start"][0, ::2] = 1
    roll["episode_start"][2, 1] = roll["episode_start"][3, 1] = roll["episode_start"][3, 4] = 1
    if not with_returns:
        roll["returns"] = None
    envs = np.array([3, 1, -1, 4, 6, 7, 0])                                # one entry below and one above the rollout
    kw = dict(loss=loss, ent_coef=0.01, vf_coef=0.5)
    total, stats, g = bt.loss_and_grad(spec, flat, roll, envs, **kw)
    assert stats["loss"] == total and np.isfinite(total)
    index = np.unique(np.concatenate([np.arange(0, len(flat), 11), [len(flat) - 2, len(flat) - 1]]))
    fd = bt.finite_difference_grad(spec, flat, roll, envs, index, **kw)
    assert np.all(np.abs(fd - g[index]) <= 1e-7 * np.maximum(1.0, np.abs(g[index]))), np.abs(fd - g[index]).max()
    got = tw.views(spec, g)
    assert got["lstm_actor.weight_hh_l0"].any() and got["action_net.weight"].any()
    assert bool(got["log_std"].any()) == (loss == "nll")
    critic = [k for k in got if "value_net" in k or k.startswith("lstm_critic")]
    assert all(bool(got[k].any()) == with_returns for k in critic)


def test_a_column_without_an_env_counts_in_n_and_reads_nothing():
    spec, flat, roll = _case(False, T=3)
    kw = dict(loss="nll", ent_coef=0.0, vf_coef=0.5)
    a = bt.loss_and_grad(spec, flat, roll, np.array([0, 1, 2, 3]), **kw)
    b = bt.loss_and_grad(spec, flat, roll, np.array([0, 1, -5, 2, 3, 7, 99, 100]), **kw)
    # the four columns without an env are h = 0 rows with target = returns = 0: the same rows whatever the entry, and nothing of the
    # LSTM's gradient comes from them — half of it is left, since every mean now divides by twice the rows
    n_lstm = 2 * 4 * spec["H"] * (spec["n_in"] + spec["H"] + 2)
    assert np.allclose(b[2][:n_lstm], a[2][:n_lstm] / 2.0, rtol=1e-12, atol=0.0) and a[2][:n_lstm].any()
    zero = dict(roll, labels=np.zeros_like(roll["labels"]), returns=np.zeros_like(roll["returns"]),
                lstm_state0=np.zeros_like(roll["lstm_state0"]))
    flat0 = flat.copy()
    for name, sl in _slices(spec):
        if name.startswith("lstm_"):
            flat0[sl] = 0.0                                               # an LSTM of zeros from the zero state: h = 0 on every row
    c = bt.loss(spec, torch.tensor(flat0), zero, np.array([0, 1]), **kw)[1]
    d = bt.loss(spec, torch.tensor(flat), roll, np.array([-1, 7]), **kw)[1]
    assert all(abs(c[k] - d[k]) <= 1e-15 * max(1.0, abs(c[k])) for k in bt.STATS)
    assert b[1]["entropy"] == a[1]["entropy"]


def _slices(spec):
    out, o = [], 0
    for name, shape in tw.layout(spec):
        n = int(np.prod(shape))
        out.append((name, slice(o, o + n)))
        o += n
    return out


def test_train_descends_and_walks_the_documented_minibatches():
    spec, flat, roll = _case(True, T=4, B=7)
    perms = np.stack([np.random.default_rng(e).permutation(7) for e in range(6)])
    w, log = bt.train(spec, flat, roll, perms, 3, lr=3e-3, loss="mse")
    # (the log's entries are losses of DIFFERENT minibatches: descent is judged on the whole rollout, before and after)
    before, after = (bt.loss_value(spec, x, roll, np.arange(7), loss="mse") for x in (flat, w))
    assert len(log) == 6 * 3 and log[0]["mse"] == log[0]["loss"] and after < before and np.abs(w - flat).max() > 1e-3
    assert np.array_equal(tw.views(spec, w)["log_std"], tw.views(spec, flat)["log_std"])          # MSE: its gradient is exactly 0


# ---- the trainer's device-free side ----------------------------------------------------------------------------------------------------
def test_batch_size_is_whole_sequences():
    from windgym_amd.recurrent_ppo import envs_per_minibatch
    for bs, T, B in ((None, 8, 10), (16, 8, 10), (80, 8, 10), (8, 8, 1)):
        assert envs_per_minibatch(bs, T, B) == tw.envs_per_batch(bs, T, B)
    for bs in (20, 4):
        with pytest.raises(ValueError, match="multiple of n_steps"):
            tw.envs_per_batch(bs, 8, 10)
        with pytest.raises(ValueError, match="multiple of n_steps"):
            envs_per_minibatch(bs, 8, 10)


def test_refusals_need_no_device():
    from windgym_amd.imitation import BehaviorCloning
    env = dict(batch=types.SimpleNamespace(obs_dim=9), rollout=None, num_envs=4, n_turb=2)
    ok = types.SimpleNamespace(as_torch=True, **env)
    lstm = types.SimpleNamespace(recurrent=True)
    with pytest.raises(ValueError, match="needs a recurrent policy"):
        RecurrentBehaviorCloning(types.SimpleNamespace(recurrent=False), ok)
    with pytest.raises(ValueError, match="only 'MlpLstmPolicy'"):
        RecurrentBehaviorCloning("MlpPolicy", ok)
    with pytest.raises(NotImplementedError, match="WindFarmVecEnvMulti"):
        RecurrentBehaviorCloning(lstm, types.SimpleNamespace(as_torch=True, possible_agents=["a"], **env))
    with pytest.raises(NotImplementedError, match="population"):
        RecurrentBehaviorCloning(lstm, types.SimpleNamespace(as_torch=True, population=object(), **env))
    with pytest.raises(ValueError, match="as_torch"):
        RecurrentBehaviorCloning(lstm, types.SimpleNamespace(as_torch=False, **env))
    with pytest.raises(ValueError, match="loss must be one of"):
        RecurrentBehaviorCloning(lstm, ok, loss="huber")
    with pytest.raises(ValueError, match="expert must be one of"):
        RecurrentBehaviorCloning(lstm, ok, expert="floris")
    with pytest.raises(ValueError, match="expert must be one of"):
        RecurrentBehaviorCloning(lstm, ok, expert=object())
    for kw in (dict(vf_coef=-0.5), dict(ent_coef=-1e-3), dict(vf_coef=float("nan"))):
        with pytest.raises(ValueError, match="vf_coef and ent_coef must be >= 0"):
            RecurrentBehaviorCloning(lstm, ok, **kw)
    with pytest.raises(ValueError, match="multiple of n_steps"):
        RecurrentBehaviorCloning(lstm, ok, n_steps=8, batch_size=20)
    with pytest.raises(ValueError, match="policy_kwargs only applies"):
        RecurrentBehaviorCloning(lstm, ok, policy_kwargs=dict(lstm_hidden_size=32))
    with pytest.raises(NotImplementedError, match="recurrent"):            # the MLP trainer still refuses one
        BehaviorCloning(lstm, ok)
