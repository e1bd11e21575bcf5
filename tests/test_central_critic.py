"""CPU-side checks of the centralised-critic path: the flat layout of a split policy (a critic with its own input width), the
checkpoint reader, the ctypes mirror of wg_ppo_batch_shared, and the float64 references the GPU tests lean on, pinned by
themselves (oracle/ppo_oracle.py: the shared forms against finite differences and against the plain ones, which call them)."""
import ctypes as C
import io
import zipfile

import numpy as np
import pytest

from helpers import c_layout
from oracle import ppo_oracle as oo
from windgym_amd import binding
from windgym_amd.policy import critic_width, make_desc, n_params, pack_params, param_layout, read_sb3_zip, unpack_params


def _random_tensors(desc, seed=0):
    rng = np.random.default_rng(seed)
    return {name: rng.standard_normal(shape).astype(np.float32) for name, shape in param_layout(desc)}


def test_layout_with_a_critic_of_its_own_width():
    desc = make_desc(5, 1, (8, 4), (6,), n_in_vf=23)
    lay = dict(param_layout(desc))
    assert [n for n, _ in param_layout(desc)] == [n for n, _ in param_layout(make_desc(5, 1, (8, 4), (6,)))]      # SB3's names, same order
    assert lay["mlp_extractor.policy_net.0.weight"] == (8, 5) and lay["mlp_extractor.value_net.0.weight"] == (6, 23)
    assert lay["value_net.weight"] == (1, 6) and critic_width(desc) == 23
    assert n_params(desc) == n_params(make_desc(5, 1, (8, 4), (6,))) + 6 * (23 - 5)
    # no hidden critic layer: the head itself is [1][n_in_vf]
    d0 = make_desc(5, 2, (8,), (), n_in_vf=23)
    assert dict(param_layout(d0))["value_net.weight"] == (1, 23)
    t = _random_tensors(desc, 1)
    flat = pack_params(desc, t)
    assert flat.shape == (n_params(desc),)
    back = unpack_params(desc, flat)
    assert all(np.array_equal(back[k], t[k]) for k in t)
    # the critic's first W sits where it sat, [h][n_in_vf] row-major, right behind the actor's head
    o = 8 * 5 + 8 + 4 * 8 + 4 + 1 * 4 + 1
    assert np.array_equal(flat[o:o + 6 * 23].reshape(6, 23), t["mlp_extractor.value_net.0.weight"])
    with pytest.raises(ValueError, match="shape"):
        pack_params(make_desc(5, 1, (8, 4), (6,)), t)                        # the equal-width layout does not take these tensors


def test_a_desc_without_the_key_is_todays():
    new = make_desc(7, 3, (16,), (16, 8))
    old = {k: v for k, v in new.items() if k != "n_in_vf"}                   # a dict written before the key existed
    assert new["n_in_vf"] is None and critic_width(old) == critic_width(new) == 7
    assert param_layout(old) == param_layout(new) and n_params(old) == n_params(new)
    assert param_layout(make_desc(7, 3, (16,), (16, 8), n_in_vf=7)) == param_layout(new)
    t = _random_tensors(new, 2)
    assert np.array_equal(pack_params(old, t), pack_params(new, t))
    with pytest.raises(ValueError, match="critic"):
        make_desc(7, 3, (16,), None, n_in_vf=9)                              # no critic: nothing n_in_vf could be the width of
    with pytest.raises(ValueError, match=">= 1"):
        make_desc(7, 3, (16,), (4,), n_in_vf=0)


@pytest.mark.parametrize("hidden_vf", [(8, 4), ()])
def test_read_sb3_zip_reports_a_wider_critic(tmp_path, hidden_vf):
    import torch
    desc = make_desc(6, 1, (8,), hidden_vf, n_in_vf=40)
    sd = _random_tensors(desc, 3)
    b = io.BytesIO()
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, b)
    path = tmp_path / "split.zip"
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", b.getvalue())
    d2, t2 = read_sb3_zip(path)
    assert d2 == desc and d2["n_in_vf"] == 40 and all(np.array_equal(t2[k], sd[k]) for k in sd)
    # the equal-width file reads exactly as before: the key is there and says "the actor's"
    same = make_desc(6, 1, (8,), hidden_vf)
    b = io.BytesIO()
    torch.save({k: torch.from_numpy(v) for k, v in _random_tensors(same, 4).items()}, b)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", b.getvalue())
    assert read_sb3_zip(path)[0] == same and read_sb3_zip(path)[0]["n_in_vf"] is None


def test_shared_batch_struct_and_symbols_match_the_header(tmp_path):
    for name in ("wg_policy_create_vf", "wg_ppo_grad_shared", "wg_ppo_update_shared"):
        assert name in binding.ABI_SYMBOLS
    fields = {"rows": "rows", "rows.n_rows": None, "obs_vf": "obs_vf", "agents": "agents"}
    out = c_layout("wg_ppo_batch_shared", fields, tmp_path)
    S = binding.CPpoBatchShared
    assert out["sizeof"] == C.sizeof(S)
    assert out["rows"] == S.rows.offset and out["obs_vf"] == S.obs_vf.offset and out["agents"] == S.agents.offset
    assert out["rows.n_rows"] == S.rows.offset + binding.CPpoBatch.n_rows.offset


# ----------------------------------------------------------------------------------------------------------------------
# the float64 reference, pinned
# ----------------------------------------------------------------------------------------------------------------------
def _tiny(agents, seed=0, n_env=6):
    rng = np.random.default_rng(seed)
    desc = make_desc(3, 2, (4,), (3,), n_in_vf=5)
    params = {k: 0.5 * rng.standard_normal(s) for k, s in param_layout(desc)}
    n = n_env * agents
    obs, obs_vf = rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n_env, 5))
    raw, lpo = rng.standard_normal((n, 2)), -2.0 + 0.3 * rng.standard_normal(n)
    adv, ret = rng.standard_normal(n_env), rng.standard_normal(n_env)
    return params, (obs, obs_vf, raw, lpo, adv, ret)


@pytest.mark.parametrize("agents,normalize", [(1, True), (3, True), (3, False)])
def test_reference_gradient_against_central_differences(agents, normalize):
    params, arrays = _tiny(agents, seed=agents)
    n = 6 * agents
    # env row 2 through all of its agents and once more, an entry outside the batch, the rest in scrambled order
    ids = np.concatenate([np.arange(agents) + 2 * agents, [2 * agents, n + 3, -1], np.random.default_rng(1).permutation(n)[:7]])
    kw = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=normalize)
    total, grads, stats, _ = oo.shared_loss_and_grad(params, *arrays, ids, agents, **kw)
    assert abs(total - oo.shared_loss_value(params, *arrays, ids, agents, **kw)) <= 1e-12 and abs(total - stats["loss"]) <= 1e-12
    fd = oo.finite_difference_grad(params, *arrays, ids, agents, **kw)
    for k in params:
        assert np.abs(fd[k] - grads[k]).max() <= 1e-6 * max(1.0, np.abs(grads[k]).max()), k
    assert any(np.abs(grads[k]).max() > 1e-3 for k in grads if "value_net" in k)
    assert any(np.abs(grads[k]).max() > 1e-3 for k in grads if "policy_net" in k)


def test_reference_is_the_plain_loss_with_one_agent_on_one_stream():
    """agents = 1, the critic on the actor's rows, no entry out of range: oracle/ppo_oracle.py's loss, statistics and gradient."""
    rng = np.random.default_rng(5)
    desc = make_desc(4, 2, (5,), (5,))
    params = {k: 0.5 * rng.standard_normal(s) for k, s in param_layout(desc)}
    n = 40
    obs, raw, lpo = rng.uniform(-1, 1, (n, 4)), rng.standard_normal((n, 2)), -2.0 + 0.3 * rng.standard_normal(n)
    adv, ret = rng.standard_normal(n), rng.standard_normal(n)
    ids = rng.permutation(n)[:25]
    for norm in (True, False):
        kw = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=norm)
        total, grads, stats, _ = oo.shared_loss_and_grad(params, obs, obs, raw, lpo, adv, ret, ids, 1, **kw)
        t0, g0, s0, _ = oo.loss_and_grad(params, obs[ids], raw[ids], lpo[ids], adv[ids], ret[ids], **kw)
        assert abs(total - t0) <= 1e-12 and all(abs(stats[k] - s0[k]) <= 1e-12 for k in s0)
        assert all(np.abs(grads[k] - g0[k]).max() <= 1e-12 for k in g0)
        # the plain forms ARE the shared ones on every row once, one agent per env, the critic on the actor's rows: exactly
        import torch
        tp = {k: torch.tensor(v) for k, v in params.items()}
        rows = [torch.tensor(x) for x in (obs, raw, lpo, adv, ret)]
        plain, shared = oo.loss(tp, *rows, **kw), oo.shared_loss(tp, rows[0], *rows, np.arange(n), 1, **kw)
        assert plain[0] == shared[0] and plain[1] == shared[1] and torch.equal(plain[2], shared[2])


def test_an_env_row_drawn_through_two_agents_counts_twice():
    params, arrays = _tiny(3, seed=9)
    kw = dict(vf_coef=1.0, normalize_advantage=False)
    one = oo.shared_loss_and_grad(params, *arrays, [6], 3, **kw)[2]["v_loss"]            # env row 2 through agent 0
    other = oo.shared_loss_and_grad(params, *arrays, [0], 3, **kw)[2]["v_loss"]          # env row 0
    both = oo.shared_loss_and_grad(params, *arrays, [6, 7, 0], 3, **kw)[2]["v_loss"]     # env row 2 twice, env row 0 once
    assert abs(both - (2 * one + other) / 3) <= 1e-12


def test_central_advantages_are_the_per_agent_recurrence_with_a_shared_value():
    rng = np.random.default_rng(3)
    T, B, A = 17, 5, 9
    r, v, fv = (rng.standard_normal((T, B)) for _ in range(3))
    tr = rng.uniform(size=(T, B)) < 0.15
    adv, ret = oo.gae(r, v, fv, tr, 0.99, 0.95)
    bc = lambda x: np.repeat(x[:, :, None], A, axis=2)                       # noqa: E731
    sa, sr = oo.gae_shared(r, bc(v), bc(fv), tr, 0.99, 0.95)
    assert np.array_equal(sa, bc(adv)) and np.array_equal(sr, bc(ret))
    # wg_gae is wg_gae_shared with one agent per env, and so are their references (recurrence and brute force): exactly
    for plain, shared in ((oo.gae, oo.gae_shared), (oo.gae_brute, oo.gae_shared_brute)):
        one = shared(r, v[..., None], fv[..., None], tr, 0.99, 0.95)
        assert all(np.array_equal(x, y[..., 0]) for x, y in zip(plain(r, v, fv, tr, 0.99, 0.95), one))


def test_tile_rows_with_the_critics_own_width():
    """Pins a TEST HELPER, not the library: ``ppo_oracle.tile_rows`` restates wg_ppo.h's LDS map in Python (the GPU gradient test
    sizes its ragged and out-of-range index cases by it) and is held here to its own default (the actor's width) at equal widths and
    to hand-computed values.  The library's own R is not exposed; a wrong per-net map in wg_ppo.hip is caught BY VALUE on the GPU, where
    ``n_in`` = 2 beside ``n_in_vf`` = 2048 and the reverse would overflow the observation chunk and corrupt the gradient."""
    for n_in, hidden, hidden_vf, n_out in ((32, (64, 64), (64, 64), 16), (256, (256,) * 4, (256,) * 4, 16), (2048, (256, 256), (64,), 4)):
        assert oo.tile_rows(n_in, n_out, hidden, hidden_vf, n_in_vf=n_in) == oo.tile_rows(n_in, n_out, hidden, hidden_vf)
    # each net's map counts its OWN input chunk: a wide critic beside a narrow actor can halve the tile, and the reverse
    R = lambda n_in, n_in_vf, *net: oo.tile_rows(n_in, *net, n_in_vf=n_in_vf)[0]                # noqa: E731
    assert R(2, 2, 1, (64,), (64, 64)) == 32 and R(2, 2048, 1, (64,), (64, 64)) == 16
    assert R(2048, 2, 1, (64, 64), (64,)) == 16 and R(2048, 2, 4, (256, 256), (64,)) == 8
    assert oo.lds_floats(300, [8, 1], 32) == oo.lds_floats(256, [8, 1], 32)


def test_central_on_a_one_turbine_farm_says_so():
    """obs_dim == obs_len (one agent per env): central mode cannot be told from the per-agent one by the critic's width, and
    ``PPO(..., critic="central")`` says that, before it builds anything — not that the mode "contradicts the policy"."""
    from types import SimpleNamespace
    from windgym_amd.ppo import PPO
    one = SimpleNamespace(possible_agents=["turbine_0"], n_turb=1, num_envs=4, obs_len=6, batch=SimpleNamespace(obs_dim=6))
    with pytest.raises(ValueError, match="more than one turbine.*nothing to centralise"):
        PPO("MlpPolicy", one, n_steps=4, critic="central")
    single = SimpleNamespace(possible_agents=None, n_turb=3, num_envs=4, batch=SimpleNamespace(obs_dim=18))
    with pytest.raises(ValueError, match="needs a WindFarmVecEnvMulti.*nothing to centralise"):
        PPO("MlpPolicy", single, n_steps=4, critic="central")
