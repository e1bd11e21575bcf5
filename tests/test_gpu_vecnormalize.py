"""VecNormalize on the device (wg_norm.hip, wg_rollout_norm, normalize.py) against the float64 twin of tests/vecnormalize_twin.py
and against its own documented loops.  Shapes sit at the edges of the 64-row chunks and 64-feature tiles of the two observation
kernels, not at the workload's size; every figure a bar is held against is printed before the assertion."""
import copy
import os

import numpy as np
import pytest

from rl_helpers import _torch, _venv, dev, make
from vecnormalize_twin import VecNormalizeTwin

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23          # both sides compute in float64 and round to float32 once; a different summation order can move that rounding by one ulp


def _norm(n_obs, n_envs, **kw):
    from windgym_amd.binding import Norm
    return Norm(n_obs, n_envs, 0, **kw)


def _one_ulp(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: worst |got - want| / max(1, |want|) = {err.max():.3e} (bar {ULP:.3e})")
    assert err.max() <= ULP, what


def _rel(got, want, what, rtol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / np.abs(want)
    print(f"{what}: worst relative error {np.max(err):.3e} (bar {rtol:.0e})")
    assert np.all(np.abs(got - want) <= rtol * np.abs(want)), what


def _obs_batches(rows, O, n, seed, clip_scale):
    """``n`` batches uniform in [-1, 1]; with O >= 2 feature 0 is constant (var -> 0 under epsilon) and the last feature is scaled
    by ``clip_scale`` in about one row of fifty, so that values land beyond the clip"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (n, rows, O)).astype(np.float32)
    if O >= 2:
        x[..., 0] = np.float32(0.3)
        x[..., -1] *= np.where(rng.uniform(size=(n, rows)) < 0.02, clip_scale, 1.0).astype(np.float32)
    return x


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, O", [(1, 1), (5, 33), (50, 64), (257, 65), (64, 2048), (4096, 32)])
def test_obs_half_matches_the_twin(rows, O):
    """20 consecutive wg_norm_obs updates with final rows: normalised rows within one float32 ulp, clipped entries bit for bit,
    count exact, mean and var to rtol 1e-12."""
    t = _torch()
    n = _norm(O, rows)
    twin = VecNormalizeTwin(O, rows)
    obs = _obs_batches(rows, O, 20, seed=rows + O, clip_scale=1000.0)
    extra = _obs_batches(rows, O, 20, seed=rows + O + 1, clip_scale=1.0)
    if O >= 2:                                                  # the final rows: every entry of the last feature beyond the clip
        extra[..., -1] = np.where(extra[..., -1] < 0, np.float32(-1e6), np.float32(1e6))
    out, eout = t.zeros((rows, O), device="cuda"), t.zeros((rows, O), device="cuda")
    worst, clipped = 0.0, 0
    for k in range(20):
        (x, e) = dev(obs[k], extra[k])
        n.obs(x, out, e, eout)
        want, ewant = twin.obs_half(obs[k], extra[k])
        for got, w in ((out.cpu().numpy(), want), (eout.cpu().numpy(), ewant)):
            err = np.abs(got.astype(np.float64) - w) / np.maximum(1.0, np.abs(w))
            worst = max(worst, float(err.max()))
            at = np.abs(w) == 10.0
            clipped += int(at.sum())
            assert np.array_equal(got[at], w[at])                  # clipped entries: bit for bit
    print(f"rows {rows} x O {O}: worst normalised error / max(1, |want|) = {worst:.3e} (bar {ULP:.3e}); {clipped} clipped entries")
    assert worst <= ULP
    assert O < 2 or clipped >= 20 * rows
    s = n.stats()
    assert s["obs_count"] == twin.obs_rms.count and abs(s["obs_count"] - (1e-4 + 20 * rows)) < 1e-8        # (count grows by 20 additions)
    if O >= 2:
        assert s["obs_var"][0] < 1e-4 / rows                       # the constant feature: only the prior's share is left
    _rel(s["obs_var"], twin.obs_rms.var, "obs var")
    _rel(s["obs_mean"], twin.obs_rms.mean, "obs mean")
    assert s["ret_count"] == 1e-4 and s["ret_var"] == 1.0 and not s["returns"].any()
    n.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, O", [(257, 65), (4096, 32)])
def test_obs_half_is_deterministic_and_rows_are_independent_of_extra(rows, O):
    t = _torch()
    obs = dev(*_obs_batches(rows, O, 4, seed=3, clip_scale=1000.0))
    extra = dev(*_obs_batches(rows, O, 4, seed=4, clip_scale=1e4))
    runs = []
    for with_extra in (True, True, False):
        n = _norm(O, rows)
        outs = []
        for k in range(4):
            out, eout = t.zeros((rows, O), device="cuda"), t.zeros((rows, O), device="cuda")
            n.obs(obs[k], out, *((extra[k], eout) if with_extra else (None, None)))
            outs.append((out, eout))
        runs.append((outs, n.state()))
        n.close()
    (a, sa), (b, sb), (c, sc) = runs
    assert sa == sb == sc
    for k in range(4):
        assert t.equal(a[k][0], b[k][0]) and t.equal(a[k][1], b[k][1]) and t.equal(a[k][0], c[k][0])
        assert not c[k][1].any()


# 3 ------------------------------------------------------------------------------------------------------------------------
def _norm_rollout_equals_the_loop(va, vb, na, nb, p, T, rec=("power_agent", "yaw_agent"), min_trunc=1):
    """na.rollout(p, T) on va == the documented loop of wg_rollout_norm from single calls on the twin (vb, nb): policy.act on the
    normalised row, step, wg_norm_obs — every buffer, both normalised buffers, the handle's state and the wg_norm's, bit for bit."""
    t = _torch()
    B, N = va.num_envs, va.n_turb
    seed, counter0 = int(va._base_seed), vb._policy_steps
    assert va._policy_steps == counter0 and t.equal(na._cur, nb._cur) and na.state() == nb.state()
    out = na.rollout(p, T, record=rec, normalize_reward=False)
    ref = {k: [] for k in ("actions", "raw", "logp", "value", "final_value", "reward", "truncated", "final_obs", "env_final_obs") + tuple(rec)}
    ref["obs"], ref["env_obs"] = [nb._cur.clone()], [vb.batch.obs.clone()]
    for i in range(T):
        a, raw, logp, v = p.act(ref["obs"][-1], counter=counter0 + i, seed=seed, row_offset=0)
        a = a.reshape(B, N).clone()
        ref["actions"].append(a); ref["raw"].append(raw.reshape(B, N).clone())
        ref["logp"].append(logp.reshape(B).clone()); ref["value"].append(v.reshape(B).clone())
        vb.batch.step(a)
        ref["reward"].append(vb.batch.reward.clone()); ref["truncated"].append(vb.batch.truncated.clone())
        ref["env_obs"].append(vb.batch.obs.clone()); ref["env_final_obs"].append(vb.batch.final_obs.clone())
        for name in rec:
            ref[name].append(vb.batch.info(name))
        no, nf = t.empty_like(vb.batch.obs), t.empty_like(vb.batch.obs)
        nb._norm.obs(vb.batch.obs, no, vb.batch.final_obs, nf)
        ref["obs"].append(no); ref["final_obs"].append(nf)
        ref["final_value"].append(p.value(nf).reshape(B).clone())
    vb._policy_steps = counter0 + T
    nb._cur.copy_(ref["obs"][-1])                                 # the twin wrapper keeps the normalised current observation too
    ref["env_reward"] = ref["reward"]
    assert set(out) == set(ref), set(out) ^ set(ref)
    for k, x in ref.items():
        x = t.stack(x)
        assert out[k].shape == x.shape and t.equal(out[k], x), k
    n_trunc = int(out["truncated"].sum())
    assert n_trunc >= min_trunc, n_trunc
    va.batch.check(); vb.batch.check()
    assert va.batch.get_state() == vb.batch.get_state() and na.state() == nb.state()
    # the env's persistent outputs hold its own rows, the wrapper keeps the normalised current observation
    assert t.equal(va.batch.obs, out["env_obs"][T]) and t.equal(va.batch.final_obs, out["env_final_obs"][T - 1])
    assert t.equal(na._cur, out["obs"][T]) and not t.equal(out["obs"], out["env_obs"])
    return out


@pytest.mark.parametrize("B, T, min_trunc", [(48, 300, 1), (50, 40, 0)])
def test_rollout_norm_equals_its_documented_loop(B, T, min_trunc):
    from windgym_amd.normalize import VecNormalize
    t = _torch()
    va, vb = _venv(B), _venv(B)
    na, nb = VecNormalize(va), VecNormalize(vb)
    oa, ob = na.reset(seed=77)[0], nb.reset(seed=77)[0]
    assert t.equal(oa, ob) and na.obs_rms[2] == 1e-4 + B
    twin_count = 1e-4 + B
    for _ in range(T):
        twin_count += B
    p, _ = make(va.batch.obs_dim, (64, 64), va.n_turb)
    out = _norm_rollout_equals_the_loop(va, vb, na, nb, p, T, min_trunc=min_trunc)
    assert na.obs_rms[2] == twin_count                             # one update per step, never one for the final rows
    # a second rollout starts from the kept normalised observation and the moved statistics
    if T <= 40:
        first = out["obs"][T].clone()
        out = _norm_rollout_equals_the_loop(va, vb, na, nb, p, T, min_trunc=0)
        assert t.equal(out["obs"][0], first)
    for x in (na, nb, p, va, vb):
        x.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_halves_switched_off_are_the_identity():
    from windgym_amd.normalize import VecNormalize
    t = _torch()
    B, T = 48, 24
    va, vb, vc = _venv(B), _venv(B), _venv(B)
    p, _ = make(va.batch.obs_dim, (64, 64), va.n_turb)
    plain = vb.rollout(p, T)
    no_obs = VecNormalize(va, norm_obs=False)
    out = no_obs.rollout(p, T)
    for k in plain:
        if k != "reward":
            assert t.equal(out[k], plain[k]), k
    assert t.equal(out["env_reward"], plain["reward"]) and not t.equal(out["reward"], plain["reward"])
    assert t.equal(out["env_obs"], plain["obs"]) and t.equal(out["env_final_obs"], plain["final_obs"])
    assert va.batch.get_state() == vb.batch.get_state()
    assert no_obs.obs_rms[2] == 1e-4 and abs(no_obs.ret_rms[2] - (1e-4 + T * B)) < 1e-8        # obs_rms never moved, ret_rms did
    no_rew = VecNormalize(vc, norm_reward=False)
    out = no_rew.rollout(p, T)
    assert t.equal(out["reward"], out["env_reward"]) and no_rew.ret_rms[2] > 1.0     # the env's own, though ret_rms still moves (rule 4)
    assert not t.equal(out["obs"], out["env_obs"]) and t.equal(out["env_obs"][0], plain["obs"][0])
    for x in (no_obs, no_rew, p, va, vb, vc):
        x.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def _rewards(T, B, seed):
    """Synthetic rewards of a power-like scale, POSITIVE so that neither the returns nor their mean cancel (rtol 1e-12 is then a
    statement about the arithmetic), and truncation flags at a rate of 1 in 20."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 2.0, (T, B)).astype(np.float32) * np.float32(37.0), (rng.uniform(size=(T, B)) < 0.05).astype(np.uint8)


@pytest.mark.parametrize("T, B", [(1, 1), (7, 5), (128, 50), (300, 48)])
def test_reward_half_matches_the_twin(T, B):
    t = _torch()
    n, one = _norm(1, B, gamma=0.97), _norm(1, B, gamma=0.97)
    twin = VecNormalizeTwin(1, B, gamma=0.97)
    n_trunc = 0
    for call in range(3):
        r, tr = _rewards(T, B, seed=10 * T + B + call)
        n_trunc += int(tr.sum())
        rd, td = dev(r, tr)
        got = n.reward(rd, td, t.empty_like(rd))
        want = twin.reward_pass(r, tr)
        _one_ulp(got.cpu().numpy(), want, f"T {T} x B {B}, call {call}: normalised reward")
        s = n.stats()
        assert s["ret_count"] == twin.ret_rms.count and abs(s["ret_count"] - (1e-4 + (call + 1) * T * B)) < 1e-8
        _rel(s["ret_var"], twin.ret_rms.var, "ret var")
        _rel(s["ret_mean"], twin.ret_rms.mean, "ret mean")
        keep = twin.returns != 0.0
        assert np.array_equal(s["returns"] == 0.0, ~keep)
        if keep.any():
            _rel(s["returns"][keep], twin.returns[keep], "returns")
        # T steps in one call == T calls of one step, bit for bit
        step_out = t.stack([one.reward(rd[i], td[i], t.empty_like(rd[i])) for i in range(T)])
        assert t.equal(step_out, got) and one.state() == n.state()
        assert s["obs_count"] == 1e-4
    assert T * B < 100 or n_trunc > 0
    # in place, and clipped where the statistics say so
    r, tr = _rewards(T, B, seed=5)
    r[0, 0] = np.float32(1e9)
    rd, td = dev(r, tr)
    want = twin.reward_pass(r, tr)
    got = n.reward(rd, td, rd)
    assert got.data_ptr() == rd.data_ptr() and float(got[0, 0]) == float(want[0, 0])
    assert T * B < 100 or float(want[0, 0]) == 10.0              # (in a small batch the outlier itself sets the variance)
    _one_ulp(got.cpu().numpy(), want, "in place")
    n.close(); one.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_freeze_state_and_reset_returns():
    from windgym_amd.binding import unpack_norm_state
    from windgym_amd.normalize import VecNormalize
    t = _torch()
    B = 48
    v = _venv(B)
    O = v.batch.obs_dim
    vn = VecNormalize(v, gamma=0.9)
    p, _ = make(O, (64, 64), v.n_turb)
    vn.rollout(p, 8)
    assert vn.returns.all()
    vn.training = False
    before = vn.state()
    out = vn.rollout(p, 300)
    ended = out["truncated"].bool().any(dim=0).cpu().numpy()
    assert ended.any()
    s0, s1 = unpack_norm_state(before, O, B), vn._norm.stats()
    for k in s0:                     # no statistic moves by a bit; of the blob only returns[done] = 0 does (rule 7 holds frozen too)
        assert np.array_equal(s1[k], np.where(ended, 0.0, s0[k]) if k == "returns" else s0[k]), k
    assert vn.state() == before or ended.any() and s0["returns"][ended].any()
    want = vn.normalize_obs(out["env_obs"][7])
    assert t.equal(want, out["obs"][7]) and not t.equal(want, out["env_obs"][7])    # still normalises, with the frozen statistics
    inside = (want.abs() < 10.0).cpu().numpy()                                    # (a clipped entry has no inverse)
    assert np.allclose(vn.unnormalize_obs(want).cpu().numpy()[inside], out["env_obs"][7].cpu().numpy()[inside], atol=1e-5)
    vn.training = True
    # get_state -> a fresh wg_norm -> set_state continues bit-identically
    a, b = _norm(33, 70), _norm(33, 70)
    obs = dev(*_obs_batches(70, 33, 6, seed=9, clip_scale=1000.0))
    r, tr = _rewards(6, 70, seed=2)
    rd, td = dev(r, tr)
    outs = [t.zeros((70, 33), device="cuda") for _ in range(4)]
    for k in range(3):
        a.obs(obs[k], outs[0], obs[k], outs[1]); b.obs(obs[k], outs[2], obs[k], outs[3])
        a.reward(rd[k], td[k], t.empty_like(rd[k])); b.reward(rd[k], td[k], t.empty_like(rd[k]))
    c = _norm(33, 70)
    assert c.state() != b.state()
    c.load_state(b.state())
    assert c.state() == b.state() == a.state()
    for k in range(3, 6):
        a.obs(obs[k], outs[0], obs[k], outs[1]); c.obs(obs[k], outs[2], obs[k], outs[3])
        assert t.equal(outs[0], outs[2]) and t.equal(outs[1], outs[3])
        ra, rc = a.reward(rd[k], td[k], t.empty_like(rd[k])), c.reward(rd[k], td[k], t.empty_like(rd[k]))
        assert t.equal(ra, rc)
    assert a.state() == c.state()
    # reset_returns under a mask, then for all
    mask = np.arange(70) % 3 == 0
    before = a.stats()
    assert before["returns"][mask].any() and before["returns"][~mask].any()
    a.reset_returns(mask)
    after = a.stats()
    assert np.array_equal(after["returns"], np.where(mask, 0.0, before["returns"]))
    assert all(np.array_equal(after[k], before[k]) for k in before if k != "returns")
    a.reset_returns()
    assert not a.stats()["returns"].any()
    for x in (a, b, c, vn, p, v):
        x.close()


def test_npz_round_trip_and_from_stats(tmp_path):
    from windgym_amd.normalize import VecNormalize
    t = _torch()
    va, vb = _venv(16), _venv(16)
    p, _ = make(va.batch.obs_dim, (64, 64), va.n_turb)
    vn = VecNormalize(va, clip_obs=5.0, gamma=0.95)
    vn.rollout(p, 8)
    path = vn.save(os.path.join(tmp_path, "vecnormalize.npz"))
    back = VecNormalize.load(path, vb)
    assert back.args() == vn.args() and back.state() == vn.state()
    frozen = VecNormalize.load(path, vb, training=False, norm_reward=False)
    assert not frozen.training and not frozen.norm_reward and frozen.state() == vn.state()
    mean, var, count = vn.obs_rms
    fs = VecNormalize.from_stats(vb, mean, var, count, ret_var=vn.ret_rms[1], clip_obs=5.0)
    x = vb.batch.obs
    assert t.equal(fs.normalize_obs(x), back.normalize_obs(x)) and fs.obs_rms[2] == count and fs.ret_rms[1] == vn.ret_rms[1]
    r = t.linspace(-3, 3, 16, device="cuda")
    assert t.equal(fs.normalize_reward(r), back.normalize_reward(r))
    with pytest.raises(ValueError, match="obs_mean"):
        VecNormalize.from_stats(vb, mean[:-1], var, count)
    for x in (vn, back, frozen, fs, p, va, vb):
        x.close()


def test_step_is_the_wrappers_step_for_host_loops():
    """reset + step from Python == the twin fed with the env's own rows (get_original_obs / get_original_reward)."""
    from windgym_amd.normalize import VecNormalize
    t = _torch()
    B = 20
    v = _venv(B)
    vn = VecNormalize(v, gamma=0.9)
    twin = VecNormalizeTwin(v.batch.obs_dim, B, gamma=0.9)
    obs, _ = vn.reset(seed=5)
    _one_ulp(obs.cpu().numpy(), twin.reset(vn.get_original_obs().cpu().numpy()), "reset")
    rng = np.random.default_rng(0)
    for i in range(5):
        a = t.from_numpy(rng.uniform(-1, 1, (B, v.n_turb)).astype(np.float32)).cuda()
        obs, rew, term, trunc, infos = vn.step(a)
        wo, wr, wf = twin.step(vn.get_original_obs().cpu().numpy(), vn.get_original_reward().cpu().numpy(), trunc.cpu().numpy(),
                               v.batch.final_obs.cpu().numpy())
        _one_ulp(obs.cpu().numpy(), wo, f"step {i}: obs")
        _one_ulp(rew.cpu().numpy(), wr, f"step {i}: reward")
        _one_ulp(infos["final_obs"].cpu().numpy(), wf, f"step {i}: final obs")
        assert not term.any()
    assert vn.obs_rms[2] == twin.obs_rms.count and vn.ret_rms[2] == twin.ret_rms.count and twin.obs_rms.count > 6 * B
    vn.close(); v.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
NORM_ARGS = dict(clip_obs=8.0, gamma=0.98)


def test_ppo_trains_on_the_normalised_rollout():
    from windgym_amd.normalize import VecNormalize
    from windgym_amd.ppo import PPO
    t = _torch()
    B, T = 32, 16
    kw = dict(n_steps=T, n_epochs=2, ent_coef=0.001, seed=11)
    va, vb = _venv(B), _venv(B)
    a = PPO("MlpPolicy", va, normalize=NORM_ARGS, **kw)
    a.learn(3 * T * B)
    b = PPO("MlpPolicy", vb, **kw)
    nb = VecNormalize(vb, **NORM_ARGS)
    for it in range(3):
        out = nb.rollout(b.policy, T)
        b.opt.gae(out["reward"], out["value"], out["final_value"], out["truncated"], b.gamma, b.gae_lambda, out=(b._adv, b._ret))
        norm_mean, var = float(out["reward"].double().mean()), nb.ret_rms[1]
        b.train(out, 3e-4, 0.2)
        rec = a.log[it]
        assert rec["mean_norm_reward"] == norm_mean and rec["ret_rms_var"] == var
        # wg_metrics sums the T * B float32 rewards in float32: at most n * 2^-24 of sum |r| away from the float64 mean, per term
        assert abs(rec["mean_step_reward"] - float(out["env_reward"].double().mean())) <= (T * B + 4) * 2.0 ** -24 * float(out["env_reward"].double().abs().mean())
    assert t.equal(a.policy.params, b.policy.params) and np.array_equal(a.opt.state()[0], b.opt.state()[0])
    assert a.opt.state()[1] == b.opt.state()[1] and a.normalize.state() == nb.state()
    # predict normalises the rows it is given
    rows = va.batch.obs.cpu().numpy()
    got = a.predict(rows, deterministic=True)[0]
    want = a.policy.predict(a.normalize.normalize_obs(rows), deterministic=True)[0]
    assert np.array_equal(got, want) and not np.array_equal(got, a.policy.predict(rows, deterministic=True)[0])
    with pytest.raises(ValueError, match="another env"):
        PPO("MlpPolicy", va, normalize=nb, **kw)
    for x in (a, b):
        x.close(); x.policy.close()
    nb.close(); va.close(); vb.close()


def test_ppo_save_load_resumes_bit_identically(tmp_path):
    import zipfile
    from windgym_amd.ppo import PPO
    t = _torch()
    B, T = 32, 16
    kw = dict(n_steps=T, n_epochs=2, ent_coef=0.001, seed=11)
    va, vb = _venv(B), _venv(B)
    a = PPO("MlpPolicy", va, normalize=NORM_ARGS, **kw)
    a.learn(3 * T * B)
    b = PPO("MlpPolicy", vb, normalize=NORM_ARGS, **kw)
    b.learn(2 * T * B)
    path = os.path.join(tmp_path, "ppo_normalize.zip")
    b.save(path)
    with zipfile.ZipFile(path) as z:
        assert z.read("normalize_state.bin") == b.normalize.state() and b'"format": "windgym_amd.PPO/1"' in z.read("windgym_ppo.json")
    vc = _venv(B)
    vc.batch.set_state(vb.batch.get_state())
    for name in ("obs", "final_obs", "reward", "truncated"):                     # the last step's outputs live in the caller's tensors
        getattr(vc.batch, name).copy_(getattr(vb.batch, name))
    c = PPO.load(path, vc)
    assert c.normalize.args() == b.normalize.args() and c.normalize.state() == b.normalize.state()
    assert t.equal(c.normalize._cur, b.normalize._cur)
    c.learn(T * B, reset_num_timesteps=False)
    assert c.iteration == 3 and c.num_timesteps == a.num_timesteps
    assert t.equal(c.policy.params, a.policy.params) and np.array_equal(c.opt.state()[0], a.opt.state()[0])
    assert c.normalize.state() == a.normalize.state() and c.log[-1]["ret_rms_var"] == a.log[-1]["ret_rms_var"]
    # without normalize the checkpoint has neither the member nor the key, and loads without one
    d = PPO("MlpPolicy", vb, **kw)
    plain = os.path.join(tmp_path, "ppo_plain.zip")
    d.save(plain)
    with zipfile.ZipFile(plain) as z:
        assert "normalize_state.bin" not in z.namelist() and b"normalize\"" not in z.read("windgym_ppo.json")
    e = PPO.load(plain, vb)
    assert e.normalize is None
    for x in (a, b, c, d, e):
        x.close(); x.policy.close()
    for v in (va, vb, vc):
        v.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnvMulti
    from windgym_amd.normalize import VecNormalize
    from windgym_amd.population import PPOPopulation
    from windgym_amd.turbine import V80
    from windgym_amd.ppo import PPO
    t = _torch()
    B, T = 8, 3
    v, w = _venv(B), _venv(B)
    b, O, N = v.batch, v.batch.obs_dim, v.n_turb
    p, _ = make(O, (64, 64), N)
    vn, other = VecNormalize(v), VecNormalize(w)
    with pytest.raises(ValueError, match="another env"):
        PPO(p, v, normalize=other, n_steps=T)
    with pytest.raises(NotImplementedError, match="curriculum"):
        PPO(p, v, normalize=vn, curriculum=dict(curriculum_steps=10, pure_similarity_steps=1), n_steps=T)
    with pytest.raises(NotImplementedError, match="normalize"):
        PPOPopulation("MlpPolicy", v, n_members=2, normalize={})
    w.shard(0, 2, n_envs_total=2 * B)
    with pytest.raises(NotImplementedError, match="all-reduce"):
        VecNormalize(w)
    # the library: widths, env counts, missing buffers
    z = lambda *shape, dtype=t.float32: t.zeros(shape, dtype=dtype, device=b.device)          # noqa: E731
    bufs = dict(obs=z(T + 1, B, O), actions=z(T, B, N), raw=z(T, B, N), logp=z(T, B), value=z(T, B), final_obs=z(T, B, O),
                final_value=z(T, B), reward=z(T, B), truncated=z(T, B, dtype=t.uint8), norm_obs=z(T + 1, B, O), norm_final_obs=z(T, B, O))
    run = lambda n, bf: b.rollout("wg_rollout_norm", (p._h, n._h), T, bf, (), (False, 0, 0, 0), tail=("norm_obs", "norm_final_obs"))   # noqa: E731
    state = b.get_state()
    for n_obs, n_envs in ((O + 1, B), (O, B + 1)):
        n = _norm(n_obs, n_envs)
        with pytest.raises(ValueError, match="wg_norm holds statistics"):
            run(n, bufs)
        n.close()
    for key in ("obs", "final_obs"):
        with pytest.raises(ValueError, match="obs, final_obs"):
            run(vn._norm, {k: x for k, x in bufs.items() if k != key})
    assert b.get_state() == state                                                            # nothing was enqueued
    n = _norm(O, B)
    with pytest.raises(ValueError, match="at most n_envs"):
        n.obs(z(B + 1, O), z(B + 1, O))
    n.set_training(False)
    n.obs(z(B + 1, O), z(B + 1, O))                                                          # frozen: any number of rows
    with pytest.raises(ValueError, match="go together"):
        n.obs(z(B, O), z(B, O), z(B, O), None)
    with pytest.raises(ValueError, match="statistics of"):
        n.load_state(_norm(O + 1, B).state())
    with pytest.raises(ValueError, match="CUDA tensor"):
        n.obs(z(B, O).cpu(), z(B, O))
    with pytest.raises(ValueError, match="gamma"):
        _norm(O, B, gamma=2.0)
    t.cuda.synchronize()
    b.check()
    for x in (n, vn, other, p, v, w):
        x.close()
    m = WindFarmVecEnvMulti(V80(), 4, yaml_dict=copy.deepcopy(presets.multi_3x3_config()), seed=5, turbtype="None", n_rotor_pts=16)
    with pytest.raises(NotImplementedError, match="WindFarmVecEnvMulti"):
        VecNormalize(m)
    m.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
class _NormalisedPredict:
    """A host-loop model: predict() normalises the rows with a frozen wg_norm (the kernel the closed loop uses), then asks the policy"""

    def __init__(self, p, norm):
        self.p, self.norm = p, norm

    def predict(self, obs, state=None, episode_start=None, deterministic=False):
        t = _torch()
        x = t.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).cuda()
        return self.p.predict(self.norm.obs(x, t.empty_like(x)), deterministic=deterministic)


def test_evaluation_through_a_frozen_wrapper(tmp_path):
    from windgym_amd import presets
    from windgym_amd.binding import pack_norm_state
    from windgym_amd.evaluate import eval_sweep
    from windgym_amd.normalize import save_stats
    from windgym_amd.turbine import V80
    p, _ = make(8, (64, 64), 4)
    rng = np.random.default_rng(4)
    stats = dict(obs_mean=rng.uniform(-0.3, 0.3, 8), obs_var=rng.uniform(0.05, 0.5, 8), obs_count=5000.0001, ret_mean=0.1, ret_var=3.0,
                 ret_count=5000.0001, returns=np.zeros(6))
    args = dict(norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8, training=True)
    path = save_stats(os.path.join(tmp_path, "vecnormalize.npz"), args, stats)
    kw = dict(yaml_dict=presets.env1_config(), winddirs=(260.0, 270.0, 280.0), windspeeds=(8.0, 11.0), t_sim=40, turbtype="Random", seed=1)
    norm = _norm(8, 6)
    norm.load_state(pack_norm_state(8, 6, **stats))
    norm.set_training(False)
    dev_ds = eval_sweep(V80(), None, p, normalize=path, **kw)
    host_ds = eval_sweep(V80(), None, _NormalisedPredict(p, norm), **kw)
    raw_ds = eval_sweep(V80(), None, p, **kw)
    data = lambda d: d["data"] if isinstance(d, dict) else {k: d[k].values for k in d.data_vars}      # noqa: E731
    dd, hd, rd = data(dev_ds), data(host_ds), data(raw_ds)
    assert set(dd) == set(hd) == set(rd)
    for k in hd:
        assert dd[k].shape == rd[k].shape and np.array_equal(dd[k], hd[k]), k
    assert not np.array_equal(dd["yaw_a"], rd["yaw_a"])               # the policy read other rows than the env's own
    assert norm.state() == pack_norm_state(8, 6, **stats)             # frozen
    with pytest.raises(ValueError, match="normalize"):
        eval_sweep(V80(), None, _NormalisedPredict(p, norm), normalize=path, **kw)
    norm.close(); p.close()
