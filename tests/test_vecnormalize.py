"""CPU side of VecNormalize: the float64 twin (tests/vecnormalize_twin.py) against hand-computed values and the step-order
quirks of SB3's class, the ABI surface of the wg_norm entries, the files and the refusals that need no device."""
import ctypes as C
import json
import os
import re
import types
import zipfile

import numpy as np
import pytest

from vecnormalize_twin import RunningMeanStd, VecNormalizeTwin
from windgym_amd import binding, build
from windgym_amd.normalize import ARGS, VecNormalize, check_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"wg_norm_create": 3, "wg_norm_destroy": 1, "wg_norm_get_state": 3, "wg_norm_set_state": 3, "wg_norm_set_training": 2,
           "wg_norm_reset_returns": 3, "wg_norm_obs": 7, "wg_norm_reward": 6, "wg_rollout_norm": 12}       # name -> arguments


def test_two_updates_equal_one_update_of_the_concatenation():
    rng = np.random.default_rng(0)
    a, b = rng.normal(2.0, 3.0, (7, 4)), rng.normal(-1.0, 0.5, (12, 4))
    two, one = RunningMeanStd((4,)), RunningMeanStd((4,))
    two.update(a); two.update(b)
    one.update(np.concatenate([a, b]))
    assert two.count == 1e-4 + 19 == one.count
    assert np.allclose(two.mean, one.mean, rtol=1e-13, atol=0) and np.allclose(two.var, one.var, rtol=1e-13, atol=0)
    # and both are the moments of the 19 rows weighted against the prior (mean 0, var 1) of weight 1e-4, by the same merge
    x = np.concatenate([a, b])
    w, n = 1e-4, 19
    mean = x.mean(0) * n / (w + n)
    var = (w * 1.0 + n * x.var(0) + x.mean(0) ** 2 * w * n / (w + n)) / (w + n)
    assert np.allclose(two.mean, mean, rtol=1e-13, atol=0) and np.allclose(two.var, var, rtol=1e-13, atol=0)


def test_hand_computed_2x2():
    """batch [[1, 10], [3, 14]]: bm = (2, 12), bv = (1, 4); tot = 2.0001."""
    r = RunningMeanStd((2,))
    r.update(np.array([[1.0, 10.0], [3.0, 14.0]]))
    tot = 2.0001
    assert r.count == tot
    assert np.allclose(r.mean, [2.0 * 2 / tot, 12.0 * 2 / tot], rtol=1e-15, atol=0)
    want_var = [(1e-4 + 1.0 * 2 + 4.0 * 1e-4 * 2 / tot) / tot, (1e-4 + 4.0 * 2 + 144.0 * 1e-4 * 2 / tot) / tot]
    assert np.allclose(r.var, want_var, rtol=1e-15, atol=0)
    vn = VecNormalizeTwin(2, 2)
    out = vn.reset(np.array([[1.0, 10.0], [3.0, 14.0]], np.float32))
    sd = np.sqrt(np.array(want_var) + 1e-8)
    want = ((np.array([[1.0, 10.0], [3.0, 14.0]]) - r.mean) / sd).astype(np.float32)
    assert out.dtype == np.float32 and np.array_equal(out, want)
    assert abs(float(out[0, 0]) + 1.0) < 1e-3 and abs(float(out[1, 1]) - 1.0) < 1e-3      # about -1 / +1 standard deviations


def test_terminal_row_uses_post_update_statistics_and_never_enters_them():
    vn, ref = VecNormalizeTwin(1, 2), RunningMeanStd((1,))
    obs = [np.array([[1.0], [2.0]]), np.array([[3.0], [5.0]]), np.array([[4.0], [0.0]])]
    fin = np.array([[100.0], [-50.0]])
    for t in range(3):
        ref.update(obs[t])
        o, _, f = vn.step(obs[t], np.zeros(2), np.array([False, t == 1]), fin)
        # the statistics hold the env's rows only, whatever the final rows were
        assert np.array_equal(vn.obs_rms.mean, ref.mean) and np.array_equal(vn.obs_rms.var, ref.var) and vn.obs_rms.count == ref.count
        # and the final rows are normalised with the statistics AFTER this step's update
        want = np.clip((fin - ref.mean) / np.sqrt(ref.var + 1e-8), -10, 10).astype(np.float32)
        assert np.array_equal(f, want)
    assert vn.obs_rms.count == 1e-4 + 6


def test_returns_are_zeroed_after_the_update():
    vn = VecNormalizeTwin(1, 2, gamma=0.5)
    ref = RunningMeanStd(())
    r = [np.array([1.0, 2.0]), np.array([3.0, 4.0]), np.array([5.0, 6.0])]
    done = [np.array([False, False]), np.array([True, False]), np.array([False, False])]
    want_returns = [np.array([1.0, 2.0]), np.array([3.5, 5.0]), np.array([5.0, 8.5])]       # env 0: 0.5 * 1 + 3 = 3.5 enters, THEN zero
    for t in range(3):
        ref.update(want_returns[t])
        out = vn.reward_half(r[t], done[t])
        assert vn.ret_rms.var == ref.var and vn.ret_rms.mean == ref.mean
        assert np.array_equal(out, np.clip(r[t] / np.sqrt(ref.var + 1e-8), -10, 10).astype(np.float32))
        kept = want_returns[t].copy()
        kept[done[t]] = 0.0
        assert np.array_equal(vn.returns, kept)


def test_frozen_statistics_still_normalise():
    vn = VecNormalizeTwin(1, 2)
    vn.step(np.array([[1.0], [3.0]]), np.array([1.0, 2.0]), np.array([False, False]))
    before = (vn.obs_rms.mean.copy(), vn.obs_rms.var.copy(), vn.obs_rms.count, vn.ret_rms.mean, vn.ret_rms.var, vn.ret_rms.count)
    vn.training = False
    returns = vn.returns.copy()
    for t in range(3):
        o, r, _ = vn.step(np.array([[7.0], [9.0]]), np.array([4.0, 5.0]), np.array([False, t == 1]))
        assert np.array_equal(o, np.clip((np.array([[7.0], [9.0]]) - before[0]) / np.sqrt(before[1] + 1e-8), -10, 10).astype(np.float32))
        assert np.array_equal(r, np.clip(np.array([4.0, 5.0]) / np.sqrt(before[4] + 1e-8), -10, 10).astype(np.float32))
        assert not np.array_equal(o, np.array([[7.0], [9.0]], np.float32))
        if t >= 1:
            returns[1] = 0.0                     # (rule 7 does not ask whether the wrapper trains)
        assert np.array_equal(vn.returns, returns)
    after = (vn.obs_rms.mean, vn.obs_rms.var, vn.obs_rms.count, vn.ret_rms.mean, vn.ret_rms.var, vn.ret_rms.count)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_header_bindings_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "windgym_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "wg_norm.hip" in build.SOURCES
    L = C.CDLL(build.build())
    bound = binding.load_library()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in binding.ABI_SYMBOLS and hasattr(L, name), name
        assert len(getattr(bound, name).argtypes) == n_args, name
    L.wg_abi_version.restype = C.c_int
    assert L.wg_abi_version() == 4
    # the ctypes mirror of wg_norm_desc: 4 int32, 2 float, 2 double
    assert C.sizeof(binding.CNormDesc) == 40 and binding.CNormDesc.gamma.offset == 24


def test_library_refusals_before_any_device_call():
    build.build()
    L = binding.load_library()
    out = C.c_void_p()
    assert L.wg_norm_create(None, 0, C.byref(out)) == -1 and b"null" in L.wg_last_error()
    good = dict(n_obs=3, n_envs=2, norm_obs=1, norm_reward=1, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)
    for key, bad in (("n_obs", 0), ("n_envs", 0), ("clip_obs", 0.0), ("clip_reward", -1.0), ("gamma", 1.5), ("gamma", -0.1),
                     ("epsilon", 0.0), ("epsilon", float("nan"))):
        d = binding.CNormDesc(**{**good, key: bad})
        assert L.wg_norm_create(C.byref(d), 0, C.byref(out)) == -1 and key.encode() in L.wg_last_error(), key
        assert not out.value
    assert L.wg_norm_obs(None, 1, None, None, None, None, None) == -1
    assert L.wg_norm_reward(None, 1, None, None, None, None) == -1
    assert L.wg_rollout_norm(None, None, None, 1, 0, 0, 0, 0, None, None, None, None) == -1
    assert L.wg_norm_get_state(None, None, None) == -1 and L.wg_norm_set_state(None, None, 0) == -1
    assert L.wg_norm_set_training(None, 1) == -1 and L.wg_norm_reset_returns(None, None, None) == -1
    assert L.wg_norm_destroy(None) == 0


def test_state_blob_packing_round_trip():
    rng = np.random.default_rng(1)
    s = dict(obs_mean=rng.normal(size=5), obs_var=rng.uniform(0.1, 2, 5), obs_count=123.0001, ret_mean=0.3, ret_var=4.5, ret_count=77.0001,
             returns=rng.normal(size=3))
    blob = binding.pack_norm_state(5, 3, **s)
    assert len(blob) == 16 + 8 * (2 * 5 + 4 + 3)
    back = binding.unpack_norm_state(blob, 5, 3)
    assert all(np.array_equal(back[k], s[k]) for k in s)
    with pytest.raises(ValueError, match="wrong width"):
        binding.pack_norm_state(4, 3, **s)


@pytest.mark.parametrize("kw, name", [(dict(gamma=1.5), "gamma"), (dict(gamma=-0.1), "gamma"), (dict(epsilon=0.0), "epsilon"),
                                      (dict(epsilon=2.0), "epsilon"), (dict(clip_obs=0.0), "clip_obs"), (dict(clip_reward=-3.0), "clip_reward"),
                                      (dict(clip_obs=float("nan")), "clip_obs")])
def test_argument_ranges(kw, name):
    host_env = types.SimpleNamespace(batch=object(), _rollout=None, as_torch=True, num_envs=2)
    with pytest.raises(ValueError, match=name):
        VecNormalize(host_env, **kw)
    with pytest.raises(ValueError, match=name):
        check_args(**{**dict(clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8), **kw})


def test_env_refusals_need_no_device():
    base = dict(batch=object(), _rollout=None, num_envs=4)
    with pytest.raises(ValueError, match="as_torch"):
        VecNormalize(types.SimpleNamespace(as_torch=False, **base))
    with pytest.raises(NotImplementedError, match="WindFarmVecEnvMulti"):
        VecNormalize(types.SimpleNamespace(as_torch=True, possible_agents=["a"], **base))
    with pytest.raises(NotImplementedError, match="population"):
        VecNormalize(types.SimpleNamespace(as_torch=True, population=object(), **base))
    with pytest.raises(NotImplementedError, match="all-reduce"):
        VecNormalize(types.SimpleNamespace(as_torch=True, _global_offset=4, **base))
    with pytest.raises(NotImplementedError, match="all-reduce"):
        VecNormalize(types.SimpleNamespace(as_torch=True, _global_offset=0, _sharded=True, **base))
    with pytest.raises(ValueError, match="WindFarmVecEnv"):
        VecNormalize(object())
    assert ARGS == ("norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma", "epsilon", "training")


def test_trainers_refuse_what_is_out_of_scope():
    from windgym_amd.population import PPOPopulation
    from windgym_amd.ppo import PPO
    multi = types.SimpleNamespace(possible_agents=["a"], n_turb=2, num_envs=4, obs_len=3, batch=types.SimpleNamespace(obs_dim=9))
    with pytest.raises(NotImplementedError, match="normalize"):
        PPO("MlpPolicy", multi, normalize={})
    flat = types.SimpleNamespace(n_turb=2, num_envs=4, as_torch=True, _rollout=None, batch=types.SimpleNamespace(obs_dim=9))
    with pytest.raises(NotImplementedError, match="curriculum"):
        PPO("MlpPolicy", flat, normalize={}, curriculum=dict(curriculum_steps=10, pure_similarity_steps=1))
    with pytest.raises(ValueError, match="normalize"):
        PPO("MlpPolicy", flat, normalize=3)
    with pytest.raises(NotImplementedError, match="normalize"):
        PPOPopulation("MlpPolicy", flat, n_members=2, normalize={})


class _Opt:
    def state(self):
        return np.arange(6, dtype=np.float32), 5


def _fake_policy():
    import torch
    return types.SimpleNamespace(state_dict=lambda: {"log_std": torch.zeros(2)}, desc={"n_in": 3}, seed=1, counter=2)


def test_checkpoint_members_without_normalize_are_unchanged(tmp_path):
    import torch
    from windgym_amd.ppo import HYPER, write_checkpoint
    hyper = {k: 1 for k in HYPER}
    args = (_fake_policy(), _Opt(), torch.Generator(), hyper, 0, 10, 1, [], None, 7)
    plain = write_checkpoint(os.path.join(tmp_path, "a.zip"), *args)
    with zipfile.ZipFile(plain) as z:
        assert z.namelist() == ["policy.pth", "adam_state.npy", "generator_state.npy", "windgym_ppo.json"]
        meta = json.loads(z.read("windgym_ppo.json"))
        assert "normalize" not in meta and meta["format"] == "windgym_amd.PPO/1"
    vn = types.SimpleNamespace(args=lambda: dict(gamma=0.9), state=lambda: b"blob")
    with_norm = write_checkpoint(os.path.join(tmp_path, "b.zip"), *args, None, vn)
    with zipfile.ZipFile(with_norm) as z:
        assert z.namelist() == ["policy.pth", "adam_state.npy", "generator_state.npy", "windgym_ppo.json", "normalize_state.bin"]
        meta = json.loads(z.read("windgym_ppo.json"))
        assert meta["normalize"] == dict(gamma=0.9) and meta["format"] == "windgym_amd.PPO/1" and z.read("normalize_state.bin") == b"blob"


def test_npz_round_trip_holds_arrays_and_arguments_only(tmp_path):
    from windgym_amd.normalize import STATS, load_stats, save_stats
    rng = np.random.default_rng(2)
    s = dict(obs_mean=rng.normal(size=5), obs_var=rng.uniform(0.1, 2, 5), obs_count=123.0001, ret_mean=0.3, ret_var=4.5, ret_count=77.0001,
             returns=rng.normal(size=3))
    args = dict(norm_obs=True, norm_reward=False, clip_obs=5.0, clip_reward=10.0, gamma=0.9, epsilon=1e-8, training=True)
    path = save_stats(os.path.join(tmp_path, "vecnormalize.npz"), args, s)
    with np.load(path, allow_pickle=False) as z:                 # loads with pickling refused: arrays and one string
        assert set(z.files) == set(STATS) | {"args"} and all(z[k].dtype == np.float64 for k in STATS)
    got_args, got = load_stats(path)
    assert got_args == args and set(got_args) == set(ARGS)
    assert all(np.array_equal(got[k], s[k]) for k in STATS)
    other = os.path.join(tmp_path, "other.npz")
    np.savez(other, x=np.zeros(3))
    with pytest.raises(ValueError, match="not a VecNormalize file"):
        load_stats(other)


def test_from_stats_refuses_another_width():
    env = types.SimpleNamespace(batch=types.SimpleNamespace(obs_dim=4))
    with pytest.raises(ValueError, match="obs_mean"):
        VecNormalize.from_stats(env, np.zeros(3), np.ones(4), 10.0)
    with pytest.raises(ValueError, match="obs_var"):
        VecNormalize.from_stats(env, np.zeros(4), np.ones((4, 1)), 10.0)
