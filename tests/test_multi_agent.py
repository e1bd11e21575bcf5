"""CPU tests of the multi-agent path (one agent per turbine, one shared policy): the new ABI entries and their buffer struct
are the same in the header, the built library and the ctypes mirror; the float64 shared-reward GAE reference
(oracle/ppo_oracle.py) against its definition and against the single-agent oracle; argument validation of
``WindFarmVecEnvMulti`` and of ``PPO`` on a multi-agent env that needs no device.  The kernels are tested on the GPU
(tests/test_gpu_multi_agent.py)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from oracle import ppo_oracle as oo
from oracle.ppo_oracle import gae_shared, gae_shared_brute
from helpers import c_layout
from windgym_amd import binding, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wg_set_final_obs_multi_buffer", "wg_rollout_multi", "wg_gae_shared")


def _header():
    hdr = open(os.path.join(ROOT, "include", "windgym_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_new_entries_header_exports_ctypes_agree():
    hdr = _header()
    L = C.CDLL(build.build())
    bound = binding.load_library()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in windgym_hip.h"
        n_params = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in binding.ABI_SYMBOLS
        assert hasattr(L, name), f"{name} not exported"
        assert len(getattr(bound, name).argtypes) == n_params, name
    assert "WG_ABI_VERSION 4" in hdr          # entries were added, none changed


def test_rollout_multi_bufs_layout_matches_c(tmp_path):
    fields = [f[0] for f in binding.CRolloutMultiBufs._fields_]
    m = re.search(r"typedef struct wg_rollout_multi_bufs \{(.*?)\} wg_rollout_multi_bufs;", _header(), flags=re.S)
    declared = re.findall(r"(\w+)\s*;", m.group(1))
    assert declared == fields                  # same members, same order
    out = c_layout("wg_rollout_multi_bufs", fields, tmp_path)
    assert out["sizeof"] == C.sizeof(binding.CRolloutMultiBufs)
    for f in fields:
        assert out[f] == getattr(binding.CRolloutMultiBufs, f).offset, f


@pytest.mark.parametrize("T,B,A,p", [(1, 3, 2, 0.5), (7, 5, 9, 0.3), (30, 4, 3, 0.0), (30, 4, 3, 1.0)])
def test_shared_gae_reference_equals_its_definition(T, B, A, p):
    rng = np.random.default_rng(T * 100 + B * 10 + A)
    r = rng.standard_normal((T, B))
    v, fv = rng.standard_normal((T, B, A)), rng.standard_normal((T, B, A))
    tr = rng.uniform(size=(T, B)) < p
    a, ret = gae_shared(r, v, fv, tr, 0.97, 0.9)
    b, ret_b = gae_shared_brute(r, v, fv, tr, 0.97, 0.9)
    assert np.allclose(a, b, rtol=1e-12, atol=1e-12) and np.allclose(ret, ret_b, rtol=1e-12, atol=1e-12)
    # every agent of an env is the single-agent recurrence on its own values with the env's reward and flags
    for i in range(A):
        s, sr = oo.gae(r, v[:, :, i], fv[:, :, i], tr, 0.97, 0.9)
        assert np.array_equal(a[:, :, i], s) and np.array_equal(ret[:, :, i], sr)
    # the reward is the ENV's: an agent-indexed reward (row b * A + i of a flat array) is a different number
    if A > 1 and B > 1:
        wrong = r.reshape(-1)[(np.arange(B)[:, None] * A + np.arange(A)[None, :]) % (T * B)]
        assert not np.allclose(a[-1], wrong + 0.97 * fv[-1] - v[-1])


def test_vec_env_multi_validates_before_touching_a_device():
    from windgym_amd.envs import WindFarmVecEnvMulti
    from windgym_amd.turbine import V80
    with pytest.raises(ValueError, match="n_envs"):
        WindFarmVecEnvMulti(V80(), 0)
    with pytest.raises(ValueError, match="CUDA tensors"):
        WindFarmVecEnvMulti(V80(), 4, as_torch=False)
    import windgym_amd
    assert windgym_amd.WindFarmVecEnvMulti is WindFarmVecEnvMulti


def _stub_envs():
    batch = types.SimpleNamespace(obs_dim=18)
    single = types.SimpleNamespace(num_envs=8, n_turb=9, batch=batch)
    multi = types.SimpleNamespace(num_envs=8, n_turb=9, batch=batch, obs_len=2, possible_agents=[f"turbine_{i}" for i in range(9)])
    return single, multi


def test_ppo_rows_are_agent_rows_on_a_multi_agent_env():
    from windgym_amd.ppo import PPO
    single, multi = _stub_envs()
    # batch_size is bounded by n_steps * num_envs * n_turb there, by n_steps * num_envs on the single-agent env
    with pytest.raises(ValueError, match=r"n_steps \* num_envs \* n_turb = 288"):
        PPO("MlpPolicy", multi, n_steps=4, batch_size=289)
    with pytest.raises(ValueError, match=r"n_steps \* num_envs = 32"):
        PPO("MlpPolicy", single, n_steps=4, batch_size=33)


@pytest.mark.parametrize("which,shape", [("multi", (18, 9)), ("multi", (2, 9)), ("single", (2, 1)), ("single", (18, 1))])
def test_ppo_refuses_a_mismatched_policy_naming_both_shapes(which, shape):
    from windgym_amd.ppo import PPO
    single, multi = _stub_envs()
    pol = types.SimpleNamespace(n_in=shape[0], n_out=shape[1])
    with pytest.raises(ValueError) as ei:
        PPO(pol, multi if which == "multi" else single, n_steps=4)
    msg = str(ei.value)
    assert f"{shape[0]} -> {shape[1]}" in msg
    assert ("2 -> 1" if which == "multi" else "18 -> 9") in msg
    assert "obs_dim -> n_turb" in msg and "obs_len -> 1" in msg
