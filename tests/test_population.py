"""CPU tests of populations (windgym_amd/population.py): per-member hyper-parameters, the local -> global row map, the member
checkpoint layout, and the new entries in header, export list and ctypes signatures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from windgym_amd import binding, population as pop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("wg_pop_create", "wg_pop_destroy", "wg_pop_act", "wg_pop_rollout", "wg_gae_pop", "wg_pop_update")


def test_broadcast_of_per_member_hyper_parameters():
    assert pop.broadcast_hyper("gamma", 0.99, 3) == [0.99] * 3
    assert pop.broadcast_hyper("gamma", (0.9, 0.8), 2) == [0.9, 0.8]
    assert pop.broadcast_hyper("gamma", np.array([0.9, 0.8]), 2) == [0.9, 0.8]
    f = lambda p: 1e-3 * p                                                # noqa: E731  (a schedule is every member's)
    assert pop.broadcast_hyper("learning_rate", f, 2) == [f, f]
    assert pop.broadcast_hyper("seed", None, 2) == [None, None]
    with pytest.raises(ValueError, match="3 values for 2 members"):
        pop.broadcast_hyper("gamma", [0.9, 0.8, 0.7], 2)


def test_population_shape():
    assert pop.check_population_shape(4, 64) == 16
    assert pop.check_population_shape(1, 7) == 7
    assert pop.POP_MAX == binding.WG_POP_MAX == 16
    for P in (0, 17):
        with pytest.raises(ValueError, match="1 .. 16 members"):
            pop.check_population_shape(P, 64)
    with pytest.raises(ValueError, match="does not divide by 3"):
        pop.check_population_shape(3, 64)


@pytest.mark.parametrize("T,B,P", [(5, 6, 3), (4, 150, 3), (3, 8, 1), (2, 32, 16)])
def test_global_rows_against_a_restatement(T, B, P):
    Bm = B // P
    grid = np.arange(T * B).reshape(T, B)                                 # the batch's row ids, [T, B]
    seen = []
    for m in range(P):
        want = grid[:, m * Bm:(m + 1) * Bm].reshape(-1)                   # the member's contiguous copy, row by row
        got = pop.global_rows(np.arange(T * Bm), m, B, Bm)
        assert np.array_equal(got, want)
        seen.append(got)
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(T * B))   # the members partition the batch
    import torch
    assert np.array_equal(pop.global_rows(torch.arange(T * Bm), P - 1, B, Bm).numpy(), seen[-1])


def test_constructor_refusals_need_no_device():
    class V:
        num_envs = 10
    with pytest.raises(NotImplementedError, match="out of scope"):
        pop.PPOPopulation("MlpPolicy", type("M", (), dict(possible_agents=[1], num_envs=8))(), n_members=2)
    with pytest.raises(ValueError, match="needs n_members"):
        pop.PPOPopulation("MlpPolicy", V())
    with pytest.raises(ValueError, match="does not divide by 4"):
        pop.PPOPopulation("MlpPolicy", V(), n_members=4)
    with pytest.raises(ValueError, match="3 values for 2 members"):
        pop.PPOPopulation("MlpPolicy", V(), n_members=2, gamma=[0.9, 0.9, 0.9])
    with pytest.raises(ValueError, match="member 1: gamma"):
        pop.PPOPopulation("MlpPolicy", V(), n_members=2, gamma=[0.9, 1.5])
    with pytest.raises(ValueError, match="batch_size must lie"):
        pop.PPOPopulation("MlpPolicy", V(), n_members=2, n_steps=4, batch_size=21)


def test_member_checkpoint_is_a_plain_ppo_zip(tmp_path):
    import json
    import zipfile

    import torch
    from windgym_amd.policy import make_desc, n_params, param_layout, read_sb3_zip
    from windgym_amd.ppo import write_checkpoint
    desc = make_desc(6, 2, (8,), (8,), "tanh", True, None)
    flat = torch.arange(n_params(desc), dtype=torch.float32) * 0.01

    class Pol:
        seed, counter = 5, 0

        def state_dict(self):
            out, o = {}, 0
            for name, shape in param_layout(desc):
                n = int(np.prod(shape))
                out[name] = flat[o:o + n].view(shape)
                o += n
            return out
    Pol.desc = desc

    class Opt:
        def state(self):
            return np.zeros(2 * flat.numel(), np.float32), 12
    g = torch.Generator()
    g.manual_seed(5)
    hyper = dict(n_steps=16, batch_size=32, n_epochs=3, gamma=0.9, gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, vf_coef=0.5,
                 max_grad_norm=0.5, learning_rate=lambda p: 1e-3, normalize_advantage=True)
    path = write_checkpoint(str(tmp_path / "member_01.zip"), Pol(), Opt(), g, hyper, 5, 384, 3, [dict(member=1, loss=0.5)], None, 48)
    d, tensors = read_sb3_zip(path)
    assert d["n_in"] == 6 and d["n_out"] == 2 and d["hidden_pi"] == (8,)
    assert np.array_equal(np.asarray(tensors["log_std"]), flat[-2:].numpy())
    with zipfile.ZipFile(path) as z:
        meta = json.loads(z.read("windgym_ppo.json"))
        assert {"policy.pth", "adam_state.npy", "generator_state.npy", "windgym_ppo.json"} <= set(z.namelist())
    assert meta["format"] == "windgym_amd.PPO/1" and meta["adam_step"] == 12 and meta["env_policy_steps"] == 48 and meta["critic"] is None
    assert meta["hyper"]["gamma"] == 0.9 and meta["hyper"]["learning_rate"] is None and meta["hyper"]["batch_size"] == 32
    assert set(meta["hyper"]) == set(pop.SHARED + pop.PER_MEMBER)


def test_header_exports_and_ctypes_agree():
    from windgym_amd import build
    hdr = open(os.path.join(ROOT, "include", "windgym_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "#define WG_POP_MAX 16" in hdr
    L = C.CDLL(build.build())
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in the header"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in binding.ABI_SYMBOLS and hasattr(L, name)
    import torch  # noqa: F401  (load_library imports it first)
    lib = binding.load_library()
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert len(getattr(lib, name).argtypes) == n_args, name


def test_package_exports():
    import windgym_amd
    assert windgym_amd.PPOPopulation is pop.PPOPopulation and windgym_amd.Population is pop.Population
