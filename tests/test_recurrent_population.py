"""CPU tests of populations of recurrent policies: the pure host helpers of windgym_amd/recurrent_population.py, the refusals that need
no device, and the C structs the new entries take against their ctypes mirrors (gcc sizeof / offsetof)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import c_layout
from windgym_amd import binding
from windgym_amd.recurrent_population import check_same_architecture, global_envs, member_minibatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_global_envs():
    local = np.array([[3, 0, 2, 1], [1, 2, 3, 0]], np.int32)
    assert np.array_equal(global_envs(local, 0, 4), local)
    assert np.array_equal(global_envs(local, 2, 4), local + 8)
    # member m's entries are a permutation of its shard [m Bm, (m + 1) Bm)
    for m in range(3):
        for row in global_envs(local, m, 4):
            assert sorted(row.tolist()) == list(range(4 * m, 4 * m + 4))
    assert global_envs(5, 3, 40) == 125
    torch = pytest.importorskip("torch")
    x = torch.tensor([2, 0, 1], dtype=torch.int64)
    assert global_envs(x, 1, 3).tolist() == [5, 3, 4]


def test_member_minibatch_is_envs_per_minibatch_on_the_member():
    from windgym_amd.recurrent_ppo import envs_per_minibatch
    assert member_minibatch(None, 128, 4096, 16) == (256, 64, 4)              # default: ceil(Bm / 4) envs of ONE member
    assert member_minibatch(None, 8, 120, 3) == (40, 10, 4)
    assert member_minibatch(6 * 16, 6, 120, 3) == (40, 16, 3)                 # minibatches of 16, 16 and 8 envs
    assert member_minibatch(8 * 5, 8, 10, 2) == (5, 5, 1)
    assert member_minibatch(None, 8, 10, 2) == (5, envs_per_minibatch(None, 8, 5), 3)
    with pytest.raises(ValueError, match="multiple of n_steps"):
        member_minibatch(20, 8, 16, 2)
    with pytest.raises(ValueError, match=r"n_steps \* num_envs = 40"):        # counted per member: 5 envs x 8 steps
        member_minibatch(48, 8, 10, 2)
    with pytest.raises(ValueError, match="does not divide by 3"):
        member_minibatch(None, 8, 16, 3)
    with pytest.raises(ValueError, match="1 .. 16 members"):
        member_minibatch(None, 8, 34, 17)


class _Fake:
    recurrent = True

    def __init__(self, **desc):
        self.desc = dict(n_in=7, hidden=40, nets=2, **desc)


def test_refusals_without_a_device():
    from windgym_amd.recurrent_population import RecurrentPPOPopulation, RecurrentPopulation
    a, b = _Fake(), _Fake()
    assert check_same_architecture([a, b]) == [a, b]
    with pytest.raises(ValueError, match="1 .. 16 members, not 0"):
        check_same_architecture([])
    with pytest.raises(ValueError, match="1 .. 16 members, not 17"):
        RecurrentPopulation([_Fake() for _ in range(17)])
    with pytest.raises(ValueError, match="member 1 has another architecture"):
        RecurrentPopulation([a, _Fake(shared_lstm=True)])
    with pytest.raises(ValueError, match="member 2 is the same policy"):
        RecurrentPopulation([a, b, a])

    class Mlp:
        recurrent = False
    with pytest.raises(ValueError, match="member 1 is not a recurrent policy"):
        RecurrentPopulation([a, Mlp()])

    class Env:
        num_envs = 12
    with pytest.raises(ValueError, match="member 0 is not a recurrent policy"):
        RecurrentPPOPopulation([Mlp()], Env())
    with pytest.raises(ValueError, match="only 'MlpLstmPolicy' or a list of MlpLstmPolicy objects"):
        RecurrentPPOPopulation("MlpPolicy", Env(), n_members=2)
    with pytest.raises(ValueError, match="needs n_members"):
        RecurrentPPOPopulation("MlpLstmPolicy", Env())
    for k in ("curriculum", "normalize"):
        with pytest.raises(NotImplementedError, match=k):
            RecurrentPPOPopulation("MlpLstmPolicy", Env(), n_members=2, **{k: object()})

    class Multi(Env):
        possible_agents = ["a"]
    with pytest.raises(NotImplementedError, match="WindFarmVecEnvMulti"):
        RecurrentPPOPopulation("MlpLstmPolicy", Multi(), n_members=2)
    with pytest.raises(ValueError, match="does not divide by 5"):
        RecurrentPPOPopulation("MlpLstmPolicy", Env(), n_members=5)
    with pytest.raises(ValueError, match="multiple of n_steps"):
        RecurrentPPOPopulation("MlpLstmPolicy", Env(), n_members=2, n_steps=8, batch_size=20)
    with pytest.raises(ValueError, match="2 values for 3 members"):
        RecurrentPPOPopulation("MlpLstmPolicy", Env(), n_members=3, gamma=[0.9, 0.99])


def test_the_plain_populations_still_refuse_a_recurrent_policy():
    from windgym_amd.population import PPOPopulation

    class Env:
        num_envs = 12
    with pytest.raises(NotImplementedError, match="PPOPopulation: training / wrapping a recurrent policy"):
        PPOPopulation([_Fake()], Env())


@pytest.mark.parametrize("name,mirror", [("wg_rollout_lstm_bufs", binding.CRolloutLstmBufs), ("wg_lstm_ppo_batch", binding.CLstmPpoBatch),
                                         ("wg_rollout_bufs", binding.CRolloutBufs), ("wg_ppo_hyper", binding.CPpoHyper)])
def test_structs_of_the_population_entries_match_c(tmp_path, name, mirror):
    """sizeof / offsetof of every struct wg_lstm_pop_rollout and wg_lstm_pop_update take, as gcc sees them == the ctypes mirrors."""
    fields = [f[0] for f in mirror._fields_]
    out = c_layout(name, fields, tmp_path)
    assert out["sizeof"] == C.sizeof(mirror)
    for f in fields:
        assert out[f] == getattr(mirror, f).offset, f


def test_new_entries_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "windgym_hip.h")).read()
    src = open(binding.__file__).read()
    for name in ("wg_lstm_pop_create", "wg_lstm_pop_destroy", "wg_lstm_pop_act", "wg_lstm_pop_rollout", "wg_lstm_pop_update"):
        assert f"int {name}(" in hdr and name in binding.ABI_SYMBOLS and f"L.{name}.argtypes" in src, name
    assert "#define WG_ABI_VERSION 4" in hdr or "WG_ABI_VERSION" in hdr
