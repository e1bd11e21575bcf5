"""The KL-adaptive learning rate, decided on the CPU: the rule of windgym_amd/csrc/wg_train.h (plain C++, the function the Adam
kernels call) at its edges and bit for bit against numpy float32, the words the rate travels through during an update, the host's
half of Adam's scalars, the trainers' argument checks without a device, and the checkpoint members.  tests/kl_lr_shim.cpp hands the
header's functions over."""
import ctypes as C
import types

import numpy as np
import pytest

from helpers import host_shim
from kl_lr_cases import F, np_next, np_rule, replay

INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = host_shim(tmp_path_factory, "kl_lr")
    lib.kl_lr_rule.argtypes = [C.c_float] * 4 + [C.c_void_p]
    lib.kl_lr_next.argtypes = [C.c_float, C.c_float, C.c_void_p]
    lib.kl_lr_next.restype = C.c_float
    lib.kl_lr_refusal.argtypes = [C.c_float] * 4
    lib.kl_lr_refusal.restype = C.c_char_p
    lib.kl_lr_words.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.adam_kl_scalars.argtypes = [C.c_uint64, C.POINTER(C.c_double)]
    lib.adam_kl_scalars.restype = C.c_float
    lib.adam_scalars.argtypes = [C.c_uint64, C.c_float, C.c_void_p]
    return lib


def bits(x):
    return np.asarray(x, F).view(np.uint32)


def c_rule(shim, *args):
    out = np.zeros(6, F)
    shim.kl_lr_rule(*args, out.ctypes.data_as(C.c_void_p))
    return out


def c_next(shim, lr, kl, rule):
    r = np.asarray(rule, F)
    return F(shim.kl_lr_next(float(lr), float(kl), r.ctypes.data_as(C.c_void_p)))


@pytest.mark.parametrize("args", [(0.01, 1.5, 1e-5, 1e-2), (0.005, 1.5, 1e-5, 1e-2), (1e-12, 3.0, 1e-6, 1.0), (1e3, 1.1, 3e-4, 3e-4),
                                  (0.02, 1.0, 1e-5, 1e-2), (0.0123, 7.0, 1e-7, 0.3)])
def test_band_and_down_from_the_public_arguments(shim, args):
    """kl_low = desired_kl / 2, kl_high = 2 desired_kl, up = factor, down = 1 / factor — each rounded once, in float32."""
    got, ref = c_rule(shim, *args), np.array(np_rule(*args), F)
    print(args, got, ref)
    assert np.array_equal(bits(got), bits(ref))


def test_the_rule_at_its_edges(shim):
    rule = np_rule(0.01)                                     # band 0.005 .. 0.02, factor 1.5, clamp 1e-5 .. 1e-2
    kl_low, kl_high, up, down, lr_min, lr_max = rule
    lr = F(3e-4)
    same = [kl_low, kl_high, F(0.01), 0.0, -0.0, -1e-3, -INF, NAN]           # strict inequalities at the band's ends; no step without a KL > 0
    for kl in same:
        assert bits(c_next(shim, lr, kl, rule)) == bits(lr), kl
    assert bits(c_next(shim, lr, np.nextafter(kl_high, F(1)), rule)) == bits(F(lr * down))
    assert bits(c_next(shim, lr, np.nextafter(kl_low, F(0)), rule)) == bits(F(lr * up))
    assert bits(c_next(shim, lr, INF, rule)) == bits(F(lr * down))
    assert bits(c_next(shim, lr, np.finfo(F).tiny, rule)) == bits(F(lr * up))
    # a step that would cross a bound ends exactly on it
    assert bits(c_next(shim, F(1.2e-5), 1.0, rule)) == bits(lr_min) and F(F(1.2e-5) * down) < lr_min
    assert bits(c_next(shim, F(9e-3), 1e-4, rule)) == bits(lr_max) and F(F(9e-3) * up) > lr_max
    assert bits(c_next(shim, lr_min, 1.0, rule)) == bits(lr_min) and bits(c_next(shim, lr_max, 1e-4, rule)) == bits(lr_max)
    # factor = 1: nothing ever moves; lr_min == lr_max: the rate is pinned
    one = np_rule(0.01, factor=1.0)
    for kl in (1.0, 1e-4, 0.01, INF):
        assert bits(c_next(shim, lr, kl, one)) == bits(lr)
    pinned = np_rule(0.01, lr_min=3e-4, lr_max=3e-4)
    for kl in (1.0, 1e-4, 0.01, NAN):
        assert bits(c_next(shim, lr, kl, pinned)) == bits(lr)


def test_the_rule_equals_its_numpy_restatement(shim):
    rng = np.random.default_rng(0)
    rule = np_rule(0.01, factor=1.5, lr_min=1e-5, lr_max=1e-2)
    lrs = np.exp(rng.uniform(np.log(1e-5), np.log(1e-2), 400)).astype(F)
    kls = np.exp(rng.uniform(np.log(1e-4), np.log(1.0), 400)).astype(F)
    got = np.array([c_next(shim, a, b, rule) for a, b in zip(lrs, kls)], F)
    ref = np.array([np_next(a, b, rule) for a, b in zip(lrs, kls)], F)
    assert np.array_equal(bits(got), bits(ref))
    assert (got < lrs).any() and (got > lrs).any() and (got == lrs).any()
    # a walk: down to the lower clamp and up again, the first minibatch of each update skipped
    walk = replay(1e-2, [5.0] * 20, rule)
    assert walk[0] == F(1e-2) and walk[1] == F(F(1e-2) * rule[3]) and walk[-1] == rule[4]


def test_refusals_name_the_argument(shim):
    r = lambda *a: shim.kl_lr_refusal(*a).decode()           # noqa: E731
    assert r(0.01, 1.5, 1e-5, 1e-2) == "" and r(0.01, 1.0, 3e-4, 3e-4) == ""
    for bad in (0.0, -1.0, INF, NAN):
        assert r(bad, 1.5, 1e-5, 1e-2).startswith("desired_kl")
    for bad in (0.99, 0.0, -2.0, INF, NAN):
        assert r(0.01, bad, 1e-5, 1e-2).startswith("factor")
    for bad in (0.0, -1e-5, NAN):
        assert r(0.01, 1.5, bad, 1e-2).startswith("lr_min must be > 0")
    assert r(0.01, 1.5, 1e-2, 1e-3).startswith("lr_min must be <= lr_max") and r(0.01, 1.5, 1e-5, NAN).startswith("lr_min must be <= lr_max")


@pytest.mark.parametrize("n", [1, 2, 3, 12])
def test_the_rate_never_reads_the_word_it_writes(shim, n):
    """The caller's word -> slots alternated by parity -> the caller's word: every minibatch reads what the one before wrote, writes
    another word than it reads, and the update ends in the caller's word."""
    w = np.zeros(2, np.int32)
    words = []
    for mb in range(n):
        shim.kl_lr_words(mb, int(mb == n - 1), w.ctypes.data_as(C.c_void_p))
        words.append((int(w[0]), int(w[1])))
    assert words[0][0] == 0 and all(a != b for a, b in words)
    assert all(words[i + 1][0] == words[i][1] for i in range(n - 1))
    assert words[-1][1] == (0 if n > 1 else -1)              # one minibatch: the rule does not act, the word already holds the rate


@pytest.mark.parametrize("step", [1, 2, 10, 1000, 10 ** 6, 2 ** 32 + 1])
def test_adam_scalars_with_the_rate_on_the_device(shim, step):
    """bc1 in double and bc2_sqrt: float(double(lr) / bc1) is wg_adam_scalars' step_size to the bit for any lr."""
    bc1 = C.c_double()
    bc2 = F(shim.adam_kl_scalars(step, C.byref(bc1)))
    assert bc1.value == 1.0 - np.float64(0.9) ** np.float64(step)
    for lr in (3e-4, 1e-5, 1e-2, 7.7e-4):
        ref = np.zeros(2, F)
        shim.adam_scalars(step, lr, ref.ctypes.data_as(C.c_void_p))
        assert bits(F(np.float64(F(lr)) / bc1.value)) == bits(ref[0]) and bits(bc2) == bits(ref[1])


# ---- the trainers' arguments, without a device -------------------------------------------------------------------------------------
ENV = dict(batch=types.SimpleNamespace(obs_dim=9), rollout=None, num_envs=4, n_turb=2)
BAD = [(dict(desired_kl=0.0), "desired_kl must be > 0"), (dict(desired_kl=-0.01), "desired_kl must be > 0"),
       (dict(desired_kl=INF), "desired_kl must be > 0 and finite"), (dict(desired_kl=NAN), "desired_kl must be > 0"),
       (dict(desired_kl=0.01, factor=0.9), "factor must be >= 1"), (dict(desired_kl=0.01, factor=INF), "factor must be >= 1 and finite"),
       (dict(desired_kl=0.01, lr_min=0.0), "lr_min must be > 0"), (dict(desired_kl=0.01, lr_min=1e-3, lr_max=1e-4), "lr_min must be <= lr_max"),
       (dict(desired_kl=0.01, lr_min=1e-3), "learning_rate = 0.0003, the starting rate"),
       (dict(desired_kl=0.01, lr_max=1e-4), "learning_rate = 0.0003, the starting rate"),
       (dict(factor=1.5), "needs desired_kl"), (dict(desired_kl=0.01, target=1), "unknown keys"), (0.01, "must be a dict")]


def trainers():
    from windgym_amd.population import PPOPopulation
    from windgym_amd.ppo import PPO
    from windgym_amd.recurrent_population import RecurrentPPOPopulation
    from windgym_amd.recurrent_ppo import RecurrentPPO
    env = types.SimpleNamespace(**ENV)
    return [lambda **kw: PPO("MlpPolicy", env, **kw), lambda **kw: RecurrentPPO("MlpLstmPolicy", env, **kw),
            lambda **kw: PPOPopulation("MlpPolicy", env, n_members=2, **kw),
            lambda **kw: RecurrentPPOPopulation("MlpLstmPolicy", env, n_members=2, **kw)]


@pytest.mark.parametrize("arg, says", BAD)
def test_trainers_refuse_a_bad_rule_by_name(arg, says):
    for make in trainers():
        with pytest.raises(ValueError, match=says):
            make(adaptive_lr=arg)


def test_trainers_refuse_a_schedule_with_the_rule():
    for make in trainers():
        with pytest.raises(ValueError, match="learning_rate is a schedule"):
            make(adaptive_lr=dict(desired_kl=0.01), learning_rate=lambda p: 3e-4 * p)


def test_population_rules_per_member():
    from windgym_amd.population import PPOPopulation, member_adaptive_lr
    rules = member_adaptive_lr(dict(desired_kl=[0.005, 0.02], lr_max=1e-3), [3e-4, 1e-4], 2)
    assert [r["desired_kl"] for r in rules] == [float(F(0.005)), float(F(0.02))]
    assert all(r["factor"] == 1.5 and r["lr_min"] == float(F(1e-5)) and r["lr_max"] == float(F(1e-3)) for r in rules)
    env = types.SimpleNamespace(**ENV)
    with pytest.raises(ValueError, match=r"adaptive_lr: desired_kl: 3 values for 2 members"):
        PPOPopulation("MlpPolicy", env, n_members=2, adaptive_lr=dict(desired_kl=[0.01, 0.02, 0.03]))
    with pytest.raises(ValueError, match=r"member 1: learning_rate = 0.05, the starting rate"):
        PPOPopulation("MlpPolicy", env, n_members=2, adaptive_lr=dict(desired_kl=0.01), learning_rate=[3e-4, 5e-2])
    with pytest.raises(ValueError, match=r"member 0: adaptive_lr: factor must be >= 1"):
        PPOPopulation("MlpPolicy", env, n_members=2, adaptive_lr=dict(desired_kl=0.01, factor=[0.5, 1.5]))


def _fake_checkpoint(path, **more):
    """write_checkpoint on a stand-in policy / optimiser / generator (no device)"""
    import torch

    from windgym_amd.ppo import write_checkpoint
    sd = {"log_std": torch.zeros(2)}
    pol = types.SimpleNamespace(desc=dict(n_in=6, n_out=2), seed=5, counter=9, state_dict=lambda: sd)
    opt = types.SimpleNamespace(state=lambda: (np.zeros(4, F), 12))
    hyper = dict(n_steps=16, batch_size=32, n_epochs=3, gamma=0.9, gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, vf_coef=0.5,
                 max_grad_norm=0.5, learning_rate=1e-3, normalize_advantage=True)
    write_checkpoint(path, pol, opt, torch.Generator(), hyper, 5, 384, 3, [], None, 48, **more)


def test_checkpoint_keeps_the_rule_and_the_rate_exactly(tmp_path):
    """The arguments under the JSON key adaptive_lr, the rate as a float32 npy member, both back to the bit."""
    import torch

    from windgym_amd.ppo import check_adaptive_lr, read_checkpoint
    rule = check_adaptive_lr(dict(desired_kl=0.01, lr_max=3e-3), 3e-4)
    assert rule == dict(desired_kl=float(F(0.01)), factor=1.5, lr_min=float(F(1e-5)), lr_max=float(F(3e-3)))
    lr = F(F(3e-4) * F(1.5) * F(1.5))                              # a rate no decimal literal of a few digits spells
    path = str(tmp_path / "k.zip")
    _fake_checkpoint(path, tensors={"learning_rate.npy": torch.from_numpy(np.array([lr], F))}, extra=dict(adaptive_lr=rule))
    meta, members = read_checkpoint(path)
    assert meta["adaptive_lr"] == rule and check_adaptive_lr(meta["adaptive_lr"], 3e-4) == rule
    got = members["learning_rate.npy"]
    assert got.dtype == F and got.shape == (1,) and bits(got)[0] == bits(lr)
    assert meta["hyper"]["learning_rate"] == 1e-3                # the starting rate stays in HYPER as given
    plain = str(tmp_path / "p.zip")
    _fake_checkpoint(plain)
    meta, members = read_checkpoint(plain)
    assert "adaptive_lr" not in meta and "learning_rate.npy" not in members
