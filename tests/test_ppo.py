"""CPU tests of the training layer: the oracle itself (GAE against its brute-force definition, Adam against torch.optim.Adam,
the loss on hand-computable rows), PPO's argument validation and SB3's initialisation.  The kernels are tested on the GPU
(tests/test_gpu_ppo.py); the ABI test (tests/test_abi.py) picks the new entries up from the header."""
import itertools
import math
import os
import re

import numpy as np
import pytest

from oracle import ppo_oracle as oo
from windgym_amd.policy import make_desc, param_layout
from windgym_amd.ppo import PPO, sb3_orthogonal_init


@pytest.mark.parametrize("T,B,p", [(1, 3, 0.5), (7, 5, 0.3), (40, 4, 0.0), (40, 4, 1.0)])
def test_gae_equals_its_definition(T, B, p):
    rng = np.random.default_rng(T + B)
    r, v, fv = (rng.standard_normal((T, B)) for _ in range(3))
    tr = rng.uniform(size=(T, B)) < p
    a, ret = oo.gae(r, v, fv, tr, 0.97, 0.9)
    b, ret_b = oo.gae_brute(r, v, fv, tr, 0.97, 0.9)
    assert np.allclose(a, b, rtol=1e-12, atol=1e-12) and np.allclose(ret, ret_b, rtol=1e-12, atol=1e-12)
    # a truncated step's advantage is its own delta; lambda = 0 makes every step so
    d = r + 0.97 * fv - v
    assert np.allclose(a[tr], d[tr])
    assert np.allclose(oo.gae(r, v, fv, tr, 0.97, 0.0)[0], d)


@pytest.mark.parametrize("max_norm", [0.1, 1e9])
def test_oracle_adam_equals_torch_adam(max_norm):
    import torch
    rng = np.random.default_rng(0)
    w = torch.tensor(rng.standard_normal(50), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([w], lr=1e-2, eps=1e-5)
    p, m, v = w.detach().numpy().copy(), np.zeros(50), np.zeros(50)
    for step in range(1, 8):
        g = rng.standard_normal(50)
        w.grad = torch.tensor(g)
        torch.nn.utils.clip_grad_norm_([w], max_norm)
        opt.step()
        p, m, v = oo.adam_step(p, g, m, v, step, 1e-2, max_norm)
        assert np.allclose(w.detach().numpy(), p, rtol=1e-12, atol=1e-13), step


def _tiny():
    """n_in 1 -> n_out 1 with no hidden layers: mean = w x + b, V = u x + c."""
    return {"action_net.weight": np.array([[2.0]]), "action_net.bias": np.array([0.5]), "value_net.weight": np.array([[-1.0]]),
            "value_net.bias": np.array([0.25]), "log_std": np.array([math.log(0.5)])}


def test_loss_pieces_on_hand_computable_rows():
    sd = _tiny()
    obs = np.array([[1.0], [0.0], [-1.0]])
    mean = np.array([2.5, 0.5, -1.5])
    raw = (mean + 0.5 * np.array([0.0, 1.0, -2.0]))[:, None]             # z = 0, 1, -2
    logp = -0.5 * np.array([0.0, 1.0, 4.0]) - math.log(0.5) - 0.5 * math.log(2 * math.pi)
    ratio = np.array([1.0, 1.5, 0.5])
    logp_old = logp - np.log(ratio)
    adv, ret = np.array([1.0, 2.0, -1.0]), np.array([0.0, 1.0, 2.0])
    total, grads, st, r = oo.loss_and_grad(sd, obs, raw, logp_old, adv, ret, clip_range=0.2, vf_coef=0.5, ent_coef=0.1,
                                           normalize_advantage=False)
    assert np.allclose(r, ratio)
    l_pi = -np.minimum(ratio * adv, np.clip(ratio, 0.8, 1.2) * adv)       # -1, -2.4, +0.8 (the pessimistic branch)
    assert np.allclose(l_pi, [-1.0, -2.4, 0.8]) and math.isclose(st["pi_loss"], l_pi.mean())
    V = np.array([-0.75, 0.25, 1.25])
    assert math.isclose(st["v_loss"], ((ret - V) ** 2).mean())
    H = 0.5 + 0.5 * math.log(2 * math.pi) + math.log(0.5)
    assert math.isclose(st["entropy"], H) and math.isclose(total, l_pi.mean() + 0.5 * st["v_loss"] - 0.1 * H)
    assert math.isclose(st["clip_fraction"], 2 / 3) and math.isclose(st["approx_kl"], ((ratio - 1) - np.log(ratio)).mean())
    # row 1 is clipped from above with a positive advantage: no gradient; row 2 (ratio 0.5, negative advantage) neither; only
    # row 0 moves the actor: d/d mean = -A ratio z / std / n = 0 there (z = 0) -> the actor's weight gradient vanishes
    assert np.allclose(grads["action_net.weight"], 0.0) and np.allclose(grads["action_net.bias"], 0.0)
    assert np.allclose(grads["log_std"], -(1.0 * 1.0 * (0.0 - 1.0)) / 3 - 0.1)          # -A ratio (z^2 - 1) / n - ent_coef
    assert np.allclose(grads["value_net.bias"], 0.5 * np.mean(2 * (V - ret)))
    # normalisation uses the unbiased std
    _, _, st2, _ = oo.loss_and_grad(sd, obs, raw, logp, adv, ret, normalize_advantage=True)
    a = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    assert math.isclose(st2["pi_loss"], -a.mean(), abs_tol=1e-12)


class _FakeEnv:
    num_envs = 8


def test_ppo_argument_validation():
    for kw in (dict(target_kl=0.01), dict(clip_range_vf=0.2), dict(use_sde=True)):
        with pytest.raises(NotImplementedError):
            PPO("MlpPolicy", _FakeEnv(), **kw)
    for kw in (dict(n_steps=0), dict(n_epochs=0), dict(gamma=1.5), dict(gae_lambda=-0.1), dict(max_grad_norm=0.0),
               dict(batch_size=0), dict(n_steps=4, batch_size=33), dict(learning_rate=-1.0), dict(clip_range=-0.1)):
        with pytest.raises(ValueError):
            PPO("MlpPolicy", _FakeEnv(), **kw)
    with pytest.raises(ValueError):
        PPO("CnnPolicy", _FakeEnv())


def test_sb3_orthogonal_init():
    desc = make_desc(32, 16, (64, 48), (64, 64))
    a, b = sb3_orthogonal_init(desc, 7), sb3_orthogonal_init(desc, 7)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["action_net.weight"], sb3_orthogonal_init(desc, 8)["action_net.weight"])
    for name, shape in param_layout(desc):
        w = a[name].astype(np.float64)
        assert w.shape == tuple(shape)
        if w.ndim == 1:
            assert not w.any()
            continue
        gain = 0.01 if name == "action_net.weight" else 1.0 if name == "value_net.weight" else math.sqrt(2.0)
        g = w @ w.T if w.shape[0] <= w.shape[1] else w.T @ w              # the short side is orthonormal up to the gain
        assert np.allclose(g, gain * gain * np.eye(g.shape[0]), atol=1e-5), name


def test_checkpoint_policy_member_reads_back(tmp_path):
    """The zip layout of PPO.save: policy.pth under SB3's names is what read_sb3_zip reads (the GPU test saves a real one)."""
    import io
    import zipfile

    import torch

    from windgym_amd.policy import read_sb3_zip
    desc = make_desc(6, 2, (8,), (8, 4))
    sd = sb3_orthogonal_init(desc, 1)
    sd["log_std"] = np.array([-0.3, 0.1], np.float32)
    b = io.BytesIO()
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, b)
    path = tmp_path / "p.zip"
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", b.getvalue())
        z.writestr("windgym_ppo.json", "{}")
    d2, t2 = read_sb3_zip(path)
    assert d2 == desc and all(np.array_equal(t2[k], sd[k]) for k in sd)


def _fake_checkpoint(path, learning_rate=1e-3, **extra):
    """write_checkpoint on a fake policy / optimiser / generator (no device) -> what was written, by member"""
    import torch
    desc = make_desc(6, 2, (8,), (8,))
    sd = {k: torch.from_numpy(v) for k, v in sb3_orthogonal_init(desc, 3).items()}
    pol = type("Pol", (), dict(desc=desc, seed=5, counter=9, state_dict=lambda self: sd))()
    mv = np.arange(2 * sum(v.numel() for v in sd.values()), dtype=np.float32) * 0.5
    opt = type("Opt", (), dict(state=lambda self: (mv, 12)))()
    g = torch.Generator()
    g.manual_seed(5)
    hyper = dict(n_steps=16, batch_size=32, n_epochs=3, gamma=0.9, gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, vf_coef=0.5,
                 max_grad_norm=0.5, learning_rate=learning_rate, normalize_advantage=True)
    log = [dict(iteration=1, loss=0.5)]
    from windgym_amd.ppo import write_checkpoint
    write_checkpoint(path, pol, opt, g, hyper, 5, 384, 3, log, "agent", 48, **extra)
    return dict(sd=sd, mv=mv, gen=g.get_state().numpy(), hyper=hyper, log=log, desc=desc)


def test_checkpoint_round_trip_without_a_device(tmp_path):
    """write_checkpoint -> read_checkpoint: the JSON, every npy member as the array and every other member as the bytes that went in."""
    import io
    import types

    import torch

    from windgym_amd.ppo import read_checkpoint
    path = str(tmp_path / "a.zip")
    cur = types.SimpleNamespace(args=lambda: dict(n_passes=2), state=lambda: b"curriculum-blob")
    vn = types.SimpleNamespace(args=lambda: dict(gamma=0.9), state=lambda: b"\x00norm\xff")
    state = torch.arange(24, dtype=torch.float32).reshape(2, 2, 3, 2) / 7
    w = _fake_checkpoint(path, curriculum=cur, normalize=vn, tensors={"lstm_state.npy": state})
    meta, members = read_checkpoint(path, needs=("lstm_state.npy",))
    assert set(members) == {"policy.pth", "adam_state.npy", "generator_state.npy", "curriculum_state.bin", "normalize_state.bin",
                            "lstm_state.npy"}
    assert members["lstm_state.npy"].dtype == np.float32 and np.array_equal(members["lstm_state.npy"], state.numpy())
    assert members["adam_state.npy"].dtype == np.float32 and np.array_equal(members["adam_state.npy"], w["mv"])
    assert members["generator_state.npy"].dtype == w["gen"].dtype and np.array_equal(members["generator_state.npy"], w["gen"])
    assert members["curriculum_state.bin"] == b"curriculum-blob" and members["normalize_state.bin"] == b"\x00norm\xff"
    sd = torch.load(io.BytesIO(members["policy.pth"]))
    assert set(sd) == set(w["sd"]) and all(torch.equal(sd[k], w["sd"][k]) for k in sd)
    assert meta["hyper"] == w["hyper"] and meta["desc"] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in w["desc"].items()}
    assert (meta["format"], meta["seed"], meta["policy_seed"], meta["policy_counter"]) == ("windgym_amd.PPO/1", 5, 5, 9)
    assert (meta["num_timesteps"], meta["iteration"], meta["adam_step"], meta["env_policy_steps"]) == (384, 3, 12, 48)
    assert meta["log"] == w["log"] and meta["critic"] == "agent"
    assert meta["curriculum"] == dict(n_passes=2) and meta["normalize"] == dict(gamma=0.9)
    # a plain one has neither blob nor key, and arguments passed to load() win over stored numbers
    plain = str(tmp_path / "b.zip")
    _fake_checkpoint(plain)
    meta, members = read_checkpoint(plain, learning_rate=0.5)
    assert set(members) == {"policy.pth", "adam_state.npy", "generator_state.npy"} and "curriculum" not in meta and "normalize" not in meta
    assert meta["hyper"]["learning_rate"] == 0.5 and meta["hyper"]["clip_range"] == 0.2


def test_checkpoint_schedules_and_refusals(tmp_path):
    import zipfile

    from windgym_amd.ppo import read_checkpoint
    from windgym_amd.recurrent_ppo import RecurrentPPO
    path = str(tmp_path / "s.zip")
    _fake_checkpoint(path, learning_rate=lambda p: 1e-3 * p)
    with pytest.raises(ValueError, match=r"^the checkpoint was trained with a learning_rate schedule: pass it to load\(\)$"):
        read_checkpoint(path)
    with pytest.raises(ValueError, match=r"^the checkpoint was trained with a learning_rate schedule: pass it to load\(\)$"):
        PPO.load(path, None)
    sched = lambda p: 2e-3 * p                                   # noqa: E731
    meta, _ = read_checkpoint(path, learning_rate=sched)
    assert meta["hyper"]["learning_rate"] is sched
    # PPO's zip has no lstm_state.npy: RecurrentPPO.load refuses it by name, PPO.load a zip without the JSON
    with pytest.raises(ValueError) as e:
        RecurrentPPO.load(path, None, learning_rate=sched)
    assert str(e.value) == ("not a windgym_amd RecurrentPPO checkpoint (an sb3-contrib zip loads with MlpLstmPolicy.from_sb3_zip, "
                            "a PPO checkpoint with PPO.load)")
    other = str(tmp_path / "o.zip")
    with zipfile.ZipFile(other, "w") as z:
        z.writestr("policy.pth", b"")
    with pytest.raises(ValueError) as e:
        PPO.load(other, None)
    assert str(e.value) == "not a windgym_amd PPO checkpoint (for an SB3 zip use MlpPolicy.from_sb3_zip)"


def _defines(header):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, *header)).read()
    return {k: int(v) for k, v in re.findall(r"^#define\s+(\w+)\s+(\d+)\b", text, flags=re.M)}


def test_row_tile_of_every_legal_architecture_corner():
    """k_ppo_grad's row tile R (wg_ppo.h: 32 when a net's activations fit the workgroup's LDS, else 16, 8, 4 or 2) over the corners
    of what wg_policy_create accepts — n_in, widths and depths of both nets, n_out at their smallest, largest and either side of
    the 256-input chunk.  R = 32, 16, 8 and 4 occur.  Only an ACTOR of four hidden layers of 256 reaches R = 4, and only with
    n_out + min(n_in, 256) > 266 (its map is (min(n_in, 256) + 1024 + n_out + 512) (R + 1) + 160 floats); a critic of that depth stays
    at R = 8 whatever n_in is (256 + 1024 + 1 + 512 = 1793 <= 1802).  R = 2 is unreachable inside the limits: no map exceeds the
    budget."""
    pol, ppo, api = (_defines(h) for h in (("windgym_amd", "csrc", "wg_policy.h"), ("windgym_amd", "csrc", "wg_ppo.h"), ("include", "windgym_hip.h")))
    pol.update(_defines(("windgym_amd", "csrc", "wg_tile.h")))        # (the tile constants: WGP_KC)
    KC, W, OUT, IN, H, LDS = pol["WGP_KC"], pol["WGP_MAX_WIDTH"], pol["WGP_MAX_OUT"], pol["WGP_MAX_IN"], api["WG_POLICY_MAX_HIDDEN"], ppo["WGT_LDS_BYTES"]
    assert (KC, W, OUT, IN, H, LDS) == (256, 256, 128, 2048, 4, 65536) and pol["WGP_MAX_LAYERS"] == H + 1
    stacks = [()] + [(w,) * n for n in range(1, H + 1) for w in (1, 33, 64, W)] + [(W, 1, W, 1), (1, W), (64, W, 64)]
    seen = {}
    for n_in, n_out, pi, vf in itertools.product((1, 32, KC - 1, KC, KC + 1, IN), (1, 16, 33, OUT), stacks, stacks):
        R, need = oo.tile_rows(n_in, n_out, pi, vf, LDS, KC)
        assert R is not None and need <= LDS, (n_in, n_out, pi, vf)
        if R < 32:                                             # the next larger tile did not fit: R is the largest that does
            assert 4 * max(oo.lds_floats(n_in, list(w) + [o], 2 * R, KC) for w, o in ((pi, n_out), (vf, 1))) > LDS
        seen.setdefault(R, []).append((n_in, n_out, pi, vf))
    assert sorted(seen) == [4, 8, 16, 32], sorted(seen)
    for R, shapes in seen.items():
        for n_in, n_out, pi, vf in shapes:
            assert (R == 4) == (pi == (W,) * H and n_out + min(n_in, KC) > 266), (R, n_in, n_out, pi, vf)
    # the worst case of the limits, by hand: (256 + 4 * 256 + 128 + 2 * 256) * 5 + 160 floats at R = 4
    assert oo.tile_rows(IN, OUT, (W,) * H, (W,) * H, LDS, KC) == (4, 4 * (1920 * 5 + 160))
    # and the shapes the GPU tests name in their ids
    assert oo.tile_rows(8, 4, (64, 64), (64, 64))[0] == 32 and oo.tile_rows(1600, 16, (256, 256), (256, 256))[0] == 8
    assert oo.tile_rows(200, 2, (128, 128, 128), (128, 128, 128))[0] == 16
    assert oo.tile_rows(256, 16, (W,) * H, (W,) * H)[0] == 4 and oo.tile_rows(256, 16, (W,) * H, (64, 64))[0] == 4
    assert oo.tile_rows(256, 16, (64, 64), (W,) * H)[0] == 8 and oo.tile_rows(32, 16, (64, 64), (W,) * H)[0] == 8
