"""CPU tests of the learned-policy layer: SB3 checkpoint reader, flat parameter order, oracle, ctypes mirrors, noise stream."""
import ctypes as C
import io
import json
import os
import zipfile

import numpy as np
import pytest

from helpers import c_layout
from oracle import policy_oracle as po
from windgym_amd import policy as pol
from windgym_amd.binding import CPolicyDesc, CRolloutBufs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ppo_2975000_policy.npz")
NON_TENSORS = ("last_obs", "mean64", "value64", "meta")


def fixture():
    z = np.load(FIX, allow_pickle=False)
    return z, {k: z[k] for k in z.files if k not in NON_TENSORS}


def write_zip(path, tensors, data=None):
    import torch
    buf = io.BytesIO()
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in tensors.items()}, buf)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf.getvalue())
        z.writestr("data", json.dumps(data if data is not None else {"use_sde": False}))
        z.writestr("_stable_baselines3_version", "2.3.2")
    return str(path)


def test_read_sb3_zip_roundtrip(tmp_path):
    _, t = fixture()
    desc, out = pol.read_sb3_zip(write_zip(tmp_path / "m.zip", t))
    assert (desc["n_in"], desc["n_out"], desc["hidden_pi"], desc["hidden_vf"]) == (8, 4, (64, 64), (64, 64))
    assert desc["has_log_std"] and desc["activation"] == "tanh"
    assert set(out) == set(t)
    for k in t:
        assert np.array_equal(out[k], t[k]), k


def test_read_sb3_zip_never_unpickles(tmp_path, monkeypatch):
    import pickle
    _, t = fixture()

    def boom(*a, **k):
        raise AssertionError("unpickled")

    data = {"use_sde": False, "policy_class": {":type:": "<class 'abc.ABCMeta'>", ":serialized:": "gAWVAAAA"}}
    path = write_zip(tmp_path / "m.zip", t, data)      # (written before the patch: torch.save pickles)
    monkeypatch.setattr(pickle, "loads", boom)
    monkeypatch.setattr(pickle, "load", boom)
    try:
        import cloudpickle
        monkeypatch.setattr(cloudpickle, "loads", boom)
        monkeypatch.setattr(cloudpickle, "load", boom)
    except ImportError:
        pass
    desc, out = pol.read_sb3_zip(path)
    assert desc["n_in"] == 8 and np.array_equal(out["log_std"], t["log_std"])


def test_read_sb3_zip_refusals(tmp_path):
    _, t = fixture()
    with pytest.raises(ValueError, match="use_sde"):
        pol.read_sb3_zip(write_zip(tmp_path / "a.zip", t, {"use_sde": True}))
    with pytest.raises(ValueError, match="shared"):
        pol.read_sb3_zip(write_zip(tmp_path / "b.zip", dict(t, **{"mlp_extractor.shared_net.0.weight": np.zeros((4, 8), np.float32)})))
    with pytest.raises(ValueError, match="feature extractor"):
        pol.read_sb3_zip(write_zip(tmp_path / "c.zip", dict(t, **{"features_extractor.cnn.0.weight": np.zeros((4, 8), np.float32)})))
    miss = {k: v for k, v in t.items() if k != "action_net.bias"}
    with pytest.raises(ValueError, match="missing"):
        pol.read_sb3_zip(write_zip(tmp_path / "d.zip", miss))
    miss = {k: v for k, v in t.items() if k != "mlp_extractor.value_net.2.bias"}
    with pytest.raises(ValueError, match="missing"):
        pol.read_sb3_zip(write_zip(tmp_path / "e.zip", miss))
    bad = dict(t, **{"mlp_extractor.policy_net.2.weight": np.zeros((64, 63), np.float32)})
    with pytest.raises(ValueError, match="chain"):
        pol.read_sb3_zip(write_zip(tmp_path / "f.zip", bad))
    with pytest.raises(ValueError, match="activation"):
        pol.read_sb3_zip(write_zip(tmp_path / "g.zip", t), activation="gelu")


def test_oracle_reproduces_fixture_fp64():
    z, t = fixture()
    mean, value = po.forward(t, z["last_obs"])
    assert np.abs(mean - z["mean64"]).max() < 1e-12
    assert np.abs(value - z["value64"]).max() < 1e-12
    s = po.sample(t, z["last_obs"])
    assert np.array_equal(s["raw"], s["mean"]) and np.abs(s["action"]).max() <= 1.0
    assert np.allclose(s["logp"], np.sum(-t["log_std"].astype(np.float64) - 0.5 * np.log(2 * np.pi)))


@pytest.mark.parametrize("n_in,hp,hv,n_out,ls", [(7, (33,), (5, 3), 1, True), (8, (), None, 4, False), (200, (128, 128, 128), (1,), 2, True)])
def test_flat_parameter_order_roundtrip(n_in, hp, hv, n_out, ls):
    desc = pol.make_desc(n_in, n_out, hp, hv, "relu", ls)
    dims = [n_in, *hp, n_out]
    n = sum(a * b + b for a, b in zip(dims[:-1], dims[1:]))
    if hv is not None:
        dims = [n_in, *hv, 1]
        n += sum(a * b + b for a, b in zip(dims[:-1], dims[1:]))
    n += n_out if ls else 0
    assert pol.n_params(desc) == n
    flat = np.arange(n, dtype=np.float32)
    t = pol.unpack_params(desc, flat)
    assert np.array_equal(pol.pack_params(desc, t), flat)
    names = [k for k, _ in pol.param_layout(desc)]
    assert names[0] == ("mlp_extractor.policy_net.0.weight" if hp else "action_net.weight")
    assert names[-1] == ("log_std" if ls else ("value_net.bias" if hv is not None else "action_net.bias"))
    first = t[names[0]]
    assert first[0, 1] == 1.0 and first[1, 0] == float(n_in)          # W row-major [out][in]
    with pytest.raises(ValueError):
        pol.unpack_params(desc, flat[:-1])


@pytest.mark.parametrize("cls,cname", [(CPolicyDesc, "wg_policy_desc"), (CRolloutBufs, "wg_rollout_bufs")])
def test_policy_struct_layouts_match_c(tmp_path, cls, cname):
    """sizeof / offsetof as gcc sees them == the ctypes mirrors."""
    fields = [f[0] for f in cls._fields_]
    got = c_layout(cname, fields, tmp_path)
    assert got["sizeof"] == C.sizeof(cls)
    for f in fields:
        assert got[f] == getattr(cls, f).offset, f


def test_policy_noise_stream(oracle_lib):
    # the numpy Philox restatement against the C one of oracle/philox.h
    L = oracle_lib.lib()
    ctr, key, out = (C.c_uint32 * 4)(1, 2, 3, 4), (C.c_uint32 * 2)(5, 6), (C.c_uint32 * 4)()
    L.wgo_rng_philox(ctr, key, out)
    mine = po.philox4x32_10(np.array([[1, 2, 3, 4]], np.uint32), np.array([[5, 6]], np.uint32))[0]
    assert list(out) == [int(v) for v in mine]
    rows = np.arange(12500)
    e = po.policy_noise(7, 3, rows, 8)
    assert e.dtype == np.float32 and e.shape == (12500, 8)
    assert np.array_equal(e, po.policy_noise(7, 3, rows, 8))
    base = po.policy_noise(7, 3, [0, 1], 4)
    assert not np.array_equal(base[0], base[1])                                        # row
    assert not np.array_equal(base, po.policy_noise(8, 3, [0, 1], 4))                  # seed lo
    assert not np.array_equal(base, po.policy_noise(7 + (1 << 32), 3, [0, 1], 4))      # seed hi
    assert not np.array_equal(base, po.policy_noise(7, 4, [0, 1], 4))                  # counter lo
    assert not np.array_equal(base, po.policy_noise(7, 3 + (1 << 32), [0, 1], 4))      # counter hi
    assert not np.array_equal(base, po.policy_noise(7, 3, [1 << 32, (1 << 32) + 1], 4))  # row hi
    assert len(np.unique(base[0])) == 4                                                # output index
    # rows [100, 101] of a batch == rows [0, 1] at row_offset 100
    assert np.array_equal(po.policy_noise(7, 3, [100, 101], 4), po.policy_noise(7, 3, np.arange(102), 4)[100:])
    n = e.size
    assert abs(e.mean()) < 3.0 / np.sqrt(n)
    assert abs(e.var() - 1.0) < 3.0 * np.sqrt(2.0 / n)
    assert abs(np.mean(e[:, 0] * e[:, 1])) < 3.0 / np.sqrt(len(rows))                   # the two Box-Muller branches


def test_mlp_policy_needs_a_gpu():
    import torch
    from windgym_amd.binding import WindGymHipError
    if torch.cuda.is_available():
        pol.MlpPolicy(8, 4).close()
        return
    with pytest.raises(WindGymHipError):
        pol.MlpPolicy(8, 4)
