"""GPU tests of k_policy, the wg_policy_* ABI, MlpPolicy and WindFarmVecEnv.rollout."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rl_helpers
from oracle import policy_oracle as po
from rl_helpers import LIMIT_SHAPES, _torch, _venv, close, rollout_equals_the_loop, shape4, shape_id

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ppo_2975000_policy.npz")

SHAPES = [(8, (64, 64), 4), (32, (64, 64), 16), (7, (33,), 1), (200, (128, 128, 128), 2), (1600, (256, 256), 16),
          (160, (64, 64), 80), (32, (), 16)]
make = functools.partial(rl_helpers.make, draw="normal")        # this file's cases were written for normal biases
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("shape", SHAPES + LIMIT_SHAPES, ids=shape_id)
def test_kernel_vs_oracle_deterministic(shape, activation):
    t = _torch()
    n_in, hidden, hidden_vf, n_out = shape4(shape)
    p, sd = make(n_in, hidden, n_out, activation, hidden_vf=hidden_vf)
    rng = np.random.default_rng(11)
    for rows in (1, 389, 4096):
        x = rng.uniform(-1, 1, (rows, n_in)).astype(np.float32)
        xd = t.from_numpy(x).cuda()
        a, raw, logp, v = (o.cpu().numpy() for o in p.act(xd, deterministic=True))
        ref = po.sample(sd, x, activation=activation)
        assert close(raw, ref["raw"]) and close(a, ref["action"]), (rows, np.abs(raw - ref["raw"]).max())
        assert close(v, ref["value"], 2e-5, 2e-5), (rows, np.abs(v - ref["value"]).max())
        assert close(logp, ref["logp"], 1e-4)
        mean_t, v_t = p.torch_forward(xd)
        assert close(raw, mean_t.detach().cpu().numpy()) and close(v, v_t.detach().cpu().numpy(), 2e-5, 2e-5)
    p.close()


def test_shipped_checkpoint():
    from windgym_amd.policy import MlpPolicy
    t = _torch()
    z = np.load(FIX, allow_pickle=False)
    sd = {k: z[k] for k in z.files if k not in ("last_obs", "mean64", "value64", "meta")}
    p = MlpPolicy(8, 4).load_state_dict(sd)
    a, raw, _, v = p.act(t.from_numpy(z["last_obs"]).cuda(), deterministic=True)
    assert close(raw.cpu().numpy(), z["mean64"]) and close(v.cpu().numpy(), z["value64"], 2e-5, 2e-5)
    act, state = p.predict(z["last_obs"][0], deterministic=True)
    assert state is None and act.shape == (4,) and act.dtype == np.float32 and np.all(np.abs(act) <= 1.0)
    assert close(act, np.clip(z["mean64"][0], -1, 1))
    assert p.predict(z["last_obs"])[0].shape == (16, 4)
    p.close()


def test_stochastic_against_oracle_and_row_independence():
    t = _torch()
    p, sd = make(32, (64, 64), 16)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (4096, 32)).astype(np.float32)
    xd = t.from_numpy(x).cuda()
    full = [o.clone() for o in p.act(xd, counter=9, seed=1234, row_offset=0)]
    eps = po.policy_noise(1234, 9, np.arange(4096), 16)
    ref = po.sample(sd, x, eps=eps)
    a, raw, logp, v = (o.cpu().numpy() for o in full)
    assert close(raw, ref["raw"], 1e-5 + 2e-5) and np.array_equal(a, np.clip(raw, -1, 1)) and close(logp, ref["logp"], 1e-4)
    again = p.act(xd, counter=9, seed=1234)
    assert all(t.equal(u, w) for u, w in zip(full, again))
    other = p.act(xd, counter=10, seed=1234)
    assert not t.equal(full[1], other[1]) and t.equal(full[3], other[3])
    # rows 0..388 of the full call == a 389-row call; rows 100..199 == a 100-row call at row_offset 100 (bitwise)
    part = p.act(xd[:389].contiguous(), counter=9, seed=1234)
    assert all(t.equal(u[:389], w) for u, w in zip(full, part))
    part = p.act(xd[100:200].contiguous(), counter=9, seed=1234, row_offset=100)
    assert all(t.equal(u[100:200], w) for u, w in zip(full, part))
    p.close()


@pytest.mark.parametrize("shape", LIMIT_SHAPES, ids=shape_id)
def test_stochastic_against_oracle_at_the_limits(shape):
    """Samples, log-probabilities and values of a stochastic call at the architecture limits, at a row offset and a counter that
    use the high words of the noise stream's counter (global rows beyond 2^32)."""
    t = _torch()
    n_in, hidden, hidden_vf, n_out = shape4(shape)
    p, sd = make(n_in, hidden, n_out, "tanh", hidden_vf=hidden_vf)
    rows, row0, counter, seed = 389, (3 << 32) + 123457, (1 << 40) + 17, (0xABCDEF << 32) | 99
    x = np.random.default_rng(6).uniform(-1, 1, (rows, n_in)).astype(np.float32)
    a, raw, logp, v = (o.cpu().numpy() for o in p.act(t.from_numpy(x).cuda(), counter=counter, seed=seed, row_offset=row0))
    ref = po.sample(sd, x, eps=po.policy_noise(seed, counter, row0 + np.arange(rows), n_out))
    assert close(raw, ref["raw"], 1e-5 + 2e-5), np.abs(raw - ref["raw"]).max()
    assert np.array_equal(a, np.clip(raw, -1, 1)) and close(logp, ref["logp"], 1e-4), np.abs(logp - ref["logp"]).max()
    assert close(v, ref["value"], 2e-5, 2e-5), np.abs(v - ref["value"]).max()
    p.close()


def test_params_on_device_and_sync():
    t = _torch()
    p, sd = make(8, (64, 64), 4)
    x = np.random.default_rng(2).uniform(-1, 1, (64, 8)).astype(np.float32)
    xd = t.from_numpy(x).cuda()
    before = p.act(xd, deterministic=True)[1].clone()
    with t.no_grad():
        p.params.mul_(0.5)
    assert t.equal(p.act(xd, deterministic=True)[1], before)          # the kernel reads its packed copy
    p.sync()
    sd2 = {k: v.cpu().numpy() for k, v in p.state_dict().items()}
    ref = po.sample(sd2, x)
    got = p.act(xd, deterministic=True)
    assert close(got[1].cpu().numpy(), ref["raw"]) and close(got[3].cpu().numpy(), ref["value"], 2e-5, 2e-5)
    assert not t.equal(got[1], before)
    p.close()


def test_rollout_equals_the_loop():
    t = _torch()
    va, vb = _venv(), _venv()
    O, N, T = va.batch.obs_dim, va.n_turb, 300
    p, _ = make(O, (64, 64), N)
    out = rollout_equals_the_loop(va, vb, p, T)
    obs0, raw0 = out["obs"][0].clone(), out["raw"][0].clone()              # (the buffers are reused by the next rollout)
    # the next rollout draws fresh noise
    out2 = va.rollout(p, 2)
    assert not t.equal(out2["raw"][0] - p.torch_forward(out2["obs"][0])[0].detach(), raw0 - p.torch_forward(obs0)[0].detach())
    va.close(); vb.close(); p.close()


def test_per_agent_rows_on_fused_multi_buffer():
    t = _torch()
    v = _venv(16)
    buf = v.batch.fuse_obs_multi()
    v.step(t.zeros((16, v.n_turb), device="cuda"))
    om = v.batch.obs_dim_multi
    p, sd = make(om, (32,), 1)
    a, raw, _, val = p.act(buf, deterministic=True)
    assert a.shape == (16 * v.n_turb, 1)
    ref = po.sample(sd, buf.cpu().numpy().reshape(-1, om))
    assert close(raw.cpu().numpy(), ref["raw"]) and close(val.cpu().numpy(), ref["value"], 2e-5, 2e-5)
    v.close(); p.close()


def test_argument_errors():
    from windgym_amd.policy import MlpPolicy
    t = _torch()
    with pytest.raises(NotImplementedError, match="2048"):
        MlpPolicy(4096, 4)
    with pytest.raises(NotImplementedError, match="128"):
        MlpPolicy(8, 200)
    with pytest.raises(NotImplementedError, match="256"):
        MlpPolicy(8, 4, (512,), (64,))
    nols = MlpPolicy(8, 4, (16,), None, has_log_std=False)
    x = t.zeros((5, 8), device="cuda")
    assert nols.act(x, deterministic=True)[3] is None
    with pytest.raises(ValueError, match="log_std"):
        nols.act(x, deterministic=False)
    with pytest.raises(ValueError, match="critic"):
        nols.value(x)
    with pytest.raises(ValueError):
        nols.act(t.zeros((5, 9), device="cuda"))
    v = _venv(8)
    with pytest.raises(ValueError, match="policy maps"):
        v.rollout(nols, 4)
    ok = MlpPolicy(v.batch.obs_dim, v.n_turb, (16,), None, has_log_std=False)
    with pytest.raises(ValueError, match="log_std"):
        v.rollout(ok, 4, deterministic=False)
    out = v.rollout(ok, 4, deterministic=True)
    assert "value" not in out and "logp" not in out and out["obs"].shape[0] == 5
    with pytest.raises(ValueError, match="unknown info"):
        v.rollout(ok, 4, deterministic=True, record=("nope",))
    v.close(); ok.close(); nols.close()


def test_bench_policy_cli_reports_the_policy_legs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_policy.py"), "--envs", "256", "--api-steps", "100",
                        "--preroll", "20"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    api = json.loads(lines[0])
    for leg in ("abi", "vecenv_torch", "closed_loop_torch_policy", "closed_loop_hip_policy", "rollout_hip_policy"):
        assert api[leg]["value"] > 0, leg
        assert leg == "abi" or api[leg]["frac_of_abi"] > 0, leg


class _PredictOnly:
    """Forwards predict() only: eval_sweep then takes the host loop."""

    def __init__(self, p):
        self._p = p

    def predict(self, obs, **kw):
        return self._p.predict(obs, **kw)


def test_eval_sweep_device_path_equals_host_loop():
    from windgym_amd import presets
    from windgym_amd.evaluate import eval_sweep
    from windgym_amd.policy import MlpPolicy
    from windgym_amd.turbine import V80
    z = np.load(FIX, allow_pickle=False)
    sd = {k: z[k] for k in z.files if k not in ("last_obs", "mean64", "value64", "meta")}
    p = MlpPolicy(8, 4).load_state_dict(sd)
    cfg = presets.env1_config()
    kw = dict(yaml_dict=cfg, winddirs=(260.0, 270.0, 280.0), windspeeds=(8.0, 11.0), t_sim=40, turbtype="Random", seed=1)
    dev = eval_sweep(V80(), None, p, **kw)
    host = eval_sweep(V80(), None, _PredictOnly(p), **kw)
    dd, hd = (d["data"] if isinstance(d, dict) else {k: d[k].values for k in d.data_vars} for d in (dev, host))
    assert set(dd) == set(hd) and "pct_inc" in dd
    for k in hd:
        assert np.array_equal(dd[k], hd[k]), k
    tc = (lambda d: np.asarray(d["coords"]["time"]) if isinstance(d, dict) else d["time"].values)
    assert np.array_equal(tc(dev), tc(host))
    assert np.all(dd["reward"][0] == 0.0) and np.any(dd["reward"][1:] != 0.0)
    assert dd["yaw_a"].min() >= cfg["farm"]["yaw_min"] and dd["yaw_a"].max() <= cfg["farm"]["yaw_max"]
    assert np.any(dd["yaw_a"][-1] != dd["yaw_a"][0])
    p.close()
