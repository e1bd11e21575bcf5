"""bench.py's launch contract on a box without GPUs: a GPU count that cannot run is an error, never a line; and what
--dump-outputs writes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=300, env=e)


def test_more_gpus_than_visible_fails_loudly():
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        return          # an 8-GPU node really runs it; covered by the driver's scaling run
    r = _run("--gpus", "2", "--steps", "2", "--warmup", "1")
    assert r.returncode != 0
    assert "needs 2 visible GPUs" in r.stderr
    assert "n_gpus" not in r.stdout          # no JSON line claiming a GPU count


def test_world_size_must_match_gpus_flag():
    import torch
    if not torch.cuda.is_available():
        # the visible-GPU check fires first on a CPU box; the message still names the flag
        r = _run("--gpus", "1", env={"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0"})
        assert r.returncode != 0 and "--gpus 1" in r.stderr
        return
    r = _run("--gpus", "1", "--steps", "2", "--warmup", "1", env={"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0",
                                                                   "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29999"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_host_cores_respects_affinity_and_quota():
    sys.path.insert(0, ROOT)
    import bench
    n = bench.host_cores()
    assert 1 <= n <= len(os.sched_getaffinity(0))


def test_dump_outputs_float32_and_row_sample_over_the_limit(tmp_path):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(1)
    arrays = {"obs": rng.standard_normal((100, 6)).astype(np.float32), "truncated": (rng.random(100) < 0.3).astype(np.uint8)}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    for k, a in arrays.items():
        got = np.load(tmp_path / "all" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, a)
    # 28 bytes per env row: a limit of 280 keeps 10 rows — the same ones, in env order, in every array and every call
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=280)
    obs, tr = np.load(tmp_path / "s1" / "obs.npy"), np.load(tmp_path / "s1" / "truncated.npy")
    assert obs.shape == (10, 6) and tr.shape == (10,) and obs.nbytes + tr.nbytes <= 280
    rows = [int(np.flatnonzero((arrays["obs"] == o).all(axis=1))[0]) for o in obs]
    assert rows == sorted(set(rows)) and np.array_equal(tr, arrays["truncated"][rows])
    assert np.array_equal(obs, np.load(tmp_path / "s2" / "obs.npy"))


@pytest.mark.gpu
def test_dump_outputs_is_the_kth_timed_step_and_repeats(tmp_path):
    """--dump-outputs holds what step() returned preroll + warmup + steps after reset(), whatever the repetition count, and
    is the same from run to run."""
    import json
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from windgym_amd import binding
    B, preroll, warm = 64, 40, 3
    dumps = {}
    for tag, k in (("a", 7), ("b", 7), ("c", 9)):
        d = str(tmp_path / tag)
        r = _run("--gpus", "1", "--steps", str(k), "--warmup", str(warm), "--preroll", str(preroll), "--envs", str(B),
                 "--no-cpu", "--dump-outputs", d)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout)
        assert line["steps"] == k and line["reps"] > 5          # (the clock raised the repetition count)
        dumps[tag] = {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}
        assert sorted(dumps[tag]) == ["final_obs", "obs", "reward", "truncated"]
        assert all(a.dtype == np.float32 and len(a) == B for a in dumps[tag].values())
    env = binding.HipBatch(bench.make_cfg(B), device=0)
    env.reset(seeds=1234 + np.arange(B))
    gen = torch.Generator(device="cpu").manual_seed(0)
    acts = (torch.rand((16, B, env.N), generator=gen) * 2 - 1).to(env.device).contiguous()
    tag_at = {preroll + warm + 7: "a", preroll + warm + 9: "c"}
    for i in range(preroll + warm + 9):
        got = dict(zip(("obs", "reward", "truncated", "final_obs"), env.step(acts[i % 16])))
        if i + 1 in tag_at:
            for n, t in got.items():
                assert np.array_equal(dumps[tag_at[i + 1]][n], t.cpu().numpy().astype(np.float32)), (tag_at[i + 1], n)
    env.check()
    env.close()
    for n in dumps["a"]:
        assert np.array_equal(dumps["a"][n], dumps["b"][n]), n
    assert not np.array_equal(dumps["a"]["obs"], dumps["c"]["obs"])
