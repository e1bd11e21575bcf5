"""CPU-side checks of the yaw curriculum (windgym_amd/curriculum.py): the float64 numpy restatement and the weight schedule against
what the reference's own CurriculumWrapper returned (tests/golden/curriculum_wrapper.npz, recorded by make_curriculum_golden.py), the
ABI entries, the refusals that need no GPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from windgym_amd import binding, build
from windgym_amd.curriculum import YawCurriculum, curriculum_weights, shape_numpy, targets_per_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("wg_curriculum_create", "wg_curriculum_destroy", "wg_curriculum_get_state", "wg_curriculum_set_state",
           "wg_curriculum_set_targets", "wg_curriculum_shape")
CASES = ("n2", "n4")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "curriculum_wrapper.npz"))
    return {c: {k[len(c) + 1:]: z[k] for k in z.files if k.startswith(c + "_")} for c in CASES}


@pytest.mark.parametrize("case", CASES)
def test_golden_covers_what_the_penalties_distinguish(golden, case):
    g = golden[case]
    T, N = g["yaws"].shape
    assert N == int(case[1:]) and T >= 60 and int(g["truncated"].sum()) == 2
    assert np.array_equal(g["yaws"], g["yaws"].astype(np.float32).astype(np.float64))            # float32-representable
    c = np.abs(np.diff(g["yaws"], axis=0))
    assert (c == 0).all(axis=1).any() and ((c == 0).any(axis=1) & (c != 0).any(axis=1)).any()    # sign 0 on all / on some turbines
    s = np.sign(np.diff(g["yaws"], axis=0))
    assert (s[1:] * s[:-1] < 0).any()                                                             # reversals
    w = g["weight"]
    assert (w == 0).sum() >= 2 and (w == 1).sum() >= 2 and ((w > 0) & (w < 1)).sum() >= 2         # pure similarity, ramp, plateau
    tr = np.flatnonzero(g["truncated"])
    for t in tr:            # the step that truncates is paid against the old target, the next one against the new
        assert np.array_equal(g["targets"][t], g["targets"][t - 1]) and not np.array_equal(g["targets"][t + 1], g["targets"][t])


@pytest.mark.parametrize("case", CASES)
def test_shape_numpy_reproduces_the_reference_wrapper(golden, case):
    """Both sides are float64; only the order of the N-term sums differs (the wrapper sums its history over time first)."""
    g = golden[case]
    shaped, diff, st = shape_numpy(g["yaws"], g["rewards"], g["targets"], g["weight"], float(g["momentum"]), float(g["yaw_max"]))
    np.testing.assert_allclose(shaped, g["shaped"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(diff, g["yaw_diff"], rtol=1e-12, atol=0)
    assert st["L"] == len(shaped) - 1
    # the state carries: two halves == the whole, bit for bit
    h = len(shaped) // 2
    a, da, s1 = shape_numpy(g["yaws"][:h], g["rewards"][:h], g["targets"][:h], g["weight"][:h], float(g["momentum"]), float(g["yaw_max"]))
    b, db, _ = shape_numpy(g["yaws"][h:], g["rewards"][h:], g["targets"][h:], g["weight"][h:], float(g["momentum"]), float(g["yaw_max"]), s1)
    assert np.array_equal(np.concatenate([a, b]), shaped) and np.array_equal(np.concatenate([da, db]), diff)


@pytest.mark.parametrize("case", CASES)
def test_weight_schedule_is_the_callbacks(golden, case):
    g = golden[case]
    T = len(g["weight"])
    w = curriculum_weights(0, T, int(g["num_envs"]), int(g["curriculum_steps"]), int(g["pure_similarity_steps"]))
    assert w.dtype == np.float64 and np.array_equal(w, g["weight"])
    # a rollout that starts later continues the same schedule
    k = 7
    assert np.array_equal(curriculum_weights(k * int(g["num_envs"]), T - k, int(g["num_envs"]), int(g["curriculum_steps"]),
                                             int(g["pure_similarity_steps"])), g["weight"][k:])


@pytest.mark.parametrize("case", CASES)
def test_targets_per_step_follows_the_resets(golden, case):
    g = golden[case]
    tr = np.flatnonzero(g["truncated"])
    new = [g["targets"][t + 1] for t in tr]
    assert np.array_equal(targets_per_step(g["targets"][0], g["truncated"], new), g["targets"])


def test_header_declares_and_library_exports_the_entries():
    hdr = open(os.path.join(ROOT, "include", "windgym_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(wg_[a-z_0-9]+)\s*\(", hdr))
    assert set(ENTRIES) <= declared and set(ENTRIES) <= set(binding.ABI_SYMBOLS)
    assert "wg_curriculum.hip" in build.SOURCES
    L = C.CDLL(build.build())
    for name in ENTRIES:
        assert hasattr(L, name), f"{name} not exported"


def test_null_and_range_refusals_need_no_device():
    """The argument checks that come before any HIP call: a null curriculum, a null handle."""
    build.build()
    L = binding.load_library()
    out = C.c_void_p()
    assert L.wg_curriculum_create(None, C.byref(out)) == -1 and b"null" in L.wg_last_error()
    assert L.wg_curriculum_shape(None, 1, *([None] * 6), 0, None, 0.5, *([None] * 5)) == -1
    assert L.wg_curriculum_set_targets(None, None, None) == -1
    assert L.wg_curriculum_destroy(None) == 0


@pytest.mark.parametrize("steps", [(10, 10), (5, 10), (-1, -5), (10, -1)])
def test_schedule_value_errors(steps):
    with pytest.raises(ValueError):
        YawCurriculum(object(), *steps)
    with pytest.raises(ValueError):
        curriculum_weights(0, 4, 2, *steps)


def test_env_must_work_on_cuda_tensors():
    host_env = types.SimpleNamespace(batch=object(), rollout=lambda *a, **k: None, as_torch=False, num_envs=2)
    with pytest.raises(ValueError, match="as_torch"):
        YawCurriculum(host_env, 100, 10)
    with pytest.raises(ValueError):
        YawCurriculum(object(), 100, 10)            # not an env at all
    with pytest.raises(ValueError, match="momentum"):
        YawCurriculum(host_env, 100, 10, reward_momentum=1.0)
    with pytest.raises(ValueError, match="model"):
        YawCurriculum(host_env, 100, 10, model="fancy")
