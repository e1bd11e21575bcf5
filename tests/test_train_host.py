"""The trainers' shared host code, decided on the CPU: windgym_amd/csrc/wg_train.h is plain C++, so Adam's per-step scalars (the
bias corrections wg_ppo_apply, wg_pop_update and wg_lstm_ppo_apply all take from ONE function) and the minibatch loop of every
update entry are pinned here without a device.  tests/train_shim.cpp hands the header's functions over."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import host_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "windgym_amd", "csrc")
STEPS = [1, 2, 10, 1000, 10 ** 6, 2 ** 32 + 1]
LRS = [3e-4, 0.0, 1.0]
LOOPS = [(1, 1, 1), (7, 2, 3), (8, 2, 4), (5, 3, 8), (33, 1, 32)]          # (rows, epochs, batch)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """g++ alone, no ROCm include path: the header must stay free of HIP headers."""
    lib = host_shim(tmp_path_factory, "train")
    lib.adam_scalars.argtypes = [C.c_uint64, C.c_float, C.c_void_p]
    lib.adam_count_twice.argtypes = [C.c_uint64, C.c_float, C.c_void_p]
    lib.adam_count_twice.restype = C.c_uint64
    lib.n_minibatches.argtypes = [C.c_int64, C.c_int]
    lib.each_minibatch.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    return lib


def ref_scalars(step, lr):
    """float32(lr / (1 - 0.9^step)), float32(sqrt(1 - 0.999^step)), everything before the one rounding in float64 (lr is the float32
    the entry was given)"""
    step, lr = np.float64(step), np.float64(np.float32(lr))
    return np.array([lr / (1.0 - np.float64(0.9) ** step), np.sqrt(1.0 - np.float64(0.999) ** step)]).astype(np.float32)


def test_adam_constants(shim):
    c = (C.c_double * 3)()
    shim.adam_consts(c)
    assert list(c) == [0.9, 0.999, float(np.float32(1e-5))]


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("step", STEPS)
def test_adam_scalars_bits(shim, step, lr):
    got = np.zeros(2, np.float32)
    shim.adam_scalars(step, lr, got.ctypes.data_as(C.c_void_p))
    ref = ref_scalars(step, lr)
    print(step, lr, got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("step", [0, 9, 2 ** 32])
def test_adam_count_is_one_step_then_its_scalars(shim, step):
    got = np.zeros(4, np.float32)
    assert shim.adam_count_twice(step, 3e-4, got.ctypes.data_as(C.c_void_p)) == step + 2
    ref = np.concatenate([ref_scalars(step + 1, 3e-4), ref_scalars(step + 2, 3e-4)])
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def walk(shim, rows, epochs, batch, stop_at=-1):
    out, rc = np.full((64, 3), -1, np.int64), C.c_int(-1)
    calls = shim.each_minibatch(rows, epochs, batch, stop_at, out.ctypes.data_as(C.c_void_p), len(out), C.byref(rc))
    return [tuple(int(x) for x in r) for r in out[:calls]], rc.value


@pytest.mark.parametrize("rows, epochs, batch", LOOPS)
def test_minibatch_loop(shim, rows, epochs, batch):
    n_mb = -(-rows // batch)
    ref = [(e * n_mb + k, e * rows + k * batch, min(batch, rows - k * batch)) for e in range(epochs) for k in range(n_mb)]
    got, rc = walk(shim, rows, epochs, batch)
    assert shim.n_minibatches(rows, batch) == n_mb
    assert got == ref and rc == 0
    # every row of every epoch's permutation exactly once, in order
    assert [o + i for _, o, n in got for i in range(n)] == list(range(epochs * rows))


def test_minibatch_loop_stops_at_the_first_failure(shim):
    got, rc = walk(shim, 7, 2, 3, stop_at=3)
    assert len(got) == 4 and got[-1] == (3, 7, 3) and rc == 7


def test_header_is_host_only(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "wg_train.h"\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, str(src)], check=True)
