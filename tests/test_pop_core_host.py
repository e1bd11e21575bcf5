"""What a population is, decided on the CPU: the slot table of k_policy_pop (one builder for wg_pop_* on observation rows and for
wg_lstm_pop_* on the LSTMs' h rows), the hyper-parameter / statistics prologue of an update's member table and the comparison of two
architectures are plain C++ in windgym_amd/csrc/wg_policy.h and wg_ppo.h.  tests/pop_core_shim.cpp hands them over; every expected
table below is written out from the rule the headers document (member m on rows [m Bm, (m + 1) Bm) of every array)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import host_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "windgym_amd", "csrc")
ACTION, RAW, LOGP, VALUE, FINAL = 1, 2, 4, 8, 16
# columns of a slot: obs - rows, obs_step, act_step, row_step, net, t_shift, action, raw, logp, value, seed, row_offset, member


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """g++ alone, no ROCm include path: the headers must stay free of HIP headers."""
    lib = host_shim(tmp_path_factory, "pop_core")
    lib.pop_slots.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pop_slots.restype = None
    lib.pop_members.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.same_arch.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    return lib


def slots(shim, P, Bm, n_out, width, step, want, out_step, seeds, offsets):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731
    width, step = np.array(width, np.int32), np.array(step, np.int64)
    seeds = None if seeds is None else np.array(seeds, np.uint64)
    offsets = None if offsets is None else np.array(offsets, np.uint64)
    head, tab = np.full(4, -7, np.int64), np.full((48, 13), -7, np.int64)
    shim.pop_slots(P, Bm, n_out, ptr(width), ptr(step), want, out_step, ptr(seeds), ptr(offsets), ptr(head), ptr(tab))
    return head.tolist(), tab[:head[0]].tolist()


def test_slots_plain_all_kinds(shim):
    """P = 3, Bm = 5, n_in = n_in_vf = 7, n_out = 2, a rollout's buffers (steps B = 15 rows apart)"""
    head, tab = slots(shim, 3, 5, 2, [7, 7, 7], [105, 105, 105], ACTION | RAW | LOGP | VALUE | FINAL, 15, [11, 12, 13], [100, 105, 110])
    assert head == [9, 2, 1, 5]
    assert tab == [[0, 105, 30, 15, 0, 0, 0, 0, 0, -1, 11, 100, 0],
                   [35, 105, 30, 15, 0, 0, 10, 10, 5, -1, 12, 105, 1],
                   [70, 105, 30, 15, 0, 0, 20, 20, 10, -1, 13, 110, 2],
                   [0, 105, 30, 15, 1, 0, -1, -1, -1, 0, 0, 0, 0],
                   [35, 105, 30, 15, 1, 0, -1, -1, -1, 5, 0, 0, 1],
                   [70, 105, 30, 15, 1, 0, -1, -1, -1, 10, 0, 0, 2],
                   [0, 105, 30, 15, 1, -1, -1, -1, -1, 0, 0, 0, 0],
                   [35, 105, 30, 15, 1, -1, -1, -1, -1, 5, 0, 0, 1],
                   [70, 105, 30, 15, 1, -1, -1, -1, -1, 10, 0, 0, 2]]


def test_slots_plain_value_only(shim):
    """only `value` wanted: P critic slots, no seeds read"""
    head, tab = slots(shim, 3, 5, 2, [7, 7, 7], [105, 105, 105], VALUE, 15, None, None)
    assert head == [3, 1, 0, 5]
    assert tab == [[0, 105, 30, 15, 1, 0, -1, -1, -1, 0, 0, 0, 0],
                   [35, 105, 30, 15, 1, 0, -1, -1, -1, 5, 0, 0, 1],
                   [70, 105, 30, 15, 1, 0, -1, -1, -1, 10, 0, 0, 2]]


def test_slots_null_row_offsets_and_a_null_actor_output(shim):
    """any actor output makes the actor's slots; row_offsets == NULL gives 0; an output not wanted stays null"""
    head, tab = slots(shim, 3, 5, 2, [7, 7, 7], [105, 105, 105], ACTION | LOGP, 15, [11, 12, 13], None)
    assert head == [3, 1, 0, 5]
    assert tab == [[0, 105, 30, 15, 0, 0, 0, -1, 0, -1, 11, 0, 0],
                   [35, 105, 30, 15, 0, 0, 10, -1, 5, -1, 12, 0, 1],
                   [70, 105, 30, 15, 0, 0, 20, -1, 10, -1, 13, 0, 2]]


def test_slots_recurrent_rollout(shim):
    """P = 2, Bm = 33, H = 40, n_out = 3: the h rows are the running step's (obs_step = 0), the outputs a rollout's (B = 66)"""
    head, tab = slots(shim, 2, 33, 3, [40, 40, 40], [0, 0, 0], ACTION | RAW | LOGP | VALUE | FINAL, 66, [5, 6], [0, 33])
    assert head == [6, 2, 1, 33]
    assert tab == [[0, 0, 198, 66, 0, 0, 0, 0, 0, -1, 5, 0, 0],
                   [1320, 0, 198, 66, 0, 0, 99, 99, 33, -1, 6, 33, 1],
                   [0, 0, 198, 66, 1, 0, -1, -1, -1, 0, 0, 0, 0],
                   [1320, 0, 198, 66, 1, 0, -1, -1, -1, 33, 0, 0, 1],
                   [0, 0, 198, 66, 1, -1, -1, -1, -1, 0, 0, 0, 0],
                   [1320, 0, 198, 66, 1, -1, -1, -1, -1, 33, 0, 0, 1]]


def test_slots_recurrent_one_call(shim):
    """the same members in one call (wg_lstm_pop_act): no stride anywhere, no final rows"""
    head, tab = slots(shim, 2, 33, 3, [40, 40, 40], [0, 0, 0], ACTION | RAW | LOGP | VALUE, 0, [5, 6], [0, 33])
    assert head == [4, 2, 0, 33]
    assert tab == [[0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 5, 0, 0],
                   [1320, 0, 0, 0, 0, 0, 99, 99, 33, -1, 6, 33, 1],
                   [0, 0, 0, 0, 1, 0, -1, -1, -1, 0, 0, 0, 0],
                   [1320, 0, 0, 0, 1, 0, -1, -1, -1, 33, 0, 0, 1]]


@pytest.mark.parametrize("normalize, any_norm", [((0, 0, 0), 0), ((0, 1, 0), 1)])
@pytest.mark.parametrize("with_stats", [1, 0])
def test_member_prologue(shim, with_stats, normalize, any_norm):
    """P = 3, n_epochs = 2, n_mb = 3: member m's records start 6 m records into stats_out, a record apart; without a stats_out every
    minibatch writes the fallback record (step 0)"""
    hp = np.array([[0.25 + m, 0.5 + m, 0.125 + m, normalize[m]] for m in range(3)], np.float32)
    out = np.full((3, 7), -7.0)
    assert shim.n_stat() == 8
    assert shim.pop_members(3, 2, 3, with_stats, hp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == any_norm
    want = [[6 * m if with_stats else -1, 8 if with_stats else 0, 0.25 + m, 0.5 + m, 0.125 + m, normalize[m], normalize[m]] for m in range(3)]
    assert out.tolist() == want


BASE = dict(n_in=7, n_out=2, activation=0, has_log_std=1, pi=(64, 32), vf=(64, 32), n_in_vf=7)


def desc(**kw):
    d = dict(BASE, **kw)
    pad = lambda h: [len(h)] + list(h) + [0] * (4 - len(h))          # noqa: E731
    return np.array([d["n_in"], d["n_out"], d["activation"], d["has_log_std"]] + pad(d["pi"]) + pad(d["vf"]) + [d["n_in_vf"]], np.int32)


def same(shim, a, b, widths):
    return shim.same_arch(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), widths)


@pytest.mark.parametrize("widths", [1, 0])
def test_equal_architectures_compare_equal(shim, widths):
    assert same(shim, desc(), desc(), widths) == 1
    assert same(shim, desc(pi=(), vf=(256, 256, 256, 256)), desc(pi=(), vf=(256, 256, 256, 256)), widths) == 1


@pytest.mark.parametrize("widths", [1, 0])
@pytest.mark.parametrize("change", [dict(n_out=3), dict(activation=1), dict(has_log_std=0), dict(pi=(64, 33)), dict(vf=(48, 32)),
                                    dict(vf=(64, 32, 32)), dict(vf=(64,)), dict(pi=(64,))], ids=str)
def test_one_differing_field_is_found(shim, change, widths):
    assert same(shim, desc(), desc(**change), widths) == 0
    assert same(shim, desc(**change), desc(), widths) == 0


def test_input_widths_take_part_only_when_asked(shim):
    wide = desc(n_in=9, n_in_vf=9)
    assert same(shim, desc(), wide, 1) == 0 and same(shim, wide, desc(), 1) == 0
    assert same(shim, desc(), desc(n_in_vf=9), 1) == 0
    assert same(shim, desc(), wide, 0) == 1 and same(shim, wide, desc(), 0) == 1


def test_headers_are_host_only(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "wg_ppo.h"\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, str(src)], check=True)
