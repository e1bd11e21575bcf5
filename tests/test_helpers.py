"""The tests' own harness, pinned without a device: binding.debug_hooks (the one place that writes the library's WG_* hooks into
the environment), binding.HOOK_ENV against the hooks wg_api.hip reads and the array of tests/plan_shim.cpp, helpers.make_batch's
check of the running variant, and one module name per file of tests/."""
import collections
import os
import re
import sys

import pytest

import helpers
import test_plan
from windgym_amd import binding
from windgym_amd.binding import HOOK_ENV, HOOK_ENV_DIAGNOSTIC, debug_hooks

A, B = "WG_FLOW_BLOCK", "WG_ENV_WPE"


@pytest.fixture
def clean(monkeypatch):
    """neither hook set (the switch is on: conftest.py); whatever a test leaves behind is undone"""
    monkeypatch.delenv(A, raising=False)
    monkeypatch.delenv(B, raising=False)
    assert os.environ.get("WG_DEBUG_HOOKS") == "1"
    return monkeypatch


def test_debug_hooks_sets_and_removes(clean):
    with debug_hooks({A: "256", B: 2}):
        assert os.environ[A] == "256" and os.environ[B] == "2"       # (values are written as text)
    assert A not in os.environ and B not in os.environ


def test_debug_hooks_restores_a_value_that_was_set_before(clean):
    clean.setenv(A, "64")
    with debug_hooks({A: "256", B: "1"}):
        assert os.environ[A] == "256"
    assert os.environ[A] == "64" and B not in os.environ


def test_debug_hooks_restores_after_an_exception(clean):
    clean.setenv(A, "64")
    with pytest.raises(KeyError):
        with debug_hooks({A: "256", B: "1"}):
            raise KeyError("inside")
    assert os.environ[A] == "64" and B not in os.environ


def test_debug_hooks_nest(clean):
    with debug_hooks({A: "64"}):
        with debug_hooks({A: "256", B: "1"}):
            assert os.environ[A] == "256" and os.environ[B] == "1"
        assert os.environ[A] == "64" and B not in os.environ
    assert A not in os.environ


@pytest.mark.parametrize("switch", [None, "0", "true", "11"])
def test_debug_hooks_refuses_without_the_switch(clean, switch):
    """the library honours its hooks under WG_DEBUG_HOOKS=1 alone (wg_api.hip: wg_hook)"""
    if switch is None:
        clean.delenv("WG_DEBUG_HOOKS")
    else:
        clean.setenv("WG_DEBUG_HOOKS", switch)
    with pytest.raises(binding.WindGymHipError, match="WG_DEBUG_HOOKS"):
        with debug_hooks({A: "256"}):
            pass
    assert A not in os.environ
    with debug_hooks({}):       # no hook asked for, nothing to ignore
        pass


def test_hook_env_is_what_wg_hooks_read_reads():
    text = open(os.path.join(helpers.CSRC, "wg_api.hip")).read()
    body = text[text.index("static WgHooks wg_hooks_read()"):]
    body = body[:body.index("\n}\n")]
    read = re.findall(r'"(WG_[A-Z0-9_]+)"', body)
    assert len(read) == len(set(read)) and "WG_DEBUG_HOOKS" not in read
    assert set(read) - set(HOOK_ENV_DIAGNOSTIC.values()) == set(HOOK_ENV.values())
    assert set(HOOK_ENV_DIAGNOSTIC.values()) <= set(read) and len(set(HOOK_ENV.values())) == len(HOOK_ENV)
    # every name is a member of WgHooks (wg_plan.h), which the plan reads
    plan_h = open(os.path.join(helpers.CSRC, "wg_plan.h")).read()
    struct = plan_h[plan_h.index("struct WgHooks"):]
    struct = struct[:struct.index("};")]
    for field in list(HOOK_ENV) + list(HOOK_ENV_DIAGNOSTIC):
        assert re.search(r"\b%s\b" % field, struct), field


def test_plan_shim_array_is_the_head_of_hook_env():
    src = open(os.path.join(helpers.TESTS, "plan_shim.cpp")).read()
    slots = re.search(r"slot\[10\]\s*=\s*\{(.*?)\}", src, flags=re.S).group(1)
    assert re.findall(r"&hk\.(\w+)", slots) == test_plan.HOOKS == list(HOOK_ENV)[:10]


class _Handle:
    def __init__(self, variant):
        self.variant, self.multi = variant, 0

    def flow_variant(self):
        return self.variant

    def fuse_obs_multi(self):
        self.multi += 1


class _Binding:
    """stands in for the binding: HipBatch(cfg) -> a handle that runs `cfg`, and records the hooks it was created under"""
    seen = None

    def HipBatch(self, cfg):
        self.seen = {k: v for k, v in os.environ.items() if k in (A, B)}
        return _Handle(cfg)


def test_make_batch_checks_the_variant_that_runs(clean):
    hip = _Binding()
    env = helpers.make_batch(hip, (64, True, 2), {A: "64"}, variant=(64, True, 2), multi=True)
    assert hip.seen == {A: "64"} and A not in os.environ and env.multi == 1
    assert helpers.make_batch(hip, (256, False, 0), variant=(256, None, 0)).multi == 0       # None: a place left open
    assert hip.seen == {}
    helpers.make_batch(hip, (256, False, 0))                                                    # no variant named, none checked
    for runs, asked in [((64, True, 0), (64, True, 2)), ((256, True, 2), (64, True, 2)), ((64, False, 2), (64, True, 2)),
                        ((64, True, 0), (None, None, 2)), ((64, True, 2), (64, True))]:
        with pytest.raises(AssertionError):
            helpers.make_batch(hip, runs, {A: "64"}, variant=asked)
        assert A not in os.environ


def test_no_test_file_is_imported_under_two_names():
    """`import rl_helpers` and `from tests import rl_helpers` would execute the file twice (and build its cached tables twice)"""
    names = collections.defaultdict(set)
    for name, mod in list(sys.modules.items()):
        path = getattr(mod, "__file__", None)
        if path and os.path.dirname(os.path.abspath(path)) == helpers.TESTS:
            names[os.path.abspath(path)].add(name)
    assert names, "the test modules are in sys.modules"
    assert not {p: n for p, n in names.items() if len(n) > 1}
    for d in (helpers.TESTS, os.path.join(helpers.ROOT, "tools")):
        for f in sorted(os.listdir(d)):
            if f.endswith(".py"):
                assert not re.search(r"^\s*(from tests\b|import tests\b)", open(os.path.join(d, f)).read(), flags=re.M), f
