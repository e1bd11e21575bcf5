"""GPU tests of the layer under every handle (windgym_amd/csrc/wg_host.h, binding.Handle): each kind of handle lives and dies once,
the three state blobs go round bit for bit and refuse what they refused before, word for word, and a host pointer where device
memory is required is refused before anything is launched.  The paths a failing HIP call takes are tests/test_host_layer.py's, on
a fake device; nothing here makes a HIP call fail.  Smallest shapes only."""
import ctypes as C
import re

import numpy as np
import pytest

from helpers import hip, physics_cfg  # noqa: F401

pytestmark = pytest.mark.gpu

DESTROYS = ["wg_destroy", "wg_policy_destroy", "wg_lstm_destroy", "wg_ppo_destroy", "wg_lstm_ppo_destroy", "wg_pop_destroy",
            "wg_lstm_pop_destroy", "wg_curriculum_destroy", "wg_norm_destroy", "wg_yaw_table_destroy"]


def _batch(hip, n_envs=2):
    return hip.HipBatch(physics_cfg(n_envs, True, 0.3, nx=2, ny=1))


def _mlp(seed=0):
    from windgym_amd.policy import MlpPolicy
    return MlpPolicy(4, 2, (8,), (8,), seed=seed)


def _lstm(seed=0):
    from windgym_amd.recurrent import MlpLstmPolicy
    return MlpLstmPolicy(4, 2, lstm_hidden_size=8, hidden_pi=(8,), hidden_vf=(8,), seed=seed)


def _table(hip, t, dev, N=2):
    yaw = t.arange(8 * N, dtype=t.float64, device=dev).reshape(8, N).contiguous()
    return hip.YawTableHandle(t, dev, [0.05, 0.1], [6.0, 10.0], [260.0, 280.0], False, yaw)


def _err(hip):
    return hip.load_library().wg_last_error().decode()


def test_every_handle_lives_once(hip):
    import torch as t
    from windgym_amd.population import Population
    from windgym_amd.ppo import PPOOptimizer
    from windgym_amd.recurrent_population import RecurrentPopulation
    from windgym_amd.recurrent_ppo import RecurrentPPOOptimizer
    L = hip.load_library()
    for name in DESTROYS:
        assert getattr(L, name)(None) == 0, name
    b = _batch(hip)
    dev = b.device
    pols, lstms = [_mlp(0), _mlp(1)], [_lstm(0), _lstm(1)]
    opts, ropts = [PPOOptimizer(p) for p in pols], [RecurrentPPOOptimizer(p, 2, 2) for p in lstms]
    pop, rpop = Population(pols, opts), RecurrentPopulation(lstms, ropts)
    cur, norm, tab, lab = hip.Curriculum(b), hip.Norm(3, 2, dev.index), _table(hip, t, dev), hip.ExpertLabels(b)
    assert lab._err.device == dev and int(lab._err.abs().sum()) == 0          # the label latch: the caller's four ints, clear
    # each one does a piece of its work
    obs = b.reset(seeds=[1, 2])
    assert t.isfinite(obs).all()
    x = t.ones((2, 4), dtype=t.float32, device=dev)
    a = pols[0].act(x, deterministic=True)[0]
    pa = pop.act(t.cat([x, x]), deterministic=True)[0]
    assert t.equal(pa[:2], a)
    ra = lstms[0].act(x, lstms[0].initial_state(2), deterministic=True)[0][0]
    rpa = rpop.act(t.cat([x, x]), rpop.initial_state(4), deterministic=True)[0][0]
    assert t.equal(rpa[:2], ra)
    for o in opts + ropts:
        mv, step = o.state()
        assert step == 0 and not mv.any()
    assert tab.rows(t.tensor([[10.0, 280.0, 0.1]], dtype=t.float64, device=dev)).tolist() == [7]
    assert len(cur.state()) == hip.Curriculum.HEADER_BYTES + 8 * (2 * 4 + 4 * 2) + 4 * 4
    assert norm.stats()["obs_count"] == 1e-4
    b.check()
    everything = [rpop, pop, *ropts, *opts, *lstms, *pols, cur, norm, tab, b]
    for h in everything:
        h.close()
        h.close()                                  # (idempotent)
    assert all(getattr(h, h.handle_attr) is None for h in everything) and all(p.mlp._h is None for p in lstms)


def test_a_refused_create_leaves_the_next_one_working(hip):
    import torch as t
    with pytest.raises(ValueError, match="wg_norm_create: n_obs and n_envs must be >= 1"):
        hip.Norm(0, 2, t.cuda.current_device())
    with pytest.raises(ValueError, match="wg_yaw_table_create: N must be >= 1"):
        dev = t.device("cuda", t.cuda.current_device())
        hip.YawTableHandle(t, dev, [0.1], [8.0], [270.0], False, t.zeros((1, 0), dtype=t.float64, device=dev))
    n = hip.Norm(3, 2, t.cuda.current_device())
    x = t.tensor([[1.0, 2.0, 3.0], [3.0, 2.0, 1.0]], device=n.device)
    out = n.obs(x, t.empty_like(x))
    assert t.isfinite(out).all() and n.stats()["obs_count"] == pytest.approx(2 + 1e-4, rel=1e-12)
    p = _mlp()
    assert p.act(t.ones((1, 4), device=p.device), deterministic=True)[0].shape == (1, 2)
    n.close(); p.close()


# ---- the three state blobs ---------------------------------------------------------------------------------------------------------
class Blobs:
    """One family: its handle, a handle of another geometry, the entries and the words of its refusals."""

    def __init__(self, hip, family):
        self.L = L = hip.load_library()
        self.envs = [_batch(hip, 2), _batch(hip, 3)]
        for e in self.envs:
            e.reset(seeds=list(range(e.B)))
        if family == "wg":
            self.h, self.other = self.envs
            self.get, self.set, self.prefix, self.take, self.put = L.wg_get_state, L.wg_set_state, "", "get_state", "set_state"
            self.not_ours = "not a windgym state blob"
            self.geometry = "state blob was taken from a differently configured handle (or another ABI version)"
        elif family == "wg_curriculum":
            self.h, self.other = (hip.Curriculum(e) for e in self.envs)
            self.get, self.set, self.prefix = L.wg_curriculum_get_state, L.wg_curriculum_set_state, "wg_curriculum_set_state: "
            self.not_ours = "wg_curriculum_set_state: not a curriculum state blob"
            self.geometry = "wg_curriculum_set_state: the blob was taken from a curriculum of 3 envs x 2 turbines, this one has 2 x 2"
        else:
            dev = self.envs[0].device.index
            self.h, self.other = hip.Norm(3, 2, dev), hip.Norm(4, 2, dev)
            self.get, self.set, self.prefix = L.wg_norm_get_state, L.wg_norm_set_state, "wg_norm_set_state: "
            self.not_ours = "wg_norm_set_state: not a wg_norm state blob"
            self.geometry = "wg_norm_set_state: the blob holds statistics of 4 observation entries x 2 envs, this wg_norm has 3 x 2"
        if family != "wg":
            self.take, self.put = "state", "load_state"
        self.get_prefix = self.prefix.replace("set_state", "get_state")
        # a blob of another kind of handle, long enough to hold this family's header
        foreign = hip.Norm(40, 2, self.envs[0].device.index) if family != "wg_norm" else hip.Curriculum(self.envs[0])
        self.foreign = foreign.state()
        foreign.close()

    def close(self):
        for h in {self.h, self.other, *self.envs}:
            h.close()


@pytest.mark.parametrize("family", ["wg", "wg_curriculum", "wg_norm"])
def test_blob(hip, family):
    import torch as t
    f = Blobs(hip, family)
    if family == "wg":
        f.h.step(t.zeros((2, 2), dtype=t.float32, device=f.h.device))
    elif family == "wg_norm":
        f.h.obs(t.rand((2, 3), device=f.h.device), t.empty((2, 3), device=f.h.device))
    else:
        f.h.set_targets(t.full((2, 2), 3.5, dtype=t.float64, device=f.envs[0].device))
    blob = getattr(f.h, f.take)()
    fresh = getattr(f.other, f.take)()
    assert len(blob) != len(fresh)
    getattr(f.h, f.put)(blob)
    assert getattr(f.h, f.take)() == blob                  # get -> set -> get: bit for bit
    L, raw = f.L, f.h._h
    # a buffer one byte short; the size query is untouched by it
    n = C.c_size_t(len(blob) - 1)
    assert f.get(raw, (C.c_char * len(blob))(), C.byref(n)) == -1 and _err(hip) == f.get_prefix + "state buffer too small"
    n = C.c_size_t(0)
    assert f.get(raw, None, C.byref(n)) == 0 and n.value == len(blob)
    # a blob shorter than a header, a blob of another kind of handle, a blob of another geometry
    assert f.set(raw, blob[:8], 8) == -1 and _err(hip) == f.prefix + "state blob too small"
    assert f.set(raw, f.foreign, len(f.foreign)) == -1 and _err(hip) == f.not_ours
    with pytest.raises(ValueError, match=re.escape(f.geometry)):
        getattr(f.h, f.put)(fresh)
    assert f.set(raw, blob[:-1], len(blob) - 1) == -1 and (family == "wg" or "this" in _err(hip))          # (its own size: a geometry too)
    assert getattr(f.h, f.take)() == blob                  # every refusal left the state alone
    f.close()


# ---- a host pointer where device memory is required --------------------------------------------------------------------------------
def _refused(hip, rc, family_prefix, name, family_suffix, device):
    want = rf"{re.escape(family_prefix)}{name} is not (a device pointer|memory of device {device}{re.escape(family_suffix)})"
    assert rc == -1 and re.fullmatch(want, _err(hip)), (rc, _err(hip), want)


def test_host_pointers_are_refused_before_any_launch(hip):
    import torch as t
    from windgym_amd.ppo import PPOOptimizer
    L = hip.load_library()
    b = _batch(hip)
    dev, D, B, N, T = b.device, b.device.index, 2, 2, 1
    b.reset(seeds=[3, 4])
    z = lambda shape, dtype=t.float32: t.zeros(shape, dtype=dtype, device=dev)          # noqa: E731
    host = np.zeros(64, np.float64)                        # pageable host memory, large enough for every argument below
    hp = host.ctypes.data
    st = b._stream()

    cur = hip.Curriculum(b)
    _refused(hip, L.wg_curriculum_set_targets(cur._h, hp, st), "wg_curriculum: ", "yaw_dev", ", the device of the handle the curriculum was created on", D)
    cur.set_targets(t.full((B, N), 2.5, dtype=t.float64, device=dev))
    assert (cur.targets_of(cur.state()) == 2.5).all()

    lab = hip.ExpertLabels(b)
    a = dict(yaw0=z((B, N)), yaw_after=z((T, B, N)), truncated=z((T, B), t.uint8), ep_row=z((T, B), t.int32) - 1,
             ep_target=z((1, N), t.float64), n_targets=1, targets=t.full((B, N), 4.0, dtype=t.float64, device=dev), labels=z((T, B, N)))
    p = lambda k: a[k].data_ptr()                          # noqa: E731
    rc = L.wg_expert_labels(b._h, T, hp, p("yaw_after"), p("truncated"), p("ep_row"), p("ep_target"), 1, p("targets"), p("labels"), None,
                            lab._err.data_ptr(), st)
    _refused(hip, rc, "wg_expert_labels: ", "yaw0_dev", ", the handle's device", D)
    assert lab.labels(T, **a).abs().sum() > 0              # (a target of 4 degrees from a yaw of 0: the expert moves)
    lab.check()

    tab = _table(hip, t, dev)
    rows = z((1,), t.int32)
    _refused(hip, L.wg_yaw_table_rows(tab._h, 1, hp, None, rows.data_ptr(), st), "wg_yaw_table_rows: ", "wind_dev", ", the table's device", D)
    assert tab.rows(t.tensor([[6.0, 260.0, 0.05]], dtype=t.float64, device=dev), out=rows).tolist() == [0]

    pol = _mlp()
    opt = PPOOptimizer(pol)
    before = pol.params.clone()
    _refused(hip, L.wg_ppo_apply(opt._h, hp, opt.grad_buf.data_ptr(), 3e-4, 0.5, st), "wg_ppo_apply: ", "params_dev", "", D)
    assert t.equal(pol.params, before) and opt.state()[1] == 0
    opt.grad_buf.fill_(1.0)
    opt.apply()
    assert not t.equal(pol.params, before) and opt.state()[1] == 1
    b.check()
    for h in (opt, pol, tab, cur, b):
        h.close()
