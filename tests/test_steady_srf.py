"""The one-launch Serial-Refine optimiser (k_steady_srf, wg_steady_optimize), the parts that need no GPU: the host twin the
kernel is held to (tests/steady_srf_twin.py) equals the product's own loop `steady.yaw_optimizer_srf` on the torch models,
the offsets table handed to the device is the loop's, and the batched agent optimises again exactly when an episode moved."""
import numpy as np
import pytest
import torch

import steady_cases as sc
import steady_srf_twin as tw
from windgym_amd import steady


def _layout_4x3():
    x, y = np.meshgrid(np.linspace(0, 1280, 4), np.linspace(0, 853.3, 3))
    return x.ravel(), y.ravel()


def _torch_power_fn(model, x, y, ws, wd, ti):
    """the torch model, rounded to float32 the way k_steady's output is"""
    fn = steady.steady_state_power if model == "m0" else steady.blondel_jimenez_power

    def power(yaw):
        return fn(x, y, ws[:, None], wd[:, None], ti[:, None], torch.as_tensor(yaw)).numpy().astype(np.float32)
    return power


X4, Y4 = sc.grid(4, 4)
TWIN_CASES = {
    # name: (x, y, ws, wd, ti, refine_pass_n, yaw_n)
    "4x3": (*_layout_4x3(), [7.0, 9.0, 9.0, 11.0], [270.0, 270.0, 250.0, 285.0], [0.04, 0.04, 0.08, 0.06], 3, 5),
    "n2": ([0.0, 500.0], [0.0, 0.0], [6.0], [270.0], [0.02], 8, 9),
    "n1": ([0.0], [0.0], [8.0, 11.0], [270.0, 33.0], [0.06, 0.06], 8, 9),        # +- offsets tie: the first index decides
    "4x4_aligned": (X4, Y4, [8.0, 8.0], [270.0, 180.0], [0.06, 0.06], 2, 5),
}


@pytest.mark.parametrize("model", sc.MODELS)
@pytest.mark.parametrize("name", list(TWIN_CASES))
def test_twin_equals_the_host_loop_on_the_torch_models(name, model):
    x, y, ws, wd, ti, passes, yaw_n = TWIN_CASES[name]
    x, y, ws, wd, ti = (np.asarray(a, dtype=np.float64) for a in (x, y, ws, wd, ti))
    ref = steady.yaw_optimizer_srf(x, y, ws, wd, ti, refine_pass_n=passes, yaw_n=yaw_n, model=model)
    wd_k = wd + 1e-3                                                       # what the loop evaluates (steady.py)
    got, best = tw.srf_twin(_torch_power_fn(model, x, y, ws, wd_k, ti), tw.kernel_order(x, y, wd_k),
                            steady.srf_offsets(passes, yaw_n, 30.0).numpy(), 30.0)
    assert got.shape == ref.shape == (len(ws), len(x))
    assert np.array_equal(got, ref), np.abs(got - ref).max()
    if len(x) > 1:
        assert np.abs(got).max() > 0.0                                     # (an optimiser that never moves would agree too)
    zero = tw.index_order_sum(_torch_power_fn(model, x, y, ws, wd_k, ti)(np.zeros((len(ws), 1, len(x)))))[:, 0]
    assert (best >= zero).all()


def test_twin_takes_the_first_of_equal_candidates_and_needs_a_strict_gain():
    """a power function that only sees |yaw|: +-offsets tie and the negative one (lower index) wins; a flat one never moves"""
    order = np.array([[0, 1]])
    offs = steady.srf_offsets(2, 5, 30.0).numpy()
    peak = lambda yaw: (1000.0 - np.abs(np.abs(yaw) - 15.0)).astype(np.float32)      # noqa: E731   best at |yaw| = 15
    yaw, best = tw.srf_twin(peak, order, offs, 30.0)
    assert np.array_equal(yaw, [[-15.0, -15.0]]) and best[0] == 2000.0
    yaw, best = tw.srf_twin(lambda yaw: np.full(yaw.shape, 7.0, dtype=np.float32), order, offs, 30.0)
    assert np.array_equal(yaw, [[0.0, 0.0]]) and best[0] == 14.0
    yaw, _ = tw.srf_twin(peak, order, offs, 10.0)                            # the clamp is applied at the end only
    assert np.array_equal(yaw, [[-10.0, -10.0]])


def test_index_order_sum_is_sequential():
    p = np.random.default_rng(0).uniform(0.0, 2e6, (3, 128)).astype(np.float32)
    want = [sum((float(v) for v in row), 0.0) for row in p]
    assert np.array_equal(tw.index_order_sum(p), want)


@pytest.mark.parametrize("yaw_max", [30.0, 45.0, 25.3])
def test_offsets_table_is_the_loops_linspace(yaw_max):
    passes, yaw_n = 8, 9
    table = steady.srf_offsets(passes, yaw_n, yaw_max)
    assert table.dtype == torch.float64 and tuple(table.shape) == (passes, yaw_n)
    rng = float(yaw_max)
    for r in range(passes):                                                # the loop of yaw_optimizer_srf
        assert torch.equal(table[r], torch.linspace(-rng, rng, yaw_n, dtype=torch.float64)), r
        rng /= 2.0
    assert torch.equal(steady.srf_offsets(2, 16, yaw_max)[1], torch.linspace(-yaw_max / 2, yaw_max / 2, 16, dtype=torch.float64))


class _FakeBatch:
    """stands in for a HipBatch: episode counters and an optimiser that counts its calls"""

    def __init__(self, B, N):
        self.episode = torch.zeros(B, dtype=torch.int32)
        self.calls = []
        self.B, self.N = B, N

    def info(self, name):
        assert name == "episode"
        return self.episode.clone()

    def optimal_yaws(self, **kw):
        self.calls.append(kw)
        return torch.arange(self.B * self.N, dtype=torch.float64).reshape(self.B, self.N) * 0.5 + len(self.calls)


class _FakeEnv:
    as_torch = False

    def __init__(self, B, N):
        self.batch = _FakeBatch(B, N)


@pytest.mark.parametrize("cls,model", [("SteadyStateYawVecAgent", "m0"), ("PyWakeVecAgent", "blondel_jimenez")])
def test_vec_agent_optimises_again_exactly_when_an_episode_moved(cls, model):
    import windgym_amd
    A = getattr(windgym_amd, cls)                                            # exported from the package
    env = _FakeEnv(3, 2)
    agent = A(env=env, refine_pass_n=4, yaw_n=5)
    assert agent.UseEnv and agent.model == model
    a0, state = agent.predict(None, deterministic=True)
    assert state is None and isinstance(a0, np.ndarray) and a0.dtype == np.float32 and a0.shape == (3, 2)
    assert env.batch.calls == [dict(model=model, refine_pass_n=4, yaw_n=5, yaw_max=30.0)]
    assert np.array_equal(a0, agent.scale_yaw(agent.optimized_yaws.numpy()).astype(np.float32))
    for _ in range(3):                                                     # nothing moved: the cached optimum
        a1, _ = agent.predict(None)
    assert len(env.batch.calls) == 1 and np.array_equal(a1, a0)
    env.batch.episode[1] += 1                                              # env 1 was reset: a new wind
    a2, _ = agent.predict(None)
    assert len(env.batch.calls) == 2 and not np.array_equal(a2, a0)
    agent.predict(None)
    assert len(env.batch.calls) == 2
    other = _FakeEnv(3, 2)                                                 # bound to another env (what eval_sweep does)
    agent.env = other
    agent.yaw_max, agent.yaw_min = 40, -40
    a3, _ = agent.predict(None)
    assert len(other.batch.calls) == 1 and len(env.batch.calls) == 2
    assert np.array_equal(a3, ((agent.optimized_yaws.numpy() + 40.0) / 80.0 * 2 - 1).astype(np.float32))
    agent.reset()
    agent.predict(None)
    assert len(other.batch.calls) == 2
    other.as_torch = True                                                  # an env that works on tensors gets a tensor
    a4, _ = agent.predict(None)
    assert isinstance(a4, torch.Tensor) and a4.dtype == torch.float32 and len(other.batch.calls) == 2


def test_vec_agent_without_an_env_says_so():
    with pytest.raises(ValueError):
        steady.SteadyStateYawVecAgent().predict(None)


def test_fused_needs_a_device_batch():
    with pytest.raises(ValueError):
        steady.yaw_optimizer_srf([0.0, 500.0], [0.0, 0.0], [8.0], [270.0], [0.06], fused=True)
    with pytest.raises(ValueError):
        steady.SteadyStateYawAgent(x_pos=[0, 500], y_pos=[0, 0], fused=True)
