"""One table of limit cases for the recurrent trainer, shared by the GPU tests of wg_lstm_ppo_grad (tests/test_gpu_recurrent_ppo_limits.py)
and the CPU test of the cases themselves (tests/test_recurrent_ppo_cases.py): plain data, builders on tests/lstm_bptt_twin.py and the
reference of a case, computed once per process.  No GPU import.  TEST INFRASTRUCTURE.

A BUILT case is ``(spec, flat, roll, envs, kw)``: the twin's spec, the flat float32 parameters, the rollout dict of
``lstm_bptt_twin.random_rollout``, the minibatch's env ids (int32) and the loss arguments.

THE SUPERVISED HEAD (tests/test_gpu_recurrent_imitation_limits.py, tests/test_bc_cases.py) runs the same tables: ``build_arch`` /
``build_edge`` take the rollout's generator, and ``lstm_bc_twin.random_rollout`` draws the same buffers from the same seed and adds the
labels, so a case's parameters, observations, starts and states are the PPO case's.  ``bc_arch`` / ``bc_edge`` hold a built case per
(loss, returns or not) with its ``BcReference``."""
from __future__ import annotations

import functools

import numpy as np
import torch

import lstm_bc_twin as bt
import lstm_bptt_twin as tw
from rl_helpers import DEEP

KW = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)
EXTRA = 5                                    # envs of an ARCH_CASES rollout that are in no minibatch

# (n_in, H, T, Bm, shared, hidden_pi, hidden_vf, n_out, activation)
ARCH_CASES = [
    (8, 256, 128, 2, False, (64, 64), (64, 64), 16, "tanh"),             # RecurrentPPO("MlpLstmPolicy", env)'s defaults, n_steps included
    (7, 40, 5, 33, False, (64, 64), (64, 64), 16, "relu"),               # relu through the heads' input gradient
    (7, 40, 5, 33, True, (), (), 80, "tanh"),                            # heads directly on h, a shared LSTM sums both dh, 80 outputs
    (20, 256, 3, 33, False, DEEP, (33,), 128, "tanh"),                   # the MLP's limits behind the LSTM
    (7, 40, 5, 33, False, (), DEEP, 1, "relu"),                          # actor and critic stacks of different depth
    (257, 64, 4, 33, True, (128, 128, 128), (64,), 3, "relu"),           # a chunk of one input, with a shared LSTM
    (8, 255, 3, 31, False, (16,), (16,), 2, "tanh"),                     # the last unit tile masked by one, odd K
    (8, 33, 4, 65, False, (16,), (16,), 2, "tanh"),                      # one unit in unit tile 2, one column in env tile 3
]


def _stack(h):
    return "x".join(map(str, h)) or "none"


def arch_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{'shared' if c[4] else 'two'}-pi{_stack(c[5])}-vf{_stack(c[6])}-{c[7]}-{c[8]}"


def make_spec(n_in, H, shared, hidden_pi=(16,), hidden_vf=(16,), n_out=2, activation="tanh"):
    return dict(n_in=n_in, H=H, n_out=n_out, hidden_pi=tuple(hidden_pi), hidden_vf=tuple(hidden_vf), shared=shared, activation=activation)


def build_arch(case, rollout=tw.random_rollout):
    n_in, H, T, Bm, shared, hidden_pi, hidden_vf, n_out, activation = case
    spec = make_spec(n_in, H, shared, hidden_pi, hidden_vf, n_out, activation)
    B = Bm + EXTRA
    flat = tw.random_params(spec, seed=Bm + T)
    roll = rollout(spec, flat, T, B, seed=H + T)
    envs = np.random.default_rng(n_in).permutation(B)[:Bm].astype(np.int32)
    return spec, flat, roll, envs, dict(KW)


# the degenerate cells: name -> what lstm_bptt_twin.layout's tensors the case makes EXACTLY zero (prefixes of their names)
CELL_EDGES = {
    "all_fresh": ("lstm_actor.weight_hh_l0", "lstm_critic.weight_hh_l0"),
    "none_fresh": (),
    "vf_coef_0": ("lstm_critic.", "mlp_extractor.value_net.", "value_net."),
    "saturated_gates": (),
    "long_carry": (),
    "large_c0": (),
    "start_on_last_step_only": (),
    # (0.5: the mean of n copies is exact in float32 and float64, so the normalised advantage is 0 and with it the actor's whole path)
    "constant_advantage": ("lstm_actor.", "mlp_extractor.policy_net.", "action_net."),
}
SATURATION = 20.0                            # saturated_gates: every LSTM tensor times this
# the supervised head's: constant_advantage has no meaning there; its counterpart is labels that ARE the float64 twin's means, rounded
# to float32 — the actor's path is then small (half an ulp of error per output), not zero
BC_ONLY_EDGES = ("labels_are_the_means",)
BC_CELL_EDGES = tuple(e for e in CELL_EDGES if e != "constant_advantage") + BC_ONLY_EDGES
BC_KW = dict(ent_coef=KW["ent_coef"], vf_coef=KW["vf_coef"])
BC_COMBOS = [(loss, with_ret) for loss in ("mse", "nll") for with_ret in (True, False)]
REUSE_CALLS = [(9, 40), (4, 33), (9, 1), (1, 40), (4, 33)]          # (T, Bm) of the handle-reuse tests; the handle is made at (9, 40)


def _lstm_slices(spec):
    """{tensor name: slice of the flat vector} of the LSTM tensors."""
    out, o = {}, 0
    for name, shape in tw.layout(spec):
        n = int(np.prod(shape))
        if name.startswith("lstm_"):
            out[name] = slice(o, o + n)
        o += n
    return out


def build_edge(edge, rollout=tw.random_rollout):
    """Base: n_in = 7, H = 40, T = 6, B = Bm = 37 (a full env tile and five columns, every env in the minibatch), two nets, heads
    (16,), 2 outputs, tanh."""
    assert edge in CELL_EDGES or (edge in BC_ONLY_EDGES and rollout is not tw.random_rollout), edge
    n_in, H, T, B = 7, 40, 6, 37
    if edge == "long_carry":
        H, T, B = 64, 128, 3
    spec = make_spec(n_in, H, False)
    flat = tw.random_params(spec, seed=11)
    kw = dict(KW)
    starts = None
    if edge == "all_fresh":
        starts = np.ones((T + 1, B), np.uint8)
    elif edge in ("none_fresh", "long_carry"):
        starts = np.zeros((T + 1, B), np.uint8)
    elif edge == "start_on_last_step_only":
        starts = np.zeros((T + 1, B), np.uint8)
        starts[T - 1, ::2] = 1               # every other env: a tile mixes columns whose last step is cut off with columns that carry on
    if edge == "saturated_gates":
        for sl in _lstm_slices(spec).values():
            flat[sl] *= np.float32(SATURATION)
    if edge == "long_carry":
        for name, sl in _lstm_slices(spec).items():
            if name.endswith("bias_ih_l0"):
                flat[sl][H:2 * H] += np.float32(4.0)          # the forget gate's rows of (i, f, g, o)
    roll = rollout(spec, flat, T, B, seed=12, starts=starts)
    if edge == "all_fresh":
        roll["lstm_state0"][:] = np.nan
    elif edge == "large_c0":
        roll["lstm_state0"][:, 1] *= np.float32(10.0)
    elif edge == "constant_advantage":
        roll["advantage"][:] = 0.5
    elif edge == "vf_coef_0":
        kw["vf_coef"] = 0.0
    envs = np.random.default_rng(13).permutation(B).astype(np.int32)
    return spec, flat, roll, envs, kw


def is_zero_tensor(edge, name):
    return any(name.startswith(p) for p in CELL_EDGES.get(edge, ()))


def gate_saturation(spec, flat, roll, envs):
    """The share of step 0's input and forget gates (all nets, the minibatch's envs) with s (1 - s) < 1e-3, in float64."""
    p = tw.views(spec, np.asarray(flat, np.float64))
    H = spec["H"]
    x = roll["obs"][0][envs].astype(np.float64)
    fresh = (roll["episode_start"][0][envs] != 0)[:, None]
    small = total = 0
    for i, net in enumerate(tw.NETS[:tw.nets(spec)]):
        h = np.where(fresh, 0.0, roll["lstm_state0"][i, 0][envs].astype(np.float64))
        z = p[f"{net}.bias_ih_l0"] + p[f"{net}.bias_hh_l0"] + x @ p[f"{net}.weight_ih_l0"].T + h @ p[f"{net}.weight_hh_l0"].T
        s = 1.0 / (1.0 + np.exp(-z[:, :2 * H]))
        small += int((s * (1.0 - s) < 1e-3).sum())
        total += s.size
    return small / total


class Reference:
    """The float64 twin's result on a built case and, from the reference side only, the float32 twin's distance from it."""

    def __init__(self, spec, flat, roll, envs, kw):
        self.loss, self.stats, self.grad, self.ratio = tw.loss_and_grad(spec, flat, roll, envs, **kw)
        self.grad32 = tw.loss_and_grad(spec, flat, roll, envs, dtype=torch.float32, **kw)[2]
        self._parts(spec, roll["raw"].shape[0], envs)

    def _parts(self, spec, T, envs):
        self.d32 = np.abs(self.grad32 - self.grad)
        self.n_lstm = tw.nets(spec) * 4 * spec["H"] * (spec["n_in"] + spec["H"] + 2)
        self.rows = T * len(envs)
        self.slices, o = [], 0
        for name, shape in tw.layout(spec):
            n = int(np.prod(shape))
            self.slices.append((name, slice(o, o + n)))
            o += n


class BcReference(Reference):
    """The same for the supervised head: ``lstm_bc_twin.loss_and_grad`` in float64 and, for e32, the float32 torch run of the same
    rule.  ``kw``: ``loss``, ``ent_coef``, ``vf_coef``; ``roll["returns"]`` ``None``: no critic term."""

    def __init__(self, spec, flat, roll, envs, kw):
        self.loss, self.stats, self.grad = bt.loss_and_grad(spec, flat, roll, envs, **kw)
        self.grad32 = bt.loss_and_grad(spec, flat, roll, envs, dtype=torch.float32, **kw)[2]
        self._parts(spec, roll["labels"].shape[0], envs)


def compare(ref, g):
    """A gradient ``g`` (float64 numpy) against ``ref`` -> dict(whole=(err, e32, bar), block=(err, e32, bar) of the LSTM tensors together,
    tensors=[(name, err, e32, bar)]).  The bars: whole ``max(4 e32, 1e-4 |ref|_2 + 1e-6)``; block and every tensor ``max(4 e32, 1e-4
    |ref|_2)`` of that part (no absolute term: a part's entries can be smaller than it)."""
    diff, nl = np.abs(g - ref.grad), ref.n_lstm
    part = lambda sl: (diff[sl].max(), ref.d32[sl].max(), max(4.0 * ref.d32[sl].max(), 1e-4 * np.linalg.norm(ref.grad[sl])))
    return dict(whole=(diff.max(), ref.d32.max(), max(4.0 * ref.d32.max(), 1e-4 * np.linalg.norm(ref.grad) + 1e-6)),
                block=part(slice(0, nl)), tensors=[(name,) + part(sl) for name, sl in ref.slices])


@functools.lru_cache(maxsize=None)
def arch(i):
    """(built case, Reference) of ARCH_CASES[i]; computed once, read-only."""
    built = build_arch(ARCH_CASES[i])
    return built, Reference(*built)


@functools.lru_cache(maxsize=None)
def edge(name):
    """(built case, Reference) of the cell edge ``name``; computed once, read-only."""
    built = build_edge(name)
    return built, Reference(*built)


def _bc_case(built, loss, with_ret):
    spec, flat, roll, envs, kw = built
    roll = roll if with_ret else dict(roll, returns=None)
    built = (spec, flat, roll, envs, dict(loss=loss, ent_coef=kw["ent_coef"], vf_coef=kw["vf_coef"]))
    return built, BcReference(*built)


@functools.lru_cache(maxsize=None)
def _bc_built(kind, key):
    if kind == "arch":
        return build_arch(ARCH_CASES[key], rollout=bt.random_rollout)
    sigma = 0.0 if key == "labels_are_the_means" else 0.3
    return build_edge(key, rollout=functools.partial(bt.random_rollout, sigma=sigma))


@functools.lru_cache(maxsize=None)
def bc_arch(i, loss, with_ret):
    """(built case, BcReference) of ARCH_CASES[i] under the supervised ``loss``, with the returns or without; computed once, read-only."""
    return _bc_case(_bc_built("arch", i), loss, with_ret)


@functools.lru_cache(maxsize=None)
def bc_edge(name, loss, with_ret):
    """(built case, BcReference) of the cell edge ``name`` of BC_CELL_EDGES; computed once, read-only."""
    return _bc_case(_bc_built("edge", name), loss, with_ret)


def bc_is_zero_tensor(edge, name, loss, with_ret):
    """What a supervised case makes EXACTLY zero: the cell edge's tensors, the critic's side without returns, log_std under MSE."""
    critic = name.startswith("lstm_critic.") or "value_net" in name
    return is_zero_tensor(edge, name) or (critic and not with_ret) or (name == "log_std" and loss == "mse")


def tensor_class(name):
    """The class a tensor's error is reported under."""
    if name == "log_std":
        return "log_std"
    if name.startswith("lstm_"):
        return "lstm_" + ("w_ih" if "weight_ih" in name else "w_hh" if "weight_hh" in name else "bias")
    return "mlp_weight" if name.endswith("weight") else "mlp_bias"
