"""One table of loss-head edges for the supervised gradient of an MLP policy (k_bc_grad / k_bc_reduce of wg_ppo.hip), shared by the GPU
test (tests/test_gpu_imitation_limits.py) and the CPU test of the cases themselves (tests/test_bc_cases.py): plain data, builders on
tests/imitation_twin.py and the float64 reference of a case, computed once per process.  No GPU import.  TEST INFRASTRUCTURE.

A BUILT case is a namespace ``(shape, activation, sd, obs, target, ret, rows, kw)``: ``(n_in, hidden, n_out)`` with the actor's stack
for both nets, the float64 state dict (every entry a float32 value, so the device holds the same numbers), the batch, the minibatch's
row ids and the arguments of ``imitation_twin.bc_loss_and_grad`` / ``PPOOptimizer.bc_grad``.  The edges ``saturated_tanh`` and
``dead_relu_layer`` change the parameters as tests/test_gpu_ppo.py's edges of the same names do."""
from __future__ import annotations

import functools
import types

import numpy as np

import imitation_twin as tw
from oracle import policy_oracle as po

SHAPE, N_ROWS, TOTAL = (32, (64, 64), 16), 1024, 1500
KW = dict(ent_coef=0.01, vf_coef=0.5)
FAR_SIGMAS = 50.0                            # far_targets: every target this many standard deviations (+-10 %) from the mean
PRE = "mlp_extractor.policy_net."
PRE_VF = "mlp_extractor.value_net."

# name -> the losses it runs under (both, unless one of them does not see the edge); every case is run WITH returns
BC_EDGES = {
    "log_std_-3": ("mse", "nll"),
    "log_std_+1.5": ("mse", "nll"),
    "log_std_spread": ("mse", "nll"),        # linspace(-3, 1.5, n_out): a wrong output index in ls / sd cannot cancel
    "vf_coef_0": ("mse", "nll"),
    "ent_coef_0": ("nll",),                  # (MSE has no entropy term)
    "saturated_tanh": ("mse", "nll"),
    "dead_relu_layer": ("mse", "nll"),
    "repeated_rows": ("mse", "nll"),
    "far_targets": ("nll",),                 # (z enters the MSE gradient nowhere)
    "n_out_1": ("mse", "nll"),               # at 7-(33,)-1: inv_no = 1
    "targets_are_the_means": ("mse", "nll"),
}
CASES = [(e, loss) for e, losses in BC_EDGES.items() for loss in losses]


def zero_tensors(edge, loss):
    """The tensors whose gradient the case makes EXACTLY zero (SB3 names)."""
    out = ["log_std"] if loss == "mse" else []
    if edge == "dead_relu_layer":                                        # upstream of the dead layers, as tests/test_gpu_ppo.py lists them
        out += [PRE + "0.weight", PRE + "0.bias", PRE + "2.weight", PRE_VF + "0.weight", PRE_VF + "0.bias", PRE_VF + "2.weight"]
    if edge == "vf_coef_0":
        out += [PRE_VF + "0.weight", PRE_VF + "0.bias", PRE_VF + "2.weight", PRE_VF + "2.bias", "value_net.weight", "value_net.bias"]
    return out


def _f32(sd):
    return {k: np.asarray(v, np.float32).astype(np.float64) for k, v in sd.items()}


def build_edge(edge, loss):
    assert edge in BC_EDGES and loss in BC_EDGES[edge], (edge, loss)
    n_in, hidden, n_out = (7, (33,), 1) if edge == "n_out_1" else SHAPE
    activation = "relu" if edge == "dead_relu_layer" else "tanh"
    sd = _f32(tw.random_params(n_in, hidden, n_out, seed=20))
    kw = dict(KW, loss=loss)
    kw.update({"vf_coef_0": dict(vf_coef=0.0), "ent_coef_0": dict(ent_coef=0.0)}.get(edge, {}))
    if edge == "saturated_tanh":                                         # |pre-activation| of every hidden unit far beyond tanh's range
        for k in sd:
            if k.startswith("mlp_extractor") and k.endswith("weight"):
                sd[k] = sd[k] * 400.0
    elif edge == "dead_relu_layer":                                      # no unit of either net's first hidden layer ever fires
        sd[PRE + "0.bias"][:] = -100.0
        sd[PRE_VF + "0.bias"][:] = -100.0
        sd[PRE + "2.bias"][:] = np.abs(sd[PRE + "2.bias"]) + 0.1         # (the layer behind it lives on its biases)
    elif edge in ("log_std_-3", "log_std_+1.5"):
        sd["log_std"][:] = float(edge.split("_")[-1])
    elif edge == "log_std_spread":
        sd["log_std"][:] = np.linspace(-3.0, 1.5, n_out)
    elif edge == "far_targets":
        sd["log_std"][:] = -3.0
    sd = _f32(sd)
    rng = np.random.default_rng(21)
    obs = rng.uniform(-1, 1, (TOTAL, n_in)).astype(np.float32)
    mean, value = po.forward(sd, obs, activation)
    target = mean + 0.3 * rng.standard_normal((TOTAL, n_out))
    ret = (value + rng.standard_normal(TOTAL)).astype(np.float32)
    rows = np.random.default_rng(22).permutation(TOTAL)[:N_ROWS]
    if edge == "repeated_rows":
        rows = np.random.default_rng(22).integers(0, 40, N_ROWS)         # every one of 40 rows about 25 times
    elif edge == "far_targets":
        side = np.where(rng.uniform(size=mean.shape) < 0.5, -1.0, 1.0)
        target = mean + side * FAR_SIGMAS * rng.uniform(0.9, 1.1, mean.shape) * np.exp(sd["log_std"])
    elif edge == "targets_are_the_means":
        # the float64 means rounded to float32: an error of half an ulp per output.  The GPU test puts the DEVICE's means here (the
        # same to rounding), where the error is exactly zero
        target = mean
    return types.SimpleNamespace(shape=(n_in, hidden, n_out), activation=activation, sd=sd, obs=obs, target=target.astype(np.float32),
                                 ret=ret, rows=rows, kw=kw)


def reference(case, target=None):
    """-> ({name: gradient}, statistics) of the float64 twin on a built case (``target``: in place of the case's)."""
    _, grads, stats = tw.bc_loss_and_grad(case.sd, case.obs, case.target if target is None else target, case.ret, case.rows,
                                          activation=case.activation, **case.kw)
    return grads, stats


@functools.lru_cache(maxsize=None)
def edge(name, loss):
    """(built case, (gradients, statistics) of the float64 twin) of the edge ``name`` under ``loss``; computed once, read-only."""
    case = build_edge(name, loss)
    return case, reference(case)


def z_scores(case):
    """(target - mean) / sigma of the minibatch's rows in float64."""
    mean, _ = po.forward(case.sd, case.obs[case.rows], case.activation)
    return (case.target[case.rows].astype(np.float64) - mean) / np.exp(case.sd["log_std"])


def first_hidden(case, net):
    """The first hidden layer's PRE-activations of ``net`` (PRE / PRE_VF) on the minibatch's rows."""
    return case.obs[case.rows].astype(np.float64) @ case.sd[net + "0.weight"].T + case.sd[net + "0.bias"]
