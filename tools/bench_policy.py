#!/usr/bin/env python
"""Closed-loop throughput with a learned policy in the loop, beside the bare C-ABI rate — one JSON line.

The protocol and the workload are those of `bench.py --api` (its `api_legs`): cfg2 (4x4 farm, 16 turbines, O = 32), `--envs`
envs on one MI355X, env-steps/s over `--api-steps` steps between two device synchronisations, host time of a call as the mean
of 200 calls after a synchronisation.  The policy is stable-baselines3's default MlpPolicy shape for that env (actor
32 -> 64 -> 64 -> 16, critic 32 -> 64 -> 64 -> 1, tanh, seeded random weights), stochastic actions with value and logp.  Legs:

  abi                       HipBatch.step with pre-made action tensors (the reference point; bench.py's own `abi` leg)
  vecenv_torch              WindFarmVecEnv.step on CUDA tensors with pre-made actions
  closed_loop_torch_policy  venv.step(torch_forward(obs) -> sample -> clamp) in eager torch: what a user writes without k_policy
  closed_loop_hip_policy    venv.step(policy.act(obs)[0]): one k_policy launch per step
  rollout_hip_policy        venv.rollout(policy, api_steps): the whole loop inside the library, with final_value

With --multi the workload is cfg4 instead (3x3 farm, one agent per turbine, `presets.multi_3x3_config()`, 2048 envs by default) and
ONE policy shared by the turbines (obs_len -> 64 -> 64 -> 1), its critic per agent (`--critic agent`: obs_len -> 64 -> 64 -> 1) or
centralised on the flat observation (`--critic central`: obs_dim -> 64 -> 64 -> 1).  Legs: `vecenv_multi` (step with pre-made
actions), `loop_hip_policy` (the loop of single calls the rollout is documented as: act, value, step, value of the final rows) and
`rollout_hip_policy` (WindFarmVecEnvMulti.rollout: the same inside the library).

With --lstm H the same workload is also run with a recurrent policy (recurrent.MlpLstmPolicy: two LSTMs 32 -> H in front of the MLP
H -> 64 -> 64 -> 16 / 1), its legs beside the MLP's: `lstm_closed_loop_torch_policy` (torch_forward + sample + step in eager torch),
`lstm_closed_loop_hip_policy` (act + step: k_lstm, k_policy and the step kernel per step) and `lstm_rollout_hip_policy`
(venv.rollout: wg_rollout_lstm, with final_value).

usage: python tools/bench_policy.py [--envs 4096] [--api-steps 2000] [--lstm H] [--multi [--critic agent|central]]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def multi(args):
    """--multi: cfg4, one policy shared by the turbines, per-agent or centralised critic"""
    import torch
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnvMulti
    from windgym_amd.policy import MlpPolicy
    from windgym_amd.turbine import V80
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, steps = args.envs or 2048, args.api_steps
    menv = WindFarmVecEnvMulti(V80(), B, yaml_dict=presets.multi_3x3_config(), seed=1234, device=0, turbtype="None", n_passthrough=5,
                               n_rotor_pts=16)
    obs = menv.reset(seed=1234)
    N, Om, O = menv.n_turb, menv.obs_len, menv.batch.obs_dim
    central = args.critic == "central"
    policy = MlpPolicy(Om, 1, (64, 64), (64, 64), "tanh", device=0, seed=1234, n_in_vf=O if central else None)
    gen = torch.Generator(device="cpu").manual_seed(0)
    acts = list((torch.rand((16, B, N), generator=gen) * 2 - 1).to(dev).contiguous())
    for i in range(args.preroll):
        menv.step(acts[i % 16])

    def timed(fn):
        for i in range(50):
            fn(i)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i)
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        return {"value": B * steps / el, "unit": "env-steps/s", "ms_per_step": el / steps * 1e3}

    flat, flat_fin = menv.batch.obs, menv.batch.final_obs
    vbuf, fvbuf = (torch.zeros(B if central else B * N, device=dev) for _ in range(2))

    def loop_step(i):
        a = policy.act(obs)[0]
        if central:
            policy.value(flat, out=vbuf)
        fin = menv.step(a.view(B, N))[4]
        policy.value(flat_fin if central else fin, out=fvbuf)

    out = {"metric": "env-steps/s with ONE learned policy shared by the turbines, 3x3 farm x %d envs (%d agent rows), one GPU" % (B, B * N),
           "envs": B, "steps": steps, "critic": args.critic}
    out["vecenv_multi"] = timed(lambda i: menv.step(acts[i % 16]))
    out["loop_hip_policy"] = timed(loop_step)
    menv.rollout(policy, steps)                      # warm-up: allocates the buffers for this T
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    menv.rollout(policy, steps)
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t0
    out["rollout_hip_policy"] = {"value": B * steps / el, "unit": "env-steps/s", "ms_per_step": el / steps * 1e3}
    out["policy"] = {"n_in": Om, "n_out": 1, "n_in_vf": policy.n_in_vf, "hidden_pi": [64, 64], "hidden_vf": [64, 64], "activation": "tanh"}
    for k in ("loop_hip_policy", "rollout_hip_policy"):
        out[k]["frac_of_vecenv_multi"] = out[k]["value"] / out["vecenv_multi"]["value"]
    out["rollout_hip_policy"]["speedup_vs_loop"] = out["rollout_hip_policy"]["value"] / out["loop_hip_policy"]["value"]
    menv.batch.check()
    policy.close()
    menv.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=None, help="default: 4096 (--multi: 2048)")
    ap.add_argument("--multi", action="store_true", help="cfg4: one policy shared by the turbines of a 3x3 farm")
    ap.add_argument("--critic", choices=("agent", "central"), default="agent", help="with --multi: what the critic reads")
    ap.add_argument("--lstm", type=int, default=0, metavar="H", help="also time a recurrent policy with LSTMs of hidden size H (off: 0)")
    ap.add_argument("--api-steps", type=int, default=2000, help="timed steps of each leg")
    ap.add_argument("--preroll", type=int, default=300, help="untimed steps that take the batch out of its synchronised start")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_policy.py: no HIP device (there is no CPU path to time)")
    if args.multi:
        return multi(args)
    args.envs = args.envs or 4096
    from windgym_amd import binding, presets
    from windgym_amd.config import EnvConfig
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.policy import MlpPolicy
    from windgym_amd.turbine import V80
    if not torch.cuda.is_available():
        sys.exit("bench_policy.py: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, steps, warm = args.envs, args.api_steps, 50
    kw = dict(turbtype="None", n_passthrough=5, n_rotor_pts=16)
    gen = torch.Generator(device="cpu").manual_seed(0)
    n_act = 16
    acts = list((torch.rand((n_act, B, 16), generator=gen) * 2 - 1).to(dev).contiguous())

    def measure(step_fn):
        for i in range(warm):
            step_fn(i)
        torch.cuda.synchronize(dev)
        host = 0.0
        for i in range(200):
            t0 = time.perf_counter()
            step_fn(i)
            host += time.perf_counter() - t0
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(steps):
            step_fn(i)
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        return {"value": B * steps / el, "unit": "env-steps/s", "ms_per_step": el / steps * 1e3, "host_us_per_call": host / 200 * 1e6}

    out = {"metric": "env-steps/s with a learned policy in the loop, 16-turbine farm x %d envs, one GPU" % B, "envs": B, "steps": steps}
    abi = binding.HipBatch(EnvConfig(turbine=V80(), yaml_dict=presets.bench_cfg2_config(), n_envs=B, autoreset=True, **kw), device=0)
    abi.reset(seeds=[1234 + i for i in range(B)])
    for i in range(args.preroll):
        abi.step(acts[i % n_act])
    out["abi"] = measure(lambda i: abi.step(acts[i % n_act]))
    abi.check()
    abi.close()
    venv = WindFarmVecEnv(V80(), B, yaml_dict=presets.bench_cfg2_config(), seed=1234, device=0, as_torch=True, **kw)
    venv.reset(seed=1234)
    for i in range(args.preroll):
        venv.step(acts[i % n_act])
    out["vecenv_torch"] = measure(lambda i: venv.step(acts[i % n_act]))
    o_dim = venv.batch.obs_dim
    policy = MlpPolicy(o_dim, venv.n_turb, (64, 64), (64, 64), "tanh", device=0, seed=1234)
    log_std = policy.state_dict()["log_std"]
    state = {"obs": venv.batch.obs}

    def torch_step(i):
        with torch.no_grad():
            mean, value = policy.torch_forward(state["obs"])
            eps = torch.randn_like(mean)
            raw = mean + log_std.exp() * eps
            logp = (-0.5 * eps * eps - log_std - 0.9189385332046727).sum(-1)     # noqa: F841
            state["obs"] = venv.step(raw.clamp(-1.0, 1.0))[0]

    def hip_step(i):
        state["obs"] = venv.step(policy.act(state["obs"])[0])[0]

    out["closed_loop_torch_policy"] = measure(torch_step)
    state["obs"] = venv.batch.obs
    out["closed_loop_hip_policy"] = measure(hip_step)
    # rollout(): ONE call for `steps` steps; host_us_per_call = host time of that call / its steps (the enqueue cost per step
    # as long as the launch queue has room)
    venv.rollout(policy, steps)                      # warm-up: allocates the buffers for this T
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    venv.rollout(policy, steps)
    host = time.perf_counter() - t0
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    venv.rollout(policy, steps)
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t0
    out["rollout_hip_policy"] = {"value": B * steps / el, "unit": "env-steps/s", "ms_per_step": el / steps * 1e3,
                                 "host_us_per_call": host / steps * 1e6}
    out["policy"] = {"n_in": o_dim, "n_out": venv.n_turb, "hidden_pi": [64, 64], "hidden_vf": [64, 64], "activation": "tanh"}
    legs = ["vecenv_torch", "closed_loop_torch_policy", "closed_loop_hip_policy", "rollout_hip_policy"]
    if args.lstm:
        from windgym_amd.recurrent import MlpLstmPolicy
        rp = MlpLstmPolicy(o_dim, venv.n_turb, args.lstm, (64, 64), (64, 64), device=0, seed=1234)
        r_log_std = rp.state_dict()["log_std"]
        rs = {"obs": venv.batch.obs, "h": rp.initial_state(B), "start": torch.zeros(B, dtype=torch.uint8, device=dev)}

        def lstm_torch_step(i):
            with torch.no_grad():
                mean, value, rs["h"] = rp.torch_forward(rs["obs"], rs["h"], rs["start"])
                eps = torch.randn_like(mean)
                raw = mean + r_log_std.exp() * eps
                logp = (-0.5 * eps * eps - r_log_std - 0.9189385332046727).sum(-1)     # noqa: F841
                rs["obs"], _, _, trunc, _ = venv.step(raw.clamp(-1.0, 1.0))
                rs["start"] = trunc.view(torch.uint8)

        def lstm_hip_step(i):
            (a, _, _, _), _ = rp.act(rs["obs"], rs["h"], rs["start"], state_out=rs["h"])
            rs["obs"], _, _, trunc, _ = venv.step(a)
            rs["start"].copy_(trunc.view(torch.uint8))

        out["lstm_closed_loop_torch_policy"] = measure(lstm_torch_step)
        rs.update(obs=venv.batch.obs, h=rp.initial_state(B), start=torch.zeros(B, dtype=torch.uint8, device=dev))
        out["lstm_closed_loop_hip_policy"] = measure(lstm_hip_step)
        venv.rollout(rp, steps)                      # warm-up: allocates the buffers for this T
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        venv.rollout(rp, steps)
        host = time.perf_counter() - t0
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        venv.rollout(rp, steps)
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        out["lstm_rollout_hip_policy"] = {"value": B * steps / el, "unit": "env-steps/s", "ms_per_step": el / steps * 1e3,
                                          "host_us_per_call": host / steps * 1e6,
                                          "speedup_vs_torch": B * steps / el / out["lstm_closed_loop_torch_policy"]["value"],
                                          "frac_of_mlp_rollout": B * steps / el / out["rollout_hip_policy"]["value"]}
        out["lstm_policy"] = {"n_in": o_dim, "n_out": venv.n_turb, "lstm_hidden_size": args.lstm, "hidden_pi": [64, 64], "hidden_vf": [64, 64],
                              "shared_lstm": False, "activation": "tanh"}
        legs += ["lstm_closed_loop_torch_policy", "lstm_closed_loop_hip_policy", "lstm_rollout_hip_policy"]
        rp.close()
    venv.batch.check()
    policy.close()
    venv.close()
    for k in legs:
        out[k]["frac_of_abi"] = out[k]["value"] / out["abi"]["value"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
