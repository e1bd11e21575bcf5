#!/usr/bin/env python
"""What the KL-adaptive learning rate does to a run — one JSON line per run (`k_ppo_adam_kl`, "Effect").

The 16-turbine farm the trainer tests run on (cfg2, `turbtype="None"`, `n_passthrough=1`, 16 rotor points, seed 77), `--envs` envs,
`PPO("MlpPolicy", venv, n_steps=--n-steps, n_epochs=--epochs, seed=11)` for `--iterations` iterations, every run on a fresh env of
the same seed: a fixed rate and `adaptive_lr=dict(desired_kl=--desired-kl)` started from it, for each rate of `--rates`.  Per run:
`approx_kl` (the iteration's mean over its minibatches) and the rate after every iteration, and over the last `--tail` iterations the
mean KL, the episodes ended, their mean return and the mean step reward.  Reported, not asserted.

usage: python tools/effect_kl_lr.py [--rates 3e-4 3e-3] [--desired-kl 0.01] [--envs 256] [--n-steps 64] [--epochs 10]
                                    [--iterations 40] [--tail 10] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", type=float, nargs="*", default=[3e-4, 3e-3])
    ap.add_argument("--desired-kl", type=float, default=0.01)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--n-steps", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--tail", type=int, default=10)
    ap.add_argument("--out", default=None, help="write the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.ppo import PPO
    from windgym_amd.turbine import V80
    if not torch.cuda.is_available():
        sys.exit("effect_kl_lr.py: no HIP device (there is no CPU path to train on)")
    B, T, n, tail = args.envs, args.n_steps, args.iterations, args.tail
    lines = []
    for lr0 in args.rates:
        for adaptive in (None, dict(desired_kl=args.desired_kl)):
            v = WindFarmVecEnv(V80(), B, yaml_dict=presets.bench_cfg2_config(), seed=77, as_torch=True, turbtype="None", n_passthrough=1,
                               n_rotor_pts=16)
            v.reset(seed=77)
            p = PPO("MlpPolicy", v, n_steps=T, n_epochs=args.epochs, seed=11, learning_rate=lr0, adaptive_lr=adaptive)
            p.learn(n * T * B)
            kl, last = [r["approx_kl"] for r in p.log], p.log[-tail:]
            n_ep = sum(r["n_episodes"] for r in last)
            rec = dict(learning_rate=lr0, adaptive=adaptive is not None, envs=B, n_steps=T, iterations=n,
                       approx_kl_iter=[round(x, 5) for x in kl], lr_iter=[float("%.3g" % r["learning_rate"]) for r in p.log],
                       approx_kl_first5=sum(kl[:5]) / 5, approx_kl_last10=sum(kl[-tail:]) / tail, approx_kl_max=max(kl),
                       mean_episode_return_last10=sum(r["mean_episode_return"] * r["n_episodes"] for r in last) / max(n_ep, 1),
                       episodes_last10=n_ep, mean_step_reward_last10=sum(r["mean_step_reward"] for r in last) / tail)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            p.close(); p.policy.close(); v.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
