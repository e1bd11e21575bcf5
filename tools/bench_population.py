#!/usr/bin/env python
"""Populations against the same members trained one after the other — one JSON line per (layout, P).

Workload and protocol of tools/bench_ppo.py: cfg2 (4x4 farm, 16 turbines, O = 32), SB3's default MlpPolicy shape, T = `--n-steps`
steps per rollout, `--epochs` epochs, four minibatches per epoch; every leg is warmed up once, then timed `--reps` times between
two device synchronisations, and the median is reported.  For P in `--members`, at (a) Bm = `--envs-member` envs per member
(B = P * Bm) and (b) B = `--envs-total` in total (Bm = B / P):

  pop_collect / pop_train   PPOPopulation.collect (wg_pop_rollout + wg_gae_pop) / .train (permutations + ONE wg_pop_update)
  seq_collect / seq_train   the same P members as P standalone PPO objects on envs of Bm each, one after the other
                            (P x venv.rollout + wg_gae, P x wg_ppo_update)

usage: python tools/bench_population.py [--members 1 2 4 8 16] [--envs-member 512] [--envs-total 4096] [--out FILE] [--adaptive-lr]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="*", default=[1, 2, 4, 8, 16])
    ap.add_argument("--envs-member", type=int, default=512)
    ap.add_argument("--envs-total", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--preroll", type=int, default=50)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--adaptive-lr", action="store_true", help="every trainer with the KL-adaptive learning rate set "
                    "(adaptive_lr=dict(desired_kl=0.01)): compare with a run without the switch")
    args = ap.parse_args()
    import torch
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.population import PPOPopulation
    from windgym_amd.ppo import PPO
    from windgym_amd.turbine import V80
    if not torch.cuda.is_available():
        sys.exit("bench_population.py: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T, E = args.n_steps, args.epochs
    adapt = dict(adaptive_lr=dict(desired_kl=0.01)) if args.adaptive_lr else {}

    def venv(B):
        v = WindFarmVecEnv(V80(), B, yaml_dict=presets.bench_cfg2_config(), seed=1234, device=0, as_torch=True, turbtype="None",
                           n_passthrough=5, n_rotor_pts=16)
        v.reset(seed=1234)
        zero = torch.zeros((B, v.n_turb), device=dev)
        for _ in range(args.preroll):
            v.step(zero)
        return v

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e3

    for layout in ("per_member", "total"):
        for P in args.members:
            Bm = args.envs_member if layout == "per_member" else args.envs_total // P
            B = P * Bm
            v = venv(B)
            pp = PPOPopulation("MlpPolicy", v, n_members=P, n_steps=T, n_epochs=E, seed=list(range(P)), **adapt)
            lr, clip = [3e-4] * P, [0.2] * P
            rec = {"metric": "PPO population vs the same members one after the other, 16-turbine farm, one GPU", "layout": layout,
                   "members": P, "envs_member": Bm, "envs": B, "n_steps": T, "epochs": E, "batch_size": pp.batch_size, "unit": "ms, median",
                   "adaptive_lr": bool(args.adaptive_lr)}
            rec["pop_collect"] = timed(pp.collect)
            out = pp.collect()
            rec["pop_train"] = timed(lambda: pp.train(out, lr, clip))
            pp.close()
            for m in pp.members:
                m.close()
            v.close()
            vs = [venv(Bm) for _ in range(P)]
            ps = [PPO("MlpPolicy", x, n_steps=T, n_epochs=E, seed=m, **adapt) for m, x in enumerate(vs)]
            rec["seq_collect"] = timed(lambda: [p.collect() for p in ps])
            outs = [{k: (x.clone() if torch.is_tensor(x) else x) for k, x in p.collect().items()} for p in ps]
            rec["seq_train"] = timed(lambda: [p.train(o, 3e-4, 0.2) for p, o in zip(ps, outs)])
            for p, x in zip(ps, vs):
                p.close(); p.policy.close(); x.close()
            rec["speedup_collect"] = rec["seq_collect"] / rec["pop_collect"]
            rec["speedup_train"] = rec["seq_train"] / rec["pop_train"]
            rec["speedup_iteration"] = (rec["seq_collect"] + rec["seq_train"]) / (rec["pop_collect"] + rec["pop_train"])
            line = json.dumps({k: (round(x, 3) if isinstance(x, float) else x) for k, x in rec.items()})
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
