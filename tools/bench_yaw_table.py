#!/usr/bin/env python
"""The yaw table beside what it replaces — one JSON line per leg.

Workload of tools/bench_ppo.py: cfg2 (4x4 farm, 16 turbines) x `--envs` envs (4096), T = `--n-steps` steps per rollout (128), SB3's
default MlpPolicy shape.  Every timed sample lies between two device synchronisations; legs that are compared ALTERNATE inside one
process, `--reps` times after a warm-up, and report the median and every sample.

  build        YawTable.build on the default grid of the env's ranges (1 m/s, 1 degree, three TI nodes): nodes, seconds
  closed_loop  venv.rollout(YawTableAgent) | venv.rollout(MlpPolicy) | T bare wg_step calls on a fixed action, alternating (ms per
               rollout), and the per-step cost of the SteadyStateYawVecAgent host loop over `--host-steps` steps.  The statement
               checked: the table rollout is not slower than the policy rollout by more than the spread of the repetitions.
  trainers     one iteration of PPO with a curriculum and of BehaviorCloning, the targets from the optimiser per rollout ("exact")
               and from the table, alternating (ms per iteration), and the parts of one collect of each (rollout / serial_refine /
               k_curriculum or labels / plumbing)
  quality      for `--winds` winds drawn uniformly from the env's ranges: steady farm power (k_steady, both wake models) with the
               table's yaws, with the optimiser's own yaws for the same winds and with zero yaws — the ratios table / exact and
               table / zero (mean and worst case), mean_yaw_diff between table and exact — at the default spacing and at half of
               it in wd

usage: python tools/bench_yaw_table.py [--envs 4096] [--n-steps 128] [--reps 5] [--legs build,closed_loop,trainers,quality]
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
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--winds", type=int, default=4096)
    ap.add_argument("--preroll", type=int, default=300, help="env steps before anything is timed (episodes out of phase)")
    ap.add_argument("--legs", default="build,closed_loop,trainers,quality")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_yaw_table.py: no HIP device (there is no CPU path to time)")
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.imitation import BehaviorCloning
    from windgym_amd.policy import MlpPolicy
    from windgym_amd.ppo import PPO
    from windgym_amd.steady import PyWakeVecAgent
    from windgym_amd.turbine import V80
    from windgym_amd.yaw_table import YawTable, YawTableAgent, default_axis
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, T, legs = args.envs, args.n_steps, args.legs.split(",")

    def sync():
        torch.cuda.synchronize(dev)

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def alternate(fns, reps=args.reps):
        """{name: samples in ms}: one warm-up round, then `reps` rounds of every leg in turn"""
        for fn in fns.values():
            fn()
        out = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                out[k].append(timed(fn))
        return out

    def summary(samples):
        return {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), samples_ms=[round(x, 3) for x in v])
                for k, v in samples.items()}

    def env():
        v = WindFarmVecEnv(V80(), B, yaml_dict=presets.bench_cfg2_config(), seed=1234, device=0, as_torch=True, turbtype="None", n_passthrough=5,
                           n_rotor_pts=16)
        v.reset(seed=1234)
        return v

    def emit(leg, **rec):
        print(json.dumps(dict(leg=leg, envs=B, n_steps=T, **rec)), flush=True)

    v = env()
    b, c = v.batch, v.cfg
    t0 = time.perf_counter()
    tab = YawTable.build(v)
    sync()
    build_s = time.perf_counter() - t0
    if "build" in legs:
        emit("build", n_ti=len(tab.ti), n_ws=len(tab.ws), n_wd=len(tab.wd), rows=tab.n_rows, seconds=round(build_s, 3), args=tab.args)

    if "closed_loop" in legs or "trainers" in legs:
        zero = torch.zeros((B, v.n_turb), dtype=torch.float32, device=dev)
        for _ in range(args.preroll):
            b.step(zero)
        sync()

    if "closed_loop" in legs:
        pol = MlpPolicy(b.obs_dim, v.n_turb, (64, 64), (64, 64), "tanh", device=0, seed=1)
        agent = YawTableAgent(tab, env=v)

        def bare():
            for _ in range(T):
                b.step(zero)
        s = alternate({"rollout_table": lambda: v.rollout(agent, T), "rollout_policy": lambda: v.rollout(pol, T), "bare_steps": bare})
        host = PyWakeVecAgent(env=v, yaw_max=c.yaw_max, yaw_min=c.yaw_min)
        host.predict()                                               # (its first call optimises in any case)
        per_step = []
        for _ in range(args.host_steps):
            per_step.append(timed(lambda: v.step(host.predict()[0])))
        r = summary(s)
        spread = r["rollout_policy"]["max_ms"] - r["rollout_policy"]["min_ms"]
        emit("closed_loop", **r, host_agent_ms_per_step=[round(x, 3) for x in per_step],
             table_minus_policy_ms=round(r["rollout_table"]["median_ms"] - r["rollout_policy"]["median_ms"], 3), policy_spread_ms=round(spread, 3),
             table_not_slower=bool(r["rollout_table"]["median_ms"] <= r["rollout_policy"]["median_ms"] + spread))
        pol.close()

    if "trainers" in legs:
        cur = dict(curriculum_steps=10 ** 9, pure_similarity_steps=10 ** 8)
        trainers = {}
        def rolled():                                                # every trainer on an env of its own, its episodes out of phase
            u = env()
            for _ in range(args.preroll):
                u.batch.step(zero)
            return u
        for name, kw in (("exact", {}), ("table", dict(targets=tab))):       # (tools/bench_ppo.py's 10 epochs, tools/bench_imitation.py's 4)
            trainers["ppo_curriculum_" + name] = PPO("MlpPolicy", rolled(), n_steps=T, n_epochs=10, seed=1, curriculum=dict(cur, **kw))
            trainers["bc_" + name] = BehaviorCloning("MlpPolicy", rolled(), n_steps=T, n_epochs=4, seed=1, **({"expert": tab} if kw else {}))
        s = alternate({k: (lambda tr=tr: tr.learn(T * B, log_interval=None)) for k, tr in trainers.items()})
        parts = {}
        for k, tr in trainers.items():
            timing = {}
            if k.startswith("bc"):
                tr.collect(timing=timing)
                n_new = tr.last_n_targets
            else:
                tr.curriculum.rollout(tr.policy, T, num_timesteps=tr.num_timesteps, timing=timing)
                n_new = tr.curriculum.last_n_targets
            parts[k] = dict({p: round(x, 3) for p, x in timing.items() if not p.startswith("_")}, serial_refine_conditions=n_new)
        emit("trainers", **summary(s), collect_parts_ms=parts)
        for tr in trainers.values():
            tr.venv.batch.check()

    if "quality" in legs:
        rng = np.random.default_rng(7)
        n = args.winds
        wind = np.stack([rng.uniform(c.ws_min, c.ws_max, n), rng.uniform(c.wd_min, c.wd_max, n), rng.uniform(c.TI_min, c.TI_max, n)], axis=1)
        dw = torch.from_numpy(wind).to(dev)
        exact = b.steady_optimize(wind[:, 0], wind[:, 1], wind[:, 2], model=tab.args["model"], refine_pass_n=tab.args["refine_pass_n"],
                                  yaw_n=tab.args["yaw_n"], yaw_max=tab.args["search_yaw_max"])[0]
        half = YawTable.build(v, wd=default_axis(c.wd_min, c.wd_max, 0.5))
        for name, table in (("default_spacing", tab), ("half_spacing_in_wd", half)):
            ty = table.targets(dw)
            rec = dict(n_wd=len(table.wd), rows=table.n_rows, mean_yaw_diff_deg=round(float((ty - exact).abs().mean()), 4),
                       max_yaw_diff_deg=round(float((ty - exact).abs().max()), 3))
            for model in ("m0", "blondel_jimenez"):
                pw = {k: b.steady_power(wind[:, 0], wind[:, 1] + 1e-3, wind[:, 2], y.float(), model=model).double().sum(dim=1)
                      for k, y in (("table", ty), ("exact", exact), ("zero", torch.zeros_like(exact)))}
                te, tz, ez = pw["table"] / pw["exact"], pw["table"] / pw["zero"], pw["exact"] / pw["zero"]
                rec[model] = dict(table_over_exact_mean=round(float(te.mean()), 5), table_over_exact_worst=round(float(te.min()), 5),
                                  table_over_zero_mean=round(float(tz.mean()), 5), table_over_zero_worst=round(float(tz.min()), 5),
                                  exact_over_zero_mean=round(float(ez.mean()), 5))
            emit("quality", spacing=name, winds=n, optimiser=tab.args, **rec)
        half.close()
    b.check()


if __name__ == "__main__":
    main()
