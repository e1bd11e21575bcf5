#!/usr/bin/env python
"""Recurrent training throughput on the device: one RecurrentPPO iteration (rollout + update) and the same update by two eager-torch
baselines on the same buffers — one JSON line per size.

Workload: cfg2 (4x4 farm, 16 turbines, O = 32), sb3-contrib's default MlpLstmPolicy heads (64, 64), T = `--n-steps` steps per
rollout, `--epochs` epochs of `--minibatches` minibatches of whole env sequences.  Sizes: 4096 envs x H = 256 and 256 envs x H = 64.
Legs, each in a child process of its own under a time limit of its own (`--leg-timeout` seconds; a leg that runs out is reported as
``"timeout"``), every child building the same env, policy, rollout and permutations from the same seeds:

  hip      venv.rollout + wg_gae (``rollout_ms``) and wg_lstm_ppo_update (``train_ms``), medians of `--reps`
  torch_a  the update by MlpLstmPolicy.torch_forward step by step + autograd + clip_grad_norm_ + torch.optim.Adam: what a user
           writes without the BPTT kernels — the baseline ``train_ms`` must not lose to
  torch_b  the same with torch.nn.LSTM (the vendor library's LSTM) over the whole sequence.  It ignores the episode starts INSIDE
           the rollout (a fused sequence call cannot reset single rows mid-way), so it is a lower bound of what a correct trainer on
           that path costs; reported with no bar.

With ``--members P`` the sizes are envs PER MEMBER and the legs are the two ways to run P recurrent runs of that size, one JSON line
per size (``rollout_*_ms`` / ``train_*_ms`` of ONE iteration of all P runs, medians of `--reps`, and their ratios):

  pop      a RecurrentPPOPopulation of P members on P x envs envs: venv.rollout + wg_gae_pop, and ONE wg_lstm_pop_update
  seq      the same P runs one after another: P RecurrentPPO objects, each on a shard env of its own — the sum of their rollouts (+
           wg_gae) and of their wg_lstm_ppo_update calls.  It uses single-policy entries only, so it also runs from a checkout of an
           earlier commit (`--legs seq`), which is how the population is compared against the build before it.

usage: python tools/bench_recurrent_ppo.py [--sizes 4096x256 256x64] [--n-steps 128] [--epochs 10] [--minibatches 4] [--reps 3]
       python tools/bench_recurrent_ppo.py --members 16 --sizes 256x64 [--legs pop seq]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HALF_LOG_2PI = 0.9189385332046727


def leg(args):
    import torch
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.recurrent_ppo import RecurrentPPO
    from windgym_amd.turbine import V80
    if not torch.cuda.is_available():
        sys.exit("bench_recurrent_ppo.py: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, H = (int(x) for x in args.leg_size.split("x"))
    T, E = args.n_steps, args.epochs
    Bm = -(-B // args.minibatches)
    venv = WindFarmVecEnv(V80(), B, yaml_dict=presets.bench_cfg2_config(), seed=1234, device=0, as_torch=True, turbtype="None",
                          n_passthrough=5, n_rotor_pts=16)
    venv.reset(seed=1234)
    ppo = RecurrentPPO("MlpLstmPolicy", venv, n_steps=T, n_epochs=E, batch_size=Bm * T, seed=1234, policy_kwargs=dict(lstm_hidden_size=H),
                       adaptive_lr=dict(desired_kl=0.01) if args.adaptive_lr else None)
    pol = ppo.policy
    zero = torch.zeros((B, venv.n_turb), device=dev)
    for _ in range(args.preroll):
        venv.step(zero)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": statistics.median(ts), "ms_all": [round(x, 3) for x in ts]}

    out = {}
    if args.leg == "hip":
        out["rollout"] = timed(ppo.collect, args.reps)
    roll = ppo.collect()
    torch.cuda.synchronize(dev)
    N = pol.n_out
    obs, raw, lpo, es, s0 = roll["obs"], roll["raw"], roll["logp"], roll["episode_start"], roll["lstm_state0"]
    adv, ret = ppo._adv, ppo._ret
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    perm = torch.stack([torch.randperm(B, device=dev, generator=gen) for _ in range(E)]).to(torch.int32).contiguous()
    start = pol.params.clone()

    def ppo_step(w, opt, mean, V, envs):
        ls = w[-N:]
        z = (raw[:, envs].reshape(-1, N) - mean) / ls.exp()
        logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(1)
        ratio = (logp - lpo[:, envs].reshape(-1)).exp()
        A = adv[:, envs].reshape(-1)
        A = (A - A.mean()) / (A.std() + 1e-8)
        loss = -torch.min(ratio * A, ratio.clamp(0.8, 1.2) * A).mean() + 0.5 * ((ret[:, envs].reshape(-1) - V) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([w], 0.5)
        opt.step()

    def update_torch(vendor):
        w = start.clone().requires_grad_(True)
        saved, pol.params = pol.params, w
        saved_mlp, pol.mlp.params = pol.mlp.params, w[pol.n_lstm_params:]
        opt = torch.optim.Adam([w], lr=3e-4, eps=1e-5)
        lstms = [torch.nn.LSTM(pol.n_in, pol.H).to(dev) for _ in range(pol.nets)] if vendor else None
        try:
            for e in range(E):
                for s in range(0, B, Bm):
                    envs = perm[e, s:s + Bm].long()
                    pol.mlp.params = w[pol.n_lstm_params:]
                    if vendor:
                        v = pol._views(w)
                        hs = []
                        fresh = es[0, envs].bool().reshape(1, -1, 1)
                        for i, net in enumerate(("lstm_actor", "lstm_critic")[:pol.nets]):
                            st = tuple(torch.where(fresh, torch.zeros_like(x), x).contiguous() for x in (s0[i, 0][envs][None], s0[i, 1][envs][None]))
                            pr = {k: v[f"{net}.{k}"] for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")}
                            hs.append(torch.func.functional_call(lstms[i], pr, (obs[:T, envs], st))[0])
                        mean, V = pol.mlp.torch_forward(hs[0].reshape(-1, pol.H), obs_vf=hs[-1].reshape(-1, pol.H))
                    else:
                        state, means, values = s0[:, :, envs], [], []
                        for t in range(T):
                            m, val, state = pol.torch_forward(obs[t, envs], state, es[t, envs])
                            means.append(m); values.append(val)
                        mean, V = torch.cat(means), torch.cat(values)
                    ppo_step(w, opt, mean, V.reshape(-1), envs)
        finally:
            pol.params, pol.mlp.params = saved, saved_mlp

    def update_hip():
        with torch.no_grad():
            pol.params.copy_(start)
        pol.sync()
        ppo.opt.load_state(torch.zeros(2 * start.numel()).numpy(), 0)
        ppo.opt.update(roll, perm, Bm, learning_rate=3e-4, max_grad_norm=0.5)

    if args.leg == "hip":
        out["train"] = timed(update_hip, args.reps)
    else:
        out["train"] = timed(lambda: update_torch(args.leg == "torch_b"), args.torch_reps)
    venv.batch.check()
    ppo.close(); pol.close(); venv.close()
    print("LEG " + json.dumps(out))


def members_leg(args):
    """The `pop` / `seq` leg of ``--members P``: P runs of `--leg-size` (envs per member x H) -> rollout and train of one iteration."""
    import torch
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.turbine import V80
    if not torch.cuda.is_available():
        sys.exit("bench_recurrent_ppo.py: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    P = args.members
    Bm, H = (int(x) for x in args.leg_size.split("x"))
    T, E = args.n_steps, args.epochs
    epb = -(-Bm // args.minibatches)
    kw = dict(n_steps=T, n_epochs=E, batch_size=epb * T, policy_kwargs=dict(lstm_hidden_size=H),
              adaptive_lr=dict(desired_kl=0.01) if args.adaptive_lr else None)
    seeds = [1234 + m for m in range(P)]

    def env(n):
        return WindFarmVecEnv(V80(), n, yaml_dict=presets.bench_cfg2_config(), seed=1234, device=0, as_torch=True, turbtype="None",
                              n_passthrough=5, n_rotor_pts=16)
    if args.leg == "pop":
        from windgym_amd.recurrent_population import RecurrentPPOPopulation
        venvs = [env(P * Bm)]
        venvs[0].reset(seed=1234)
        runs = [RecurrentPPOPopulation("MlpLstmPolicy", venvs[0], n_members=P, seed=seeds, **kw)]
        policies, opts = runs[0].members, runs[0].opts
    else:
        from windgym_amd.recurrent_ppo import RecurrentPPO
        venvs = [env(Bm).shard(m, P) for m in range(P)]
        for v in venvs:
            v.reset(seed=1234)
        runs = [RecurrentPPO("MlpLstmPolicy", v, seed=s, **kw) for v, s in zip(venvs, seeds)]
        policies, opts = [r.policy for r in runs], [r.opt for r in runs]
    for v in venvs:
        zero = torch.zeros((v.num_envs, v.n_turb), device=dev)
        for _ in range(args.preroll):
            v.step(zero)

    def timed(fn, before=None):
        ts = []
        for i in range(args.reps + 1):               # (the first one warms up)
            if before is not None:
                before()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": statistics.median(ts[1:]), "ms_all": [round(x, 3) for x in ts[1:]]}

    out = {"rollout": timed(lambda: [r.collect() for r in runs])}
    rolls = [r.collect() for r in runs]
    start = [p.params.clone() for p in policies]

    def reset():                                      # every repetition trains the same weights from Adam's zero state
        for p, o, w in zip(policies, opts, start):
            with torch.no_grad():
                p.params.copy_(w)
            p.sync()
            o.load_state(torch.zeros(2 * w.numel()).numpy(), 0)

    def train():
        for r, roll in zip(runs, rolls):
            r.train(roll, [3e-4] * P if args.leg == "pop" else 3e-4, [0.2] * P if args.leg == "pop" else 0.2)
    out["train"] = timed(train, reset)
    for v in venvs:
        v.batch.check()
    for x in runs + list(policies) + venvs:
        x.close()
    print("LEG " + json.dumps(out))


def members_main(args):
    legs = [x for x in args.legs if x in ("pop", "seq")] or ["pop", "seq"]
    for size in args.sizes:
        Bm, H = (int(x) for x in size.split("x"))
        res = {"metric": "%d recurrent PPO runs of %d envs x %d steps, LSTM H = %d, %d epochs x %d minibatches, 16-turbine farm, one GPU: a "
                         "population (pop) against the runs one after another (seq), per iteration of all runs"
                         % (args.members, Bm, args.n_steps, H, args.epochs, args.minibatches),
               "members": args.members, "envs_per_member": Bm, "hidden": H, "n_steps": args.n_steps, "epochs": args.epochs,
               "minibatches": args.minibatches, "adaptive_lr": bool(args.adaptive_lr)}
        for name in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--leg-size", size, "--members", str(args.members), "--n-steps",
                   str(args.n_steps), "--epochs", str(args.epochs), "--minibatches", str(args.minibatches), "--reps", str(args.reps),
                   "--preroll", str(args.preroll)] + (["--adaptive-lr"] if args.adaptive_lr else [])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
                lines = [x for x in r.stdout.splitlines() if x.startswith("LEG ")]
                got = json.loads(lines[-1][4:]) if r.returncode == 0 and lines else {"error": (r.stderr or r.stdout)[-400:]}
            except subprocess.TimeoutExpired:
                got = "timeout"
            if isinstance(got, dict) and "train" in got:
                for k in ("rollout", "train"):
                    res["%s_%s_ms" % (k, name)], res["%s_%s_ms_all" % (k, name)] = got[k]["ms"], got[k]["ms_all"]
            else:
                res[name] = got
                break                                            # a leg that hung or died: start nothing more on the device
        for k in ("rollout", "train"):
            if "%s_pop_ms" % k in res and "%s_seq_ms" % k in res:
                res["%s_seq_over_pop" % k] = res["%s_seq_ms" % k] / res["%s_pop_ms" % k]
        print(json.dumps(res), flush=True)
        if any(k in res for k in legs):
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["4096x256", "256x64"], help="<envs>x<lstm_hidden_size>")
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=1, help="repetitions of the eager-torch legs (they are slow)")
    ap.add_argument("--preroll", type=int, default=300)
    ap.add_argument("--legs", nargs="*", default=["hip", "torch_a", "torch_b"])
    ap.add_argument("--leg-timeout", type=float, default=240.0, help="seconds each leg's process may take")
    ap.add_argument("--members", type=int, default=0, help="P > 0: the sizes are envs per member, the legs `pop` and `seq` (module docstring)")
    ap.add_argument("--adaptive-lr", action="store_true", help="the device legs (hip, pop, seq) with the KL-adaptive learning rate set "
                    "(adaptive_lr=dict(desired_kl=0.01)): compare with a run without the switch")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--leg-size", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.members:
        return members_leg(args) if args.leg else members_main(args)
    if args.leg:
        return leg(args)
    for size in args.sizes:
        B, H = (int(x) for x in size.split("x"))
        res = {"metric": "RecurrentPPO on the device, 16-turbine farm x %d envs x %d steps, LSTM H = %d, %d epochs x %d minibatches, one GPU"
                         % (B, args.n_steps, H, args.epochs, args.minibatches),
               "envs": B, "hidden": H, "n_steps": args.n_steps, "epochs": args.epochs, "minibatches": args.minibatches,
               "adaptive_lr": bool(args.adaptive_lr)}
        for name in args.legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--leg-size", size, "--n-steps", str(args.n_steps), "--epochs",
                   str(args.epochs), "--minibatches", str(args.minibatches), "--reps", str(args.reps), "--torch-reps", str(args.torch_reps),
                   "--preroll", str(args.preroll)] + (["--adaptive-lr"] if args.adaptive_lr else [])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
                lines = [x for x in r.stdout.splitlines() if x.startswith("LEG ")]
                got = json.loads(lines[-1][4:]) if r.returncode == 0 and lines else {"error": (r.stderr or r.stdout)[-400:]}
            except subprocess.TimeoutExpired:
                got = "timeout"
            if name == "hip" and isinstance(got, dict) and "train" in got:
                res["rollout_ms"], res["train_ms"] = got["rollout"]["ms"], got["train"]["ms"]
                res["rollout_ms_all"], res["train_ms_all"] = got["rollout"]["ms_all"], got["train"]["ms_all"]
            elif isinstance(got, dict) and "train" in got:
                res["train_%s_ms" % name], res["train_%s_ms_all" % name] = got["train"]["ms"], got["train"]["ms_all"]
            else:
                res[name] = got
            if got == "timeout" or (isinstance(got, dict) and "error" in got):
                break                                        # a leg that hung or died: start nothing more on the device
        if "train_ms" in res and "train_torch_a_ms" in res:
            res["speedup_vs_torch_a"] = res["train_torch_a_ms"] / res["train_ms"]
        print(json.dumps(res), flush=True)
        if any(res.get(k) == "timeout" or (isinstance(res.get(k), dict) and "error" in res[k]) for k in args.legs):
            break


if __name__ == "__main__":
    main()
