#!/usr/bin/env python
"""Training throughput on the device: one PPO iteration (rollout + update) and its parts — one JSON line.

Workload of tools/bench_policy.py: cfg2 (4x4 farm, 16 turbines, O = 32), `--envs` envs on one MI355X, SB3's default MlpPolicy
shape (actor 32 -> 64 -> 64 -> 16, critic 32 -> 64 -> 64 -> 1, tanh), T = `--n-steps` steps per rollout, `--epochs` epochs.
Every leg is warmed up once, then timed `--reps` times between two device synchronisations; the median is reported.  Legs:

  rollout            venv.rollout(policy, T) + wg_gae                                      (env-steps/s)
  update_torch_<mb>  the update in eager torch: torch_forward + autograd + clip_grad_norm_ + torch.optim.Adam, the same
                     permutations and minibatches — what a user writes without wg_ppo_update   (trained samples/s)
  update_hip_<mb>    wg_ppo_update (k_ppo_grad + clipping + Adam + repack per minibatch)        (trained samples/s)
  learn_hip          PPO.learn end to end at the first minibatch size, log_interval=None      (trained samples/s, i.e.
                     env-steps/s collected AND trained on for `epochs` epochs), with the share of an iteration spent collecting.

<mb> = minibatch rows, `--minibatches` (default 4096 and a quarter of the rollout).

With --multi the workload is cfg4 instead (3x3 farm, one agent per turbine, `presets.multi_3x3_config()`, 2048 envs by default), ONE
policy shared by the turbines and rows = AGENT rows (envs x steps x 9).  `--critic agent`: each agent's critic on its own observation
(wg_gae_shared + wg_ppo_update); `--critic central`: one critic per env on the flat observation (wg_gae on [T, B] +
wg_ppo_update_shared; the eager-torch leg gathers the env row of every minibatch entry the same way).

With --curriculum (single-agent workload only) the tool measures what the yaw curriculum adds instead: PPO.learn per iteration with
``curriculum=None`` and with a ``YawCurriculum``, the two ALTERNATING in one process (`--reps` pairs; medians and every sample are
reported), then `--reps` instrumented rollouts (``YawCurriculum.rollout(timing=...)``: device synchronisations between the parts)
that split the curriculum's share into the Serial-Refine launch (with the number of conditions C it served), k_curriculum and the
torch plumbing (the compaction's host synchronisation included).  The eager-torch legs are skipped.

With --normalize (single-agent workload only) the tool measures what VecNormalize adds: the closed-loop rate of ``venv.rollout``, of
``VecNormalize.rollout`` with ``norm_obs`` on (with and without the reward post-pass) and with ``norm_obs`` off (the normalised buffers
are copies), and PPO.learn per iteration with ``normalize=None`` and with a ``VecNormalize`` — the legs ALTERNATING in one process
(`--reps` rounds; median, min and max are reported).  The eager-torch legs are skipped.

With --adaptive-lr the trainer is built with ``adaptive_lr=dict(desired_kl=0.01)``: update_hip_<mb> and learn_hip then run with the
KL-adaptive rate set on the handle (k_ppo_adam_kl in k_ppo_adam's place), the eager-torch legs are skipped; a run without the switch
on the same machine is the other side of the comparison.

usage: python tools/bench_ppo.py [--envs 4096] [--n-steps 128] [--epochs 10] [--reps 5] [--multi [--critic agent|central]]
                                 [--curriculum | --normalize] [--adaptive-lr]
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

HALF_LOG_2PI = 0.9189385332046727


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=None, help="default: 4096 (--multi: 2048)")
    ap.add_argument("--multi", action="store_true", help="cfg4: one policy shared by the turbines of a 3x3 farm")
    ap.add_argument("--critic", choices=("agent", "central"), default="agent", help="with --multi: what the critic reads")
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=3, help="repetitions of the eager-torch legs (they are slow)")
    ap.add_argument("--minibatches", type=int, nargs="*", default=None)
    ap.add_argument("--preroll", type=int, default=300)
    ap.add_argument("--curriculum", action="store_true", help="measure PPO with and without a YawCurriculum, and the curriculum's parts")
    ap.add_argument("--normalize", action="store_true", help="measure rollouts and PPO with and without a VecNormalize")
    ap.add_argument("--adaptive-lr", action="store_true", help="every leg with the KL-adaptive learning rate set (adaptive_lr=dict(desired_kl=0.01)); "
                    "the eager-torch legs are skipped: compare with a run without the switch")
    args = ap.parse_args()
    if (args.curriculum or args.normalize) and args.multi:
        ap.error("--curriculum / --normalize measure the single-agent workload")
    if args.curriculum and args.normalize:
        ap.error("--curriculum and --normalize are two measurements: run them one at a time")
    import torch
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv, WindFarmVecEnvMulti
    from windgym_amd.ppo import PPO
    from windgym_amd.turbine import V80
    if not torch.cuda.is_available():
        sys.exit("bench_ppo.py: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, T, E = args.envs or (2048 if args.multi else 4096), args.n_steps, args.epochs
    central = args.multi and args.critic == "central"
    if args.multi:
        venv = WindFarmVecEnvMulti(V80(), B, yaml_dict=presets.multi_3x3_config(), seed=1234, device=0, turbtype="None", n_passthrough=5,
                                   n_rotor_pts=16)
    else:
        venv = WindFarmVecEnv(V80(), B, yaml_dict=presets.bench_cfg2_config(), seed=1234, device=0, as_torch=True, turbtype="None",
                              n_passthrough=5, n_rotor_pts=16)
    A = venv.n_turb if args.multi else 1                    # agent rows per env step
    n_rows = B * T * A
    mbs = args.minibatches or sorted({min(4096, n_rows), max(1, n_rows // 4)})
    venv.reset(seed=1234)
    ppo = PPO("MlpPolicy", venv, n_steps=T, n_epochs=E, batch_size=mbs[0], seed=1234, critic=args.critic if args.multi else None,
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
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), ts

    if args.curriculum:
        from windgym_amd.curriculum import YawCurriculum
        iters = 3
        cur = YawCurriculum(venv, curriculum_steps=100 * B * T, pure_similarity_steps=10 * B * T)
        ppo_c = PPO("MlpPolicy", venv, n_steps=T, n_epochs=E, batch_size=mbs[0], seed=1234, curriculum=cur)
        legs = {"plain": ppo, "curriculum": ppo_c}
        for x in legs.values():                                  # warm-up: every shape, both trainers
            x.learn(B * T, log_interval=None)
        torch.cuda.synchronize(dev)
        ms = {k: [] for k in legs}
        for _ in range(args.reps):                               # A/B in one process, alternating
            for k, x in legs.items():
                t0 = time.perf_counter()
                x.learn(iters * B * T, log_interval=None)
                torch.cuda.synchronize(dev)
                ms[k].append((time.perf_counter() - t0) * 1e3 / iters)
        parts = []
        for _ in range(args.reps):
            d = {}
            cur.rollout(ppo_c.policy, T, num_timesteps=ppo_c.num_timesteps, timing=d)
            d.pop("_t")
            d["C"] = cur.last_n_targets
            parts.append({k: round(v, 3) if k != "C" else v for k, v in d.items()})
        med = lambda xs: statistics.median(xs)                  # noqa: E731
        res = {"metric": "PPO on the device with and without the yaw curriculum, 16-turbine farm x %d envs x %d steps, %d epochs, one GPU" % (B, T, E),
               "envs": B, "n_steps": T, "epochs": E, "minibatch": mbs[0], "iterations_per_sample": iters,
               "learn_plain": {"ms_per_iteration": med(ms["plain"]), "ms_all": [round(x, 3) for x in ms["plain"]]},
               "learn_curriculum": {"ms_per_iteration": med(ms["curriculum"]), "ms_all": [round(x, 3) for x in ms["curriculum"]]},
               "added_ms_per_iteration": med(ms["curriculum"]) - med(ms["plain"]),
               "curriculum_rollout_parts_ms": {k: med([p.get(k, 0.0) for p in parts]) for k in ("rollout", "serial_refine", "k_curriculum", "plumbing", "C")},
               "curriculum_rollout_parts_all": parts,
               "model": cur.model, "refine_pass_n": cur.refine_pass_n, "yaw_n": cur.yaw_n}
        venv.batch.check()
        for x in legs.values():
            x.close(); x.policy.close()
        cur.close(); venv.close()
        print(json.dumps(res))
        return

    if args.normalize:
        from windgym_amd.normalize import VecNormalize
        iters = 3
        vn_on, vn_off = VecNormalize(venv), VecNormalize(venv, norm_obs=False)
        ppo_n = PPO("MlpPolicy", venv, n_steps=T, n_epochs=E, batch_size=mbs[0], seed=1234, normalize=vn_on)
        rolls = {"venv_rollout": lambda: venv.rollout(pol, T),
                 "norm_obs_on": lambda: vn_on.rollout(pol, T),
                 "norm_obs_on_no_reward_pass": lambda: vn_on.rollout(pol, T, normalize_reward=False),
                 "norm_obs_off": lambda: vn_off.rollout(pol, T)}
        learns = {"plain": ppo, "normalize": ppo_n}
        for fn in rolls.values():                                # warm-up: every buffer set, every kernel
            fn()
        for x in learns.values():
            x.learn(B * T, log_interval=None)
        torch.cuda.synchronize(dev)
        ms = {k: [] for k in list(rolls) + ["learn_" + k for k in learns]}
        for _ in range(args.reps):                               # every leg once per round: the legs alternate
            for k, fn in rolls.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                ms[k].append((time.perf_counter() - t0) * 1e3)
            for k, x in learns.items():
                t0 = time.perf_counter()
                x.learn(iters * B * T, log_interval=None)
                torch.cuda.synchronize(dev)
                ms["learn_" + k].append((time.perf_counter() - t0) * 1e3 / iters)
        stat = lambda xs: {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}      # noqa: E731
        res = {"metric": "VecNormalize on the device, 16-turbine farm x %d envs x %d steps, %d epochs, one GPU" % (B, T, E),
               "envs": B, "n_steps": T, "epochs": E, "minibatch": mbs[0], "reps": args.reps, "iterations_per_learn_sample": iters,
               "rollout_ms": {k: stat(ms[k]) for k in rolls},
               "rollout_env_steps_per_s": {k: round(B * T / (statistics.median(ms[k]) * 1e-3), 1) for k in rolls},
               "us_per_step_added_by_norm_obs": round((statistics.median(ms["norm_obs_on_no_reward_pass"]) - statistics.median(ms["venv_rollout"])) * 1e3 / T, 3),
               "learn_ms_per_iteration": {k: stat(ms["learn_" + k]) for k in learns},
               "ret_rms_var": vn_on.ret_rms[1]}
        venv.batch.check()
        for x in learns.values():
            x.close(); x.policy.close()
        vn_on.close(); vn_off.close(); venv.close()
        print(json.dumps(res))
        return

    out = {"metric": "PPO on the device, %s x %d envs x %d steps, %d epochs, one GPU"
                     % ("3x3 farm, one policy shared by 9 agents, critic per %s" % ("env (central)" if central else "agent") if args.multi
                        else "16-turbine farm", B, T, E),
           "envs": B, "n_steps": T, "epochs": E, "rows": n_rows, "minibatches": mbs}
    if args.multi:
        out["critic"] = args.critic
    el, ts = timed(ppo.collect, args.reps)
    out["rollout"] = {"value": B * T / el, "unit": "env-steps/s", "ms": el * 1e3, "ms_all": [round(x * 1e3, 3) for x in ts]}
    roll = ppo.collect()
    torch.cuda.synchronize(dev)
    O, N = pol.n_in, pol.n_out
    obs, raw, lpo = roll["obs"][:T].reshape(-1, O), roll["raw"].reshape(-1, N), roll["logp"].reshape(-1)
    adv, ret = ppo._adv.reshape(-1), ppo._ret.reshape(-1)
    obs_vf = roll["flat_obs"][:T].reshape(-1, pol.n_in_vf) if central else None     # [T * B, O]: the env rows the critic reads
    shared = dict(obs_vf=obs_vf, agents=A) if central else {}
    perm = torch.stack([torch.randperm(n_rows, device=dev) for _ in range(E)]).to(torch.int32).contiguous()
    start = pol.params.clone()

    def update_torch(bs):
        w = start.clone().requires_grad_(True)
        saved, pol.params = pol.params, w
        opt = torch.optim.Adam([w], lr=3e-4, eps=1e-5)
        try:
            for e in range(E):
                for s in range(0, n_rows, bs):
                    i = perm[e, s:s + bs].long()
                    if central:                          # entry i is an agent row of env row i // A
                        r = i // A
                        mean, V = pol.torch_forward(obs[i], obs_vf[r])
                        adv_i, ret_i = adv[r], ret[r]
                    else:
                        mean, V = pol.torch_forward(obs[i])
                        adv_i, ret_i = adv[i], ret[i]
                    ls = w[-N:]
                    z = (raw[i] - mean) / ls.exp()
                    logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(1)
                    ratio = (logp - lpo[i]).exp()
                    An = (adv_i - adv_i.mean()) / (adv_i.std() + 1e-8)
                    loss = -torch.min(ratio * An, ratio.clamp(0.8, 1.2) * An).mean() + 0.5 * ((ret_i - V) ** 2).mean()
                    opt.zero_grad()
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_([w], 0.5)
                    opt.step()
        finally:
            pol.params = saved

    def update_hip(bs):
        with torch.no_grad():
            pol.params.copy_(start)
        pol.sync()
        ppo.opt.load_state(torch.zeros(2 * start.numel()).numpy(), 0)
        ppo.opt.update(obs, raw, lpo, adv, ret, perm, bs, learning_rate=3e-4, max_grad_norm=0.5, **shared)

    out["adaptive_lr"] = bool(args.adaptive_lr)
    for bs in mbs:
        if args.adaptive_lr:                    # (the rule is set on the handle: wg_ppo_update reads the rate from ppo.lr)
            el, ts = timed(lambda: update_hip(bs), args.reps)
            out["update_hip_%d" % bs] = {"value": n_rows * E / el, "unit": "trained samples/s", "ms": el * 1e3,
                                         "ms_all": [round(x * 1e3, 3) for x in ts]}
            continue
        el, ts = timed(lambda: update_torch(bs), args.torch_reps)
        out["update_torch_%d" % bs] = {"value": n_rows * E / el, "unit": "trained samples/s", "ms": el * 1e3,
                                       "ms_all": [round(x * 1e3, 3) for x in ts]}
        el, ts = timed(lambda: update_hip(bs), args.reps)
        out["update_hip_%d" % bs] = {"value": n_rows * E / el, "unit": "trained samples/s", "ms": el * 1e3,
                                     "ms_all": [round(x * 1e3, 3) for x in ts],
                                     "speedup_vs_torch": out["update_torch_%d" % bs]["ms"] / (el * 1e3)}
    with torch.no_grad():
        pol.params.copy_(start)
    pol.sync()
    iters = 3
    el, ts = timed(lambda: ppo.learn(iters * B * T, log_interval=None), args.reps)
    per_iter = el / iters
    out["learn_hip"] = {"value": n_rows / per_iter, "unit": "trained samples/s", "ms_per_iteration": per_iter * 1e3,
                        "minibatch": mbs[0], "collect_share": out["rollout"]["ms"] / (per_iter * 1e3),
                        "ms_all": [round(x * 1e3 / iters, 3) for x in ts]}
    venv.batch.check()
    ppo.close()
    pol.close()
    venv.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
