"""GPU box: one fixed scenario (seeds, actions) through step(), or through the policy kernels; every output goes to an .npz — run it
under two builds (WG_LIB=... with WG_DEBUG_HOOKS=1) and compare the files bit for bit:
    python tools/dump_run.py out_a.npz [workload] [n_envs] [steps];  python tools/dump_run.py --compare out_a.npz out_b.npz
    python tools/dump_run.py policy out_a.npz      k_policy / k_policy_pop / k_lstm at the kernels' edge shapes + 8-step closed loops
    python tools/dump_run.py train out_a.npz       two learn iterations of every trainer: parameters, Adam's state, statistics, logs"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    bad = [k for k in a.files if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]
    print("arrays:", len(a.files), "differing:", bad if bad else "none -> BIT-IDENTICAL")
    for k in bad:
        d = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))
        print("  ", k, "max |diff|", d.max(), "first step that differs", int(np.argmax(d.reshape(d.shape[0], -1).max(1) > 0)))
    sys.exit(1 if bad else 0)
import torch  # noqa: E402
import bench  # noqa: E402
from windgym_amd import binding  # noqa: E402

MLP_SHAPES = [(7, (33,), 1, 33), (257, (64,), 3, 389), (2048, (256, 256), 128, 32)]        # (n_in, hidden, n_out, rows)
LSTM_SHAPES = [(3, 1, 1, False), (7, 40, 31, True), (257, 64, 389, False), (300, 256, 33, False)]     # (n_in, H, rows, shared_lstm)


def dump_policy(out):
    """MlpPolicy.act (deterministic, stochastic with value) and Population.act (P = 3, on the rows that divide by 3) per MLP shape,
    three chained MlpLstmPolicy.act and RecurrentPopulation.act (P = 3, on the rows that divide by 3) per LSTM shape, then one 8-step
    venv.rollout of a policy, of a population (P = 2: the members own equal shares of the 4 envs), of a recurrent policy and of a
    recurrent population (P = 2) on 4 envs of the 2-turbine preset.  Every weight and input is drawn on the host from fixed seeds."""
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv
    from windgym_amd.policy import MlpPolicy
    from windgym_amd.population import Population
    from windgym_amd.recurrent import MlpLstmPolicy
    from windgym_amd.recurrent_population import RecurrentPopulation
    from windgym_amd.turbine import V80
    rng, A = np.random.default_rng(20), {}
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")          # noqa: E731
    names = ("action", "raw", "logp", "value")

    def keep(tag, tensors):
        for n, x in zip(names, tensors):
            A[f"{tag}_{n}"] = np.atleast_1d(x.cpu().numpy())

    for n_in, hidden, n_out, rows in MLP_SHAPES:
        tag = f"mlp{n_in}"
        ms = [MlpPolicy(n_in, n_out, hidden, hidden, "tanh", device=0, seed=5 + m) for m in range(3)]
        obs = dev(rng.uniform(-1, 1, (rows, n_in)).astype(np.float32))
        keep(tag + "_det", ms[0].act(obs, deterministic=True, counter=1))
        keep(tag + "_sto", ms[0].act(obs, counter=2))
        pop = Population(ms)
        keep(tag + "_pop", pop.act(obs[:rows // 3 * 3].contiguous(), counter=3))
        pop.close()
        for m in ms:
            m.close()
    for n_in, H, rows, shared in LSTM_SHAPES:
        tag = f"lstm{n_in}"
        p = MlpLstmPolicy(n_in, 3, H, (32,), (32,), shared_lstm=shared, device=0, seed=9)
        state = dev(rng.uniform(-1, 1, (p.nets, 2, rows, H)).astype(np.float32))
        for i in range(3):
            start = dev((rng.random(rows) < 0.3).astype(np.uint8))
            outs, state = p.act(dev(rng.uniform(-1, 1, (rows, n_in)).astype(np.float32)), state, start, counter=i)
            keep(f"{tag}_t{i}", outs)
            A[f"{tag}_t{i}_state"] = state.cpu().numpy()
            state = state.clone()
        p.close()
        n = rows // 3 * 3
        if n == 0:
            continue
        ms = [MlpLstmPolicy(n_in, 3, H, (32,), (32,), shared_lstm=shared, device=0, seed=40 + m) for m in range(3)]
        pop = RecurrentPopulation(ms)
        state = dev(rng.uniform(-1, 1, (3, pop.nets, 2, n // 3, H)).astype(np.float32))
        for i in range(3):
            start = dev((rng.random(n) < 0.3).astype(np.uint8))
            outs, state = pop.act(dev(rng.uniform(-1, 1, (n, n_in)).astype(np.float32)), state, start, counter=i)
            keep(f"{tag}_pop_t{i}", outs)
            A[f"{tag}_pop_t{i}_state"] = state.cpu().numpy()
            state = state.clone()
        pop.close()
        for m in ms:
            m.close()

    def venv():
        v = WindFarmVecEnv(V80(), 4, yaml_dict=presets.two_turb_config(), seed=77, as_torch=True, turbtype="None", n_passthrough=1)
        v.reset(seed=77)
        return v

    v = venv()
    O, N = v.batch.obs_dim, v.n_turb
    ms = [MlpPolicy(O, N, (64, 64), (64, 64), "tanh", device=0, seed=31 + m) for m in range(2)]
    pop, rec = Population(ms), MlpLstmPolicy(O, N, 64, (32,), (32,), device=0, seed=33)
    rpop = RecurrentPopulation([MlpLstmPolicy(O, N, 64, (32,), (32,), device=0, seed=34 + m) for m in range(2)])
    for tag, pol in (("roll_mlp", ms[0]), ("roll_pop", pop), ("roll_lstm", rec), ("roll_lstm_pop", rpop)):
        for k, x in v.rollout(pol, 8).items():
            A[f"{tag}_{k}"] = np.atleast_1d(x.cpu().numpy())
        v.close()
        v = venv()
    v.close()
    np.savez(out, **A)
    print("wrote", out, len(A), "arrays")


def dump_train(out):
    """Two ``learn`` iterations (n_steps = 8, 2 epochs, fixed seeds) on 4 envs of the 2-turbine preset of: PPO; PPO on the multi-agent
    env with the per-agent and with the centralised critic; PPO(normalize={}); PPOPopulation with P = 2; RecurrentPPO (H = 40) with an
    LSTM per net and with a shared one; RecurrentPPOPopulation with P = 2 (H = 40).  Kept per trainer: the parameters, ``opt.state()``, ``_stats``, ``_perm`` and the logged
    records without ``fps``."""
    from windgym_amd import presets
    from windgym_amd.envs import WindFarmVecEnv, WindFarmVecEnvMulti
    from windgym_amd.population import PPOPopulation
    from windgym_amd.ppo import PPO
    from windgym_amd.recurrent_population import RecurrentPPOPopulation
    from windgym_amd.recurrent_ppo import RecurrentPPO
    from windgym_amd.turbine import V80
    A, T, B = {}, 8, 4
    env_kw = dict(yaml_dict=presets.two_turb_config(), seed=77, turbtype="None", n_passthrough=1)
    kw = dict(n_steps=T, n_epochs=2, ent_coef=0.001)

    def single():
        return WindFarmVecEnv(V80(), B, as_torch=True, **env_kw)

    def multi():
        return WindFarmVecEnvMulti(V80(), B, **env_kw)

    def lstm(shared):
        return dict(policy_kwargs=dict(lstm_hidden_size=40, net_arch=[16], shared_lstm=shared))

    runs = [("ppo", single, PPO, "MlpPolicy", dict(seed=11)),
            ("ppo_multi_agent", multi, PPO, "MlpPolicy", dict(seed=12, critic="agent")),
            ("ppo_multi_central", multi, PPO, "MlpPolicy", dict(seed=13, critic="central")),
            ("ppo_normalize", single, PPO, "MlpPolicy", dict(seed=14, normalize={})),
            ("population", single, PPOPopulation, "MlpPolicy", dict(n_members=2, seed=[15, 16], learning_rate=[3e-4, 1e-3])),
            ("recurrent", single, RecurrentPPO, "MlpLstmPolicy", dict(seed=17, **lstm(False))),
            ("recurrent_shared", single, RecurrentPPO, "MlpLstmPolicy", dict(seed=18, **lstm(True))),
            ("recurrent_population", single, RecurrentPPOPopulation, "MlpLstmPolicy",
             dict(n_members=2, seed=[19, 20], learning_rate=[3e-4, 1e-3], **lstm(False)))]
    for tag, make, cls, policy, extra in runs:
        v = make()
        v.reset(seed=77)
        tr = cls(policy, v, **kw, **extra)
        tr.learn(2 * tr.n_env_steps)
        pairs = list(zip(tr.members, tr.opts)) if hasattr(tr, "opts") else [(tr.policy, tr.opt)]
        for m, (pol, opt) in enumerate(pairs):
            mv, step = opt.state()
            A[f"{tag}_{m}_params"], A[f"{tag}_{m}_adam"], A[f"{tag}_{m}_step"] = pol.params.cpu().numpy(), mv, np.array([step])
        A[f"{tag}_stats"], A[f"{tag}_perm"] = tr._stats.cpu().numpy(), tr._perm.cpu().numpy()
        assert len(tr.log) == 2
        recs = tr.log if isinstance(tr.log[0], dict) else [r for it in tr.log for r in it]
        keys = sorted(k for k in recs[0] if k != "fps")
        A[f"{tag}_log"] = np.array([[float("nan") if r[k] is None else float(r[k]) for k in keys] for r in recs], np.float64)
        tr.close()
        v.close()
    np.savez(out, **A)
    print("wrote", out, len(A), "arrays")


if sys.argv[1] in ("policy", "train"):
    (dump_policy if sys.argv[1] == "policy" else dump_train)(sys.argv[2])
    sys.exit(0)
out = sys.argv[1]
wl = sys.argv[2] if len(sys.argv) > 2 else "cfg2"
B = int(sys.argv[3]) if len(sys.argv) > 3 else 48
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 500
cfg = bench.make_cfg(B, autoreset=True, farms2=True, workload=wl)
env = binding.HipBatch(cfg, device=0)
if wl == "cfg5":      # frozen-box inflow: a box made on the host, the same under every build
    from windgym_amd.mann import generate_mann_box
    env.set_turbulence_box(generate_mann_box((256, 64, 32), (3.0, 3.0, 3.0), seed=1234), (3.0, 3.0, 3.0))
obs0 = env.reset(seeds=7 + np.arange(B))
gen = torch.Generator(device="cpu").manual_seed(3)
acts = (torch.rand((16, B, cfg.n_turb), generator=gen) * 2 - 1).to("cuda").contiguous()
O, R, T, F = [obs0.cpu().numpy()], [], [], []
for i in range(steps):
    o, r, t, f = env.step(acts[i % 16])
    O.append(o.cpu().numpy()); R.append(r.cpu().numpy()); T.append(t.cpu().numpy()); F.append(f.cpu().numpy())
env.check()
np.savez(out, obs=np.stack(O), rew=np.stack(R), trunc=np.stack(T), fin=np.stack(F),
         yaw=env.info("yaw_agent").cpu().numpy(), pw=env.info("power_turb_agent").cpu().numpy(), pwb=env.info("power_turb_base").cpu().numpy())
print("wrote", out, "variant", env.flow_variant(), "truncations", int(np.stack(T).sum()))
