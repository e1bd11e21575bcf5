"""The converse of test_plan.py's "no plan names a kernel that is not built": every step kernel that IS built (the three launch
tables, 74 instantiations, restated in tests/variant_census.py) is the one some case of variant_census.CASES launches — decided
on the CPU from the plan, so that tests/test_gpu_variant_census.py, which runs those cases by value, runs what is built."""
from collections import Counter

import numpy as np

import variant_census as vc
from test_plan import shim  # noqa: F401  (the g++-only plan fixture)


def test_the_launch_tables_build_74_instantiations():
    assert len(vc.ALL_KEYS) == len(set(vc.ALL_KEYS)) == 74
    assert Counter(k[0] for k in vc.ALL_KEYS) == {"k_flow": 36, "k_flow_env": 20, "k_flow_envb": 18}
    # the rows of wg_flow.hip's table: 20 + 8 + 8
    assert Counter((k[1], k[2]) for k in vc.K_FLOW_KEYS) == {(64, True): 20, (256, True): 8, (256, False): 8}
    assert set(vc.UNREACHABLE) <= set(vc.ALL_KEYS)


def test_every_built_instantiation_is_launched_by_a_case(shim):  # noqa: F811
    assert len({c.name for c in vc.CASES}) == len(vc.CASES)
    reached = {}
    for cs in vc.CASES:
        plan = vc.plan_of(shim, cs)
        assert plan["rc"] == 0, (cs.name, plan)
        reached.setdefault(vc.key_of(cs, plan), []).append(cs.name)
    missing = [k for k in vc.ALL_KEYS if k not in reached and k not in vc.UNREACHABLE]
    print(f"[variant census] {len(set(reached) & set(vc.ALL_KEYS))} / {len(vc.ALL_KEYS)} keys reached by {len(vc.CASES)} cases; "
          f"unreachable: {sorted(vc.UNREACHABLE)}")
    assert missing == [], missing
    assert set(reached) == set(vc.ALL_KEYS) - set(vc.UNREACHABLE), set(reached) - set(vc.ALL_KEYS)
    # the cases with noise on all four channels run one instantiation of each kernel family
    four = {vc.key_of(c, vc.plan_of(shim, c))[0] for c in vc.CASES if dict(c.kw).get("all_channels")}
    assert four == {"k_flow", "k_flow_env", "k_flow_envb"}
    for name in vc.CONTROLS:
        assert dict(vc.case(name).kw)["noise"]
    assert {vc.key_of(vc.case(n), vc.plan_of(shim, vc.case(n)))[0] for n in vc.CONTROLS} == {"k_flow", "k_flow_env", "k_flow_envb"}


def test_fused_cases_are_fused_and_all_channel_cases_carry_four_sigmas(shim):  # noqa: F811
    for cs in vc.CASES:
        c = cs.cfg().to_c()
        if cs.multi:      # the per-agent buffer selects glue 2 on a fused handle only
            assert vc.plan_of(shim, cs)["path_fused"] == 1, cs.name
        sig = tuple(c.noise_sigma[i] for i in range(4))
        assert sig == (vc.AllChannelNoiseConfig.SIGMA if dict(cs.kw).get("all_channels") else (0.0, 2.0, 0.0, 0.0)), cs.name


def test_noise_is_alive_in_every_noise_case(oracle_lib):
    """The observation bar separates noise on from noise off: the oracle with `noise: "None"` against the oracle of the case,
    same seeds and action, misses the case's bar by a wide margin at the first step (sigma 2 deg on the 40-deg wd sensor range
    is 0.1 in observation units; the bar is 5e-4)."""
    seen = set()
    for cs in vc.CASES:
        if not dict(cs.kw).get("noise") or cs.ref_id in seen:
            continue
        seen.add(cs.ref_id)
        on, off = vc.reference(oracle_lib, cs, steps=1), vc.reference(oracle_lib, cs, steps=1, noise=False)
        np.testing.assert_array_equal(on["tr"][0], off["tr"][0])
        for q in ("obs", "multi"):
            d = np.abs(on[q][0] - off[q][0])
            assert d.max() > 40 * vc.obs_atol(cs), (cs.name, q, d.max())
            # and in most entries of the noised channels, not in one: at least a fifth of all entries miss the bar
            assert (d > vc.obs_atol(cs)).mean() > 0.2, (cs.name, q, (d > vc.obs_atol(cs)).mean())
    assert len(seen) >= 15
