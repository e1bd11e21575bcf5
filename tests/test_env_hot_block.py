"""k_flow_env's hot parameter block (EnvHotP, windgym_amd/csrc/wg_flow.h) is a copy: the words its common STEP path reads out of
FlowP / FlowPtrs and — for the glue's early request — WgParams / WgPtrs, laid side by side per phase so that a phase fetches them
in one scalar trip.  wg_plan_env_hot (wg_plan.h) builds it on the host from the very blocks a launch passes; this module pins it
without a device.  tests/env_hot_shim.cpp hands back every word of the block next to the member it copies (its table is the
second statement of which word copies what; every pointer member of the two pointer blocks carries an address of its own), and

  * every word equals its source, bit for bit (floats by pattern);
  * the named words and their zero padding tile the block exactly: no word is unnamed, none overlaps;
  * every group starts on a 16-byte boundary and is a multiple of 16 bytes long — the width a wide scalar load wants —, a pointer
    sits on 8 bytes, a four-channel row on 16;
  * the size is the one the kernel asserts (WG_ENV_HOT_BYTES).

Configurations: the cfg2 preset, the 3 x 3 multi-agent preset with extra_timestep_inc, F = 1 / N = 2, K = 3, the Power_diff reward
at Power_avg 40, sensor noise on all four channels."""
import ctypes as C

import pytest

import bench
from helpers import host_shim
from variant_census import AllChannelNoiseConfig, _yaml
from windgym_amd import presets
from windgym_amd.config import CConfig, EnvConfig
from windgym_amd.turbine import V80

CASES = ["cfg2", "multi_extra_inc", "two_turb_one_farm", "substeps3", "power_diff", "noise4"]


def _cfg(case):
    common = dict(turbine=V80(), turbtype="None", n_envs=64, autoreset=True, n_rotor_pts=16)
    cfg2 = presets.bench_cfg2_config()
    if case == "cfg2":
        return bench.make_cfg(4096, workload="cfg2")
    if case == "multi_extra_inc":
        return EnvConfig(yaml_dict=presets.multi_3x3_config(), n_passthrough=0.25, n_particles=96, extra_timestep_inc=True, **common)
    if case == "two_turb_one_farm":
        d = presets._upd(presets.env1_config(), ActionMethod="yaw", farm=dict(nx=2, ny=1), power_def=dict(Power_reward="Power_avg"))
        return EnvConfig(yaml_dict=d, n_passthrough=0.4, **common)
    if case == "substeps3":
        return EnvConfig(yaml_dict=_yaml(False, 3, 2), n_passthrough=0.3, dt_env=3, dt_sim=1, **common)
    if case == "power_diff":
        d = presets._upd(cfg2, power_def=dict(Power_reward="Power_diff", Power_avg=40))
        return EnvConfig(yaml_dict=d, n_passthrough=0.2, n_particles=128, **common)
    if case == "noise4":
        return AllChannelNoiseConfig(yaml_dict=_yaml(True, 3, 2, False, True), n_passthrough=0.25, **common)
    raise KeyError(case)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = host_shim(tmp_path_factory, "env_hot", include_header_dir=True)
    lib.env_hot_dump.argtypes = [C.POINTER(CConfig), C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_int]

    def dump(cfg):
        buf = C.create_string_buffer(1 << 16)
        cc = cfg.to_c()
        rc = lib.env_hot_dump(C.byref(cc), (C.c_int * 21)(), 65536, buf, 1 << 16)
        assert rc == 0, buf.value.decode()
        head, groups, words, raw = {}, {}, [], None
        for ln in buf.value.decode().splitlines():
            f = ln.split()
            if f[0] == "word":
                words.append(dict(group=f[1], name=f[2], off=int(f[3]), size=int(f[4]), got=int(f[5], 16), src=int(f[6], 16)))
            elif f[0] == "group":
                groups[f[1]] = (int(f[2]), int(f[3]))
            elif f[0] == "raw":
                raw = bytes.fromhex(f[1])
            else:
                head[f[0]] = int(f[1])
        return head, groups, words, raw

    return dump


@pytest.fixture(scope="module")
def blocks(shim):
    return {c: shim(_cfg(c)) for c in CASES}


@pytest.mark.parametrize("case", CASES)
def test_every_word_equals_the_member_it_copies(blocks, case):
    head, groups, words, raw = blocks[case]
    assert head["envw"] == 1, "the configuration runs k_flow_env"
    assert len(words) > 100
    for w in words:
        assert w["got"] == w["src"], f"{w['group']}.{w['name']}: {w['got']:#x} != {w['src']:#x}"
        # (what the shim printed is what the block's bytes hold at that offset)
        assert int.from_bytes(raw[w["off"]:w["off"] + w["size"]], "little") == w["got"], w


def test_the_cases_differ_where_they_should(blocks):
    """the configurations are not six copies of one: the words the issue's cases are about take the values of their case"""
    def val(case, group, name):
        return next(w["got"] for w in blocks[case][2] if w["group"] == group and w["name"] == name)
    assert blocks["cfg2"][0]["N"] == 16 and blocks["cfg2"][0]["F"] == 2 and val("cfg2", "pro", "N") == 16 and val("cfg2", "pro", "F") == 2
    assert val("two_turb_one_farm", "pro", "N") == 2 and val("two_turb_one_farm", "pro", "F") == 1 and val("two_turb_one_farm", "req", "N") == 2
    assert val("substeps3", "pro", "K") == 3 and val("cfg2", "pro", "K") == 1
    assert val("multi_extra_inc", "pro", "env_inc") == 2 and val("cfg2", "pro", "env_inc") == 1 and val("multi_extra_inc", "pro", "N") == 9
    assert val("power_diff", "req", "power_avg") == 40 and val("power_diff", "farm", "power_avg") == 40
    assert blocks["noise4"][0]["noise"] == 1 and all(val("noise4", "tail", f"noise_sigma[{i}]") != 0 for i in range(4))
    assert blocks["cfg2"][0]["noise"] == 0
    # the pointer words of one block are all different addresses (a word copied from a neighbour would have shown above)
    for grp, n in (("pro", 14), ("req", 5)):
        ptrs = [w["got"] for w in blocks["cfg2"][2] if w["group"] == grp and w["size"] == 8]
        assert len(ptrs) == n and len(set(ptrs)) == n


@pytest.mark.parametrize("case", ["cfg2", "noise4"])
def test_layout_groups_aligned_words_tile_the_block(blocks, case):
    head, groups, words, raw = blocks[case]
    assert head["size"] == head["asserted"] == len(raw) == sum(sz for _, sz in groups.values())
    end = 0
    for name in ("pro", "set", "req", "tail", "farm"):              # in this order, back to back
        off, sz = groups[name]
        assert off == end and off % 16 == 0 and sz % 16 == 0, (name, off, sz)
        end = off + sz
    covered = bytearray(len(raw))
    for w in words:
        off, sz = groups[w["group"]]
        assert off <= w["off"] and w["off"] + w["size"] <= off + sz, w      # inside its group
        assert w["off"] % w["size"] == 0, w                                  # naturally aligned (pointers on 8 bytes)
        if w["name"].endswith("[0]"):
            assert w["off"] % 16 == 0, w                                     # a four-channel row is one 16-byte load
        assert not any(covered[w["off"]:w["off"] + w["size"]]), f"{w['group']}.{w['name']} overlaps"
        covered[w["off"]:w["off"] + w["size"]] = b"\x01" * w["size"]
    pad = [i for i in range(len(raw)) if not covered[i]]
    assert all(raw[i] == 0 for i in pad), "padding is zero"
    assert len(pad) <= 4 * 16, f"{len(pad)} bytes of padding"               # at most three words per group + the request's one
