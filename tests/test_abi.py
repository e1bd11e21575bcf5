"""CPU-side checks of the drop-in boundary: the built library loads and exports every symbol that
include/windgym_hip.h declares; the ctypes mirror of wg_config matches the C layout."""
import ctypes as C
import os
import re

import pytest

from helpers import c_layout
from windgym_amd import binding, build
from windgym_amd.config import CConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    return build.build()


def test_header_symbols_are_exported(lib_path):
    hdr = open(os.path.join(ROOT, "include", "windgym_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(wg_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(binding.ABI_SYMBOLS), declared ^ set(binding.ABI_SYMBOLS)
    L = C.CDLL(lib_path)
    for name in declared:
        assert hasattr(L, name), f"{name} not exported"
    L.wg_abi_version.restype = C.c_int
    assert L.wg_abi_version() == 4


def test_every_bound_symbol_is_defined_by_a_listed_source():
    """Builds nothing: every name the binding needs is defined at file scope in a translation unit of build.SOURCES (a
    source missing from that list links a library that load_library() cannot load)."""
    text = "".join(open(os.path.join(build.CSRC, s)).read() for s in build.SOURCES)
    bound = set(re.findall(r"\bL\.(wg_\w+)\.argtypes", open(binding.__file__).read())) | set(binding.ABI_SYMBOLS)
    assert not [n for n in sorted(bound) if not re.search(r"^[A-Za-z][\w\"* ]*\b%s\(" % n, text, re.M)]


def test_config_struct_layout_matches_c(tmp_path):
    """sizeof/offsetof of wg_config as gcc sees it == the ctypes mirror."""
    fields = [f[0] for f in CConfig._fields_]
    out = c_layout("wg_config", fields, tmp_path)
    assert out["sizeof"] == C.sizeof(CConfig)
    for f in fields:
        assert out[f] == getattr(CConfig, f).offset, f


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from windgym_amd.config import EnvConfig
    from windgym_amd.turbine import V80
    from helpers import load_golden
    _, meta = load_golden("env1")
    cfg = EnvConfig(turbine=V80(), yaml_dict=meta["cfg"], turbtype="None")
    with pytest.raises(binding.WindGymHipError):
        binding.HipBatch(cfg)
