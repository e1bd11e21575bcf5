"""The packed weight layout of the MFMA tile core, decided on the CPU: the layout half of windgym_amd/csrc/wg_tile.h is plain C++,
so what k_policy_pack / k_lstm_pack write and what wg_policy_create_vf / wg_lstm_create allocate is pinned here without a device,
against a numpy restatement of the header's formula.  tests/tile_shim.cpp hands the header's functions over."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import host_shim
from windgym_amd.binding import CLstmDesc, CPolicyDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "windgym_amd", "csrc")
MLP_LAYERS = [(1, 1), (33, 7), (64, 257), (128, 32)]        # (M, K)
LSTM_SHAPES = [(3, 1), (7, 40), (257, 64)]                  # (n_in, H)
GROUP, SLACK = 8, 8 * 64                                    # the header's WGP_GROUP and its slack, restated


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """g++ alone, no ROCm include path: the layout half must stay free of HIP headers."""
    lib = host_shim(tmp_path_factory, "tile", include_header_dir=True)
    lib.tile_wsize.restype = lib.tile_bsize.restype = C.c_uint
    return lib


def ref_nks(K):
    """ceil(K / 2) k-steps, rounded up to PAIRS of groups"""
    return -(-(-(-K // 2)) // (2 * GROUP)) * 2 * GROUP


def ref_block(rows_of_tile, ntiles, K):
    """Wp[tile][ks][lane] = W[row(tile, lane & 31)][2 ks + (lane >> 5)] as source indices row * K + k, -1 = padding;
    rows_of_tile(tile) -> the 32 rows of W behind a tile (-1: none)."""
    nks = ref_nks(K)
    out = np.full((ntiles, nks, 64), -1, np.int64)
    lane = np.arange(64)
    for tile in range(ntiles):
        rows = rows_of_tile(tile)[lane & 31]
        for ks in range(nks):
            k = 2 * ks + (lane >> 5)
            out[tile, ks] = np.where((rows >= 0) & (k < K), rows * K + k, -1)
    return out.reshape(-1)


def check_block(got, ref, n_rows, K):
    assert got.shape == ref.shape and np.array_equal(got, ref)          # every element at the documented position, the rest padding
    src = got[got >= 0]
    assert np.array_equal(np.sort(src), np.arange(n_rows * K))         # every (row, k) exactly once


def test_constants_and_header_is_host_only(shim, tmp_path):
    c = (C.c_int * 5)()
    shim.tile_consts(c)
    assert list(c) == [32, 256, 4, GROUP, SLACK]
    src = tmp_path / "t.cpp"
    src.write_text('#include "wg_tile.h"\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, str(src)], check=True)


@pytest.mark.parametrize("K", [1, 7, 32, 33, 64 + 7, 257, 2048, 2048 + 256])
def test_nks(shim, K):
    nks = shim.tile_nks(K)
    assert nks == ref_nks(K) and nks % (2 * GROUP) == 0 and nks >= -(-K // 2) and nks - 2 * GROUP < -(-K // 2)
    for kc in (K % 256 or 256,):                                        # a staged chunk's padding: whole pairs of groups of k-steps
        assert shim.tile_kpad(kc) == 2 * ref_nks(kc)


@pytest.mark.parametrize("M, K", MLP_LAYERS)
def test_mlp_layer(shim, M, K):
    ntiles, nks = -(-M // 32), ref_nks(K)
    assert (shim.tile_count(M), shim.tile_wsize(ntiles, nks), shim.tile_bsize(ntiles)) == (ntiles, ntiles * nks * 64, ntiles * 32)
    got = np.zeros(ntiles * nks * 64, np.int32)
    shim.decode_mlp(M, K, got.ctypes.data_as(C.c_void_p))
    check_block(got, ref_block(lambda t: np.where(32 * t + np.arange(32) < M, 32 * t + np.arange(32), -1), ntiles, K), M, K)
    # a policy that is this one layer (actor head, no critic, no log_std): its weight block, its bias block, the slack
    d = CPolicyDesc(K, M, 0, 0, (C.c_int32 * 4)(), -1, (C.c_int32 * 4)(), 0)
    out = (C.c_uint * 4)()
    shim.policy_layout(C.byref(d), K, out)
    assert list(out) == [M * K + M, ntiles * nks * 64 + ntiles * 32 + SLACK, 0, ntiles * nks * 64]


def test_policy_layout_walk(shim):
    """two nets, hidden layers, a split critic, log_std: blocks back to back in the flat order's sequence"""
    d = CPolicyDesc(257, 3, 0, 1, (C.c_int32 * 4)(64), 2, (C.c_int32 * 4)(33, 7), 1)
    out = (C.c_uint * 12)()
    shim.policy_layout(C.byref(d), 40, out)
    layers = [(64, 257), (3, 64), (33, 40), (7, 33), (1, 7)]
    flat = packed = 0
    for i, (M, K) in enumerate(layers):
        nt = -(-M // 32)
        assert out[2 + 2 * i] == packed and out[3 + 2 * i] == packed + nt * ref_nks(K) * 64
        flat, packed = flat + M * K + M, packed + nt * ref_nks(K) * 64 + nt * 32
    assert (out[0], out[1]) == (flat + 3, packed + 3 + SLACK)


@pytest.mark.parametrize("n_in, H", LSTM_SHAPES)
def test_lstm_net(shim, n_in, H):
    K, nub = n_in + H, -(-H // 32)
    nks = ref_nks(K)
    j = np.arange(32)
    for tile in range(4 * nub):                                         # tile 4u + q -> row q H + 32 u + j
        u, q = tile // 4, tile % 4
        assert [shim.lstm_tile_row(tile, int(i), H) for i in j] == list(np.where(32 * u + j < H, q * H + 32 * u + j, -1))
    got = np.zeros(4 * nub * nks * 64, np.int32)
    shim.decode_lstm(n_in, H, got.ctypes.data_as(C.c_void_p))
    rows = lambda t: np.where(32 * (t // 4) + j < H, (t % 4) * H + 32 * (t // 4) + j, -1)      # noqa: E731
    check_block(got, ref_block(rows, 4 * nub, K), 4 * H, K)
    for nets in (1, 2):
        d = CLstmDesc(n_in, H, nets)
        out = (C.c_uint * 6)()
        shim.lstm_layout(C.byref(d), out)
        per = 4 * nub * nks * 64 + 4 * nub * 32
        assert (out[0], out[1]) == (nets * (4 * H * K + 8 * H), nets * per + SLACK)
        assert [out[2 + i] for i in range(2 * nets)] == [v for n in range(nets) for v in (n * per, n * per + 4 * nub * nks * 64)]
