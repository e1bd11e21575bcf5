"""Row f2: the Mann box generator of libwindgym_hip.so (wg_generate_mann_box: HIP spectral-tensor kernel + hipFFT) pinned
cell by cell against the numpy restatement fed with the IDENTICAL complex white noise, and the host-side eddy-lifetime
table against scipy's 2F1.  (hipersim itself — MannTurbulenceField.generate, Wind_Farm_Env.py:624-637 — is not
installable here: both sides restate the published algorithm, Mann 1998.)"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from windgym_amd import mann  # noqa: E402


def test_beta_table_matches_scipy_hyp2f1():
    """wg_mann_beta_table (Euler integral of 2F1(1/3, 17/6; 4/3; -x) by Gauss-Legendre panels, host code of the library)
    against scipy.special.hyp2f1 over the whole table range."""
    for gamma in (3.9, 2.0):
        tab = mann.mann_beta_table(gamma)
        kl = np.logspace(mann.BETA_TABLE["log10_lo"], mann.BETA_TABLE["log10_hi"], mann.BETA_TABLE["n"])
        ref = mann._eddy_lifetime_beta(kl, gamma)
        np.testing.assert_allclose(tab, ref, rtol=1e-12)
    assert np.all(mann.mann_beta_table(0.0) == 0.0)
    # asymptotes (Mann 1998): beta -> Gamma (kL)^(-2/3) for kL >> 1, ~ 1 / kL for kL << 1
    tab = mann.mann_beta_table(3.9)
    assert abs(tab[-1] / (3.9 * 1e6 ** (-2.0 / 3.0)) - 1.0) < 1e-6
    assert abs(tab[0] * 1e-6 / (tab[1] * 10 ** (-6 + 12 / 4095)) - 1.0) < 1e-6


def test_table_interpolation_is_a_faithful_beta():
    """the numpy restatement with the kernel's table interpolation == with 2F1 evaluated per cell (5e-4 of the field's
    standard deviation: the interpolation error of a 4096-point log table)"""
    rng = np.random.default_rng(0)
    shape = (3, 64, 32, 16)
    n = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    a = mann.mann_field_from_noise(n, (3.0, 3.0, 3.0))
    b = mann.mann_field_from_noise(n, (3.0, 3.0, 3.0), beta_table=mann.mann_beta_table(3.9))
    assert np.abs(a - b).max() < 5e-4
    assert abs(a[0].std() - 1.0) < 1e-12


def test_philox_noise_stream_of_the_generator():
    """wgo_mann_noise (the oracle-side restatement of the kernel's Philox stream): unit complex variance, independent
    parts, reproducible, different per seed"""
    from oracle import oracle as om
    n = om.mann_noise(7, (32, 16, 8))
    assert n.shape == (3, 32, 16, 8)
    assert abs(np.mean(np.abs(n) ** 2) - 1.0) < 0.03
    assert abs(n.real.var() - 0.5) < 0.02 and abs(n.imag.var() - 0.5) < 0.02
    assert abs(np.mean(n.real * n.imag)) < 0.02
    assert np.array_equal(n, om.mann_noise(7, (32, 16, 8)))
    assert not np.array_equal(n, om.mann_noise(8, (32, 16, 8)))


@pytest.mark.gpu
@pytest.mark.parametrize("dims,spacing,gamma,L", [
    ((256, 64, 32), (3.0, 3.0, 3.0), 3.9, 33.6),      # the sheared tensor of the ambient field
    ((256, 64, 32), (3.0, 3.0, 3.0), 0.0, 5.0),       # isotropic: the wake-added turbulence box (ADDED_BOX_SPEC)
    ((128, 48, 20), (4.0, 5.0, 6.0), 3.9, 33.6),      # non-cubic spacing, non-power-of-two dims
])
def test_hip_generator_equals_numpy_on_identical_noise(dims, spacing, gamma, L):
    """Same complex white noise into wg_generate_mann_box and into the float64 numpy restatement (with the kernel's beta
    table): every cell of the unit-variance box agrees to fp32 rounding."""
    rng = np.random.default_rng(11)
    shape = (3,) + dims
    n = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)).astype(np.complex64)
    ref = mann.mann_field_from_noise(n.astype(np.complex128), spacing, 0.1, L, gamma, beta_table=mann.mann_beta_table(gamma))
    got = mann.generate_mann_box_hip(dims, spacing, 0.1, L, gamma, seed=0, noise=n).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == shape
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)
    assert abs(float(got[0].std()) - 1.0) < 1e-5


@pytest.mark.gpu
def test_hip_generator_builtin_noise_is_the_pinned_philox_stream():
    """Without a noise argument the kernel draws from Philox keyed by the seed: the numpy restatement fed with the
    oracle-side restatement of that stream reproduces the box (the float Box-Muller of the two sides may differ in the
    last bits of a few samples: 1e-3 of the field's standard deviation)."""
    from oracle import oracle as om
    dims, spacing = (128, 32, 16), (3.0, 3.0, 3.0)
    got = mann.generate_mann_box_hip(dims, spacing, seed=1234).cpu().numpy()
    ref = mann.mann_field_from_noise(om.mann_noise(1234, dims).astype(np.complex128), spacing,
                                     beta_table=mann.mann_beta_table(3.9))
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-3)
    other = mann.generate_mann_box_hip(dims, spacing, seed=1235).cpu().numpy()
    assert np.abs(other - got).max() > 0.5            # another seed, another realisation


@pytest.mark.gpu
def test_hip_generator_reference_box_size_and_statistics():
    """the reference's MannFixed box (2048 x 512 x 64 @ 3 m, Wind_Farm_Env.py:649-658) generated on the device: unit
    variance of u, anisotropy of the sheared tensor (sigma_u > sigma_v > sigma_w), zero mean, a decaying correlation"""
    import torch
    spec = mann.reference_box_spec("MannFixed", 80.0)
    box = mann.generate_mann_box_hip(**spec)
    assert tuple(box.shape) == (3, 2048, 512, 64)
    sd = box.reshape(3, -1).std(dim=1).cpu().numpy()
    assert abs(sd[0] - 1.0) < 1e-4 and sd[0] > sd[1] > sd[2] > 0.4
    assert float(box.reshape(3, -1).mean(dim=1).abs().max()) < 1e-3
    u = box[0]
    c1 = float((u[:-8] * u[8:]).mean())        # 24 m along x
    c2 = float((u[:-64] * u[64:]).mean())      # 192 m
    assert 0.4 < c1 < 1.0 and c2 < c1
    assert torch.isfinite(box).all()


# ---- by value at the sizes that ship and at awkward dimensions ------------------------------------------------------------
# The reference is mann_field_from_noise (complex128, the kernel's beta table) fed the identical noise; at 2^26 cells and up
# its component-at-a-time form mann_field_components (bit-equal on small boxes: asserted below on the CPU).  Errors are
# reported (-s) as the worst absolute error of the unit-variance box and as `u`, the worst error in units of the bar this
# file has always used, |got - ref| <= 1e-4 + 1e-4 |ref|.
def _noise(dims, seed):
    """complex white noise [3, Nx, Ny, Nz] (E|n|^2 = 1) as complex64, drawn one component at a time"""
    rng = np.random.default_rng(seed)
    n = np.empty((3,) + tuple(dims), dtype=np.complex64)
    for c in range(3):
        v = n[c].view(np.float32)
        v[...] = rng.standard_normal(v.shape, dtype=np.float32)
        v *= np.float32(np.sqrt(0.5))
    return n


def _u(got, ref, rtol=1e-4, atol=1e-4):
    d = np.abs(got - ref)
    return float(d.max()), float((d / (atol + rtol * np.abs(ref))).max())


def _hip_box(dims, spacing, ae, L, gamma, noise):
    """the generator's box for this noise (handed over as the float tensor [3, Nx, Ny, Nz, 2] that shares the array's memory)"""
    import torch
    t = torch.from_numpy(noise.view(np.float32).reshape(noise.shape + (2,)))
    got = mann.generate_mann_box_hip(dims, spacing, ae, L, gamma, seed=0, noise=t).cpu().numpy()
    torch.cuda.empty_cache()
    return got


@pytest.mark.parametrize("dims,slab", [((64, 32, 16), 16), ((33, 17, 5), 7), ((16, 8, 4), 64)])
def test_component_at_a_time_reference_is_the_whole_box_reference(dims, slab):
    """mann_field_components (slabs of x-planes, one component at a time: what the 2^26-cell tests use) is BIT-EQUAL to
    mann_field_from_noise with numpy's FFT, and equal to 1e-12 with scipy's threaded one"""
    n = _noise(dims, 2)
    tab = mann.mann_beta_table(3.9)
    whole = mann.mann_field_from_noise(n, (3.0, 4.0, 5.0), beta_table=tab)
    parts = list(mann.mann_field_components(n, (3.0, 4.0, 5.0), beta_table=tab, slab=slab))
    assert len(parts) == 3 and all(np.array_equal(p, w) for p, w in zip(parts, whole))
    threaded = list(mann.mann_field_components(n, (3.0, 4.0, 5.0), beta_table=tab, slab=slab, workers=4))
    assert max(np.abs(p - w).max() for p, w in zip(threaded, whole)) < 1e-12
    # the complex64 noise is promoted per cell: the same box as from its complex128 copy
    assert np.array_equal(whole, mann.mann_field_from_noise(n.astype(np.complex128), (3.0, 4.0, 5.0), beta_table=tab))


AWKWARD = {
    "all_odd": ((127, 33, 17), (3.0, 3.0, 3.0), 0.1, 33.6, 3.9),            # no Nyquist plane: fftfreq_k's (n + 1) / 2 branch
    "primes": ((67, 31, 13), (3.0, 3.0, 3.0), 0.1, 33.6, 3.9),              # hipFFT's non-radix path
    "minimum": ((2, 2, 2), (3.0, 3.0, 3.0), 0.1, 33.6, 3.9),
    "pencil": ((256, 2, 2), (3.0, 3.0, 3.0), 0.1, 33.6, 3.9),
    "three_deep": ((64, 64, 3), (3.0, 3.0, 3.0), 0.1, 33.6, 3.9),
    "anisotropic_spacing": ((96, 40, 24), (1.0, 8.0, 0.5), 0.1, 33.6, 3.9),
    "gamma_0": ((128, 48, 20), (4.0, 5.0, 6.0), 0.1, 33.6, 0.0),
    "gamma_5": ((128, 48, 20), (4.0, 5.0, 6.0), 0.1, 33.6, 5.0),
    "L_5": ((128, 48, 20), (4.0, 5.0, 6.0), 0.1, 5.0, 3.9),
    "L_200": ((128, 48, 20), (4.0, 5.0, 6.0), 0.1, 200.0, 3.9),
    "alphaepsilon_1e-3": ((128, 48, 20), (4.0, 5.0, 6.0), 1e-3, 33.6, 3.9),
    "alphaepsilon_10": ((128, 48, 20), (4.0, 5.0, 6.0), 10.0, 33.6, 3.9),
}
# worst u on the MI355X (gfx950, ROCm 7.0, hipFFT); each bar is 5 x that and never looser than u = 1 (today's bar).
# The error does grow with the size of the transform, but slowly: 1.0e-6 .. 3.0e-6 of the unit-variance field at 2^13 .. 2^17
# cells, 3.1e-6 at 2^26 (2048 x 512 x 64) and 5.9e-6 at 2^27 (4096 x 512 x 64): u = 0.027 and 0.056 — the bar chosen at 2^19
# cells holds with a factor of 17 to spare at the largest box that ships, so no bar moved.
# "pencil" (256 x 2 x 2) is the one shape near the bar (5.2e-5, u = 0.49, its bar stays u = 1): the box has 1024 modes only,
# so the fp32 rounding of a single mode's tensor is not averaged over many modes as it is in every other shape.
MEASURED_U = {
    "all_odd": 0.0131,                             # worst abs 1.6e-06
    "primes": 0.0103,                              # worst abs 1.1e-06
    "minimum": 0.0017,                             # worst abs 2.9e-07
    "pencil": 0.4921,                              # worst abs 5.2e-05
    "three_deep": 0.0100,                          # worst abs 1.2e-06
    "anisotropic_spacing": 0.0056,                 # worst abs 9.5e-07
    "gamma_0": 0.0072,                             # worst abs 1.0e-06
    "gamma_5": 0.0167,                             # worst abs 1.8e-06
    "L_5": 0.0210,                                 # worst abs 3.0e-06
    "L_200": 0.0111,                               # worst abs 1.9e-06
    "alphaepsilon_1e-3": 0.0138,                   # worst abs 1.7e-06
    "alphaepsilon_10": 0.0143,                     # worst abs 2.0e-06
    "mann_fixed_2048x512x64": 0.0273,              # worst abs 3.1e-06
    "added_128x128x128": 0.0088,                   # worst abs 1.3e-06
    "mann_generate_4096x512x64": 0.0561,           # worst abs 5.9e-06
    "builtin_noise_2048x512x64": 0.0025,           # worst abs 2.8e-06
}


def _bar(name):
    return min(1.0, 5.0 * MEASURED_U[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(AWKWARD))
def test_hip_generator_by_value_at_awkward_dimensions(name):
    dims, spacing, ae, L, gamma = AWKWARD[name]
    n = _noise(dims, 12)
    ref = mann.mann_field_from_noise(n, spacing, ae, L, gamma, beta_table=mann.mann_beta_table(gamma))
    got = _hip_box(dims, spacing, ae, L, gamma, n)
    assert got.shape == (3,) + dims and np.isfinite(got).all()
    a, u = _u(got, ref)
    print(f"[mann {name} {dims}] worst abs {a:.3e}, u {u:.4f}")
    assert u <= _bar(name), (u, _bar(name))
    assert abs(float(got[0].std()) - 1.0) < 1e-5


@pytest.mark.gpu
def test_hip_generator_box_does_not_depend_on_alphaepsilon():
    """the box is normalised to unit std of u: alphaepsilon 1e-3 and 10 give the same box to rounding"""
    dims, spacing, _, L, gamma = AWKWARD["alphaepsilon_10"]
    n = _noise(dims, 12)
    lo, hi = _hip_box(dims, spacing, 1e-3, L, gamma, n), _hip_box(dims, spacing, 10.0, L, gamma, n)
    a, u = _u(lo, hi, rtol=5e-6, atol=5e-6)
    print(f"[mann alphaepsilon 1e-3 vs 10] worst abs {a:.3e}")
    assert u <= 1.0           # measured 1.2e-6: the amplitude's rounding (sqrt, one product) before the transform


SHIPPED = {
    # reference_box_spec("MannFixed"): 2^26 cells
    "mann_fixed_2048x512x64": ((2048, 512, 64), (3.0, 3.0, 3.0), 0.1, 33.6, 3.9),
    # ADDED_BOX_SPEC (the wake-added turbulence box)
    "added_128x128x128": (mann.ADDED_BOX_SPEC["Nxyz"], mann.ADDED_BOX_SPEC["dxyz"], mann.ADDED_BOX_SPEC["alphaepsilon"],
                          mann.ADDED_BOX_SPEC["L"], mann.ADDED_BOX_SPEC["Gamma"]),
    # reference_box_spec("MannGenerate", D = 80): 2^27 cells
    "mann_generate_4096x512x64": ((4096, 512, 64), (4.0, 8.0, 8.0), 0.1, 33.6, 3.9),
}
WORKERS = 16                  # threads of the host-side reference (slabs of the spectral tensor, scipy's FFT)


def _peak_gb():
    import resource
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20


def _by_value_at_size(name, got, n, spacing, ae, L, gamma, rtol=1e-4, atol=1e-4):
    """every cell of ``got`` against the component-at-a-time reference; -> (worst abs, worst u); asserts that no half of the
    box repeats the other and that the error does not grow towards high x"""
    _, Nx, Ny, _ = got.shape
    worst_a = worst_u = 0.0
    for c, ref in enumerate(mann.mann_field_components(n, spacing, ae, L, gamma, beta_table=mann.mann_beta_table(gamma),
                                                       workers=WORKERS)):
        d = np.abs(got[c] - ref)
        a, u = float(d.max()), float((d / (atol + rtol * np.abs(ref))).max())
        first, last = float(d[:Nx // 8].max()), float(d[-(Nx // 8):].max())
        print(f"[mann {name} component {c}] worst abs {a:.3e}, u {u:.4f}; first / last eighth of x {first:.3e} / {last:.3e}")
        assert last <= 2.0 * first and first <= 2.0 * last, (c, first, last)
        # a region written twice or a wrapped cell index repeats planes: no x-plane i equals plane i + Nx / 2, no y-row j row j + Ny / 2
        assert float(np.abs(got[c][:Nx // 2] - got[c][Nx // 2:2 * (Nx // 2)]).max(axis=(1, 2)).min()) > 0.5
        assert float(np.abs(got[c][:, :Ny // 2] - got[c][:, Ny // 2:2 * (Ny // 2)]).max(axis=(0, 2)).min()) > 0.5
        worst_a, worst_u = max(worst_a, a), max(worst_u, u)
        del ref, d
    return worst_a, worst_u


@pytest.fixture(scope="module")
def mann_fixed():
    """the 2048 x 512 x 64 box for one noise array, shared by the by-value test and its negative controls"""
    dims, spacing, ae, L, gamma = SHIPPED["mann_fixed_2048x512x64"]
    n = _noise(dims, 13)
    return n, _hip_box(dims, spacing, ae, L, gamma, n)


@pytest.mark.gpu
def test_hip_generator_by_value_at_2048x512x64(mann_fixed):
    """Every one of the 3 x 2^26 cells of the MannFixed box against the float64 reference fed the identical noise.
    Measured on the MI355X machine's host with 16 workers: reference 4.2 s, peak host memory
    of the test process 9.2 GB (noise 1.5 GB, the box's copy 0.8 GB, three complex128 dZ arrays 3 GB, one transform)."""
    import time
    name = "mann_fixed_2048x512x64"
    dims, spacing, ae, L, gamma = SHIPPED[name]
    n, got = mann_fixed
    t0 = time.perf_counter()
    a, u = _by_value_at_size(name, got, n, spacing, ae, L, gamma)
    print(f"[mann {name}] worst abs {a:.3e}, u {u:.4f}; reference {time.perf_counter() - t0:.1f} s, peak host memory {_peak_gb():.1f} GB")
    assert u <= _bar(name), (u, _bar(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["added_128x128x128", "mann_generate_4096x512x64"])
def test_hip_generator_by_value_at_the_other_shipped_sizes(name):
    """The 128^3 wake-added box and the 2^27-cell MannGenerate box: every cell, the reference one full-size float64 FFT per
    component (the whole-box form, not the subset of z-columns).  Measured for 4096 x 512 x 64 with 16 workers: noise + box
    6.6 s, reference 7.0 s, peak host memory of the test process 18.7 GB."""
    import time
    dims, spacing, ae, L, gamma = SHIPPED[name]
    t0 = time.perf_counter()
    n = _noise(dims, 14)
    got = _hip_box(dims, spacing, ae, L, gamma, n)
    t1 = time.perf_counter()
    a, u = _by_value_at_size(name, got, n, spacing, ae, L, gamma)
    print(f"[mann {name}] worst abs {a:.3e}, u {u:.4f}; noise + box {t1 - t0:.1f} s, reference {time.perf_counter() - t1:.1f} s, "
          f"peak host memory {_peak_gb():.1f} GB")
    assert u <= _bar(name), (u, _bar(name))
    assert abs(float(got[0].std()) - 1.0) < 1e-4


@pytest.mark.gpu
def test_hip_generator_builtin_noise_at_2048x512x64():
    """the built-in Philox stream at cell indices up to 2^26 (beyond 2^24, where an index kept in a float would lose bits):
    the box for seed 1234 against the reference fed the oracle-side restatement of the stream; the bars of
    test_hip_generator_builtin_noise_is_the_pinned_philox_stream"""
    import torch
    from oracle import oracle as om
    name = "builtin_noise_2048x512x64"
    dims, spacing, ae, L, gamma = SHIPPED["mann_fixed_2048x512x64"]
    got = mann.generate_mann_box_hip(dims, spacing, seed=1234).cpu().numpy()
    torch.cuda.empty_cache()
    n = om.mann_noise(1234, dims)
    # the stream itself beyond 2^24: the last cell's sample is not the sample of the cell 2^24 or 2^25 before it
    flat = n.reshape(3, -1)
    assert flat[0, -1] != flat[0, -1 - 2 ** 24] and flat[0, -1] != flat[0, -1 - 2 ** 25] and flat[0, 2 ** 24 + 1] != flat[0, 2 ** 24]
    a, u = _by_value_at_size(name, got, n, spacing, ae, L, gamma, rtol=1e-3, atol=1e-3)
    print(f"[mann {name}] worst abs {a:.3e}, u (of 1e-3 + 1e-3 |ref|) {u:.4f}")
    assert u <= _bar(name), (u, _bar(name))


@pytest.mark.gpu
def test_hip_generator_properties_at_2048x512x64(mann_fixed):
    """no reference needed: the same seed twice is bit-equal; the caller's noise tensor is untouched; a call on a non-default
    torch stream, read on that stream, gives the same box"""
    import torch
    dims, spacing, ae, L, gamma = SHIPPED["mann_fixed_2048x512x64"]
    a = mann.generate_mann_box_hip(dims, spacing, seed=77)
    b = mann.generate_mann_box_hip(dims, spacing, seed=77)
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = mann.generate_mann_box_hip(dims, spacing, seed=77)
        same = bool(torch.equal(a, c))          # read on s
    assert same
    del a, b, c
    torch.cuda.empty_cache()
    n, got = mann_fixed
    t = torch.from_numpy(n.view(np.float32).reshape(n.shape + (2,))).cuda()
    keep = t.clone()
    again = mann.generate_mann_box_hip(dims, spacing, ae, L, gamma, seed=0, noise=t)
    assert torch.equal(t, keep)
    assert np.array_equal(again.cpu().numpy(), got)          # and the given noise, twice: bit-equal
    del t, keep, again
    torch.cuda.empty_cache()


def _u_of_component_0(got, n, spacing, ae, L, gamma, workers=None):
    gen = mann.mann_field_components(n, spacing, ae, L, gamma, beta_table=mann.mann_beta_table(gamma), workers=workers)
    ref = next(gen)
    gen.close()
    return _u(got[0], ref)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["256x64x32", "2048x512x64"])
def test_a_wrong_reference_breaks_the_bar_by_a_wide_margin(size, request):
    """negative controls: the box stays as it is, the REFERENCE is fed the noise rolled by one cell along x, along z, or
    Gamma 3.8 for 3.9 — each is hundreds of bars away (u component; u = 1 is today's bar)"""
    dims, spacing, ae, L, gamma = SHIPPED["mann_fixed_2048x512x64"]
    if size == "256x64x32":
        dims, workers = (256, 64, 32), None
        n = _noise(dims, 13)
        got = _hip_box(dims, spacing, ae, L, gamma, n)
    else:
        workers = WORKERS
        n, got = request.getfixturevalue("mann_fixed")
    right = _u_of_component_0(got, n, spacing, ae, L, gamma, workers)
    assert right <= 1.0
    wrong = {"noise rolled by one cell along x": (np.roll(n, 1, axis=1), gamma), "noise rolled by one cell along z": (np.roll(n, 1, axis=3), gamma),
             "Gamma 3.8 for 3.9": (n, 3.8)}
    for what, (nn, g) in wrong.items():
        u = _u_of_component_0(got, nn, spacing, ae, L, g, workers)
        print(f"[mann control {size}] {what}: u {u:.1f} (right reference: {right:.4f})")
        assert u > 100.0, (what, u)
        del nn
