"""The float64 box-lookup reference of the GPU box tests (tests/box_reference.py), pinned on the CPU: against the C oracle's
flow-field view on the small box shapes of the parity tests, at the coordinates where lookups go wrong, against closed forms, and
with a negative control — a box rolled by one cell must fail the comparison at the bar in use, on white noise by a wide margin."""
import numpy as np
import pytest

import box_reference as br

# both are float64; they differ in the order of the operations only (nested interpolation against a plain weighted sum): worst
# difference observed 1.8e-15 m/s on a clipped white-noise box at TI U <= 2.25 m/s
ORACLE_ATOL = 1e-13
SMALL_SHAPES = [((256, 64, 32), (3.0, 3.0, 3.0)),       # powers of two, multiples of 4
                ((240, 72, 40), (3.0, 3.0, 3.0)),       # multiples of 4, no powers of two
                ((90, 30, 18), (4.0, 5.0, 6.0))]        # neither, anisotropic spacing


def _cfg(turbtype="MannFixed", n_envs=2):
    from windgym_amd.config import EnvConfig
    from windgym_amd.presets import env1_config
    from windgym_amd.turbine import V80
    d = env1_config()
    d["ActionMethod"] = "yaw"
    d["farm"].update(nx=2, ny=1)
    return EnvConfig(turbine=V80(), yaml_dict=d, turbtype=turbtype, n_envs=n_envs, autoreset=True, n_passthrough=1.0, n_rotor_pts=4)


def _oracle_with(oracle_lib, box, spacing, seeds=(11, 12)):
    orc = oracle_lib.Oracle(_cfg(n_envs=len(seeds)))
    orc.set_turbulence_box(box, spacing)
    orc.reset(seeds=np.asarray(seeds))
    return orc


def _grid_errors(orc, env, ref_box, spacing, classes):
    """worst |oracle view - reference| per coordinate class; the view's grid is x[n] x y[n] at one z, so every class is
    evaluated on the full product of its x and y values at three of its heights"""
    ws, ti, t = (float(orc.info(k)[env]) for k in ("ws_global", "ti_global", "fs_time"))
    worst = {}
    for name, (x, y, z) in classes.items():
        e = 0.0
        for zz in z[:3]:
            got = orc.windspeed(env, x + ws * t, y, z=float(zz), include_wakes=False)
            ref = br.ambient_wind(ref_box, spacing, ws, ti, t, (x + ws * t)[:, None], y[None, :], float(zz))
            e = max(e, float(np.abs(got - ref).max()))
        worst[name] = e
    return worst


@pytest.mark.parametrize("shape,spacing", SMALL_SHAPES)
def test_reference_equals_the_oracle_flow_view_on_white_noise(oracle_lib, shape, spacing):
    """MannFixed reads the box un-shifted: the oracle's get_windspeed(include_wakes=False) is U + TI U g(x - U t, y, z).  Nodes, the
    last cell of each axis, negative coordinates, more than ten box lengths away; after the reset and after 150 more steps."""
    box = br.white_noise_box(shape, seed=5)
    orc = _oracle_with(oracle_lib, box, spacing)
    classes = br.coordinate_classes(shape, spacing, np.random.default_rng(1), n=24)
    rng = np.random.default_rng(2)
    for phase in range(2):
        for env in (0, 1):
            worst = _grid_errors(orc, env, box, spacing, classes)
            assert max(worst.values()) <= ORACLE_ATOL, (phase, env, worst)
        for _ in range(150):
            orc.step(rng.uniform(-1, 1, size=(2, 2)))
    assert float(orc.info("fs_time")[0]) >= 150.0              # (an episode of these envs is longer than that: no rollover)
    orc.close()


def test_reference_equals_the_oracle_flow_view_on_a_mann_box(oracle_lib):
    """the same on the smooth box of the parity tests (the field every earlier value-level test used)"""
    from windgym_amd.mann import generate_mann_box
    shape, spacing = (256, 64, 32), (3.0, 3.0, 3.0)
    box = generate_mann_box(shape, spacing, seed=1234)
    orc = _oracle_with(oracle_lib, box, spacing)
    worst = _grid_errors(orc, 0, box, spacing, br.coordinate_classes(shape, spacing, np.random.default_rng(1), n=24))
    assert max(worst.values()) <= ORACLE_ATOL, worst
    orc.close()


@pytest.mark.parametrize("shape,spacing", SMALL_SHAPES)
def test_reference_on_nodes_and_on_a_linear_field(shape, spacing):
    """closed forms: on a node the lookup returns the node's value, whole box lengths away too; a field linear in the node index
    is reproduced exactly inside the box and jumps back across the periodic seam"""
    rng = np.random.default_rng(3)
    box = br.white_noise_box(shape, seed=6)
    i, j, k = (rng.integers(0, n, 200) for n in shape)
    for shift in (0, 1, -1, 12):
        got = br.trilinear_periodic(box, spacing, (i + shift * shape[0]) * spacing[0], (j - shift * shape[1]) * spacing[1], k * spacing[2])
        np.testing.assert_array_equal(got, box[:, i, j, k].astype(np.float64))
    ii, jj, kk = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    lin = (2.0 * ii - 3.0 * jj + 0.5 * kk)[None]
    f = [rng.uniform(0.0, n - 1.0, 300) for n in shape]               # fractional node indices off the seam
    got = br.trilinear_periodic(lin, spacing, f[0] * spacing[0], f[1] * spacing[1], f[2] * spacing[2])[0]
    np.testing.assert_allclose(got, 2.0 * f[0] - 3.0 * f[1] + 0.5 * f[2], rtol=0, atol=1e-9)
    # in the last cell of x the upper neighbour is node 0: the value falls from 2 (nx - 1) towards 0
    got = br.trilinear_periodic(lin, spacing, (shape[0] - 0.25) * spacing[0], 0.0, 0.0)[0]
    assert got == pytest.approx(0.25 * 2.0 * (shape[0] - 1))


def test_block_average_is_centred_at_fine_index_4i_plus_1p5():
    """the meandering field: coarse cell I holds the mean of fine cells 4 I .. 4 I + 3 of every axis and sits at fine index
    4 I + 1.5 — a field linear in the fine index is therefore reproduced by the coarse lookup away from the seam, and a coarse
    node returns the plain mean of its 64 cells"""
    shape, spacing = (48, 24, 20), (3.0, 2.0, 5.0)
    rng = np.random.default_rng(4)
    box = br.white_noise_box(shape, seed=7)
    c = br.block_average(box)
    assert c.shape == (3, 12, 6, 5)
    assert c[1, 3, 2, 4] == pytest.approx(box[1, 12:16, 8:12, 16:20].astype(np.float64).mean(), abs=1e-12)
    I, J, K = 3, 2, 4
    got = br.coarse_trilinear_periodic(c, spacing, (4 * I + 1.5) * spacing[0], (4 * J + 1.5) * spacing[1], (4 * K + 1.5) * spacing[2])
    np.testing.assert_allclose(got, c[:, I, J, K], rtol=0, atol=1e-12)
    ii, jj, kk = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    lin = (ii - 2.0 * jj + 3.0 * kk)[None]
    f = [rng.uniform(1.5, n - 2.5, 200) for n in shape]               # between the first and the last coarse node
    got = br.coarse_trilinear_periodic(br.block_average(lin), spacing, f[0] * spacing[0], f[1] * spacing[1], f[2] * spacing[2])[0]
    np.testing.assert_allclose(got, f[0] - 2.0 * f[1] + 3.0 * f[2], rtol=0, atol=1e-9)


@pytest.mark.parametrize("axis", ["z", "x"])
def test_negative_control_a_box_rolled_by_one_cell_fails_on_white_noise(oracle_lib, axis):
    """Sensitivity of the comparison itself: the reference is handed the oracle's box rolled by ONE cell along z / x.  On white
    noise nearly every point must then miss the bar in use, by orders of magnitude."""
    shape, spacing = (256, 64, 32), (3.0, 3.0, 3.0)
    box = br.white_noise_box(shape, seed=5)
    orc = _oracle_with(oracle_lib, box, spacing)
    rolled = np.roll(box, 1, axis={"x": 1, "z": 3}[axis])
    classes = br.coordinate_classes(shape, spacing, np.random.default_rng(1), n=24)
    ws, ti, t = (float(orc.info(k)[0]) for k in ("ws_global", "ti_global", "fs_time"))
    x, y, z = classes["interior"]
    got = orc.windspeed(0, x + ws * t, y, z=float(z[0]), include_wakes=False)
    good = np.abs(got - br.ambient_wind(box, spacing, ws, ti, t, (x + ws * t)[:, None], y[None, :], float(z[0])))
    bad = np.abs(got - br.ambient_wind(rolled, spacing, ws, ti, t, (x + ws * t)[:, None], y[None, :], float(z[0])))
    assert good.max() <= ORACLE_ATOL
    assert (bad > ORACLE_ATOL).mean() > 0.99 and np.median(bad) > 0.05, (float(np.median(bad)), float((bad > ORACLE_ATOL).mean()))
    orc.close()
