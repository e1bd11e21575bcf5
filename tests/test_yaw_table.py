"""CPU tests of the yaw table (windgym_amd/yaw_table.py, windgym_amd/csrc/wg_yaw_table.h): the numpy twin of the node rule against
a brute-force nearest node, the header's function against the twin bit for bit (compiled by g++ alone), the row formula, the npz
round trip and every refusal that needs no device."""
import ctypes as C
import io

import numpy as np
import pytest

import yaw_table_twin as tw
from helpers import host_shim
from windgym_amd import yaw_table as yt

# Axes whose nodes are multiples of 2^-3 below 2^10, and values that are multiples of 2^-11: every sum of two nodes, every midpoint
# and every difference value - node is then exact in float64, so the brute-force argmin below has no rounding of its own to decide a
# tie and "nearest, the lower node on a tie" is a fact about the numbers, not about an implementation.
rng = np.random.default_rng(11)


def _nonuniform(n):
    return np.cumsum(rng.integers(1, 40, n)).astype(np.float64) * 0.125 - 7.0


AXES = {"uniform_1": np.array([8.0]), "uniform_2": np.array([3.0, 3.625]), "uniform_37": 3.0 + 0.625 * np.arange(37),
        "nonuniform_1": np.array([-2.375]), "nonuniform_2": _nonuniform(2), "nonuniform_37": _nonuniform(37)}
WRAP_AXES = {"wrap_1": np.array([12.5]), "wrap_2": np.array([0.0, 181.25]), "wrap_37": 2.25 + 9.5 * np.arange(37),
             "wrap_nonuniform_37": np.cumsum(rng.integers(1, 76, 37)).astype(np.float64) * 0.125 - 20.0}


def _values(a, lo, hi, n=4000):
    """random values, every node, every exact midpoint (the virtual node's included), values outside both ends"""
    span = max(hi - lo, 1.0)
    x = np.round(rng.uniform(lo - 0.25 * span, hi + 0.25 * span, n) * 2048.0) / 2048.0
    ext = np.append(a, a[0] + 360.0)
    return np.concatenate([x, a, (ext[:-1] + ext[1:]) / 2.0, [lo - 1000.0, hi + 1000.0, lo - 0.125, hi + 0.125]])


def _nearest(nodes, x):
    """brute force: argmin of |x - node| in float64, the lower node on a tie (np.argmin returns the first minimum)"""
    return np.abs(x[:, None] - nodes[None, :]).argmin(axis=1)


@pytest.mark.parametrize("name", list(AXES))
def test_twin_is_the_nearest_node(name):
    a = AXES[name]
    x = _values(a, a[0], a[-1])
    assert np.array_equal(tw.axis_index(a, x), _nearest(a, x))
    # the ends, and what is not a number: +-inf go to the end nodes, NaN compares below every midpoint
    assert list(tw.axis_index(a, np.array([-np.inf, np.inf, np.nan]))) == [0, len(a) - 1, 0]


@pytest.mark.parametrize("name", list(WRAP_AXES))
def test_twin_wraps_to_the_nearest_node_on_the_circle(name):
    a = WRAP_AXES[name]
    assert a[-1] - a[0] < 360.0
    x = np.concatenate([_values(a, a[0] - 720.0, a[0] + 720.0, 8000), a - 360.0, a + 360.0, [a[0] - 720.0, a[0] + 720.0]])
    assert x.min() >= a[0] - 720.0 - 1000.0 and np.all(x * 2048.0 == np.round(x * 2048.0))
    # the same argmin after the value is brought into [a_0, a_0 + 360) exactly (everything here is a multiple of 2^-11), with the
    # first node returning as a_0 + 360
    u = x - 360.0 * np.floor((x - a[0]) / 360.0)
    assert np.all((u >= a[0]) & (u < a[0] + 360.0))
    k = _nearest(np.append(a, a[0] + 360.0), u)
    assert np.array_equal(tw.axis_index(a, x, wrap=True), np.where(k == len(a), 0, k))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return host_shim(tmp_path_factory, "yaw_table")


def _shim_axis(shim, a, x, wrap):
    a, x = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(x, np.float64)
    out = np.full(len(x), -7, np.int32)
    shim.yt_axis(a.ctypes.data_as(C.c_void_p), len(a), int(wrap), x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p))
    return out


# axes with no exactness to lean on: the header and the twin must still agree, both being the same rule
ROUGH = {"linspace_37": np.linspace(0.04, 0.16, 37), "random_37": np.sort(rng.uniform(-50.0, 300.0, 37)), "thirds_2": np.array([1.0 / 3.0, 2.0 / 3.0]),
         "one": np.array([0.1])}


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("name", list(AXES) + list(WRAP_AXES) + list(ROUGH))
def test_header_equals_twin(shim, name, wrap):
    a = {**AXES, **WRAP_AXES, **ROUGH}[name]
    assert a[-1] - a[0] < 360.0                                 # (every axis here may wrap)
    ext = np.append(a, a[0] + 360.0)
    mid = (ext[:-1] + ext[1:]) / 2.0
    x = np.concatenate([_values(a, a[0] - 720.0, a[0] + 720.0), rng.uniform(a[0] - 720.0, a[0] + 720.0, 4000), a, mid, np.nextafter(mid, np.inf),
                        np.nextafter(mid, -np.inf), a - 360.0, a + 360.0, [np.inf, -np.inf, np.nan, 0.0, -0.0, 1e300, -1e300]])
    assert np.array_equal(_shim_axis(shim, a, x, wrap), tw.axis_index(a, x, wrap).astype(np.int32))


def test_row_formula_header_and_twin(shim):
    ti, ws, wd = np.array([0.05, 0.1]), np.array([6.0, 8.0, 10.0, 12.0, 14.0]), np.array([260.0, 270.0, 280.0])
    wind = yt.node_winds(ti, ws, wd)
    assert np.array_equal(tw.rows(ti, ws, wd, wind), np.arange(2 * 5 * 3))                 # node r's own wind has row r
    assert tw.rows(ti, ws, wd, [[9.0, 275.0, 0.075]])[0] == (0 * 5 + 1) * 3 + 1            # three ties, three lower nodes
    assert tw.rows(ti, ws, wd, [[9.1, 275.1, 0.0751]])[0] == (1 * 5 + 2) * 3 + 2
    w = np.concatenate([wind, rng.uniform([4.0, 200.0, 0.0], [16.0, 340.0, 0.2], (500, 3)),
                        [[np.nan, 270.0, 0.07], [8.0, np.inf, 0.07], [8.0, 270.0, -np.inf], [8.0, 270.0, 0.07]]])
    mask = (rng.uniform(size=len(w)) < 0.7).astype(np.uint8)
    for wrap in (False, True):
        ref = tw.rows(ti, ws, wd, w, wrap_wd=wrap)
        assert list(ref[-4:-1]) == [-1, -1, -1] and ref[-1] == (0 * 5 + 1) * 3 + 1
        assert np.array_equal(tw.rows(ti, ws, wd, w, mask, wrap)[mask == 0], np.full(int((mask == 0).sum()), -1))
        ax = np.concatenate([ti, ws, wd])
        out = np.full(len(w), -7, np.int32)
        wc = np.ascontiguousarray(w)
        shim.yt_rows(ax.ctypes.data_as(C.c_void_p), 2, 5, 3, int(wrap), wc.ctypes.data_as(C.c_void_p), len(w), out.ctypes.data_as(C.c_void_p))
        assert np.array_equal(out, ref)
    # on a wrapping axis 355 degrees is nearer to the node at 0 than to the one at 340
    assert tw.rows([0.07], [8.0], np.arange(0.0, 360.0, 20.0), [[8.0, 355.0, 0.07], [8.0, -5.0, 0.07]], wrap_wd=True).tolist() == [0, 0]
    assert tw.rows([0.07], [8.0], np.arange(0.0, 360.0, 20.0), [[8.0, 355.0, 0.07], [8.0, -5.0, 0.07]]).tolist() == [17, 0]


def test_default_axes():
    assert np.array_equal(yt.default_axis(6.0, 14.0, 1.0), np.arange(6.0, 15.0))
    assert np.array_equal(yt.default_axis(8.0, 8.0, 1.0), [8.0])
    a = yt.default_axis(6.0, 8.5, 1.0)                          # both ends are nodes, the spacing never exceeds the step
    assert a[0] == 6.0 and a[-1] == 8.5 and len(a) == 4
    assert np.array_equal(yt.default_axis(0.02, 0.12, 0.05), np.linspace(0.02, 0.12, 3))


def _table(**kw):
    ti, ws, wd = np.array([0.05, 0.1]), np.array([6.0, 8.0, 10.0]), np.array([265.0, 270.0, 275.0, 280.0])
    yaw = rng.uniform(-30, 30, (24, 5))
    args = dict(ti=ti, ws=ws, wd=wd, yaw=yaw, power=rng.uniform(1e6, 2e6, 24), wrap_wd=False, args=dict(model="m0", refine_pass_n=4, yaw_n=5,
                                                                                                        search_yaw_max=30.0))
    args.update(kw)
    return yt.YawTable(**args)


def test_npz_round_trip_without_pickle(tmp_path):
    tab = _table(wrap_wd=True)
    path = tab.save(str(tmp_path / "table"))                    # (no ".npz" is appended to the name)
    assert path == str(tmp_path / "table")
    with np.load(path, allow_pickle=False) as z:                # every member loads with pickling refused
        assert sorted(z.files) == ["meta", "power", "ti", "wd", "ws", "yaw"] and all(z[k].dtype != object for k in z.files)
    for back in (yt.YawTable.load(path), yt.YawTable.from_bytes(tab.to_bytes())):
        assert back.wrap_wd is True and back.args == tab.args and (back.n_rows, back.N) == (24, 5) and back.device is None
        for k in ("ti", "ws", "wd", "yaw", "power"):
            assert np.array_equal(getattr(back, k), getattr(tab, k)) and getattr(back, k).dtype == np.float64
    bad = io.BytesIO()
    np.savez(bad, ti=tab.ti, ws=tab.ws, wd=tab.wd)
    bad.seek(0)
    with pytest.raises(ValueError, match="not a YawTable file"):
        yt.YawTable.load(bad)
    pickled = tmp_path / "pickled.npz"
    np.savez(str(pickled), ti=tab.ti, ws=tab.ws, wd=tab.wd, yaw=tab.yaw, meta=np.array([{"wrap_wd": False}], dtype=object))
    with pytest.raises(ValueError, match="(?i)pickle"):
        yt.YawTable.load(str(pickled))


def test_refusals_name_the_argument():
    with pytest.raises(ValueError, match="^ws: .*strictly ascending"):
        _table(ws=np.array([6.0, 10.0, 8.0]), yaw=np.zeros((24, 5)))
    with pytest.raises(ValueError, match="^wd: .*strictly ascending"):
        _table(wd=np.array([265.0, 270.0, 270.0, 280.0]))
    with pytest.raises(ValueError, match="^ti: .*non-empty"):
        _table(ti=np.array([]), yaw=np.zeros((0, 5)), power=None)
    with pytest.raises(ValueError, match="^ws: .*non-empty"):
        _table(ws=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="^ti: .*finite"):
        _table(ti=np.array([0.05, np.nan]))
    with pytest.raises(ValueError, match="^wrap_wd: wd spans 360"):
        _table(wd=np.array([0.0, 120.0, 240.0, 360.0]), wrap_wd=True)
    with pytest.raises(ValueError, match="^wrap_wd: wd spans 400"):
        _table(wd=np.array([0.0, 120.0, 240.0, 400.0]), wrap_wd=True)
    _table(wd=np.array([0.0, 120.0, 240.0, 359.0]), wrap_wd=True)
    _table(wd=np.array([0.0, 120.0, 240.0, 400.0]))             # (without the statement an axis may span anything)
    with pytest.raises(ValueError, match=r"^yaw: expected \[24, N\]"):
        _table(yaw=np.zeros((23, 5)))
    with pytest.raises(ValueError, match=r"^power: expected \[24\]"):
        _table(power=np.zeros(5))
    with pytest.raises(ValueError, match="^ti / ws / wd: 1027 nodes"):
        yt.check_axes([0.1], [8.0, 9.0], np.arange(1024.0))
    tab = _table()
    for call in (lambda: tab.rows(None), lambda: tab.targets(None)):
        with pytest.raises(ValueError, match="not on a device"):
            call()

    class FakeBatch:
        N = 4
    with pytest.raises(ValueError, match="^venv: the table holds yaws of 5 turbines, this env has 4"):
        _table(venv=type("V", (), {"batch": FakeBatch()})())
    with pytest.raises(ValueError, match="^venv: "):
        _table(venv=object())
    with pytest.raises(ValueError, match="table must be a YawTable"):
        yt.YawTableAgent(object())
