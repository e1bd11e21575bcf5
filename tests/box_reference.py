"""Plain float64 reference of the frozen-box lookups (helper of the box tests, not a test).

Written from the definition in MODEL.md §1 item 6, not from the kernels or the C oracle:

* the box is a periodic field of ``Nx x Ny x Nz`` nodes, node ``(i, j, k)`` sitting at ``(i dx, j dy, k dz)``;
* the value at a point is the trilinear interpolation of the 8 nodes around it — here the textbook weighted sum
  ``sum_abc w_a(x) w_b(y) w_c(z) g[i + a, j + b, k + c]`` in float64, indices taken modulo the dimension;
* Taylor's hypothesis: an env whose free wind is ``U`` reads the box at ``(x - U t + o_x, y + o_y, z)`` and adds
  ``TI U g`` to the inflow;
* the wake particles read the transverse components from the 4 x 4 x 4 block average of the same field, whose coarse
  cell ``I`` is centred at fine index ``4 I + 1.5``.
"""
import numpy as np


def trilinear_periodic(box, spacing, x, y, z):
    """``box`` [C, Nx, Ny, Nz], ``spacing`` (dx, dy, dz) in metres, points ``x, y, z`` (broadcast against each other, metres,
    any sign, any number of box lengths away) -> float64 [C, *points.shape]."""
    box = np.asarray(box)
    x, y, z = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(z, dtype=np.float64))
    idx, wgt = [], []
    for coord, d, n in zip((x, y, z), spacing, box.shape[1:]):
        f = coord / float(d)
        i = np.floor(f)
        t = f - i
        i = i.astype(np.int64)
        idx.append((np.mod(i, n), np.mod(i + 1, n)))
        wgt.append((1.0 - t, t))
    out = np.zeros((box.shape[0],) + x.shape)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                w = wgt[0][a] * wgt[1][b] * wgt[2][c]
                out += w * box[:, idx[0][a], idx[1][b], idx[2][c]].astype(np.float64)
    return out


def block_average(box):
    """The 4 x 4 x 4 block average [C, Nx/4, Ny/4, Nz/4] (float64) of a box whose dimensions are multiples of 4."""
    box = np.asarray(box)
    c, nx, ny, nz = box.shape
    assert nx % 4 == 0 and ny % 4 == 0 and nz % 4 == 0
    return box.reshape(c, nx // 4, 4, ny // 4, 4, nz // 4, 4).astype(np.float64).mean(axis=(2, 4, 6))


def coarse_trilinear_periodic(coarse, spacing, x, y, z):
    """Lookup of the block-averaged field ``coarse = block_average(box)`` at points given in the FINE box's metres
    (``spacing`` is the fine spacing): coarse node I sits at fine index 4 I + 1.5."""
    dx, dy, dz = (float(d) for d in spacing)
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    return trilinear_periodic(coarse, (4 * dx, 4 * dy, 4 * dz), x - 1.5 * dx, y - 1.5 * dy, z - 1.5 * dz)


def ambient_wind(box, spacing, ws, ti, time, x, y, z, offset=(0.0, 0.0)):
    """(u, v, w) float64 [3, *points.shape] of the wake-free inflow of an env with free wind ``ws``, turbulence intensity
    ``ti`` at flow time ``time``: U + TI U g_u, TI U g_v, TI U g_w with g read at (x - U t + o_x, y + o_y, z)."""
    g = trilinear_periodic(box[:3], spacing, np.asarray(x, dtype=np.float64) - ws * time + offset[0],
                           np.asarray(y, dtype=np.float64) + offset[1], z)
    out = ti * ws * g
    out[0] += ws
    return out


def white_noise_box(shape, seed, clip=3.0):
    """Unit-variance independent values per cell, clipped at ``clip`` sigma (float32 [3, Nx, Ny, Nz]): any wrong cell or weight
    of a lookup is then an error of the size of the field, while TI U g stays a physical fluctuation."""
    rng = np.random.default_rng(seed)
    return np.clip(rng.standard_normal((3,) + tuple(shape), dtype=np.float32), -clip, clip)


def coordinate_classes(shape, spacing, rng, n=48):
    """Box coordinates (x, y, z float64 arrays of one length) of the classes where a lookup goes wrong first; dict name -> (x, y, z).
    Every value is a multiple of 2^-6 m, so that float32 carries it exactly up to 2^18 m."""
    (nx, ny, nz), (dx, dy, dz) = shape, spacing
    q = lambda a: np.round(np.asarray(a, dtype=np.float64) * 64.0) / 64.0          # noqa: E731
    L = (nx * dx, ny * dy, nz * dz)
    u = lambda k: rng.uniform(0.0, 1.0, n) * L[k]                                   # noqa: E731
    out = {}
    # exactly on nodes: weights 0 / 1, including node 0 and the last node of every axis
    i = np.concatenate([[0, nx - 1, 0, nx - 1], rng.integers(0, nx, n - 4)])
    j = np.concatenate([[0, ny - 1, ny - 1, 0], rng.integers(0, ny, n - 4)])
    k = np.concatenate([[0, nz - 1, 0, nz - 1], rng.integers(0, nz, n - 4)])
    out["nodes"] = (i * float(dx), j * float(dy), k * float(dz))
    # inside the last cell of one axis: the upper neighbour is node 0 of that axis
    last = lambda k_, n_, d_: q((n_ - 1 + rng.uniform(0.05, 0.95, n)) * d_)        # noqa: E731
    out["wrap_x"] = (last(0, nx, dx), q(u(1)), q(u(2)))
    out["wrap_y"] = (q(u(0)), last(1, ny, dy), q(u(2)))
    out["wrap_z"] = (q(u(0)), q(u(1)), last(2, nz, dz))
    out["wrap_xyz"] = (last(0, nx, dx), last(1, ny, dy), last(2, nz, dz))
    out["interior"] = (q(u(0)), q(u(1)), q(u(2)))
    # negative box coordinates (floor, not truncation; the wrap of a negative index)
    out["negative"] = (q(-u(0) - 0.5 * dx), q(-u(1) - 0.5 * dy), q(u(2)))
    out["negative_small"] = (q(-rng.uniform(0.01, 0.99, n) * dx), q(-rng.uniform(0.01, 0.99, n) * dy), q(u(2)))
    # more than ten box lengths downstream / to the side
    out["far"] = (q(u(0) + rng.integers(10, 14, n) * L[0]), q(u(1) + rng.integers(10, 14, n) * L[1]), q(u(2)))
    return out
