"""Steady-state wake models and the serial-refine yaw optimiser built on them.

The reference's `PyWakeAgent` (WindGym/Agents/PyWakeAgent.py:21-143) optimises yaw set-points with the Serial-Refine
Method (:144-288) over py_wake's `Blondel_Cathelain_2020(site, turbine, turbulenceModel=CrespoHernandez(),
deflectionModel=JimenezWakeDeflection())`.  py_wake is not installed here, so the published models are restated:

  * `blondel_jimenez_power` — the wake model `PyWakeAgent` uses: super-Gaussian deficit of Blondel & Cathelain (2020,
    Wind Energ. Sci. 5, 1225-1236) evaluated at the rotor centre, linear superposition, free-stream reference speed,
    ambient TI in the wake width (py_wake defaults), Jimenez et al. (2010) deflection with beta = 0.1, tabular P / Ct at
    ws cos(yaw) with Ct cos^2(yaw).  Its momentum balance is checked numerically in tests/test_steady_optimizer.py.
  * `steady_state_power` — the steady state of the build's own dynamic model M0 (what the batched env converges to for
    constant yaws, pinned against the converged oracle): `SteadyStateYawAgent`.

Everything is batched over arbitrary leading dimensions with torch (CPU or GPU), so all wind conditions and all
candidate yaw offsets of a refine step are evaluated in one call.
"""
from __future__ import annotations

import numpy as np

from .agents import BaseAgent
from .config import rotor_points
from .turbine import V80, as_tabular


def _interp(x, xs, ys):
    """Linear interpolation on a uniform or non-uniform ascending table, 0 outside (torch)."""
    import torch
    idx = torch.clamp(torch.searchsorted(xs, x.contiguous(), right=True) - 1, 0, len(xs) - 2)
    f = (x - xs[idx]) / (xs[idx + 1] - xs[idx])
    out = ys[idx] + f * (ys[idx + 1] - ys[idx])
    return torch.where((x >= xs[0]) & (x <= xs[-1]), out, torch.zeros_like(out))


def steady_state_power(x, y, ws, wd, ti, yaw, turbine=None, n_rotor_pts=16, n_quad=48, device="cpu"):
    """Per-turbine power [..., N] of the steady state of model M0.

    x, y [N] layout; ws, wd, ti broadcastable to the batch shape [...]; yaw [..., N] in degrees (flow frame)."""
    import torch
    tab = as_tabular(turbine if turbine is not None else V80())
    dt = torch.float64
    dev = torch.device(device)
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dt, device=dev)   # noqa: E731
    x, y, yaw = T(x), T(y), (yaw.to(dev, dt) if isinstance(yaw, torch.Tensor) else T(yaw))
    batch = yaw.shape[:-1]
    N = yaw.shape[-1]
    ws = T(ws).expand(batch) if not isinstance(ws, torch.Tensor) else ws.to(dev, dt).expand(batch)
    wd = T(wd).expand(batch) if not isinstance(wd, torch.Tensor) else wd.to(dev, dt).expand(batch)
    ti = T(ti).expand(batch) if not isinstance(ti, torch.Tensor) else ti.to(dev, dt).expand(batch)
    D, hub = float(tab.diameter()), float(tab.hub_height())
    tws, tp, tc = T(tab.ws_tab), T(tab.power_tab), T(tab.ct_tab)
    ry, rz = (T(a) for a in rotor_points(n_rotor_pts, 0.5 * D))
    th = torch.deg2rad(270.0 - wd)[..., None]
    cx, cy = x.mean(), y.mean()
    xr = cx + (x - cx) * torch.cos(th) + (y - cy) * torch.sin(th)          # [..., N]
    yr = cy - (x - cx) * torch.sin(th) + (y - cy) * torch.cos(th)
    order = torch.argsort(xr, dim=-1)
    g = torch.deg2rad(yaw)
    cg, sg = torch.cos(g), torch.sin(g)
    u = ws[..., None].expand(batch + (N,)).clone()
    til = ti[..., None].expand(batch + (N,)).clone()
    ct = torch.zeros_like(u)
    hv = torch.zeros_like(u)
    s01 = torch.linspace(0.0, 1.0, n_quad, dtype=dt, device=dev)
    R = 0.5 * D

    def cfrac(ctv, sp):
        m = torch.clamp(1.0 / (8.0 * sp * sp), max=1.0)
        return 1.0 - torch.sqrt(torch.clamp(1.0 - ctv * m, min=0.0))

    for pos in range(N):
        t = order[..., pos:pos + 1]                                            # [..., 1] target index
        xt, yt, cgt = (a.gather(-1, t) for a in (xr, yr, cg))
        dx = xt - xr                                                            # [..., N] distance from every source
        up = dx > 1e-9
        k = 0.38 * til + 0.004
        q = torch.sqrt(1.0 - ct)
        eps = 0.2 * torch.sqrt(0.5 * (1.0 + q) / q)
        xd = torch.clamp(dx, min=0.0) / D
        sp = k * xd + eps
        sig = sp * D
        # wake-centre deflection: (hv / U) * integral_0^dx C(x') dx'  (trapezoid on n_quad points)
        xq = torch.clamp(dx, min=0.0)[..., None] * s01                          # [..., N, Q]
        cq = cfrac(ct[..., None], k[..., None] * (xq / D) + eps[..., None])
        integ = torch.trapezoid(cq, xq, dim=-1)
        yc = yr + hv / ws[..., None] * integ
        amp = u * cfrac(ct, sp)
        ys = yt[..., None] + ry * cgt[..., None]                                # [..., 1, S]
        r2 = (ys - yc[..., None]) ** 2 + rz ** 2                                # [..., N, S]
        rc2 = (yt - yc) ** 2
        keep = up & (rc2 <= (R + 5.0 * sig) ** 2)
        dfc = torch.where(keep[..., None], amp[..., None] * torch.exp(-r2 / (2.0 * sig[..., None] ** 2)), torch.zeros_like(r2))
        ut = ws[..., None] - dfc.sum(dim=(-1, -2))[..., None] / n_rotor_pts
        ind = 0.5 * (1.0 - torch.sqrt(1.0 - ct))
        tia = 0.73 * ind ** 0.8325 * ti[..., None] ** 0.0325 * torch.clamp(xd, min=1.0) ** (-0.32) * torch.exp(-rc2 / (2 * sig ** 2))
        tia = torch.where(keep, tia, torch.zeros_like(tia)).amax(dim=-1, keepdim=True)
        tit = torch.sqrt(ti[..., None] ** 2 + tia ** 2)
        wsn = torch.clamp(ut * cgt, min=0.0)
        ctt = torch.clamp(_interp(wsn, tws, tc) * cgt ** 2, 0.0, 0.96)
        u = u.scatter(-1, t, ut)
        til = til.scatter(-1, t, tit)
        ct = ct.scatter(-1, t, ctt)
        hv = hv.scatter(-1, t, -0.4 * sg.gather(-1, t) * ut)
    return _interp(torch.clamp(u * cg, min=0.0), tws, tp)


# constants of Blondel & Cathelain (2020), Table 2 / py_wake BlondelSuperGaussianDeficit2020 defaults
BC_A_S, BC_B_S, BC_C_S = 0.17, 0.005, 0.2          # characteristic width sigma/D = (a_s TI + b_s) x/D + c_s sqrt(beta)
BC_A_F, BC_B_F, BC_C_F = 3.11, -0.68, 2.41         # super-Gaussian order n = a_f exp(b_f x/D) + c_f
JIMENEZ_BETA = 0.1                                  # wake-expansion factor of the deflection model (py_wake default)


def blondel_centre_deficit(ct, sigma, n):
    """Centre-line deficit fraction C of the super-Gaussian wake (Blondel & Cathelain 2020, eq. 6), from mass and
    momentum conservation: C = 2^(2/n - 1) - sqrt(2^(4/n - 2) - n ct / (16 Gamma(2/n) sigma^(4/n))); n = 2 gives the
    Gaussian wake of Bastankhah & Porte-Agel."""
    import torch
    a1 = 2.0 ** (2.0 / n - 1.0)
    a2 = 2.0 ** (4.0 / n - 2.0)
    g = torch.exp(torch.lgamma(2.0 / n))
    return a1 - torch.sqrt(torch.clamp(a2 - n * ct / (16.0 * g * sigma ** (4.0 / n)), min=0.0))


def blondel_jimenez_power(x, y, ws, wd, ti, yaw, turbine=None, n_quad=20, device="cpu"):
    """Per-turbine power [..., N] of the steady-state model behind the reference's PyWakeAgent (see the module
    docstring).  x, y [N]; ws, wd, ti broadcastable to the batch shape; yaw [..., N] degrees."""
    import torch
    tab = as_tabular(turbine if turbine is not None else V80())
    dt = torch.float64
    dev = torch.device(device)
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dt, device=dev)   # noqa: E731
    x, y, yaw = T(x), T(y), (yaw.to(dev, dt) if isinstance(yaw, torch.Tensor) else T(yaw))
    batch = yaw.shape[:-1]
    N = yaw.shape[-1]
    ws, wd, ti = ((a.to(dev, dt) if isinstance(a, torch.Tensor) else T(a)).expand(batch) for a in (ws, wd, ti))
    D = float(tab.diameter())
    tws, tp, tc = T(tab.ws_tab), T(tab.power_tab), T(tab.ct_tab)
    th = torch.deg2rad(270.0 - wd)[..., None]
    cx, cy = x.mean(), y.mean()
    xr = cx + (x - cx) * torch.cos(th) + (y - cy) * torch.sin(th)
    yr = cy - (x - cx) * torch.sin(th) + (y - cy) * torch.cos(th)
    order = torch.argsort(xr, dim=-1)
    g = torch.deg2rad(yaw)
    cg, sg = torch.cos(g), torch.sin(g)
    u = ws[..., None].expand(batch + (N,)).clone()          # effective wind speed of every turbine
    ct = torch.zeros_like(u)
    # py_wake's quadrature of the Jimenez angle: points clustered towards the rotor
    s01 = (torch.logspace(0.0, 1.1, n_quad, dtype=dt, device=dev) - 1.0) / (10.0 ** 1.1 - 1.0)
    for pos in range(N):
        t = order[..., pos:pos + 1]
        xt, yt = xr.gather(-1, t), yr.gather(-1, t)
        dx = xt - xr
        up = dx > 1e-9
        xd = torch.clamp(dx, min=1e-9) / D
        q = torch.sqrt(1.0 - torch.clamp(ct, max=0.999))
        beta = 0.5 * (1.0 + q) / q
        sigma = (BC_A_S * ti[..., None] + BC_B_S) * xd + BC_C_S * torch.sqrt(beta)
        n = BC_A_F * torch.exp(BC_B_F * xd) + BC_C_F
        C = blondel_centre_deficit(ct, sigma, n)
        # Jimenez: initial skew angle cos^2 sin ct/2, decaying with (1 + beta x/D)^-2; the deflection is its integral
        xq = torch.clamp(dx, min=0.0)[..., None] * s01
        alpha = (cg ** 2 * sg * ct * 0.5)[..., None] / (1.0 + JIMENEZ_BETA * xq / D) ** 2
        defl = -torch.trapezoid(torch.sin(alpha), xq, dim=-1)       # positive yaw pushes the wake towards -y (env frame)
        r = torch.abs(yt - (yr + defl)) / D
        dfc = torch.where(up, ws[..., None] * C * torch.exp(-r ** n / (2.0 * sigma ** 2)), torch.zeros_like(r))
        ut = ws[..., None] - dfc.sum(dim=-1, keepdim=True)
        cgt = cg.gather(-1, t)
        ctt = torch.clamp(_interp(torch.clamp(ut * cgt, min=0.0), tws, tc) * cgt ** 2, 0.0, 0.999)
        u = u.scatter(-1, t, ut)
        ct = ct.scatter(-1, t, ctt)
    return _interp(torch.clamp(u * cg, min=0.0), tws, tp)


WAKE_MODELS = {"m0": None, "blondel_jimenez": blondel_jimenez_power}
MODEL_IDS = {"m0": 0, "blondel_jimenez": 1}        # `model` of wg_steady_power / wg_steady_optimize


def hip_batch_for(x, y, turbine=None, n_rotor_pts=16, device=None, deficit=None, model_constants=None):
    """A minimal :class:`windgym_amd.binding.HipBatch` (one env) that carries a layout and a turbine to the device, so that
    ``HipBatch.steady_power`` (k_steady) can evaluate steady-state farm powers for it.  ``deficit`` / ``model_constants``: those
    of the env the yaws are optimised for (EnvConfig's) — model "m0" is the steady state of THAT flow model, and the library
    refuses it (WG_ERR_UNSUPPORTED) for a deficit k_steady does not carry rather than answering with Gaussian powers."""
    from .binding import HipBatch
    from .config import EnvConfig
    from .presets import env1_config
    d = env1_config()
    d["power_def"]["Power_reward"] = "Power_avg"
    extra = {}
    if deficit is not None:
        extra["deficit"] = deficit
    if model_constants is not None:
        extra["model_constants"] = model_constants
    cfg = EnvConfig(turbine=turbine if turbine is not None else V80(), yaml_dict=d, turbtype="None", n_envs=1,
                    x_pos=np.asarray(x, dtype=float), y_pos=np.asarray(y, dtype=float), n_rotor_pts=n_rotor_pts, **extra)
    return HipBatch(cfg, device=device)


def srf_offsets(refine_pass_n, yaw_n, yaw_max):
    """The candidate offsets of every Serial-Refine pass, float64 [refine_pass_n, yaw_n] degrees: row r is the linspace over
    +-yaw_max / 2**r that `yaw_optimizer_srf` walks (the table wg_steady_optimize is handed, so that the device does not
    restate torch.linspace)."""
    import torch
    rows = [torch.linspace(-float(yaw_max) / 2.0 ** r, float(yaw_max) / 2.0 ** r, int(yaw_n), dtype=torch.float64)
            for r in range(int(refine_pass_n))]
    return torch.stack(rows) if rows else torch.zeros((0, int(yaw_n)), dtype=torch.float64)


def yaw_optimizer_srf(x, y, ws, wd, ti, turbine=None, refine_pass_n=8, yaw_n=9, yaw_max=30.0, device="cpu",
                      model="m0", batch=None, fused=False):
    """Serial-Refine yaw optimisation (PyWakeAgent.py:144-288) for a batch of wind conditions at once.
    ws, wd, ti: arrays of the same length C.  Returns yaw [C, N] in degrees.  model: "m0" (steady state of the build's
    dynamic model) or "blondel_jimenez" (the reference agent's py_wake model).
    ``batch``: a HipBatch of the same layout / turbine — every refine step is then ONE launch of the HIP kernel k_steady
    over [conditions x candidates] cases (wg_steady_power) instead of the torch restatement.  ``fused=True`` (needs
    ``batch``): the whole optimisation of all conditions is ONE launch of k_steady_srf (HipBatch.steady_optimize) — the same
    rules, candidate powers bit-equal to k_steady's, no host round trip per refine step."""
    import torch
    if fused:
        if batch is None:
            raise ValueError("yaw_optimizer_srf(fused=True) runs on the device: pass batch= (steady.hip_batch_for)")
        return batch.steady_optimize(ws, wd, ti, model=model, refine_pass_n=refine_pass_n, yaw_n=yaw_n,
                                     yaw_max=yaw_max)[0].cpu().numpy()
    fn = WAKE_MODELS[model]
    steady_state_power = fn if fn is not None else globals()["steady_state_power"]
    if batch is not None:
        def steady_state_power(x_, y_, ws_, wd_, ti_, yaw_, turbine_=None, device=None):      # noqa: F811
            yaw_ = torch.as_tensor(yaw_)
            shp = yaw_.shape
            b = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float32), shp[:-1]).reshape(-1)   # noqa: E731
            return batch.steady_power(b(ws_), b(wd_), b(ti_), yaw_.reshape(-1, shp[-1]), model=model).double().reshape(shp)
    ws, wd, ti = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (ws, wd, ti))
    C, N = len(ws), len(x)
    wd = wd + 1e-3                                   # break the two-maxima tie of perfectly aligned rows (:188-189)
    yaw = torch.zeros((C, N), dtype=torch.float64)
    power = steady_state_power(x, y, ws, wd, ti, yaw, turbine, device=device).sum(-1).cpu()
    th = np.radians((270.0 - wd) % 360)
    xrot = np.asarray(x)[None, :] * np.cos(th)[:, None] + np.asarray(y)[None, :] * np.sin(th)[:, None]
    order = np.argsort(xrot, axis=1)                 # upstream -> downstream (:203-210)
    rng = float(yaw_max)
    ar = torch.arange(C)
    for _ in range(refine_pass_n):
        offs = torch.linspace(-rng, rng, yaw_n, dtype=torch.float64)
        rng /= 2.0
        for pos in range(N):
            tidx = torch.as_tensor(order[:, pos])
            cand = yaw[:, None, :].repeat(1, yaw_n, 1)                          # [C, yaw_n, N]
            cand[ar[:, None], torch.arange(yaw_n)[None, :], tidx[:, None]] = yaw[ar, tidx][:, None] + offs[None, :]
            p = steady_state_power(x, y, ws[:, None], wd[:, None], ti[:, None], cand, turbine, device=device).sum(-1).cpu()
            best = p.argmax(dim=1)
            bp = p[ar, best]
            better = bp > power
            yaw[ar[better], tidx[better]] = cand[ar[better], best[better], tidx[better]]
            power[better] = bp[better]
    return torch.clamp(yaw, -yaw_max, yaw_max).numpy()


class SteadyStateYawAgent(BaseAgent):
    """Serial-Refine yaw agent with the reference PyWakeAgent's interface (same constructor, `update_wind`, `optimize`,
    `optimized_yaws`, `predict`); `model` selects the wake model: "m0" = steady state of the env's own flow model (the
    yaws that are optimal FOR THE ENV), "blondel_jimenez" = the model the reference agent uses."""
    model = "m0"

    def __init__(self, x_pos, y_pos, wind_speed=8, wind_dir=270, TI=0.07, yaw_max=45, yaw_min=-45, refine_pass_n=8,
                 yaw_n=9, turbine=None, device="cpu", model=None, deficit=None, model_constants=None, fused=False):
        if model is not None:
            self.model = model
        if fused and not str(device).startswith(("cuda", "hip")):
            raise ValueError('fused=True is the one-launch optimiser on the device: it needs device="cuda"')
        self.fused = bool(fused)
        super().__init__(yaw_max, yaw_min)
        self.pywakeagent = True
        self.optimized = False
        self.x_pos, self.y_pos = np.asarray(x_pos, dtype=float), np.asarray(y_pos, dtype=float)
        if len(self.x_pos) != len(self.y_pos):
            raise ValueError("x_pos and y_pos must have the same length.")
        self.n_wt = len(self.x_pos)
        self.wsp, self.wdir, self.TI = np.asarray([wind_speed], float), np.asarray([wind_dir], float), TI
        self.refine_pass_n, self.yaw_n = refine_pass_n, yaw_n
        self.turbine = turbine if turbine is not None else V80()
        self.device = device
        # device "cuda" / "hip": the candidates of every refine step are evaluated by the HIP kernel k_steady
        self._batch = None
        if str(device).startswith(("cuda", "hip")):
            self._batch = hip_batch_for(self.x_pos, self.y_pos, self.turbine, deficit=deficit, model_constants=model_constants)

    def close(self):
        """release the device handle behind device="cuda" (the agent stays usable on its torch path)"""
        if self._batch is not None:
            self._batch.close()
            self._batch = None
            self.device = "cpu"

    def update_wind(self, wind_speed, wind_direction, TI):
        self.wsp, self.wdir, self.TI = np.asarray([wind_speed], float), np.asarray([wind_direction], float), TI
        self.optimized = False

    def reset(self):
        self.optimized = False

    def optimize(self):
        self.optimized_yaws = yaw_optimizer_srf(self.x_pos, self.y_pos, self.wsp, self.wdir, [self.TI], self.turbine,
                                                self.refine_pass_n, self.yaw_n, device="cpu" if self._batch is not None else self.device,
                                                model=self.model, batch=self._batch, fused=self.fused and self._batch is not None)[0]
        self.action = self.scale_yaw(self.optimized_yaws).astype(np.float32)
        self.optimized = True

    def power(self, yaws):
        if self._batch is not None:
            return float(self._batch.steady_power(self.wsp[0], self.wdir[0], self.TI, np.asarray(yaws, dtype=np.float32)[None],
                                                  model=self.model).sum())
        fn = WAKE_MODELS[self.model] or steady_state_power
        return float(fn(self.x_pos, self.y_pos, self.wsp[0], self.wdir[0], self.TI, np.asarray(yaws, dtype=float),
                        self.turbine, device=self.device).sum())

    def predict(self, *args, **kwargs):
        if not self.optimized:
            self.optimize()
        return self.action, None


class PyWakeAgent(SteadyStateYawAgent):
    """The reference's PyWakeAgent (WindGym/Agents/PyWakeAgent.py): Serial-Refine over Blondel-Cathelain (2020) +
    Jimenez deflection, restated from the publications (py_wake itself is not installed: values are not pinned against
    py_wake, only against the equations — tests/test_steady_optimizer.py)."""
    model = "blondel_jimenez"


class SteadyStateYawVecAgent(BaseAgent):
    """The Serial-Refine yaw agent for a whole batch of envs (`WindFarmVecEnv`, or anything with a `.batch` / `._batch`
    HipBatch): `predict` returns `scale_yaw` of the optimal yaws of every env's CURRENT wind, float32 [B, N].  The winds are
    read on the device and all envs are optimised by ONE launch (HipBatch.optimal_yaws -> k_steady_srf); the agent optimises
    again whenever an env's episode counter (info "episode") has moved since the last call, so it follows autoresets.
    `UseEnv`: `eval_sweep` binds it to the sweep's env, and every condition of the sweep gets its own yaws.
    `optimized_yaws` [B, N] float64 degrees stays on the device; the actions are a numpy array unless the env works on CUDA
    tensors (`as_torch`)."""
    model = "m0"

    def __init__(self, env=None, model=None, refine_pass_n=8, yaw_n=9, yaw_max=45, yaw_min=-45, search_yaw_max=30.0):
        if model is not None:
            self.model = model
        super().__init__(yaw_max, yaw_min)
        self.UseEnv = True
        self.pywakeagent = True
        self.env = env
        self.refine_pass_n, self.yaw_n, self.search_yaw_max = refine_pass_n, yaw_n, search_yaw_max
        self.reset()

    def reset(self):
        """forget the optimum: the next `predict` optimises again"""
        self.optimized_yaws = None
        self._episode = self._batch_seen = None

    def _batch(self):
        if self.env is None:
            raise ValueError(f"{type(self).__name__} needs an env (env=, or eval_sweep binds it)")
        b = getattr(self.env, "batch", None)
        return b if b is not None else getattr(self.env, "_batch")

    def optimize(self):
        b = self._batch()
        self.optimized_yaws = b.optimal_yaws(model=self.model, refine_pass_n=self.refine_pass_n, yaw_n=self.yaw_n,
                                             yaw_max=self.search_yaw_max)
        self._batch_seen = b

    def predict(self, *args, **kwargs):
        b = self._batch()
        episode = b.info("episode")
        if (self.optimized_yaws is None or self._batch_seen is not b or self._episode is None
                or tuple(episode.shape) != tuple(self._episode.shape) or not bool((episode == self._episode).all())):
            self.optimize()
            self._episode = episode
        a = ((self.optimized_yaws - self.yaw_min) / (self.yaw_max - self.yaw_min) * 2 - 1).float()      # scale_yaw, on the device
        if not getattr(self.env, "as_torch", False):
            a = a.cpu().numpy()
        return (a if hasattr(self.env, "batch") else a[0]), None


class PyWakeVecAgent(SteadyStateYawVecAgent):
    """`SteadyStateYawVecAgent` over the reference PyWakeAgent's wake model (Blondel-Cathelain 2020 + Jimenez)."""
    model = "blondel_jimenez"
