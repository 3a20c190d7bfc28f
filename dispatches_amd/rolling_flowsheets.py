"""Device-resident batched double loop for ANY of the three flowsheets of the reference (BASELINE config 2 is a "Nuclear case
double-loop"; config 4 the wind + battery one, whose specialised form - fused update kernel, recording - is dispatches_amd/rolling.py).

The same simulated day as rolling.py (1 day-ahead bidding solve, then per hour: real-time bid, stub clearing, tracking, state hand-off)
written once over a small DESCRIPTOR of the flowsheet's rolling-horizon state:

    flowsheet        realised state handed from the tracker to the next hour's LPs                          window data
    wind_battery     state of charge, energy throughput, rounded to 2 dp  (wind_battery_double_loop.py:181-209)    capacity factors
    wind_pem         none: only the capacity-factor window advances        (wind_PEM_double_loop.py:185-204)        capacity factors
    nuclear          tank holdup, rounded to an integer `round(holdup[-1])` (nuclear_flowsheet_multiperiod_class.py:218-239)   -

Everything per plant lives in HBM and is updated by device index operations; the solves go through the C ABI on device pointers
(day-ahead: PDLP kernel; 4-h / 12-h LPs: in-wave simplex first); the steps of a day are captured into hipGraphs on the second day and
replayed.  Power output and objective come from the flowsheet's own expressions as dense rows (P_T = PT x + PT_const), so nothing
below knows a flowsheet's columns except through the descriptor.  By default the market is the stub of rolling.py (every offer clears
at its maximum; day-ahead bids of day d at hour 0 of day d).

Stochastic mode (n_price_scenarios / forecaster="backcast" / market="price_taker"; the reference's nuclear double loop runs a Bidder with
n_scenario = 3 on a Backcaster, nuclear_flowsheet_double_loop.ipynb): the semantics of rolling.py's stochastic mode over the descriptor.
Every plant bids on S backcast scenarios (rows b * S + i of the bidding batches), the S solutions of a period become one bid curve that
starts at the generator's p_min (400 MW for the nuclear unit, Bidder._assemble_bids), a price-taker market dispatches the plant along it,
and the tracker follows the cleared dispatch.  `_day_ahead_step_stochastic` / `_hour_step_bid` are the executable specification as
tensor operations; csrc/dsp_market.hip (dsp_loop_market_*) is the same arithmetic in two kernels, bit for bit.

Parametrized mode (bidder="parametrized", bid_price, storage_mw; the reference's wind + PEM study run_double_loop_PEM.py bids with a
PEMParametrizedBidder on a PerfectForecaster, run_double_loop_battery_parametrized.py with a FixedParametrizedBidder): no bidding LP.
The curve of a (plant, period) is a closed form of the available wind w, the plant's storage size and its bid price - the pairs
(0, 0), (max(0, w - storage_mw), 0), (p_max, bid_price) through the same curve and clearing rules -, day-ahead on the day-ahead capacity
factors, hourly on the real-time ones; only the tracking LPs are solved.  `_day_ahead_step_parametrized` / `_hour_step_parametrized`
are the specification as tensor operations; csrc/dsp_param.hip (dsp_loop_param_step) is the same arithmetic in one kernel per step.

Per-plant sizes (wind_mw, battery_mw, battery_mwh with the LP bidder; the reference's run_double_loop_battery.py takes --wind_pmax,
--battery_pmax and --battery_energy_capacity and its study runs one job per size point): in these flowsheets a size is never a matrix
coefficient.  The wind size is the upper bound of the wind columns (wind_kw[b] * capacity factor, every step) and two objective
constants (curtailment, fixed O&M); the battery's power and energy limits are static column / row bounds written once.  So a batch of
DIFFERENT plants shares one template - built at the batch's largest sizes, see `_check_template` - and the kernels read two arrays
[B] where they read two scalars (dsp_loop_model / dsp_loop_market_model: wind_kw_plant, c0_base_plant).

Bidding at the RUC hour (ruc_hour=H with the LP bidder; the reference's DoubleLoopCoordinator.bid_into_DAM, run_double_loop_battery.py:255-294
builds its two trackers; our host restatement is workflow/coordinator.py::_project_tracking_trajectory): the day-ahead market of day d + 1
runs at hour H of day d.  Day 0 bids at hour 0 from the initial state, as above.  At hour-of-day H of every day, before that hour's
real-time step, the PROJECTION tracker - a _Model of its own on the tracker's template - starts from the realised state and solves 24 - H
chained tracking LPs: step j tracks da_offer[H + j + t] on the periods with H + j + t < 24, its rows past midnight are free on both sides
(Tracker._pass_market_dispatch on a short dispatch list), its wind window starts at hour 24 d + H + j, and its rounded first-period state
is step j + 1's.  The day-ahead step then runs on the projected state with every window at 24 (d + 1) - backcast day-ahead scenario i is
day d - i, real-time scenario i day d - 1 - i (day d is not a whole day of real-time prices when the RUC runs) - into PENDING buffers; at
the start of day d + 1 day_ahead() solves nothing and makes them current (activate_pending_DA_bids).  The hourly steps are unchanged,
including what their backcast knows - OURS: a Prescient-fed Backcaster would hold tomorrow's day-ahead prices after the RUC.
`_project_write` / `_project_hand_off` / `_activate` are the specification as tensor operations; csrc/dsp_project.hip (dsp_loop_project)
is the same arithmetic in one kernel per step.  proj_state / proj_real / proj_obj keep the last chain.

Self-scheduling (bidder="self_schedule"; the reference's run_double_loop_battery.py --participation_mode SelfSchedule, idaes'
SelfScheduler; our host restatement is workflow/bidder.py::SelfScheduler on workflow/coupling.py::CoupledScenarioModel): the plant offers
ONE schedule for all S price scenarios, day_ahead_power[s, t] == day_ahead_power[0, t].  The day-ahead step therefore solves ONE
coupled LP per plant - B rows of S * n1 columns, block i of row b being what row b * S + i of the LP bidder is, plus (S - 1) T static
coupling rows with bounds 0, 0 - with objective constant c0[b] = sum_i c0(b, i) added in the order of i.  The schedule of hour t is
block 0's day_ahead_power; the bid is the one pair (schedule, 0 $/MWh) through the same curve and clearing rules - (p_min, 0) in front,
integer cents where the reference rounds to 4 dp - so a price taker runs at its schedule when the price is >= 0 and at p_min otherwise.
Inside the cleared day every day_ahead_power column of the hourly problem is fixed to the cleared offer in all scenarios, the coupling
rows are vacuous and the coupled LP separates: the hourly step solves B real-time LPs, scenario 0 only, and bids (P_T[t], 0).  OURS:
in the last T_rt - 1 hours of a day the look-ahead periods past midnight have a free day_ahead_power which the host would still tie
across scenarios; this loop does not unless past_midnight="coupled" (__init__'s docstring; `_hour_step_past_midnight`).  `_day_ahead_step_self_schedule` / `_hour_step_bid` (the one hourly bidding step, here with
one row per plant and pairs priced at 0) are the specification as tensor operations; csrc/dsp_market.hip (dsp_loop_schedule_prepare; dsp_loop_market_prepare / _clear on an S = 1 state with
row_stride / self_schedule / curve_slots) is the same arithmetic, bit for bit.

Monotone bid curves (bidder="lp", scenario_coupling="monotone"; the reference's published double loops - wind + battery, nuclear - bid with
idaes' Bidder, n_scenario = 3 on a Backcaster; our host restatement is workflow/bidder.py::Bidder(scenario_coupling="monotone") on
workflow/coupling.py::CoupledScenarioModel): that bidder does not solve its price scenarios one by one, it orders every pair of them in
every period, (day_ahead_power[k, t] - day_ahead_power[j, t]) (price[k, t] - price[j, t]) >= 0.  Day-ahead: ONE coupled LP per plant - B rows
of S * n1 columns, the blocks of the self-schedule (same template col_scale, tiled) plus S (S - 1) / 2 * T static rows
pda[k, t] - pda[j, t], pair order CoupledScenarioModel.pairs (j < k, k fastest), row S * m1 + p * T + t.  Per day only the BOUNDS of
those rows change, with plant b's day-ahead scenario prices (the backcast index rule of the blocks' objective): d = da[k, t] - da[j, t],
rlo = 0 if d > 0 else -inf, rhi = 0 if d < 0 else +inf - CoupledScenarioModel.load.  Blocks, state, wind and c0[b] = sum_i c0(b, i) (in the
order of i) are the self-schedule's.  Bid: the S pairs of a plant and period are block i's day_ahead_power and scenario i's day-ahead
forecast, through the unchanged curve and clearing rules (integer cents, the p_min point, S + 1 slots); status and flags of plant b's ONE
solve stand for all its S pairs, `uncertified` counts a flagged plant once.  Real time: inside the cleared day every day_ahead_power
column is fixed to the same cleared offer in all scenarios, and the host's coupled real-time problem puts its rows on those columns: they
are vacuous there, so the hourly step is the stochastic mode's `_hour_step_bid` with B * S rows, unchanged.  OURS (the self-schedule's
third choice again): in the last T_rt - 1 hours of a day the look-ahead periods past midnight have a free day_ahead_power, which the host
would still order across scenarios; this loop does not unless past_midnight="coupled".  Not settled here: whether upstream idaes additionally orders the real-time power
output across scenarios - idaes is not available to this project; the loop follows this project's host Bidder.
`_day_ahead_step_monotone` (on `_coupled_blocks`, shared with the self-schedule) is the specification as tensor operations;
csrc/dsp_market.hip (dsp_loop_monotone_prepare; dsp_loop_market_clear on a state with coupled = 1) is the same arithmetic, bit for bit.

Recording (record=(plants, days); loop_record.py): what the reference's four result files per generator are made of - states, solutions,
curves, dispatches, delivered power - kept hour by hour for up to 64 plants in device buffers, by one gather launch per write
(dsp_loop_record) inside the captured steps, and written as those files through the host classes' own row builders (write_results).

Solve health (health=True): `bad` and `uncertified` say that SOME row of SOME plant failed or went uncertified; the health counters say
which plant, in which kind of solve (day-ahead, real-time, tracking, projection), from which hour on, and what the solves cost in
iterations - one launch per solve (dsp_loop_health, csrc/dsp_health.hip) inside the captured steps, over exactly the rows that feed the
two global flags.  `_health_book` is the specification as tensor operations; integers, so the two agree exactly.

Day profiles (profiles=days): the delivered power of EVERY plant, hour by hour, in `profile` [days + 1, 24, B] - what the reference's
market-surrogate workflow cuts into days, clusters into representative days and turns into each simulation's dispatch frequency
(representative_days.py).  One launch per hour step after the hand-off (dsp_loop_profile, csrc/dsp_days.hip) inside the captured step;
`_profile_write_tensors` is the specification as tensor operations, a copy, so the two agree bit for bit."""
from __future__ import annotations

import numpy as np

from . import scenarios
from ._device_loop import _DeviceLoop, _NoSolver, attach_solver


def exact_fma(torch, a, b, c):
    """round(a * b + c) with ONE rounding, as tensor operations (float64; no overflow / underflow in a * b): the fused multiply-add of
    the kernels, which torch does not offer.  Boldo & Melquiond, "Emulation of a FMA and correctly rounded sums: proved algorithms using
    rounding to odd" (IEEE TC 2008), algorithm Fma-emul: a * b = uh + ul exactly (Dekker's product on Veltkamp splits, as
    bid_curves.cents), (th, tl) = TwoSum(c, ul), (vh, vl) = TwoSum(uh, th), z = tl + vl rounded TO ODD, result = vh + z."""
    def split(v):
        t = v * 134217729.0                            # 2^27 + 1
        hi = t - (t - v)
        return hi, v - hi

    def two_sum(x, y):
        s = x + y
        yy = s - x
        return s, (x - (s - yy)) + (y - yy)
    uh = a * b
    (ah, al), (bh, bl) = split(a), split(b)
    ul = al * bl - (((uh - ah * bh) - al * bh) - ah * bl)
    th, tl = two_sum(c, ul)
    vh, vl = two_sum(uh, th)
    z, err = two_sum(tl, vl)
    # to odd: an inexact sum whose last mantissa bit is even moves one ulp towards the lost part (integer step on the bit pattern)
    bits = z.view(torch.int64)
    step = torch.where((err > 0) == (z > 0), torch.ones_like(bits), -torch.ones_like(bits))
    z = torch.where((err != 0) & ((bits & 1) == 0), bits + step, bits).view(torch.float64)
    return vh + z


def _dense_rows(block, family, n, hours):
    ex = block.expressions[family]
    return np.stack([ex[t].dense(n) for t in hours]), np.array([ex[t].const for t in hours])


class _Model:
    """One of the three LPs on the device, described without reference to a flowsheet."""

    def __init__(self, model, block_family, B, dev, device_index, power_output, state_init, wind, lp_backend=None, solved=True, simplex_certify=False):
        import torch
        self.lp = model.lp
        self.T = len(model.HOUR)
        n = self.lp.n
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), device=dev)
        idx = lambda cols: torch.as_tensor(np.asarray(cols, np.int64), device=dev)
        lb, ub, rlo, rhi = model.block.current_bounds()
        base_c = model.base_c if hasattr(model, "base_c") else model.c[0]
        self.base_c = t(base_c)
        self.base_c0 = float(model.base_c0) if hasattr(model, "base_c0") else float(np.asarray(model.c0).ravel()[0])
        self.c = self.base_c.repeat(B, 1)
        self.c0 = torch.full((B,), self.base_c0, dtype=torch.float64, device=dev)
        self.lb, self.ub = t(lb).repeat(B, 1), t(ub).repeat(B, 1)
        self.rlo, self.rhi = t(rlo).repeat(B, 1), t(rhi).repeat(B, 1)
        PT, PT_const = _dense_rows(model.block, power_output, n, model.HOUR)
        self.PT, self.PT_const = t(PT), t(PT_const)                       # [T, n], [T]
        self.state_init = [int(c) for c in state_init]                    # columns fixed to the realised state
        self.pda_cols = self.track_rows = self.state_real = None          # day-ahead power columns (bidding models); dispatch rows, state after period 0 (trackers)
        self.c_static = None                                              # [rows, n] per-row cost vector without prices where plants differ in it (nuclear h2_price), else base_c
        self.kw_plant = self.c0_plant = None                              # per-plant sizes: wind kW [B, 1], objective constant [B] (set_plant_sizes)
        self.per_plant = None                                             # rows per plant of a bidding model (None: the loop's S)
        self.wind = None
        if wind is not None:                                              # (columns, kW, curtailment cost per kW, template availability sum)
            cols, kw, per_kw, template_sum = wind
            self.wind = (idx(cols), float(kw), float(per_kw))
            self.base_c0 -= float(per_kw) * float(template_sum)           # the template's curtailment constant leaves; the window's enters
        attach_solver(self, B, dev, device_index, getattr(model, "solver_hints", None), lp_backend, solved, simplex_certify)      # (solved=False: parametrized mode never solves its bidding templates)

    def couple(self, model, S, B, dev, device_index, lp_backend, mode="non_anticipative", simplex_certify=False):
        """-> the COUPLED day-ahead model of a batch built on this one-row block model (of `model`, the day-ahead template): B rows of
        the LP of CoupledScenarioModel(model, mode) - S blocks of this LP side by side and its coupling rows from row
        `first_coupling_row` = S * m1 on.  mode "non_anticipative" (a self-schedule): (S - 1) T rows pda[s, t] - pda[0, t] with bounds
        0, 0 written here, once, like the blocks' static bounds.  mode "monotone" (the Bidder's ordered curve): S (S - 1) / 2 * T rows
        pda[k, t] - pda[j, t] over `pairs` (j < k, k fastest), free here - the day-ahead step writes their bounds every day, from the
        order of the day's scenario prices.  Afterwards THIS model is the [B * S, n1] view of the coupled rows' c / lb / ub (block i
        of row b = its row b * S + i), which _set_rows writes; its c0 [B * S] holds the scenario constants that the coupled c0 sums."""
        import types
        import torch
        from .workflow.coupling import CoupledScenarioModel
        shim = types.SimpleNamespace(lp=model.lp, n_scenario=S, HOUR=model.HOUR, pda_cols=model.pda_cols, block=model.block,
                                     solver_hints=getattr(model, "solver_hints", None))
        coupled = CoupledScenarioModel(shim, mode)
        cm = _Model.__new__(_Model)
        cm.__dict__.update(self.__dict__)                                 # block data: base_c, PT, state / wind / day-ahead columns (block-relative)
        cm.lp, cm.S, cm.n1 = coupled.lp, S, self.lp.n
        cm.pairs, cm.first_coupling_row = coupled.pairs, S * self.lp.m
        if getattr(self.lp, "col_scale", None) is not None:               # the blocks keep the template's column scaling (DeviceLP reads it):
            cm.lp.col_scale = np.tile(np.asarray(self.lp.col_scale, np.float64), S)      # wind + battery columns span 200 .. 1e9
        n1, m1, Tc = self.lp.n, self.lp.m, len(coupled.pairs) * self.T
        cm.c = self.base_c.repeat(S).repeat(B, 1)
        cm.c0 = torch.zeros(B, dtype=torch.float64, device=dev)
        cm.lb, cm.ub = self.lb[0].repeat(S).repeat(B, 1), self.ub[0].repeat(S).repeat(B, 1)
        side = lambda v: torch.full((Tc,), 0.0 if mode == "non_anticipative" else v, dtype=torch.float64, device=dev)
        cm.rlo = torch.cat([self.rlo[0, :m1].repeat(S), side(float("-inf"))]).repeat(B, 1)
        cm.rhi = torch.cat([self.rhi[0, :m1].repeat(S), side(float("inf"))]).repeat(B, 1)
        attach_solver(cm, B, dev, device_index, coupled.solver_hints, lp_backend, True, simplex_certify)      # (a day-ahead horizon: a T > 16 model's options; the hourly coupled model of past_midnight="coupled": a T <= 16 model's)
        self.c,self.lb, self.ub = (v.view(B * S, n1) for v in (cm.c, cm.lb, cm.ub))
        self.c0 = torch.zeros(B * S, dtype=torch.float64, device=dev)
        return cm

    def power_output(self, x):
        return x @ self.PT.T + self.PT_const                              # [B, T] MW

    def set_plant_sizes(self, wind_kw, c0_base, dev):
        """wind_kw, c0_base: float64 arrays [B] per PLANT, computed once on the host - the tensor form and the kernels read these very
        arrays instead of the scalars wind[1] / base_c0"""
        import torch
        self.kw_plant = torch.as_tensor(np.ascontiguousarray(wind_kw, np.float64), device=dev)[:, None]
        self.c0_plant = torch.as_tensor(np.ascontiguousarray(c0_base, np.float64), device=dev)

    def kw(self):
        """the wind size as the window's factor: the scalar, or [B, 1] per plant"""
        return self.wind[1] if self.kw_plant is None else self.kw_plant

    def terms(self):
        """P_T[t] = (x[a] ca + x[b] cb) + const_t as index / coefficient arrays [T, 2] (-1 / 0.0: no such term): the
        elementwise form of the power output, the one the kernels compute and the descriptors carry"""
        PT = self.PT.cpu().numpy()
        cols, coef = np.full((self.T, 2), -1, np.int64), np.zeros((self.T, 2))
        for t in range(self.T):
            nz = np.nonzero(PT[t])[0]
            if len(nz) > 2:
                raise ValueError("the kernels take power outputs of at most two columns per period")
            cols[t, :len(nz)], coef[t, :len(nz)] = nz, PT[t, nz]
        return cols, coef

    def set_first_period_terms(self, dev):
        """P_T[0] as phase 2 of dsp_loop_update reads it, for the exact form of the hand-off (BatchedDoubleLoop._hand_off)"""
        import torch
        cols, coef = self.terms()
        used = cols[0] >= 0
        self.p0_cols = torch.as_tensor(cols[0][used], dtype=torch.int64, device=dev)
        self.p0_coef = torch.as_tensor(coef[0][used], dtype=torch.float64, device=dev)

    def set_terms(self, dev):
        import torch
        cols, coef = self.terms()
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
        used = cols >= 0
        self.term_cols, self.term_coef = t(cols[used], torch.int64), t(coef[used], torch.float64)      # the objective entries the prices touch
        self.term_t = t(np.nonzero(used)[0], torch.int64)
        self.pt_a, self.pt_b = t(np.maximum(cols[:, 0], 0), torch.int64), t(np.maximum(cols[:, 1], 0), torch.int64)
        self.pt_ca, self.pt_cb = t(coef[:, 0], torch.float64), t(coef[:, 1], torch.float64)
        self.has_const = bool((self.PT_const != 0).any().item())
        self.base_c0_t = torch.full((), self.base_c0, dtype=torch.float64, device=dev)
        return cols

    def solve(self, B, hour=None):
        opts = self.opts if (hour is None or self.opts is None) else (self.opts_first if hour == 0 else self.opts_warm)
        self.out = self.dlp.solve(B, self.c, self.lb, self.ub, self.rlo if self.lp.m else None, self.rhi if self.lp.m else None,
                                  options=opts, out=self.out, sync_stats=False, obj_offset=self.c0)
        return self.out


def _per_plant(v, name, B, positive=False, below=None):
    """a scalar or an array [B], finite, >= 0 (positive: > 0) and, if given, below `below` -> float64 array [B]"""
    a = np.asarray(v, np.float64)
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
        raise ValueError(f"{name} is a scalar or an array of length {B}, not of shape {a.shape}")
    if not np.isfinite(a).all() or ((a <= 0).any() if positive else (a < 0).any()) or (below is not None and (a >= below).any()):
        raise ValueError(f"{name} must be finite, {'> 0' if positive else '>= 0'}" + ("" if below is None else f" and below {below:.0e}".replace("e+0", "e")))
    return np.broadcast_to(a, (B,)).copy()


def _describe(cls, m, n_state):
    """-> the descriptor `cls()` - DspLoopModel or DspLoopMarketModel (hip_solver.py) - of a _Model.  What the two share: buffers, sizes,
    the two-term power output (_Model.terms), day-ahead power / wind / state columns, the wind size and the objective constants, per
    plant where the model carries them (None: the pointers stay NULL, the kernels read the scalars).  What only a DspLoopModel has:
    rows, dispatch rows, the state after period 0.  Entries past the horizon are -1 / 0."""
    w = cls()
    w.c, w.lb, w.ub, w.base_c, w.x, w.c0 = (t.data_ptr() for t in (m.c, m.lb, m.ub, m.base_c, m.out["x"], m.c0))
    w.status, w.flags = m.out["status"].data_ptr(), m.out["flags"].data_ptr()
    w.n, w.T, w.n_state = getattr(m, "n1", m.lp.n), m.T, n_state      # (a coupled model is described by ONE of its blocks)
    cols, coef = m.terms()
    PTc = m.PT_const.cpu().numpy()
    pda = m.pda_cols.cpu().tolist() if m.pda_cols is not None else []
    wind = m.wind[0].cpu().tolist() if m.wind is not None else []
    for t in range(len(w.pda_cols)):
        live = t < m.T
        for e in range(2):
            w.pt_cols[t][e] = int(cols[t, e]) if live else -1
            w.pt_coef[t][e] = float(coef[t, e]) if live else 0.0
        w.pt_const[t] = float(PTc[t]) if live else 0.0
        w.pda_cols[t] = int(pda[t]) if t < len(pda) else -1
        w.wind_cols[t] = int(wind[t]) if t < len(wind) else -1
    for j in range(len(w.state_init)):
        w.state_init[j] = m.state_init[j] if j < len(m.state_init) else 0
    w.wind_kw, w.waste_per_kw = (m.wind[1], m.wind[2]) if m.wind is not None else (0.0, 0.0)
    w.c0_base = m.base_c0
    if m.kw_plant is not None:
        w.wind_kw_plant, w.c0_base_plant = m.kw_plant.data_ptr(), m.c0_plant.data_ptr()
    if hasattr(w, "track_rows"):
        w.rlo, w.rhi, w.m = m.rlo.data_ptr(), m.rhi.data_ptr(), m.lp.m
        track = m.track_rows.cpu().tolist() if m.track_rows is not None else []
        for t in range(len(w.track_rows)):
            w.track_rows[t] = int(track[t]) if t < len(track) else -1
        for j in range(len(w.state_real)):
            w.state_real[j] = m.state_real[j] if m.state_real is not None and j < len(m.state_real) else 0
    return w


LEDGER_MAX_FORMS = LEDGER_MAX_TERMS = 8                # DSP_LEDGER_MAX_FORMS / DSP_LEDGER_MAX_TERMS of include/dsp_hip.h


def _ledger_expression(block, n, d, family, scale, per_avail):
    """family[0] * scale of a populated block as (row [n], constant, per_avail * scale), the capacity-factor constant per_avail *
    (the block's wind_kw * the series' cf[0], what every template and model object is built on) taken out of the constant.  The ONE
    statement of a ledger constant: the template's (_ledger_forms) and every sized plant's (_ledger_setup)."""
    rows, const = _dense_rows(block, family, n, [0])
    row, const = rows[0], float(const[0])
    if per_avail:
        fam = getattr(block, d["family"])
        wind = fam["periods"][0]["wind"].index
        if row[wind] != -per_avail:
            raise RuntimeError(f"{family}[0] carries the wind column with {row[wind]!r}, not with minus its curtailment weight {per_avail!r}")
        const -= per_avail * float(fam["wind_kw"] * d["prices"][2][0])
    return row * scale, const * scale, per_avail * scale


def _ledger_wind_expressions(d):
    """key -> (expression family, scale, per_avail) of the two forms whose constant carries the capacity factor and the wind size"""
    per_kw, to_mwh = d["waste"]
    return {"tot_cost": ("tot_cost", 1.0, d["per_kw"]), "curtailed_mwh": ("wind_waste", to_mwh, per_kw)}


def _ledger_forms(flowsheet, tr_model, d, with_h2_kg=True):
    """The ledger of the implemented hour as linear forms over the TRACKER's period 0, taken from the host model's own expressions by the
    route P_T takes (_dense_rows) -> list of (key, row [n], constant, per_avail).  A form's value is row . x + constant + per_avail *
    avail0, avail0 = wind_kw * cf of the hour; `constant` is the expression's constant with the TEMPLATE's capacity-factor share taken
    out (as _Model.__init__ does for c0): the window's enters at run time.
        tot_cost        tot_cost[0] as the flowsheet defines it (nuclear: the hydrogen credit included)
        under_mwh, over_mwh     the tracker's power_underdelivered[0] / power_overdelivered[0]
        curtailed_mwh   wind_waste[0] in MWh (wind + PEM states it in kW)
        h2_kg           wind + PEM: MultiPeriodWindPEM._h2_kg_per_hr(pem_elec[0]); nuclear: outlet_to_pipeline[0] * mw_h2 * 3600
                        (with_h2_kg=False: the parametrized wind + PEM loop, which books it in a kernel phase of its own)
        pem_mwh         PEM electricity of the hour
        h2_revenue      nuclear: h2_kg * h2_price, the share of tot_cost that is revenue"""
    from .flowsheets import parameters as prm
    block, n = tr_model.block, tr_model.lp.n
    fam = getattr(block, d["family"])
    p0 = fam["periods"][0]

    def unit(var, coef=1.0):
        row = np.zeros(n)
        row[var.index] = coef
        return row

    windy = d.get("waste") is not None
    expression = lambda key: _ledger_expression(block, n, d, *(_ledger_wind_expressions(d)[key] if windy else ("tot_cost", 1.0, 0.0)))
    forms = [("tot_cost",) + expression("tot_cost"),
             ("under_mwh", unit(tr_model.power_underdelivered[0]), 0.0, 0.0), ("over_mwh", unit(tr_model.power_overdelivered[0]), 0.0, 0.0)]
    if windy:
        forms.append(("curtailed_mwh",) + expression("curtailed_mwh"))
    if flowsheet == "wind_pem":
        if with_h2_kg:
            forms.append(("h2_kg", unit(p0["pem_elec"], prm.pem_electricity_to_mol / prm.h2_mols_per_kg * 3600), 0.0, 0.0))
        forms.append(("pem_mwh", unit(p0["pem_elec"], 1e-3), 0.0, 0.0))
    if flowsheet == "nuclear":
        h2_kg = prm.mw_h2 * 3600
        credit = -float(block.expressions["tot_cost"][0].coef[p0["outlet_to_pipeline"].index])      # mw_h2 * 3600 * h2_price, as tot_cost carries it
        forms += [("h2_kg", unit(p0["outlet_to_pipeline"], h2_kg), 0.0, 0.0), ("pem_mwh", unit(p0["pem_elec"], 1e-3), 0.0, 0.0),
                  ("h2_revenue", unit(p0["outlet_to_pipeline"], credit), 0.0, 0.0)]
    return forms


def _describe_ledger(L):
    """-> the DspLoopLedgerDesc (hip_solver.py) of a loop's ledger L (BatchedDoubleLoop._ledger_setup); its columns are the tracker's"""
    from .hip_solver import DspLoopLedgerDesc
    g = DspLoopLedgerDesc()
    g.n_forms = len(L["keys"])
    for f, cols in enumerate(L["cols"]):
        g.n_terms[f] = len(cols)
        for e, col in enumerate(cols):
            g.cols[f][e] = col
        g.per_avail[f] = L["per_avail"][f]
    g.coef, g.constant = L["coef"].data_ptr(), L["const"].data_ptr()
    g.coef_stride = L["coef"].stride(0) if L["coef"].dim() == 3 else 0          # [B, F, 8] per plant, [F, 8] shared
    g.const_stride = L["const"].stride(0) if L["const"].dim() == 2 else 0       # [B, F] per plant, [F] shared
    g.acc, g.hour_value = L["acc"].data_ptr(), L["hour"].data_ptr()
    return g


_WIND_BATTERY_SIZES = dict(wind_mw=200.0, battery_mw=25.0, battery_mwh=100.0)      # the plant of the reference's wind + battery double loop


def _templates(flowsheet, day_ahead_horizon, tracking_horizon, sizes=None):
    """(bidder, day-ahead model, real-time model, tracker, descriptor) built ONCE through the product's own model objects (B = 1).
    sizes: dict(wind_mw, battery_mw, battery_mwh) [wind_pem: wind_mw] of the template plant, None = the flowsheet's default plant."""
    from .workflow import Tracker
    if flowsheet == "wind_battery":
        series, stride, cap = "rts_gmlc_309.npz", 17, 500.0
        z = _WIND_BATTERY_SIZES if sizes is None else sizes
        bidder, da = scenarios.wind_battery_batch(1, day_ahead_horizon, _NoSolver(), series=series, stride=stride, wind_mw=z["wind_mw"],
                                                  batt_mw=z["battery_mw"], batt_mwh=z["battery_mwh"])
        s = scenarios.load_series(series)
        mo = bidder.bidding_model_object
        tr_obj = mo.__class__(model_data=mo.model_data, wind_capacity_factors=list(s["rt_cf"][:tracking_horizon]), wind_pmax_mw=z["wind_mw"],
                              battery_pmax_mw=z["battery_mw"], battery_energy_capacity_mwh=z["battery_mwh"])
        fam = "windBattery"
        desc = dict(family=fam, per_kw=mo.wind_waste_penalty * 1e-3, decimals=[2, 2],
                    init=lambda blk: [getattr(blk, fam)["soc_init"].index, getattr(blk, fam)["thr_init"].index],
                    real=lambda blk: [getattr(blk, fam)["periods"][0]["state_of_charge"].index, getattr(blk, fam)["periods"][0]["energy_throughput"].index])
        prices = (np.clip(s["da_lmp"], 0.0, cap), np.clip(s["rt_lmp"], 0.0, cap), s["rt_cf"])
        desc["da_cf"] = s["da_cf"]
        desc["waste"] = (1e-3, 1.0)                  # wind_waste[t] = 1e-3 (available kW - wind): MW, the ledger's MWh of an hour as it stands
    elif flowsheet == "wind_pem":
        series, stride, cap = "rts_gmlc_303.npz", 37, 500.0
        bidder, da = scenarios.wind_pem_batch(1, day_ahead_horizon, _NoSolver(), series=series, stride=stride,
                                              **({} if sizes is None else dict(wind_mw=sizes["wind_mw"])))
        s = scenarios.load_series(series)
        mo = bidder.bidding_model_object
        tr_obj = mo.__class__(mo.model_data, wind_capacity_factors=list(s["rt_cf"][:tracking_horizon]), wind_pmax_mw=mo._wind_pmax_mw,
                              pem_pmax_mw=mo._pem_pmax_mw)
        fam = "windPEM"
        desc = dict(family=fam, per_kw=1.0, decimals=[], init=lambda blk: [], real=lambda blk: [], da_cf=s["da_cf"],
                    waste=(1.0, 1e-3))               # wind_waste[t] = available kW - wind, in kW: 1e-3 of it is the ledger's MWh of an hour
        prices = (np.clip(s["da_lmp"], 0.0, cap), np.clip(s["rt_lmp"], 0.0, cap), s["rt_cf"])
    elif flowsheet == "nuclear":
        stride = 29
        bidder, da = scenarios.nuclear_batch(1, day_ahead_horizon, _NoSolver(), **(sizes or {}))      # sizes: pem_mw, tank_kg, h2_price, h2_demand
        s = scenarios.load_series("nuclear_price_taker_lmps.npz")        # bus Attlee, generator 121_NUCLEAR_1 (rts_gmlc_15_500.csv)
        tr_obj = bidder.bidding_model_object.__class__(bidder.bidding_model_object.model_data, **(sizes or {}))
        fam = "nuclear"
        desc = dict(family=fam, per_kw=None, decimals=[0],
                    init=lambda blk: [blk.nuclear["holdup_init"].index], real=lambda blk: [blk.nuclear["periods"][0]["tank_holdup"].index])
        prices = (np.clip(s["da_lmp"], 0.0, None), np.clip(s["rt_lmp"], 0.0, None), None)
    else:
        raise ValueError(f"unknown flowsheet {flowsheet!r}: wind_battery, wind_pem or nuclear")
    tracker = Tracker(tracking_model_object=tr_obj, tracking_horizon=tracking_horizon, n_tracking_hour=1, solver=_NoSolver())
    tracker._pass_market_dispatch([0.0] * tracking_horizon)              # dispatch rows become equalities
    desc.update(stride=stride, prices=prices)
    return bidder, da, bidder.real_time_model, tracker, desc


_default_rows_cache = {}


def _default_kept_rows(flowsheet, day_ahead_horizon, tracking_horizon):
    """names of the rows presolve keeps in the three LPs of the DEFAULT plant (built once per shape)"""
    key = (flowsheet, int(day_ahead_horizon), int(tracking_horizon))
    if key not in _default_rows_cache:
        _, da, rt, tracker, _ = _templates(*key)
        _default_rows_cache[key] = tuple(tuple(m.lp.row_names) for m in (da, rt, tracker.model))
    return _default_rows_cache[key]


def _check_template(flowsheet, day_ahead_horizon, tracking_horizon, models):
    """Soundness of ONE template for a batch of different plants.  Presolve, the hulls and the implied-range column scaling belong to
    the handle, not to the plant.  The template is built at the batch's LARGEST sizes: every size-dependent bound of a plant (wind and
    battery column upper bounds, the right-hand side of state_of_charge_bounds, all with lower side 0 / -inf) lies inside the template's,
    which presolve takes as the hull - so a row it proved never binding for the template never binds for a smaller plant either.
    (The argument rests on that ONE-SIDEDNESS: a size-dependent bound whose other side moved with the size - a minimum load, say -
    would make a smaller plant's box stick out of the template's, and would need a declared hull instead.)
    What remains to be shown is that it did not KEEP or DROP anything else than for the default plant (whose LP shape the kernels and the
    tests are validated on): the kept rows must be the default plant's, name by name.  An energy capacity beyond the 1e8 kWh ramp
    bound, for instance, keeps the 48 energy-ramp rows; a battery of 0 MW lets presolve drop rows a battery needs."""
    want = _default_kept_rows(flowsheet, day_ahead_horizon, tracking_horizon)
    for name, m, rows in zip(("day-ahead", "real-time", "tracking"), models, want):
        got = tuple(m.lp.row_names)
        if got != rows:
            diff = sorted(set(got) ^ set(rows))
            raise ValueError(f"the sizes of this batch leave the range for which one LP template is sound: presolve keeps {len(got)} rows of the "
                             f"{name} LP at the batch's largest sizes, {len(rows)} for the default plant (kept rows differ in {diff[:4]}"
                             f"{' ...' if len(diff) > 4 else ''})" +
                             ("; battery_mwh * 1e3 may be at most the 1e8 kWh energy-ramp bound and the batch's largest battery_mw must be above 0"
                              if flowsheet == "wind_battery" else ""))


def _objective_constant(model_object, horizon, weighted_family, per_kw, cf):
    """base_c0 of a template built on `model_object`, in the arithmetic that builds it: the constants of tot_cost[t] * weight added in
    the order of t (Bidder._refresh_cost_objective / Tracker._refresh_objective; the penalty terms carry no constant), less the
    template's curtailment constant per_kw * (wind_kw * sum cf[:T]) (_Model.__init__).  Bit for bit the template's own value."""
    from .lp import LinearBlock
    block = LinearBlock("fs")
    model_object.populate_model(block, horizon)
    name, weight = weighted_family
    const = 0.0
    for t in range(horizon):
        const += block.expressions[name][t].const * float(weight)
    fam = getattr(block, "windBattery", None) or getattr(block, "windPEM")
    return float(const) - float(per_kw) * float(fam["wind_kw"] * float(np.sum(cf[:horizon])))


class BatchedDoubleLoop(_DeviceLoop):
    past_midnight = "free"                             # (class default: the loop sets the attribute only where it is "coupled")

    def __init__(self, flowsheet, n_scenarios, device=0, first_scenario=0, day_ahead_horizon=48, tracking_horizon=4, lp_backend=None,
                 use_graphs=True, use_fused=True, simplex_warm=True, n_price_scenarios=1, forecaster="perfect", max_historical_days=10,
                 market="stub", bidder="lp", bid_price=None, storage_mw=None, plant_windows=None, wind_mw=None, battery_mw=None,
                 battery_mwh=None, ruc_hour=None, scenario_coupling="independent", ledger=False, pem_mw=None, tank_kg=None,
                 h2_price=None, h2_demand=None, record=None, record_max_bytes=2 ** 30, simplex_certify=False, health=False,
                 profiles=None, profile_max_bytes=2 ** 30, past_midnight="free"):
        """flowsheet: "wind_battery", "wind_pem" or "nuclear".  Plant k sees the year that starts at hour (stride * k) mod N of its bus's
        series (strides 17 / 37 / 29).  lp_backend: tests pass tests/_highs_solver.py::HighsTensorLP to run the same logic on CPU tensors.
        use_fused: on the GPU the ~100 element-wise tensor operations of an hour step are THREE launches of one HIP kernel driven by the
        descriptor (dsp_loop_update, include/dsp_hip.h) - the nuclear loop of 256 plants is launch-bound otherwise (21 ms per simulated day).
        n_price_scenarios, forecaster, max_historical_days, market: the STOCHASTIC mode, with the meaning and the validation of
        BatchedWindBatteryDoubleLoop (rolling.py): forecaster="backcast" bids on S scenarios out of the D last days of the
        plant's own circular series, market="price_taker" dispatches along the bid curve at the price that occurs ("stub": at its last
        point).  The curves start at the generator's p_min.  The defaults are the deterministic loop, unchanged.
        plant_windows: int array [B]; plant b sees the year that starts at hour (stride * (first_scenario + plant_windows[b])) mod N
        (None: arange(B)), so that several plants - parameter points of a sweep - can share one window.
        bidder="parametrized" (wind_pem, wind_battery; perfect forecaster, one scenario, tracking_horizon <= 16), bid_price [$/MWh] and
        storage_mw [MW of PEM / battery the upper tier covers], scalars or arrays [B]: the two-tier closed-form curves of the
        reference's parametrized bidders instead of bidding LPs (module docstring); market "price_taker" or "stub".
        wind_mw, battery_mw [MW], battery_mwh [MWh], scalars or arrays [B] (bidder="lp"): the SIZE of every plant, so that a design
        sweep is one batch (sweeps.design_sweep).  "wind_battery" takes all three; what is left None keeps the default plant's 200 MW
        of wind and 25 MW / 100 MWh of battery, except that battery_mw without battery_mwh means the flowsheet's own default of four
        hours, 4 * battery_mw.  "wind_pem" takes wind_mw only (default 847 MW): in the reference's LP, and in this one, the PEM capacity
        is a free column that the bidding LP chooses - it is not a design parameter of the LP bidder (bidder="parametrized" has
        storage_mw for it).  Refused (ValueError): sizes for "nuclear" or for bidder="parametrized", battery sizes for "wind_pem", a
        wrong array length, non-finite values, wind_mw <= 0, negative battery sizes, wind_mw + battery_mw >= 2e7 (the cent arithmetic
        of the curves), and a batch whose largest sizes change what presolve keeps (_check_template).  With all three None the loop is
        the default one, unchanged: same templates, descriptors with NULL per-plant pointers, same launches.
        ruc_hour: None (the loop above: the day-ahead bid of day d is made at hour 0 of day d, same launches, same bits) or an integer
        H, 1 <= H <= 23: the reference's timeline (module docstring, "Bidding at the RUC hour").  Explicit, no default of ours: the
        reference's drivers leave Prescient's ruc_execution_hour at Prescient's own default, 16.  Refused (ValueError): a value that
        is not an integer of 1 .. 23, bidder="parametrized" (no bidding LP and no state in the bid: nothing to project), and
        forecaster="backcast" with 24 (max_historical_days + 1) hours more than the series holds.
        bidder="self_schedule" (all three flowsheets; n_price_scenarios = S, forecaster, max_historical_days, market, plant_windows and
        the horizons with the stochastic mode's meaning and validation; S = 1 on the perfect forecaster works and has no coupling rows):
        the reference's SelfSchedule participation mode (module docstring, "Self-scheduling").  ONE day-ahead schedule per plant for all
        S price scenarios, from one coupled LP per plant (self.da: B rows of S * n1 columns; self.da_block is its [B * S, n1] view);
        the schedule is offered at cost 0, so da_curve / da_count keep the stochastic mode's shapes (S + 1 slots) with one or two points
        used, prices 0, p_min in front; powers are integer cents where the reference rounds to 4 dp.  The hourly steps solve B real-time
        LPs on scenario 0.  results() has the stochastic mode's keys.  The hourly steps replay from graphs; so does the day-ahead step
        where the coupled LP stays in the fused kernels (nuclear, wind + PEM) - a coupled LP that the solver streams (wind + battery)
        is solved from the host and its step stays eager (day_ahead()).  Refused (ValueError): ruc_hour, per-plant sizes (wind_mw,
        battery_mw, battery_mwh), bid_price / storage_mw.
        scenario_coupling: "independent" (the default: the loops above, bit for bit - the LP bidder solves its B * S scenario LPs one by
        one and the running maximum of the curve repairs their order) or "monotone" (bidder="lp", forecaster="backcast",
        n_price_scenarios = S >= 2; all three flowsheets, both markets): the reference's stochastic Bidder (module docstring, "Monotone
        bid curves").  ONE coupled day-ahead LP per plant (self.da: B rows of S * n1 columns, S (S - 1) / 2 * T ordered-pair rows whose
        bounds follow the day's scenario prices; self.da_block is its [B * S, n1] view); the S pairs of a plant-hour are block i's
        day_ahead_power and scenario i's forecast, through the unchanged curve and clearing rules; status and flags of the plant's one
        solve stand for its S pairs and `uncertified` counts a flagged plant once.  The hourly steps, results() and reset() are the
        stochastic mode's.  The day-ahead step replays from a graph where the coupled LP stays in the fused kernels, as the
        self-schedule's.  Refused (ValueError): another value, bidder other than "lp", ruc_hour, per-plant sizes, bid_price /
        storage_mw, forecaster="perfect", n_price_scenarios=1 (no pairs: that is the independent loop).
        simplex_certify: False (the loops above: same launches, same bits) or True: every model of at most 16 periods - the real-time
        model, the tracker, the projection tracker - is solved under dsp_options::simplex_certify = 1, also in its first-hour / warm
        option copies: the in-wave simplex stores an optimum only after the stored (x, y) passed the KKT certificate against the
        original LP (primal, dual_col, dual_row, gap <= 1e-9; include/dsp_hip.h) and flags it DSP_FLAG_SIMPLEX_KKT; a vertex it
        rejects is solved by the PDLP pass of the same call, whose status and flags feed `bad` / `uncertified` as ever.  No kernel of
        the loop changes; each such model's out["kkt"] [rows, 4] holds the last solve's certificates.
        ledger: False (the loops above: same launches, same bits) or True: every implemented hour is BOOKED per plant, after the tracking
        solve and before the hand-off, from the tracker's solution of its period 0 - tot_cost [$] (the flowsheet's own tot_cost[0], its
        constant at this hour's capacity factor and this plant's wind size; nuclear: the hydrogen credit included), under_mwh / over_mwh
        (the tracker's missed delivery), curtailed_mwh (wind flowsheets), h2_kg and pem_mwh (wind + PEM, nuclear), h2_revenue [$]
        (nuclear); _ledger_forms.  Works in every mode (each ends an hour with a tracking solve and a hand-off); the projection
        tracker's chain of ruc_hour is not booked, those hours are not implemented.  results() gains these keys and profit = obj -
        tot_cost; ledger_keys names the rows of ledger_acc / ledger_hour [F, B] (running sums / the last hour's values); reset()
        zeroes both.  With bidder="parametrized" on wind + PEM h2_kg stays the existing accumulator, the ledger adds no second one.
        Arithmetic (the kernel's, dsp_loop_ledger, and bit for bit the tensor form's, _ledger_book): constant, then one fma per term in
        the form's order, then one fma with the hour's available wind, then a plain add into the accumulator.  Refused (ValueError): a
        form of more than 8 terms, more than 8 forms.
        pem_mw [MW], tank_kg [kg], h2_price [$/kg], h2_demand [kg/s] ("nuclear" only; scalars or arrays [B]; what is left None keeps the
        flowsheet's 100 MW, parameters.tank_capacity_kg, 4 $/kg, 0.35 kg/s; all None = the loop above, bit for bit): every plant's
        own PEM, tank and hydrogen market, so that the reference's (h2 price x PEM size) study is one batch (sweeps.nuclear_sweep).
        None is a matrix coefficient: pem_mw is the upper bound of the np_to_pem columns, tank_kg of the holdup columns, h2_demand of
        the pipeline columns, h2_price the objective entry of the pipeline columns - all static, written once per row of every model
        (the projection tracker included) - and h2_price the per-plant coefficient of the ledger's tot_cost / h2_revenue.  One
        template at the batch's largest values (_check_template).  The bid curves start at the plant's own p_min = p_max - pem_mw
        (the notebook: 500 - 100 = 400), so a larger PEM can offer below 400 MW (dsp_loop_market_state::p_min_cents_plant); p_max
        stays 500.  They combine with plant_windows, n_price_scenarios, forecaster, market, ruc_hour, graphs and ledger.  Refused
        (ValueError): another flowsheet, bidder="self_schedule" / "parametrized", scenario_coupling="monotone", a wrong length,
        non-finite or negative values, pem_mw outside (0, 500].
        record: None (the loops above: same launches, same bits) or (plants, days): keep, for up to 64 plants of the batch (strictly
        increasing indices) and `days` simulated days, what the reference's four result files per generator are made of, in device
        buffers [hours or days (+ 1 spare row), plants, ...] (loop_record.py).  Per day, in the row of the day the bid is FOR (a bid made
        at the RUC hour of day d: row d + 1): da_state (the state the bid was built on; ruc_hour: the projected one), da_x [S, n] (a
        plant's S rows, or the S blocks of its one coupled row), da_obj / da_c0 / da_status / da_iters (per row of the batch), da_curve /
        da_count (modes with curves), da_offer / da_prices (of a pending bid: the pending buffers).  Per hour, after the tracking solve
        and the ledger and before the hand-off: state (the state the hour's LPs were built from), rt_x [per, n] / rt_obj / rt_c0 /
        rt_status (per = S, 1 for a self-schedule), rt_curve / rt_count / rt_dispatch, tr_x / tr_obj / tr_c0 / tr_status, ledger_hour
        [F] with ledger=True; after the hand-off: delivered.  bidder="parametrized" has no bidding LP: curves, offers and the tracker
        only.  The projection tracker's chain of ruc_hour is not recorded (the reference writes no files for it; it ends on da_state).
        Each of the three writes is one launch of dsp_loop_record inside the step, so the captured graphs stay as many and replay the
        record; hours and days past the span land in the spare row.  recorded() returns host arrays cut to what was run, plus
        `plants`; write_results(path) the reference's files; reset() zeroes the record; record_bytes is its size.  Refused
        (ValueError): plants that are not increasing, not distinct or outside [0, B), more than 64 plants, days < 1, buffers above
        record_max_bytes (default 2 ** 30: a guard against recording a whole batch by mistake, not a measured figure).
        health: False (the loops above: same launches, same bits, no new attributes) or True: the solve health PER PLANT beside the two
        global flags.  Every mode is a sequence of solves of four kinds, health_kinds = ("day_ahead", "real_time", "tracking",
        "projection"); directly after every solve its rows are booked to the plant they belong to - a solve with R rows per plant books
        rows b * R .. b * R + R - 1 to plant b; R = S for the independent bidding batches, 1 for a coupled day-ahead row, a
        self-schedule's hourly LP, the tracker and the projection tracker: exactly the rows whose status and flags feed `bad` and
        `uncertified` - into persistent device tensors, all zeroed by reset(): health_solves / health_fail / health_waived [4, B] int32
        (rows solved; rows with status != 0; rows with status 0 and DSP_FLAG_OBJ_WAIVED), health_status [4, B] int32 (the OR of
        1 << status over the failed rows: bits 1 .. 4), health_iters [4, B] int64 / health_iters_max [4, B] int32 (sum and maximum of
        dsp_batch::iters: PDHG iterations or simplex pivots, whatever the path reports) and health_first [B] int64 (device clock + 1
        at the plant's first non-optimal row of any kind, 0 = none).  So bool(bad) == bool(health_fail.sum() > 0) and uncertified ==
        health_waived.sum() at every point of a run.  The pending bid of ruc_hour is booked as day_ahead at the clock of the hour it
        is made; the 24 - H solves of its projection chain as projection; bidder="parametrized" books tracking only.  Works in every
        mode, with ledger and record, eagerly or from graphs: one launch of dsp_loop_health per solve inside the step (csrc/dsp_health.hip;
        use_fused=False and the CPU stand-in: the same integers as tensor operations, _health_book).  results() gains failed_solves,
        uncertified_solves, first_failure_hour (-1: none) and valid [B].
        profiles: None (the loops above: same launches, same bits, no `profile` attribute) or an integer days >= 1: the loop keeps the
        delivered power of EVERY plant, hour by hour, in `profile` [days + 1, 24, B] float64 MW - plant-minor, so that one wave's stores
        and the later loads of representative_days.py are consecutive; the last row is the spare row for hours past the span (the
        recorder's rule).  Written after the hand-off of every hour step, at h = clock - 1: profile[min(h // 24, days), h % 24, :] =
        delivered - one launch of dsp_loop_profile (csrc/dsp_days.hip) inside the captured step, so the graphs stay as many;
        use_fused=False and the CPU stand-in: index_copy_ at the same row rule, the same bits.  Works in every mode and with sizes,
        nuclear operands, ledger, health and record, since every mode ends an hour by writing `delivered`.  reset() zeroes the buffer;
        profiles_host() returns [B, whole days run (at most days), 24]; profile_bytes is its size.  Refused (ValueError): days that is
        not an integer >= 1, a buffer above profile_max_bytes (default 2 ** 30: a guard like record_max_bytes, not a measured figure).
        What the profiles are for: representative_days.DayPoints.
        past_midnight: "free" (the default: the loops above, same launches, same bits, no new attribute) or "coupled"
        (bidder="self_schedule" or scenario_coupling="monotone"; all three flowsheets, both markets; with ledger, health, record,
        profiles, simplex_warm, simplex_certify, eagerly or from graphs): the last T_rt - 1 hours of a day - whose real-time look-ahead
        reaches past midnight, where day_ahead_power is free - solve ONE coupled real-time LP per plant, as the host bidders do
        (workflow/bidder.py::compute_real_time_bids on CoupledScenarioModel(energy_prices=rt)): self.rtc, B rows of S blocks of the
        real-time LP (block i of row b = row b * S + i of the stochastic mode's hourly batch at that hour; self.rt_block is that view)
        plus the coupling rows over ALL T_rt periods - static 0, 0 for a self-schedule, for the monotone Bidder bounds that follow the
        order of the hour's REAL-TIME scenario prices.  Curves: block i's P_T[t] with scenario i's real-time forecast, the plant's one
        status for its S pairs (a self-schedule: the one pair (block 0's P_T[t], 0)); clearing, tracking, hand-off, ledger and profile
        are unchanged; health books one real_time solve per plant and `solves` counts B + B in those hours; the coupled handle's
        warm-start chain begins at the day's first such hour.  A recorded late hour hands the coupled solve to the real-time batch's
        buffers (_tied_record).  The earlier hours are unchanged.  csrc/dsp_market.hip (dsp_loop_midnight_prepare; dsp_loop_market_clear
        on the coupled rows with k >= 0) is the same arithmetic as _tied_blocks, bit for bit.  A coupled hourly LP that the solver
        streams keeps its hours' steps eager (hour_step); the project's shapes stay in the fused kernels or the in-wave simplex.
        Refused (ValueError): another value; "coupled" with a bidder that does not couple its scenarios."""
        import torch
        self.flowsheet = flowsheet
        self.B = B = int(n_scenarios)
        self._rec, self.record_bytes = None, 0
        self._profile_days = None if profiles is None else self._check_profiles(profiles, B, int(profile_max_bytes))
        if record is not None:
            from .loop_record import check_record
            record = check_record(record, B)
        self.S = S = int(n_price_scenarios)
        self.D = D = int(max_historical_days)
        bid_price, storage_mw, ruc_hour, sizes, plant_windows = self._validate(
            forecaster, market, bidder, tracking_horizon, bid_price, storage_mw, ruc_hour, wind_mw, battery_mw, battery_mwh, plant_windows,
            scenario_coupling)
        self._check_past_midnight(past_midnight)
        nuclear = self._nuclear_operands(pem_mw, tank_kg, h2_price, h2_demand)
        self.nuclear_sized = nuclear is not None
        if self.nuclear_sized:
            sizes = nuclear
        self.ruc_hour, self.sized = ruc_hour, sizes is not None and not self.nuclear_sized
        self.forecaster, self.market = forecaster, market
        self.stochastic = forecaster != "perfect" or market != "stub" or self.parametrized or self.self_schedule
        rows = 1 if self.parametrized else B if self.self_schedule else B * S                           # rows of the bidding batches (plant b, scenario i: row b * S + i; no bidding LP is solved in parametrized mode: one template row)
        self.dev = dev = torch.device("cuda", device) if lp_backend is None else torch.device("cpu")
        # one template for the batch, built at its largest sizes (None: the default plant's, untouched)
        bidder, da_model, rt_model, tracker, d = _templates(flowsheet, day_ahead_horizon, tracking_horizon,
                                                            None if sizes is None else {k: float(v.max()) for k, v in sizes.items()})
        tr_model = tracker.model
        if self.sized or self.nuclear_sized:
            _check_template(flowsheet, day_ahead_horizon, tracking_horizon, (da_model, rt_model, tr_model))
        self.bidder, self.tracker_template = bidder, tracker
        da_s, rt_s, cf_s = d["prices"]
        self.N = N = len(rt_s)
        if not self.parametrized and tracking_horizon > len(rt_model.HOUR):       # (the parametrized mode has no real-time LP)
            raise ValueError(f"tracking_horizon must be <= the real-time horizon ({len(rt_model.HOUR)}): the tracker follows the first periods of the real-time offer")
        if self.stochastic and not self.parametrized and (24 * D > N or not 24 <= len(da_model.HOUR) <= 48):
            raise ValueError("the stochastic mode needs max_historical_days whole days inside the series and a day-ahead horizon of 24 .. 48 periods")
        if ruc_hour is not None and forecaster == "backcast" and 24 * (D + 1) > N:
            raise ValueError("ruc_hour with forecaster='backcast' needs max_historical_days + 1 whole days inside the series: the real-time "
                             "history of a bid made at the RUC hour ends one day earlier")
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), device=dev)
        idx = lambda cols: torch.as_tensor(np.asarray(cols, np.int64), device=dev)
        self.da_series, self.rt_series = t(da_s), t(rt_s)
        self.cf_series = t(cf_s) if cf_s is not None else None
        self.stride = d["stride"]
        self.start = idx((d["stride"] * (first_scenario + plant_windows)) % N)
        power = bidder.bidding_model_object.power_output
        fam = d["family"]

        def wind_of(model):
            if cf_s is None:
                return None
            f = getattr(model.block, fam)
            cols = [p["wind"].index for p in f["periods"]]
            return cols, f["wind_kw"], d["per_kw"], f["wind_kw"] * float(np.sum(cf_s[:len(cols)]))
        self.simplex_certify = bool(simplex_certify) and lp_backend is None      # hourly LPs under dsp_options::simplex_certify = 1 (attach_solver)
        mk = lambda model, nb, solved=True: _Model(model, fam, nb, dev, device, power, d["init"](model.block), wind_of(model), lp_backend, solved, self.simplex_certify)
        if self.coupled_da:                           # ONE coupled day-ahead LP per plant (module docstring)
            self.da_block = mk(da_model, 1, False)
            self.da_block.pda_cols = idx(da_model.pda_cols)
            self.da = self.da_block.couple(da_model, S, B, dev, device, lp_backend, "monotone" if self.monotone else "non_anticipative")
            self.rt, self.tr = mk(rt_model, B if self.self_schedule else B * S), mk(tr_model, B)
            if self.self_schedule:                    # its hourly LPs are scenario 0's; the monotone Bidder's are the stochastic mode's B * S
                self.rt.per_plant = 1
        else:
            self.da, self.rt, self.tr = mk(da_model, rows, not self.parametrized), mk(rt_model, rows, not self.parametrized), mk(tr_model, B)
        self.da.pda_cols, self.rt.pda_cols = idx(da_model.pda_cols), idx(rt_model.pda_cols)
        self.tr.track_rows = idx([tr_model.block.kept_row_index(r) for r in tr_model.tracking_rows])
        self.tr.state_real = d["real"](tr_model.block)
        self.scale = [10.0 ** k for k in d["decimals"]]
        self.penalty = float(bidder.real_time_underbid_penalty)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        self.state = z(B, len(self.scale))                                # realised state of every plant
        self.revenue, self.energy_mwh, self.delivered = z(B), z(B), z(B)
        self.da_offer, self.da_prices = z(B, 24), z(B, 24)
        self.bad = torch.zeros((), dtype=torch.bool, device=dev)
        self.uncertified = torch.zeros((), dtype=torch.int64, device=dev)
        self.hour_t = torch.zeros((), dtype=torch.int64, device=dev)     # the clock on the device (graphs replay across days)
        self._clk, self._st = self.hour_t, self.state                     # what a bidding step reads as clock and state (ruc_hour: the bid's)
        self._scale_t = [torch.full((), s, dtype=torch.float64, device=dev) for s in self.scale]
        self.hour = self.solves = 0
        self.use_graphs = bool(use_graphs) and lp_backend is None
        self.simplex_warm = bool(simplex_warm) and lp_backend is None
        self._graphs, self._warm, self._pending = {}, False, False
        self._da_capturable = None                    # a coupled day-ahead LP: may its step be a graph node (day_ahead)
        self.use_fused = bool(use_fused) and lp_backend is None and self.rt.T <= 16 and self.tr.T <= 16 and len(self.scale) <= 2
        self.exact = self.sized or self.nuclear_sized or self.parametrized or self.coupled_da       # these state phase 2 of dsp_loop_update exactly, sums included (_hand_off)
        # what reset() zeroes and what results() reports beyond obj / energy_mwh / state: every setup below adds its own
        self._zeroed = [self.state, self.revenue, self.energy_mwh, self.delivered, self.da_offer, self.da_prices, self.hour_t, self.uncertified, self.bad]
        self._result_keys = []
        if self.exact:
            self.tr.set_first_period_terms(dev)
        if self.sized:
            self._sizes_setup(sizes, d, tracker)
        if self.parametrized:
            self._parametrized_setup(d, bid_price, storage_mw, tr_model, fam)
        elif self.stochastic:
            self.p_min_cents = int(round(float(bidder.bidding_model_object.model_data.p_min) * 100.0))     # Bidder._assemble_bids: p_min of the generator
            for m in ((self.da_block if self.coupled_da else self.da), self.rt):
                cols = m.set_terms(dev)
                if set(cols[cols >= 0].tolist()) & set(m.pda_cols.cpu().tolist()):
                    raise ValueError("a column is both a term of the power output and day_ahead_power: the prices' objective entries would collide")
            self._market_buffers(S + 1)
            if self.past_midnight == "coupled":
                self._past_midnight_setup(rt_model, mk, idx(rt_model.pda_cols), lp_backend, device)
        if self.ruc_hour is not None:
            self._ruc_setup(mk(tr_model, B))
        self.p_min_cents_plant = None
        if self.nuclear_sized:
            self._nuclear_setup(nuclear, tr_model)
        self.ledger = bool(ledger)
        if self.ledger:
            self._ledger_setup(d, tr_model)
        if self.use_fused:
            self._fused_setup()
            if self.parametrized:
                self._param_setup()
            elif self.stochastic:
                self._market_setup()
        self.health = bool(health)
        if self.health:
            self._health_setup()
        if self._profile_days is not None:
            self._profile_setup()
        # the mode's day-ahead step, hour step and LP solves per call of day_ahead() / hour_step(), bound once
        if self.parametrized:
            self._da_step, self._hour, self._n_da, self._n_hour = self._day_ahead_step_parametrized, self._hour_step_parametrized, 0, B
        elif self.self_schedule:
            self._da_step, self._hour, self._n_da, self._n_hour = self._day_ahead_step_self_schedule, self._hour_step_bid, B, 2 * B
        elif self.monotone:
            self._da_step, self._hour, self._n_da, self._n_hour = self._day_ahead_step_monotone, self._hour_step_bid, B, B * S + B
        else:
            self._da_step = self._day_ahead_step_stochastic if self.stochastic else self._day_ahead_step
            self._hour = self._hour_step_bid if self.stochastic else self._hour_step
            self._n_da, self._n_hour = B * S, B * S + B
        if self.past_midnight == "coupled":            # the last T_rt - 1 hours of a day: ONE coupled real-time LP per plant
            self._hour = self._hour_step_past_midnight
        if record is not None:
            self._record_setup(record, int(record_max_bytes))

    # -- setup: buffers, argument checks, per-mode operands, the kernels' descriptors -----------------------------------------------------
    def _market_buffers(self, slots):
        """curves (integer cents: power, price; `count` points each, `slots` stored) and dispatches of the current day / hour, and the
        day's sums: persistent, like everything a step touches"""
        import torch
        B, dev, Tc = self.B, self.dev, self.tr.T
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        self.da_curve, self.da_count = i32(B, 24, slots, 2), i32(B, 24)
        self.rt_curve, self.rt_count = i32(B, Tc, slots, 2), i32(B, Tc)
        self.rt_dispatch = z(B, Tc)
        self.da_energy_mwh, self.offered_mwh = z(B), z(B)
        self._hundred = torch.full((), 100.0, dtype=torch.float64, device=dev)
        self._zeroed += [self.da_energy_mwh, self.offered_mwh]
        self._result_keys += ["da_energy_mwh", "offered_mwh"]             # what the market left on the table: offered (the curves' last points) against cleared

    def _validate(self, forecaster, market, bidder, tracking_horizon, bid_price, storage_mw, ruc_hour, wind_mw, battery_mw, battery_mwh, plant_windows,
                  scenario_coupling="independent"):
        """the arguments' checks that need no template (ValueError; __init__'s docstring) -> the normalised (bid_price, storage_mw,
        ruc_hour, sizes, plant_windows); sets self.parametrized / self.self_schedule / self.monotone / self.coupled_da"""
        flowsheet, B, S = self.flowsheet, self.B, self.S
        self._check_market_arguments(forecaster, market, S, self.D)
        if bidder not in ("lp", "parametrized", "self_schedule"):
            raise ValueError(f"bidder is 'lp', 'parametrized' or 'self_schedule', not {bidder!r}")
        self.parametrized = bidder == "parametrized"
        self.self_schedule = bidder == "self_schedule"
        if scenario_coupling not in ("independent", "monotone"):
            raise ValueError(f"scenario_coupling is 'independent' or 'monotone', not {scenario_coupling!r}")
        self.monotone = scenario_coupling == "monotone"
        self.coupled_da = self.self_schedule or self.monotone             # ONE coupled day-ahead LP per plant
        if self.monotone:
            if bidder != "lp":
                raise ValueError(f"scenario_coupling='monotone' belongs to bidder='lp': the LP Bidder's curve is what it orders, not {bidder!r}'s")
            if forecaster != "backcast":
                raise ValueError("scenario_coupling='monotone' orders the curve across backcast price scenarios: forecaster='backcast'")
            if S < 2:
                raise ValueError("scenario_coupling='monotone' needs n_price_scenarios >= 2: one scenario has no pairs to order (that is scenario_coupling='independent')")
            if ruc_hour is not None:
                raise ValueError("ruc_hour belongs to scenario_coupling='independent': a monotone bid made at the RUC hour on a projected state is a follow-up (DESIGN 9)")
            sized = [k for k, v in (("wind_mw", wind_mw), ("battery_mw", battery_mw), ("battery_mwh", battery_mwh)) if v is not None]
            if sized:
                raise ValueError(f"{', '.join(sized)}: per-plant sizes belong to scenario_coupling='independent' (a monotone batch of different plants is a follow-up, DESIGN 9)")
        if self.self_schedule:
            if ruc_hour is not None:
                raise ValueError("ruc_hour belongs to bidder='lp': a self-schedule made at the RUC hour on a projected state is a follow-up (DESIGN 9)")
            sized = [k for k, v in (("wind_mw", wind_mw), ("battery_mw", battery_mw), ("battery_mwh", battery_mwh)) if v is not None]
            if sized:
                raise ValueError(f"{', '.join(sized)}: per-plant sizes belong to bidder='lp' (a self-scheduling batch of different plants is a follow-up, DESIGN 9)")
        if self.parametrized:
            if flowsheet not in ("wind_pem", "wind_battery"):
                raise ValueError(f"bidder='parametrized' is the wind + PEM / wind + battery bidders' rule: not for {flowsheet!r}")
            if S != 1 or forecaster != "perfect":
                raise ValueError("bidder='parametrized' bids on a perfect forecast: forecaster='perfect', n_price_scenarios=1")
            if not 1 <= int(tracking_horizon) <= 16:
                raise ValueError("bidder='parametrized' takes a tracking_horizon of 1 .. 16 periods")
            for name, v in (("bid_price", bid_price), ("storage_mw", storage_mw)):
                if v is None:
                    raise ValueError(f"bidder='parametrized' needs {name}")
            bid_price, storage_mw = (_per_plant(v, name, B, below=2.0e7) for v, name in ((bid_price, "bid_price"), (storage_mw, "storage_mw")))      # (2e7: the range of the cent arithmetic, bid_curves.cents)
        elif bid_price is not None or storage_mw is not None:
            raise ValueError("bid_price and storage_mw belong to bidder='parametrized'")
        if ruc_hour is not None:
            if isinstance(ruc_hour, bool) or not isinstance(ruc_hour, (int, np.integer)) or not 1 <= int(ruc_hour) <= 23:
                raise ValueError(f"ruc_hour is None or an integer hour of the day 1 .. 23, not {ruc_hour!r}")
            if self.parametrized:
                raise ValueError("ruc_hour belongs to bidder='lp': a parametrized bid has no bidding LP and no state, nothing to project")
            ruc_hour = int(ruc_hour)
        sizes = self._plant_sizes(flowsheet, B, wind_mw, battery_mw, battery_mwh)
        if plant_windows is None:
            plant_windows = np.arange(B)
        else:
            plant_windows = np.asarray(plant_windows)
            if plant_windows.shape != (B,) or plant_windows.dtype.kind not in "iu":
                raise ValueError(f"plant_windows is an int array of length {B}")
            plant_windows = plant_windows.astype(np.int64)
        return bid_price, storage_mw, ruc_hour, sizes, plant_windows

    def _check_past_midnight(self, past_midnight):
        """past_midnight (ValueError; __init__'s docstring); "coupled" becomes an attribute of the loop, "free" leaves the class's"""
        if past_midnight not in ("free", "coupled"):
            raise ValueError(f"past_midnight is 'free' or 'coupled', not {past_midnight!r}")
        if past_midnight == "coupled":
            if not self.coupled_da:
                raise ValueError("past_midnight='coupled' ties the real-time look-ahead hours of a bidder that couples its price scenarios: "
                                 "bidder='self_schedule' or scenario_coupling='monotone'")
            self.past_midnight = "coupled"

    def _past_midnight_setup(self, rt_model, mk, pda_cols, lp_backend, device):
        """the coupled REAL-TIME model of past_midnight="coupled": self.rtc, B rows of S blocks of the real-time template plus the
        coupling rows over all T_rt periods (_Model.couple, as self.da on the day-ahead template), with a handle, output buffers and a
        warm-start chain of its own; self.rt_block is its [B * S, n1] view, which _set_rows writes; the pair index operands of the
        monotone rows' bounds (persistent: a captured step creates no tensor from host data)"""
        import torch
        B, S, dev = self.B, self.S, self.dev
        self.rt_block = mk(rt_model, 1, False)
        self.rt_block.pda_cols = pda_cols
        self.rtc = self.rt_block.couple(rt_model, S, B, dev, device, lp_backend, "monotone" if self.monotone else "non_anticipative",
                                        self.simplex_certify)
        self.rt_block.set_terms(dev)
        self._first_tied_hour = 24 - self.rt.T + 1
        at = lambda v: torch.as_tensor(v, dtype=torch.int64, device=dev)
        self._rtc_pair_j, self._rtc_pair_k = at([j for j, _ in self.rtc.pairs]), at([k for _, k in self.rtc.pairs])
        self._rtc_side = tuple(torch.full((), v, dtype=torch.float64, device=dev) for v in (0.0, float("-inf"), float("inf")))
        self._rtc_capturable = None                    # may a late hour's step be a graph node (hour_step; as day_ahead's _da_capturable)

    def _tied_hour(self, k):
        """hour k of the day is one of the last T_rt - 1, whose real-time look-ahead reaches past midnight, and the loop ties them"""
        return self.past_midnight == "coupled" and 24 - k < self.rt.T

    def _plant_sizes(self, flowsheet, B, wind_mw, battery_mw, battery_mwh):
        """validated sizes -> dict of float64 arrays [B] (wind_mw; wind_battery: battery_mw, battery_mwh too), or None without sizes"""
        given = {k: v for k, v in (("wind_mw", wind_mw), ("battery_mw", battery_mw), ("battery_mwh", battery_mwh)) if v is not None}
        if not given:
            return None
        if flowsheet == "nuclear":
            raise ValueError(f"{', '.join(given)}: the nuclear flowsheet has no plant sizes in this loop")
        if self.parametrized:
            raise ValueError(f"{', '.join(given)}: per-plant sizes belong to bidder='lp' (the parametrized bidders take storage_mw; their wind_mw is the flowsheet's)")
        if flowsheet == "wind_pem" and (battery_mw is not None or battery_mwh is not None):
            raise ValueError("wind_pem has no battery: battery_mw / battery_mwh are refused (the PEM capacity is a free column of its LP, not a size)")
        out = {name: _per_plant(v, name, B, positive=name == "wind_mw") for name, v in given.items()}
        if flowsheet == "wind_battery":
            if "battery_mwh" not in out:                                   # the flowsheet's own default: four hours of the given power
                out["battery_mwh"] = 4.0 * out["battery_mw"] if "battery_mw" in out else np.full(B, _WIND_BATTERY_SIZES["battery_mwh"])
            for name in ("wind_mw", "battery_mw"):
                out.setdefault(name, np.full(B, _WIND_BATTERY_SIZES[name]))
        total = out["wind_mw"] + out.get("battery_mw", 0.0)
        if (total >= 2.0e7).any():                                         # (2e7 MW: the range of the cent arithmetic, bid_curves.cents)
            raise ValueError("wind_mw + battery_mw must stay below 2e7")
        return out

    def _nuclear_operands(self, pem_mw, tank_kg, h2_price, h2_demand):
        """validated nuclear operands -> dict of float64 arrays [B] (what was left None at the flowsheet's default), or None without any"""
        from .flowsheets import parameters as prm
        given = {k: v for k, v in (("pem_mw", pem_mw), ("tank_kg", tank_kg), ("h2_price", h2_price), ("h2_demand", h2_demand)) if v is not None}
        if not given:
            return None
        names = ", ".join(given)
        if self.flowsheet != "nuclear":
            raise ValueError(f"{names}: the nuclear flowsheet's operands, not {self.flowsheet!r}'s")
        if self.parametrized or self.self_schedule:
            raise ValueError(f"{names}: per-plant sizes belong to bidder='lp'")
        if self.monotone:
            raise ValueError(f"{names}: per-plant sizes belong to scenario_coupling='independent' (a monotone batch of different plants is a follow-up, DESIGN 9)")
        out = {name: _per_plant(v, name, self.B, positive=name == "pem_mw") for name, v in given.items()}
        if "pem_mw" in out and (out["pem_mw"] > prm.np_capacity_mw).any():
            raise ValueError(f"pem_mw must be > 0 and at most the plant's {prm.np_capacity_mw:g} MW")
        for name, default in (("pem_mw", prm.nuclear_pem_capacity_mw), ("tank_kg", prm.tank_capacity_kg), ("h2_price", 4.0), ("h2_demand", 0.35)):
            out.setdefault(name, np.full(self.B, float(default)))
        return out

    def _nuclear_setup(self, ops, tr_model):
        """the per-plant operands of a nuclear batch, written ONCE into the per-row tensors of every model (rows b * S + i of the bidding
        models, row b of the tracker and of the projection tracker): np_to_pem <= pem kW, tank_holdup <= tank mol (every period but the
        last, as the flowsheet), outlet_to_pipeline <= demand mol/s, and the pipeline columns' objective entry -(mw_h2 * 3600 * h2_price)
        in the arithmetic of the flowsheet's tot_cost.  No step rewrites those; c_static keeps the deterministic tensor form from doing
        so.  p_min_cents_plant: the curves' first point, p_max - pem_mw in integer cents."""
        import torch
        from .flowsheets import parameters as prm
        B, S, dev = self.B, self.S, self.dev
        self.pem_mw, self.tank_kg, self.h2_price, self.h2_demand = (ops[k] for k in ("pem_mw", "tank_kg", "h2_price", "h2_demand"))
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), device=dev)
        pem_kw, tank_mol, demand = self.pem_mw * 1e3, self.tank_kg / prm.mw_h2, self.h2_demand / prm.mw_h2
        credit = np.array([prm.mw_h2 * 3600 * float(p) for p in self.h2_price])      # tot_cost: - outlet_to_pipeline * (mw_h2 * 3600 * h2_price)
        at = int(np.argmax(self.h2_price))                                          # the template IS the largest price: the same number, bit for bit
        models = [(self.da, self.bidder.day_ahead_model, S), (self.rt, self.bidder.real_time_model, S), (self.tr, tr_model, 1)]
        if self.ruc_hour is not None:
            models.append((self.pj, tr_model, 1))
        for m, model, per in models:
            periods = model.block.nuclear["periods"]
            pem, out = [p["pem_elec"].index for p in periods], [p["outlet_to_pipeline"].index for p in periods]
            hold = [p["tank_holdup"].index for p in periods[:-1]]
            base = m.base_c[out].cpu().numpy()
            if not (base == -credit[at]).all():
                raise RuntimeError(f"the template's pipeline objective entries {base!r} are not minus the hydrogen credit {credit[at]!r}")
            rows = lambda a: t(np.repeat(a, per))[:, None]
            m.ub[:, pem], m.ub[:, out] = rows(pem_kw), rows(demand)
            if hold:
                m.ub[:, hold] = rows(tank_mol)
            m.c[:, out] = rows(-credit)
            m.c_static = m.base_c.repeat(m.c.shape[0], 1)
            m.c_static[:, out] = rows(-credit)
            m.pem_cols, m.out_cols, m.hold_cols = pem, out, hold
        md = self.bidder.bidding_model_object.model_data
        self.p_min_cents_plant = torch.as_tensor(np.round((float(md.p_max) - self.pem_mw) * 100.0).astype(np.int64), device=dev)
        self._credit = credit

    def _sizes_setup(self, sizes, d, tracker):
        """the per-plant operands of a sized batch: wind kW and objective constant [B] of each of the three models (host, float64,
        once), and the battery's static bounds written into the per-row tensors (rows b * S + i of the bidding models, row b of the
        tracker) - elec_in / elec_out <= battery kW, state_of_charge_bounds <= battery kWh.  No step ever rewrites those."""
        import torch
        B, S, fam = self.B, self.S, d["family"]
        mo = self.bidder.bidding_model_object
        cf = d["prices"][2]
        self.wind_mw, self.battery_mw, self.battery_mwh = sizes["wind_mw"], sizes.get("battery_mw"), sizes.get("battery_mwh")
        wind_kw = self.wind_mw * 1e3
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), device=self.dev)

        def model_object(w):
            if self.flowsheet == "wind_battery":
                return mo.__class__(model_data=mo.model_data, wind_capacity_factors=list(cf[:max(self.da.T, self.rt.T, self.tr.T)]), wind_pmax_mw=w,
                                    battery_pmax_mw=mo._battery_pmax_mw, battery_energy_capacity_mwh=mo._battery_energy_capacity_mwh)
            return mo.__class__(mo.model_data, wind_capacity_factors=list(cf[:max(self.da.T, self.rt.T, self.tr.T)]), wind_pmax_mw=w,
                                pem_pmax_mw=mo._pem_pmax_mw)
        self._sized_model_object = model_object                            # (the ledger's per-plant constants: _ledger_setup)
        distinct, inverse = np.unique(self.wind_mw, return_inverse=True)
        for m, family in ((self.da, mo.total_cost), (self.rt, mo.total_cost), (self.tr, tracker.tracking_model_object.total_cost)):
            c0 = np.array([_objective_constant(model_object(float(w)), m.T, family, m.wind[2], cf) for w in distinct])
            at = int(np.argmax(distinct))                                  # the template IS the largest wind size: the same number, bit for bit
            if c0[at] != m.base_c0 or float(distinct[at]) * 1e3 != m.wind[1]:
                raise RuntimeError(f"the objective constant recomputed for the template's wind size ({c0[at]!r}) is not the template's ({m.base_c0!r})")
            m.set_plant_sizes(wind_kw, c0[inverse], self.dev)
        if self.flowsheet != "wind_battery":
            return
        batt_kw, batt_kwh = self.battery_mw * 1e3, self.battery_mwh * 1e3
        for m, model, per in ((self.da, self.bidder.day_ahead_model, S), (self.rt, self.bidder.real_time_model, S), (self.tr, tracker.model, 1)):
            periods = getattr(model.block, fam)["periods"]
            cols = [p[key].index for p in periods for key in ("elec_in", "elec_out")]
            rows = [model.lp.row_names.index(f"battery.state_of_charge_bounds[{k}]") for k in range(len(periods))]
            m.batt_cols, m.soc_rows = cols, rows
            m.ub[:, cols] = t(np.repeat(batt_kw, per))[:, None]
            m.rhi[:, rows] = t(np.repeat(batt_kwh, per))[:, None]

    def _ledger_setup(self, d, tr_model):
        """the ledger's operands, once: the forms of _ledger_forms as index lists and device arrays - coefficients [F, 8] and constants
        [F] shared by all plants, or per plant ([B, F, 8] / [B, F]) where plants differ: a sized wind batch carries each plant's own
        constants (fixed O&M on ITS wind_kw), computed like its objective constant from a model object of its size - and the
        accumulators / last hour's values [F, B]"""
        import torch
        from .lp import LinearBlock
        B, dev, tr = self.B, self.dev, self.tr
        forms = _ledger_forms(self.flowsheet, tr_model, d, with_h2_kg=not (self.parametrized and self.flowsheet == "wind_pem"))
        if len(forms) > LEDGER_MAX_FORMS:
            raise ValueError(f"the ledger takes at most {LEDGER_MAX_FORMS} forms, not {len(forms)}")
        keys, cols, coef, const, per_avail = [], [], np.zeros((len(forms), LEDGER_MAX_TERMS)), np.zeros(len(forms)), []
        for f, (key, row, c, pa) in enumerate(forms):
            nz = np.nonzero(row)[0]
            if len(nz) > LEDGER_MAX_TERMS:
                raise ValueError(f"the ledger's form {key!r} has {len(nz)} terms: the kernel takes at most {LEDGER_MAX_TERMS}")
            keys.append(key)
            cols.append([int(j) for j in nz])
            coef[f, :len(nz)], const[f] = row[nz], c
            per_avail.append(float(pa))
        if self.sized:                                 # per-plant constants: the same expressions of a model object of the plant's wind size
            distinct, inverse = np.unique(self.wind_mw, return_inverse=True)
            each = np.tile(const, (len(distinct), 1))
            for i, w in enumerate(distinct):
                block = LinearBlock("fs")
                self._sized_model_object(float(w)).populate_model(block, tr.T)
                for key, spec in _ledger_wind_expressions(d).items():
                    each[i, keys.index(key)] = _ledger_expression(block, len(block.col_names), d, *spec)[1]
            const = each[inverse]
        if self.nuclear_sized:                         # per-plant coefficients: the hydrogen credit at the plant's own price
            out0 = tr.out_cols[0]
            coef = np.tile(coef, (B, 1, 1))
            coef[:, keys.index("tot_cost"), cols[keys.index("tot_cost")].index(out0)] = -self._credit
            coef[:, keys.index("h2_revenue"), cols[keys.index("h2_revenue")].index(out0)] = self._credit
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), device=dev)
        z = lambda: torch.zeros((len(keys), B), dtype=torch.float64, device=dev)
        self.ledger_keys = keys
        self.ledger_acc, self.ledger_hour = z(), z()
        self._ledger = dict(keys=keys, cols=cols, per_avail=per_avail, coef=t(coef), const=t(const), acc=self.ledger_acc, hour=self.ledger_hour,
                            per_avail_t=t(per_avail))
        self._zeroed += [self.ledger_acc, self.ledger_hour]

    def _health_setup(self):
        """the health counters (persistent, zeroed by reset()), the operands of the tensor form and - with the kernels - the descriptor"""
        import torch
        from .hip_solver import HEALTH_KINDS
        B, dev = self.B, self.dev
        z = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=dev)
        self.health_kinds = HEALTH_KINDS
        K = len(HEALTH_KINDS)
        self.health_solves, self.health_fail = z(torch.int32, K, B), z(torch.int32, K, B)
        self.health_status, self.health_waived = z(torch.int32, K, B), z(torch.int32, K, B)
        self.health_iters, self.health_iters_max = z(torch.int64, K, B), z(torch.int32, K, B)
        self.health_first = z(torch.int64, B)
        self._zeroed += [self.health_solves, self.health_fail, self.health_status, self.health_waived, self.health_iters, self.health_iters_max,
                         self.health_first]
        self._result_keys += ["failed_solves", "uncertified_solves", "first_failure_hour", "valid"]
        # (persistent operands: a captured step creates no tensor from host data)
        self._health_consts = tuple(torch.full((), v, dtype=torch.int32, device=dev) for v in (0, 1, 30))
        if self.use_fused:
            from .hip_solver import DspLoopHealthState
            h = DspLoopHealthState()
            h.B, h.clock = B, self.hour_t.data_ptr()
            h.solves, h.fail, h.status_mask, h.waived = (v.data_ptr() for v in (self.health_solves, self.health_fail, self.health_status, self.health_waived))
            h.iters, h.iters_max, h.first = self.health_iters.data_ptr(), self.health_iters_max.data_ptr(), self.health_first.data_ptr()
            self._health_state = h

    # what results() reports of the health counters (the keys _health_setup adds to _result_keys)
    @property
    def failed_solves(self):
        return self.health_fail.sum(0)

    @property
    def uncertified_solves(self):
        return self.health_waived.sum(0)

    @property
    def first_failure_hour(self):
        return self.health_first - 1

    @property
    def valid(self):
        return self.health_fail.sum(0) == 0

    def _parametrized_setup(self, d, bid_price, storage_mw, tr_model, fam):
        import torch
        from .flowsheets import parameters as prm
        dev = self.dev
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), device=dev)
        self.p_min_cents = 0
        self.bid_price, self.storage_mw = t(bid_price), t(storage_mw)
        self.da_cf_series = t(d["da_cf"])
        if len(d["da_cf"]) != self.N or self.N < 24:
            raise ValueError("the day-ahead capacity factors must cover the series, and the series a day")
        self.wind_mw = float(self.bidder.bidding_model_object._wind_pmax_mw)       # the host bidders' wind_mw
        self.battery = self.flowsheet == "wind_battery"                            # p_max = max(w, storage_mw) (FixedParametrizedBidder)
        self._market_buffers(4)                                                    # three pairs: at most 3 points in the S + 1 = 4 slots of plant_curves
        self.h2_kg = None
        if self.flowsheet == "wind_pem":                                           # MultiPeriodWindPEM._h2_kg_per_hr of the implemented hour
            self.h2_kg = torch.zeros(self.B, dtype=torch.float64, device=dev)
            self._zeroed.append(self.h2_kg)
            self._result_keys.append("h2_kg")
            self.pem_col = int(getattr(tr_model.block, fam)["periods"][0]["pem_elec"].index)
            self._h2_mul = float(prm.pem_electricity_to_mol)
            self._h2_div = torch.full((), float(prm.h2_mols_per_kg), dtype=torch.float64, device=dev)

    def _param_setup(self):
        from .hip_solver import DspLoopParamState
        ps = DspLoopParamState()
        ps.B, ps.N, ps.price_taker, ps.battery = self.B, self.N, int(self.market == "price_taker"), int(self.battery)
        for name in ("start", "hour", "da_series", "rt_series", "state", "da_offer", "da_prices"):
            setattr(ps, name, getattr(self._loop_state, name))
        ps.da_cf_series, ps.rt_cf_series = self.da_cf_series.data_ptr(), self.cf_series.data_ptr()
        ps.bid_price, ps.storage_mw, ps.wind_mw = self.bid_price.data_ptr(), self.storage_mw.data_ptr(), self.wind_mw
        ps.da_curve, ps.da_count = self.da_curve.data_ptr(), self.da_count.data_ptr()
        ps.rt_dispatch, ps.rt_curve, ps.rt_count = self.rt_dispatch.data_ptr(), self.rt_curve.data_ptr(), self.rt_count.data_ptr()
        if self.h2_kg is not None:
            ps.h2_kg, ps.pem_col = self.h2_kg.data_ptr(), self.pem_col
            ps.h2_mul, ps.h2_div = self._h2_mul, float(self._h2_div.item())
        self._param_state = ps

    def _fused_setup(self):
        from .hip_solver import DspLoopModel, DspLoopState, load_library
        self._lib = load_library()
        loop_model = lambda m: _describe(DspLoopModel, m, len(self.scale))
        st = DspLoopState()
        st.B, st.N = self.B, self.N
        st.start, st.hour = self.start.data_ptr(), self.hour_t.data_ptr()
        st.da_series, st.rt_series = self.da_series.data_ptr(), self.rt_series.data_ptr()
        st.cf_series = self.cf_series.data_ptr() if self.cf_series is not None else None
        st.state = self.state.data_ptr()
        for j in range(2):
            st.state_scale[j] = self.scale[j] if j < len(self.scale) else 1.0
        st.da_offer, st.da_prices = self.da_offer.data_ptr(), self.da_prices.data_ptr()
        st.delivered, st.revenue, st.energy_mwh = self.delivered.data_ptr(), self.revenue.data_ptr(), self.energy_mwh.data_ptr()
        st.bad, st.uncertified = self.bad.data_ptr(), self.uncertified.data_ptr()
        self._loop_state = st
        self._loop_rt, self._loop_tr = loop_model(self.rt), loop_model(self.tr)
        if self.ledger:
            self._loop_ledger = _describe_ledger(self._ledger)
        if self.ruc_hour is not None:
            from .hip_solver import DspLoopProjectState
            self._loop_pj = loop_model(self.pj)
            ps = DspLoopProjectState()
            ps.B, ps.N, ps.ruc_hour = self.B, self.N, self.ruc_hour
            ps.slots = self.da_curve.shape[2] if self.stochastic else 0
            for name in ("start", "hour", "cf_series", "state", "bad", "uncertified", "da_offer", "da_prices"):
                setattr(ps, name, getattr(st, name))
            for j in range(2):
                ps.state_scale[j] = st.state_scale[j]
            ps.obj = self.pj.out["obj"].data_ptr()
            ps.proj_state, ps.proj_real, ps.proj_obj = self.proj_state.data_ptr(), self.proj_real.data_ptr(), self.proj_obj.data_ptr()
            ps.pend_offer, ps.pend_prices = self.pend_offer.data_ptr(), self.pend_prices.data_ptr()
            if self.stochastic:
                ps.da_curve, ps.da_count = self.da_curve.data_ptr(), self.da_count.data_ptr()
                ps.pend_curve, ps.pend_count = self.pend_curve.data_ptr(), self.pend_count.data_ptr()
            self._proj_state_c = ps

    def _market_setup(self):
        from .hip_solver import DspLoopMarketModel, DspLoopMarketState
        mk = DspLoopMarketState()
        mk.B, mk.S, mk.D, mk.N = self.B, self.S, self.D, self.N
        mk.backcast, mk.price_taker = int(self.forecaster == "backcast"), int(self.market == "price_taker")
        for name in ("start", "hour", "da_series", "rt_series", "cf_series", "state", "da_offer", "da_prices", "bad", "uncertified"):
            setattr(mk, name, getattr(self._loop_state, name))
        mk.p_min_cents = self.p_min_cents
        if self.p_min_cents_plant is not None:
            mk.p_min_cents_plant = self.p_min_cents_plant.data_ptr()
        self._mk_state = mk
        self._mk_da, self._mk_rt = (_describe(DspLoopMarketModel, m, len(self.scale)) for m in (self.da, self.rt))
        if self.monotone:
            # the coupled rows: one block described, blocks S * n1 apart; c0 / status / flags one entry per plant.  The day-ahead
            # clearing reads scenario i of plant b from block i of row b (coupled = 1); the hourly steps run on the ordinary state
            self._mk_da.row_stride = self.da.lp.n
            self._mk_coupled = DspLoopMarketState.from_buffer_copy(mk)
            self._mk_coupled.coupled = 1
        if self.self_schedule:
            # the coupled rows: one block described, blocks S * n1 apart; c0 / status / flags one entry per plant.  Everything but the
            # day-ahead fan-out runs on an S = 1 state (scenario 0 = the most recent backcast day): pairs priced at 0, curves in the
            # loop's S + 1 slots
            self._mk_da.row_stride = self.da.lp.n
            self._mk_sched = mk
            one = DspLoopMarketState.from_buffer_copy(mk)
            one.S, one.self_schedule, one.curve_slots = 1, 1, self.S + 1
            self._mk_state = one
        if self.past_midnight == "coupled":            # the coupled real-time rows: one block described, blocks S * n1 apart, as the day-ahead ones
            self._mk_rtc = _describe(DspLoopMarketModel, self.rtc, len(self.scale))
            self._mk_rtc.row_stride = self.rtc.lp.n
        if self.ruc_hour is not None:                  # the bid made at the RUC hour: its own clock, the projected state, the pending buffers
            bid = DspLoopMarketState.from_buffer_copy(mk)
            bid.hour, bid.state = self.bid_hour_t.data_ptr(), self.proj_state[-1].data_ptr() if len(self.scale) else None
            bid.da_offer, bid.da_prices = self.pend_offer.data_ptr(), self.pend_prices.data_ptr()
            bid.rt_history_lag_days = 1
            self._mk_bid = bid

    @staticmethod
    def _check_profiles(days, B, max_bytes):
        if isinstance(days, bool) or not isinstance(days, (int, np.integer)) or days < 1:
            raise ValueError(f"profiles is None or an integer number of days >= 1, not {days!r}")
        total = (int(days) + 1) * 24 * B * 8
        if total > max_bytes:
            raise ValueError(f"profiles: the buffer of {B} plants over {int(days)} days takes {total} bytes, more than profile_max_bytes = {max_bytes}")
        return int(days)

    def _profile_setup(self):
        """the profile buffer (persistent, zeroed by reset()), the operand of the tensor form and - with the kernels - the descriptor"""
        import torch
        B, days, dev = self.B, self._profile_days, self.dev
        self.profile = torch.zeros((days + 1, 24, B), dtype=torch.float64, device=dev)
        self.profile_bytes = self.profile.numel() * 8
        self._zeroed.append(self.profile)
        self._profile_days_t = torch.full((), days, dtype=torch.int64, device=dev)
        if self.use_fused:
            from .hip_solver import DspLoopProfileDesc
            d = DspLoopProfileDesc()
            d.B, d.days, d.clock = B, days, self.hour_t.data_ptr()
            d.delivered, d.profile = self.delivered.data_ptr(), self.profile.data_ptr()
            self._profile_desc = d

    def _profile_write(self):
        """the hour that just ended (clock - 1), AFTER the hand-off: every plant's delivered power into the row the device clock names;
        hours past the span go to the spare row.  With the kernels one launch of dsp_loop_profile; otherwise its statement as tensor
        operations - a copy, so the two are equal bit for bit."""
        if self._profile_days is None:
            return
        if self.use_fused:
            import ctypes as C
            self._call(self._lib.dsp_loop_profile, C.byref(self._profile_desc))
            return
        self._profile_write_tensors(self.profile)

    def _profile_write_tensors(self, profile):
        """the specification of dsp_loop_profile on a buffer [days + 1, 24, B]"""
        import torch
        h, days = self.hour_t - 1, self._profile_days_t
        day = torch.minimum(torch.div(h, 24, rounding_mode="floor"), days)
        row = torch.where(h < 0, days * 24, day * 24 + h % 24).view(1)
        profile.view(-1, self.B).index_copy_(0, row, self.delivered.unsqueeze(0))

    def profiles_host(self):
        """-> numpy [B, D, 24], D = whole days run so far (at most the span): plant b's delivered MW of day d, hour h"""
        if self._profile_days is None:
            raise RuntimeError("this loop keeps no profiles: construct it with profiles=days")
        D = min(self.hour // 24, self._profile_days)
        return np.ascontiguousarray(self.profile[:D].cpu().numpy().transpose(2, 0, 1))

    def _record_setup(self, record, max_bytes):
        """the recorder (loop_record.LoopRecorder: buffers, segments, descriptors) and the day-ahead step that ends with its daily write"""
        from .loop_record import LoopRecorder
        self._rec = LoopRecorder(self, record[0], record[1], max_bytes)
        self.record_bytes = self._rec.bytes
        step = self._da_step

        def recorded_step(bid=False):
            if bid:
                step(bid=True)
            else:
                step()
            self._rec.write("bid" if bid else "daily")
        self._da_step = recorded_step

    # -- the kernels (C ABI, on the current stream: _call) ------------------------------------------------------------------------------
    def _fused(self, phase, k):
        import ctypes as C
        if phase == 2 and self.ledger:                 # the implemented hour is booked before the hand-off advances the clock
            self._call(self._lib.dsp_loop_ledger, C.byref(self._loop_state), C.byref(self._loop_tr), C.byref(self._loop_ledger))
        if phase == 2 and self._rec is not None:       # ... and recorded: the state is still the one the hour's LPs were built from
            self._rec.write("hour")
        self._call(self._lib.dsp_loop_update, C.byref(self._loop_state), C.byref(self._loop_rt), C.byref(self._loop_tr), phase, k)
        if phase == 2 and self._rec is not None:       # after the hand-off: delivered power of the hour that just ended (clock - 1)
            self._rec.write("after")
        if phase == 2:
            self._profile_write()

    def _param(self, phase, k):
        import ctypes as C
        self._call(self._lib.dsp_loop_param_step, C.byref(self._param_state), C.byref(self._loop_tr), phase, k)

    def _project(self, phase, j):
        import ctypes as C
        self._call(self._lib.dsp_loop_project, C.byref(self._proj_state_c), C.byref(self._loop_pj), phase, j)

    def _market_prepare(self, m, k, bid=False):
        """objective, bounds, state and constant of bidding model m's rows at hour k of the day (-1: the day-ahead bid; bid: the one
        made at the RUC hour)"""
        import ctypes as C
        self._call(self._lib.dsp_loop_market_prepare, C.byref(self._mk_bid if bid else self._mk_state), C.byref(m), k)

    def _market_clear(self, m, tr, k, T, dispatch, curve, count, bid=False, state=None):
        """curves of the T periods from m's solution, cleared into `dispatch` (status / flags of the solve: folded into bad / uncertified
        by the kernel); tr: the tracker whose LP the clearing lanes also write, or None; state: a market state of its own"""
        import ctypes as C
        self._call(self._lib.dsp_loop_market_clear, C.byref(state or (self._mk_bid if bid else self._mk_state)), C.byref(m), None if tr is None else C.byref(tr), k, T,
                   *(C.c_void_p(v.data_ptr()) for v in (dispatch, curve, count)))

    # -- pieces of a step (all capturable: persistent tensors, the clock read on the device; windows, curves, clearing: _DeviceLoop) ------
    def _set_prices(self, m, da, rt):
        """c = base - RT . dP_T/dx - (DA - RT) on day_ahead_power ; c0 = base - RT . PT_const (Bidder._pass_price_forecasts)"""
        m.c.copy_((m.base_c if m.c_static is None else m.c_static) - rt @ m.PT)
        m.c[:, m.pda_cols] -= da - rt
        return -(rt @ m.PT_const)                                         # the prices' share of the objective constant [B]

    def _set_state(self, m, price_c0=None):
        """what update_model writes: the state columns fixed to the realised values, wind availability of the window; and the objective
        constant of every plant (dsp_batch::obj_offset: the scale of the solver's objective-accuracy test, cf. rolling.py)"""
        for k, col in enumerate(m.state_init):
            m.lb[:, col] = self._st[:, k]
            m.ub[:, col] = self._st[:, k]
        if m.c0_plant is None:
            m.c0.fill_(m.base_c0)
        else:
            m.c0.copy_(m.c0_plant)
        if price_c0 is not None:
            m.c0 += price_c0
        if m.wind is not None:
            cols, _, per_kw = m.wind
            avail = m.kw() * self._window(self.cf_series, m.T)
            m.ub[:, cols] = avail
            m.c0 += per_kw * avail.sum(1)

    # -- the deterministic loop: perfect forecast, stub market ----------------------------------------------------------------------------
    def _day_ahead_step(self, bid=False):
        """bid: the bid made at the RUC hour for the next day (clock and state are the bid's, self._clk / self._st; the pending buffers)"""
        m = self.da
        da, rt = self._window(self.da_series, m.T), self._window(self.rt_series, m.T)
        self._set_state(m, self._set_prices(m, da, rt))
        self._free_day_ahead_power(m)
        out = m.solve(self.B)
        self._health_book("day_ahead", m, 1)
        self._check(out)
        (self.pend_offer if bid else self.da_offer).copy_(out["x"][:, m.pda_cols][:, :24])
        (self.pend_prices if bid else self.da_prices).copy_(da[:, :24])

    def _hour_step(self, k):
        if self.use_fused:
            hour = k if self.simplex_warm else None
            self._fused(0, k)
            self.rt.solve(self.B, hour=hour)            # (status / flags: checked by the kernel's next phase)
            self._health_book("real_time", self.rt, 1)
            self._fused(1, k)
            self.tr.solve(self.B, hour=hour)
            self._health_book("tracking", self.tr, 1)
            self._fused(2, k)
            return
        m = self.rt
        rt = self._window(self.rt_series, m.T)
        da = self._window(self.da_series, m.T).clone()
        known = min(m.T, 24 - k)                                          # hours of the horizon inside the cleared day
        da[:, :known] = self.da_prices[:, k:k + known]
        self._set_state(m, self._set_prices(m, da, rt))
        self._free_day_ahead_power(m, k)
        hour = k if self.simplex_warm else None
        out = m.solve(self.B, hour=hour)
        self._health_book("real_time", m, 1)
        self._check(out)
        offer = m.power_output(out["x"])                                  # real-time offer = SCED dispatch in the stub market
        tr = self.tr
        self._set_state(tr)
        rhs = offer[:, :tr.T] - tr.PT_const
        tr.rlo[:, tr.track_rows] = rhs
        tr.rhi[:, tr.track_rows] = rhs
        out = tr.solve(self.B, hour=hour)
        self._health_book("tracking", tr, 1)
        self._check(out)
        self._hand_off(out["x"], rt[:, 0], k, exact=False)

    def _hand_off(self, x, rt0, k, exact):
        """the end of hour k on the tracker's solution x: delivered power, the implemented profile -> next hour's state rounded as
        update_model does, revenue, energy, clock.  exact: delivered power and revenue in the arithmetic of phase 2 of dsp_loop_update,
        so that the tensor form and the kernels agree bit for bit on the sums too - P_T[0] = fma(cb, x[b], fma(ca, x[a], const)),
        revenue += fma(delivered, rt, da_offer * (da - rt)); otherwise the matrix form, equal to the kernels' to a tolerance"""
        import torch
        tr = self.tr
        if self.ledger:
            self._ledger_book(x)
        if self._rec is not None:
            self._rec.write("hour")
        day_ahead = self.da_offer[:, k] * (self.da_prices[:, k] - rt0)
        if exact:
            p = tr.PT_const[0].expand(self.B)
            for e in range(tr.p0_cols.shape[0]):
                p = exact_fma(torch, tr.p0_coef[e].expand(self.B), x[:, tr.p0_cols[e]], p)
            self.delivered.copy_(p)
        else:
            self.delivered.copy_(tr.power_output(x)[:, 0])
        for j, col in enumerate(tr.state_real):
            self.state[:, j] = torch.round(x[:, col] * self.scale[j]) / self._scale_t[j]
        self.revenue += exact_fma(torch, self.delivered, rt0, day_ahead) if exact else self.delivered * rt0 + day_ahead
        self.energy_mwh += self.delivered
        self.hour_t += 1
        if self._rec is not None:
            self._rec.write("after")
        self._profile_write()

    def _ledger_book(self, x):
        """the ledger of the implemented hour on the tracker's solution x [B, n], BEFORE the hand-off (the clock is still the hour's), in
        the arithmetic of dsp_loop_ledger so that the two agree bit for bit: v = constant; v = fma(coef_e, x[col_e], v) in the order of
        e; v = fma(per_avail, avail0, v) where the form has a per_avail, avail0 = wind_kw[b] * cf[(start[b] + hour) % N] rounded on its
        own; ledger_hour[f] = v; ledger_acc[f] += v"""
        import torch
        L, B = self._ledger, self.B
        coef, const = L["coef"], L["const"]
        avail0 = None
        if any(L["per_avail"]):
            kw = self.tr.kw()
            avail0 = (kw if isinstance(kw, float) else kw[:, 0]) * self.cf_series[(self.start + self.hour_t) % self.N]
        for f, cols in enumerate(L["cols"]):
            v = (const[f] if const.dim() == 1 else const[:, f]).expand(B)
            for e, col in enumerate(cols):
                v = exact_fma(torch, (coef[f, e] if coef.dim() == 2 else coef[:, f, e]).expand(B), x[:, col], v)
            if L["per_avail"][f] != 0.0:
                v = exact_fma(torch, L["per_avail_t"][f].expand(B), avail0, v)
            self.ledger_hour[f].copy_(v)
            self.ledger_acc[f] += v

    def _health_book(self, kind, m, rows_per_plant):
        """the solve of model m that has just finished, booked per plant under `kind` (health_kinds), BEFORE the step advances the clock:
        rows b * R .. b * R + R - 1 of m.out belong to plant b.  With the kernels one launch of dsp_loop_health; otherwise its statement
        as tensor operations - integers, so the two are equal exactly.  A backend without flags / iters (the CPU stand-in has no
        flags) leaves the counters that need them untouched, like the kernel's NULL."""
        if not self.health:
            return
        import torch
        out, B, R, k = m.out, self.B, int(rows_per_plant), self.health_kinds.index(kind)
        if self.use_fused:
            import ctypes as C
            ptr = lambda key: C.c_void_p(out[key].data_ptr()) if out.get(key) is not None else None
            self._call(self._lib.dsp_loop_health, C.byref(self._health_state), ptr("status"), ptr("flags"), ptr("iters"), R, k)
            return
        zero, one, other = self._health_consts
        status = out["status"].reshape(B, R)
        failed = status != 0
        n_failed = failed.sum(1)
        self.health_solves[k] += R
        self.health_fail[k] += n_failed.to(torch.int32)
        bit = torch.where(failed, torch.bitwise_left_shift(one, torch.where((status >= 1) & (status <= 29), status, other)), zero)
        mask = bit[:, 0]
        for i in range(1, R):
            mask = mask | bit[:, i]
        self.health_status[k] |= mask
        if out.get("flags") is not None:
            self.health_waived[k] += (~failed & ((out["flags"].reshape(B, R) & 1) != 0)).sum(1).to(torch.int32)
        if out.get("iters") is not None:
            iters = out["iters"].reshape(B, R)
            self.health_iters[k] += iters.sum(1)
            self.health_iters_max[k].copy_(torch.maximum(self.health_iters_max[k], iters.amax(1).clamp(min=0)))
        self.health_first.copy_(torch.where((n_failed > 0) & (self.health_first == 0), self.hour_t + 1, self.health_first))

    # -- stochastic mode: backcast scenarios, bid curves from p_min, market clearing (semantics: rolling.py, generalised over the descriptor) --
    def _avail(self, m, offset=0):
        """wind availability of the window [B, T] and its sum accumulated in the order of t (the kernels' order: bit-identical constants)"""
        cols, _, per_kw = m.wind
        avail = m.kw() * self._window(self.cf_series, m.T, offset)
        total = avail[:, 0]
        for t in range(1, m.T):
            total = total + avail[:, t]
        return cols, avail, per_kw * total

    def _set_rows(self, m, da, rt):
        """objective, state, wind and objective constant of the B * S rows of a bidding model on prices da, rt [B * S, T]:
        c0 = (base_c0 - sum_t rt[t] PT_const[t]) + per_kw sum_t avail[t], both sums in the order of t; products rounded on their own"""
        m.c[:, m.term_cols] = m.base_c[m.term_cols] - m.term_coef * rt[:, m.term_t]
        m.c[:, m.pda_cols] = m.base_c[m.pda_cols] - (da - rt)
        if m.has_const:                               # (an all-zero PT_const leaves base_c0 - 0 = base_c0: the loop is skipped, the value is the same)
            psum = rt[:, 0] * m.PT_const[0]
            for t in range(1, m.T):
                psum = psum + rt[:, t] * m.PT_const[t]
            c0 = (m.base_c0_t if m.c0_plant is None else self._rows(m.c0_plant, m)) - psum
        else:
            c0 = m.base_c0_t.expand(rt.shape[0]) if m.c0_plant is None else self._rows(m.c0_plant, m)
        for j, col in enumerate(m.state_init):
            v = self._rows(self._st[:, j], m)
            m.lb[:, col] = v
            m.ub[:, col] = v
        if m.wind is not None:
            cols, avail, waste = self._avail(m)
            m.ub[:, cols] = self._rows(avail, m)
            c0 = c0 + self._rows(waste, m)
        m.c0.copy_(c0)

    def _set_tracker(self):
        """the tracker's LP on the cleared dispatch: dispatch rows = dispatch - PT_const, state, wind, c0 = base_c0 + per_kw sum_t avail[t]"""
        tr = self.tr
        rhs = self.rt_dispatch - tr.PT_const
        tr.rlo[:, tr.track_rows] = rhs
        tr.rhi[:, tr.track_rows] = rhs
        self._set_tracker_plant(tr, self.state)

    def _set_tracker_plant(self, m, state, offset=0):
        """the plant half of a tracker's LP: state columns fixed to state [B, n_state], wind bounds of the window that starts `offset`
        hours after the clock, c0 = base_c0 + per_kw sum_t avail[t]"""
        for j, col in enumerate(m.state_init):
            m.lb[:, col] = state[:, j]
            m.ub[:, col] = state[:, j]
        if m.wind is not None:
            cols, avail, waste = self._avail(m, offset)
            m.ub[:, cols] = avail
            m.c0.copy_((m.base_c0 if m.c0_plant is None else m.c0_plant) + waste)
        else:
            m.c0.fill_(m.base_c0)

    def _day_ahead_buffers(self, bid=False):
        """(offer, curve, count, prices) a day-ahead step writes: the current day's, or - the bid made at the RUC hour - the pending ones"""
        if bid:
            return self.pend_offer, self.pend_curve, self.pend_count, self.pend_prices
        return self.da_offer, self.da_curve, self.da_count, self.da_prices

    def _day_ahead_market(self, curves=None, bid=False):
        """the tail of every day-ahead step with curves: (U, M, count) of the day's 24 hours cleared at the realised day-ahead price and
        stored (None: the kernels have done that), then the day's sums - which, for a pending bid, wait for midnight"""
        if curves is not None:
            offer, curve, cnt, prices = self._day_ahead_buffers(bid)
            realised = self._window(self.da_series, 24)
            offer.copy_(self._clear(*curves, realised))
            prices.copy_(realised)
            self._store_curves(curve, cnt, *curves)
        if not bid:
            self._account_day_ahead()

    def _day_ahead_step_stochastic(self, bid=False):
        """B * S day-ahead LPs (row b * S + i on scenario i's prices, plant b's state and wind, day_ahead_power free), one curve per
        plant-hour from the S day_ahead_power values and day-ahead forecasts, cleared at the realised day-ahead price.
        bid: the bid made at the RUC hour for the next day - clock and state are the bid's (self._clk / self._st), the real-time
        history is one day older, and offers, prices, curves and counts go to the pending buffers; the day's sums wait for midnight"""
        m, B, S = self.da, self.B, self.S
        if self.use_fused:
            self._market_prepare(self._mk_da, -1, bid)
            m.solve(B * S)
            self._health_book("day_ahead", m, S)
            self._market_clear(self._mk_da, None, -1, 24, *self._day_ahead_buffers(bid)[:3], bid=bid)
            return self._day_ahead_market(None, bid)
        da = self._forecast(self.da_series, m.T, 0).expand(B, S, m.T)
        rt = self._forecast(self.rt_series, m.T, 0, lag_days=int(bid)).expand(B, S, m.T)
        self._set_rows(m, da.reshape(B * S, m.T), rt.reshape(B * S, m.T))
        self._free_day_ahead_power(m)
        out = m.solve(B * S)
        self._health_book("day_ahead", m, S)
        self._check(out)
        power = out["x"][:, m.pda_cols[:24]].reshape(B, S, 24)
        self._day_ahead_market(self._curves(power, self._forecast(self.da_series, 24, 0), out["status"]), bid)

    def _hour_step_bid(self, k):
        """Hour k of the day with a bidding LP and a curve - the stochastic mode's B * S real-time LPs, or the B of a self-schedule,
        which bids on scenario 0 alone (the most recent backcast day; inside the cleared day the coupled hourly problem separates):
        scenario i = the real-time backcast at hour-of-day k; realised day-ahead prices and the cleared day_ahead_power inside the cleared
        day; one curve per plant and tracked period from the pairs (P_T, real-time forecast) - a schedule: the one pair (P_T, 0) -,
        cleared at the realised price for the hour at hand and at scenario 0's forecast for the look-ahead periods; tracking of the
        cleared dispatch (B LPs); state hand-off, revenue and clock as _hour_step."""
        import torch
        m, tr, B = self.rt, self.tr, self.B
        per = m.per_plant or self.S                                       # rows per plant
        hour = k if self.simplex_warm else None
        if self.use_fused:
            self._market_prepare(self._mk_rt, k)
            m.solve(B * per, hour=hour)
            self._health_book("real_time", m, per)
            self._market_clear(self._mk_rt, self._loop_tr, k, tr.T, self.rt_dispatch, self.rt_curve, self.rt_count)
            tr.solve(B, hour=hour)
            self._health_book("tracking", tr, 1)
            self._fused(2, k)                         # delivered power, state hand-off, revenue, energy, clock: unchanged (reads the tracker only)
            return
        rt_f = self._forecast(self.rt_series, m.T, k)[:, :per].expand(B, per, m.T)
        da_f = self._forecast(self.da_series, m.T, k)[:, :per].expand(B, per, m.T).clone()
        known = min(m.T, 24 - k)                                          # hours of the horizon inside the cleared day
        da_f[:, :, :known] = self.da_prices[:, None, k:k + known]
        self._set_rows(m, da_f.reshape(B * per, m.T), rt_f.reshape(B * per, m.T))
        self._free_day_ahead_power(m, k, per)
        out = m.solve(B * per, hour=hour)
        self._health_book("real_time", m, per)
        self._check(out)
        x, Tc = out["x"], tr.T
        power = (x[:, m.pt_a[:Tc]] * m.pt_ca[:Tc] + x[:, m.pt_b[:Tc]] * m.pt_cb[:Tc]) + m.PT_const[:Tc]      # two-term elementwise form, not a matmul
        if self.self_schedule:
            U, M, count = self._schedule_curves(power, out["status"])
        else:
            U, M, count = self._curves(power.reshape(B, per, Tc), rt_f[:, :, :Tc], out["status"])
        rt0 = self._window(self.rt_series, 1)
        self.rt_dispatch.copy_(self._clear(U, M, count, torch.cat([rt0, rt_f[:, 0, 1:Tc]], dim=1)))
        self._store_curves(self.rt_curve, self.rt_count, U, M, count)
        self._set_tracker()
        out = tr.solve(B, hour=hour)
        self._health_book("tracking", tr, 1)
        self._check(out)
        self._hand_off(out["x"], rt0[:, 0], k, exact=self.exact)

    # -- past_midnight="coupled": the last T_rt - 1 hours of a day tie their look-ahead periods across the price scenarios ---------------------
    def _tied_blocks(self, k):
        """the S blocks of the B coupled real-time rows at hour k: block i of row b is what _set_rows / _free_day_ahead_power(m, k, S) give
        row b * S + i of the stochastic mode's real-time batch, c0[b] = sum_i c0(b, i) in the order of i; the monotone Bidder's pair rows
        follow the order of the hour's REAL-TIME scenario prices in every period (CoupledScenarioModel.load(energy_prices=rt))
        -> the real-time scenario prices [B, S, T]"""
        import torch
        m, blk, B, S = self.rtc, self.rt_block, self.B, self.S
        rt_f = self._forecast(self.rt_series, m.T, k).expand(B, S, m.T)
        da_f = self._forecast(self.da_series, m.T, k).expand(B, S, m.T).clone()
        known = 24 - k
        da_f[:, :, :known] = self.da_prices[:, None, k:k + known]
        self._set_rows(blk, da_f.reshape(B * S, m.T), rt_f.reshape(B * S, m.T))
        self._free_day_ahead_power(blk, k, S)
        each = blk.c0.view(B, S)
        total = each[:, 0]
        for i in range(1, S):
            total = total + each[:, i]
        m.c0.copy_(total)
        if self.monotone:
            zero, below, above = self._rtc_side
            d = (rt_f[:, self._rtc_pair_k, :] - rt_f[:, self._rtc_pair_j, :]).reshape(B, -1)      # [B, P * T]: pair p, period t at p * T + t
            rows = slice(m.first_coupling_row, m.first_coupling_row + d.shape[1])
            m.rlo[:, rows] = torch.where(d > 0, zero, below)
            m.rhi[:, rows] = torch.where(d < 0, zero, above)
        return rt_f

    def _tied_record(self):
        """a recorded late hour: the recorder reads the real-time batch's buffers, so the coupled solve is handed to them - rt_x the
        blocks (a self-schedule: block 0), rt_status the plant's one status on all its rows, rt_obj block i's c . x, rt_c0 the coupled
        constant in the plant's first row and 0 in the others"""
        m, rt, B, S = self.rtc, self.rt, self.B, self.S
        per = rt.per_plant or S
        x, c = m.out["x"].view(B, S, m.n1)[:, :per], m.c.view(B, S, m.n1)[:, :per]
        rt.out["x"].view(B, per, m.n1).copy_(x)
        rt.out["obj"].view(B, per).copy_((c * x).sum(2))
        rt.out["status"].view(B, per).copy_(m.out["status"][:, None].expand(B, per))
        rt.c0.zero_()
        rt.c0.view(B, per)[:, 0] = m.c0

    def _hour_step_past_midnight(self, k):
        """Hour k of the day with past_midnight="coupled".  While the whole horizon lies inside the cleared day (24 - k >= T_rt) every
        day_ahead_power column is fixed, the coupled problem separates and the step is _hour_step_bid's, unchanged.  In the last T_rt - 1
        hours the look-ahead periods past midnight have a free day_ahead_power, which the host bidders tie across the scenarios
        (workflow/bidder.py::compute_real_time_bids on CoupledScenarioModel): B coupled LPs (_tied_blocks) instead of B * S / B
        independent ones, on a handle whose warm-start chain begins at the first such hour of the day.  Curves: block i's P_T[t] and
        scenario i's real-time forecast, the plant's one status standing for its S pairs (a self-schedule: the one pair (block 0's
        P_T[t], 0)); clearing, tracking and hand-off as _hour_step_bid."""
        import torch
        if not self._tied_hour(k):
            return self._hour_step_bid(k)
        m, tr, B, S = self.rtc, self.tr, self.B, self.S
        hour = k if self.simplex_warm else None
        first = (k - self._first_tied_hour) if self.simplex_warm else None        # 0: the slack basis / cold point, then hour k - 1's
        if self.use_fused:
            import ctypes as C
            bounds = (C.c_void_p(m.rlo.data_ptr()), C.c_void_p(m.rhi.data_ptr())) if self.monotone else (None, None)
            self._call(self._lib.dsp_loop_midnight_prepare, C.byref(self._mk_coupled if self.monotone else self._mk_sched), C.byref(self._mk_rtc),
                       *bounds, m.lp.m, m.first_coupling_row, k)
            m.solve(B, hour=first)
            self._health_book("real_time", m, 1)
            if self._rec is not None:
                self._tied_record()
            self._market_clear(self._mk_rtc, self._loop_tr, k, tr.T, self.rt_dispatch, self.rt_curve, self.rt_count,
                               state=self._mk_coupled if self.monotone else self._mk_state)
            tr.solve(B, hour=hour)
            self._health_book("tracking", tr, 1)
            self._fused(2, k)
            return
        rt_f = self._tied_blocks(k)
        out = m.solve(B, hour=first)
        self._health_book("real_time", m, 1)
        self._check(out)
        if self._rec is not None:
            self._tied_record()
        rt, Tc = self.rt, tr.T
        x = out["x"].reshape(B * S, m.n1)              # block i of row b: the block-relative columns
        power = ((x[:, rt.pt_a[:Tc]] * rt.pt_ca[:Tc] + x[:, rt.pt_b[:Tc]] * rt.pt_cb[:Tc]) + rt.PT_const[:Tc]).view(B, S, Tc)
        if self.self_schedule:
            U, M, count = self._schedule_curves(power[:, 0], out["status"])
        else:
            U, M, count = self._curves(power, rt_f[:, :, :Tc], out["status"].repeat_interleave(S))
        rt0 = self._window(self.rt_series, 1)
        self.rt_dispatch.copy_(self._clear(U, M, count, torch.cat([rt0, rt_f[:, 0, 1:Tc]], dim=1)))
        self._store_curves(self.rt_curve, self.rt_count, U, M, count)
        self._set_tracker()
        out = tr.solve(B, hour=hour)
        self._health_book("tracking", tr, 1)
        self._check(out)
        self._hand_off(out["x"], rt0[:, 0], k, exact=self.exact)

    # -- self-scheduling: one coupled day-ahead LP per plant, the schedule offered at cost 0 (module docstring); its hours: _hour_step_bid --
    def _schedule_curves(self, power, status):
        """power [B, Tc] MW, status [B] -> the curves of the ONE pair (power, 0 $/MWh) per plant and period (plant_curves with S = 1)"""
        import torch
        return self._curves(power[:, None, :], torch.zeros_like(power)[:, None, :], status)

    def _coupled_blocks(self):
        """the S blocks of the B coupled day-ahead rows: block i of row b on scenario i's backcast prices, plant b's state and wind,
        day_ahead_power free (what _set_rows gives row b * S + i), and c0[b] = sum_i c0(b, i) in the order of i
        -> the day-ahead scenario prices [B, S, T]"""
        m, blk, B, S = self.da, self.da_block, self.B, self.S
        da = self._forecast(self.da_series, m.T, 0).expand(B, S, m.T)
        rt = self._forecast(self.rt_series, m.T, 0).expand(B, S, m.T)
        self._set_rows(blk, da.reshape(B * S, m.T), rt.reshape(B * S, m.T))
        self._free_day_ahead_power(blk)
        each = blk.c0.view(B, S)
        total = each[:, 0]
        for i in range(1, S):
            total = total + each[:, i]
        m.c0.copy_(total)
        return da

    def _day_ahead_step_self_schedule(self):
        """B coupled day-ahead LPs (_coupled_blocks), tied by the static coupling rows.  The schedule - block 0's day_ahead_power - is
        offered at cost 0 and cleared at the realised day-ahead price."""
        import ctypes as C
        m, B = self.da, self.B
        if self.use_fused:
            self._call(self._lib.dsp_loop_schedule_prepare, C.byref(self._mk_sched), C.byref(self._mk_da))
            m.solve(B)
            self._health_book("day_ahead", m, 1)
            self._market_clear(self._mk_da, None, -1, 24, *self._day_ahead_buffers()[:3])
            return self._day_ahead_market()
        self._coupled_blocks()
        out = m.solve(B)
        self._health_book("day_ahead", m, 1)
        self._check(out)
        self._day_ahead_market(self._schedule_curves(out["x"][:, m.pda_cols[:24]], out["status"]))      # (block 0: the block-relative columns)

    # -- monotone bid curves: one coupled day-ahead LP per plant, its S pairs per hour ordered by the LP itself (module docstring) --------
    def _day_ahead_step_monotone(self):
        """B coupled day-ahead LPs (_coupled_blocks), tied by the ordered-pair rows pda[k, t] - pda[j, t] of m.pairs, row
        first_coupling_row + p * T + t: with d = da[k, t] - da[j, t] of plant b's day-ahead scenario prices, rlo = 0 if d > 0 else -inf,
        rhi = 0 if d < 0 else +inf (CoupledScenarioModel.load).  One curve per plant-hour from block i's day_ahead_power and scenario
        i's day-ahead forecast, cleared at the realised day-ahead price; the status of plant b's one solve stands for its S pairs."""
        import ctypes as C
        import torch
        m, B, S = self.da, self.B, self.S
        if self.use_fused:
            self._call(self._lib.dsp_loop_monotone_prepare, C.byref(self._mk_coupled), C.byref(self._mk_da), C.c_void_p(m.rlo.data_ptr()),
                       C.c_void_p(m.rhi.data_ptr()), m.lp.m, m.first_coupling_row)
            m.solve(B)
            self._health_book("day_ahead", m, 1)
            self._market_clear(self._mk_da, None, -1, 24, *self._day_ahead_buffers()[:3], state=self._mk_coupled)
            return self._day_ahead_market()
        da = self._coupled_blocks()
        if not hasattr(self, "_pair_j"):              # (persistent operands: a captured step creates no tensor from host data)
            at = lambda v: torch.as_tensor(v, dtype=torch.int64, device=self.dev)
            self._pair_j, self._pair_k = at([j for j, _ in m.pairs]), at([k for _, k in m.pairs])
            self._side = tuple(torch.full((), v, dtype=torch.float64, device=self.dev) for v in (0.0, float("-inf"), float("inf")))
        zero, below, above = self._side
        d = (da[:, self._pair_k, :] - da[:, self._pair_j, :]).reshape(B, -1)          # [B, P * T]: pair p, period t at p * T + t
        rows = slice(m.first_coupling_row, m.first_coupling_row + d.shape[1])
        m.rlo[:, rows] = torch.where(d > 0, zero, below)
        m.rhi[:, rows] = torch.where(d < 0, zero, above)
        out = m.solve(B)
        self._health_book("day_ahead", m, 1)
        self._check(out)
        power = out["x"].reshape(B, S, m.n1)[:, :, m.pda_cols[:24]]                  # block i: the block-relative columns
        self._day_ahead_market(self._curves(power, self._forecast(self.da_series, 24, 0), out["status"].repeat_interleave(S)))

    # -- parametrized mode: two-tier closed-form curves (workflow/parametrized_bidder.py), no bidding LP ---------------------------------
    def _param_curves(self, cf):
        """cf [B, Tc] capacity factors -> (U, M [4, B * Tc] int64 cents, count): the pairs (0, 0), (max(0, w - storage), 0), (p_max, bid)
        as three "scenarios" of plant_curves with p_min = 0"""
        import torch
        from .workflow.market import plant_curves
        w = cf * self.wind_mw
        storage = self.storage_mw[:, None]
        lo = torch.clamp(w - storage, min=0.0)
        hi = torch.maximum(w, storage.expand_as(w)) if self.battery else w
        zero = torch.zeros_like(w)
        power = torch.stack([zero, lo, hi]).reshape(3, -1)
        price = torch.stack([zero, zero, self.bid_price[:, None].expand_as(w)]).reshape(3, -1)
        return plant_curves(torch, power, price, torch.ones_like(power, dtype=torch.bool), p_min_cents=0)

    def _day_ahead_step_parametrized(self):
        """one curve per plant-hour from the day-ahead capacity factors, cleared at the realised day-ahead price; no LP"""
        if self.use_fused:
            self._param(0, -1)
            return self._day_ahead_market()
        self._day_ahead_market(self._param_curves(self._window(self.da_cf_series, 24)))

    def _param_dispatch(self, k):
        """the first half of hour k: curves of the tracked periods, their clearing, and the tracker's LP on the cleared dispatch"""
        if self.use_fused:
            self._param(1, k)
            return
        tr = self.tr
        U, M, count = self._param_curves(self._window(self.cf_series, tr.T))
        self.rt_dispatch.copy_(self._clear(U, M, count, self._window(self.rt_series, tr.T)))
        self._store_curves(self.rt_curve, self.rt_count, U, M, count)
        self._set_tracker()

    def _param_hydrogen(self, k):
        """h2_kg += MultiPeriodWindPEM._h2_kg_per_hr(PEM electricity of the implemented hour) (a tensor divisor: cf. clear_curves)"""
        if self.h2_kg is None:
            return
        if self.use_fused:
            self._param(2, k)
        else:
            self.h2_kg += ((self.tr.out["x"][:, self.pem_col] * self._h2_mul) / self._h2_div) * 3600.0

    def _hour_step_parametrized(self, k):
        """Hour k of the day: one curve per plant and tracked period from the real-time capacity factors, cleared at the real-time price
        of that period (the perfect forecast IS the realised price; the day-ahead dispatch plays no part, as in the reference); tracking
        of the cleared dispatch (B LPs); hydrogen of the implemented hour; state hand-off, revenue and clock as _hour_step."""
        tr, B = self.tr, self.B
        hour = k if self.simplex_warm else None
        self._param_dispatch(k)
        out = tr.solve(B, hour=hour)
        self._health_book("tracking", tr, 1)
        self._param_hydrogen(k)
        if self.use_fused:
            self._fused(2, k)                         # delivered power, state hand-off, revenue, energy, clock: unchanged (reads the tracker only)
            return
        self._check(out)
        self._hand_off(out["x"], self._window(self.rt_series, 1)[:, 0], k, exact=True)

    # -- bidding at the RUC hour (ruc_hour=H): projection tracker, pending bid, activation at midnight ----------------------------------
    def _ruc_setup(self, pj):
        """the projection tracker (a _Model of its own on the tracker's template: own buffers, own handle, own simplex basis - the
        reference keeps a separate Tracker object for the same reason), the trace of its last chain, the pending bid, the bid clock"""
        import torch
        B, dev, L, ns = self.B, self.dev, 24 - self.ruc_hour, len(self.scale)
        self.pj = pj
        pj.track_rows, pj.state_real = self.tr.track_rows, self.tr.state_real
        pj.kw_plant, pj.c0_plant = self.tr.kw_plant, self.tr.c0_plant      # per-plant sizes: the tracker's arrays (read only)
        for name in ("lb", "ub", "rlo", "rhi"):                            # ... and its static battery bounds
            getattr(pj, name).copy_(getattr(self.tr, name))
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        self.proj_state, self.proj_real, self.proj_obj = z(L + 1, B, ns), z(L, B, ns), z(L, B)
        self.pend_offer, self.pend_prices = z(B, 24), z(B, 24)
        self.bid_hour_t = torch.zeros((), dtype=torch.int64, device=dev)   # the bid clock: hour 0 of the day the pending bid is for
        self._zeroed += [self.proj_state, self.proj_real, self.proj_obj, self.pend_offer, self.pend_prices, self.bid_hour_t]
        if self.stochastic:
            self.pend_curve, self.pend_count = torch.zeros_like(self.da_curve), torch.zeros_like(self.da_count)
            self._zeroed += [self.pend_curve, self.pend_count]

    def _project_write(self, j):
        """the projection tracker's LP of chain step j (the window that starts at clock + j): dispatch rows inside the day on the
        current day-ahead dispatch, rows past midnight free on both sides (Tracker._pass_market_dispatch on a short list), state
        columns fixed to proj_state[j], wind and c0 of the window (_set_tracker_plant)"""
        if self.use_fused:
            self._project(0, j)
            return
        pj, H = self.pj, self.ruc_hour
        if j == 0:
            self.proj_state[0].copy_(self.state)
        known = min(pj.T, 24 - H - j)
        rhs = self.da_offer[:, H + j:H + j + known] - pj.PT_const[:known]
        pj.rlo[:, pj.track_rows[:known]] = rhs
        pj.rhi[:, pj.track_rows[:known]] = rhs
        if known < pj.T:
            pj.rlo[:, pj.track_rows[known:]] = float("-inf")
            pj.rhi[:, pj.track_rows[known:]] = float("inf")
        self._set_tracker_plant(pj, self.proj_state[j], offset=j)

    def _project_hand_off(self, j, out):
        import torch
        if self.use_fused:
            self._project(1, j)
            return
        self._check(out)
        for e, col in enumerate(self.pj.state_real):
            real = out["x"][:, col]
            self.proj_real[j, :, e] = real
            self.proj_state[j + 1, :, e] = torch.round(real * self.scale[e]) / self._scale_t[e]
        self.proj_obj[j].copy_(out["obj"] + self.pj.c0)

    def _ruc_step(self):
        """hour H of day d, before that hour's real-time step: the projection chain to midnight (flowsheets with state), then the
        day-ahead bid of day d + 1 on the projected state, into the pending buffers"""
        import torch
        pj, B, H = self.pj, self.B, self.ruc_hour
        if len(self.scale):
            for j in range(24 - H):
                self._project_write(j)
                hour = (0 if j == 0 else 1) if self.simplex_warm else None         # step 0 from the slack basis, then from the step before
                out = pj.solve(B, hour=hour)
                self._health_book("projection", pj, 1)
                self._project_hand_off(j, out)
        torch.add(self.hour_t, 24 - H, out=self.bid_hour_t)
        self._clk, self._st = self.bid_hour_t, self.proj_state[-1]
        try:
            self._da_step(bid=True)
        finally:
            self._clk, self._st = self.hour_t, self.state

    def _activate(self):
        """midnight: the pending bid becomes the current one (DoubleLoopCoordinator.activate_pending_DA_bids)"""
        if self.use_fused:
            self._project(2, 0)
        else:
            self.da_offer.copy_(self.pend_offer)
            self.da_prices.copy_(self.pend_prices)
            if self.stochastic:
                self.da_curve.copy_(self.pend_curve)
                self.da_count.copy_(self.pend_count)
        if self.stochastic:
            self._account_day_ahead()

    # -- the loop (run_day: _DeviceLoop; the mode's steps and solve counts were bound by __init__) -------------------------------------------
    def day_ahead(self):
        self.day_start = self.hour
        if self._pending:                              # ruc_hour, day d >= 1: nothing to solve, yesterday's bid takes over
            self._run("activate", self._activate)
            self._pending = False
            return self.da_offer.clone()
        # A coupled LP (self-schedule, monotone bid curves) beyond the register / LDS-resident kernels (wind + battery: 582 columns, 408 rows at 24 h) runs in
        # the solver's HBM-resident streaming form, which is driven from the host (it polls the scenarios' completion between check
        # periods): it cannot be a node of a captured graph, and the step stays eager, once per simulated day.  A coupled LP that stays
        # in the fused kernels (nuclear, wind + PEM at S = 3) is captured and replayed like the stochastic mode's.  Which of the two a
        # handle is, the first - eager - day's solve reports (dsp_stats::streaming).
        if self.coupled_da and self._da_capturable is None and self._warm:
            self._da_capturable = self.use_graphs and not self.da.dlp.last_stats.streaming
        if self.coupled_da and not self._da_capturable:
            self._da_step()
        else:
            self._run("da", self._da_step)
        self.solves += self._n_da
        if self._rec is not None:
            self._rec.days_bid = max(self._rec.days_bid, self.hour // 24 + 1)
        return self.da_offer.clone()

    def hour_step(self):
        k = self.hour - self.day_start
        if k == self.ruc_hour:                         # the projection chain and tomorrow's bid in front of this hour's step
            self._run(k, lambda: (self._ruc_step(), self._hour(k)))
            self.solves += self._n_da + (self.B * (24 - k) if len(self.scale) else 0)
            self._pending = True
            if self._rec is not None:                  # the bid of the next day sits in its daily row
                self._rec.days_bid = max(self._rec.days_bid, self.hour // 24 + 2)
        elif self._tied_hour(k):
            # a coupled hourly LP that the solver streams is driven from the host, like such a day-ahead LP (day_ahead): its step stays
            # eager.  The first - eager - day's solve reports which of the two the handle is (dsp_stats::streaming).
            if self._rtc_capturable is None and self._warm:
                self._rtc_capturable = self.use_graphs and not self.rtc.dlp.last_stats.streaming
            if self._rtc_capturable:
                self._run(k, lambda: self._hour(k))
            else:
                self._hour(k)
        else:
            self._run(k, lambda: self._hour(k))
        self.solves += 2 * self.B if self._tied_hour(k) else self._n_hour
        self.hour += 1
        return self.delivered.clone()

    def reset(self):
        for t in self._zeroed:
            t.zero_()
        self._pending = False
        self.hour = self.solves = 0
        if self._rec is not None:
            self._rec.reset()

    def recorded(self):
        """-> dict of host arrays [hours or days run, plants, ...] of the record (record=... at construction; keys: __init__'s docstring),
        and `plants`"""
        if self._rec is None:
            raise RuntimeError("this loop records nothing: construct it with record=(plants, days)")
        return self._rec.recorded()

    def write_results(self, path, start_date="2020-01-02"):
        """the reference's bidder_detail.csv, bidding_model_detail.csv, tracker_detail.csv and tracking_model_detail.csv of every recorded
        plant, in path/plant_<index>/, hour 0 of the run being hour 0 of start_date (loop_record.write_results)"""
        from .loop_record import write_results
        if self._rec is None:
            raise RuntimeError("this loop records nothing: construct it with record=(plants, days)")
        write_results(self, path, start_date)

    def results(self):
        """-> (dict of per-plant device tensors, ok): obj / energy_mwh / state, the mode's sums, the ledger's rows and profit (ledger=True),
        and with health=True failed_solves, uncertified_solves, first_failure_hour (int64, -1: none) and valid = failed_solves == 0 [B].
        From first_failure_hour on, a plant with valid == False ran on a bid whose failed rows were dropped, or on an unconverged LP.
        ok: no LP of any plant ended with a status other than 0."""
        res = dict(obj=self.revenue, energy_mwh=self.energy_mwh, state=self.state)
        res.update((key, getattr(self, key)) for key in self._result_keys)
        if self.ledger:
            res.update((key, self.ledger_acc[f]) for f, key in enumerate(self.ledger_keys))
            res["profit"] = self.revenue - res["tot_cost"]
        return res, not bool(self.bad.item())

