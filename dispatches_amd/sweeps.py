"""Parameter sweeps of the parametrized double loop as ONE batch.

The reference runs its wind + PEM study (run_double_loop_PEM.py, `sweep_design_*`) as one Prescient job per (--pem_bid, --pem_pmax)
point.  In the device double loop (rolling_flowsheets.py::BatchedDoubleLoop with bidder="parametrized") a whole
(bid price x storage size x price window) grid is one batch of plants: every window carries the full grid through `plant_windows`,
bidding is arithmetic, and only the tracking LPs are solved.

The wind + battery study (run_double_loop_battery.py: --wind_pmax, --battery_pmax, --battery_energy_capacity, one Prescient job per size
point of new_wind_battery_ratio_duration_sweep_sb) bids with the stochastic LP Bidder: `design_sweep` runs a (wind size x battery power
x duration x price window) grid as one batch of DIFFERENT plants through BatchedDoubleLoop's wind_mw / battery_mw / battery_mwh."""
from __future__ import annotations

import numpy as np


def grid_layout(bid_prices, storage_mws, n_windows):
    """-> (bid_price [B], storage_mw [B], plant_windows [B]) of the grid flattened in C order: plant (i, j, w) -> (i * J + j) * W + w"""
    bid_prices, storage_mws = np.asarray(bid_prices, np.float64).ravel(), np.asarray(storage_mws, np.float64).ravel()
    if len(bid_prices) < 1 or len(storage_mws) < 1 or int(n_windows) < 1:
        raise ValueError("a sweep needs at least one bid price, one storage size and one window")
    bid, sto, win = np.meshgrid(bid_prices, storage_mws, np.arange(int(n_windows)), indexing="ij")
    return bid.ravel(), sto.ravel(), win.ravel().astype(np.int64)


def _ledger_outputs(loop, res, shape):
    """the ledger's sums and the profit of a loop run with ledger=True, shaped like a sweep's other outputs"""
    return {key: res[key].cpu().numpy().reshape(shape).copy() for key in list(loop.ledger_keys) + ["profit"]}


def _health_outputs(res, shape):
    """the per-plant solve health of a loop run with health=True, shaped like a sweep's other outputs: which grid points' numbers can be
    trusted (valid), how many of their LP rows failed, and from which simulated hour on (-1: never)"""
    return {key: res[key].cpu().numpy().reshape(shape).copy() for key in ("valid", "failed_solves", "first_failure_hour")}


def _want_profiles(representative_days, n_days, loop_kw):
    """representative_days checked before anything runs; the loop then keeps the sweep's day profiles"""
    if representative_days is None:
        return
    if isinstance(representative_days, (int, np.integer)) and not isinstance(representative_days, bool):
        if not 1 <= representative_days <= 64:
            raise ValueError(f"representative_days: K is in 1 .. 64, not {representative_days}")
    else:
        centers = np.asarray(representative_days, np.float64)
        if centers.ndim != 2 or centers.shape[1] not in (24, 48) or not 1 <= centers.shape[0] <= 64:
            raise ValueError(f"representative_days is a number of clusters K or centres [K, 24] / [K, 48] with K in 1 .. 64, not an array of shape {list(centers.shape)}")
    loop_kw.setdefault("profiles", int(n_days))


def _representative_days(loop, representative_days, shape):
    """the second label of the reference's market surrogates for a loop run with profiles= (representative_days.py): an int K fits K
    representative days on the sweep's own days (seed 42, k-means++), a centre array [K, 24] or [K, 48] only labels.  One channel
    (dispatch) for the nuclear flowsheet, two (dispatch and the day's capacity factors) for the wind flowsheets, as in the reference,
    unless a centre array says otherwise.  -> dispatch_frequency, grid shape + (K + 2,) = [zero days, days at centre 0 .. K - 1, full
    days] / days, and day_centers [K, 24 * channels]"""
    from .representative_days import DayPoints
    if isinstance(representative_days, (int, np.integer)) and not isinstance(representative_days, bool):
        points = DayPoints(loop, channels=1 if loop.flowsheet == "nuclear" else 2)
        centers = points.fit(int(representative_days)).centers
    else:
        centers = np.asarray(representative_days, np.float64)
        points = DayPoints(loop, channels=centers.shape[1] // 24)
    freq = points.frequency(centers).cpu().numpy()
    return {"dispatch_frequency": freq.reshape(tuple(shape) + (freq.shape[1],)).copy(), "day_centers": np.array(centers)}


def parametrized_sweep(flowsheet, bid_prices, storage_mws, n_windows, n_days, device=0, market="price_taker", lp_backend=None, ledger=False,
                       health=False, representative_days=None, **loop_kw):
    """Runs `n_days` simulated days of the (bid price x storage size x window) grid of `flowsheet` ("wind_pem" or "wind_battery").
    -> dict of numpy arrays shaped [len(bid_prices), len(storage_mws), n_windows]: revenue, energy_mwh (delivered), da_energy_mwh
    (cleared day-ahead), offered_mwh (the day-ahead curves' last points), h2_kg (wind + PEM only); and all_optimal (bool).
    ledger=True: also the loop's ledger (BatchedDoubleLoop(ledger=True): tot_cost, under_mwh, over_mwh, curtailed_mwh, pem_mwh for
    wind + PEM) and profit = revenue - tot_cost, same shape.
    health=True: also valid (bool), failed_solves and first_failure_hour (-1: none) of every grid point (BatchedDoubleLoop(health=True)),
    same shape: all_optimal == False no longer condemns the whole sweep.
    representative_days=K or centres: the loop keeps every plant's day profiles (BatchedDoubleLoop(profiles=n_days)) and the sweep also
    returns dispatch_frequency, shape + (K + 2,), and day_centers (_representative_days): with revenue, the two labels the reference's
    market surrogates are trained on."""
    from .rolling_flowsheets import BatchedDoubleLoop
    _want_profiles(representative_days, n_days, loop_kw)
    bid, sto, win = grid_layout(bid_prices, storage_mws, n_windows)
    shape = (len(np.ravel(bid_prices)), len(np.ravel(storage_mws)), int(n_windows))
    loop = BatchedDoubleLoop(flowsheet, len(bid), device=device, lp_backend=lp_backend, bidder="parametrized", bid_price=bid, storage_mw=sto,
                             plant_windows=win, market=market, ledger=ledger, health=health, **loop_kw)
    for _ in range(int(n_days)):
        loop.run_day()
    res, ok = loop.results()
    out = {name: res[key].cpu().numpy().reshape(shape).copy()
           for name, key in (("revenue", "obj"), ("energy_mwh", "energy_mwh"), ("da_energy_mwh", "da_energy_mwh"), ("offered_mwh", "offered_mwh"),
                             ("h2_kg", "h2_kg")) if key in res}
    if ledger:
        out.update(_ledger_outputs(loop, res, shape))
    if health:
        out.update(_health_outputs(res, shape))
    if representative_days is not None:
        out.update(_representative_days(loop, representative_days, shape))
    out["all_optimal"] = bool(ok)
    return out


def design_layout(wind_mws, battery_mws, durations_h, n_windows):
    """-> (wind_mw [B], battery_mw [B], battery_mwh [B], plant_windows [B]) of the grid flattened in C order with the window axis last
    (the rule of grid_layout): plant (i, j, d, w) -> ((i * J + j) * D + d) * W + w;  battery_mwh = battery_mw * duration_h"""
    axes = [np.asarray(a, np.float64).ravel() for a in (wind_mws, battery_mws, durations_h)]
    if min(len(a) for a in axes) < 1 or int(n_windows) < 1:
        raise ValueError("a sweep needs at least one wind size, one battery size, one duration and one window")
    wind, batt, dur, win = np.meshgrid(*axes, np.arange(int(n_windows)), indexing="ij")
    return wind.ravel(), batt.ravel(), (batt * dur).ravel(), win.ravel().astype(np.int64)


def design_sweep(flowsheet, wind_mws, battery_mws, durations_h, n_windows, n_days, n_price_scenarios=1, forecaster="perfect",
                 market="price_taker", device=0, lp_backend=None, ledger=False, health=False, representative_days=None, **loop_kw):
    """Runs `n_days` simulated days of the (wind MW x battery MW x duration h x window) grid of `flowsheet` with the LP bidder, every grid
    point a plant of its own size.  "wind_battery": all axes; "wind_pem": the wind axis only - battery_mws and durations_h must have
    length 1 and are not used (pass [0.0], [0.0]).  -> dict of numpy arrays shaped [len(wind_mws), len(battery_mws), len(durations_h),
    n_windows]: revenue, energy_mwh (delivered), da_energy_mwh and offered_mwh (where the mode has them: not the deterministic loop,
    forecaster="perfect" with market="stub"), throughput_kwh (wind_battery: the final accumulated battery throughput); and all_optimal.
    ledger=True: also the loop's ledger (tot_cost - degradation, fixed O&M and curtailment penalty of the implemented hours, the
    reference's "Total Cost [$]" -, under_mwh, over_mwh, curtailed_mwh; wind_pem: h2_kg, pem_mwh) and profit = revenue - tot_cost, same
    shape: what ranks designs, where revenue alone always prefers the larger battery.
    health=True: also valid, failed_solves and first_failure_hour of every grid point, same shape (parametrized_sweep).
    representative_days=K or centres: also dispatch_frequency, shape + (K + 2,), and day_centers (parametrized_sweep)."""
    from .rolling_flowsheets import BatchedDoubleLoop
    _want_profiles(representative_days, n_days, loop_kw)
    wind, batt, mwh, win = design_layout(wind_mws, battery_mws, durations_h, n_windows)
    shape = tuple(len(np.ravel(a)) for a in (wind_mws, battery_mws, durations_h)) + (int(n_windows),)
    if flowsheet == "wind_pem":
        if shape[1] != 1 or shape[2] != 1:
            raise ValueError("wind_pem has no battery: the battery and duration axes of its sweep must have length 1")
        sizes = dict(wind_mw=wind)
    else:
        sizes = dict(wind_mw=wind, battery_mw=batt, battery_mwh=mwh)
    loop = BatchedDoubleLoop(flowsheet, len(wind), device=device, lp_backend=lp_backend, n_price_scenarios=n_price_scenarios, forecaster=forecaster,
                             market=market, plant_windows=win, ledger=ledger, health=health, **sizes, **loop_kw)
    for _ in range(int(n_days)):
        loop.run_day()
    res, ok = loop.results()
    out = {name: res[key].cpu().numpy().reshape(shape).copy()
           for name, key in (("revenue", "obj"), ("energy_mwh", "energy_mwh"), ("da_energy_mwh", "da_energy_mwh"), ("offered_mwh", "offered_mwh"))
           if key in res}
    if flowsheet == "wind_battery":
        out["throughput_kwh"] = res["state"][:, 1].cpu().numpy().reshape(shape).copy()
    if ledger:
        out.update(_ledger_outputs(loop, res, shape))
    if health:
        out.update(_health_outputs(res, shape))
    if representative_days is not None:
        out.update(_representative_days(loop, representative_days, shape))
    out["all_optimal"] = bool(ok)
    return out


def nuclear_layout(h2_prices, pem_mws, n_windows):
    """-> (h2_price [B], pem_mw [B], plant_windows [B]) of the grid flattened in C order with the window axis last (the rule of
    design_layout): plant (i, j, w) -> (i * J + j) * W + w"""
    axes = [np.asarray(a, np.float64).ravel() for a in (h2_prices, pem_mws)]
    if min(len(a) for a in axes) < 1 or int(n_windows) < 1:
        raise ValueError("a sweep needs at least one hydrogen price, one PEM size and one window")
    price, pem, win = np.meshgrid(*axes, np.arange(int(n_windows)), indexing="ij")
    return price.ravel(), pem.ravel(), win.ravel().astype(np.int64)


def nuclear_sweep(h2_prices, pem_mws, n_windows, n_days, tank_kg=None, h2_demand=None, n_price_scenarios=3, forecaster="backcast",
                  market="price_taker", device=0, lp_backend=None, health=False, representative_days=None, **loop_kw):
    """Runs `n_days` simulated days of the (hydrogen price $/kg x PEM size MW x window) grid of the nuclear double loop as ONE batch, every
    grid point a plant with its own h2_price and pem_mw (the reference's study reports elec_rev, h2_rev, net_profit and pem_cap_factor
    over such a grid, nuclear_case/report/price_taker_analysis.py); tank_kg / h2_demand: scalars for all plants (None: the flowsheet's).
    The loop keeps its ledger.  -> dict of numpy arrays shaped [len(h2_prices), len(pem_mws), n_windows]: revenue (electricity), h2_revenue,
    tot_cost (operating cost minus hydrogen revenue), profit = revenue - tot_cost, energy_mwh, h2_kg, pem_capacity_factor = PEM MWh /
    (pem_mw * hours); and all_optimal.  health=True: also valid, failed_solves and first_failure_hour of every grid point, same shape
    (parametrized_sweep).  representative_days=K or centres: also dispatch_frequency, shape + (K + 2,), and day_centers
    (parametrized_sweep)."""
    from .rolling_flowsheets import BatchedDoubleLoop
    _want_profiles(representative_days, n_days, loop_kw)
    price, pem, win = nuclear_layout(h2_prices, pem_mws, n_windows)
    shape = (len(np.ravel(h2_prices)), len(np.ravel(pem_mws)), int(n_windows))
    loop = BatchedDoubleLoop("nuclear", len(price), device=device, lp_backend=lp_backend, n_price_scenarios=n_price_scenarios, forecaster=forecaster,
                             market=market, plant_windows=win, h2_price=price, pem_mw=pem, tank_kg=tank_kg, h2_demand=h2_demand, ledger=True,
                             health=health, **loop_kw)
    for _ in range(int(n_days)):
        loop.run_day()
    res, ok = loop.results()
    out = {name: res[key].cpu().numpy().reshape(shape).copy()
           for name, key in (("revenue", "obj"), ("h2_revenue", "h2_revenue"), ("tot_cost", "tot_cost"), ("profit", "profit"), ("energy_mwh", "energy_mwh"),
                             ("h2_kg", "h2_kg"))}
    out["pem_capacity_factor"] = res["pem_mwh"].cpu().numpy().reshape(shape) / (pem.reshape(shape) * float(loop.hour))
    if health:
        out.update(_health_outputs(res, shape))
    if representative_days is not None:
        out.update(_representative_days(loop, representative_days, shape))
    out["all_optimal"] = bool(ok)
    return out
