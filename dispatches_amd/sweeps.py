"""Parameter sweeps of the parametrized double loop as ONE batch.

The reference runs its wind + PEM study (run_double_loop_PEM.py, `sweep_design_*`) as one Prescient job per (--pem_bid, --pem_pmax)
point.  In the device double loop (rolling_flowsheets.py::BatchedDoubleLoop with bidder="parametrized") a whole
(bid price x storage size x price window) grid is one batch of plants: every window carries the full grid through `plant_windows`,
bidding is arithmetic, and only the tracking LPs are solved."""
from __future__ import annotations

import numpy as np


def grid_layout(bid_prices, storage_mws, n_windows):
    """-> (bid_price [B], storage_mw [B], plant_windows [B]) of the grid flattened in C order: plant (i, j, w) -> (i * J + j) * W + w"""
    bid_prices, storage_mws = np.asarray(bid_prices, np.float64).ravel(), np.asarray(storage_mws, np.float64).ravel()
    if len(bid_prices) < 1 or len(storage_mws) < 1 or int(n_windows) < 1:
        raise ValueError("a sweep needs at least one bid price, one storage size and one window")
    bid, sto, win = np.meshgrid(bid_prices, storage_mws, np.arange(int(n_windows)), indexing="ij")
    return bid.ravel(), sto.ravel(), win.ravel().astype(np.int64)


def parametrized_sweep(flowsheet, bid_prices, storage_mws, n_windows, n_days, device=0, market="price_taker", lp_backend=None, **loop_kw):
    """Runs `n_days` simulated days of the (bid price x storage size x window) grid of `flowsheet` ("wind_pem" or "wind_battery").
    -> dict of numpy arrays shaped [len(bid_prices), len(storage_mws), n_windows]: revenue, energy_mwh (delivered), da_energy_mwh
    (cleared day-ahead), offered_mwh (the day-ahead curves' last points), h2_kg (wind + PEM only); and all_optimal (bool)."""
    from .rolling_flowsheets import BatchedDoubleLoop
    bid, sto, win = grid_layout(bid_prices, storage_mws, n_windows)
    shape = (len(np.ravel(bid_prices)), len(np.ravel(storage_mws)), int(n_windows))
    loop = BatchedDoubleLoop(flowsheet, len(bid), device=device, lp_backend=lp_backend, bidder="parametrized", bid_price=bid, storage_mw=sto,
                             plant_windows=win, market=market, **loop_kw)
    for _ in range(int(n_days)):
        loop.run_day()
    res, ok = loop.results()
    out = {name: res[key].cpu().numpy().reshape(shape).copy()
           for name, key in (("revenue", "obj"), ("energy_mwh", "energy_mwh"), ("da_energy_mwh", "da_energy_mwh"), ("offered_mwh", "offered_mwh"),
                             ("h2_kg", "h2_kg")) if key in res}
    out["all_optimal"] = bool(ok)
    return out
