"""Time the parametrized double loop (BatchedDoubleLoop with bidder="parametrized") on the reference-shaped sweep.  Prints ONE JSON line.

    python tools/gpu_parametrized_sweep.py                      # run_double_loop_PEM.py's grid on bus 303: pem_bid 15 .. 45 step 5
                                                                # x pem_pmax = fractions of 847 MW (211.75 MW included) x --windows
    python tools/gpu_parametrized_sweep.py --plants 8192        # the grid tiled over as many windows as 8192 plants take
    python tools/gpu_parametrized_sweep.py --plants 8192 --bidder lp      # the yardstick: the LP-bidding loop of as many plants

Warm-up days first (handles, kernels, the hipGraphs of a day), then reset() and `--days` timed days from hour 0."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEM_BIDS = [15.0, 20.0, 25.0, 30.0, 35.0, 40.0, 45.0]
PEM_FRACTIONS = [0.05, 0.1, 0.25, 0.5, 1.0]                  # of the 847 MW wind farm; 0.25 -> 211.75 MW, the reference's default --pem_pmax


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flowsheet", default="wind_pem", choices=["wind_pem", "wind_battery"])
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--plants", type=int, default=0, help="> 0: that many plants (the grid repeated over windows, cut to size)")
    ap.add_argument("--bidder", default="parametrized", choices=["parametrized", "lp"])
    ap.add_argument("--market", default="price_taker")
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=1, help="timed repetitions (each after a reset): the line carries all of them")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd.hip_solver import load_library
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    wind = 847.0 if a.flowsheet == "wind_pem" else 200.0
    sizes = [wind * f for f in PEM_FRACTIONS]
    grid = len(PEM_BIDS) * len(sizes)
    windows = a.windows if a.plants <= 0 else -(-a.plants // grid)
    if a.bidder == "parametrized":
        from dispatches_amd.sweeps import grid_layout
        bid, sto, win = grid_layout(PEM_BIDS, sizes, windows)
        if a.plants > 0:                                         # window-major, so that a cut keeps whole grids
            order = np.argsort(win, kind="stable")[:a.plants]
            bid, sto, win = bid[order], sto[order], win[order]
        loop = BatchedDoubleLoop(a.flowsheet, len(bid), device=0, bidder="parametrized", bid_price=bid, storage_mw=sto, plant_windows=win, market=a.market)
    else:
        loop = BatchedDoubleLoop(a.flowsheet, a.plants if a.plants > 0 else grid * windows, device=0)
    for _ in range(a.warmup):
        loop.run_day()
    torch.cuda.synchronize()
    seconds = []
    for _ in range(a.repeat):
        loop.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.days):
            loop.run_day()
        torch.cuda.synchronize()
        seconds.append(time.perf_counter() - t0)
    res, ok = loop.results()
    best = min(seconds)
    line = dict(tool="gpu_parametrized_sweep", flowsheet=a.flowsheet, bidder=a.bidder, market=a.market if a.bidder == "parametrized" else "stub",
                B=loop.B, grid=[len(PEM_BIDS), len(sizes), windows], days=a.days, seconds=best, ms_per_simulated_day=1e3 * best / a.days,
                all_seconds=seconds, solves=loop.solves, all_optimal=bool(ok), uncertified=int(loop.uncertified.item()),
                revenue_sum=float(res["obj"].sum().item()), source_hash=load_library().dsp_source_hash().decode())
    if "offered_mwh" in res:
        line.update(offered_mwh=float(res["offered_mwh"].sum().item()), cleared_mwh=float(res["da_energy_mwh"].sum().item()))
    if "h2_kg" in res:
        line.update(h2_kg=float(res["h2_kg"].sum().item()))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
