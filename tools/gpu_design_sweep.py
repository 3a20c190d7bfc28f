"""Time a design sweep of the LP-bidding wind + battery double loop (BatchedDoubleLoop with wind_mw / battery_mw / battery_mwh per plant;
sweeps.design_layout) against the DEFAULT loop of as many plants and scenarios.  Prints one JSON line per timed run.

    python tools/gpu_design_sweep.py                 # 200 MW of wind, battery = 0.1 .. 1.0 of it x 2 / 4 / 6 / 8 h x --windows, S = 3
    python tools/gpu_design_sweep.py --rounds 2      # sized, default, sized, default: the spread between rounds is the noise

The grid is the shape of the reference's study (run_double_loop_battery.py --wind_pmax --battery_pmax --battery_energy_capacity, one
Prescient job per point of new_wind_battery_ratio_duration_sweep_sb/battery_duration_*).  Both loops see the SAME windows
(plant_windows), so the only difference is the sizes.  Per loop: warm-up days (handles, kernels, the hipGraphs of a day), reset(), `--days`
timed days from hour 0; then, untimed, `--iter-days` more days whose day-ahead iteration counts are read back after every day-ahead
solve: plants far from the template's scaling (it is built at the batch's largest sizes) may iterate longer, and the line says so per
size."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIND_MW = 200.0
BATTERY_RATIOS = [0.1, 0.25, 0.5, 0.75, 1.0]                 # battery power as a share of the wind farm
DURATIONS_H = [2.0, 4.0, 6.0, 8.0]


def quantiles(a):
    a = np.asarray(a)
    return dict(median=float(np.median(a)), p95=float(np.percentile(a, 95)), max=int(a.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--scenarios", type=int, default=3)
    ap.add_argument("--market", default="price_taker")
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2, help="alternating rounds sized / default")
    ap.add_argument("--iter-days", type=int, default=5, help="untimed days whose day-ahead iteration counts are collected")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd.hip_solver import load_library
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from dispatches_amd.sweeps import design_layout
    wind, batt, mwh, win = design_layout([WIND_MW], [WIND_MW * r for r in BATTERY_RATIOS], DURATIONS_H, a.windows)
    kw = dict(device=0, n_price_scenarios=a.scenarios, forecaster="backcast" if a.scenarios > 1 else "perfect", market=a.market, plant_windows=win)
    loops = dict(sized=BatchedDoubleLoop("wind_battery", len(wind), wind_mw=wind, battery_mw=batt, battery_mwh=mwh, **kw),
                 default=BatchedDoubleLoop("wind_battery", len(wind), **kw))
    for loop in loops.values():
        for _ in range(a.warmup):
            loop.run_day()
    torch.cuda.synchronize()
    S = a.scenarios
    for rnd in range(1, a.rounds + 1):
        for name, loop in loops.items():
            loop.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.days):
                loop.run_day()
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            res, ok = loop.results()
            line = dict(tool="gpu_design_sweep", run=f"{name}_{rnd}", flowsheet="wind_battery", market=a.market, B=loop.B, S=S,
                        grid=[1, len(BATTERY_RATIOS), len(DURATIONS_H), a.windows], days=a.days, seconds=seconds,
                        ms_per_simulated_day=1e3 * seconds / a.days, solves=loop.solves, all_optimal=bool(ok),
                        uncertified=int(loop.uncertified.item()), revenue_sum=float(res["obj"].sum().item()),
                        source_hash=load_library().dsp_source_hash().decode())
            if rnd == a.rounds and a.iter_days > 0:              # untimed: day-ahead iterations of every row, day by day
                iters = []
                for _ in range(a.iter_days):
                    loop.day_ahead()
                    iters.append(loop.da.out["iters"].cpu().numpy().reshape(loop.B, S).copy())
                    for _ in range(24):
                        loop.hour_step()
                iters = np.stack(iters)                          # [days, B, S]
                line["da_iterations"] = quantiles(iters)
                if name == "sized":
                    shape = (len(BATTERY_RATIOS), len(DURATIONS_H), a.windows)
                    per = iters.reshape((a.iter_days,) + shape + (S,))
                    line["da_iterations_per_size"] = {f"{WIND_MW * r:g}MW_{d:g}h": quantiles(per[:, i, j])
                                                      for i, r in enumerate(BATTERY_RATIOS) for j, d in enumerate(DURATIONS_H)}
                _, ok = loop.results()
                line["all_optimal_after_iteration_days"] = bool(ok)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
