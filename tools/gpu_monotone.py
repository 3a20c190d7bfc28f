"""Time the monotone-bid-curve mode of the descriptor double loop (dispatches_amd/rolling_flowsheets.py::BatchedDoubleLoop with
bidder="lp", scenario_coupling="monotone") against its two neighbours at the same B and S: the independent LP bidder
(scenario_coupling="independent": S day-ahead LPs per plant, the curve repaired by a running maximum) and the self-schedule
(bidder="self_schedule": one coupled LP per plant with (S - 1) T equality rows instead of S (S - 1) / 2 * T ordered-pair rows).

    python tools/gpu_monotone.py [--out profiles/monotone_timings.jsonl] [--days 10] [--rounds 1]

Cases (flowsheet:plants:S): nuclear, wind + PEM at S = 3 and wind + battery at S = 2 - coupled LPs inside the fused kernels - and wind +
battery at S = 3, whose coupled LP (582 x 432) the solver streams.  Every measurement is a child process of its own under `timeout`, the
three modes alternating, `--rounds` rounds; the driver stops at the first child that fails (no retries) and appends one JSON line per
measurement to --out.  A line of a coupled mode also records how the coupled day-ahead solve ran: dsp_stats::streaming / stream_form of
the last day's solve, the distribution of its iteration counts, and the share of optimal / uncertified rows - whether the streamed wind +
battery LP certifies inside the loop is written down here.  The numbers are recorded, not gated.

    python tools/gpu_monotone.py --one nuclear --plants 256 --scenarios 3 --mode monotone      (one measurement: prints its JSON line)

Warm-up days first (handles, kernels, the hipGraphs of a day), then reset() and `--days` timed days from hour 0."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"monotone": dict(bidder="lp", scenario_coupling="monotone"), "independent": dict(bidder="lp", scenario_coupling="independent"),
         "self_schedule": dict(bidder="self_schedule")}


def one(a):
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd.hip_solver import load_library
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    loop = BatchedDoubleLoop(a.one, a.plants, device=0, n_price_scenarios=a.scenarios, forecaster="backcast", max_historical_days=a.history_days,
                             market="price_taker", day_ahead_horizon=a.day_ahead_horizon, **MODES[a.mode])
    for _ in range(a.warmup):
        loop.run_day()
    torch.cuda.synchronize()
    loop.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.days):
        loop.run_day()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    res, ok = loop.results()
    line = dict(tool="gpu_monotone", flowsheet=a.one, B=a.plants, S=a.scenarios, mode=a.mode, day_ahead_horizon=a.day_ahead_horizon,
                days=a.days, seconds=seconds, ms_per_simulated_day=1e3 * seconds / a.days, solves=loop.solves, all_optimal=bool(ok),
                uncertified=int(loop.uncertified.item()), revenue_sum=float(res["obj"].sum().item()),
                offered_mwh=float(res["offered_mwh"].sum().item()), cleared_mwh=float(res["da_energy_mwh"].sum().item()),
                day_ahead_columns=loop.da.lp.n, day_ahead_rows=loop.da.lp.m, graphs=len(loop._graphs),
                source_hash=load_library().dsp_source_hash().decode())
    # the last day's day-ahead solve (its outputs are still in place: the hourly models have their own)
    stats = loop.da.dlp.last_stats
    iters = loop.da.out["iters"].cpu().numpy()
    status, flags = loop.da.out["status"].cpu().numpy(), loop.da.out["flags"].cpu().numpy()
    line.update(streaming=int(stats.streaming), stream_form=int(stats.stream_form),
                day_ahead_iterations=dict(min=int(iters.min()), median=float(np.median(iters)), p90=float(np.percentile(iters, 90)), max=int(iters.max())),
                day_ahead_optimal_share=float((status == 0).mean()), day_ahead_uncertified_share=float(((flags & 1) != 0).mean()))
    print(json.dumps(line), flush=True)
    return 0           # (a run with rows that are not optimal is a result here: all_optimal and the shares are in the line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monotone_timings.jsonl"))
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--history-days", type=int, default=10)
    ap.add_argument("--day-ahead-horizon", type=int, default=24)
    ap.add_argument("--seconds", type=int, default=240, help="time limit of one measurement")
    ap.add_argument("--cases", default="nuclear:256:3,wind_pem:256:3,wind_battery:256:2,wind_battery:64:3")
    ap.add_argument("--modes", default="monotone,independent,self_schedule")
    ap.add_argument("--one", default=None, help="flowsheet of ONE measurement in this process (with --plants / --scenarios / --mode)")
    ap.add_argument("--plants", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=3)
    ap.add_argument("--mode", default="monotone", choices=tuple(MODES))
    a = ap.parse_args()
    if a.one:
        return one(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases.split(","):
        flowsheet, plants, scenarios = case.split(":")
        for r in range(a.rounds):
            for mode in a.modes.split(","):
                cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--one", flowsheet, "--plants", plants,
                       "--mode", mode, "--scenarios", scenarios, "--days", str(a.days), "--warmup", str(a.warmup),
                       "--history-days", str(a.history_days), "--day-ahead-horizon", str(a.day_ahead_horizon)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
                if p.returncode != 0 or not lines:
                    print(f"{case} {mode} round {r + 1}: exit status {p.returncode} - stopping here", flush=True)
                    return p.returncode or 1
                line = dict(run=f"{flowsheet}{plants}x{scenarios}_{mode}_{r + 1}", **json.loads(lines[-1]))
                print(json.dumps(line), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
