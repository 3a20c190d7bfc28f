"""Time the double loop that bids day-ahead at the RUC hour on a projected state (BatchedDoubleLoop(..., ruc_hour=H)) against the DEFAULT
loop (ruc_hour=None) of the same build at the same B and S.  Prints one JSON line per timed run.

    python tools/gpu_ruc_hour.py                                  # nuclear 256 x 3 and wind + battery 8192 x 3, H = 16, 30 days, 2 rounds
    python tools/gpu_ruc_hour.py --flowsheet nuclear --plants 256 --scenarios 1 --market stub

Per loop: warm-up days (handles, kernels, the hipGraphs of a day - the hour of the bid and the activation among them), reset(), `--days`
timed days from hour 0; the two loops alternate for `--rounds` rounds, the spread between rounds is the noise.  The mode adds 24 - H
tracker solves and 2 (24 - H) + 1 small launches per day and moves the day-ahead solve from hour 0 to hour H; it removes nothing."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_CASES = (("nuclear", 256), ("wind_battery", 8192))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flowsheet", default=None, help="one flowsheet instead of the two default cases")
    ap.add_argument("--plants", type=int, default=None)
    ap.add_argument("--scenarios", type=int, default=3)
    ap.add_argument("--market", default="price_taker")
    ap.add_argument("--ruc-hour", type=int, default=16)
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2, help="alternating rounds ruc_hour / default")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd.hip_solver import load_library
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    cases = DEFAULT_CASES if a.flowsheet is None else ((a.flowsheet, a.plants or 256),)
    S = a.scenarios
    for flowsheet, B in cases:
        kw = dict(device=0, n_price_scenarios=S, forecaster="backcast" if S > 1 else "perfect", market=a.market)
        loops = dict(ruc_hour=BatchedDoubleLoop(flowsheet, B, ruc_hour=a.ruc_hour, **kw), default=BatchedDoubleLoop(flowsheet, B, **kw))
        for loop in loops.values():
            for _ in range(a.warmup):
                loop.run_day()
        torch.cuda.synchronize()
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
                print(json.dumps(dict(tool="gpu_ruc_hour", run=f"{name}_{rnd}", flowsheet=flowsheet, market=a.market, B=B, S=S,
                                      ruc_hour=loop.ruc_hour, days=a.days, seconds=seconds, ms_per_simulated_day=1e3 * seconds / a.days,
                                      solves=loop.solves, all_optimal=bool(ok), uncertified=int(loop.uncertified.item()),
                                      revenue_sum=float(res["obj"].sum().item()), source_hash=load_library().dsp_source_hash().decode())),
                      flush=True)
        del loops
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
