"""Time the device-resident double loop in its stochastic mode (or, with --scenarios 1 --forecaster perfect --market stub, the
deterministic loop: the yardstick is the deterministic loop at plants x scenarios plants).  Prints ONE JSON line.

    python tools/gpu_stochastic_loop.py --plants 8192 --scenarios 3 --days 30

Warm-up days first (handles, kernels, the hipGraphs of a day), then reset() and `--days` timed days from hour 0, as the config-4 leg
of bench.py does."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plants", type=int, default=8192)
    ap.add_argument("--scenarios", type=int, default=3)
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=0)
    ap.add_argument("--forecaster", default="backcast")
    ap.add_argument("--market", default="price_taker")
    ap.add_argument("--history-days", type=int, default=10)
    ap.add_argument("--cold", action="store_true", help="no rolling warm start of the day-ahead LPs")
    ap.add_argument("--repeat", type=int, default=1, help="timed repetitions (each after a reset): the line carries all of them")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd.hip_solver import load_library
    from dispatches_amd.rolling import PipelinedDoubleLoops
    loop = PipelinedDoubleLoops(a.plants, device=0, groups=a.groups, n_price_scenarios=a.scenarios, forecaster=a.forecaster,
                                max_historical_days=a.history_days, market=a.market, warm_start=not a.cold)
    for _ in range(a.warmup):
        loop.run_day()
    torch.cuda.synchronize()
    seconds = []
    for _ in range(a.repeat):
        loop.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run_days(a.days)
        torch.cuda.synchronize()
        seconds.append(time.perf_counter() - t0)
    res, ok = loop.results()
    best = min(seconds)
    line = dict(tool="gpu_stochastic_loop", B=a.plants, S=a.scenarios, days=a.days, groups=loop.groups, forecaster=a.forecaster, market=a.market,
                warm_start=not a.cold, seconds=best, ms_per_simulated_day=1e3 * best / a.days, all_seconds=seconds,
                solves=sum(l.solves for l in loop.loops), all_optimal=bool(ok), uncertified=int(loop.uncertified.item()),
                revenue_sum=float(res["obj"].sum().item()), source_hash=load_library().dsp_source_hash().decode())
    if "offered_mwh" in res:
        line.update(offered_mwh=float(res["offered_mwh"].sum().item()), cleared_mwh=float(res["da_energy_mwh"].sum().item()))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
