"""Time the double loop that keeps a per-plant ledger (BatchedDoubleLoop(..., ledger=True)) against the same loop without it
(ledger=False) on the same build, at the same B and S.  Prints one JSON line per timed run and appends it to
profiles/ledger_timings.jsonl (--out).

    python tools/gpu_ledger.py                                    # nuclear 256 x 3 (backcast, price taker) and wind + battery 8192 x 1
    python tools/gpu_ledger.py --flowsheet wind_pem --plants 1024 --scenarios 3

Per loop: warm-up days (handles, kernels, the hipGraphs of a day), reset(), `--days` timed days from hour 0; the two loops alternate for
`--rounds` rounds, the spread between rounds is the noise.  The ledger adds one launch of an F * B-lane kernel per simulated hour, inside
the captured hour graphs; it removes nothing."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_CASES = (("nuclear", 256, 3), ("wind_battery", 8192, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flowsheet", default=None, help="one flowsheet instead of the two default cases")
    ap.add_argument("--plants", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=3)
    ap.add_argument("--days", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds ledger / no ledger")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ledger_timings.jsonl"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd.hip_solver import load_library
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    cases = DEFAULT_CASES if a.flowsheet is None else ((a.flowsheet, a.plants, a.scenarios),)
    for flowsheet, B, S in cases:
        kw = dict(device=0, n_price_scenarios=S, forecaster="backcast" if S > 1 else "perfect", market="price_taker" if S > 1 else "stub")
        loops = dict(ledger=BatchedDoubleLoop(flowsheet, B, ledger=True, **kw), no_ledger=BatchedDoubleLoop(flowsheet, B, **kw))
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
                line = dict(tool="gpu_ledger", run=f"{name}_{rnd}", flowsheet=flowsheet, market=kw["market"], B=B, S=S, ledger=loop.ledger,
                            graphs=len(loop._graphs), days=a.days, seconds=seconds, ms_per_simulated_day=1e3 * seconds / a.days,
                            solves=loop.solves, all_optimal=bool(ok), uncertified=int(loop.uncertified.item()),
                            revenue_sum=float(res["obj"].sum().item()),
                            tot_cost_sum=float(res["tot_cost"].sum().item()) if loop.ledger else None,
                            source_hash=load_library().dsp_source_hash().decode())
                print(json.dumps(line), flush=True)
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(line) + "\n")
        del loops
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
