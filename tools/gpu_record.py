"""Time the double loop that records (BatchedDoubleLoop(..., record=(plants, days))) against the same loop without it (record=None) on
the same build, at the same B and S.  Prints one JSON line per timed run and appends it to profiles/record_timings.jsonl (--out).

    python tools/gpu_record.py                                    # nuclear 256 x 3 (backcast, price taker) and wind + battery 8192 x 1
    python tools/gpu_record.py --flowsheet wind_pem --plants 1024 --scenarios 3
    python tools/gpu_record.py --untouched --build new            # the paths this feature leaves alone, to compare two builds

Per loop: warm-up days (handles, kernels, the hipGraphs of a day), reset(), `--days` timed days from hour 0; the two loops alternate for
`--rounds` rounds, the spread between rounds is the noise.  Recording adds three launches of the gather kernel per simulated hour (the
hour's record before the hand-off, `delivered` after it; the daily one once per day), inside the captured graphs; it removes nothing.
--untouched: the default stochastic nuclear loop and the ruc_hour=16 loop, both without record, tagged `--build` - run it from the tree
of each build (it passes no keyword an older build lacks), alternating, into the same file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT_CASES = (("nuclear", 256, 3), ("wind_battery", 8192, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flowsheet", default=None, help="one flowsheet instead of the two default cases")
    ap.add_argument("--plants", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=3)
    ap.add_argument("--recorded", type=int, default=16, help="recorded plants, spread over the batch")
    ap.add_argument("--days", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds record / no record")
    ap.add_argument("--first-round", type=int, default=1, help="number of the first round (builds alternate from a script: one round per call)")
    ap.add_argument("--untouched", action="store_true", help="time the default loops only (no record keyword at all)")
    ap.add_argument("--build", default="new", help="tag of the build under --untouched")
    ap.add_argument("--root", default=ROOT, help="the tree whose package and library are timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "record_timings.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd.hip_solver import load_library
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop

    def timed(tag, loops, extra):
        for loop in loops.values():
            for _ in range(a.warmup):
                loop.run_day()
        torch.cuda.synchronize()
        for rnd in range(a.first_round, a.first_round + a.rounds):
            for name, loop in loops.items():
                loop.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.days):
                    loop.run_day()
                torch.cuda.synchronize()
                seconds = time.perf_counter() - t0
                res, ok = loop.results()
                line = dict(tool="gpu_record", run=f"{name}_{rnd}", **tag, graphs=len(loop._graphs), days=a.days, seconds=seconds,
                            ms_per_simulated_day=1e3 * seconds / a.days, solves=loop.solves, all_optimal=bool(ok),
                            uncertified=int(loop.uncertified.item()), revenue_sum=float(res["obj"].sum().item()), **extra(loop),
                            source_hash=load_library().dsp_source_hash().decode())
                print(json.dumps(line), flush=True)
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(line) + "\n")

    stochastic = dict(n_price_scenarios=3, forecaster="backcast", market="price_taker")
    if a.untouched:
        loops = dict(default=BatchedDoubleLoop("nuclear", a.plants, device=0, **stochastic),
                     ruc_hour_16=BatchedDoubleLoop("nuclear", a.plants, device=0, ruc_hour=16, **stochastic))
        timed(dict(build=a.build, flowsheet="nuclear", B=a.plants, S=3), loops, lambda loop: {})
        return
    cases = DEFAULT_CASES if a.flowsheet is None else ((a.flowsheet, a.plants, a.scenarios),)
    for flowsheet, B, S in cases:
        kw = dict(device=0, n_price_scenarios=S, forecaster="backcast" if S > 1 else "perfect", market="price_taker" if S > 1 else "stub")
        plants = sorted({(q * B) // a.recorded for q in range(a.recorded)})
        loops = dict(record=BatchedDoubleLoop(flowsheet, B, record=(plants, a.days), **kw), no_record=BatchedDoubleLoop(flowsheet, B, **kw))
        timed(dict(flowsheet=flowsheet, market=kw["market"], B=B, S=S), loops,
              lambda loop: dict(record=loop._rec is not None, recorded_plants=len(plants) if loop._rec is not None else 0,
                                record_bytes=loop.record_bytes))
        del loops
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
