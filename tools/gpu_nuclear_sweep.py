"""Time the reference-shaped nuclear hydrogen grid - 6 hydrogen prices 0.75 .. 2 $/kg by 10 PEM sizes 5 .. 50 % of the 500 MW plant, at
`--windows` price windows - as ONE batch of the device double loop (BatchedDoubleLoop("nuclear", ..., h2_price=, pem_mw=, ledger=True);
sweeps.nuclear_layout) against the UNSIZED loop at the same B, and ledger=True against False on the unsized loop.  Prints one JSON line
per timed run and appends it to profiles/ledger_timings.jsonl (--out).

    python tools/gpu_nuclear_sweep.py                 # 60 grid points x 4 windows = 240 plants, S = 3, 20 days, 3 rounds

Per loop: warm-up days (handles, kernels, the hipGraphs of a day), reset(), `--days` timed days from hour 0; the loops alternate for
`--rounds` rounds, the spread between rounds is the noise."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H2_PRICES = np.linspace(0.75, 2.0, 6)
PEM_MWS = 500.0 * np.arange(1, 11) * 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--scenarios", type=int, default=3)
    ap.add_argument("--days", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ledger_timings.jsonl"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd.hip_solver import load_library
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from dispatches_amd.sweeps import nuclear_layout
    price, pem, win = nuclear_layout(H2_PRICES, PEM_MWS, a.windows)
    B, S = len(price), a.scenarios
    kw = dict(device=0, n_price_scenarios=S, forecaster="backcast" if S > 1 else "perfect", market="price_taker", plant_windows=win)
    loops = dict(grid=BatchedDoubleLoop("nuclear", B, h2_price=price, pem_mw=pem, ledger=True, **kw),
                 unsized_ledger=BatchedDoubleLoop("nuclear", B, ledger=True, **kw), unsized=BatchedDoubleLoop("nuclear", B, **kw))
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
            line = dict(tool="gpu_nuclear_sweep", run=f"{name}_{rnd}", flowsheet="nuclear", market="price_taker", B=B, S=S, windows=a.windows,
                        ledger=loop.ledger, sized=loop.nuclear_sized, graphs=len(loop._graphs), days=a.days, seconds=seconds,
                        ms_per_simulated_day=1e3 * seconds / a.days, solves=loop.solves, all_optimal=bool(ok),
                        uncertified=int(loop.uncertified.item()), revenue_sum=float(res["obj"].sum().item()),
                        profit_sum=float(res["profit"].sum().item()) if loop.ledger else None,
                        source_hash=load_library().dsp_source_hash().decode())
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
