"""Time the descriptor double loop (dispatches_amd/rolling_flowsheets.py::BatchedDoubleLoop) in its stochastic mode against its yardstick:
the deterministic loop of the same flowsheet at S x the plants - as many bidding LPs, S times the tracking LPs.

    python tools/gpu_flowsheet_stochastic.py [--out profiles/flowsheet_stochastic_timings.jsonl] [--days 30] [--rounds 2]

Cases: nuclear, 256 plants x S = 3 (yardstick: 768 plants); wind + PEM, 8192 plants x S = 3 (yardstick: 24 576 plants).  Every
measurement is a child process of its own under `timeout`, stochastic and yardstick alternating, `--rounds` rounds; the driver stops at
the first child that fails (no retries) and appends one JSON line per measurement to --out.

    python tools/gpu_flowsheet_stochastic.py --one nuclear --plants 256 --scenarios 3       (one measurement: prints its JSON line)

Warm-up days first (handles, kernels, the hipGraphs of a day), then reset() and `--days` timed days from hour 0."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("nuclear", 256, 3, 300), ("wind_pem", 8192, 3, 420))     # flowsheet, plants, scenarios, seconds allowed per measurement


def one(a):
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd.hip_solver import load_library
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    kw = dict(n_price_scenarios=a.scenarios, forecaster="backcast", max_historical_days=a.history_days, market="price_taker") if a.scenarios > 1 else {}
    loop = BatchedDoubleLoop(a.one, a.plants, device=0, **kw)
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
    line = dict(tool="gpu_flowsheet_stochastic", flowsheet=a.one, B=a.plants, S=a.scenarios, stochastic=loop.stochastic, days=a.days,
                seconds=seconds, ms_per_simulated_day=1e3 * seconds / a.days, solves=loop.solves, all_optimal=bool(ok),
                uncertified=int(loop.uncertified.item()), revenue_sum=float(res["obj"].sum().item()),
                source_hash=load_library().dsp_source_hash().decode())
    if "offered_mwh" in res:
        line.update(offered_mwh=float(res["offered_mwh"].sum().item()), cleared_mwh=float(res["da_energy_mwh"].sum().item()))
    print(json.dumps(line), flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowsheet_stochastic_timings.jsonl"))
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--history-days", type=int, default=10)
    ap.add_argument("--cases", default="nuclear,wind_pem")
    ap.add_argument("--one", default=None, help="flowsheet of ONE measurement in this process (with --plants / --scenarios)")
    ap.add_argument("--plants", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=3)
    a = ap.parse_args()
    if a.one:
        return one(a)
    for flowsheet, plants, S, limit in CASES:
        if flowsheet not in a.cases.split(","):
            continue
        for r in range(a.rounds):
            for tag, B, s in (("stochastic", plants, S), ("yardstick", plants * S, 1)):
                cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", flowsheet, "--plants", str(B),
                       "--scenarios", str(s), "--days", str(a.days), "--warmup", str(a.warmup), "--history-days", str(a.history_days)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
                if p.returncode != 0 or not lines:
                    print(f"{flowsheet} {tag} round {r + 1}: exit status {p.returncode} - stopping here", flush=True)
                    return p.returncode or 1
                line = dict(run=f"{flowsheet}_{tag}_{r + 1}", **json.loads(lines[-1]))
                print(json.dumps(line), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
