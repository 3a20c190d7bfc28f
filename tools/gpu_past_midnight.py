"""Time past_midnight="coupled" of the descriptor double loop (dispatches_amd/rolling_flowsheets.py::BatchedDoubleLoop: the last T_rt - 1
hours of a day solve ONE coupled real-time LP per plant) against past_midnight="free" at the same B and S, and - with --parent - the
paths the feature does not touch against a checkout of the parent commit.

    python tools/gpu_past_midnight.py [--out profiles/past_midnight_timings.jsonl] [--days 20] [--rounds 3]
    python tools/gpu_past_midnight.py --parent /path/to/a/built/checkout/of/the/parent [--parent-rounds 2]

Cases (flowsheet:plants:S:mode): nuclear 256 x 3 monotone, wind + PEM 256 x 3 monotone, nuclear 256 x 3 self-schedule; "coupled" and
"free" alternate, `--rounds` rounds of `--days` days from hour graphs.  With --parent, lines tagged build = "parent" / "this" alternate
for `--parent-rounds` rounds over the untouched paths: the default stochastic nuclear loop, the default monotone nuclear loop (the
argument left out, so that the parent's constructor takes the call) and bench.py --gpus 1.  Every measurement is a child process of
its own under `timeout`; the driver stops at the first child that fails (no retries) and appends one JSON line per measurement to --out.
The numbers are recorded, not gated.

    python tools/gpu_past_midnight.py --one nuclear --plants 256 --scenarios 3 --mode monotone --past-midnight coupled      (one line)

Warm-up days first (handles, kernels, the hipGraphs of a day), then reset() and `--days` timed days from hour 0."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = {"monotone": dict(bidder="lp", scenario_coupling="monotone"), "independent": dict(bidder="lp", scenario_coupling="independent"),
         "self_schedule": dict(bidder="self_schedule")}


def one(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd.hip_solver import load_library
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    kw = dict(MODES[a.mode])
    if a.past_midnight != "default":               # (left out: the call the parent's constructor takes too)
        kw["past_midnight"] = a.past_midnight
    loop = BatchedDoubleLoop(a.one, a.plants, device=0, n_price_scenarios=a.scenarios, forecaster="backcast", max_historical_days=a.history_days,
                             market="price_taker", day_ahead_horizon=24, **kw)
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
    line = dict(tool="gpu_past_midnight", flowsheet=a.one, B=a.plants, S=a.scenarios, mode=a.mode, past_midnight=a.past_midnight, days=a.days,
                seconds=seconds, ms_per_simulated_day=1e3 * seconds / a.days, solves=loop.solves, all_optimal=bool(ok),
                uncertified=int(loop.uncertified.item()), revenue_sum=float(res["obj"].sum().item()), graphs=len(loop._graphs),
                source_hash=load_library().dsp_source_hash().decode())
    if a.past_midnight == "coupled":               # how the last coupled hourly solve ran
        stats, iters = loop.rtc.dlp.last_stats, loop.rtc.out["iters"].cpu().numpy()
        line.update(coupled_columns=loop.rtc.lp.n, coupled_rows=loop.rtc.lp.m, streaming=int(stats.streaming), simplex=int(stats.simplex),
                    coupled_iterations=dict(min=int(iters.min()), median=float(np.median(iters)), max=int(iters.max())))
    print(json.dumps(line), flush=True)
    return 0           # (a run with rows that are not optimal is a result here: all_optimal is in the line)


def child(cmd, seconds, cwd=None):
    p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, stdout=subprocess.PIPE, text=True, cwd=cwd)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    return p.returncode, (json.loads(lines[-1]) if lines else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "past_midnight_timings.jsonl"))
    ap.add_argument("--days", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--history-days", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=240, help="time limit of one measurement")
    ap.add_argument("--cases", default="nuclear:256:3:monotone,wind_pem:256:3:monotone,nuclear:256:3:self_schedule")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: time the untouched paths there and here")
    ap.add_argument("--parent-rounds", type=int, default=2)
    ap.add_argument("--untouched", default="nuclear:256:3:independent,nuclear:256:3:monotone")
    ap.add_argument("--bench", default="--gpus 1 --steps 20 --warmup 5", help="bench.py arguments of the untouched-path lines")
    ap.add_argument("--one", default=None, help="flowsheet of ONE measurement in this process (with --plants / --scenarios / --mode / --past-midnight)")
    ap.add_argument("--root", default=HERE, help="--one: the tree whose package is measured")
    ap.add_argument("--plants", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=3)
    ap.add_argument("--mode", default="monotone", choices=tuple(MODES))
    ap.add_argument("--past-midnight", default="coupled", choices=("coupled", "free", "default"))
    a = ap.parse_args()
    if a.one:
        return one(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def measure(run, cmd, cwd=None, **tags):
        rc, line = child(cmd, a.seconds, cwd)
        if rc != 0 or line is None:
            print(f"{run}: exit status {rc} - stopping here", flush=True)
            return rc or 1
        if "bench.py" in tags.get("path", ""):          # bench.py's line is long: its headline figures
            line = {k: line[k] for k in ("metric", "value", "unit", "steps", "ms_per_step", "optimal") if k in line}
        line = {"run": run, **tags, **line}
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        return 0

    def loop_cmd(case, past_midnight, root=HERE):
        flowsheet, plants, scenarios, mode = case.split(":")
        return [sys.executable, os.path.abspath(__file__), "--one", flowsheet, "--plants", plants, "--scenarios", scenarios, "--mode", mode,
                "--past-midnight", past_midnight, "--days", str(a.days), "--warmup", str(a.warmup), "--history-days", str(a.history_days),
                "--root", root]

    if a.parent is None:
        for case in a.cases.split(","):
            for r in range(a.rounds):
                for past_midnight in ("coupled", "free"):
                    rc = measure(f"{case.replace(':', '_')}_{past_midnight}_{r + 1}", loop_cmd(case, past_midnight))
                    if rc:
                        return rc
        return 0
    parent = os.path.abspath(a.parent)
    for r in range(a.parent_rounds):
        for build, root in (("parent", parent), ("this", HERE)):
            for case in a.untouched.split(","):
                rc = measure(f"{case.replace(':', '_')}_default_{build}_{r + 1}", loop_cmd(case, "default", root), build=build)
                if rc:
                    return rc
            rc = measure(f"bench_{build}_{r + 1}", [sys.executable, os.path.join(root, "bench.py")] + a.bench.split(), cwd=root, build=build,
                         tool="gpu_past_midnight", path="bench.py " + a.bench)
            if rc:
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
