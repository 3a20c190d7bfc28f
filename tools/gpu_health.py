"""Time the double loop that keeps the per-plant solve health (BatchedDoubleLoop(..., health=True)) against the same loop without it on
the same build, time the untouched paths against another build of the library (the parent commit's tree), and report whether slow plants
are persistent.  Prints one JSON line per timed run and appends it to profiles/health_timings.jsonl (--out).

    python tools/gpu_health.py                       # with / without health: nuclear 256 x 3 and wind + battery 8192 x 1, hour graphs
    python tools/gpu_health.py --parent PATH         # ... then the untouched paths, this tree against the tree at PATH (built), two rounds
    python tools/gpu_health.py --persistence         # ... then the 60-day report of 8192 wind + battery plants

With / without: per loop warm-up days (handles, kernels, the hipGraphs of a day), reset(), `--days` timed days from hour 0; the two loops
alternate for `--rounds` rounds, the spread between rounds is the noise.  health=True adds one launch of a B-lane kernel per solve, inside
the captured graphs (two or three an hour, one per day-ahead solve, 24 - H per projection chain); it removes nothing.
Untouched paths (lines tagged `build`: "parent" or "this"): the default stochastic nuclear loop, its ruc_hour=16 loop and bench.py, each
build in a fresh child process that imports the package of ITS tree, the builds alternating for `--parent-rounds` rounds.
Persistence: one 60-day run with health=True; the distribution of health_iters_max[day_ahead] over the plants, and Spearman's rank
correlation of the per-plant day-ahead iteration sums of the first 30 days with those of the second 30."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_CASES = (("nuclear", 256, 3), ("wind_battery", 8192, 1))


def emit(path, line):
    print(json.dumps(line), flush=True)
    with open(path, "a") as fh:
        fh.write(json.dumps(line) + "\n")


def timed_days(loop, days):
    import torch
    loop.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(days):
        loop.run_day()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def describe(loop, seconds, days):
    from dispatches_amd.hip_solver import load_library
    res, ok = loop.results()
    return dict(graphs=len(loop._graphs), days=days, seconds=seconds, ms_per_simulated_day=1e3 * seconds / days, solves=loop.solves,
                all_optimal=bool(ok), uncertified=int(loop.uncertified.item()), revenue_sum=float(res["obj"].sum().item()),
                source_hash=load_library().dsp_source_hash().decode())


def with_and_without(a):
    import torch
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    cases = DEFAULT_CASES if a.flowsheet is None else ((a.flowsheet, a.plants, a.scenarios),)
    for flowsheet, B, S in cases:
        kw = dict(device=0, n_price_scenarios=S, forecaster="backcast" if S > 1 else "perfect", market="price_taker" if S > 1 else "stub")
        loops = dict(health=BatchedDoubleLoop(flowsheet, B, health=True, **kw), no_health=BatchedDoubleLoop(flowsheet, B, **kw))
        for loop in loops.values():
            for _ in range(a.warmup):
                loop.run_day()
        torch.cuda.synchronize()
        for rnd in range(1, a.rounds + 1):
            for name, loop in loops.items():
                seconds = timed_days(loop, a.days)
                line = dict(tool="gpu_health", run=f"{name}_{rnd}", flowsheet=flowsheet, market=kw["market"], B=B, S=S, health=loop.health,
                            **describe(loop, seconds, a.days))
                if loop.health:
                    line.update(failed_plants=int((~loop.valid).sum().item()), health_launch_rows=int(loop.health_solves.sum().item()))
                emit(a.out, line)
        del loops
        torch.cuda.empty_cache()


def untouched_worker(a):
    """in a child process of its own: the package of the tree at a.root (sys.path), health never asked for"""
    import torch
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    kw = dict(device=0, n_price_scenarios=3, forecaster="backcast", market="price_taker")
    for run, extra in (("default", {}), ("ruc_hour", dict(ruc_hour=16))):
        loop = BatchedDoubleLoop("nuclear", 256, **kw, **extra)
        for _ in range(a.warmup):
            loop.run_day()
        torch.cuda.synchronize()
        seconds = timed_days(loop, a.days)
        emit(a.out, dict(build=a.tag, round=a.round, tool="gpu_health", run=f"{run}_{a.round}", flowsheet="nuclear", market="price_taker", B=256, S=3,
                         ruc_hour=loop.ruc_hour, **describe(loop, seconds, a.days)))
        del loop
        torch.cuda.empty_cache()


def untouched(a):
    """this tree and the parent's, alternating, each run in a fresh child process; then each tree's own bench.py"""
    for rnd in range(1, a.parent_rounds + 1):
        for tag, root in (("parent", os.path.abspath(a.parent)), ("this", ROOT)):
            env = dict(os.environ, PYTHONPATH=root)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tag", tag, "--round", str(rnd), "--days", str(a.days),
                            "--warmup", str(a.warmup), "--out", a.out], cwd=root, env=env, check=True, timeout=600)
            done = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "3"],
                                  cwd=root, env=env, check=True, timeout=600, capture_output=True, text=True)
            result = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("{")][-1])
            emit(a.out, dict(build=tag, round=rnd, tool="gpu_health", run=f"bench_{rnd}", metric=result.get("metric"), value=result.get("value"),
                             unit=result.get("unit")))


def persistence(a):
    """are the slow plants of the day-ahead launch the same plants every day?"""
    import numpy as np
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    B, half = 8192, a.persistence_days // 2
    loop = BatchedDoubleLoop("wind_battery", B, device=0, health=True)
    sums = []
    for _ in range(2):
        before = loop.health_iters[0].clone()
        for _ in range(half):
            loop.run_day()
        sums.append((loop.health_iters[0] - before).cpu().numpy().astype(np.float64))
    rank = lambda v: np.argsort(np.argsort(v, kind="stable"), kind="stable").astype(np.float64)
    rho = float(np.corrcoef(rank(sums[0]), rank(sums[1]))[0, 1])
    most = loop.health_iters_max[0].cpu().numpy()
    res, ok = loop.results()
    top = np.argsort(-sums[0])[:B // 100]
    emit(a.out, dict(tool="gpu_health", run="persistence", flowsheet="wind_battery", B=B, S=1, days=2 * half,
                     iters_max_percentiles={str(q): int(np.percentile(most, q)) for q in (0, 50, 90, 99, 100)},
                     mean_iters_per_solve=float((sums[0] + sums[1]).sum() / (B * 2 * half)),
                     spearman_first_half_second_half=rho,
                     top_1_percent_of_first_half_in_top_1_percent_of_second=float(np.isin(top, np.argsort(-sums[1])[:B // 100]).mean()),
                     failed_plants=int((~res["valid"]).sum().item()), all_optimal=bool(ok)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flowsheet", default=None, help="one flowsheet instead of the two default cases")
    ap.add_argument("--plants", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=3)
    ap.add_argument("--days", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds health / no health")
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: time the untouched paths against it")
    ap.add_argument("--parent-rounds", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--persistence", action="store_true", help="the 60-day report of 8192 wind + battery plants")
    ap.add_argument("--persistence-days", type=int, default=60)
    ap.add_argument("--skip-health", action="store_true", help="only what --parent / --persistence ask for")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "health_timings.jsonl"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tag", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--round", type=int, default=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.out = os.path.abspath(a.out)                     # (the child processes run in their own tree's directory)
    if a.worker:                                       # (the package comes from PYTHONPATH / the working directory: the tree under test)
        return untouched_worker(a)
    sys.path.insert(0, ROOT)
    if not a.skip_health:
        with_and_without(a)
    if a.parent:
        untouched(a)
    if a.persistence:
        persistence(a)


if __name__ == "__main__":
    main()
