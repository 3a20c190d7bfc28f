"""Time the day profiles and the representative days (BatchedDoubleLoop(profiles=days); representative_days.py): the loop with and without
profiles on the same build, the untouched paths against another build of the library (the parent commit's tree), and the clustering
kernels at the size of a year of 8192 plants next to the numpy statement on the host.  Prints one JSON line per timed run and appends it
to profiles/representative_days_timings.jsonl (--out).

    python tools/gpu_representative_days.py                    # with / without profiles: nuclear 256 x 3 and wind + battery 8192 x 1
    python tools/gpu_representative_days.py --parent PATH      # ... then the untouched paths, this tree against the tree at PATH (built)
    python tools/gpu_representative_days.py --clustering       # ... then assign / update / frequency at 8192 plants x 366 days, K = 20, 30

With / without: per loop warm-up days (handles, kernels, the hipGraphs of a day), reset(), `--days` timed days from hour 0; the two loops
alternate for `--rounds` rounds, the spread between rounds is the noise.  profiles=days adds one launch of a B-lane copy kernel per hour
step, inside the captured graphs; it removes nothing.
Untouched paths (lines tagged `build`: "parent" or "this"): the default stochastic nuclear loop and bench.py, each build in a fresh child
process that imports the package of ITS tree, the builds alternating for `--parent-rounds` rounds.
Clustering: a seeded random year (a fifth zero days, a fifth full days) in a profile buffer on the device, channels=2 for K = 20 and
channels=1 for K = 30 as in the reference's two cases; `--repeats` timed calls of each kernel after one warm-up call; achieved bytes/s of
dsp_days_assign against the profile buffer's size (what it must read at least once); the numpy statement on the host for the same points
(--host-days limits the host's share to the first days, 0 skips it; the line says how many points the host was given)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_CASES = (("nuclear", 256, 3), ("wind_battery", 8192, 1))
TOOL = "gpu_representative_days"


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
    for flowsheet, B, S in DEFAULT_CASES:
        kw = dict(device=0, n_price_scenarios=S, forecaster="backcast" if S > 1 else "perfect", market="price_taker" if S > 1 else "stub")
        loops = dict(profiles=BatchedDoubleLoop(flowsheet, B, profiles=a.days, **kw), no_profiles=BatchedDoubleLoop(flowsheet, B, **kw))
        for loop in loops.values():
            for _ in range(a.warmup):
                loop.run_day()
        torch.cuda.synchronize()
        for rnd in range(1, a.rounds + 1):
            for name, loop in loops.items():
                seconds = timed_days(loop, a.days)
                emit(a.out, dict(tool=TOOL, run=f"{name}_{rnd}", flowsheet=flowsheet, market=kw["market"], B=B, S=S,
                                 profile_bytes=getattr(loop, "profile_bytes", 0), **describe(loop, seconds, a.days)))
        del loops
        torch.cuda.empty_cache()


def untouched_worker(a):
    """in a child process of its own: the package of the tree at the working directory, profiles never asked for"""
    import torch
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    loop = BatchedDoubleLoop("nuclear", 256, device=0, n_price_scenarios=3, forecaster="backcast", market="price_taker")
    for _ in range(a.warmup):
        loop.run_day()
    torch.cuda.synchronize()
    seconds = timed_days(loop, a.days)
    emit(a.out, dict(build=a.tag, round=a.round, tool=TOOL, run=f"default_{a.round}", flowsheet="nuclear", market="price_taker", B=256, S=3,
                     **describe(loop, seconds, a.days)))


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
            emit(a.out, dict(build=tag, round=rnd, tool=TOOL, run=f"bench_{rnd}", metric=result.get("metric"), value=result.get("value"),
                             unit=result.get("unit")))


def clustering(a):
    import numpy as np
    import torch
    from dispatches_amd import representative_days as rd
    dev = torch.device("cuda", 0)
    B, D, N = a.cluster_plants, a.cluster_days, 8784
    gen = torch.Generator(device=dev).manual_seed(7)
    profile = torch.rand((D, 24, B), dtype=torch.float64, device=dev, generator=gen)
    kind = torch.randint(0, 5, (D, 1, B), device=dev, generator=gen)
    profile = torch.where(kind == 0, 0.0, torch.where(kind == 1, 1.0, profile)).contiguous()
    series = torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    start = (37 * torch.arange(B, dtype=torch.int64, device=dev)) % N

    def gpu_time(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.repeats):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.repeats, out

    for K, channels in ((20, 2), (30, 1)):
        points = rd.DayPoints(rd.Profiles(profile, series, start), channels=channels, p_min=0.0, p_max=1.0)
        centers = np.random.default_rng(K).random((K, 24 * channels))
        t_assign, (label, dist2) = gpu_time(lambda: points.assign(centers))
        t_update, (new, count, inertia) = gpu_time(lambda: points.update(label, dist2, centers))
        t_freq, freq = gpu_time(lambda: points.label_frequency(label, K))
        line = dict(tool=TOOL, run=f"clustering_K{K}", B=B, days=D, K=K, channels=channels, points=B * D, repeats=a.repeats,
                    profile_bytes=profile.numel() * 8, assign_ms=1e3 * t_assign, update_ms=1e3 * t_update, lloyd_iteration_ms=1e3 * (t_assign + t_update),
                    frequency_ms=1e3 * t_freq, assign_profile_bytes_per_s=profile.numel() * 8 / t_assign, labelled=int(count.sum()),
                    inertia=inertia, note="update_ms includes its host round trip (centres, counts and inertia are returned to the host)")
        host_days = D if a.host_days < 0 else min(a.host_days, D)
        if host_days:
            host = profile[:host_days].cpu().numpy()
            t0 = time.perf_counter()
            X = rd.points(host, np.zeros(B), np.ones(B), channels, series.cpu().numpy(), start.cpu().numpy())
            want_label, want_dist2 = rd.assign(X, centers)
            t1 = time.perf_counter()
            rd.update(X, want_label, want_dist2, centers)
            t2 = time.perf_counter()
            want_freq = rd.frequency(want_label.reshape(host_days, B), K)
            t3 = time.perf_counter()
            line.update(host_points=B * host_days, host_assign_ms=1e3 * (t1 - t0), host_update_ms=1e3 * (t2 - t1), host_frequency_ms=1e3 * (t3 - t2),
                        host_labels_equal=bool(np.array_equal(label[:host_days].cpu().numpy().reshape(-1), want_label)),
                        host_frequency_equal=bool(host_days == D and np.array_equal(freq.cpu().numpy(), want_freq)))
        emit(a.out, line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds profiles / no profiles")
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: time the untouched paths against it")
    ap.add_argument("--parent-rounds", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--clustering", action="store_true", help="the clustering kernels at --cluster-plants x --cluster-days")
    ap.add_argument("--cluster-plants", type=int, default=8192)
    ap.add_argument("--cluster-days", type=int, default=366)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-days", type=int, default=-1, help="days of the points the numpy statement is timed on (-1: all, 0: none)")
    ap.add_argument("--skip-loops", action="store_true", help="only what --parent / --clustering ask for")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "representative_days_timings.jsonl"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tag", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--round", type=int, default=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.out = os.path.abspath(a.out)                     # (the child processes run in their own tree's directory)
    if a.worker:                                       # (the package comes from PYTHONPATH / the working directory: the tree under test)
        return untouched_worker(a)
    sys.path.insert(0, ROOT)
    if not a.skip_loops:
        with_and_without(a)
    if a.parent:
        untouched(a)
    if a.clustering:
        clustering(a)


if __name__ == "__main__":
    main()
