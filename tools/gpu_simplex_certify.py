"""Time the in-wave simplex' KKT certificate (dsp_options::simplex_certify; BatchedDoubleLoop(..., simplex_certify=True)) against the same
build without it.  Prints one JSON line per timed run and appends it to profiles/simplex_certify_timings.jsonl (--out).

    python tools/gpu_simplex_certify.py --part hourly        # the six hourly LP families at 4096 scenarios, cold and warm: kernel us
    python tools/gpu_simplex_certify.py --part loops         # ms per simulated day, nuclear 256 x 3 and wind + battery 8192 x 1
    python tools/gpu_simplex_certify.py --part default --tree DIR --tag NAME
                                                             # the DEFAULT stochastic nuclear loop (no option of this tool's) of the checkout
                                                             # in DIR: run on this tree and on a checkout of the parent commit, alternating,
                                                             # to show that the untouched path did not move
    python tools/gpu_simplex_certify.py --part bench --tree DIR --tag NAME
                                                             # `bench.py --gpus 1 --steps 20 --warmup 5` of the checkout in DIR, in a child
                                                             # process; its result line is recorded with tool = "bench.py", run = NAME

The lines always go to --out (default: profiles/ of THIS checkout), also when --tree names another checkout: one file holds both sides.
The parent / new comparison that is in the file was taken as
    for r in 1 2; do for part in default bench; do
        python tools/gpu_simplex_certify.py --part $part --tree <checkout of the parent commit> --tag parent_$r
        python tools/gpu_simplex_certify.py --part $part --tag new_$r;  done; done

hourly: fixture inputs (tests/golden/oracle_hourly.npz), one solver per (family, warm, certify); three untimed solves, then the smallest
hipEvent time of `--repeats` solves.  "cold" is simplex_warm = 0 (batches up to 2048 would run in the register kernel; 4096 runs in the
LDS-tableau kernel either way), "warm" is simplex_warm = 1 solved again from its own final basis: no pivots at all, only the loads, the
checks and the stores - the case in which the certificate is the largest share of the kernel.
loops: as tools/gpu_ledger.py - warm-up days, reset(), `--days` timed days, the two loops alternate for `--rounds` rounds."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOURLY = ("wind_battery_rt4", "wind_pem_rt4", "nuclear_rt12", "wind_battery_track4", "wind_pem_track4", "nuclear_track4")
LOOPS = (("nuclear", 256, 3), ("wind_battery", 8192, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["hourly", "loops", "default", "bench"], required=True)
    ap.add_argument("--tree", default=HERE, help="--part default / bench: the checkout to import and time")
    ap.add_argument("--tag", default="new")
    ap.add_argument("--scenarios", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--days", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "simplex_certify_timings.jsonl"))
    a = ap.parse_args()
    root = os.path.abspath(a.tree)
    if a.part == "bench":
        import subprocess
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
        done = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, text=True, check=True)
        result = json.loads(done.stdout.strip().splitlines()[-1])
        result.pop("rank_devices", None)                 # (names the card it ran on: of no use in the record)
        line = dict(tool="bench.py", part="bench", run=a.tag, cmd=" ".join(cmd[1:]), **result)
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")
        return
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from dispatches_amd import scenarios
    from dispatches_amd.hip_solver import HipPdlpSolver, load_library
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    source = load_library().dsp_source_hash().decode()

    def emit(**line):
        line = dict(tool="gpu_simplex_certify", part=a.part, **line, source_hash=source)
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")

    def timed_days(loop):
        loop.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.days):
            loop.run_day()
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        res, ok = loop.results()
        return dict(graphs=len(loop._graphs), days=a.days, seconds=seconds, ms_per_simulated_day=1e3 * seconds / a.days, solves=loop.solves,
                    all_optimal=bool(ok), uncertified=int(loop.uncertified.item()), revenue_sum=float(res["obj"].sum().item()))

    if a.part == "hourly":
        fx = np.load(os.path.join(root, "tests", "golden", "oracle_hourly.npz"))
        for case in HOURLY:
            inp = {k.split("/", 1)[1]: fx[k][:a.scenarios] for k in fx.files if k.startswith(case + "/")}
            for warm in (0, 1):
                for certify in (0, 1):
                    solver = HipPdlpSolver(device=0, simplex_warm=warm, simplex_certify=certify)
                    make = scenarios.hourly_bid_batch if "rt" in case.split("_")[-1] else scenarios.hourly_tracking_batch
                    _, model = make(case, inp, solver)
                    for _ in range(3):
                        solver.solve(model)
                    ms = []
                    for _ in range(a.repeats):
                        solver.solve(model)
                        ms.append(float(solver.last_stats.kernel_ms))
                    st = solver.last_stats
                    kkt = getattr(model, "kkt", None) if certify else None
                    emit(case=case, n=model.lp.n, m=model.lp.m, B=model.n_scenario, start="warm" if warm else "cold", simplex_certify=certify,
                         kernel_us=1e3 * min(ms), kernel_us_median=1e3 * sorted(ms)[len(ms) // 2], pivots_mean=float(model.iterations.mean()),
                         optimal=int((model.status == 0).sum()), simplex=int(st.simplex), simplex_unsolved=int(getattr(st, "simplex_unsolved", -1)),
                         flagged_kkt=int(((model.flags & 8) != 0).sum()),
                         kkt_worst=None if kkt is None else [float(v) for v in np.nanmax(kkt, 0)])
    elif a.part == "loops":
        for flowsheet, B, S in LOOPS:
            kw = dict(device=0, n_price_scenarios=S, forecaster="backcast" if S > 1 else "perfect", market="price_taker" if S > 1 else "stub")
            loops = dict(certify=BatchedDoubleLoop(flowsheet, B, simplex_certify=True, **kw), plain=BatchedDoubleLoop(flowsheet, B, **kw))
            for loop in loops.values():
                for _ in range(a.warmup):
                    loop.run_day()
            torch.cuda.synchronize()
            for rnd in range(1, a.rounds + 1):
                for name, loop in loops.items():
                    emit(run=f"{name}_{rnd}", flowsheet=flowsheet, market=kw["market"], B=B, S=S, simplex_certify=loop.simplex_certify, **timed_days(loop))
            del loops
            torch.cuda.empty_cache()
    else:
        flowsheet, B, S = LOOPS[0]
        loop = BatchedDoubleLoop(flowsheet, B, device=0, n_price_scenarios=S, forecaster="backcast", market="price_taker")
        for _ in range(a.warmup):
            loop.run_day()
        torch.cuda.synchronize()
        emit(run=a.tag, flowsheet=flowsheet, market="price_taker", B=B, S=S, **timed_days(loop))


if __name__ == "__main__":
    main()
