"""GPU tool: record what the fused PDLP kernel computes on both sides of every edge of the ANCHOR-WEIGHT TABLE - the metric kernel
reads the Halpern weight 1 / (k + 2) of its plain iterations from a device table of K = 4096 entries where a whole segment fits
below K, and computes it as before where one does not - as the yardstick of that change, which must leave the results
BIT-IDENTICAL (tests/test_hip_anchor_weight.py).

    python tools/make_anchor_weight_fixture.py      # on the build whose results are the reference: writes the fixture

Per case the fixture holds status / iters / jumps / flags (int32), obj (float64) and one uint64 wrap-around sum of the bit patterns
of every scenario's x row and y row, for 4 scenarios (one [cases, 4] array per quantity, rows in the order of `cases`):

* the default cadence 16 under iteration limits 1 (no check), 17 (one segment, one check, one iteration) and 400;
* the default options to the end: every scenario restarts and the recorded `jumps` show ray jumps, so k returns to 0 in mid-solve and
  the table is entered again;
* cadence 4000 under a limit of 8200 with every restart, jump and termination switched off (NO_EVENT): k runs from 0 to 8200, the first
  segment reads k = 0 .. 3998 from the table, the second crosses K, the third starts beyond it;
* cadences 4097 and 4098 the same way: a first segment that ends exactly on K, and one iteration past it;
* cadence 3 on another register-resident shape and on the generic LDS-matrix kernel, which share the source and keep their loop."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "anchor_weight_parent.npz")

B = 4
TABLE = 4096                                  # kAnchorWeights, dispatches_amd/csrc/dsp_device.hpp
KEYS = ("status", "iters", "jumps", "flags", "obj", "xsum", "ysum")
# no restart (the decay factors are 0, the artificial one is out of reach), no ray jump, no termination (the residuals are never <= 1e-30):
# k counts every iteration of the solve
NO_EVENT = dict(restart_sufficient=0.0, restart_necessary=0.0, restart_artificial=1e9, ray_jumps=0, eps_rel=1e-30, stall_rescue=0,
                polish_patience=0, eps_infeasible=0.0)
METRIC = dict(matreg=1, rtc=0, cols_per_lane=4, rows_per_lane=2)

# name: (workload, solver options, expected dsp_stats fields, what the recorded results must show)
CASES = {}
for mi in (1, 17, 400):
    CASES[f"wind_battery_24h_ce16_mi{mi}"] = ("wind_battery_24h", dict(check_every=16, max_iter=mi), METRIC, "limit")
CASES["wind_battery_24h_ce16_restarts"] = ("wind_battery_24h", dict(check_every=16), METRIC, "restarts")
CASES["wind_battery_24h_ce4000_mi8200"] = ("wind_battery_24h", dict(check_every=4000, max_iter=8200, **NO_EVENT), METRIC, "limit")
for ce in (TABLE + 1, TABLE + 2):
    CASES[f"wind_battery_24h_ce{ce}_mi4200"] = ("wind_battery_24h", dict(check_every=ce, max_iter=4200, **NO_EVENT), METRIC, "limit")
CASES["nuclear_24h_ce3"] = ("nuclear_24h", dict(check_every=3, max_iter=2000), dict(matreg=1, rtc=0), None)
CASES["wind_battery_24h_no_matreg_ce3"] = ("wind_battery_24h", dict(no_matreg=1, check_every=3, max_iter=2000), dict(matreg=0), None)


def solve_case(name):
    """Solve one case with the library that is loaded; returns (results dict, dsp_stats)."""
    from dispatches_amd import scenarios
    from dispatches_amd.hip_solver import HipPdlpSolver
    from tools.make_check_path_fixture import _device_results
    workload, options, _, _ = CASES[name]
    solver = HipPdlpSolver(device=0, recertify=0, lazy_solution=False, **options)
    _, model = scenarios.make_batch(workload, B, solver)
    solver.solve(model)
    return _device_results(solver, model), solver.last_stats


def path_misses(name, res, stats):
    """Why this case's results do NOT come from the kernel the fixture is there for ([] = they do)."""
    return [f"dsp_stats.{k} = {getattr(stats, k)}, expected {v}" for k, v in CASES[name][2].items() if getattr(stats, k) != v]


def shape_misses(name, iters, jumps, status):
    """Why the RECORDED results of this case do not walk the path it is there for ([] = they do)."""
    options, shows = CASES[name][1], CASES[name][3]
    out = []
    if shows == "limit" and not ((iters == options["max_iter"]).all() and (jumps == 0).all()):
        out.append(f"not every scenario runs to the limit of {options['max_iter']} without a jump: iters {iters.tolist()}, jumps {jumps.tolist()}")
    if shows == "restarts" and not ((status == 0).all() and (jumps > 0).any() and (iters > 2 * 16).all()):
        out.append(f"no solved batch with ray jumps: status {status.tolist()}, iters {iters.tolist()}, jumps {jumps.tolist()}")
    return out


def main():
    from dispatches_amd.hip_solver import load_library
    lib = load_library()
    data = {"source_hash": np.array(lib.dsp_source_hash().decode()), "cases": np.array(list(CASES))}
    rows = {k: [] for k in KEYS}
    failed = False
    for name in CASES:
        res, stats = solve_case(name)
        misses = path_misses(name, res, stats) + shape_misses(name, res["iters"], res["jumps"], res["status"])
        print(f"{name}: matreg={stats.matreg} rtc={stats.rtc} cpl/rpl={stats.cols_per_lane}/{stats.rows_per_lane} "
              f"statuses={np.bincount(res['status']).tolist()} iters {res['iters'].tolist()} jumps {res['jumps'].tolist()}"
              + "".join(f"\n    MISSING: {m}" for m in misses), flush=True)
        failed |= bool(misses)
        for k in KEYS:
            rows[k].append(res[k])
    if failed:
        raise SystemExit("fixture NOT written: a case does not run the path it is there for")
    data.update({k: np.stack(v) for k, v in rows.items()})
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"wrote {out} ({os.path.getsize(out)} bytes), sources {data['source_hash']}")


if __name__ == "__main__":
    main()
