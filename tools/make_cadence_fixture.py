"""GPU tool: record what the fused PDLP kernel computes at the EDGES of its segment loop - check cadences 1, 2, 3 and 16 (no plain
iteration, one, two, the default fifteen between checks) against iteration limits that end the solve inside a segment, on a
check, or before the first one - as the yardstick of changes to the order of the plain-iteration loop that must leave the
results BIT-IDENTICAL (tests/test_hip_hot_loop_cadence.py).  tests/golden/check_path_parent.npz covers the default cadence only.

    python tools/make_cadence_fixture.py            # on the build whose results are the reference: writes the fixture

Per case the fixture holds status / iters / jumps / flags (int32), obj (float64) and one uint64 wrap-around sum of the bit
patterns of every scenario's x row and y row, for 32 scenarios (one [cases, 32] array per quantity, rows in the order of
`cases`): the full grid of cadences and limits on the 24-h metric shape, and cadences 1 and 3 under a limit of 2000 on the other
instantiations (another register-resident shape, the 4-h one, the generic LDS-matrix kernel, the QP and the run-time compiled
kernel).  Scenarios that stop at the iteration limit are as good as solved ones here: the bits are what is compared."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "hot_loop_cadence_parent.npz")

B = 32
CADENCES = (1, 2, 3, 16)
LIMITS = (1, 2, 16, 17, 47, None)        # None: the library's default
OTHER_LIMIT = 2000
KEYS = ("status", "iters", "jumps", "flags", "obj", "xsum", "ysum")

# name: (batch builder, solver options, expected dsp_stats fields)
CASES = {}
for ce in CADENCES:
    for mi in LIMITS:
        CASES[f"wind_battery_24h_ce{ce}_mi{mi or 'default'}"] = (
            ("day_ahead", "wind_battery_24h"), dict(check_every=ce, **({} if mi is None else dict(max_iter=mi))),
            dict(matreg=1, rtc=0, cols_per_lane=4, rows_per_lane=2))
for ce in (1, 3):
    o = dict(check_every=ce, max_iter=OTHER_LIMIT)
    CASES[f"nuclear_24h_ce{ce}"] = (("day_ahead", "nuclear_24h"), o, dict(matreg=1, rtc=0))
    CASES[f"wind_battery_rt4_no_simplex_ce{ce}"] = (("hourly", "wind_battery_rt4"), dict(no_simplex=1, **o),
                                                    dict(matreg=1, simplex=0, cols_per_lane=1, rows_per_lane=1))
    CASES[f"wind_battery_24h_no_matreg_ce{ce}"] = (("day_ahead", "wind_battery_24h"), dict(no_matreg=1, **o), dict(matreg=0))
    CASES[f"wind_battery_24h_qp01_ce{ce}"] = (("day_ahead", "wind_battery_24h_qp01"), o, dict(matreg=1, quadratic=1))
    CASES[f"wind_battery_30h_rtc_ce{ce}"] = (("horizon", 30), o, dict(matreg=1, rtc=1))


def solve_case(name):
    """Solve one case with the library that is loaded; returns (results dict, dsp_stats)."""
    from dispatches_amd import scenarios
    from dispatches_amd.hip_solver import HipPdlpSolver
    from tools.make_check_path_fixture import _device_results
    (kind, arg), options, _ = CASES[name]
    solver = HipPdlpSolver(device=0, recertify=0, lazy_solution=False, **options)
    if kind == "day_ahead":
        _, model = scenarios.make_batch(arg, B, solver)
    elif kind == "horizon":
        bidder, model = scenarios.wind_battery_batch(B, arg, solver)
        scenarios.load_prices(bidder, model)
    else:
        fx = np.load(os.path.join(ROOT, "tests", "golden", "oracle_hourly.npz"))
        inp = {k.split("/", 1)[1]: fx[k][:B] for k in fx.files if k.startswith(arg + "/")}
        _, model = scenarios.hourly_bid_batch(arg, inp, solver)
    solver.solve(model)
    return _device_results(solver, model), solver.last_stats


def path_misses(name, res, stats):
    """Why this case's results do NOT come from the kernel the fixture is there for ([] = they do)."""
    expect = CASES[name][2]
    return [f"dsp_stats.{k} = {getattr(stats, k)}, expected {v}" for k, v in expect.items() if getattr(stats, k) != v]


def main():
    from dispatches_amd.hip_solver import load_library
    lib = load_library()
    data = {"source_hash": np.array(lib.dsp_source_hash().decode()), "cases": np.array(list(CASES))}
    rows = {k: [] for k in KEYS}
    failed = False
    for name in CASES:
        res, stats = solve_case(name)
        misses = path_misses(name, res, stats)
        print(f"{name}: matreg={stats.matreg} rtc={stats.rtc} simplex={stats.simplex} quadratic={stats.quadratic} "
              f"cpl/rpl={stats.cols_per_lane}/{stats.rows_per_lane} statuses={np.bincount(res['status']).tolist()} "
              f"iters {res['iters'].min()}..{res['iters'].max()} jumped {(res['jumps'] > 0).sum()}"
              + "".join(f"\n    MISSING: {m}" for m in misses), flush=True)
        failed |= bool(misses)
        for k in KEYS:
            rows[k].append(res[k])
    if failed:
        raise SystemExit("fixture NOT written: a case does not run the kernel it is there for")
    data.update({k: np.stack(v) for k, v in rows.items()})
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"wrote {out} ({os.path.getsize(out)} bytes), sources {data['source_hash']}")


if __name__ == "__main__":
    main()
