"""GPU tool: record what the fused PDLP kernel computes on the small cases that reach every path of its check iteration (KKT
test, restart, ray jump, warm start given up, iteration-limit epilogue; the register-resident, generic, QP and run-time compiled
instantiations), as the yardstick of changes that must leave the results BIT-IDENTICAL (tests/test_hip_check_path.py).

    python tools/make_check_path_fixture.py            # on the build whose results are the reference: writes the fixture

Per case the fixture holds status / iters / jumps / flags (int32), obj (float64) and one uint64 wrap-around sum of the bit
patterns of every scenario's x row and y row; the two warm-start cases also hold the primal weights read back.  A few KB.
The recorder refuses to write a fixture that misses a path: every PDLP case needs a scenario that jumped, the warm cases one
that gave its warm start up (and one that did not), the iteration-limit case nothing but iteration limits.  Two cases cannot jump
and are exempt (NO_JUMP): no scenario of the 24-h batch jumps within its first 600 iterations, so none does under max_iter = 200;
and the first 64 wind + PEM scenarios converge in 204 - 300 iterations without a steady stretch - the first of that batch to jump
is scenario 193, so the 256-scenario case beside it covers the ray jump of the long-vector kernel."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "check_path_parent.npz")

WARM_PATIENCE = 256         # iterations a warm start gets before the solve starts over from the cold point
WARM_PERTURBATION = 1e-6    # relative; from there the 64 scenarios need 144 - 768 iterations when left alone: some make it, some give up
NO_JUMP = ("wind_pem_48h", "wind_battery_24h_max_iter")
MAX_ITER_SHORT = 200        # the iteration-limit case
STATUS_ITERATION_LIMIT = 1

# name: (batch builder, scenarios, solver options, expected dsp_stats fields)
CASES = {
    "wind_battery_24h": (("day_ahead", "wind_battery_24h"), 256, {}, dict(matreg=1, rtc=0, cols_per_lane=4, rows_per_lane=2)),
    "wind_battery_48h": (("day_ahead", "wind_battery_48h"), 128, {}, dict(matreg=1, rtc=0, cols_per_lane=7, rows_per_lane=4)),
    "wind_pem_48h": (("day_ahead", "wind_pem_48h"), 64, {}, dict(matreg=1, rtc=0)),
    "wind_pem_48h_256": (("day_ahead", "wind_pem_48h"), 256, {}, dict(matreg=1, rtc=0)),
    "nuclear_24h": (("day_ahead", "nuclear_24h"), 64, {}, dict(matreg=1, rtc=0)),
    "wind_battery_rt4_no_simplex": (("hourly", "wind_battery_rt4"), 64, dict(no_simplex=1),
                                    dict(matreg=1, simplex=0, cols_per_lane=1, rows_per_lane=1)),
    "wind_battery_24h_qp01": (("day_ahead", "wind_battery_24h_qp01"), 64, {}, dict(matreg=1, quadratic=1)),
    "wind_battery_24h_no_matreg": (("day_ahead", "wind_battery_24h"), 64, dict(no_matreg=1), dict(matreg=0)),
    "wind_battery_30h_rtc": (("horizon", 30), 32, {}, dict(matreg=1, rtc=1)),
    "wind_battery_24h_max_iter": (("day_ahead", "wind_battery_24h"), 64, dict(max_iter=MAX_ITER_SHORT), dict(matreg=1)),
    "wind_battery_24h_warm": (("warm", False), 64, dict(warm_patience=WARM_PATIENCE), dict(matreg=1)),
    "wind_battery_24h_warm_weight": (("warm", True), 64, dict(warm_patience=WARM_PATIENCE), dict(matreg=1)),
}


def row_sums(a):
    """uint64 wrap-around sum of the bit patterns of every row."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64).sum(axis=1, dtype=np.uint64)


def _device_results(solver, model):
    out = solver.last_device_out
    m = model.lp.m
    host = {k: out[k].cpu().numpy() for k in ("x", "y", "obj", "status", "iters", "jumps", "flags")}
    return dict(status=host["status"].astype(np.int32), iters=host["iters"].astype(np.int32), jumps=host["jumps"].astype(np.int32),
                flags=host["flags"].astype(np.int32), obj=host["obj"].astype(np.float64), xsum=row_sums(host["x"]),
                ysum=row_sums(host["y"][:, :m]))


def solve_case(name):
    """Solve one case with the library that is loaded; returns (results dict, dsp_stats)."""
    from dispatches_amd import scenarios
    from dispatches_amd.hip_solver import HipPdlpSolver
    (kind, arg), B, options, _ = CASES[name]
    solver = HipPdlpSolver(device=0, recertify=0, lazy_solution=False, **options)
    if kind == "day_ahead":
        _, model = scenarios.make_batch(arg, B, solver)
    elif kind == "horizon":
        bidder, model = scenarios.wind_battery_batch(B, arg, solver)
        scenarios.load_prices(bidder, model)
    elif kind == "hourly":
        fx = np.load(os.path.join(ROOT, "tests", "golden", "oracle_hourly.npz"))
        inp = {k.split("/", 1)[1]: fx[k][:B] for k in fx.files if k.startswith(arg + "/")}
        _, model = scenarios.hourly_bid_batch(arg, inp, solver)
    else:
        # warm start from a perturbed solution: the cold solve of the same build (no patience set), every entry moved by up to
        # WARM_PERTURBATION (relative) with a fixed seed - some scenarios finish within the patience, the others start over cold
        cold = HipPdlpSolver(device=0, recertify=0, lazy_solution=False)
        _, model = scenarios.make_batch("wind_battery_24h", B, cold)
        cold.solve(model)
        rng = np.random.default_rng(20240613)
        model.x = model.x * (1.0 + WARM_PERTURBATION * rng.uniform(-1.0, 1.0, model.x.shape))
        model.y = model.y * (1.0 + WARM_PERTURBATION * rng.uniform(-1.0, 1.0, model.y.shape))
        if not arg:
            model.primal_weight = None            # automatic weight; the final weights are still read back
        model.solve_handle = None                 # a handle of its own, created under this case's options
        solver.solve(model, warm_start=True)
        res = _device_results(solver, model)
        res["pw"] = np.asarray(model.primal_weight, np.float64).copy()
        return res, solver.last_stats
    solver.solve(model)
    return _device_results(solver, model), solver.last_stats


def path_misses(name, res, stats):
    """Why this case's results do NOT reach the paths the fixture is there for ([] = they do)."""
    (kind, _), _, options, expect = CASES[name]
    bad = [f"dsp_stats.{k} = {getattr(stats, k)}, expected {v}" for k, v in expect.items() if getattr(stats, k) != v]
    if name not in NO_JUMP and not (res["jumps"] > 0).any():
        bad.append("no scenario made a ray jump")
    if kind == "warm" and not (res["iters"] > WARM_PATIENCE).any():
        bad.append(f"no scenario ran past warm_patience = {WARM_PATIENCE}")
    if kind == "warm" and not (res["iters"] <= WARM_PATIENCE).any():
        bad.append(f"no scenario finished within warm_patience = {WARM_PATIENCE}")
    if "max_iter" in options and not (res["status"] == STATUS_ITERATION_LIMIT).all():
        bad.append(f"statuses {np.bincount(res['status'])}: not all at the iteration limit")
    return bad


def main():
    from dispatches_amd.hip_solver import load_library
    lib = load_library()
    data = {"source_hash": np.array(lib.dsp_source_hash().decode())}
    failed = False
    for name in CASES:
        res, stats = solve_case(name)
        misses = path_misses(name, res, stats)
        print(f"{name}: B={len(res['status'])} matreg={stats.matreg} rtc={stats.rtc} simplex={stats.simplex} quadratic={stats.quadratic} "
              f"cpl/rpl={stats.cols_per_lane}/{stats.rows_per_lane} statuses={np.bincount(res['status']).tolist()} "
              f"iters {res['iters'].min()}..{res['iters'].max()} jumped {(res['jumps'] > 0).sum()} flagged {(res['flags'] != 0).sum()}"
              + "".join(f"\n    MISSING: {m}" for m in misses), flush=True)
        failed |= bool(misses)
        for k, v in res.items():
            data[f"{name}/{k}"] = v
    if failed:
        raise SystemExit("fixture NOT written: a case misses a path it is there for")
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"wrote {out} ({os.path.getsize(out)} bytes), sources {data['source_hash']}")


if __name__ == "__main__":
    main()
