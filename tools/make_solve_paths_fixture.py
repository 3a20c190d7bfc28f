"""GPU tool: record what dsp_solve returns on every branch of dsp_solve and dsp_create that the other bit-equality fixtures do not
reach, as the yardstick of host-side changes that must leave the results BIT-IDENTICAL (tests/test_hip_solve_paths.py).

    python tools/make_solve_paths_fixture.py            # on the build whose results are the reference: writes the fixture

A case is one handle (dsp_create under the case's options) and a list of solves on it; 4 scenarios unless the step says otherwise.
Per solve the fixture holds status / iters / jumps / flags (int32), obj (float64), one uint64 wrap-around sum of the bit patterns of
every scenario's x row and y row, and every field of dsp_stats but kernel_ms.  Every case is solved twice, each time on a fresh
handle: a fused, simplex, float32 or run-time compiled case that differs between the two runs is refused; a streaming solve that
differs is marked `loose` (the test then compares its objectives at the tolerance of tests/test_hip_stream.py)."""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "solve_paths_parent.npz")

F32 = dict(precision=1, eps_rel=1e-4, eps_obj=0.0, max_iter=20000)      # the float32 solves of tests/test_hip_qp.py
STATS = ("total_iterations", "max_iterations", "n_optimal", "grid_blocks", "block_threads", "lds_bytes", "cols_per_lane", "rows_per_lane",
         "matreg", "lds_conflicts_identity", "lds_conflicts_chosen", "simplex", "streaming", "stream_bytes_per_iteration", "quadratic",
         "precision", "rtc", "stream_form", "stream_phases", "ipm_solved")
KEYS = ("status", "iters", "jumps", "flags", "obj", "xsum", "ysum", "stats")
STATUS_ITERATION_LIMIT = 1

# name: (batch, options of dsp_create, steps, dsp_stats fields every step must show)
# step: (label, scenarios, options of this solve on top of the handle's, soft rows, sync_stats)
CASES = {
    "fused_matreg": ("wind_battery_24h", {}, [("defaults", 4, {}, False, True), ("wpb2", 4, dict(waves_per_block=2), False, True),
                                              ("defaults_again", 4, {}, False, True)], dict(matreg=1, rtc=0, simplex=0, streaming=0)),
    "generic": ("wind_battery_24h", dict(no_matreg=1), [("defaults", 4, {}, False, True)], dict(matreg=0, streaming=0)),
    "simplex_warm": ("wind_battery_track4", {}, [("b4", 4, dict(simplex_warm=1), False, True), ("b8_grown", 8, dict(simplex_warm=1), False, True),
                                                 ("b8_reused", 8, dict(simplex_warm=1), False, True)], dict(simplex=1)),
    "qp": ("wind_battery_24h_qp01", {}, [("float64", 4, {}, True, True), ("float32", 4, F32, True, True)], dict(quadratic=1, streaming=0)),
    "lp_float32": ("wind_battery_24h", {}, [("float32", 4, F32, False, True)], dict(precision=1, quadratic=0)),
    "rtc": ("wind_battery_20h_ramp", {}, [("lp", 4, {}, False, True), ("qp_lazy_compile", 4, {}, True, True)], dict(matreg=1, rtc=1)),
    # (no_interior_point: a precaution taken when the fixture was recorded, so that the case reaches the PDLP iteration and its max_iter exit
    #  whatever form dsp_create plans for the handle; the recorded default handle of this LP, streaming_one, shows ipm_solved = 0 as well)
    "streaming_limit": ("price_taker_168", dict(no_interior_point=1), [("limit", 2, dict(check_every=64, max_iter=128), False, True)],
                        dict(streaming=1)),
    "streaming_one": ("price_taker_168", {}, [("to_the_end", 1, dict(check_every=64), False, True)], dict(streaming=1)),
    "certificates": ("wind_battery_24h_infeasible", {}, [("host_reads_suspects", 8, {}, False, True), ("eight_blocks", 8, {}, False, False)],
                     dict(matreg=1, streaming=0)),
}
STREAMING = ("streaming_limit", "streaming_one")
INFEASIBLE = [1, 4, 6]


def build_batch(kind):
    """(lp, dict of [B, .] host arrays) of the largest batch a case solves; smaller steps take its first scenarios."""
    from dispatches_amd import scenarios
    from dispatches_amd.hip_solver import HipPdlpSolver
    solver = HipPdlpSolver(device=0, recertify=0, lazy_solution=False)
    if kind == "wind_battery_track4":
        fx = np.load(os.path.join(ROOT, "tests", "golden", "oracle_hourly.npz"))
        inp = {k.split("/", 1)[1]: fx[k][:8] for k in fx.files if k.startswith(kind + "/")}
        _, model = scenarios.hourly_tracking_batch(kind, inp, solver)
    elif kind == "wind_battery_20h_ramp":       # the shape tests/test_hip_parity.py compiles at run time, with soft ramp rows
        bidder, model = scenarios.wind_battery_batch(4, 20, solver, ramp_cost=0.1)
        scenarios.load_prices(bidder, model)
    elif kind == "price_taker_168":
        _, model = scenarios.price_taker_batch(168, 2, solver)
    elif kind == "wind_battery_24h_infeasible":  # tests/test_hip_infeasible.py: an initial state of charge of 10 x the battery
        _, model = scenarios.make_batch("wind_battery_24h", 8, solver)
    else:
        _, model = scenarios.make_batch(kind, 4, solver)
    B = model.n_scenario
    lb, ub, rlo, rhi = (np.broadcast_to(np.asarray(a, np.float64), (B, np.shape(a)[-1])).copy() for a in model.scenario_bounds())
    if kind == "wind_battery_24h_infeasible":
        j = model.lp.col_names.index("battery.initial_state_of_charge")
        lb[INFEASIBLE, j] = ub[INFEASIBLE, j] = 1.0e6
    c0 = np.broadcast_to(np.asarray(model.c0, np.float64), (B,)).copy()
    return model.lp, dict(c=np.asarray(model.c, np.float64), lb=lb, ub=ub, rlo=rlo, rhi=rhi, c0=c0)


def stats_row(stats):
    return np.array([getattr(stats, k) for k in STATS], np.int64)


def solve_case(name):
    """Create the case's handle with the library that is loaded and run its steps; returns {label: results dict}."""
    import torch
    from dispatches_amd.hip_solver import DeviceLP, default_options
    from tools.make_check_path_fixture import _device_results
    kind, create, steps, _ = CASES[name]
    lp, host = build_batch(kind)
    dev = torch.device("cuda", 0)
    dlp = DeviceLP(lp, 0, default_options(**create))
    kappa = getattr(lp, "row_compliance", None)
    results = {}
    for label, B, options, soft, sync in steps:
        t = {k: torch.as_tensor(np.ascontiguousarray(v[:B]), device=dev) for k, v in host.items()}
        out = dlp.solve(B, t["c"], t["lb"], t["ub"], t["rlo"], t["rhi"], obj_offset=t["c0"], sync_stats=sync,
                        options=default_options(**{**create, **options}),
                        row_compliance=torch.as_tensor(np.asarray(kappa, np.float64), device=dev) if soft else None)
        torch.cuda.synchronize(dev)
        res = _device_results(SimpleNamespace(last_device_out=out), SimpleNamespace(lp=lp))
        res["stats"] = stats_row(out["stats"])
        results[label] = res
    dlp.close()
    return results


def path_misses(name, results):
    """Why this case's results do NOT show the branch the fixture holds it for ([] = they do)."""
    _, _, steps, expect = CASES[name]
    bad = []
    for label, B, options, soft, sync in steps:
        res = results[label]
        stats = dict(zip(STATS, res["stats"].tolist()))
        bad += [f"{label}: dsp_stats.{k} = {stats[k]}, expected {v}" for k, v in expect.items() if stats[k] != v]
        bad += [f"{label}: dsp_stats.{k} = {stats[k]}, expected {v}" for k, v in (("quadratic", int(soft)), ("precision", options.get("precision", 0)))
                if stats[k] != v]
        if len(res["status"]) != B:
            bad.append(f"{label}: {len(res['status'])} scenarios, expected {B}")
    if name == "fused_matreg" and not np.array_equal(results["defaults"]["stats"], results["defaults_again"]["stats"]):
        bad.append("the requested geometry entered the handle's cache: the third solve's stats differ from the first's")
    if name == "fused_matreg" and results["wpb2"]["stats"][STATS.index("block_threads")] != 128:
        bad.append("waves_per_block=2 did not give blocks of 128 threads")
    if name == "streaming_limit" and not (results["limit"]["status"] == STATUS_ITERATION_LIMIT).all():
        bad.append(f"statuses {results['limit']['status'].tolist()}: not all at the iteration limit")
    if name == "certificates":
        for label in ("host_reads_suspects", "eight_blocks"):
            want = [2 if k in INFEASIBLE else 0 for k in range(8)]
            if results[label]["status"].tolist() != want:
                bad.append(f"{label}: statuses {results[label]['status'].tolist()}, expected {want}")
        if results["eight_blocks"]["stats"][STATS.index("n_optimal")] != 0:
            bad.append("eight_blocks: the asynchronous solve read the statuses back")
    return bad


def same_bits(a, b):
    """Two results of one solve agree in every array, floating-point ones by their bit patterns."""
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in KEYS)


def main():
    from dispatches_amd.hip_solver import load_library
    lib = load_library()
    data = {"source_hash": np.array(lib.dsp_source_hash().decode()), "stats_fields": np.array(STATS)}
    failed = False
    for name in CASES:
        first, second = solve_case(name), solve_case(name)
        misses = path_misses(name, first)
        for label, res in first.items():
            loose = not same_bits(res, second[label])
            if loose and name not in STREAMING:
                misses.append(f"{label}: two runs of this build differ")
            stats = dict(zip(STATS, res["stats"].tolist()))
            print(f"{name}/{label}: B={len(res['status'])} statuses={res['status'].tolist()} iters={res['iters'].tolist()} "
                  f"flagged {(res['flags'] != 0).sum()}{' LOOSE (two runs differ)' if loose else ''} "
                  + " ".join(f"{k}={v}" for k, v in stats.items() if v), flush=True)
            for k in KEYS:
                data[f"{name}/{label}/{k}"] = res[k]
            data[f"{name}/{label}/loose"] = np.array(int(loose))
        for m in misses:
            print(f"    MISSING: {m}", flush=True)
        failed |= bool(misses)
    if failed:
        raise SystemExit("fixture NOT written: a case misses the branch it is there for, or is not reproducible")
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"wrote {out} ({os.path.getsize(out)} bytes), sources {data['source_hash']}")


if __name__ == "__main__":
    main()
