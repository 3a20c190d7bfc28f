"""GPU tool: record what a solve returns in every form of the HBM-resident ("streaming") path and on every branch of its host layer
(csrc/dsp_stream.hip: stream_solve; csrc/dsp_stream_lane.hip: lane_run), as the yardstick of host-side changes that must leave the
results as they are (tests/test_hip_stream_forms.py).

    python tools/make_stream_forms_fixture.py            # on the build whose results are the reference: writes the fixture

A case is one handle of scenarios.price_taker_batch(T, B) under the case's development variables (set here and put back afterwards)
and one or two solves on it, check_every = 64.  Per solve the fixture holds what tools/make_solve_paths_fixture.py holds: status /
iters / jumps / flags (int32), obj (float64), one uint64 wrap-around sum of the bit patterns of every scenario's x row and y row, and
every field of dsp_stats but kernel_ms.  Every case is solved twice, each time on a fresh handle: a case whose floating-point outputs
differ between the two runs is marked `loose` (the test then compares its objectives at the tolerance of tests/test_hip_stream.py); a
case whose integer outputs or stats differ is refused.

The PDHG cases run with DSP_NO_IPM=1 like tests/test_hip_stream.py and tests/test_hip_infeasible.py (the interior-point form would take
these time-banded LPs first); `ipm_leaves_one` runs without it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "stream_forms_parent.npz")

from tools.make_solve_paths_fixture import KEYS, STATS, same_bits, stats_row     # noqa: E402  (one record layout for both fixtures)

TWO_LAUNCH, TILE, LANE, BLOCK, IPM = 1, 2, 3, 4, 5           # DSP_STREAM_FORM_* (include/dsp_hip.h)
STATUS_ITERATION_LIMIT, STATUS_PRIMAL_INFEASIBLE = 1, 2
ENV = ("DSP_NO_IPM", "DSP_STREAM_NO_LANE", "DSP_STREAM_NO_FUSED", "DSP_STREAM_NO_BLOCK", "DSP_LANE_MIN_B", "DSP_LANE_COMPACT", "DSP_LANE_ROWS",
       "DSP_LANE_WAVES", "DSP_LANE_GRAPH", "DSP_FUSED_V", "DSP_FUSED_RB", "DSP_FUSED_XCD", "DSP_FUSED_DEFER")
NO_LANE = {"DSP_STREAM_NO_LANE": "1"}
NO_FUSED = {"DSP_STREAM_NO_LANE": "1", "DSP_STREAM_NO_FUSED": "1"}
# the smallest of 72, 96, 130 scenarios at which the recording build packs the scenarios still iterating into fewer lane groups
# (stream_phases >= 2; main() looks for it and refuses to write a fixture that disagrees)
LANE_REPACK_B = 72
BAD = 3                                                      # the member that gets an impossible power balance


def grid_limits(model):
    """A grid-connection limit per member (tests/test_hip_stream.py): the column bounds differ per scenario on short columns."""
    B = model.n_scenario
    lb, ub, _, _ = model.block.current_bounds()
    model.lb, model.ub = np.tile(lb, (B, 1)), np.tile(ub, (B, 1))
    cols = [j for j, name in enumerate(model.lp.col_names) if name.startswith("splitter.grid_elec[")]
    for k in range(B):
        model.ub[k, cols] = 847.0e3 * (0.55 + 0.4 * ((37 * k) % B) / B if B > 6 else 0.55 + 0.08 * k)


def infeasible_member(model):
    """tests/test_hip_infeasible.py: member 3's splitter row of period 5 asks for 1e9 kW more than the wind plant can deliver."""
    B = model.n_scenario
    full = lambda a: np.broadcast_to(a, (B, a.shape[-1])).copy()
    model.lb, model.ub, model.rlo, model.rhi = (full(a) for a in model.scenario_bounds())
    model.c = model.c.copy()
    model.x = model.y = None
    i = model.lp.row_names.index("splitter.sum_split[5]")
    model.rlo[BAD, i] = model.rhi[BAD, i] = 1.0e9


def infeasible_member_rows_only(model):
    """tests/test_hip_ipm.py::test_an_infeasible_member_alone_goes_to_the_pdhg_forms: the same edit on per-scenario ROW bounds only."""
    B = model.n_scenario
    _, _, rlo, rhi = model.scenario_bounds()
    model.rlo, model.rhi = np.tile(rlo, (B, 1)), np.tile(rhi, (B, 1))
    i = next(i for i, nm in enumerate(model.lp.row_names) if nm.startswith("splitter.sum_split[5]"))
    model.rlo[BAD, i] = model.rhi[BAD, i] = 1e9


def case(T, B, env, form, *, mutate=None, solves=1, ipm=False, throughput="two_level", max_iter=400_000, **expect):
    return dict(T=T, B=B, env={**({} if ipm else {"DSP_NO_IPM": "1"}), **env}, form=form, mutate=mutate, solves=solves, throughput=throughput,
                max_iter=max_iter, expect=expect)


# expect: phases (stream_phases), shared (False: the per-scenario byte figure), bad (member 3 certified infeasible), limit (all at max_iter),
# ipm_solved
CASES = {
    "two_launch_chain": case(336, 6, NO_FUSED, TWO_LAUNCH, throughput="chain"),
    "two_launch_long_columns": case(336, 6, NO_FUSED, TWO_LAUNCH),                       # two_level: the *_long_finish launches
    "tile_deferred": case(336, 6, NO_LANE, TILE),
    "tile_staged": case(336, 6, {**NO_LANE, "DSP_FUSED_V": "1"}, TILE),
    "tile_small_tiles": case(336, 6, {**NO_LANE, "DSP_FUSED_RB": "64"}, TILE),
    "tile_per_scenario_bounds": case(336, 6, NO_LANE, TILE, mutate=grid_limits, shared=False),
    "lane_one_phase": case(336, 6, {"DSP_LANE_MIN_B": "1"}, LANE, phases=1),
    "lane_repacking": case(336, LANE_REPACK_B, {}, LANE, phases=">=2"),
    "lane_no_repacking": case(336, LANE_REPACK_B, {"DSP_LANE_COMPACT": "0"}, LANE, phases=1),
    "lane_per_scenario_bounds": case(336, 40, {}, LANE, mutate=grid_limits, shared=False),
    # (two solves: the second one's report is the first one's - nothing of another solve stays in the handle)
    "block": case(96, 5, {}, BLOCK, solves=2),
    "certificate_lane": case(336, 40, {}, LANE, mutate=infeasible_member, bad=True),     # certify, then repack
    "certificate_tile": case(336, 6, NO_LANE, TILE, mutate=infeasible_member, bad=True),  # stream_certify from the period loop
    "certificate_two_launch": case(336, 6, NO_FUSED, TWO_LAUNCH, mutate=infeasible_member, bad=True),
    "certificate_block": case(96, 5, {}, BLOCK, mutate=infeasible_member, bad=True),     # in-kernel
    "limit_tile": case(336, 6, NO_LANE, TILE, max_iter=128, limit=True),
    "limit_lane": case(336, 6, {"DSP_LANE_MIN_B": "1"}, LANE, max_iter=128, limit=True, phases=1),
    # the interior-point form solves five members and gives up on the infeasible one; that subset is below DSP_LANE_MIN_B, so the lane
    # form passes and the member goes to the first of the other forms that applies (at this size: the block form)
    "ipm_leaves_one": case(168, 6, {}, IPM, mutate=infeasible_member_rows_only, ipm=True, throughput="chain", bad=True, ipm_solved=5),
}


def solve_case(name, B=None):
    """Build the case's batch and handle under its environment with the library that is loaded, run its solves; {label: results dict}."""
    from dispatches_amd import scenarios
    from dispatches_amd.hip_solver import HipPdlpSolver
    from tools.make_check_path_fixture import _device_results
    c = CASES[name]
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update(c["env"])
    try:
        solver = HipPdlpSolver(device=0, recertify=0, lazy_solution=False, check_every=64, max_iter=c["max_iter"])
        _, model = scenarios.price_taker_batch(c["T"], B or c["B"], solver, throughput=c["throughput"])
        if c["mutate"]:
            c["mutate"](model)
        results = {}
        for k in range(c["solves"]):
            solver.solve(model)
            res = _device_results(solver, model)
            res["stats"] = stats_row(solver.last_stats)
            res["nm"] = np.array([model.lp.n, model.lp.m], np.int64)
            results[f"solve{k}"] = res
        return results
    finally:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def form_misses(name, results):
    """Why this case's results do NOT show the form and branch the fixture holds it for ([] = they do)."""
    c = CASES[name]
    expect = c["expect"]
    bad = []
    if len(results) != c["solves"]:
        bad.append(f"{len(results)} solves, expected {c['solves']}")
    for label, res in results.items():
        stats = dict(zip(STATS, res["stats"].tolist()))
        n, m = (int(v) for v in res["nm"])
        B = len(res["status"])
        want = dict(streaming=1, stream_form=c["form"], ipm_solved=expect.get("ipm_solved", 0))
        one_launch = 8 * (4 * n + 3 * m) if expect.get("shared", True) else 8 * (6 * n + 5 * m)
        # the block form and the two-launch form report the two-launch figure; the edited member gives every scenario bounds of its own
        if c["form"] in (TWO_LAUNCH, BLOCK):
            want["stream_bytes_per_iteration"] = 8 * (8 * n + 6 * m)
        elif c["form"] in (TILE, LANE):
            want["stream_bytes_per_iteration"] = 8 * (6 * n + 5 * m) if expect.get("bad") else one_launch
        if isinstance(expect.get("phases"), int):
            want["stream_phases"] = expect["phases"]
        bad += [f"{label}: dsp_stats.{k} = {stats[k]}, expected {v}" for k, v in want.items() if stats[k] != v]
        if expect.get("phases") == ">=2" and stats["stream_phases"] < 2:
            bad.append(f"{label}: stream_phases = {stats['stream_phases']}, expected >= 2")
        if B != c["B"]:
            bad.append(f"{label}: {B} scenarios, expected {c['B']}")
        status = [STATUS_PRIMAL_INFEASIBLE if expect.get("bad") and k == BAD else (STATUS_ITERATION_LIMIT if expect.get("limit") else 0) for k in range(B)]
        if res["status"].tolist() != status:
            bad.append(f"{label}: statuses {res['status'].tolist()}, expected {status}")
        if expect.get("limit") and not (res["iters"] == c["max_iter"]).all():
            bad.append(f"{label}: iteration counts {res['iters'].tolist()}, expected {c['max_iter']}")
    if c["solves"] == 2 and len(results) == 2 and not np.array_equal(results["solve0"]["stats"], results["solve1"]["stats"]):
        bad.append("the second solve of the handle reports other stats than the first")
    return bad


RECORDED = KEYS + ("nm",)


def main():
    from dispatches_amd.hip_solver import load_library
    lib = load_library()
    data = {"source_hash": np.array(lib.dsp_source_hash().decode()), "stats_fields": np.array(STATS)}
    failed = False
    ph = STATS.index("stream_phases")
    smallest = next((B for B in (72, 96, 130) if solve_case("lane_repacking", B)["solve0"]["stats"][ph] >= 2), None)
    print(f"lane form: phases >= 2 from B = {smallest} (of 72, 96, 130); LANE_REPACK_B = {LANE_REPACK_B}", flush=True)
    failed |= smallest != LANE_REPACK_B
    data["lane_repack_B"] = np.array(LANE_REPACK_B)
    for name in CASES:
        first, second = solve_case(name), solve_case(name)
        misses = form_misses(name, first)
        for label, res in first.items():
            loose = not same_bits(res, second[label])
            if any(not np.array_equal(res[k], second[label][k]) for k in ("status", "iters", "jumps", "flags", "stats")):
                misses.append(f"{label}: integer outputs or stats differ between two runs of this build")
            stats = dict(zip(STATS, res["stats"].tolist()))
            print(f"{name}/{label}: B={len(res['status'])} statuses={res['status'].tolist()} iters={res['iters'].tolist()[:8]} "
                  f"{' LOOSE (two runs differ)' if loose else ''} " + " ".join(f"{k}={v}" for k, v in stats.items() if v), flush=True)
            for k in RECORDED:
                data[f"{name}/{label}/{k}"] = res[k]
            data[f"{name}/{label}/loose"] = np.array(int(loose))
        for m in misses:
            print(f"    MISSING: {m}", flush=True)
        failed |= bool(misses)
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    if failed:
        out += ".refused.npz"
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"wrote {out} ({os.path.getsize(out)} bytes), sources {data['source_hash']}")
    if failed:
        raise SystemExit("fixture REFUSED: a case misses the form it is there for, or its integer outputs are not reproducible")


if __name__ == "__main__":
    main()
