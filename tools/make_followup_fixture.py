"""GPU tool: record what the FOLLOW-UP passes of the fused PDLP solve compute - the certificate pass that takes over the suspects of
a register-resident first pass, and the re-certification passes (dsp_options::recertify_passes) - as the yardstick of changes to
how those passes are compiled and launched that must leave the results BIT-IDENTICAL (tests/test_hip_followup_passes.py).

    python tools/make_followup_fixture.py            # on the build whose results are the reference: writes the fixture

The batch is the 24-h wind + battery bidding LP, 8 scenarios, with scenarios 1, 4 and 6 made infeasible as in
tests/test_hip_infeasible.py (initial state of charge fixed at 1e6 kWh), solved through DeviceLP.solve in every way a caller
reaches the passes: with sync_stats (the host reads the count of suspects and sizes the certificate pass by it), without it on a
side stream (the fixed launch of 8 blocks), and without it on four streams at once, each with its own outputs; then all of that
again with recertify_passes = 3, which must change nothing because no scenario is flagged.  One more case provokes
DSP_FLAG_OBJ_WAIVED the way tests/test_hip_parity.py::test_device_side_recertification_passes does (polish patience 8 at an
objective tolerance of 5e-9) on 256 scenarios of the same LP with the three passes on, so that the passes have work: without
them the provocation leaves 6 of the 256 flagged, with them none (the recorder prints both counts).

Per leg the fixture holds status / iters / jumps / flags (int32), obj (float64) and one uint64 wrap-around sum of the bit
patterns of every scenario's x row and y row."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "followup_parent.npz")

B = 8
BAD = (1, 4, 6)
STATUSES = [0, 2, 0, 0, 2, 0, 2, 0]
N_STREAMS = 4
B_WAIVED = 256
WAIVED_OPTIONS = dict(polish_patience=8, eps_obj=5e-9)
KEYS = ("status", "iters", "jumps", "flags", "obj", "xsum", "ysum")

# case: (scenarios, infeasible scenarios, solver options, how it is launched, legs it yields)
CASES = {}
for _p, _o in (("", {}), ("recertify3_", dict(recertify_passes=3))):
    CASES[_p + "sync"] = (B, BAD, _o, "sync", [_p + "sync"])
    CASES[_p + "side_stream"] = (B, BAD, _o, "streams1", [_p + "side_stream"])
    CASES[_p + "four_streams"] = (B, BAD, _o, "streams4", [f"{_p}four_streams_{k}" for k in range(N_STREAMS)])
CASES["waived_recertify3_side_stream"] = (B_WAIVED, (), dict(recertify_passes=3, **WAIVED_OPTIONS), "streams1", ["waived_recertify3_side_stream"])
LEGS = [leg for case in CASES.values() for leg in case[4]]
INFEASIBLE_LEGS = [leg for case in CASES.values() if case[1] for leg in case[4]]


def _results(out, m):
    from tools.make_check_path_fixture import row_sums
    host = {k: out[k].cpu().numpy() for k in KEYS[:5] + ("x", "y")}
    return dict(status=host["status"].astype(np.int32), iters=host["iters"].astype(np.int32), jumps=host["jumps"].astype(np.int32),
                flags=host["flags"].astype(np.int32), obj=host["obj"].astype(np.float64), xsum=row_sums(host["x"]),
                ysum=row_sums(host["y"][:, :m]))


def solve_case(name, options=None):
    """Solve one case with the library that is loaded; returns ({leg: results dict}, dsp_stats of the last launch)."""
    import torch
    from dispatches_amd import scenarios
    from dispatches_amd.hip_solver import DeviceLP, HipPdlpSolver, default_options
    nb, bad, case_options, how, legs = CASES[name]
    options = case_options if options is None else options
    _, model = scenarios.make_batch("wind_battery_24h", nb, HipPdlpSolver(device=0))
    lp = model.lp
    full = lambda a: np.broadcast_to(a, (nb, a.shape[-1])).copy()
    lb, ub, rlo, rhi = (full(a) for a in model.scenario_bounds())
    j = lp.col_names.index("battery.initial_state_of_charge")
    lb[list(bad), j] = ub[list(bad), j] = 1.0e6                     # kWh; the battery holds 1e5
    up = lambda a: torch.as_tensor(np.array(a, dtype=np.float64)).cuda()
    opts = default_options(**{**(getattr(model, "solver_hints", None) or {}), **options})
    dlp = DeviceLP(lp, 0, opts)
    args = (nb, up(model.c), up(lb), up(ub), up(rlo), up(rhi))
    kw = dict(options=opts, obj_offset=up(np.broadcast_to(np.asarray(model.c0, np.float64), (nb,))))
    if how == "sync":
        outs = [dlp.solve(*args, sync_stats=True, **kw)]
    else:
        main = torch.cuda.current_stream()
        streams = [torch.cuda.Stream() for _ in legs]
        outs = []
        for s in streams:                                           # every launch is queued before any is waited for
            s.wait_stream(main)
            with torch.cuda.stream(s):
                outs.append(dlp.solve(*args, sync_stats=False, **kw))
        for s in streams:
            s.synchronize()
    stats = dlp.last_stats
    res = {leg: _results(out, lp.m) for leg, out in zip(legs, outs)}
    dlp.close()
    return res, stats


def path_misses(name, stats):
    """Why this case's results do NOT come from the kernels the fixture is there for ([] = they do)."""
    expect = dict(matreg=1, rtc=0, cols_per_lane=4, rows_per_lane=2, quadratic=0)
    return [f"dsp_stats.{k} = {getattr(stats, k)}, expected {v}" for k, v in expect.items() if getattr(stats, k) != v]


def main():
    from dispatches_amd.hip_solver import load_library
    lib = load_library()
    data = {"source_hash": np.array(lib.dsp_source_hash().decode()), "legs": np.array(LEGS)}
    failed = False
    for name in CASES:
        res, stats = solve_case(name)
        misses = path_misses(name, stats)
        for leg, r in res.items():
            if CASES[name][1] and r["status"].tolist() != STATUSES:
                misses.append(f"{leg}: statuses {r['status'].tolist()}")
            print(f"{leg}: B={len(r['status'])} statuses={np.bincount(r['status']).tolist()} iters {r['iters'].min()}..{r['iters'].max()} "
                  f"jumped {(r['jumps'] > 0).sum()} flagged {(r['flags'] & 1).sum()}", flush=True)
            for k in KEYS:
                data[f"{leg}/{k}"] = r[k]
        print("".join(f"    MISSING: {m}\n" for m in misses), end="", flush=True)
        failed |= bool(misses)
    # what the provocation flags when no pass follows (not stored: the test compares the case above)
    o = {k: v for k, v in CASES["waived_recertify3_side_stream"][2].items() if k != "recertify_passes"}
    res, _ = solve_case("waived_recertify3_side_stream", options=o)
    print(f"provocation without re-certification passes: flagged {int((res['waived_recertify3_side_stream']['flags'] & 1).sum())} of {B_WAIVED}")
    if failed:
        raise SystemExit("fixture NOT written: a case does not run the kernels it is there for")
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"wrote {out} ({os.path.getsize(out)} bytes), sources {data['source_hash']}")


if __name__ == "__main__":
    main()
