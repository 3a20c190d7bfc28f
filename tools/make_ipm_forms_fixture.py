"""GPU tool: record what a solve returns on every branch of the interior-point form's host layer (csrc/dsp_ipm.hip: ipm_create,
ipm_workspace, ipm_loop, ipm_repack; csrc/dsp_ipm_plan.hpp), as the yardstick of host-side changes that must leave the results as
they are (tests/test_hip_ipm_forms.py).

    DSP_LIB=<the library built from the reference commit's csrc/> python tools/make_ipm_forms_fixture.py      # writes the fixture

A case is one handle of a one-week wind + battery LP (scenarios.price_taker_batch(168, B, throughput="chain"): n = 1011, m = 1010,
half-bandwidth 6, one wide column) or of the four-week nuclear LP (nuclear_price_taker_batch(672, 12): half-bandwidth 8, no wide
column) under the case's development variables (set here and put back afterwards), and one or more solves on it, check_every = 64.
The record layout is that of tools/make_solve_paths_fixture.py and tools/make_stream_forms_fixture.py.  A case that runs under
DSP_IPM_TRACE also records what the form printed: how often it packed its lanes, its last `steps taken back` line and its `lanes`
line.  Every case is solved twice, each time on a fresh handle: a case whose floating-point outputs differ between the two runs is
marked `loose`; a case whose integer outputs, stats or printed lines differ is refused.

Two settings are looked for on the recording build, and a fixture that disagrees with the constants below is refused: the smallest
batch at which the form packs its lanes (PACK_B), and a small LP on which a step is taken back (TAKEN_BACK; None: no setting tried
reaches k_ipm_undo, and the branch stays with tests/test_hip_ipm.py::test_year_long_batch_of_256_distinct_lps[steps_taken_back])."""
import contextlib
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "ipm_forms_parent.npz")

from tools.make_solve_paths_fixture import KEYS, STATS, same_bits, stats_row     # noqa: E402  (one record layout for the fixtures)
from tools.make_stream_forms_fixture import BAD, IPM, infeasible_member_rows_only     # noqa: E402

ENV = ("DSP_NO_IPM", "DSP_IPM_PARTS", "DSP_IPM_COMPACT", "DSP_IPM_MAXIT", "DSP_IPM_TRACE", "DSP_IPM_DEBUG", "DSP_IPM_REFTOL_END")
TRACE = {"DSP_IPM_TRACE": "1"}
# the smallest of 72, 96, 130 members of the wide family at which the recording build packs the lanes still iterating into fewer groups
PACK_B = 72
PACK_CANDIDATES = (72, 96, 130)
# (T, DSP_IPM_REFTOL_END) of the first setting at which the recording build takes a step back on TAKEN_BACK_B members of the wide family
TAKEN_BACK = None
TAKEN_BACK_B = 64
TAKEN_BACK_CANDIDATES = tuple((T, tol) for T in (168, 672) for tol in ("1e-7", "1e-5", "1e-3"))
INTS = ("status", "iters", "jumps", "flags", "stats", "nm")
TEXT = ("packed", "taken_back", "lanes")                     # of a traced solve: int64, two strings


def case(steps, env=None, *, kind="wind_battery", T=168, family="base", mutate=None, max_iter=1_000_000, **expect):
    """steps: the batch sizes solved one after the other on the case's handle (the first `B` members of its largest batch)."""
    steps = (steps,) if isinstance(steps, int) else tuple(steps)
    return dict(steps=steps, env=dict(env or {}), kind=kind, T=T, family=family, mutate=mutate, max_iter=max_iter, expect=expect)


def _taken_back_case(setting):
    T, tol = setting
    return case(TAKEN_BACK_B, {**TRACE, "DSP_IPM_REFTOL_END": tol}, T=T, family="wide", taken_back=True)


# expect: phases (stream_phases; "auto": what the rows give), ipm_solved (default: all), bad (member 3 certified infeasible),
# packed (True / False: the trace shows a packing / none), taken_back (the trace counts a step taken back)
CASES = {
    "default": case(16, phases=3),                                                   # W = 6, one wide column, three partitions
    "sequential_walks": case(16, {"DSP_IPM_PARTS": "1"}, phases=1),
    "ragged_partitions": case(16, {"DSP_IPM_PARTS": "9"}, phases=9),
    "nuclear": case(12, kind="nuclear", T=672, phases="auto"),                       # W = 8, no wide column, the one-wave reduced solve
    "nuclear_31_partitions": case(12, {"DSP_IPM_PARTS": "31"}, kind="nuclear", T=672, phases=31),
    "lane_packing": case(PACK_B, TRACE, family="wide", packed=True),
    "no_packing": case(PACK_B, {**TRACE, "DSP_IPM_COMPACT": "0"}, family="wide", packed=False),
    "ragged_lane_groups": case(80),                                                  # two lane groups, the second one ragged
    "gives_up_on_one": case(6, mutate=infeasible_member_rows_only, max_iter=400_000, bad=True, ipm_solved=5),
    "warm_hand_off": case(6, {"DSP_IPM_MAXIT": "5"}, ipm_solved=0),                  # every member finishes in the PDHG forms
    "workspace_reuse": case((6, 80, 6)),                                             # one handle: the workspace grows, then is reused
    "trace": case(16, TRACE, phases=3),                                              # the bits of `default`
}
if TAKEN_BACK is not None:
    CASES["steps_taken_back"] = _taken_back_case(TAKEN_BACK)


@contextlib.contextmanager
def stderr_text():
    """What the process writes to file descriptor 2 inside the block (the library's own fprintf included), as box[0] afterwards; it is
    passed on to the stderr in place before."""
    sys.stderr.flush()
    saved = os.dup(2)
    box = []
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            yield box
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
            tmp.seek(0)
            box.append(tmp.read().decode(errors="replace"))
            sys.stderr.write(box[0])


def trace_record(text):
    """How often the form packed its lanes, its last `steps taken back` line and its `lanes` line, from what it printed."""
    lines = [ln for ln in text.splitlines() if ln.startswith("[ipm] ")]
    back = [ln for ln in lines if ln.startswith("[ipm] steps taken back:")]
    lanes = [ln for ln in lines if ln.startswith("[ipm] lanes (state:newton iterations):")]
    packed = [ln for ln in lines if re.search(r"packed into \d+ group\(s\)$", ln)]
    return dict(packed=np.array(len(packed), np.int64), taken_back=np.array(back[-1] if back else ""), lanes=np.array(lanes[-1] if lanes else ""))


def build_batch(c, B):
    from dispatches_amd import scenarios
    from dispatches_amd.hip_solver import HipPdlpSolver
    solver = HipPdlpSolver(device=0, recertify=0, lazy_solution=False)
    if c["kind"] == "nuclear":
        _, model = scenarios.nuclear_price_taker_batch(c["T"], B, solver)
    else:
        _, model = scenarios.price_taker_batch(c["T"], B, solver, throughput="chain", family=c["family"])
    if c["mutate"]:
        c["mutate"](model)
    host = dict(zip(("lb", "ub", "rlo", "rhi"), (np.ascontiguousarray(a, np.float64) for a in model.scenario_bounds())))
    host["c"] = np.ascontiguousarray(model.c, np.float64)
    host["c0"] = np.broadcast_to(np.asarray(model.c0, np.float64), (B,)).copy()
    return model, host


def solve_case(name, c=None):
    """Build the case's batch and handle under its environment with the library that is loaded, run its solves; {label: results dict}.
    DeviceLP.solve is the entry that lets one handle take batches of different sizes."""
    import torch
    from types import SimpleNamespace
    from dispatches_amd.hip_solver import DeviceLP, default_options
    from tools.make_check_path_fixture import _device_results
    c = c or CASES[name]
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update(c["env"])
    try:
        model, host = build_batch(c, max(c["steps"]))
        lp, dev = model.lp, torch.device("cuda", 0)
        options = default_options(**{**dict(getattr(model, "solver_hints", None) or {}), "check_every": 64, "max_iter": c["max_iter"]})
        dlp = DeviceLP(lp, 0, options)
        results = {}
        for k, B in enumerate(c["steps"]):
            t = {key: torch.as_tensor(np.ascontiguousarray(v[:B] if v.ndim == 2 or key == "c0" else v), device=dev) for key, v in host.items()}
            with stderr_text() as printed:
                out = dlp.solve(B, t["c"], t["lb"], t["ub"], t["rlo"], t["rhi"], obj_offset=t["c0"], options=options)
                torch.cuda.synchronize(dev)
            res = _device_results(SimpleNamespace(last_device_out=out), SimpleNamespace(lp=lp))
            res["stats"] = stats_row(out["stats"])
            res["nm"] = np.array([lp.n, lp.m], np.int64)
            if "DSP_IPM_TRACE" in c["env"]:
                res.update(trace_record(printed[0]))
            results[f"solve{k}"] = res
        dlp.close()
        return results
    finally:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def recorded_keys(c):
    return KEYS + ("nm",) + (TEXT if "DSP_IPM_TRACE" in c["env"] else ())


def steps_back(res):
    found = re.search(r"steps taken back: (\d+)", str(res.get("taken_back", "")))
    return int(found.group(1)) if found else -1


def form_misses(name, results, c=None):
    """Why this case's results do NOT show the branch the fixture holds it for ([] = they do)."""
    c = c or CASES[name]
    expect = c["expect"]
    bad = []
    if len(results) != len(c["steps"]):
        bad.append(f"{len(results)} solves, expected {len(c['steps'])}")
    for (label, res), B in zip(results.items(), c["steps"]):
        stats = dict(zip(STATS, res["stats"].tolist()))
        m = int(res["nm"][1])
        want = dict(streaming=1, ipm_solved=expect.get("ipm_solved", B))
        if want["ipm_solved"] > 0:
            want["stream_form"] = IPM
        elif stats["stream_form"] == IPM or (res["iters"] <= 300).any():         # (PDHG iterations; the form itself counts Newton iterations)
            bad.append(f"{label}: form {stats['stream_form']}, iterations {res['iters'].tolist()}: not every member went through the PDHG forms")
        if "phases" in expect:
            want["stream_phases"] = (min(64, m // 256) if m >= 512 else 1) if expect["phases"] == "auto" else expect["phases"]
        bad += [f"{label}: dsp_stats.{k} = {stats[k]}, expected {v}" for k, v in want.items() if stats[k] != v]
        if len(res["status"]) != B:
            bad.append(f"{label}: {len(res['status'])} scenarios, expected {B}")
        status = [2 if expect.get("bad") and k == BAD else 0 for k in range(B)]
        if res["status"].tolist() != status:
            bad.append(f"{label}: statuses {res['status'].tolist()}, expected {status}")
        if "DSP_IPM_TRACE" in c["env"]:
            if not str(res["lanes"]).startswith("[ipm] lanes") or len(str(res["lanes"]).split()) != 4 + B or steps_back(res) < 0:
                bad.append(f"{label}: no complete trace ({str(res['taken_back'])!r}, {str(res['lanes'])[:60]!r})")
            if "packed" in expect and (int(res["packed"]) > 0) != expect["packed"]:
                bad.append(f"{label}: the lanes were packed {int(res['packed'])} time(s), expected {'some' if expect['packed'] else 'none'}")
            if expect.get("taken_back") and steps_back(res) < 1:
                bad.append(f"{label}: {str(res['taken_back'])!r}, expected a step taken back")
    return bad


def main():
    from dispatches_amd.hip_solver import load_library
    lib = load_library()
    data = {"source_hash": np.array(lib.dsp_source_hash().decode()), "stats_fields": np.array(STATS)}
    failed = False
    smallest = next((B for B in PACK_CANDIDATES
                     if int(solve_case("lane_packing", case(B, TRACE, family="wide"))["solve0"]["packed"]) > 0), None)
    print(f"lanes packed from B = {smallest} (of {PACK_CANDIDATES}); PACK_B = {PACK_B}", flush=True)
    failed |= smallest != PACK_B
    data["pack_B"] = np.array(PACK_B)
    found = None
    for setting in TAKEN_BACK_CANDIDATES:
        count = steps_back(solve_case("steps_taken_back", _taken_back_case(setting))["solve0"])
        print(f"T = {setting[0]}, DSP_IPM_REFTOL_END = {setting[1]}, {TAKEN_BACK_B} wide members: {count} step(s) taken back", flush=True)
        if count >= 1:
            found = setting
            break
    print(f"steps taken back first at {found}; TAKEN_BACK = {TAKEN_BACK}", flush=True)
    failed |= found != TAKEN_BACK
    data["taken_back_found"] = np.array(int(TAKEN_BACK is not None))
    data["taken_back_setting"] = np.array(list(map(str, TAKEN_BACK or ())), dtype=str)
    for name, c in CASES.items():
        first, second = solve_case(name), solve_case(name)
        misses = form_misses(name, first)
        for label, res in first.items():
            loose = not same_bits(res, second[label])
            exact = INTS + (TEXT if "DSP_IPM_TRACE" in c["env"] else ())
            if any(not np.array_equal(res[k], second[label][k]) for k in exact):
                misses.append(f"{label}: integer outputs, stats or printed lines differ between two runs of this build")
            stats = dict(zip(STATS, res["stats"].tolist()))
            print(f"{name}/{label}: B={len(res['status'])} statuses={res['status'].tolist()[:8]} iters={res['iters'].tolist()[:8]} "
                  f"{' LOOSE (two runs differ)' if loose else ''} " + " ".join(f"{k}={v}" for k, v in stats.items() if v), flush=True)
            for k in recorded_keys(c):
                data[f"{name}/{label}/{k}"] = res[k]
            data[f"{name}/{label}/loose"] = np.array(int(loose))
        for miss in misses:
            print(f"    MISSING: {miss}", flush=True)
        failed |= bool(misses)
    for key in KEYS:                                                                 # the trace changes nothing
        if data[f"trace/solve0/{key}"].tobytes() != data[f"default/solve0/{key}"].tobytes():
            print(f"    MISSING: trace/solve0/{key} differs from default/solve0/{key}", flush=True)
            failed = True
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    if failed:
        out += ".refused.npz"
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"wrote {out} ({os.path.getsize(out)} bytes), sources {data['source_hash']}")
    if failed:
        raise SystemExit("fixture REFUSED: a case misses the branch it is there for, its integer outputs are not reproducible, or a "
                         "constant of this file disagrees with what the recording build does")


if __name__ == "__main__":
    main()
