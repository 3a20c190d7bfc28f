"""The per-plant solve health of the device double loop (BatchedDoubleLoop(health=True)) on the CPU backend of the tests (HiGHS per LP),
B = 5, two simulated days: solver outcomes INJECTED through a wrapper around the stand-in backend - a listed set of (kind, plant, row,
hour) gets another status, flag or iteration count - must show up in the seven counters exactly as the list implies, in every mode of
the loop; the two invariants against the global flags `bad` / `uncertified` hold after every hour; without injections the counters say
"all valid" and count the mode's solves; health=True changes no other number; the sweeps pass the new outputs on; and the C ABI's new
struct and symbol are what the header says, under an unchanged DSP_VERSION."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, DAYS = 5, 2
KINDS = ("day_ahead", "real_time", "tracking", "projection")
STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast", max_historical_days=10, market="price_taker")
SIZED = dict(wind_mw=[50.0, 200.0, 400.0, 100.0, 300.0], battery_mw=[5.0, 25.0, 100.0, 10.0, 50.0], battery_mwh=[20.0, 100.0, 200.0, 40.0, 100.0],
             plant_windows=np.array([1, 1, 2, 0, 3]))


class Injected:
    """the stand-in backend with rewritten outcomes: lp_backend=Injected(plan) builds one wrapped HighsTensorLP per model; attach(loop)
    names each model's kind.  plan: a list of dicts with kind, plant, row (of the plant's R rows), hour (the device clock of the solve),
    nth (which solve of that kind within the hour: the projection chain has several), and any of status, flag, iters."""

    def __init__(self, plan=()):
        self.plan, self.loop, self.applied = list(plan), None, 0

    def __call__(self, lp):
        from tests._highs_solver import HighsTensorLP
        return _InjectedLP(self, HighsTensorLP(lp))

    def attach(self, loop):
        self.loop = loop
        for kind, m in (("day_ahead", loop.da), ("real_time", loop.rt), ("tracking", loop.tr), ("projection", getattr(loop, "pj", None))):
            if m is not None and m.dlp is not None:
                m.dlp.kind = kind


class _InjectedLP:
    def __init__(self, owner, inner):
        self.owner, self.inner, self.kind, self.calls = owner, inner, None, {}

    def solve(self, rows, *args, **kw):
        import torch
        out = self.inner.solve(rows, *args, **kw)
        out["flags"] = torch.zeros(rows, dtype=torch.int32)              # (the stand-in has none: the wrapper supplies what a device solve reports)
        loop = self.owner.loop
        hour = int(loop.hour_t)
        nth = self.calls[hour] = self.calls.get(hour, -1) + 1
        per = rows // loop.B
        for e in self.owner.plan:
            if e["kind"] == self.kind and e["hour"] == hour and e.get("nth", 0) == nth:
                at = e["plant"] * per + e["row"]
                assert e["row"] < per
                for key, name in (("status", "status"), ("flag", "flags"), ("iters", "iters")):
                    if key in e:
                        out[name][at] = e[key]
                self.owner.applied += 1
        return out


def expected(plan, n_plants):
    """the seven counters (but health_solves) that a plan implies, as numpy arrays"""
    fail, mask, waived, imax = (np.zeros((4, n_plants), np.int32) for _ in range(4))
    iters, first = np.zeros((4, n_plants), np.int64), np.zeros(n_plants, np.int64)
    for e in plan:
        k, b, status = KINDS.index(e["kind"]), e["plant"], e.get("status", 0)
        if status != 0:
            fail[k, b] += 1
            mask[k, b] |= 1 << status
            first[b] = e["hour"] + 1 if first[b] == 0 else min(first[b], e["hour"] + 1)
        elif e.get("flag", 0) & 1:
            waived[k, b] += 1
        iters[k, b] += e.get("iters", 0)
        imax[k, b] = max(imax[k, b], e.get("iters", 0))
    return dict(health_fail=fail, health_status=mask, health_waived=waived, health_iters=iters, health_iters_max=imax, health_first=first)


def E(kind, plant, row, hour, **what):
    return dict(kind=kind, plant=plant, row=row, hour=hour, **what)


# mode -> (flowsheet, constructor arguments, rows per plant of (day_ahead, real_time), plan).  Every plan has failures of several statuses,
# a waived row, iteration counts, two entries on one plant (the earlier hour must win) and entries in both days.
MODES = {
    "deterministic": ("nuclear", {}, (1, 1), [
        E("day_ahead", 1, 0, 24, status=1, iters=200000), E("real_time", 1, 0, 7, status=2, iters=5), E("tracking", 3, 0, 30, status=4),
        E("tracking", 0, 0, 2, flag=1, iters=9), E("real_time", 4, 0, 47, iters=11), E("real_time", 4, 0, 46, iters=3)]),
    "stochastic": ("wind_pem", STOCHASTIC, (3, 3), [
        E("day_ahead", 2, 1, 0, status=1, iters=7), E("day_ahead", 2, 2, 24, status=3), E("real_time", 0, 2, 25, status=1, iters=40),
        E("real_time", 0, 0, 25, flag=1, iters=50), E("tracking", 4, 0, 13, status=2), E("real_time", 4, 1, 5, flag=1)]),
    "monotone": ("nuclear", dict(STOCHASTIC, scenario_coupling="monotone"), (1, 3), [
        E("day_ahead", 3, 0, 24, status=1, iters=200000), E("day_ahead", 0, 0, 0, flag=1, iters=12), E("real_time", 3, 2, 30, status=4),
        E("tracking", 1, 0, 47, status=1, iters=2)]),
    "self_schedule": ("wind_pem", dict(STOCHASTIC, n_price_scenarios=2, bidder="self_schedule"), (1, 1), [
        E("day_ahead", 4, 0, 0, status=1, iters=3), E("real_time", 2, 0, 26, status=2), E("tracking", 2, 0, 3, flag=1, iters=8),
        E("real_time", 0, 0, 40, iters=6)]),
    "parametrized": ("wind_battery", dict(bidder="parametrized", bid_price=[15.0, 20.0, 25.0, 30.0, 35.0], storage_mw=[0.0, 10.0, 25.0, 50.0, 100.0],
                                          market="price_taker"), (0, 0), [
        E("tracking", 1, 0, 5, status=1, iters=4), E("tracking", 1, 0, 29, status=3, iters=6), E("tracking", 3, 0, 47, flag=1), E("tracking", 0, 0, 0, iters=2)]),
    "ruc_hour": ("nuclear", dict(STOCHASTIC, ruc_hour=16), (3, 3), [
        E("day_ahead", 2, 1, 16, status=1, iters=99),                    # the PENDING bid, made at hour 16 of day 0 for day 1
        E("projection", 0, 0, 16, nth=3, status=2, iters=5), E("projection", 0, 0, 40, nth=0, status=1), E("projection", 4, 0, 40, nth=7, flag=1, iters=1),
        E("day_ahead", 1, 0, 0, flag=1), E("tracking", 3, 0, 16, status=4)]),
    "sized": ("wind_battery", dict(n_price_scenarios=2, forecaster="backcast", max_historical_days=10, market="price_taker", **SIZED), (2, 2), [
        E("day_ahead", 0, 1, 24, status=1, iters=200000), E("real_time", 3, 0, 11, status=1, iters=17), E("real_time", 3, 1, 11, flag=1, iters=19),
        E("tracking", 2, 0, 33, status=2)]),
}
MUST_HIT = {"monotone": ["day_ahead"], "parametrized": ["tracking"], "ruc_hour": ["projection", "day_ahead"]}


def solve_counts(mode, flowsheet, rows):
    """rows per plant that two days of a mode solve, per kind: the day-ahead solves (ruc_hour: hour 0 of day 0 and the pending bids of
    hour 16 of both days), 24 hourly steps a day, and the 24 - 16 projection steps in front of each pending bid"""
    r_da, r_rt = rows
    if mode == "parametrized":
        return [0, 0, 24 * DAYS, 0]
    if mode == "ruc_hour":
        return [r_da * (1 + DAYS), r_rt * 24 * DAYS, 24 * DAYS, 8 * DAYS]
    return [r_da * DAYS, r_rt * 24 * DAYS, 24 * DAYS, 0]


def run(flowsheet, kw, plan=None, health=True, each_hour=None):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    backend = Injected(plan or ())
    loop = BatchedDoubleLoop(flowsheet, B, lp_backend=backend, **kw, **({"health": True} if health else {}))
    backend.attach(loop)
    for _ in range(DAYS):
        loop.day_ahead()
        for _ in range(24):
            loop.hour_step()
            if each_hour is not None:
                each_hour(loop)
    return loop, backend


def invariants(loop):
    assert bool(loop.bad) == bool(loop.health_fail.sum() > 0)
    assert int(loop.uncertified) == int(loop.health_waived.sum())


def test_health_is_a_new_argument_with_new_results():
    """fails without the feature: the argument, the four results() keys and the seven tensors"""
    loop, _ = run("wind_pem", {})
    assert loop.health_kinds == KINDS
    res, ok = loop.results()
    assert ok and {"valid", "failed_solves", "uncertified_solves", "first_failure_hour"} <= set(res)
    for name, shape, dtype in (("health_solves", (4, B), "int32"), ("health_fail", (4, B), "int32"), ("health_status", (4, B), "int32"),
                               ("health_waived", (4, B), "int32"), ("health_iters", (4, B), "int64"), ("health_iters_max", (4, B), "int32"),
                               ("health_first", (B,), "int64")):
        t = getattr(loop, name)
        assert tuple(t.shape) == shape and str(t.dtype) == "torch." + dtype, name
        assert any(t is z for z in loop._zeroed), name
    assert res["valid"].dtype.is_floating_point is False and str(res["valid"].dtype) == "torch.bool"
    assert str(res["first_failure_hour"].dtype) == "torch.int64"


@pytest.mark.parametrize("mode", list(MODES))
def test_injected_outcomes(mode):
    """all seven tensors equal what the list implies, exactly; both invariants after every hour; first_failure_hour the earliest
    listed hour per plant and -1 elsewhere; health_solves the mode's solve counts; reset() zeroes everything"""
    flowsheet, kw, rows, plan = MODES[mode]
    loop, backend = run(flowsheet, kw, plan, each_hour=invariants)
    assert backend.applied == len(plan), "an entry of the plan met no solve"
    want = expected(plan, B)
    for name, value in want.items():
        assert np.array_equal(getattr(loop, name).numpy(), value), (name, getattr(loop, name).numpy(), value)
    for kind in MUST_HIT.get(mode, []):
        assert want["health_fail"][KINDS.index(kind)].sum() > 0, kind
    if mode == "parametrized":
        assert not loop.health_solves[[0, 1, 3]].numpy().any()
    if mode == "ruc_hour":                             # the pending bid is booked at the hour it is made (16), not at the bid clock (24)
        assert loop.health_first[2] == 17 and want["health_fail"][0, 2] == 1
    counts = solve_counts(mode, flowsheet, rows)
    assert np.array_equal(loop.health_solves.numpy(), np.repeat(np.array(counts, np.int32)[:, None], B, axis=1))
    assert int(loop.health_solves.sum()) == loop.solves
    res, ok = loop.results()
    first = want["health_first"] - 1
    assert not ok and (first >= 0).any() and (first == -1).any()
    assert np.array_equal(res["first_failure_hour"].numpy(), first)
    assert np.array_equal(res["failed_solves"].numpy(), want["health_fail"].sum(0))
    assert np.array_equal(res["uncertified_solves"].numpy(), want["health_waived"].sum(0))
    assert np.array_equal(res["valid"].numpy(), want["health_fail"].sum(0) == 0)
    invariants(loop)
    loop.reset()
    for name in list(want) + ["health_solves"]:
        assert not getattr(loop, name).numpy().any(), name
    assert not bool(loop.bad) and int(loop.uncertified) == 0


@pytest.mark.parametrize("mode", list(MODES))
def test_nothing_injected_and_nothing_else_changes(mode):
    """health=True without injections: all valid, no failure, the mode's solve counts; against health=False every other results() entry
    and the LP buffers of all models are bit-identical, and health=False creates no health_* attribute"""
    flowsheet, kw, rows, _ = MODES[mode]
    on, _ = run(flowsheet, kw, each_hour=invariants)
    off, _ = run(flowsheet, kw, health=False)
    res, ok = on.results()
    assert ok and bool(res["valid"].all()) and not on.health_fail.numpy().any() and not on.health_first.numpy().any()
    assert (res["first_failure_hour"] == -1).all() and not res["failed_solves"].numpy().any()
    assert np.array_equal(on.health_solves.numpy(), np.repeat(np.array(solve_counts(mode, flowsheet, rows), np.int32)[:, None], B, axis=1))
    assert not [name for name in vars(off) if name.startswith("health_")] and not hasattr(off, "valid") and not hasattr(off, "failed_solves")
    ref, ok_off = off.results()
    assert ok_off and set(res) - set(ref) == {"valid", "failed_solves", "uncertified_solves", "first_failure_hour"}
    for key, value in ref.items():
        assert np.array_equal(res[key].numpy(), value.numpy()), key
    for name in ("da", "da_block", "rt", "tr", "pj"):
        a, b = getattr(on, name, None), getattr(off, name, None)
        assert (a is None) == (b is None)
        for buf in ("c", "lb", "ub", "rlo", "rhi", "c0") if a is not None else ():
            assert np.array_equal(getattr(a, buf).numpy(), getattr(b, buf).numpy()), (name, buf)


def test_sweeps_return_the_health_of_every_grid_point():
    """2 x 2 x 1 grids, one day: valid / failed_solves / first_failure_hour in grid shape with health=True, today's keys without"""
    from dispatches_amd import sweeps
    from tests._highs_solver import HighsTensorLP
    new = {"valid", "failed_solves", "first_failure_hour"}
    calls = (
        (sweeps.parametrized_sweep, ("wind_pem", [15.0, 30.0], [0.0, 100.0], 1, 1), {}, (2, 2, 1)),
        (sweeps.design_sweep, ("wind_battery", [100.0, 200.0], [10.0, 25.0], [4.0], 1, 1), {}, (2, 2, 1, 1)),
        (sweeps.nuclear_sweep, ([3.0, 4.0], [100.0, 200.0], 1, 1), dict(n_price_scenarios=2), (2, 2, 1)),
    )
    for fn, args, kw, shape in calls:
        plain = fn(*args, lp_backend=HighsTensorLP, **kw)
        out = fn(*args, lp_backend=HighsTensorLP, health=True, **kw)
        assert not new & set(plain) and set(out) - set(plain) == new, fn.__name__
        for key in new:
            assert out[key].shape == shape, (fn.__name__, key)
        assert out["valid"].dtype == np.bool_ and out["valid"].all() and (out["first_failure_hour"] == -1).all() and not out["failed_solves"].any()
        for key, value in plain.items():
            assert np.array_equal(out[key], value), (fn.__name__, key)


def test_c_abi_declares_and_exports_the_health_entry_point():
    """the header declares the struct and the symbol, the library exports it, the ctypes mirror matches the header field for field (the
    technique of test_capi_cpu.py), and DSP_VERSION is still 22: a new symbol, no changed struct"""
    import __graft_entry__ as g
    g.build()
    from dispatches_amd import hip_solver
    lib = hip_solver.load_library()
    hdr = open(os.path.join(ROOT, "include", "dsp_hip.h")).read()
    assert re.search(r"\bint dsp_loop_health\s*\(const dsp_loop_health_state \*", hdr)
    assert hasattr(lib, "dsp_loop_health") and "dsp_loop_health" in hip_solver.EXPORTED_SYMBOLS
    assert int(re.search(r"#define DSP_VERSION (\d+)", hdr).group(1)) == 22 == hip_solver.ABI_VERSION == lib.dsp_version()
    body = re.search(r"typedef struct dsp_loop_health_state \{(.*?)\} dsp_loop_health_state;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = re.sub(r"\[[0-9\]\[]*\]", "", body)                         # array extents
    fields = [f for decl in body.split(";") for f in re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", decl.strip().split(" ", 1)[-1] if decl.strip() else "")]
    fields = [f for f in fields if f not in ("const", "double", "int32_t", "int64_t")]
    mirror = hip_solver.DspLoopHealthState
    assert fields == [f[0] for f in mirror._fields_], (fields, [f[0] for f in mirror._fields_])
    import ctypes as C
    assert C.sizeof(mirror) == 8 + 8 * 8 + 32                           # two int32, eight pointers, four reserved int64
    assert len(hip_solver.HEALTH_KINDS) == int(re.search(r"#define DSP_HEALTH_KINDS (\d+)", hdr).group(1))
    assert hip_solver.HEALTH_MAX_ROWS == int(re.search(r"#define DSP_HEALTH_MAX_ROWS (\d+)", hdr).group(1))
