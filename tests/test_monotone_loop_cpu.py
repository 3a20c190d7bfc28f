"""BatchedDoubleLoop(..., bidder="lp", scenario_coupling="monotone") on the CPU (HighsTensorLP backend): the tensor form - the executable
specification of the mode - against the oracle's row builders with the ordered-pair rows stated once more (tests/_monotone_oracle.py),
the non-vacuity of the coupling on this project's data, the order of the solutions, the host Bidder on the same coupled LP, and the
mode's edges: refusals, the default left alone, results, reset."""
import functools

import numpy as np
import pytest

from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
from tests._highs_solver import HighsTensorLP
from tests._monotone_oracle import independent_violations, oracle_walk, reference_curve


def _loop(flowsheet, B, **kw):
    args = dict(scenario_coupling="monotone", n_price_scenarios=3, forecaster="backcast", max_historical_days=3, market="price_taker",
                day_ahead_horizon=24, lp_backend=HighsTensorLP)
    args.update(kw)
    return BatchedDoubleLoop(flowsheet, B, **args)


SHAPES = [("wind_battery", 3, 3, 24, 2), ("nuclear", 2, 3, 24, 2), ("wind_pem", 2, 2, 24, 1), ("wind_battery", 1, 3, 48, 1)]


@functools.lru_cache(maxsize=None)
def _walk(flowsheet, B, S, horizon, days):
    """one teacher-forced walk per shape, shared by the tests below (read only)"""
    loop = _loop(flowsheet, B, n_price_scenarios=S, day_ahead_horizon=horizon)
    return loop, oracle_walk(loop, days, tol=1e-9)


@pytest.mark.parametrize("flowsheet,B,S,horizon,days", SHAPES)
def test_oracle_walk(flowsheet, B, S, horizon, days):
    """Every coupled day-ahead LP against the oracle's LP of the same backcast scenarios (S copies of the flowsheet's bidding LP, every
    pair j < k of every period ordered by its day-ahead prices through lp.row), every hourly LP against the oracle's *_rt of its
    scenario (past midnight: free day_ahead_power on that scenario's forecast, untied - the loop's own choice, pinned here), every
    tracking LP against *_track, to 1e-9 relative (the bound of the project's CPU walks); curves, counts and dispatches rebuilt exactly
    from the read-back solutions: S pairs per plant-hour from the S blocks of the plant's ONE row, the p_min point in front."""
    loop, seen = _walk(flowsheet, B, S, horizon, days)
    assert loop.monotone and loop.da.c.shape == (B, S * loop.da.n1) and loop.rt.c.shape[0] == B * S
    assert loop.da.lp.m == S * loop.da_block.lp.m + S * (S - 1) // 2 * horizon
    assert seen["all_optimal"] and seen["worst"] <= 1e-9
    assert seen["lps"] == B * days * (1 + 24 * S + 24) and seen["past_midnight"] == B * days * S * (loop.rt.T - 1)
    assert seen["curves"] == B * days * (24 + 24 * loop.tr.T)
    assert seen["first_powers"] == {40000 if flowsheet == "nuclear" else 0} and seen["max_points"] >= S
    res, ok = loop.results()
    assert ok and int(loop.uncertified) == 0 and loop.solves == days * (B + 24 * (B * S + B))


@pytest.mark.parametrize("flowsheet,B,S,horizon,days", SHAPES[:3])
def test_the_coupling_binds(flowsheet, B, S, horizon, days):
    """Non-vacuity, asserted: on day 0 at least one plant of every flowsheet has a coupled optimum more than 1e-4 (relative) above the
    sum of its S independent optima (measured here: 1e-3 .. 2e-2); the same plant's independent solutions - the oracle's, and the
    loop's own under scenario_coupling="independent" - break the order in at least one (pair, period) by more than 1e-6 MW $; and the
    walk has met all three cases of a row: lower side, upper side, free (equal prices)."""
    _, seen = _walk(flowsheet, B, S, horizon, days)
    margins = seen["coupling_margin"]
    assert len(margins) == B and max(margins) > 1e-4, margins
    assert min(margins) >= -1e-9, margins                                 # a restriction never improves the optimum
    bound = [b for b in range(B) if margins[b] > 1e-4]
    assert all(seen["independent_violations"][b][0] >= 1 for b in bound), seen["independent_violations"]
    free = _loop(flowsheet, B, n_price_scenarios=S, scenario_coupling="independent")
    free.day_ahead()
    got = independent_violations(free)
    assert all(got[b][0] >= 1 and got[b][1] < -1e-6 for b in bound), got
    assert all(c > 0 for c in seen["cases"]) and sum(seen["cases"]) == B * days * S * (S - 1) // 2 * horizon, seen["cases"]


@pytest.mark.parametrize("flowsheet,B,S,horizon,days", SHAPES)
def test_monotone_by_construction(flowsheet, B, S, horizon, days):
    """with the coupling the pairs of every plant-hour sorted by price have non-decreasing power to 1e-6 MW, so the stored curve is the
    curve without the running maximum to within one cent of power: no price is lifted across more than a cent"""
    _, seen = _walk(flowsheet, B, S, horizon, days)
    assert seen["disorder"] <= 1e-6, seen["disorder"]
    assert seen["repaired"] == 0


def test_against_the_host_bidder():
    """One wind + battery plant against workflow/bidder.py::Bidder(scenario_coupling="monotone") on a Backcaster fed the same D days of
    the plant's window; HiGHS gets the same coupled LP on both sides (called the same way): the coupled objective to 1e-9 and the 24
    day-ahead curves equal in integer cents."""
    from dispatches_amd.workflow import Backcaster, Bidder
    from tests.test_self_schedule_loop_cpu import _DirectHighs
    S = D = 3
    loop = _loop("wind_battery", 1)
    mo = loop.bidder.bidding_model_object
    N, start = loop.N, int(loop.start[0])
    roll = lambda t: np.roll(t.numpy(), -start)
    hist = (start + 24 * (0 - D) + np.arange(24 * D)) % N
    bus = mo.model_data.bus
    host_model = mo.__class__(model_data=mo.model_data, wind_capacity_factors=list(roll(loop.cf_series)), wind_pmax_mw=200.0,
                              battery_pmax_mw=25.0, battery_energy_capacity_mwh=100.0)
    host = Bidder(bidding_model_object=host_model, day_ahead_horizon=24, real_time_horizon=loop.rt.T, n_scenario=S, solver=_DirectHighs(),
                  forecaster=Backcaster({bus: loop.da_series.numpy()[hist].tolist()}, {bus: loop.rt_series.numpy()[hist].tolist()},
                                        max_historical_days=D), scenario_coupling="monotone")
    host.compute_day_ahead_bids(date="2020-01-01", hour=0)
    loop.day_ahead()
    got = float(loop.da.out["obj"][0] + loop.da.c0[0])
    model = host.day_ahead_model
    want = model.coupled_objective
    assert want is not None and abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)
    counts, U, M = host._scenario_points(model, np.asarray(model.da_prices), "Day-ahead")
    curve, count = loop.da_curve[0].numpy(), loop.da_count[0].numpy()
    for t in range(24):
        n = int(counts[t])
        want_U, want_M = reference_curve(U[t, :n], M[t, :n], [True] * n, loop.p_min_cents)
        c = int(count[t])
        assert (curve[t, :c, 0].tolist(), curve[t, :c, 1].tolist()) == (want_U, want_M), (t, curve[t].tolist(), want_U, want_M)
    assert (count >= 2).any()                                             # (plant 0, day 0: curves of one and two points)


@pytest.mark.parametrize("kw,match", [
    (dict(scenario_coupling="ordered"), "scenario_coupling is 'independent' or 'monotone'"), (dict(scenario_coupling=None), "scenario_coupling is"),
    (dict(bidder="self_schedule"), "scenario_coupling='monotone' belongs to bidder='lp'"),
    (dict(bidder="parametrized", bid_price=20.0, storage_mw=5.0), "scenario_coupling='monotone' belongs to bidder='lp'"),
    (dict(ruc_hour=16), "ruc_hour belongs to scenario_coupling='independent'"),
    (dict(wind_mw=150.0), "wind_mw: per-plant sizes belong to scenario_coupling='independent'"),
    (dict(battery_mw=10.0), "battery_mw: per-plant sizes belong to scenario_coupling='independent'"),
    (dict(battery_mwh=50.0), "battery_mwh: per-plant sizes belong to scenario_coupling='independent'"),
    (dict(bid_price=20.0), "belong to bidder='parametrized'"), (dict(storage_mw=10.0), "belong to bidder='parametrized'"),
    (dict(forecaster="perfect", n_price_scenarios=1), "forecaster='backcast'"), (dict(forecaster="perfect"), "knows one price scenario"),
    (dict(n_price_scenarios=1), "needs n_price_scenarios >= 2"), (dict(n_price_scenarios=4), "n_price_scenarios <= min"),
    (dict(n_price_scenarios=0), "n_price_scenarios <= min"), (dict(max_historical_days=400), "whole days inside the series"),
    (dict(day_ahead_horizon=12), "day-ahead horizon of 24 .. 48"), (dict(market="pool"), "market 'stub' or 'price_taker'")])
def test_refusals(kw, match):
    """every refusal by ITS message, next to the construction it differs from in one argument (which must succeed: the mode exists)"""
    assert _loop("wind_battery", 2).monotone
    with pytest.raises(ValueError, match=match):
        _loop("wind_battery", 2, **kw)


def _state_of(loop):
    res, ok = loop.results()
    out = {k: v.numpy().copy() for k, v in res.items()}
    for name, m in (("da", loop.da), ("rt", loop.rt), ("tr", loop.tr)):
        for key in ("c", "lb", "ub", "rlo", "rhi", "c0"):
            out[name + "_" + key] = getattr(m, key).numpy().copy()
    for key in ("da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch", "da_offer", "da_prices", "delivered"):
        out[key] = getattr(loop, key).numpy().copy()
    return out, ok


def test_independent_is_the_default_loop():
    """scenario_coupling="independent" is the loop without the keyword, bit for bit after one day: same models, same LPs, same curves"""
    runs = []
    for kw in (dict(), dict(scenario_coupling="independent")):
        loop = BatchedDoubleLoop("nuclear", 2, n_price_scenarios=3, forecaster="backcast", max_historical_days=3, market="price_taker",
                                 day_ahead_horizon=24, lp_backend=HighsTensorLP, **kw)
        assert not loop.monotone and not loop.coupled_da and loop.da.c.shape[0] == 6 and not hasattr(loop, "da_block")
        loop.run_day()
        state, ok = _state_of(loop)
        assert ok and loop.solves == 6 + 24 * 8
        runs.append(state)
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


def test_results_and_reset():
    loop = _loop("nuclear", 2)
    stochastic = _loop("nuclear", 2, scenario_coupling="independent")
    assert set(loop.results()[0]) == set(stochastic.results()[0]) == {"obj", "energy_mwh", "state", "da_energy_mwh", "offered_mwh"}
    loop.day_ahead()
    for _ in range(3):
        loop.hour_step()
    res, ok = loop.results()
    first = {k: v.clone() for k, v in res.items()}
    offer, curve = loop.da_offer.clone(), loop.da_curve.clone()
    assert ok and loop.hour == 3 and int(loop.hour_t) == 3 and loop.solves == 2 + 3 * 8 and float(res["offered_mwh"].sum()) > 0.0
    loop.reset()
    res, ok = loop.results()
    assert ok and loop.hour == 0 and int(loop.hour_t) == 0 and loop.solves == 0 and all(not v.any() for v in res.values())
    loop.day_ahead()
    for _ in range(3):
        loop.hour_step()
    res, ok = loop.results()
    assert ok and all((res[k] == first[k]).all() for k in first) and (loop.da_offer == offer).all() and (loop.da_curve == curve).all()
