"""BatchedDoubleLoop(..., past_midnight="coupled") on the CPU (HighsTensorLP backend): the tensor form - the executable specification -
against the oracle's row builders with the late hours' S scenarios tied through lp.row (tests/_past_midnight_oracle.py), the non-vacuity
of the tie on this project's data, the host Bidder / SelfScheduler at a late hour, the default left alone, and results / reset / solves."""
import functools

import numpy as np
import pytest
import torch

from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
from tests._highs_solver import HighsTensorLP
from tests._past_midnight_oracle import oracle_walk, reference_curve

MODES = {"monotone": dict(scenario_coupling="monotone"), "self_schedule": dict(bidder="self_schedule")}


def _loop(flowsheet, B, mode, **kw):
    args = dict(n_price_scenarios=3, forecaster="backcast", max_historical_days=3, market="price_taker", day_ahead_horizon=24,
                lp_backend=HighsTensorLP, past_midnight="coupled")
    args.update(MODES[mode])
    args.update(kw)
    if args["past_midnight"] is None:
        del args["past_midnight"]
    return BatchedDoubleLoop(flowsheet, B, **args)


SHAPES = [("monotone", "wind_battery", 3, 3, 2), ("monotone", "nuclear", 2, 3, 2), ("monotone", "wind_pem", 2, 2, 2),
          ("self_schedule", "wind_battery", 2, 3, 1), ("self_schedule", "nuclear", 2, 3, 1)]


@functools.lru_cache(maxsize=None)
def _walk(mode, flowsheet, B, S, days):
    """one teacher-forced walk per shape, shared by the tests below (read only)"""
    loop = _loop(flowsheet, B, mode, n_price_scenarios=S)
    return loop, oracle_walk(loop, days, tol=1e-9)


@pytest.mark.parametrize("mode,flowsheet,B,S,days", SHAPES)
def test_oracle_walk(mode, flowsheet, B, S, days):
    """Every LP of the walk to 1e-9 relative (the bound of the project's CPU walks): the coupled day-ahead LP, the hourly LPs whose horizon
    stays inside the day (one per row, as the modes' own walks), in the last T_rt - 1 hours ONE LP per plant - S copies of the oracle's
    late-hour bidding rows tied through lp.row over all T_rt periods -, every tracking LP.  Curves, counts and dispatches rebuilt
    exactly: in the late hours block i's P_T[t] with scenario i's real-time forecast, the plant's one status for its S pairs (a
    self-schedule: the one pair (block 0's P_T[t], 0))."""
    loop, seen = _walk(mode, flowsheet, B, S, days)
    T, per = loop.rt.T, 1 if mode == "self_schedule" else S
    assert loop.past_midnight == "coupled" and loop.rtc.c.shape == (B, S * loop.rt.lp.n) and loop.rt_block.c.shape == (B * S, loop.rt.lp.n)
    pairs = S - 1 if mode == "self_schedule" else S * (S - 1) // 2
    assert loop.rtc.lp.m == S * loop.rt.lp.m + pairs * T and loop.rtc.first_coupling_row == S * loop.rt.lp.m
    assert seen["all_optimal"] and seen["worst"] <= 1e-9
    early, late = 24 - (T - 1), T - 1
    assert seen["lps"] == B * days * (1 + early * per + late + 24) and len(seen["late"]) == B * days * late
    assert seen["curves"] == B * days * (24 + 24 * loop.tr.T)
    assert all(not s.any() for s in seen["late_status"])
    res, ok = loop.results()
    assert ok and int(loop.uncertified) == 0
    assert loop.solves == seen["solves"] == days * (B + early * (B * per + B) + late * (B + B))


# every flowsheet in both modes.  Wind + PEM with the walk's S = 2 meets no binding late hour in two days of plants 0 and 1 (margins
# <= 2e-13); with S = 3 plant 0 binds at hours 22 and 23 of day 0 in both modes, so that is the shape here (its walk is checked too).
BINDING = [s for s in SHAPES if s[1] != "wind_pem"] + [("monotone", "wind_pem", 1, 3, 1), ("self_schedule", "wind_pem", 1, 3, 1)]


@pytest.mark.parametrize("mode,flowsheet,B,S,days", BINDING)
def test_the_coupling_binds(mode, flowsheet, B, S, days):
    """Non-vacuity, asserted: in at least one late plant-hour of every shape the coupled optimum is strictly worse than the sum of the S
    independent optima - by more than 1e-7 relative, a hundred times the 1e-9 to which both are solved - and the independent solutions
    of that very hour break the mode's coupling rows by more than 1e-6 MW (the order of the real-time prices; a schedule: they differ
    past midnight).  A restriction never improves an optimum, and the loop's coupled solutions satisfy the rows to 1e-6 MW everywhere."""
    _, seen = _walk(mode, flowsheet, B, S, days)
    late = seen["late"]
    assert min(e[3] for e in late) >= -1e-9, min(e[3] for e in late)
    bound = [e for e in late if e[3] > 1e-7]
    assert bound, sorted(e[3] for e in late)[-3:]
    assert all(e[4] > 1e-6 for e in bound), bound
    assert max(e[5] for e in late) <= 1e-6, max(e[5] for e in late)


def _host(cls, loop, hour, **kw):
    """the host bidder `cls` of plant 0 of a wind + battery loop standing at `hour` of day 0: a Backcaster fed the D days before the
    plant's window, a model object whose capacity factors start at that hour"""
    from dispatches_amd.workflow import Backcaster
    from tests.test_self_schedule_loop_cpu import _DirectHighs
    mo = loop.bidder.bidding_model_object
    N, start, D = loop.N, int(loop.start[0]), loop.D
    hist = (start + 24 * (0 - D) + np.arange(24 * D)) % N
    bus = mo.model_data.bus
    cf = np.roll(loop.cf_series.numpy(), -(start + hour))
    host_model = mo.__class__(model_data=mo.model_data, wind_capacity_factors=list(cf), wind_pmax_mw=200.0, battery_pmax_mw=25.0,
                              battery_energy_capacity_mwh=100.0)
    return cls(bidding_model_object=host_model, day_ahead_horizon=24, real_time_horizon=loop.rt.T, n_scenario=loop.S, solver=_DirectHighs(),
               forecaster=Backcaster({bus: loop.da_series.numpy()[hist].tolist()}, {bus: loop.rt_series.numpy()[hist].tolist()},
                                     max_historical_days=D), **kw)


def _at_hour(loop, hour):
    """the loop after the day-ahead step of day 0, moved to `hour` of that day on its initial state (what the host side is given too)"""
    loop.day_ahead()
    loop.hour_t.fill_(hour)
    loop.hour = hour
    assert not loop.state.any()


HOST_HOUR = 22


def test_against_the_host_bidder():
    """Hour 22 of day 0, one wind + battery plant: workflow/bidder.py::Bidder(scenario_coupling="monotone").compute_real_time_bids on the
    same scenario prices, cleared dispatch and state; HiGHS gets the same coupled LP on both sides: the coupled objective to 1e-9 and
    the bid pairs of every tracked period equal in integer cents."""
    from dispatches_amd.workflow import Bidder
    loop = _loop("wind_battery", 1, "monotone")
    _at_hour(loop, HOST_HOUR)
    host = _host(Bidder, loop, HOST_HOUR, scenario_coupling="monotone")
    host.compute_real_time_bids(date="2020-01-01", hour=HOST_HOUR, realized_day_ahead_prices=loop.da_prices[0].tolist(),
                                realized_day_ahead_dispatches=loop.da_offer[0].tolist())
    loop.hour_step()
    model = host.real_time_model
    got, want = float(loop.rtc.out["obj"][0] + loop.rtc.c0[0]), model.coupled_objective
    assert want is not None and abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)
    counts, U, M = host._scenario_points(model, np.asarray(model.rt_prices), "Real-time")
    curve, count = loop.rt_curve[0].numpy(), loop.rt_count[0].numpy()
    for t in range(loop.tr.T):
        n = int(counts[t])
        want_U, want_M = reference_curve(U[t, :n], M[t, :n], [True] * n, loop.p_min_cents)
        c = int(count[t])
        assert (curve[t, :c, 0].tolist(), curve[t, :c, 1].tolist()) == (want_U, want_M), (t, curve[t].tolist(), want_U, want_M)


def test_against_the_host_self_scheduler():
    """the same hour against workflow/bidder.py::SelfScheduler.compute_real_time_bids: the coupled objective to 1e-9, and the one pair
    of every tracked period - the host's p_max, at cost 0 - equal in integer cents"""
    from dispatches_amd.workflow import SelfScheduler
    loop = _loop("wind_battery", 1, "self_schedule")
    _at_hour(loop, HOST_HOUR)
    host = _host(SelfScheduler, loop, HOST_HOUR)
    bids = host.compute_real_time_bids(date="2020-01-01", hour=HOST_HOUR, realized_day_ahead_prices=loop.da_prices[0].tolist(),
                                       realized_day_ahead_dispatches=loop.da_offer[0].tolist())
    loop.hour_step()
    got, want = float(loop.rtc.out["obj"][0] + loop.rtc.c0[0]), host.real_time_model.coupled_objective
    assert want is not None and abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)
    curve, count = loop.rt_curve[0].numpy(), loop.rt_count[0].numpy()
    for t in range(loop.tr.T):
        want_U, want_M = reference_curve([bids[HOST_HOUR + t][host.generator]["p_max"]], [0.0], [True], loop.p_min_cents)
        c = int(count[t])
        assert (curve[t, :c, 0].tolist(), curve[t, :c, 1].tolist()) == (want_U, want_M), (t, curve[t].tolist(), want_U, want_M)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_default_untouched(mode):
    """past_midnight="free" and the argument left out: the same tensors after two days, and no attribute the loop did not have"""
    given, left_out = _loop("wind_battery", 2, mode, past_midnight="free"), _loop("wind_battery", 2, mode, past_midnight=None)
    for loop in (given, left_out):
        loop.run_day()
        loop.run_day()
    assert set(vars(given)) == set(vars(left_out)) and not {"past_midnight", "rtc", "rt_block"} & set(vars(given))
    assert given.past_midnight == left_out.past_midnight == "free" and given.solves == left_out.solves
    for name in ("revenue", "energy_mwh", "state", "da_offer", "da_prices", "da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch",
                 "delivered", "da_energy_mwh", "offered_mwh", "hour_t"):
        assert torch.equal(getattr(given, name), getattr(left_out, name)), name
    for m in ("da", "rt", "tr"):
        for key in ("x", "obj", "status"):
            assert torch.equal(getattr(given, m).out[key], getattr(left_out, m).out[key]), (m, key)
    tied = _loop("wind_battery", 2, mode)
    assert {"past_midnight", "rtc", "rt_block"} <= set(vars(tied)) and tied.past_midnight == "coupled"


def test_refusals():
    base = dict(n_price_scenarios=3, forecaster="backcast", max_historical_days=3, market="price_taker", day_ahead_horizon=24,
                lp_backend=HighsTensorLP)
    with pytest.raises(ValueError, match="past_midnight is 'free' or 'coupled', not 'tied'"):
        BatchedDoubleLoop("nuclear", 1, past_midnight="tied", **base)
    with pytest.raises(ValueError, match="past_midnight is 'free' or 'coupled', not None"):
        BatchedDoubleLoop("nuclear", 1, past_midnight=None, scenario_coupling="monotone", **base)
    for kw in (dict(), dict(bidder="parametrized", bid_price=10.0, storage_mw=5.0, n_price_scenarios=1, forecaster="perfect")):
        with pytest.raises(ValueError, match="past_midnight='coupled' ties the real-time look-ahead hours of a bidder that couples its price "
                                             "scenarios: bidder='self_schedule' or scenario_coupling='monotone'"):
            BatchedDoubleLoop("wind_pem", 1, past_midnight="coupled", **{**base, **kw})
    # the modes' own refusals come first, word for word
    with pytest.raises(ValueError, match="ruc_hour belongs to scenario_coupling='independent'"):
        BatchedDoubleLoop("nuclear", 1, past_midnight="coupled", scenario_coupling="monotone", ruc_hour=16, **base)
    with pytest.raises(ValueError, match="wind_mw: per-plant sizes belong to bidder='lp'"):
        BatchedDoubleLoop("wind_pem", 1, past_midnight="coupled", bidder="self_schedule", wind_mw=100.0, **base)


@pytest.mark.parametrize("mode,flowsheet", [("monotone", "wind_pem"), ("self_schedule", "nuclear")])
def test_results_reset_solves(mode, flowsheet):
    """health, ledger, record and profiles ride along: bool(bad) == (health_fail.sum() > 0), B real_time solves per late hour, the
    recorder's late-hour rows hold the coupled solve's blocks, and reset() brings the same day back bit for bit"""
    B, S = 2, 3
    loop = _loop(flowsheet, B, mode, health=True, ledger=True, record=([0, 1], 1), profiles=1)
    per, T = 1 if mode == "self_schedule" else S, loop.rt.T
    early, late = 24 - (T - 1), T - 1
    kinds = loop.health_kinds
    loop.day_ahead()
    for k in range(24):
        before = loop.health_solves[kinds.index("real_time")].clone()
        loop.hour_step()
        assert (loop.health_solves[kinds.index("real_time")] - before == (1 if k >= early else per)).all(), k
        if k >= early:                                 # the recorder reads the real-time batch's buffers: the coupled solve's blocks
            assert torch.equal(loop.rt.out["x"].reshape(B, per, -1), loop.rtc.out["x"].reshape(B, S, -1)[:, :per])
    res, ok = loop.results()
    assert ok == (int(loop.health_fail.sum()) == 0) and bool(loop.bad) == (int(loop.health_fail.sum()) > 0)
    assert loop.health_solves[kinds.index("real_time")].tolist() == [early * per + late] * B
    assert loop.health_solves[kinds.index("tracking")].tolist() == [24] * B
    assert loop.solves == B + early * (B * per + B) + late * 2 * B
    assert int(loop.uncertified) == int(loop.health_waived.sum())
    rec = loop.recorded()
    assert rec["rt_x"].shape[:3] == (24, B, per) and not rec["rt_status"].any()
    np.testing.assert_array_equal(rec["rt_x"][23], loop.rtc.out["x"].reshape(B, S, -1)[:, :per].numpy())
    first = {k: v.clone() for k, v in res.items()}
    profile = loop.profile.clone()
    loop.reset()
    assert loop.solves == 0 and not loop.health_solves.any() and not loop.revenue.any()
    loop.run_day()
    again, _ = loop.results()
    for k, v in first.items():
        assert torch.equal(v, again[k]), k
    assert torch.equal(profile, loop.profile)
