"""BatchedDoubleLoop(..., ruc_hour=H) on the CPU backend of the tests (HiGHS per LP): the day-ahead bid of day d + 1 made at hour H of
day d on a state projected to midnight (dispatches_amd/rolling_flowsheets.py, "bidding at the RUC hour").  The chain and the bid walked
against the oracle's own LPs (tests/_projection_oracle.py), the chain against the host DoubleLoopCoordinator's projection tracker, day 0
and the stateless wind + PEM loop bit for bit against the default loop, non-vacuity, refusals, reset, the sweep front end, and the C
entry point's refusals without a GPU."""
import ctypes as C

import numpy as np
import pytest

STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast", max_historical_days=10, market="price_taker")
MODES = {"deterministic": {}, "backcast": STOCHASTIC}


def _loop(flowsheet, B, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from tests._highs_solver import HighsTensorLP
    return BatchedDoubleLoop(flowsheet, B, lp_backend=HighsTensorLP, **kw)


def _chain_lps(B, H, days):
    return days * B * (24 - H)


@pytest.mark.parametrize("flowsheet", ["wind_battery", "nuclear"])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("H", [16, 21, 23])
def test_chain_and_bid_against_the_oracle(flowsheet, mode, H):
    """B = 3, two days: every projection LP rebuilt from the oracle's rows with tracking rows on the periods inside the day only
    (objective, constant included, to 1e-9 relative - both sides are HiGHS on the same LP), the rounding of the hand-off exactly,
    every day-ahead LP of the pending bid on the projected state / the windows at 24 (d + 1) / the bid's backcast rule, curves and
    dispatches exactly, and the pending bid: invisible until midnight, current after it.  H = 21, 23: every window reaches past
    midnight (tracking horizon 4)."""
    from tests._projection_oracle import ruc_walk
    B, days = 3, 2
    loop = _loop(flowsheet, B, ruc_hour=H, **MODES[mode])
    seen = ruc_walk(loop, days)
    S = loop.S
    assert loop.results()[1] and seen["all_optimal"]
    assert seen["lps"] == _chain_lps(B, H, days) + days * B * S and seen["worst"] <= 1e-9, seen
    assert seen["projected_moves"], seen
    Ttr = loop.tr.T
    per_chain = sum(min(Ttr, 24 - H - j) < Ttr for j in range(24 - H))
    assert seen["midnight_windows"] == days * B * per_chain and per_chain == (24 - H if H >= 21 else Ttr - 1)
    if mode == "backcast":
        assert seen["rt_lag_differs"] > 0 and seen["curves"] == days * B * 24
    # the first day bids at hour 0, every day at hour H: chain solves + one bid per day on top of the default loop's
    assert loop.solves == days * 24 * (B * S + B) + B * S + days * (B * (24 - H) + B * S)


@pytest.mark.parametrize("flowsheet", ["wind_battery", "nuclear"])
def test_longest_chain(flowsheet):
    """H = 1: 23 chained LPs per day"""
    from tests._projection_oracle import ruc_walk
    loop = _loop(flowsheet, 3, ruc_hour=1)
    seen = ruc_walk(loop, 2)
    assert seen["all_optimal"] and seen["worst"] <= 1e-9 and seen["lps"] == _chain_lps(3, 1, 2) + 2 * 3 and seen["projected_moves"], seen
    assert loop.proj_state.shape[0] == 24


class _RecordingHighs:
    """TEST-ONLY host solver that hands HiGHS the LP exactly as tests/_highs_solver.py::HighsTensorLP does (oracle/highs_direct.py),
    and keeps the objective of every solve"""

    def __init__(self):
        self.objectives = []

    def solve(self, model, tee=False):
        from dispatches_amd.workflow.batch_model import SolveResults
        from oracle.highs_direct import HighsModel
        lb, ub, rlo, rhi = (np.asarray(a, np.float64).reshape(-1) for a in model.scenario_bounds())
        x, f, y = HighsModel(np.asarray(model.c, np.float64).reshape(-1), model.lp.csr(), rlo, rhi, lb, ub).solve()
        obj = f + float(np.asarray(model.c0).reshape(-1)[0])
        self.objectives.append(obj)
        model.store_solution(x[None, :], y[None, :], np.array([obj]), np.zeros(1, np.int32))
        return SolveResults("ok", "optimal")


@pytest.mark.parametrize("flowsheet", ["wind_battery", "nuclear"])
@pytest.mark.parametrize("H", [16, 22])
def test_chain_is_the_host_coordinators_projection(flowsheet, H):
    """For every plant: the project's DoubleLoopCoordinator with a Tracker and a projection Tracker on one model object, the tracker put
    at the loop's realised state and clock of hour H, current_DA_dispatches = the loop's da_offer, _project_tracking_trajectory(...,
    ruc_hour=H).  Both sides hand HiGHS the same LP: the per-step objectives agree to 1e-9, the projected state is exactly equal."""
    from dispatches_amd.workflow import DoubleLoopCoordinator, Tracker
    B = 3
    loop = _loop(flowsheet, B, ruc_hour=H)
    loop.day_ahead()
    for _ in range(H):
        loop.hour_step()
    state_at = loop.state.numpy().copy()
    loop.hour_step()
    offer, start, N = loop.da_offer.numpy(), loop.start.numpy(), loop.N
    ps, po = loop.proj_state.numpy(), loop.proj_obj.numpy()
    assert np.array_equal(ps[0], state_at)
    template = loop.tracker_template.tracking_model_object
    moved = 0
    for b in range(B):
        if flowsheet == "wind_battery":
            cf = np.roll(loop.cf_series.numpy(), -int(start[b]))
            obj = template.__class__(model_data=template.model_data, wind_capacity_factors=list(cf), wind_pmax_mw=template._wind_pmax_mw,
                                     battery_pmax_mw=template._battery_pmax_mw, battery_energy_capacity_mwh=template._battery_energy_capacity_mwh)
            at = lambda s: dict(realized_soc=[float(s[0])], realized_energy_throughput=[float(s[1])])
            last = lambda p: [round(p["realized_soc"][-1], 2), round(p["realized_energy_throughput"][-1], 2)]
        else:
            obj = template.__class__(template.model_data)
            at = lambda s: dict(implemented_tank_holdup=[float(s[0])])
            last = lambda p: [round(p["implemented_tank_holdup"][-1])]
        solver = _RecordingHighs()
        tracker = Tracker(tracking_model_object=obj, tracking_horizon=loop.tr.T, n_tracking_hour=1, solver=solver)
        projection = Tracker(tracking_model_object=obj, tracking_horizon=loop.tr.T, n_tracking_hour=1, solver=solver)
        for tr, state in ((tracker, state_at[b]), (projection, np.zeros_like(state_at[b]))):      # the clone must bring the STATE over
            if hasattr(tr.model.block, "_time_idx"):
                tr.model.block._time_idx = H - 1
            tr.update_model(**at(state))
        coordinator = DoubleLoopCoordinator(bidder=None, tracker=tracker, projection_tracker=projection)
        coordinator.current_DA_dispatches = [float(v) for v in offer[b]]
        profiles = coordinator._project_tracking_trajectory(None, None, H)
        assert len(solver.objectives) == 24 - H
        np.testing.assert_allclose(po[:, b], solver.objectives, rtol=1e-9, atol=1e-9, err_msg=f"plant {b}")
        assert ps[-1, b].tolist() == last(profiles), (b, ps[-1, b], last(profiles))
        moved += not np.array_equal(ps[-1, b], ps[0, b])
    assert moved >= 1


@pytest.mark.parametrize("flowsheet", ["wind_battery", "wind_pem", "nuclear"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_day_0_is_the_default_loops(flowsheet, mode):
    """the first day bids at hour 0 from the initial state (the coordinator's is_first_day): state, revenue, energy and delivered power
    after its 24 hours are the default loop's bit for bit, and so are the day's offers and prices"""
    a, b = _loop(flowsheet, 3, ruc_hour=16, **MODES[mode]), _loop(flowsheet, 3, **MODES[mode])
    a.run_day(), b.run_day()
    for name in ("state", "revenue", "energy_mwh", "delivered", "da_offer", "da_prices"):
        assert np.array_equal(getattr(a, name).numpy(), getattr(b, name).numpy()), name
    ra, rb = a.results()[0], b.results()[0]
    assert sorted(ra) == sorted(rb)
    for key in ra:
        assert np.array_equal(ra[key].numpy(), rb[key].numpy()), key


@pytest.mark.parametrize("market", ["stub", "price_taker"])
def test_wind_pem_on_a_perfect_forecast_is_invariant(market):
    """no state, the same windows, the solves in the same order: three days of results() bit for bit the default loop's"""
    a, b = _loop("wind_pem", 3, ruc_hour=16, market=market), _loop("wind_pem", 3, market=market)
    for _ in range(3):
        a.run_day(), b.run_day()
    (ra, oka), (rb, okb) = a.results(), b.results()
    assert oka and okb and sorted(ra) == sorted(rb)
    for key in ra:
        assert np.array_equal(ra[key].numpy(), rb[key].numpy()), key
    assert np.array_equal(a.da_offer.numpy(), b.da_offer.numpy()) and a.proj_state.shape == (9, 3, 0)


@pytest.mark.parametrize("flowsheet", ["wind_battery", "nuclear"])
def test_the_mode_changes_the_bid(flowsheet):
    """not vacuous (B = 4, H = 16): the projection moves the state of at least one plant, day 1's day-ahead offers differ from the default
    loop's for at least one plant, and the bid's real-time scenarios are not the lag-0 ones"""
    a, b = _loop(flowsheet, 4, ruc_hour=16, **STOCHASTIC), _loop(flowsheet, 4, **STOCHASTIC)
    a.run_day(), b.run_day()
    assert (a.proj_state[-1] != a.proj_state[0]).any(1).sum().item() >= 1
    assert np.array_equal(a.bid_hour_t.numpy(), np.array(24))
    a._clk = a.bid_hour_t
    lag1, lag0 = a._forecast(a.rt_series, a.da.T, 0, lag_days=1).numpy(), a._forecast(a.rt_series, a.da.T, 0).numpy()
    a._clk = a.hour_t
    # scenario i of the bid is scenario i + 1 of a bid made at midnight (first day of the horizon: the second wraps inside the history)
    assert (lag1 != lag0).any() and np.array_equal(lag1[:, :-1, :24], lag0[:, 1:, :24])
    oa, ob = a.day_ahead().numpy(), b.day_ahead().numpy()
    assert (oa != ob).any(1).sum() >= 1
    d = _loop(flowsheet, 4, ruc_hour=16)
    e = _loop(flowsheet, 4)
    d.run_day(), e.run_day()
    assert (d.proj_state[-1] != d.proj_state[0]).any(1).sum().item() >= (3 if flowsheet == "nuclear" else 4)
    assert (d.day_ahead().numpy() != e.day_ahead().numpy()).any(1).sum() >= 1


def test_the_wind_battery_projection_fills_the_battery():
    """the property of the rule, recorded and not asserted away: rows past midnight are free, the last windows of the chain sell nothing
    they are not asked for, and the projected day ends on a (nearly) full battery whatever the realised state was"""
    loop = _loop("wind_battery", 4, ruc_hour=16)
    loop.run_day()
    soc = loop.proj_state[-1, :, 0].numpy()
    assert (soc > 99_900.0).all() and (soc <= 100_000.0).all(), soc
    assert (loop.state[:, 0].numpy() < soc).any()


def test_refusals():
    for bad in (0, 24, -1, 16.0, "16", True, 1.5):
        with pytest.raises(ValueError):
            _loop("nuclear", 2, ruc_hour=bad)
    with pytest.raises(ValueError):
        _loop("wind_pem", 2, ruc_hour=16, bidder="parametrized", bid_price=15.0, storage_mw=20.0)
    N = _loop("nuclear", 1).N
    D = N // 24                                                            # 24 D <= N < 24 (D + 1): the default loop takes it, the bid's lag does not
    if D <= 400:
        kw = dict(n_price_scenarios=3, forecaster="backcast", max_historical_days=D, market="price_taker")
        _loop("nuclear", 1, **kw)
        with pytest.raises(ValueError):
            _loop("nuclear", 1, ruc_hour=16, **kw)
    loop = _loop("nuclear", 2, ruc_hour=np.int64(7))
    assert loop.ruc_hour == 7 and isinstance(loop.ruc_hour, int) and loop.proj_state.shape == (18, 2, 1)
    assert _loop("nuclear", 2).ruc_hour is None and not hasattr(_loop("nuclear", 2), "pj")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_reset_clears_the_pending_bid_the_trace_and_the_bid_clock(mode):
    loop = _loop("wind_battery", 2, ruc_hour=20, **MODES[mode])
    loop.run_day()
    first = {n: getattr(loop, n).numpy().copy() for n in ("proj_state", "proj_real", "proj_obj", "pend_offer", "pend_prices", "state", "revenue")}
    assert loop._pending and first["proj_obj"].any() and first["pend_offer"].any() and loop.bid_hour_t.item() == 24
    loop.reset()
    names = ("proj_state", "proj_real", "proj_obj", "pend_offer", "pend_prices", "bid_hour_t") + (("pend_curve", "pend_count") if loop.stochastic else ())
    assert not loop._pending and all(not getattr(loop, n).any() for n in names) and loop.hour == loop.solves == 0
    loop.run_day()                                                         # day 0 again: it bids at hour 0, and repeats itself
    for n, was in first.items():
        assert np.array_equal(getattr(loop, n).numpy(), was), n


def test_design_sweep_passes_ruc_hour_through():
    from dispatches_amd import sweeps
    from tests._highs_solver import HighsTensorLP
    grid = ([150.0, 200.0], [15.0, 25.0], [4.0], 2)
    out = sweeps.design_sweep("wind_battery", *grid, n_days=2, lp_backend=HighsTensorLP, ruc_hour=16, **STOCHASTIC)
    wind, batt, mwh, win = sweeps.design_layout(*grid)
    loop = _loop("wind_battery", len(wind), ruc_hour=16, wind_mw=wind, battery_mw=batt, battery_mwh=mwh, plant_windows=win, **STOCHASTIC)
    loop.run_day(), loop.run_day()
    res, ok = loop.results()
    assert ok and out["all_optimal"] and np.array_equal(out["revenue"].ravel(), res["obj"].numpy())
    assert np.array_equal(out["da_energy_mwh"].ravel(), res["da_energy_mwh"].numpy())
    plain = sweeps.design_sweep("wind_battery", *grid, n_days=2, lp_backend=HighsTensorLP, **STOCHASTIC)
    assert (plain["revenue"] != out["revenue"]).any()
    # the sized projection tracker carries each plant's own battery: its projected state of charge ends below that plant's capacity
    assert (loop.proj_state[-1, :, 0].numpy() <= mwh * 1e3).all() and (loop.proj_state[-1, :, 0].numpy() > 0.9 * mwh * 1e3).all()


# ---- the C entry point refuses bad descriptors on the host: nothing is launched, so this runs without a GPU ---------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dispatches_amd import hip_solver
    return hip_solver.load_library()


def _descriptors():
    """a well-formed (state, model) pair on fake non-NULL pointers: every refusal below is found before anything is dereferenced"""
    from dispatches_amd.hip_solver import DspLoopModel, DspLoopProjectState
    p = 0x1000
    st = DspLoopProjectState()
    st.B, st.N, st.ruc_hour, st.slots = 4, 8784, 16, 4
    for name, _ in DspLoopProjectState._fields_:
        if name not in ("B", "N", "ruc_hour", "slots", "state_scale"):
            setattr(st, name, p)
    st.state_scale[0] = st.state_scale[1] = 100.0
    m = DspLoopModel()
    for name in ("c", "lb", "ub", "rlo", "rhi", "base_c", "x", "c0", "status", "flags"):
        setattr(m, name, p)
    m.n, m.m, m.T, m.n_state = 40, 30, 4, 2
    for t in range(16):
        m.track_rows[t], m.wind_cols[t] = (t, 10 + t) if t < 4 else (-1, -1)
        m.pt_cols[t][0] = m.pt_cols[t][1] = m.pda_cols[t] = -1
    m.state_init[0], m.state_init[1], m.state_real[0], m.state_real[1] = 0, 1, 2, 3
    return st, m


def test_dsp_loop_project_refuses_bad_descriptors_without_a_gpu(lib):
    call = lambda st, m, phase, j: lib.dsp_loop_project(C.byref(st) if st is not None else None, C.byref(m) if m is not None else None, phase, j, None)
    st, m = _descriptors()
    assert call(None, m, 0, 0) == -1 and call(st, None, 0, 0) == -1 and call(st, None, 1, 0) == -1
    for phase, j in ((-1, 0), (3, 0), (0, -1), (0, 8), (1, 8), (2, 1)):
        assert call(st, m, phase, j) == -1, (phase, j)

    def broken(phases, **fields):
        for phase in phases:
            st, m = _descriptors()
            for name, value in fields.items():
                target, field = (st, name[3:]) if name.startswith("st_") else (m, name)
                if isinstance(value, tuple):
                    getattr(target, field)[value[0]] = value[1]
                else:
                    setattr(target, field, value)
            assert call(st, m, phase, 0) == -1, (phase, fields)

    for fields in (dict(st_B=0), dict(st_N=0), dict(st_ruc_hour=0), dict(st_ruc_hour=24)):
        broken((0, 1, 2), **fields)
    for fields in (dict(T=0), dict(T=17), dict(n=0), dict(m=0), dict(n_state=3), dict(n_state=-1), dict(st_start=None), dict(st_hour=None),
                   dict(st_proj_state=None), dict(st_state=None), dict(wind_kw_plant=0x1000), dict(c0_base_plant=0x1000)):
        broken((0, 1), **fields)
    for fields in (dict(st_da_offer=None), dict(lb=None), dict(ub=None), dict(rlo=None), dict(rhi=None), dict(c0=None), dict(st_cf_series=None),
                   dict(track_rows=(3, 30)), dict(track_rows=(0, -1)), dict(wind_cols=(3, 40)), dict(wind_cols=(1, -1)),
                   dict(state_init=(1, 40)), dict(state_init=(0, -1))):
        broken((0,), **fields)
    for fields in (dict(x=None), dict(status=None), dict(c0=None), dict(st_obj=None), dict(st_proj_real=None), dict(st_proj_obj=None),
                   dict(state_real=(1, 40)), dict(state_real=(0, -2)), dict(st_state_scale=(0, 0.0))):
        broken((1,), **fields)
    for fields in (dict(st_da_offer=None), dict(st_da_prices=None), dict(st_pend_offer=None), dict(st_pend_prices=None), dict(st_slots=-1),
                   dict(st_slots=18), dict(st_da_curve=None), dict(st_da_count=None), dict(st_pend_curve=None), dict(st_pend_count=None)):
        broken((2,), **fields)
