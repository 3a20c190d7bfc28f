"""The stochastic mode of the descriptor loop (dispatches_amd/rolling_flowsheets.py::BatchedDoubleLoop: n_price_scenarios / forecaster /
market) on the CPU backend of the tests (HiGHS per LP): argument validation, backcast windows against a host Backcaster, the nuclear
and wind + PEM loops walked against the oracle's own LPs with curves that start at the generator's p_min, the wind + battery loop
against rolling.py's own stochastic mode, plant_curves with a minimum power, and the deterministic defaults untouched."""
import numpy as np
import pytest

FLOWSHEETS = ("wind_battery", "wind_pem", "nuclear")
STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast", max_historical_days=10, market="price_taker")


def _loop(flowsheet, B, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from tests._highs_solver import HighsTensorLP
    return BatchedDoubleLoop(flowsheet, B, lp_backend=HighsTensorLP, **kw)


@pytest.mark.parametrize("flowsheet", FLOWSHEETS)
def test_arguments_are_validated_at_construction(flowsheet):
    for kw in (dict(forecaster="backcast", n_price_scenarios=0), dict(forecaster="backcast", n_price_scenarios=17, max_historical_days=20),
               dict(forecaster="backcast", n_price_scenarios=4, max_historical_days=3), dict(forecaster="perfect", n_price_scenarios=2),
               dict(forecaster="oracle"), dict(market="auction"), dict(forecaster="backcast", max_historical_days=400),
               dict(forecaster="backcast", tracking_horizon=13), dict(market="price_taker", day_ahead_horizon=72)):
        with pytest.raises(ValueError):
            _loop(flowsheet, 2, **kw)
    loop = _loop(flowsheet, 2, **STOCHASTIC)
    assert (loop.S, loop.D, loop.stochastic) == (3, 10, True) and loop.da.c.shape[0] == loop.rt.c.shape[0] == 6 and loop.tr.c.shape[0] == 2
    assert loop.p_min_cents == (40000 if flowsheet == "nuclear" else 0)
    assert loop.da_curve.shape == (2, 24, 4, 2) and loop.rt_curve.shape == (2, loop.tr.T, 4, 2) and loop.rt_dispatch.shape == (2, loop.tr.T)


@pytest.mark.parametrize("flowsheet", FLOWSHEETS)
@pytest.mark.parametrize("S,D", [(1, 1), (3, 10), (16, 16)])
def test_backcast_windows_are_the_host_backcasters(flowsheet, S, D):
    """the loop's gathered windows equal - exactly - what a host Backcaster built from the D days before the simulated day returns:
    days 0 .. D + 1, starts next to the end of the series, horizons 48 / 12 / 4"""
    from tests._stochastic_oracle import host_backcast
    probe = _loop(flowsheet, 1)
    N, stride = probe.N, probe.stride
    # the first plant whose year starts inside the last day of the series; its neighbours wrap to the front
    first = next(k for k in range(N) if N - 24 < (stride * k) % N < N - 1)
    B = 4
    loop = _loop(flowsheet, B, first_scenario=first, n_price_scenarios=S, forecaster="backcast", max_historical_days=D, market="price_taker")
    start = loop.start.numpy()
    assert start.max() > N - 24 and (start == (stride * (first + np.arange(B))) % N).all()
    for series in (loop.da_series, loop.rt_series):
        host = series.numpy()
        for day in range(0, D + 2):
            for hour, T in ((0, 48), (0, 12), (0, 4), (13, 12), (13, 4), (23, 4), (22, 48)):
                loop.hour_t.fill_(24 * day + hour)
                got = loop._forecast(series, T, hour).numpy()
                assert got.shape == (B, S, T)
                for b in range(B):
                    assert np.array_equal(got[b], host_backcast(host, int(start[b]), day, hour, T, S, D)), (b, day, hour, T)


@pytest.mark.parametrize("flowsheet", ["nuclear", "wind_pem"])
def test_every_lp_curve_and_dispatch_of_the_stochastic_loop(flowsheet):
    """B = 5, S = 3, D = 10, price taker, two days: every day-ahead row, every real-time row of the hours whose horizon lies inside the
    cleared day and every tracking LP against the oracle's LP of that scenario's prices, the plant's state and the cleared dispatch
    (1e-6 relative); curves and dispatches recomputed from the read-back solutions exactly; revenue re-added (1e-9).  Not vacuous: the
    forecast is wrong on most hours, the market clears below the last point and at it; the nuclear curves start at 400 MW and some
    have three or more points.  (The nuclear tracker may miss a dispatch at the inserted p_min point - not reachable from every tank
    state - so delivered == dispatch is NOT asserted; that is the reference's curve rule.)"""
    from tests._flowsheet_stochastic_oracle import oracle_walk
    B, S, days = 5, 3, 2
    loop = _loop(flowsheet, B, first_scenario=0, **STOCHASTIC)
    seen = oracle_walk(loop, days)
    res, ok = loop.results()
    assert ok and seen["all_optimal"]
    assert loop.solves == days * (B * S + 24 * (B * S + B))
    Trt = loop.rt.T
    assert seen["lps"] == days * (B * S + (24 - Trt + 1) * B * S + 24 * B) and seen["curves"] == days * B * (24 + 24 * loop.tr.T)
    assert seen["worst"] <= 1e-6
    assert seen["forecast_differs"] > 0.5 * seen["forecast_hours"], seen
    assert seen["below"] >= 1 and seen["equal"] >= 1, seen
    if flowsheet == "nuclear":
        assert seen["three"] >= 1 and seen["first_powers"] == {40000}, seen
    else:
        assert seen["first_powers"] == {0}, seen
    assert sorted(res) == ["da_energy_mwh", "energy_mwh", "obj", "offered_mwh", "state"]
    assert (res["da_energy_mwh"] <= res["offered_mwh"]).all()


def test_wind_battery_is_rolling_pys_stochastic_loop():
    """BatchedDoubleLoop("wind_battery") in stochastic mode against BatchedWindBatteryDoubleLoop with the same arguments: the same
    curves, counts, dispatches and states exactly, revenue to 1e-12 over two days"""
    from dispatches_amd.rolling import BatchedWindBatteryDoubleLoop
    from tests._highs_solver import HighsTensorLP
    B = 5
    a = BatchedWindBatteryDoubleLoop(B, stride=17, warm_start=False, lp_backend=HighsTensorLP, **STOCHASTIC)
    g = _loop("wind_battery", B, **STOCHASTIC)
    differs = total = below = equal = three = 0
    for day in range(2):
        for step in range(25):
            if step == 0:
                fa, real = a._forecast(a.da_series, 24, 0).numpy(), a._window(a.da_series, 24).numpy()
                differs, total = differs + int((fa != real[:, None, :]).sum()), total + fa.size
                assert np.array_equal(a.day_ahead().numpy(), g.day_ahead().numpy())
                pairs = (("da_curve", "da_offer"),)
            else:
                a.hour_step(), g.hour_step()
                pairs = (("rt_curve", "rt_dispatch"),)
            for curve, disp in pairs:
                count = curve.replace("curve", "count")
                for name in (curve, count, disp, "da_prices"):
                    assert np.array_equal(getattr(a, name).numpy(), getattr(g, name).numpy()), (day, step, name)
                cnt = getattr(g, count).numpy().astype(np.int64)
                last = np.take_along_axis(getattr(g, curve).numpy()[..., 0], (cnt - 1)[..., None], -1)[..., 0] / 100.0
                d = getattr(g, disp).numpy()
                below, equal, three = below + int((d < last).sum()), equal + int((d == last).sum()), three + int((cnt >= 3).sum())
            assert np.array_equal(a.soc.numpy(), g.state.numpy()[:, 0]) and np.array_equal(a.thr.numpy(), g.state.numpy()[:, 1]), (day, step)
            for x, y in (((a.da, g.da),) if step == 0 else ((a.rt, g.rt), (a.tr, g.tr))):        # the models this step wrote
                assert np.allclose(x.c0.numpy(), y.c0.numpy(), rtol=1e-13) and np.allclose(x.c.numpy(), y.c.numpy(), rtol=1e-13, atol=1e-15)
        a._warm = g._warm = True
    assert differs > 0.5 * total and below >= 1 and equal >= 1 and three >= 1, (differs, total, below, equal, three)
    ra, oka = a.results()
    rg, okg = g.results()
    assert oka and okg and a.solves == g.solves
    np.testing.assert_allclose(rg["obj"].numpy(), ra["obj"].numpy(), rtol=1e-12)
    np.testing.assert_allclose(rg["energy_mwh"].numpy(), ra["energy_mwh"].numpy(), rtol=1e-12)
    for key in ("da_energy_mwh", "offered_mwh"):
        assert np.array_equal(rg[key].numpy(), ra[key].numpy()), key


def _host_bidder_curve(power, price, ok, p_min_cents):
    """one lane through the host Bidder path: bid_curves.sorted_pairs + bid_curves.curves with p_min -> (U cents, M cents)"""
    import torch
    from dispatches_amd.workflow import bid_curves as bc
    p_min = p_min_cents / 100.0
    ps, cs, first = bc.sorted_pairs(torch, torch.as_tensor(np.asarray(power, float)).reshape(-1, 1),
                                    torch.as_tensor(np.asarray(price, float)).reshape(-1, 1), p_min, ok=torch.as_tensor(np.asarray(ok, bool)))
    f = first[:, 0].numpy()
    pts = [(ps[:, 0].numpy()[f] / 100.0, cs[:, 0].numpy()[f] / 100.0)]
    counts, Up, Mp = bc.padded(pts, width=len(power))
    n, Uc, cost = bc.curves(counts, Up, Mp, p_min, round(p_min, 2))
    n = int(n[0])
    U = [int(round(u * 100)) for u in Uc[0, :n]]
    # the host path integrates: cost_0 = U_0 M_0, cost_j = cost_{j-1} + (U_j - U_{j-1}) M_j  ->  the marginal prices back out of it
    return U, Uc[0, :n], cost[0, :n]


@pytest.mark.parametrize("p_min_cents", [0, 1, 40000])
@pytest.mark.parametrize("S", [1, 3, 16])
def test_plant_curves_with_a_minimum_power(S, p_min_cents):
    import torch
    from dispatches_amd.workflow import market
    from tests._flowsheet_stochastic_oracle import reference_curve
    from tests.test_market_cpu import adversarial_pairs
    rng = np.random.default_rng(700 + S)
    L = 300
    power, price = adversarial_pairs(rng, S, L)
    # second half of the lanes: the same pairs moved next to 400 MW, so that the minimum of 40000 cents cuts through them
    power[:, L // 2:] = np.round(power[:, L // 2:] + 399.9 - 100.0 * (rng.random((S, L - L // 2)) < 0.3), 3)
    power[rng.random((S, L)) < 0.1] = 400.0
    power[rng.random((S, L)) < 0.05] = 0.01
    ok = rng.random((S, L)) > 0.1
    ok[:, :3] = False
    T = lambda a: torch.as_tensor(a)
    U, M, count = (v.numpy() for v in market.plant_curves(torch, T(power), T(price), T(ok), p_min_cents=p_min_cents))
    if p_min_cents == 0:
        for got, was in zip((U, M, count), market.plant_curves(torch, T(power), T(price), T(ok))):
            assert np.array_equal(got, was.numpy())
    dropped = inserted = 0
    for l in range(L):
        u, m = reference_curve(power[:, l], price[:, l], ok[:, l], p_min_cents)
        assert (U[:count[l], l].tolist(), M[:count[l], l].tolist()) == (u, m), l
        assert not U[count[l]:, l].any() and not M[count[l]:, l].any() and u[0] == p_min_cents
        hu, hp, hcost = _host_bidder_curve(power[:, l], price[:, l], ok[:, l], p_min_cents)
        want = np.empty(len(u))
        uu, mm = np.array(u) / 100.0, np.array(m) / 100.0
        want[0] = uu[0] * mm[0]
        if len(u) > 1:
            want[1:] = want[0] + np.cumsum(np.diff(uu) * mm[1:])
        assert hu == u and np.array_equal(hp, uu) and np.array_equal(hcost, want), l
        live = ok[:, l]
        dropped += int((np.round(power[live, l] * 100) < p_min_cents - 1).sum())
        inserted += not any(abs(p * 100 - p_min_cents) < 0.4 for p in power[live, l])
    assert inserted >= 1 and (p_min_cents == 0 or dropped >= 1)


@pytest.mark.parametrize("flowsheet", FLOWSHEETS)
def test_explicit_defaults_are_the_default_constructor(flowsheet):
    """n_price_scenarios=1, forecaster="perfect", market="stub" given explicitly: the identical tensors as the default constructor"""
    runs = []
    for kw in ({}, dict(n_price_scenarios=1, forecaster="perfect", market="stub", max_historical_days=10)):
        loop = _loop(flowsheet, 3, **kw)
        if kw:
            assert not loop.stochastic and loop.S == 1
        loop.run_day()
        res, ok = loop.results()
        assert ok and sorted(res) == ["energy_mwh", "obj", "state"]
        out = {k: v.numpy().copy() for k, v in res.items()}
        for name, m in (("da", loop.da), ("rt", loop.rt), ("tr", loop.tr)):
            for key in ("c", "lb", "ub", "rlo", "rhi"):
                out[name + key] = getattr(m, key).numpy().copy()
            out[name + "x"] = m.out["x"].numpy().copy()
        out["da_offer"] = loop.da_offer.numpy().copy()
        runs.append(out)
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("flowsheet", FLOWSHEETS)
def test_stub_market_clears_the_last_point_and_perfect_price_taker_runs(flowsheet):
    loop = _loop(flowsheet, 2, first_scenario=40, n_price_scenarios=2, forecaster="backcast", max_historical_days=4, market="stub")
    last = lambda curve, count: np.take_along_axis(curve.numpy()[..., 0], (count.numpy().astype(np.int64) - 1)[..., None], -1)[..., 0] / 100.0
    loop.day_ahead()
    assert np.array_equal(loop.da_offer.numpy(), last(loop.da_curve, loop.da_count))
    for _ in range(24):
        loop.hour_step()
        assert np.array_equal(loop.rt_dispatch.numpy(), last(loop.rt_curve, loop.rt_count))
    assert loop.results()[1]
    loop = _loop(flowsheet, 2, first_scenario=40, n_price_scenarios=1, forecaster="perfect", market="price_taker")
    assert loop.stochastic
    loop.run_day()
    res, ok = loop.results()
    assert ok and (res["da_energy_mwh"] <= res["offered_mwh"]).all()
