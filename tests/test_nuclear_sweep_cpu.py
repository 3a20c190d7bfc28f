"""Per-plant operands of the nuclear double loop (BatchedDoubleLoop("nuclear", pem_mw=, tank_kg=, h2_price=, h2_demand=);
sweeps.nuclear_sweep) on the CPU backend of the tests (HiGHS per LP): a mixed batch walked against the oracle's LPs at every plant's own
operands, the default plant inside it against the unsized loop, offers below 400 MW, the ledger at the plant's own hydrogen price, the
refusals, all-None = the loop without the arguments, and the sweep's layout and cells."""
import numpy as np
import pytest

from dispatches_amd.flowsheets import parameters as prm

STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast", max_historical_days=10, market="price_taker")
MIXED = dict(pem_mw=[100.0, 200.0, 50.0, 150.0], tank_kg=[5000.0, 8000.0, 2000.0, 5000.0], h2_price=[4.0, 2.0, 1.0, 0.75],
             h2_demand=[0.35, 0.5, 0.2, 0.35], plant_windows=np.array([3, 3, 3, 4]))       # plant 0 is the default plant


def _loop(B, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from tests._highs_solver import HighsTensorLP
    return BatchedDoubleLoop("nuclear", B, lp_backend=HighsTensorLP, **kw)


@pytest.mark.parametrize("mode", [STOCHASTIC, {}], ids=["stochastic", "deterministic"])
def test_every_lp_of_a_mixed_nuclear_batch(mode, monkeypatch):
    """B = 4 plants with distinct (pem_mw, tank_kg, h2_price, h2_demand), one of them the default plant, two days: every day-ahead,
    in-day real-time and tracking LP against the oracle at that plant's operands and recorded state (1e-6 relative), curves
    and dispatches exact with that plant's p_min; the default plant walks like the unsized loop's plant on the same window (curves
    and dispatches in integer cents, objectives at 1e-9); the 200 MW PEM offers below 400 MW in some hour; the ledger books the
    hydrogen at each plant's own price."""
    from tests._nuclear_size_oracle import nuclear_walk
    loop = _loop(4, ledger=True, **MIXED, **mode)
    assert loop.nuclear_sized and not loop.sized and loop.p_min_cents_plant.tolist() == [40000, 30000, 45000, 35000]
    # the static bounds and objective entries, row b * S + i of the bidding models and row b of the tracker
    for m, per in ((loop.da, loop.S), (loop.rt, loop.S), (loop.tr, 1)):
        rows = lambda a: np.repeat(np.asarray(a), per)[:, None]
        assert len(m.pem_cols) == m.T and len(m.out_cols) == m.T and len(m.hold_cols) == m.T - 1
        assert (m.ub[:, m.pem_cols].numpy() == rows(MIXED["pem_mw"]) * 1e3).all()
        assert (m.ub[:, m.hold_cols].numpy() == rows(MIXED["tank_kg"]) / prm.mw_h2).all()
        assert (m.ub[:, m.out_cols].numpy() == rows(MIXED["h2_demand"]) / prm.mw_h2).all()
    seen = nuclear_walk(loop, 2, monkeypatch)
    res, ok = loop.results()
    print("mixed nuclear batch, worst relative objective gap:", seen["worst"], "over", seen["lps"], "LPs,", seen["curves"], "curves")
    S, Trt = loop.S, loop.rt.T
    assert ok and seen["all_optimal"] and seen["worst"] <= 1e-6
    assert seen["lps"] == 2 * 4 * (S + (24 - Trt + 1) * S + 24)
    for m, per in ((loop.da, S), (loop.rt, S), (loop.tr, 1)):                # no step has rewritten the static entries
        want = -np.repeat([prm.mw_h2 * 3600 * p for p in MIXED["h2_price"]], per)[:, None]
        assert (m.c[:, m.out_cols].numpy() == want).all() and (m.ub[:, m.pem_cols].numpy() == np.repeat(MIXED["pem_mw"], per)[:, None] * 1e3).all()
    # the ledger at every plant's own price
    assert np.allclose(res["h2_revenue"].numpy(), res["h2_kg"].numpy() * np.array(MIXED["h2_price"]), rtol=1e-12)
    assert res["pem_mwh"].numpy()[1] > 100.0 * 48 * 0.5 and (res["pem_mwh"].numpy() <= np.array(MIXED["pem_mw"]) * 48 + 1e-6).all()
    # the default plant of the mixed batch against the unsized loop's plant on the same window
    plain = _loop(1, ledger=True, plant_windows=np.array([3]), **mode)
    alone = nuclear_walk(plain, 2, monkeypatch)
    assert len(alone["trace"][0]) == len(seen["trace"][0])
    for got, want in zip(seen["trace"][0], alone["trace"][0]):
        if got[0] == "curve":
            assert got == want
        else:
            assert got[:2] == want[:2] and abs(got[2] - want[2]) <= 1e-9 * max(1.0, abs(want[2])), (got, want)
    if loop.stochastic:
        assert seen["curves"] == 2 * 4 * (24 + 24 * loop.tr.T)
        assert seen["lowest_offer_mw"][1] == 300.0 and seen["lowest_offer_mw"][0] == 400.0     # a 200 MW PEM offers below 400 MW
        assert loop.da_offer.numpy()[1].min() < 400.0                          # ... and is cleared there


def test_all_none_is_the_loop_without_the_arguments():
    """pem_mw = tank_kg = h2_price = h2_demand = None equals the loop without them bit for bit after a day; so does the default plant's
    operands passed explicitly in everything but the mode flag"""
    a = _loop(2, **STOCHASTIC)
    b = _loop(2, pem_mw=None, tank_kg=None, h2_price=None, h2_demand=None, **STOCHASTIC)
    c = _loop(2, pem_mw=100.0, tank_kg=prm.tank_capacity_kg, h2_price=[4.0, 4.0], h2_demand=0.35, **STOCHASTIC)
    assert not a.nuclear_sized and not b.nuclear_sized and c.nuclear_sized and b.p_min_cents_plant is None
    for loop in (a, b, c):
        loop.run_day()
    for other in (b, c):
        for m, mm in ((a.da, other.da), (a.rt, other.rt), (a.tr, other.tr)):
            for key in ("c", "c0", "lb", "ub", "rlo", "rhi"):
                assert np.array_equal(getattr(m, key).numpy(), getattr(mm, key).numpy()), key
        for key in ("da_offer", "da_prices", "da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch", "state", "energy_mwh"):
            assert np.array_equal(getattr(a, key).numpy(), getattr(other, key).numpy()), key
    assert np.array_equal(a.revenue.numpy(), b.revenue.numpy())
    np.testing.assert_allclose(c.revenue.numpy(), a.revenue.numpy(), rtol=1e-12, atol=1e-9)     # (the sized tensor form adds it in the kernels' fused arithmetic)


def test_refusals():
    ok = dict(pem_mw=[50.0, 200.0], tank_kg=[1000.0, 5000.0], h2_price=[1.0, 2.0], h2_demand=[0.2, 0.35])
    assert _loop(2, **ok, **STOCHASTIC).nuclear_sized and _loop(2, pem_mw=500.0, ruc_hour=16, **STOCHASTIC).nuclear_sized
    for kw, text in ((dict(ok, pem_mw=[50.0, 100.0, 200.0]), "length 2"), (dict(ok, tank_kg=np.ones((2, 1))), "length 2"),
                     (dict(ok, h2_price=[1.0, np.nan]), "finite"), (dict(ok, h2_demand=[np.inf, 0.1]), "finite"), (dict(ok, tank_kg=-np.inf), "finite"),
                     (dict(ok, pem_mw=[0.0, 100.0]), "> 0"), (dict(ok, pem_mw=-5.0), "> 0"), (dict(ok, pem_mw=[100.0, 500.5]), "at most"),
                     (dict(ok, tank_kg=[-1.0, 5.0]), ">= 0"), (dict(ok, h2_price=-0.5), ">= 0"), (dict(ok, h2_demand=[0.1, -0.1]), ">= 0")):
        with pytest.raises(ValueError, match=text):
            _loop(2, **kw, **STOCHASTIC)
    with pytest.raises(ValueError, match="bidder='lp'"):
        _loop(2, pem_mw=150.0, bidder="self_schedule", **STOCHASTIC)
    with pytest.raises(ValueError, match="independent"):
        _loop(2, h2_price=2.0, scenario_coupling="monotone", **STOCHASTIC)
    with pytest.raises(ValueError):
        _loop(2, pem_mw=150.0, bidder="parametrized", bid_price=10.0, storage_mw=10.0)
    for name in ("wind_mw", "battery_mw", "battery_mwh"):                       # the wind and battery sizes stay refused for nuclear
        with pytest.raises(ValueError, match="nuclear"):
            _loop(2, pem_mw=150.0, **{name: 10.0}, **STOCHASTIC)
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from tests._highs_solver import HighsTensorLP
    with pytest.raises(ValueError, match="nuclear"):
        BatchedDoubleLoop("wind_pem", 2, lp_backend=HighsTensorLP, pem_mw=100.0, **STOCHASTIC)


def test_plant_curves_take_a_minimum_per_lane():
    """workflow/market.py::plant_curves with a per-lane minimum equals lane-by-lane calls with that lane's scalar"""
    import torch
    from dispatches_amd.workflow.market import plant_curves
    rng = np.random.default_rng(3)
    power, price = torch.as_tensor(rng.uniform(250.0, 500.0, (3, 8))), torch.as_tensor(rng.uniform(0.0, 40.0, (3, 8)))
    power[0, 2] = 300.0                                                      # a pair AT the lane's minimum: no point is inserted
    ok = torch.ones(3, 8, dtype=torch.bool)
    p_min = torch.as_tensor([40000, 30000, 30000, 45000, 0, 35000, 50000, 26000])
    U, M, count = plant_curves(torch, power, price, ok, p_min_cents=p_min)
    for lane in range(8):
        u, m, c = plant_curves(torch, power[:, lane:lane + 1], price[:, lane:lane + 1], ok[:, lane:lane + 1], p_min_cents=int(p_min[lane]))
        assert torch.equal(U[:, lane], u[:, 0]) and torch.equal(M[:, lane], m[:, 0]) and int(count[lane]) == int(c[0])
    assert int(U[0, 2]) == 30000 and int(U[0, 6]) == 50000 and int(count[6]) == 1


def test_nuclear_sweep_layout_and_cells():
    """a 2 x 2 x 2 grid, one day: shapes, the layout (plant (i, j, w)), and each cell equal to the same plant run in a loop of its own to 1e-9"""
    from dispatches_amd.sweeps import nuclear_layout, nuclear_sweep
    from tests._highs_solver import HighsTensorLP
    prices, pems, W = [0.75, 2.0], [50.0, 250.0], 2
    price, pem, win = nuclear_layout(prices, pems, W)
    for i in range(2):
        for j in range(2):
            for w in range(2):
                at = (i * 2 + j) * 2 + w
                assert (price[at], pem[at], win[at]) == (prices[i], pems[j], w)
    with pytest.raises(ValueError):
        nuclear_layout([], [1.0], 1)
    out = nuclear_sweep(prices, pems, W, 1, lp_backend=HighsTensorLP)
    keys = ["revenue", "h2_revenue", "tot_cost", "profit", "energy_mwh", "h2_kg", "pem_capacity_factor"]
    assert sorted(out) == sorted(keys + ["all_optimal"]) and out["all_optimal"] and all(out[k].shape == (2, 2, 2) for k in keys)
    assert np.array_equal(out["profit"], out["revenue"] - out["tot_cost"])
    assert (out["pem_capacity_factor"] > 0).all() and (out["pem_capacity_factor"] <= 1.0 + 1e-9).all()
    assert (out["energy_mwh"][:, 1] < out["energy_mwh"][:, 0]).all()          # the larger PEM takes more of the plant's power
    for i, j, w in ((0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        own = _loop(1, ledger=True, h2_price=prices[i], pem_mw=pems[j], plant_windows=np.array([w]), **STOCHASTIC)
        own.run_day()
        res, ok = own.results()
        assert ok
        for name, key in (("revenue", "obj"), ("h2_revenue", "h2_revenue"), ("tot_cost", "tot_cost"), ("profit", "profit"), ("energy_mwh", "energy_mwh"),
                          ("h2_kg", "h2_kg")):
            np.testing.assert_allclose(out[name][i, j, w], float(res[key][0]), rtol=1e-9, atol=1e-9, err_msg=f"{name} ({i}, {j}, {w})")
        np.testing.assert_allclose(out["pem_capacity_factor"][i, j, w], float(res["pem_mwh"][0]) / (pems[j] * 24), rtol=1e-9)
