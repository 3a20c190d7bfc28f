"""The per-plant ledger of the device double loop (BatchedDoubleLoop(ledger=True)) on the CPU backend of the tests (HiGHS per LP): every
hour's booked values against closed forms written here from NAMED columns of the tracker's solution and flowsheets/parameters.py - not
through the loop's descriptor -, the sums, the profit, the forms that the project's data never makes non-zero pinned on hand-set
solutions, and ledger=True against False in every participation mode."""
import numpy as np
import pytest

from dispatches_amd.flowsheets import parameters as prm

STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast", max_historical_days=10, market="price_taker")
SIZED = dict(wind_mw=[50.0, 200.0, 400.0], battery_mw=[5.0, 25.0, 100.0], battery_mwh=[20.0, 100.0, 200.0], plant_windows=np.array([1, 1, 2]))
H2_PRICE = 4.0                                                                 # $/kg, the nuclear flowsheet's default


def _loop(flowsheet, B, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from tests._highs_solver import HighsTensorLP
    return BatchedDoubleLoop(flowsheet, B, lp_backend=HighsTensorLP, **kw)


def _columns(loop):
    """named columns of period 0 of the tracker (the template's block: every plant shares its column order)"""
    model = loop.tracker_template.model
    fam = getattr(model.block, {"wind_battery": "windBattery", "wind_pem": "windPEM", "nuclear": "nuclear"}[loop.flowsheet])
    cols = {name: var.index for name, var in fam["periods"][0].items()}
    if loop.flowsheet == "wind_pem":
        cols["pem_system_capacity"] = fam["pem_system_capacity"].index
    cols["under"], cols["over"] = model.power_underdelivered[0].index, model.power_overdelivered[0].index
    return cols


def closed_forms(loop, x, hour):
    """the ledger of the hour that starts at clock `hour` on the tracker's solution x [B, n], from physical quantities"""
    c = _columns(loop)
    v = lambda name: x[:, c[name]]
    out = dict(under_mwh=v("under"), over_mwh=v("over"))
    if loop.flowsheet != "nuclear":
        wind_kw = (loop.wind_mw if loop.sized else np.full(loop.B, loop.bidder.bidding_model_object._wind_pmax_mw)) * 1e3
        cf = loop.cf_series.numpy()[(loop.start.numpy() + hour) % loop.N]
        curtailed_kw = wind_kw * cf - v("wind")
        out["curtailed_mwh"] = curtailed_kw * 1e-3
    if loop.flowsheet == "wind_battery":
        out["tot_cost"] = (wind_kw * prm.wind_op_cost / 8760 + prm.battery_degradation_rate * prm.batt_rep_cost_kwh * (v("energy_throughput") - v("thr_prev"))
                           + 1e3 * out["curtailed_mwh"])
    elif loop.flowsheet == "wind_pem":
        out["tot_cost"] = (wind_kw * prm.wind_op_cost / 8760 + v("pem_system_capacity") * prm.pem_op_cost / 8760 + v("pem_elec") * prm.pem_var_cost
                           + curtailed_kw)
        out["h2_kg"] = v("pem_elec") * prm.pem_electricity_to_mol / prm.h2_mols_per_kg * 3600
        out["pem_mwh"] = v("pem_elec") * 1e-3
    else:
        out["h2_kg"] = v("outlet_to_pipeline") * prm.mw_h2 * 3600
        out["pem_mwh"] = v("pem_elec") * 1e-3
        out["h2_revenue"] = out["h2_kg"] * H2_PRICE
        out["tot_cost"] = (prm.np_capacity_mw * prm.npp_vom + v("pem_elec") * 1e-3 * prm.nuclear_pem_vom + v("tank_holdup") * prm.mw_h2 * prm.tank_vom
                           - out["h2_kg"] * H2_PRICE)
    return out


KEYS = dict(wind_battery=["tot_cost", "under_mwh", "over_mwh", "curtailed_mwh"],
            wind_pem=["tot_cost", "under_mwh", "over_mwh", "curtailed_mwh", "h2_kg", "pem_mwh"],
            nuclear=["tot_cost", "under_mwh", "over_mwh", "h2_kg", "pem_mwh", "h2_revenue"])
# what two days of the project's data make non-zero (by more than rounding) in some plant-hour; the rest is pinned in
# test_forms_the_data_leaves_at_zero
SHOWN = dict(wind_battery=["tot_cost", "under_mwh", "over_mwh", "curtailed_mwh"], wind_pem=["tot_cost", "h2_kg", "pem_mwh"],
             nuclear=["tot_cost", "over_mwh", "h2_kg", "pem_mwh", "h2_revenue"],
             wind_battery_sized=["tot_cost", "under_mwh", "curtailed_mwh"])         # (its point: the per-plant constants)


@pytest.mark.parametrize("flowsheet, kw", [("wind_battery", {}), ("wind_pem", {}), ("nuclear", {}), ("wind_battery", SIZED)],
                         ids=["wind_battery", "wind_pem", "nuclear", "wind_battery_sized"])
def test_hourly_values_against_closed_forms(flowsheet, kw):
    """B = 3, stochastic bidder, two days (a midnight is crossed): ledger_hour of every hour equals the closed forms to 1e-9 (relative,
    floor 1e-9: the same x, another summation order), the accumulators equal the running sum of ledger_hour exactly, profit ==
    revenue - tot_cost exactly, and every key of SHOWN is non-zero in some plant-hour."""
    loop = _loop(flowsheet, 3, ledger=True, **STOCHASTIC, **kw)
    assert loop.ledger_keys == KEYS[flowsheet] and loop.ledger_hour.shape == (len(KEYS[flowsheet]), 3)
    running = np.zeros((len(loop.ledger_keys), 3))
    largest = dict.fromkeys(loop.ledger_keys, 0.0)
    for day in range(2):
        loop.day_ahead()
        for k in range(24):
            hour = loop.hour
            loop.hour_step()
            booked = loop.ledger_hour.numpy()
            want = closed_forms(loop, loop.tr.out["x"].numpy(), hour)
            for f, key in enumerate(loop.ledger_keys):
                np.testing.assert_allclose(booked[f], want[key], rtol=1e-9, atol=1e-9, err_msg=f"{key}, day {day} hour {k}")
                largest[key] = max(largest[key], float(np.abs(booked[f]).max()))
            running += booked
            assert np.array_equal(loop.ledger_acc.numpy(), running)
    res, ok = loop.results()
    assert ok
    for f, key in enumerate(loop.ledger_keys):
        assert np.array_equal(res[key].numpy(), running[f])
    assert np.array_equal(res["profit"].numpy(), res["obj"].numpy() - res["tot_cost"].numpy())
    print(flowsheet, "largest booked value per key:", largest)
    for key in SHOWN[flowsheet + ("_sized" if kw else "")]:
        assert largest[key] > 1e-6, (key, largest)
    loop.reset()
    assert not loop.ledger_acc.numpy().any() and not loop.ledger_hour.numpy().any()


@pytest.mark.parametrize("flowsheet", ["wind_pem", "nuclear"])
def test_forms_the_data_leaves_at_zero(flowsheet):
    """In two days of the project's data the wind + PEM plant never curtails (its PEM takes what the grid does not) and never
    over-delivers, and the nuclear plant never under-delivers.  Those forms - and every other one - are pinned here on a HAND-SET
    tracker solution through the tensor statement of the ledger (_ledger_book), hour 5 of the plants' windows."""
    import torch
    loop = _loop(flowsheet, 3, ledger=True, **STOCHASTIC)
    rng = np.random.default_rng(7)
    x = rng.uniform(1.0, 1000.0, size=(3, loop.tr.lp.n))
    c = _columns(loop)
    if flowsheet == "wind_pem":
        cf = loop.cf_series.numpy()[(loop.start.numpy() + 5) % loop.N]
        x[:, c["wind"]] = 847e3 * cf * np.array([0.25, 0.5, 1.0])                # plants 0 and 1 curtail three quarters / half of the wind
    loop.hour_t.fill_(5)
    loop._ledger_book(torch.as_tensor(x))
    want = closed_forms(loop, x, 5)
    booked = loop.ledger_hour.numpy()
    for f, key in enumerate(loop.ledger_keys):
        np.testing.assert_allclose(booked[f], want[key], rtol=1e-9, atol=1e-9, err_msg=key)
    for key in ("under_mwh", "over_mwh") + (("curtailed_mwh",) if flowsheet == "wind_pem" else ()):
        assert np.abs(booked[loop.ledger_keys.index(key)]).max() > 1e-3, key
    assert np.array_equal(loop.ledger_acc.numpy(), booked)


MODES = [("nuclear", {}), ("nuclear", STOCHASTIC), ("wind_pem", dict(bidder="parametrized", bid_price=[15.0, 25.0], storage_mw=[100.0, 200.0], market="price_taker")),
         ("wind_pem", dict(STOCHASTIC, bidder="self_schedule")), ("nuclear", dict(STOCHASTIC, scenario_coupling="monotone")),
         ("nuclear", dict(STOCHASTIC, ruc_hour=16)), ("wind_battery", dict(STOCHASTIC, wind_mw=[100.0, 300.0], battery_mw=[10.0, 50.0]))]


@pytest.mark.parametrize("flowsheet, kw", MODES, ids=["deterministic", "stochastic", "parametrized", "self_schedule", "monotone", "ruc_hour", "sized"])
def test_ledger_on_against_off(flowsheet, kw):
    """two days with ledger=True and with False: revenue, energy, state, offers, curves, dispatches and solve counts bit-identical, the
    existing results() keys unchanged; the ledger only ADDS keys"""
    on, off = _loop(flowsheet, 2, ledger=True, **kw), _loop(flowsheet, 2, **kw)
    assert off.ledger is False and not hasattr(off, "ledger_acc")
    for loop in (on, off):
        for _ in range(2):
            loop.run_day()
    (res_on, ok_on), (res_off, ok_off) = on.results(), off.results()
    assert ok_on and ok_off and on.solves == off.solves and on.hour == off.hour == 48
    expected = ["obj", "energy_mwh", "state"] + ([] if not off.stochastic else ["da_energy_mwh", "offered_mwh"]) + (["h2_kg"] if off.parametrized else [])
    assert sorted(res_off) == sorted(expected)
    assert sorted(res_on) == sorted(expected + on.ledger_keys + ["profit"])
    if on.parametrized:
        assert "h2_kg" not in on.ledger_keys and "pem_mwh" in on.ledger_keys     # the parametrized loop's own accumulator stays the only one
    for key in expected:
        assert np.array_equal(res_on[key].numpy(), res_off[key].numpy()), key
    names = ["da_offer", "da_prices", "delivered"] + (["da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch"] if off.stochastic else [])
    for name in names:
        assert np.array_equal(getattr(on, name).numpy(), getattr(off, name).numpy()), name
    assert on.ledger_acc.numpy()[0].all()                                         # every plant has booked a cost


def test_sweeps_return_the_ledger_when_asked():
    from dispatches_amd.sweeps import design_sweep, parametrized_sweep
    from tests._highs_solver import HighsTensorLP
    plain = design_sweep("wind_battery", [100.0, 300.0], [10.0], [4.0], 1, 1, lp_backend=HighsTensorLP)
    full = design_sweep("wind_battery", [100.0, 300.0], [10.0], [4.0], 1, 1, lp_backend=HighsTensorLP, ledger=True)
    assert sorted(plain) == ["all_optimal", "da_energy_mwh", "energy_mwh", "offered_mwh", "revenue", "throughput_kwh"]
    assert sorted(full) == sorted(list(plain) + KEYS["wind_battery"] + ["profit"])
    for key in plain:
        assert np.array_equal(plain[key], full[key]), key
    assert full["tot_cost"].shape == (2, 1, 1, 1) and np.array_equal(full["profit"], full["revenue"] - full["tot_cost"])
    assert (full["tot_cost"][1] > full["tot_cost"][0]).all()                     # three times the wind: three times the fixed O&M
    out = parametrized_sweep("wind_pem", [15.0], [100.0, 200.0], 1, 1, lp_backend=HighsTensorLP, ledger=True)
    assert out["pem_mwh"].shape == (1, 2, 1) and out["h2_kg"].shape == (1, 2, 1) and "profit" in out


def test_too_many_terms_are_refused(monkeypatch):
    from dispatches_amd import rolling_flowsheets as rf
    monkeypatch.setattr(rf, "LEDGER_MAX_TERMS", 2)
    with pytest.raises(ValueError, match="at most 2"):
        _loop("wind_battery", 2, ledger=True)                                     # tot_cost has three terms
    monkeypatch.setattr(rf, "LEDGER_MAX_TERMS", 8)
    monkeypatch.setattr(rf, "LEDGER_MAX_FORMS", 3)
    with pytest.raises(ValueError, match="at most 3 forms"):
        _loop("wind_battery", 2, ledger=True)


def test_ledger_descriptor_mirrors_the_header():
    """DspLoopLedgerDesc is a field-for-field copy of dsp_loop_ledger_desc (names, order, size), the limits are the header's, and the
    entry point is declared and exported"""
    import ctypes as C
    import os
    import re
    import __graft_entry__ as g
    g.build()
    from dispatches_amd import hip_solver, rolling_flowsheets
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsp_hip.h")).read()
    body = re.search(r"typedef struct dsp_loop_ledger_desc \{(.*?)\} dsp_loop_ledger_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = re.sub(r"\[[0-9\]\[]*\]", "", body)
    fields = [name for decl in body.split(";") if decl.strip() for name in re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", decl.strip().split(" ", 1)[-1])]
    fields = [f for f in fields if f not in ("const", "double", "int32_t", "int64_t")]
    assert fields == [f[0] for f in hip_solver.DspLoopLedgerDesc._fields_]
    assert C.sizeof(hip_solver.DspLoopLedgerDesc) == 8 + 4 * 8 + 4 * 64 + 8 * 8 + 6 * 8
    limits = {k: int(v) for k, v in re.findall(r"#define (DSP_LEDGER_MAX_\w+) (\d+)", hdr)}
    assert limits == dict(DSP_LEDGER_MAX_FORMS=hip_solver.LEDGER_MAX_FORMS, DSP_LEDGER_MAX_TERMS=hip_solver.LEDGER_MAX_TERMS)
    assert (rolling_flowsheets.LEDGER_MAX_FORMS, rolling_flowsheets.LEDGER_MAX_TERMS) == (8, 8)
    assert "dsp_loop_ledger" in hip_solver.EXPORTED_SYMBOLS and hasattr(hip_solver.load_library(), "dsp_loop_ledger")
    assert re.search(r"int dsp_loop_ledger\(const dsp_loop_state \*st, const dsp_loop_model \*tr, const dsp_loop_ledger_desc \*ledger, void \*hipStream\);", hdr)


def test_sized_wind_pem_books_each_plant_at_its_own_wind_size():
    """three wind sizes on one window (wind_waste in kW, scaled to MWh: the other unit convention), one day: every hour against the
    closed forms with the plant's own wind_kw, per-plant constants in the descriptor"""
    wind = np.array([100.0, 847.0, 1200.0])
    loop = _loop("wind_pem", 3, ledger=True, wind_mw=wind, plant_windows=np.zeros(3, np.int64), **STOCHASTIC)
    const = loop._ledger["const"].numpy()
    assert const.shape == (3, 6) and len(set(const[:, 0].tolist())) == 3 and np.abs(const[:, 3]).max() < 1e-9
    loop.day_ahead()
    for k in range(24):
        hour = loop.hour
        loop.hour_step()
        want = closed_forms(loop, loop.tr.out["x"].numpy(), hour)
        for f, key in enumerate(loop.ledger_keys):
            np.testing.assert_allclose(loop.ledger_hour.numpy()[f], want[key], rtol=1e-9, atol=1e-9, err_msg=f"{key}, hour {k}")
    tot = loop.results()[0]["tot_cost"].numpy()
    assert tot[0] < tot[1] < tot[2]
