"""Teacher-forced walk of a SIZED stochastic BatchedDoubleLoop (wind_mw / battery_mw / battery_mwh per plant; "wind_battery" or "wind_pem")
in the style of tests/_flowsheet_stochastic_oracle.py::oracle_walk: the loop is stepped, and after every step every LP of the chosen
plants is rebuilt by the oracle (oracle/dispatch_lp_oracle.py, HiGHS) from the recorded state with THAT plant's wind_kw, batt_kw,
batt_kwh, soc0, e0 - every day-ahead row, every real-time row whose horizon lies inside the cleared day, every tracking LP - and the
objectives (constant included) are compared at the project's parity contract, 1e-6 relative.  Curves and dispatches are
recomputed exactly from the read-back solutions with the helpers that file exports; the revenue is re-added.
`deterministic_walk` is the same for the deterministic loop (perfect forecaster, stub market): the day-ahead, hourly real-time and
tracking objectives of the chosen plants against the oracle's LPs of their own size and state."""
import numpy as np

from tests._flowsheet_stochastic_oracle import _power, clear, curve_of, reference_curve
from tests._stochastic_oracle import host_backcast


def plant_lps(loop, b):
    """(day-ahead, real-time, tracking) oracle LPs of plant b: callables of (T, cf, ..., state row of the plant)"""
    from oracle import dispatch_lp_oracle as orc
    kw = float(loop.wind_mw[b]) * 1e3
    if loop.flowsheet == "wind_pem":
        return (lambda T, cf, da, rt, st: orc.wind_pem_da(T, cf, da, rt, wind_kw=kw)[0],
                lambda T, cf, rt, cleared, st: orc.wind_pem_rt(T, cf, rt, cleared, wind_kw=kw)[0],
                lambda T, cf, disp, st: orc.wind_pem_track(T, cf, disp, wind_kw=kw)[0])
    if loop.flowsheet != "wind_battery":
        raise ValueError("sized plants: wind_battery or wind_pem")
    size = dict(wind_kw=kw, batt_kw=float(loop.battery_mw[b]) * 1e3, batt_kwh=float(loop.battery_mwh[b]) * 1e3)
    own = lambda st: dict(size, soc0=float(st[0]), e0=float(st[1]))       # (the loop fixes the throughput column from hour 0 on: e0 = state)
    return (lambda T, cf, da, rt, st: orc.wind_battery_da(T, cf, da, rt, **own(st))[0],
            lambda T, cf, rt, cleared, st: orc.wind_battery_rt(T, cf, rt, cleared, **own(st))[0],
            lambda T, cf, disp, st: orc.wind_battery_track(T, cf, disp, **own(st))[0])


def design_walk(loop, days, plants=None, tol=1e-6):
    """Steps `loop` (at hour 0 of a day) through `days` days and checks the plants of `plants` (None: all) at every step.
    -> dict of what was seen; per plant: the largest elec_in / elec_out of the implemented hours ("battery_kw"), the objective
    constants of the first day-ahead rows ("da_c0")."""
    B, S, D, N = loop.B, loop.S, loop.D, loop.N
    plants = list(range(B)) if plants is None else [int(b) for b in plants]
    lps = {b: plant_lps(loop, b) for b in plants}
    Tda, Trt, Ttr = loop.da.T, loop.rt.T, loop.tr.T
    num = lambda t: t.cpu().numpy().copy()
    da_s, rt_s, cf_s, start = num(loop.da_series), num(loop.rt_series), num(loop.cf_series), num(loop.start)
    pmin, market = loop.p_min_cents, loop.market
    rt_terms, rt_const = loop.rt.terms(), num(loop.rt.PT_const)
    tr_PT, tr_const = num(loop.tr.PT), num(loop.tr.PT_const)
    pda = num(loop.da.pda_cols)
    batt_cols = getattr(loop.tr, "batt_cols", [])[:2]                     # elec_in, elec_out of the tracker's first (implemented) period
    seen = dict(worst=0.0, lps=0, curves=0, below=0, equal=0, all_optimal=True, battery_kw={b: 0.0 for b in plants}, da_c0={},
                hourly_battery_kw={b: [] for b in plants})

    def scen(series, b, hour_abs, T):
        d, h = divmod(hour_abs, 24)
        if loop.forecaster == "perfect":
            return series[(start[b] + hour_abs + np.arange(T)) % N][None, :]
        return host_backcast(series, int(start[b]), d, h, T, S, D)

    def gap(got, ref, what):
        g = abs(got - ref) / max(1.0, abs(ref))
        seen["worst"] = max(seen["worst"], g)
        seen["lps"] += 1
        assert g <= tol, (loop.flowsheet, what, got, ref, g)

    def check_curve(b, t, powers, prices, ok, lmp, curve, count, dispatch, what):
        U, M = reference_curve(powers, prices, ok, pmin)
        assert (U, M) == curve_of(curve, count), (what, b, t, U, M, curve.tolist(), int(count))
        want = clear(U, M, lmp, market)
        assert want == float(dispatch), (what, b, t, want, float(dispatch))
        seen["curves"] += 1
        seen["below" if want < U[-1] / 100.0 else "equal"] += 1

    revenue = num(loop.revenue)
    hour_abs = loop.hour
    assert hour_abs % 24 == 0
    for _ in range(days):
        state0 = num(loop.state)
        loop.day_ahead()
        x, st = num(loop.da.out["x"]), num(loop.da.out["status"])
        c0 = num(loop.da.c0)
        obj = num(loop.da.out["obj"]) + c0
        seen["all_optimal"] &= not st.any()
        offer, da_prices = num(loop.da_offer), num(loop.da_prices)
        curve, count = num(loop.da_curve), num(loop.da_count)
        for b in plants:
            da_lp = lps[b][0]
            idx = (start[b] + hour_abs + np.arange(Tda)) % N
            da_f, rt_f = scen(da_s, b, hour_abs, Tda), scen(rt_s, b, hour_abs, Tda)
            assert np.array_equal(da_prices[b], da_s[idx][:24])
            seen["da_c0"].setdefault(b, float(c0[b * S]))
            for i in range(S):
                gap(obj[b * S + i], da_lp(Tda, cf_s[idx], da_f[i], rt_f[i], state0[b]).solve(tight=True)[1], ("da", b, i))
            for t in range(24):
                rows = slice(b * S, (b + 1) * S)
                check_curve(b, t, x[rows, pda[t]], da_f[:, t], st[rows] == 0, da_s[idx][t], curve[b, t], count[b, t], offer[b, t], "da")
        for h in range(24):
            state0 = num(loop.state)
            loop.hour_step()
            x, st = num(loop.rt.out["x"]), num(loop.rt.out["status"])
            obj = num(loop.rt.out["obj"]) + num(loop.rt.c0)
            x_tr = num(loop.tr.out["x"])
            obj_tr = num(loop.tr.out["obj"]) + num(loop.tr.c0)
            seen["all_optimal"] &= not st.any() and not num(loop.tr.out["status"]).any()
            curve, count, dispatch = num(loop.rt_curve), num(loop.rt_count), num(loop.rt_dispatch)
            delivered = num(loop.delivered)
            for b in range(B):
                idx = (start[b] + hour_abs + np.arange(Trt)) % N
                if b in lps:
                    _, rt_lp, tr_lp = lps[b]
                    cf = cf_s[idx]
                    rt_f = scen(rt_s, b, hour_abs, Trt)
                    if h + Trt <= 24:                # the oracle's real-time LP fixes every hour of its horizon: hours inside the cleared day
                        cleared = offer[b, h:h + Trt]
                        for i in range(S):
                            # (the product keeps day_ahead_power as a fixed column: its objective carries - DA . cleared, the oracle's form does not)
                            ref = rt_lp(Trt, cf, rt_f[i], cleared, state0[b]).solve(tight=True)[1] - float(da_prices[b, h:h + Trt] @ cleared)
                            gap(obj[b * S + i], ref, ("rt", b, i, h))
                    rows = range(b * S, (b + 1) * S)
                    for t in range(Ttr):
                        powers = [_power(rt_terms, rt_const, x[r], t) for r in rows]
                        lmp = rt_s[idx][0] if t == 0 else rt_f[0, t]
                        check_curve(b, t, powers, rt_f[:, t], st[b * S:(b + 1) * S] == 0, lmp, curve[b, t], count[b, t], dispatch[b, t], ("rt", h))
                    gap(obj_tr[b], tr_lp(Ttr, cf[:Ttr], dispatch[b], state0[b]).solve(tight=True)[1], ("track", b, h))
                    got = float(x_tr[b] @ tr_PT[0] + tr_const[0])
                    assert abs(got - delivered[b]) <= 1e-9 * max(1.0, abs(got))
                    if batt_cols:
                        used = float(x_tr[b, batt_cols].max())
                        seen["hourly_battery_kw"][b].append(used)
                        seen["battery_kw"][b] = max(seen["battery_kw"][b], used)
                revenue[b] += delivered[b] * rt_s[idx][0] + offer[b, h] * (da_prices[b, h] - rt_s[idx][0])
            hour_abs += 1
        loop._warm = True                              # (as run_day: later days replay from graphs where the loop uses them)
    np.testing.assert_allclose(num(loop.revenue), revenue, rtol=1e-9, atol=1e-9)
    return seen


def deterministic_walk(loop, hours, plants=None, tol=1e-6):
    """Steps a SIZED deterministic loop (forecaster="perfect", market="stub", at hour 0) through day_ahead() and `hours` <= 24 - T_rt + 1
    hour steps; for every plant of `plants` the day-ahead objective and every hour's real-time and tracking objective (constant
    included) against the oracle's LP of that plant's size and recorded state.  -> dict(worst, lps, da_c0 per plant)"""
    plants = list(range(loop.B)) if plants is None else [int(b) for b in plants]
    lps = {b: plant_lps(loop, b) for b in plants}
    num = lambda t: t.cpu().numpy().copy()
    da_s, rt_s, cf_s, start, N = num(loop.da_series), num(loop.rt_series), num(loop.cf_series), num(loop.start), loop.N
    Tda, Trt, Ttr = loop.da.T, loop.rt.T, loop.tr.T
    rt_PT, rt_const = num(loop.rt.PT), num(loop.rt.PT_const)
    assert not loop.stochastic and loop.hour == 0 and hours <= 24 - Trt + 1
    seen = dict(worst=0.0, lps=0, da_c0={}, all_optimal=True)

    def gap(got, ref, what):
        g = abs(got - ref) / max(1.0, abs(ref))
        seen["worst"] = max(seen["worst"], g)
        seen["lps"] += 1
        assert g <= tol, (loop.flowsheet, what, got, ref, g)

    state0 = num(loop.state)
    offer = num(loop.day_ahead())
    c0 = num(loop.da.c0)
    obj = num(loop.da.out["obj"]) + c0
    seen["all_optimal"] &= not num(loop.da.out["status"]).any()
    for b in plants:
        idx = (start[b] + np.arange(Tda)) % N
        seen["da_c0"][b] = float(c0[b])
        gap(obj[b], lps[b][0](Tda, cf_s[idx], da_s[idx], rt_s[idx], state0[b]).solve(tight=True)[1], ("da", b))
    for h in range(hours):
        state0 = num(loop.state)
        loop.hour_step()
        obj, obj_tr = num(loop.rt.out["obj"]) + num(loop.rt.c0), num(loop.tr.out["obj"]) + num(loop.tr.c0)
        seen["all_optimal"] &= not num(loop.rt.out["status"]).any() and not num(loop.tr.out["status"]).any()
        x = num(loop.rt.out["x"])
        for b in plants:
            idx = (start[b] + h + np.arange(Trt)) % N
            cleared = offer[b, h:h + Trt]
            # (the product keeps day_ahead_power as a fixed column: its objective carries - DA . cleared, the oracle's form does not)
            gap(obj[b], lps[b][1](Trt, cf_s[idx], rt_s[idx], cleared, state0[b]).solve(tight=True)[1] - float(da_s[idx] @ cleared), ("rt", b, h))
            dispatch = (x[b] @ rt_PT.T + rt_const)[:Ttr]                  # the stub market: the offer is the dispatch
            gap(obj_tr[b], lps[b][2](Ttr, cf_s[idx][:Ttr], dispatch, state0[b]).solve(tight=True)[1], ("track", b, h))
    return seen
