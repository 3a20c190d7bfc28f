"""Plain-Python statement of the self-scheduling mode of dispatches_amd/rolling_flowsheets.py::BatchedDoubleLoop (bidder="self_schedule")
and a walk that checks a running loop against it.  The coupled day-ahead LP of every plant is built from the oracle's public row builders
(oracle/dispatch_lp_oracle.py: _LP, wind_battery_rows / wind_pem_rows / nuclear_rows, add_da_bidding, lp.row for the rows
pda[s, t] - pda[0, t] = 0), exactly as its wind_battery_da_coupled does for one flowsheet; the hourly LPs are the oracle's *_rt on
scenario 0 (in the last T_rt - 1 hours of a day: the same rows with day_ahead_power free past midnight, the loop's own choice) and
*_track; curves and dispatches are rebuilt from the read-back solutions by the rule (one pair (power, 0), the p_min point in front), not
through workflow/market.py::plant_curves."""
import numpy as np

from oracle import dispatch_lp_oracle as orc
from tests._flowsheet_stochastic_oracle import _power, clear, curve_of, reference_curve
from tests._stochastic_oracle import host_backcast


def _rows(loop, lp, T, cf, state):
    if loop.flowsheet == "wind_battery":
        return orc.wind_battery_rows(lp, T, cf, loop.rt.wind[1], 25e3, 100e3, float(state[0]), float(state[1]))
    if loop.flowsheet == "wind_pem":
        return orc.wind_pem_rows(lp, T, cf, loop.rt.wind[1])
    return orc.nuclear_rows(lp, T, float(state[0]))


def coupled_da(loop, T, cf, da, rt, state):
    """S = len(da) copies of the flowsheet's day-ahead bidding LP in ONE LP, tied by pda[s, t] = pda[0, t] -> (PreparedLP, pda columns)"""
    lp = orc._LP()
    pdas = []
    for s in range(len(da)):
        pda, _u = orc.add_da_bidding(lp, _rows(loop, lp, T, cf, state), da[s], rt[s])
        pdas.append(pda)
    for s in range(1, len(da)):
        for t in range(T):
            lp.row({pdas[s][t]: 1.0, pdas[0][t]: -1.0}, 0.0, 0.0)
    return orc.PreparedLP(lp), pdas


def independent_da(loop, T, cf, da, rt, state):
    """ONE scenario's day-ahead LP -> (PreparedLP, pda columns)"""
    lp = orc._LP()
    pda, _u = orc.add_da_bidding(lp, _rows(loop, lp, T, cf, state), da, rt)
    return orc.PreparedLP(lp), pda


def _rt_lp(loop, T, cf, rt, cleared, state):
    lp = orc._LP()
    orc.add_rt_bidding(lp, _rows(loop, lp, T, cf, state), rt, cleared)
    return orc.PreparedLP(lp)


def _rt_lp_past_midnight(loop, T, cf, da, rt, cleared, state):
    """the hourly LP of the last T - 1 hours of a day, as THIS loop states it (its own choice: scenario 0 alone, nothing tied across
    scenarios): day_ahead_power fixed to the cleared offer in the len(cleared) periods inside the day and FREE past midnight, where it
    earns scenario 0's day-ahead forecast.  The day-ahead bidding form with fixed columns: its objective carries - DA . cleared itself."""
    lp = orc._LP()
    pda, _u = orc.add_da_bidding(lp, _rows(loop, lp, T, cf, state), da, rt)
    for t, v in enumerate(cleared):
        lp.lb[pda[t]] = lp.ub[pda[t]] = float(v)
    return orc.PreparedLP(lp)


def _track_lp(loop, T, cf, dispatch, state):
    lp = orc._LP()
    orc.add_tracking(lp, _rows(loop, lp, T, cf, state), dispatch)
    return orc.PreparedLP(lp)


def oracle_walk(loop, days, tol=1e-6):
    """Steps `loop` (a self-scheduling BatchedDoubleLoop at hour 0 of a day) through `days` days with day_ahead() / hour_step() and
    checks every step, teacher-forced from the loop's own state.  -> dict of what was seen: the worst relative objective gap, and for
    day 0 of every plant the margin of the coupled optimum over the sum of the independent optima (relative) and the largest
    distance [MW] of the schedule from scenario 0's independent day_ahead_power."""
    B, S, D, N = loop.B, loop.S, loop.D, loop.N
    Tda, Trt, Ttr, n1 = loop.da.T, loop.rt.T, loop.tr.T, loop.da.n1
    num = lambda t: t.cpu().numpy().copy()
    da_s, rt_s = num(loop.da_series), num(loop.rt_series)
    cf_s = num(loop.cf_series) if loop.cf_series is not None else None
    start = num(loop.start)
    pmin, market = loop.p_min_cents, loop.market
    rt_terms, rt_const = loop.rt.terms(), num(loop.rt.PT_const)
    tr_PT, tr_const = num(loop.tr.PT), num(loop.tr.PT_const)
    pda = num(loop.da.pda_cols)
    seen = dict(worst=0.0, lps=0, curves=0, all_optimal=True, coupling_margin=[], schedule_distance=[], two_points=0, one_point=0,
                first_powers=set(), below=0, past_midnight=0)

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

    def check_curve(b, t, power, ok, lmp, curve, count, dispatch, what):
        U, M = reference_curve([power], [0.0], [ok], pmin)
        assert (U, M) == curve_of(curve, count), (what, b, t, U, M, curve.tolist(), int(count))
        assert 1 <= len(U) <= 2 and not any(M) and U[0] == pmin
        want = clear(U, M, lmp, market)
        assert want == float(dispatch), (what, b, t, want, float(dispatch))
        seen["curves"] += 1
        seen["two_points" if len(U) == 2 else "one_point"] += 1
        seen["first_powers"].add(U[0])
        seen["below"] += want < U[-1] / 100.0

    revenue = num(loop.revenue)
    hour_abs = loop.hour
    assert hour_abs % 24 == 0
    for day in range(days):
        state0 = num(loop.state)
        loop.day_ahead()
        x, st = num(loop.da.out["x"]), num(loop.da.out["status"])
        obj = num(loop.da.out["obj"]) + num(loop.da.c0)
        assert x.shape == (B, S * n1)
        seen["all_optimal"] &= not st.any()
        offer, da_prices = num(loop.da_offer), num(loop.da_prices)
        curve, count = num(loop.da_curve), num(loop.da_count)
        assert curve.shape == (B, 24, S + 1, 2)
        for b in range(B):
            idx = (start[b] + hour_abs + np.arange(Tda)) % N
            cf = cf_s[idx] if cf_s is not None else None
            da_f, rt_f = scen(da_s, b, hour_abs, Tda), scen(rt_s, b, hour_abs, Tda)
            assert np.array_equal(da_prices[b], da_s[idx][:24])
            P, _ = coupled_da(loop, Tda, cf, da_f, rt_f, state0[b])
            ref = P.solve(tight=True)[1]
            gap(obj[b], ref, ("da", b, day))
            schedule = x[b, pda[:24]]                                    # block 0
            if day == 0 and S > 1:
                alone = [independent_da(loop, Tda, cf, da_f[i], rt_f[i], state0[b]) for i in range(S)]
                sols = [Q.solve(tight=True) for Q, _ in alone]
                total = sum(f for _, f in sols)
                seen["coupling_margin"].append((ref - total) / abs(total))
                seen["schedule_distance"].append(float(np.abs(schedule - sols[0][0][alone[0][1]][:24]).max()))
            for t in range(24):
                check_curve(b, t, schedule[t], st[b] == 0, da_s[idx][t], curve[b, t], count[b, t], offer[b, t], "da")
        for h in range(24):
            state0 = num(loop.state)
            loop.hour_step()
            x, st = num(loop.rt.out["x"]), num(loop.rt.out["status"])
            obj = num(loop.rt.out["obj"]) + num(loop.rt.c0)
            assert x.shape[0] == B
            x_tr = num(loop.tr.out["x"])
            obj_tr = num(loop.tr.out["obj"]) + num(loop.tr.c0)
            seen["all_optimal"] &= not st.any() and not num(loop.tr.out["status"]).any()
            curve, count, dispatch = num(loop.rt_curve), num(loop.rt_count), num(loop.rt_dispatch)
            delivered = num(loop.delivered)
            for b in range(B):
                idx = (start[b] + hour_abs + np.arange(Trt)) % N
                cf = cf_s[idx] if cf_s is not None else None
                rt_f = scen(rt_s, b, hour_abs, Trt)
                if h + Trt <= 24:                    # the oracle's real-time LP fixes every hour of its horizon: hours inside the cleared day
                    cleared = offer[b, h:h + Trt]
                    # (the product keeps day_ahead_power as a fixed column: its objective carries - DA . cleared, the oracle's form does not)
                    ref = _rt_lp(loop, Trt, cf, rt_f[0], cleared, state0[b]).solve(tight=True)[1] - float(da_prices[b, h:h + Trt] @ cleared)
                    gap(obj[b], ref, ("rt", b, h))
                else:                                # look-ahead past midnight: free day_ahead_power there, on scenario 0's day-ahead forecast
                    known = 24 - h
                    da = np.concatenate([da_prices[b, h:], scen(da_s, b, hour_abs, Trt)[0, known:]])
                    ref = _rt_lp_past_midnight(loop, Trt, cf, da, rt_f[0], offer[b, h:], state0[b]).solve(tight=True)[1]
                    gap(obj[b], ref, ("rt past midnight", b, h))
                    seen["past_midnight"] += 1
                for t in range(Ttr):
                    lmp = rt_s[idx][0] if t == 0 else rt_f[0, t]
                    check_curve(b, t, _power(rt_terms, rt_const, x[b], t), st[b] == 0, lmp, curve[b, t], count[b, t], dispatch[b, t], ("rt", h))
                Q = _track_lp(loop, Ttr, cf[:Ttr] if cf is not None else None, dispatch[b], state0[b])
                gap(obj_tr[b], Q.solve(tight=True)[1], ("track", b, h))
                got = float(x_tr[b] @ tr_PT[0] + tr_const[0])
                assert abs(got - delivered[b]) <= 1e-9 * max(1.0, abs(got))
                revenue[b] += delivered[b] * rt_s[idx][0] + offer[b, h] * (da_prices[b, h] - rt_s[idx][0])
            hour_abs += 1
        loop._warm = True                              # (as run_day: later days replay from graphs where the loop uses them)
    np.testing.assert_allclose(num(loop.revenue), revenue, rtol=1e-9, atol=1e-9)
    return seen
