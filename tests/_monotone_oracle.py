"""Plain-Python statement of the monotone-bid-curve mode of dispatches_amd/rolling_flowsheets.py::BatchedDoubleLoop (bidder="lp",
scenario_coupling="monotone") and a walk that checks a running loop against it.  The coupled day-ahead LP of every plant is built from
the oracle's public row builders (oracle/dispatch_lp_oracle.py: _LP, wind_battery_rows / wind_pem_rows / nuclear_rows, add_da_bidding)
plus lp.row for every ordered pair j < k and period t,

    pda[k, t] - pda[j, t] >= 0  if da[k, t] > da[j, t],     <= 0  if da[k, t] < da[j, t],     no row if the prices are equal,

which is idaes' Bidder rule (day_ahead_power[k, t] - day_ahead_power[j, t]) (price[k, t] - price[j, t]) >= 0 stated once more, not
through workflow/coupling.py.  The hourly LPs are the oracle's *_rt per scenario (in the last T_rt - 1 hours of a day: the same rows with
day_ahead_power free past midnight on scenario i's forecast, untied across scenarios - the loop's own choice) and *_track; curves and
dispatches are rebuilt from the read-back solutions by the rule (tests/_flowsheet_stochastic_oracle.py::reference_curve), and once more
WITHOUT the running maximum: an ordered solution needs no repair."""
import math

import numpy as np

from oracle import dispatch_lp_oracle as orc
from tests._flowsheet_stochastic_oracle import _power, clear, curve_of, reference_curve
from tests._self_schedule_oracle import _rows, _rt_lp, _rt_lp_past_midnight, _track_lp, independent_da
from tests._stochastic_oracle import host_backcast

INF = float("inf")


def monotone_da(loop, T, cf, da, rt, state):
    """S = len(da) copies of the flowsheet's day-ahead bidding LP in ONE LP, every pair j < k ordered by its day-ahead prices
    -> (PreparedLP, pda columns per scenario, numbers of (lower-side, upper-side, free) pair-periods)"""
    lp = orc._LP()
    pdas = []
    for s in range(len(da)):
        pda, _u = orc.add_da_bidding(lp, _rows(loop, lp, T, cf, state), da[s], rt[s])
        pdas.append(pda)
    cases = [0, 0, 0]
    for j in range(len(da)):
        for k in range(j + 1, len(da)):
            for t in range(T):
                d = da[k][t] - da[j][t]
                if d > 0:
                    lp.row({pdas[k][t]: 1.0, pdas[j][t]: -1.0}, 0.0, INF)
                elif d < 0:
                    lp.row({pdas[k][t]: 1.0, pdas[j][t]: -1.0}, -INF, 0.0)
                cases[0 if d > 0 else 1 if d < 0 else 2] += 1
    return orc.PreparedLP(lp), pdas, cases


def order_violations(power, price, tol=1e-6):
    """power, price [S, T] -> number of (pair, period) with (P_k - P_j) (price_k - price_j) < -tol, and the worst product"""
    S = len(power)
    count, worst = 0, 0.0
    for j in range(S):
        for k in range(j + 1, S):
            prod = (power[k] - power[j]) * (price[k] - price[j])
            count += int((prod < -tol).sum())
            worst = min(worst, float(prod.min()))
    return count, worst


def unrepaired_curve(power, price, p_min_cents):
    """the curve of one plant-hour WITHOUT the running maximum: cents, the highest price per distinct power, the p_min point in front"""
    best = {}
    for p, c in zip(power, price):
        pc, cc = int(round(round(float(p), 2) * 100)), int(round(round(float(c), 2) * 100))
        if pc >= p_min_cents and math.isfinite(p) and math.isfinite(c):
            best[pc] = max(best.get(pc, -(1 << 62)), cc)
    U = sorted(best)
    M = [best[u] for u in U]
    if p_min_cents not in best:
        M.insert(0, min(M) if M else 0)
        U.insert(0, int(p_min_cents))
    return U, M


def oracle_walk(loop, days, tol=1e-6):
    """Steps `loop` (a monotone BatchedDoubleLoop at hour 0 of a day) through `days` days with day_ahead() / hour_step() and checks
    every step, teacher-forced from the loop's own state.  -> dict of what was seen: the worst relative objective gap, the three row
    cases met, and for day 0 of every plant the margin of the coupled optimum over the sum of the independent optima (relative), the
    order violations of those independent optima, and the worst disorder [MW] of the coupled solution."""
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
    seen = dict(worst=0.0, lps=0, curves=0, all_optimal=True, coupling_margin=[], independent_violations=[], cases=[0, 0, 0], disorder=0.0,
                repaired=0, max_points=0, first_powers=set(), below=0, past_midnight=0)

    def scen(series, b, hour_abs, T):
        d, h = divmod(hour_abs, 24)
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
        seen["max_points"] = max(seen["max_points"], len(U))
        seen["first_powers"].add(U[0])
        seen["below"] += want < U[-1] / 100.0
        return U, M

    revenue = num(loop.revenue)
    hour_abs = loop.hour
    assert hour_abs % 24 == 0
    for day in range(days):
        state0 = num(loop.state)
        loop.day_ahead()
        x, st = num(loop.da.out["x"]), num(loop.da.out["status"])
        obj = num(loop.da.out["obj"]) + num(loop.da.c0)
        assert x.shape == (B, S * n1) and st.shape == (B,)
        seen["all_optimal"] &= not st.any()
        offer, da_prices = num(loop.da_offer), num(loop.da_prices)
        curve, count = num(loop.da_curve), num(loop.da_count)
        assert curve.shape == (B, 24, S + 1, 2)
        for b in range(B):
            idx = (start[b] + hour_abs + np.arange(Tda)) % N
            cf = cf_s[idx] if cf_s is not None else None
            da_f, rt_f = scen(da_s, b, hour_abs, Tda), scen(rt_s, b, hour_abs, Tda)
            assert np.array_equal(da_prices[b], da_s[idx][:24])
            P, _, cases = monotone_da(loop, Tda, cf, da_f, rt_f, state0[b])
            seen["cases"] = [a + c for a, c in zip(seen["cases"], cases)]
            ref = P.solve(tight=True)[1]
            gap(obj[b], ref, ("da", b, day))
            power = x[b].reshape(S, n1)[:, pda]                           # [S, Tda]: block i's day_ahead_power
            # monotone by construction: the pairs of every period sorted by price have non-decreasing power
            for t in range(Tda):
                order = np.lexsort((power[:, t], da_f[:, t]))
                seen["disorder"] = max(seen["disorder"], float(-np.diff(power[order, t]).min(initial=0.0)))
            if day == 0:
                alone = [independent_da(loop, Tda, cf, da_f[i], rt_f[i], state0[b]) for i in range(S)]
                sols = [Q.solve(tight=True) for Q, _ in alone]
                total = sum(f for _, f in sols)
                seen["coupling_margin"].append((ref - total) / abs(total))
                free = np.stack([sols[i][0][alone[i][1]] for i in range(S)])
                seen["independent_violations"].append(order_violations(free, da_f))
            for t in range(24):
                U, M = check_curve(b, t, power[:, t], da_f[:, t], [st[b] == 0] * S, da_s[idx][t], curve[b, t], count[b, t], offer[b, t], "da")
                if st[b] == 0:
                    U0, M0 = unrepaired_curve(power[:, t], da_f[:, t], pmin)
                    assert U0 == U
                    # ... to within one cent of power: the running maximum may only lift a point that sits within a cent of the point
                    # whose price it takes (two powers 1e-6 MW apart can round to neighbouring cents in either order)
                    for q in range(1, len(M0)):
                        top = max(range(q), key=lambda r: M0[r])
                        seen["repaired"] += M0[q] < M0[top] and U0[q] - U0[top] > 1
        for h in range(24):
            state0 = num(loop.state)
            loop.hour_step()
            x, st = num(loop.rt.out["x"]), num(loop.rt.out["status"])
            obj = num(loop.rt.out["obj"]) + num(loop.rt.c0)
            assert x.shape[0] == B * S
            x_tr = num(loop.tr.out["x"])
            obj_tr = num(loop.tr.out["obj"]) + num(loop.tr.c0)
            seen["all_optimal"] &= not st.any() and not num(loop.tr.out["status"]).any()
            curve, count, dispatch = num(loop.rt_curve), num(loop.rt_count), num(loop.rt_dispatch)
            delivered = num(loop.delivered)
            for b in range(B):
                idx = (start[b] + hour_abs + np.arange(Trt)) % N
                cf = cf_s[idx] if cf_s is not None else None
                rt_f = scen(rt_s, b, hour_abs, Trt)
                for i in range(S):
                    if h + Trt <= 24:                # the oracle's real-time LP fixes every hour of its horizon: hours inside the cleared day
                        cleared = offer[b, h:h + Trt]
                        # (the product keeps day_ahead_power as a fixed column: its objective carries - DA . cleared, the oracle's form does not)
                        ref = _rt_lp(loop, Trt, cf, rt_f[i], cleared, state0[b]).solve(tight=True)[1] - float(da_prices[b, h:h + Trt] @ cleared)
                        gap(obj[b * S + i], ref, ("rt", b, i, h))
                    else:                            # look-ahead past midnight: free day_ahead_power there, on scenario i's forecast, untied
                        known = 24 - h
                        da = np.concatenate([da_prices[b, h:], scen(da_s, b, hour_abs, Trt)[i, known:]])
                        ref = _rt_lp_past_midnight(loop, Trt, cf, da, rt_f[i], offer[b, h:], state0[b]).solve(tight=True)[1]
                        gap(obj[b * S + i], ref, ("rt past midnight", b, i, h))
                        seen["past_midnight"] += 1
                rows = range(b * S, (b + 1) * S)
                for t in range(Ttr):
                    powers = [_power(rt_terms, rt_const, x[r], t) for r in rows]
                    lmp = rt_s[idx][0] if t == 0 else rt_f[0, t]
                    check_curve(b, t, powers, rt_f[:, t], st[b * S:(b + 1) * S] == 0, lmp, curve[b, t], count[b, t], dispatch[b, t], ("rt", h))
                Q = _track_lp(loop, Ttr, cf[:Ttr] if cf is not None else None, dispatch[b], state0[b])
                gap(obj_tr[b], Q.solve(tight=True)[1], ("track", b, h))
                got = float(x_tr[b] @ tr_PT[0] + tr_const[0])
                assert abs(got - delivered[b]) <= 1e-9 * max(1.0, abs(got))
                revenue[b] += delivered[b] * rt_s[idx][0] + offer[b, h] * (da_prices[b, h] - rt_s[idx][0])
            hour_abs += 1
        loop._warm = True                              # (as run_day: later days replay from graphs where the loop uses them)
    np.testing.assert_allclose(num(loop.revenue), revenue, rtol=1e-9, atol=1e-9)
    return seen


def independent_violations(loop):
    """the day-ahead solutions of an INDEPENDENT stochastic loop after day_ahead(): per plant the number of (pair, period) with
    (P_k - P_j) (da_k - da_j) < -1e-6 over the 24 hours of the day, and the worst product"""
    B, S, D, N = loop.B, loop.S, loop.D, loop.N
    x = loop.da.out["x"].cpu().numpy()
    pda = loop.da.pda_cols.cpu().numpy()[:24]
    da_s, start = loop.da_series.cpu().numpy(), loop.start.cpu().numpy()
    day = (loop.hour // 24) if loop.hour % 24 == 0 else None
    assert day is not None
    out = []
    for b in range(B):
        da_f = host_backcast(da_s, int(start[b]), day, 0, 24, S, D)
        out.append(order_violations(x[b * S:(b + 1) * S][:, pda], da_f))
    return out
