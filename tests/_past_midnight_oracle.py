"""Plain-Python statement of past_midnight="coupled" of dispatches_amd/rolling_flowsheets.py::BatchedDoubleLoop (bidder="self_schedule" or
scenario_coupling="monotone") and a walk that checks a running loop against it.  In the last T_rt - 1 hours of a day the real-time LP of
a plant is ONE LP: S copies of the flowsheet's bidding rows, built from the oracle's public row builders exactly as
tests/_self_schedule_oracle.py::_rt_lp_past_midnight builds one - day_ahead_power fixed to the cleared offer inside the day and free past
midnight, on scenario i's forecasts -, tied through lp.row over ALL T_rt periods:

    self-schedule   pda[s, t] - pda[0, t] = 0
    monotone        pda[k, t] - pda[j, t] >= 0 if rt[k, t] > rt[j, t],   <= 0 if rt[k, t] < rt[j, t],   no row if the prices are equal

(the order of the REAL-TIME scenario prices: what the host passes, energy_prices=rt), not through workflow/coupling.py.  Day-ahead LPs,
the hours whose horizon stays inside the day and the tracking LPs are those of the two modes' own walks."""
import numpy as np

from oracle import dispatch_lp_oracle as orc
from tests._flowsheet_stochastic_oracle import _power, clear, curve_of, reference_curve
from tests._monotone_oracle import monotone_da
from tests._self_schedule_oracle import _rows, _rt_lp, _rt_lp_past_midnight, _track_lp, coupled_da
from tests._stochastic_oracle import host_backcast

INF = float("inf")


def tied_rt(loop, T, cf, da, rt, cleared, state):
    """S = len(rt) copies of the late hour's bidding LP in ONE LP with the mode's coupling rows -> (PreparedLP, pda columns per scenario)"""
    lp = orc._LP()
    pdas = []
    for s in range(len(rt)):
        pda, _u = orc.add_da_bidding(lp, _rows(loop, lp, T, cf, state), da[s], rt[s])
        for t, v in enumerate(cleared):
            lp.lb[pda[t]] = lp.ub[pda[t]] = float(v)
        pdas.append(pda)
    for j in range(len(rt)):
        for k in range(j + 1, len(rt)):
            for t in range(T):
                if loop.self_schedule:
                    if j == 0:
                        lp.row({pdas[k][t]: 1.0, pdas[0][t]: -1.0}, 0.0, 0.0)
                    continue
                d = rt[k][t] - rt[j][t]
                if d > 0:
                    lp.row({pdas[k][t]: 1.0, pdas[j][t]: -1.0}, 0.0, INF)
                elif d < 0:
                    lp.row({pdas[k][t]: 1.0, pdas[j][t]: -1.0}, -INF, 0.0)
    return orc.PreparedLP(lp), pdas


def coupling_violation(loop, power, price):
    """power, price [S, T]: the worst violation [MW] of the mode's coupling rows by `power`"""
    worst = 0.0
    for j in range(len(power)):
        for k in range(j + 1, len(power)):
            diff = power[k] - power[j]
            if loop.self_schedule:
                worst = max(worst, float(np.abs(diff).max()))
            else:
                worst = max(worst, float(np.maximum(-diff * np.sign(price[k] - price[j]), 0.0).max()))
    return worst


def oracle_walk(loop, days, tol=1e-9):
    """Steps `loop` (a BatchedDoubleLoop with past_midnight="coupled" at hour 0 of a day) through `days` days and checks every step,
    teacher-forced from the loop's own state.  -> dict of what was seen; `late` holds one entry per late plant-hour: (day, hour, plant,
    relative margin of the coupled optimum over the sum of the S independent optima, violation of the coupling rows by those independent
    solutions [MW], violation by the loop's coupled solution [MW])."""
    B, S, D, N = loop.B, loop.S, loop.D, loop.N
    Tda, Trt, Ttr, n1 = loop.da.T, loop.rt.T, loop.tr.T, loop.da.n1
    per = 1 if loop.self_schedule else S
    num = lambda t: t.cpu().numpy().copy()
    da_s, rt_s = num(loop.da_series), num(loop.rt_series)
    cf_s = num(loop.cf_series) if loop.cf_series is not None else None
    start = num(loop.start)
    pmin, market = loop.p_min_cents, loop.market
    rt_terms, rt_const = loop.rt.terms(), num(loop.rt.PT_const)
    tr_PT, tr_const = num(loop.tr.PT), num(loop.tr.PT_const)
    pda_da, pda_rt = num(loop.da.pda_cols), num(loop.rt.pda_cols)
    seen = dict(worst=0.0, lps=0, curves=0, all_optimal=True, late=[], late_status=[], solves=0)

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

    def bid_pairs(powers, prices, ok):
        """the pairs of a plant and period as the mode offers them: a schedule is the one pair (block 0's power, 0)"""
        return ([powers[0]], [0.0], [ok]) if loop.self_schedule else (powers, prices, [ok] * S)

    revenue = num(loop.revenue)
    hour_abs = loop.hour
    assert hour_abs % 24 == 0
    for day in range(days):
        state0 = num(loop.state)
        loop.day_ahead()
        seen["solves"] += B
        x, st = num(loop.da.out["x"]), num(loop.da.out["status"])
        obj = num(loop.da.out["obj"]) + num(loop.da.c0)
        seen["all_optimal"] &= not st.any()
        offer, da_prices = num(loop.da_offer), num(loop.da_prices)
        curve, count = num(loop.da_curve), num(loop.da_count)
        for b in range(B):
            idx = (start[b] + hour_abs + np.arange(Tda)) % N
            cf = cf_s[idx] if cf_s is not None else None
            da_f, rt_f = scen(da_s, b, hour_abs, Tda), scen(rt_s, b, hour_abs, Tda)
            P = (coupled_da if loop.self_schedule else monotone_da)(loop, Tda, cf, da_f, rt_f, state0[b])[0]
            if st[b] == 0:                           # (a plant whose day-ahead solve failed shows in all_optimal; its bid drops out)
                gap(obj[b], P.solve(tight=True)[1], ("da", b, day))
            else:
                seen["lps"] += 1
            power = x[b].reshape(S, n1)[:, pda_da]
            for t in range(24):
                check_curve(b, t, *bid_pairs(power[:, t], da_f[:, t], st[b] == 0), da_s[idx][t], curve[b, t], count[b, t], offer[b, t], "da")
        for h in range(24):
            state0 = num(loop.state)
            loop.hour_step()
            late = h + Trt > 24
            m = loop.rtc if late else loop.rt
            x, st = num(m.out["x"]), num(m.out["status"])
            obj = num(m.out["obj"]) + num(m.c0)
            assert x.shape == ((B, S * n_rt(loop)) if late else (B * per, n_rt(loop)))
            seen["solves"] += (B if late else B * per) + B
            x_tr = num(loop.tr.out["x"])
            obj_tr = num(loop.tr.out["obj"]) + num(loop.tr.c0)
            seen["all_optimal"] &= not st.any() and not num(loop.tr.out["status"]).any()
            if late:
                seen["late_status"].append(st.copy())
            curve, count, dispatch = num(loop.rt_curve), num(loop.rt_count), num(loop.rt_dispatch)
            delivered = num(loop.delivered)
            for b in range(B):
                idx = (start[b] + hour_abs + np.arange(Trt)) % N
                cf = cf_s[idx] if cf_s is not None else None
                rt_f = scen(rt_s, b, hour_abs, Trt)
                if not late:                         # the horizon inside the cleared day: the modes' own hourly LPs, one per row
                    cleared = offer[b, h:h + Trt]
                    for i in range(per):
                        ref = _rt_lp(loop, Trt, cf, rt_f[i], cleared, state0[b]).solve(tight=True)[1] - float(da_prices[b, h:h + Trt] @ cleared)
                        gap(obj[b * per + i], ref, ("rt", b, i, h))
                    blocks, oks = x[b * per:(b + 1) * per], st[b * per:(b + 1) * per] == 0
                else:                                # past midnight: ONE LP per plant, the S scenarios tied
                    known = 24 - h
                    da_f = scen(da_s, b, hour_abs, Trt)
                    da = np.array([np.concatenate([da_prices[b, h:], da_f[i, known:]]) for i in range(S)])
                    P, _ = tied_rt(loop, Trt, cf, da, rt_f, offer[b, h:], state0[b])
                    ref = P.solve(tight=True)[1]
                    gap(obj[b], ref, ("rt tied", b, h))
                    alone = [_rt_lp_past_midnight(loop, Trt, cf, da[i], rt_f[i], offer[b, h:], state0[b]) for i in range(S)]
                    sols = [Q.solve(tight=True) for Q in alone]
                    total = sum(f for _, f in sols)
                    free = np.stack([free_pda(loop, Trt, cf, da[i], rt_f[i], offer[b, h:], state0[b], sols[i][0]) for i in range(S)])
                    blocks = x[b].reshape(S, -1)
                    seen["late"].append((day, h, b, (ref - total) / max(1.0, abs(total)), coupling_violation(loop, free, rt_f),
                                         coupling_violation(loop, blocks[:, pda_rt], rt_f)))
                    oks = np.full(S, st[b] == 0)
                for t in range(Ttr):
                    lmp = rt_s[idx][0] if t == 0 else rt_f[0, t]
                    powers = [_power(rt_terms, rt_const, blocks[i], t) for i in range(len(blocks))]
                    pairs = ([powers[0]], [0.0], [oks[0]]) if loop.self_schedule else (powers, rt_f[:, t], oks)
                    check_curve(b, t, *pairs, lmp, curve[b, t], count[b, t], dispatch[b, t], ("rt", h))
                Q = _track_lp(loop, Ttr, cf[:Ttr] if cf is not None else None, dispatch[b], state0[b])
                gap(obj_tr[b], Q.solve(tight=True)[1], ("track", b, h))
                got = float(x_tr[b] @ tr_PT[0] + tr_const[0])
                assert abs(got - delivered[b]) <= 1e-9 * max(1.0, abs(got))
                revenue[b] += delivered[b] * rt_s[idx][0] + offer[b, h] * (da_prices[b, h] - rt_s[idx][0])
            hour_abs += 1
        loop._warm = True                              # (as run_day: later days replay from graphs where the loop uses them)
    np.testing.assert_allclose(num(loop.revenue), revenue, rtol=1e-9, atol=1e-9)
    return seen


def n_rt(loop):
    return loop.rt.lp.n


def free_pda(loop, T, cf, da, rt, cleared, state, x):
    """day_ahead_power [T] of the oracle's solution x of ONE scenario's late-hour LP (_rt_lp_past_midnight: the same build, whose
    day_ahead_power columns are found by building it once more)"""
    lp = orc._LP()
    pda, _u = orc.add_da_bidding(lp, _rows(loop, lp, T, cf, state), da, rt)
    return np.asarray(x)[pda]
