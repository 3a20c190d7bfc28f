"""Plain-Python statement of BatchedDoubleLoop's ruc_hour mode (dispatches_amd/rolling_flowsheets.py: the day-ahead bid of day d + 1 made
at hour H of day d on a state PROJECTED to midnight) and a walk that checks a running loop against it, teacher-forced from the trace the
loop keeps: every LP of the projection chain rebuilt from the oracle's own rows (oracle/dispatch_lp_oracle.py: wind_battery_rows /
nuclear_rows) with tracking rows on the periods inside the day only, the hand-off rounding, every day-ahead LP of the pending bid on the
projected state, the windows at 24 (d + 1) and the backcast rule of the bid (day-ahead history up to day d, real-time history up to day
d - 1), curves and dispatches recomputed exactly, and the pending buffers against the current ones before and after midnight."""
import numpy as np

from tests._flowsheet_stochastic_oracle import clear, curve_of, reference_curve
from tests._stochastic_oracle import host_backcast


def plant_sizes(loop, b):
    """(wind_kw, batt_kw, batt_kwh) of plant b (wind + battery), the default plant's where the loop is not sized"""
    if getattr(loop, "sized", False):
        return float(loop.wind_mw[b]) * 1e3, float(loop.battery_mw[b]) * 1e3, float(loop.battery_mwh[b]) * 1e3
    return float(loop.tr.wind[1]), 25e3, 100e3


def projection_lp(loop, b, cf, dispatch, state):
    """the tracking LP of one chain step for plant b: the flowsheet's rows over the whole horizon, the cost of every period, and
    P_T + under - over = dispatch on the first len(dispatch) periods ONLY (the later rows are free: their under / over carry a penalty
    and no constraint, so they are 0 and leave the LP)"""
    from oracle import dispatch_lp_oracle as orc
    T = loop.tr.T
    lp = orc._LP()
    if loop.flowsheet == "wind_battery":
        kw, bkw, bkwh = plant_sizes(loop, b)
        fs = orc.wind_battery_rows(lp, T, cf, kw, bkw, bkwh, soc0=float(state[0]), e0=float(state[1]))
    elif loop.flowsheet == "nuclear":
        fs = orc.nuclear_rows(lp, T, holdup0=float(state[0]))
    else:
        raise ValueError("the projection chain runs for the flowsheets with state: wind_battery, nuclear")
    for t in range(T):
        lp.add_cost(fs["cost"][t], 1.0)
    for t in range(len(dispatch)):
        under, over = lp.var(f"under{t}"), lp.var(f"over{t}")
        d, k = fs["P_T"][t]
        row = dict(d)
        row[under], row[over] = 1.0, -1.0
        lp.row(row, dispatch[t] - k, dispatch[t] - k)
        lp.add_cost(orc._lin((under, orc.TRACK_PENALTY), (over, orc.TRACK_PENALTY)))
    return orc.PreparedLP(lp)


def day_ahead_lp(loop, b, cf, da, rt, state):
    from oracle import dispatch_lp_oracle as orc
    T = loop.da.T
    if loop.flowsheet == "wind_battery":
        kw, bkw, bkwh = plant_sizes(loop, b)
        return orc.wind_battery_da(T, cf, da, rt, wind_kw=kw, batt_kw=bkw, batt_kwh=bkwh, soc0=float(state[0]), e0=float(state[1]))[0]
    if loop.flowsheet == "nuclear":
        return orc.nuclear_da(T, da, rt, holdup0=float(state[0]))[0]
    kw = float(loop.wind_mw[b]) * 1e3 if getattr(loop, "sized", False) else float(loop.da.wind[1])
    return orc.wind_pem_da(T, cf, da, rt, wind_kw=kw)[0]


def ruc_walk(loop, days, plants=None, tol=1e-9):
    """Steps `loop` (ruc_hour=H, at hour 0 of day 0) through `days` days and checks, for the plants of `plants` (None: all), the chain
    and the bid of every day, and the pending / current hand-over.  -> dict of what was seen (for the non-vacuity assertions)"""
    B, S, D, N, H = loop.B, loop.S, loop.D, loop.N, loop.ruc_hour
    plants = list(range(B)) if plants is None else [int(b) for b in plants]
    Tda, Ttr, ns = loop.da.T, loop.tr.T, len(loop.scale)
    num = lambda t: t.cpu().numpy().copy()
    da_s, rt_s, start = num(loop.da_series), num(loop.rt_series), num(loop.start)
    cf_s = num(loop.cf_series) if loop.cf_series is not None else None
    pda = num(loop.da.pda_cols)
    scale = np.array(loop.scale)
    seen = dict(worst=0.0, lps=0, curves=0, all_optimal=True, projected_moves=set(), rt_lag_differs=0, midnight_windows=0, free_rows=0)
    assert loop.hour == 0

    def gap(got, ref, what):
        g = abs(got - ref) / max(1.0, abs(ref))
        seen["worst"] = max(seen["worst"], g)
        seen["lps"] += 1
        assert g <= tol, (loop.flowsheet, what, got, ref, g)

    def scen(series, b, day, T):
        if loop.forecaster == "perfect":
            return series[(start[b] + 24 * (day + 1) + np.arange(T)) % N][None, :] if series is not None else None
        return host_backcast(series, int(start[b]), day, 0, T, S, D)

    pending = None
    for d in range(days):
        offer_today = num(loop.day_ahead())
        if pending is not None:                      # midnight: yesterday's pending bid IS today's
            for name, was in pending.items():
                assert np.array_equal(num(getattr(loop, name.replace("pend_", "da_"))), was), (d, name)
        assert np.array_equal(offer_today, num(loop.da_offer))
        for h in range(24):
            if h != H:
                loop.hour_step()
                continue
            state_at, prices_today = num(loop.state), num(loop.da_prices)
            current = {n: num(getattr(loop, n)) for n in (("da_curve", "da_count") if loop.stochastic else ())}
            loop.hour_step()
            assert np.array_equal(num(loop.da_offer), offer_today) and np.array_equal(num(loop.da_prices), prices_today), d
            for n, was in current.items():
                assert np.array_equal(num(getattr(loop, n)), was), (d, n)
            # ---- the projection chain, teacher-forced from the trace ----
            ps, pr, po = num(loop.proj_state), num(loop.proj_real), num(loop.proj_obj)
            assert ps.shape == (24 - H + 1, B, ns) and pr.shape == (24 - H, B, ns) and po.shape == (24 - H, B)
            if ns:
                assert np.array_equal(ps[0], state_at)
                assert np.array_equal(ps[1:], np.round(pr * scale) / scale)
                for b in plants:
                    for j in range(24 - H):
                        known = min(Ttr, 24 - H - j)
                        idx = (start[b] + 24 * d + H + j + np.arange(Ttr)) % N
                        P = projection_lp(loop, b, cf_s[idx] if cf_s is not None else None, offer_today[b, H + j:H + j + known], ps[j, b])
                        gap(po[j, b], P.solve(tight=True)[1], ("project", d, b, j))
                        seen["midnight_windows"] += known < Ttr
                        seen["free_rows"] += Ttr - known
                    if not np.array_equal(ps[-1, b], ps[0, b]):
                        seen["projected_moves"].add(b)
                seen["all_optimal"] &= not num(loop.pj.out["status"]).any()
            # ---- the bid for day d + 1 ----
            x, st = num(loop.da.out["x"]), num(loop.da.out["status"])
            obj = num(loop.da.out["obj"]) + num(loop.da.c0)
            seen["all_optimal"] &= not st.any()
            pend = {n: num(getattr(loop, n)) for n in ("pend_offer", "pend_prices") + (("pend_curve", "pend_count") if loop.stochastic else ())}
            for b in plants:
                idx = (start[b] + 24 * (d + 1) + np.arange(Tda)) % N
                da_f, rt_f = scen(da_s, b, d + 1 if loop.forecaster == "backcast" else d, Tda), scen(rt_s, b, d, Tda)
                if loop.forecaster == "backcast":
                    seen["rt_lag_differs"] += int((rt_f != host_backcast(rt_s, int(start[b]), d + 1, 0, Tda, S, D)).sum())
                assert np.array_equal(pend["pend_prices"][b], da_s[idx][:24])
                state = ps[-1, b] if ns else np.zeros(0)
                for i in range(S):
                    P = day_ahead_lp(loop, b, cf_s[idx] if cf_s is not None else None, da_f[i], rt_f[i], state)
                    gap(obj[b * S + i], P.solve(tight=True)[1], ("bid", d, b, i))
                if loop.stochastic:
                    for t in range(24):
                        rows = slice(b * S, (b + 1) * S)
                        U, M = reference_curve(x[rows, pda[t]], da_f[:, t], st[rows] == 0, loop.p_min_cents)
                        assert (U, M) == curve_of(pend["pend_curve"][b, t], pend["pend_count"][b, t]), (d, b, t)
                        assert clear(U, M, da_s[idx][t], loop.market) == float(pend["pend_offer"][b, t]), (d, b, t)
                        seen["curves"] += 1
                else:
                    assert np.array_equal(pend["pend_offer"][b], x[b, pda[:24]])
            pending = pend
        loop._warm = True                              # (as run_day: later days replay from graphs where the loop uses them)
    return seen
