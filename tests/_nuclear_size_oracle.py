"""Teacher-forced walk of a nuclear BatchedDoubleLoop whose plants have their OWN pem_mw / tank_kg / h2_price / h2_demand, in the style of
tests/_design_oracle.py: the loop is stepped, and after every step every LP of every plant is rebuilt by the oracle
(oracle.dispatch_lp_oracle.nuclear_da / _rt / _track, HiGHS) at that plant's operands and recorded state - every day-ahead row, every
real-time row whose horizon lies inside the cleared day, every tracking LP - and the objectives are compared at the project's parity
contract, 1e-6 relative.  nuclear_rows takes h2_price and h2_demand as arguments and reads the PEM and tank capacities from
module constants at call time: those are set per plant through `monkeypatch` (oracle/ stays untouched).  Curves and dispatches are
recomputed exactly, in integer cents, with that plant's p_min = 500 MW - pem_mw.  Works on the stochastic loop (curves, price taker or
stub) and on the deterministic one (the offer is the dispatch).  An unsized loop walks with the flowsheet's defaults."""
import numpy as np

from tests._flowsheet_stochastic_oracle import _power, clear, curve_of, reference_curve
from tests._stochastic_oracle import host_backcast

DEFAULTS = dict(pem_mw=100.0, tank_kg=5000.0, h2_price=4.0, h2_demand=0.35)


def operands(loop, b):
    return {k: float(getattr(loop, k)[b]) if getattr(loop, "nuclear_sized", False) else v for k, v in DEFAULTS.items()}


def nuclear_walk(loop, days, monkeypatch, tol=1e-6):
    """-> dict(worst, lps, curves, all_optimal, lowest_offer_mw per plant, trace per plant: every objective, curve and dispatch in order)"""
    from oracle import dispatch_lp_oracle as orc
    B, S, D, N = loop.B, loop.S, loop.D, loop.N
    Tda, Trt, Ttr = loop.da.T, loop.rt.T, loop.tr.T
    num = lambda t: t.cpu().numpy().copy()
    da_s, rt_s, start = num(loop.da_series), num(loop.rt_series), num(loop.start)
    ops = [operands(loop, b) for b in range(B)]
    pmin = [int(round((500.0 - o["pem_mw"]) * 100.0)) for o in ops]
    rt_terms, rt_const = loop.rt.terms(), num(loop.rt.PT_const)
    rt_PT = num(loop.rt.PT)
    pda = num(loop.da.pda_cols)
    seen = dict(worst=0.0, lps=0, curves=0, all_optimal=True, lowest_offer_mw={b: np.inf for b in range(B)}, trace={b: [] for b in range(B)})

    def lp(fn, b, *args, holdup0):
        monkeypatch.setattr(orc, "PEM_CAPACITY_KW", ops[b]["pem_mw"] * 1e3)
        monkeypatch.setattr(orc, "TANK_CAPACITY_KG", ops[b]["tank_kg"])
        return fn(*args, holdup0=holdup0, h2_price=ops[b]["h2_price"], h2_demand=ops[b]["h2_demand"])[0].solve(tight=True)[1]

    def scen(series, b, hour_abs, T):
        d, h = divmod(hour_abs, 24)
        if loop.forecaster == "perfect":
            return series[(start[b] + hour_abs + np.arange(T)) % N][None, :]
        return host_backcast(series, int(start[b]), d, h, T, S, D)

    def gap(b, got, ref, what):
        g = abs(got - ref) / max(1.0, abs(ref))
        seen["worst"] = max(seen["worst"], g)
        seen["lps"] += 1
        seen["trace"][b].append(("obj", what, float(got)))
        assert g <= tol, (what, b, got, ref, g)

    def check_curve(b, t, powers, prices, ok, lmp, curve, count, dispatch, what):
        U, M = reference_curve(powers, prices, ok, pmin[b])
        assert (U, M) == curve_of(curve, count), (what, b, t, U, M, curve.tolist(), int(count))
        want = clear(U, M, lmp, loop.market)
        assert want == float(dispatch), (what, b, t, want, float(dispatch))
        seen["curves"] += 1
        seen["lowest_offer_mw"][b] = min(seen["lowest_offer_mw"][b], U[0] / 100.0)
        seen["trace"][b].append(("curve", what, t, tuple(U), tuple(M), int(round(float(dispatch) * 100.0))))

    hour_abs = loop.hour
    assert hour_abs % 24 == 0
    for _ in range(days):
        state0 = num(loop.state)
        loop.day_ahead()
        x, st = num(loop.da.out["x"]), num(loop.da.out["status"])
        obj = num(loop.da.out["obj"]) + num(loop.da.c0)
        seen["all_optimal"] &= not st.any()
        offer, da_prices = num(loop.da_offer), num(loop.da_prices)
        for b in range(B):
            idx = (start[b] + hour_abs + np.arange(Tda)) % N
            da_f, rt_f = scen(da_s, b, hour_abs, Tda), scen(rt_s, b, hour_abs, Tda)
            for i in range(S):
                gap(b, obj[b * S + i], lp(orc.nuclear_da, b, Tda, da_f[i], rt_f[i], holdup0=float(state0[b, 0])), ("da", i))
            if loop.stochastic:
                curve, count = num(loop.da_curve), num(loop.da_count)
                rows = slice(b * S, (b + 1) * S)
                for t in range(24):
                    check_curve(b, t, x[rows, pda[t]], da_f[:, t], st[rows] == 0, da_s[idx][t], curve[b, t], count[b, t], offer[b, t], "da")
        for h in range(24):
            state0 = num(loop.state)
            loop.hour_step()
            x, st = num(loop.rt.out["x"]), num(loop.rt.out["status"])
            obj = num(loop.rt.out["obj"]) + num(loop.rt.c0)
            obj_tr = num(loop.tr.out["obj"]) + num(loop.tr.c0)
            seen["all_optimal"] &= not st.any() and not num(loop.tr.out["status"]).any()
            for b in range(B):
                idx = (start[b] + hour_abs + np.arange(Trt)) % N
                rt_f = scen(rt_s, b, hour_abs, Trt)
                if h + Trt <= 24:                        # the oracle's real-time LP fixes every hour of its horizon: hours inside the cleared day
                    cleared = offer[b, h:h + Trt]
                    for i in range(S):
                        # (the product keeps day_ahead_power as a fixed column: its objective carries - DA . cleared, the oracle's form does not)
                        ref = lp(orc.nuclear_rt, b, Trt, rt_f[i], cleared, holdup0=float(state0[b, 0])) - float(da_prices[b, h:h + Trt] @ cleared)
                        gap(b, obj[b * S + i], ref, ("rt", h, i))
                if loop.stochastic:
                    curve, count, dispatch = num(loop.rt_curve), num(loop.rt_count), num(loop.rt_dispatch)
                    for t in range(Ttr):
                        powers = [_power(rt_terms, rt_const, x[r], t) for r in range(b * S, (b + 1) * S)]
                        lmp = rt_s[idx][0] if t == 0 else rt_f[0, t]
                        check_curve(b, t, powers, rt_f[:, t], st[b * S:(b + 1) * S] == 0, lmp, curve[b, t], count[b, t], dispatch[b, t], ("rt", h))
                    tracked = dispatch[b]
                else:
                    tracked = (x[b] @ rt_PT.T + rt_const)[:Ttr]       # the stub market: the offer is the dispatch
                gap(b, obj_tr[b], lp(orc.nuclear_track, b, Ttr, tracked, holdup0=float(state0[b, 0])), ("track", h))
            hour_abs += 1
        loop._warm = True                                # (as run_day: later days replay from graphs where the loop uses them)
    return seen
