"""Shared by the tests of the stochastic double loop (tests/test_market_cpu.py, test_rolling_stochastic_cpu.py - HiGHS stand-in backend - and
test_hip_rolling_stochastic.py - GPU): what the loop must compute, restated without any of its code paths.

* `host_backcast`      the price scenarios a host `Backcaster` returns when its history is the D whole days before a simulated day
* `reference_curve`    a bid curve in plain Python from Python's own round(v, 2) (the arithmetic of Bidder._assemble_bids with p_min = 0);
                       `numpy_path_agrees` ties it to workflow/bid_curves.py (cents / sorted_pairs / curves)
* `check_recorded`     teacher-forced check of a recorded trajectory: every LP against the ORACLE's own LP of the recorded state and
                       that scenario's prices (oracle/double_loop_oracle.py -> dispatch_lp_oracle.py; the product's formulation does
                       not enter), curves and dispatches recomputed from the recorded solutions, revenue re-added."""
import math

import numpy as np

BUS = "bus"


def host_backcast(series, start, day, hour, horizon, S, D):
    """[S, horizon]: forecast of a host Backcaster whose history is days day - D .. day - 1 of the circular series that starts at `start`"""
    from dispatches_amd.workflow.forecaster import Backcaster
    N = len(series)
    hist = series[(start + 24 * (day - D) + np.arange(24 * D)) % N]
    bc = Backcaster({BUS: list(hist)}, {BUS: list(hist)}, max_historical_days=D)
    da = bc.forecast_day_ahead_prices(None, hour, BUS, horizon, S)
    rt = bc.forecast_real_time_prices(None, hour, BUS, horizon, S)
    assert da == rt                                             # (one history here: both markets follow the same rule)
    return np.array([da[i] for i in range(S)])


def reference_curve(power, price, ok):
    """(U cents, M cents) integer lists of the curve of ONE (plant, period) from its S pairs"""
    best = {}
    for p, c, o in zip(power, price, ok):
        if not o or not (math.isfinite(p) and math.isfinite(c)):
            continue
        p2, c2 = round(float(p), 2), round(float(c), 2)
        if p2 < 0:
            continue
        p2 += 0.0                                               # (-0.0 is the point at 0)
        best[p2] = max(best.get(p2, -math.inf), c2)
    U = sorted(best)
    M = [best[u] for u in U]
    if 0.0 not in best:
        M.insert(0, min(M) if M else 0.0)
        U.insert(0, 0.0)
    M = list(np.maximum.accumulate(M))
    return [int(round(u * 100)) for u in U], [int(round(m * 100)) for m in M]


def numpy_path_agrees(power, price, ok, U, M):
    """the same curve through workflow/bid_curves.py: distinct points of sorted_pairs, then curves() - its powers are U and its costs
    the integral of M over U, bit for bit"""
    import torch
    from dispatches_amd.workflow import bid_curves as bc
    ps, cs, first = bc.sorted_pairs(torch, torch.as_tensor(np.asarray(power, float)).reshape(-1, 1),
                                    torch.as_tensor(np.asarray(price, float)).reshape(-1, 1), 0.0, ok=torch.as_tensor(np.asarray(ok, bool)))
    f = first[:, 0].numpy()
    pts = [(ps[:, 0].numpy()[f] / 100.0, cs[:, 0].numpy()[f] / 100.0)]
    counts, Up, Mp = bc.padded(pts, width=len(power))
    n, Uc, cost = bc.curves(counts, Up, Mp, 0.0, 0.0)
    u, m = np.array(U) / 100.0, np.array(M) / 100.0
    want = np.empty(len(u))
    want[0] = u[0] * m[0]
    if len(u) > 1:
        want[1:] = want[0] + np.cumsum(np.diff(u) * m[1:])
    return int(n[0]) == len(U) and np.array_equal(Uc[0, :len(U)], u) and np.array_equal(cost[0, :len(U)], want)


def curve_of(curve, count):
    """recorded [S + 1, 2] int32 + count -> (U, M) integer lists; unused slots must be zero"""
    c = int(count)
    assert not curve[c:].any()
    return curve[:c, 0].tolist(), curve[:c, 1].tolist()


def clear(U, M, lmp, market):
    from dispatches_amd.workflow.market import clear_price_taker
    u, m = np.array(U) / 100.0, np.array(M) / 100.0
    return clear_price_taker(u, m, lmp) if market == "price_taker" else float(u[-1])


def check_recorded(loop_args, maps, rec, revenue, stride=17, first_scenario=0):
    """rec: BatchedWindBatteryDoubleLoop.recorded() of a stochastic loop (S, D, forecaster, market in loop_args); revenue: the loop's
    accumulated revenue of the recorded plants after the recorded hours.  -> dict of what was seen (for the non-vacuity assertions)."""
    from oracle import double_loop_oracle as dl
    from tests._rolling_oracle import _feasible_and_optimal, _mapped
    S, D, forecaster, market = (loop_args[k] for k in ("S", "D", "forecaster", "market"))
    da_s, rt_s, cf_s = dl.load_year()
    N = len(rt_s)
    T, Tda = maps["rt"].shape[0], maps["da"].shape[0]
    Ttr = maps["tr"].shape[0]
    pt = lambda cols, x: 1e-3 * (x[cols[:, 1]] + x[cols[:, 3]])
    seen = dict(lps=0, forecast_differs=0, forecast_hours=0, below=0, equal=0, worst=0.0, curves=0)

    def scenarios_at(series, start, i_hour, horizon):
        d, h = divmod(i_hour, 24)
        if forecaster == "perfect":
            return dl.window(series, start, i_hour, horizon)[None, :]
        return host_backcast(series, start, d, h, horizon, S, D)

    H, n_days = rec["state"].shape[0], rec["da_obj"].shape[0]
    for p, plant in enumerate(rec["plants"]):
        k = first_scenario + int(plant)
        start = (stride * k) % N
        total = 0.0
        for d in range(n_days):
            da_f, rt_f = scenarios_at(da_s, start, 24 * d, Tda), scenarios_at(rt_s, start, 24 * d, Tda)
            cf = dl.window(cf_s, start, 24 * d, Tda)
            realised = dl.window(da_s, start, 24 * d, 24)
            seen["forecast_differs"] += int((da_f[:, :24] != realised[None, :]).sum())
            seen["forecast_hours"] += da_f[:, :24].size
            soc, thr = rec["da_state"][d, p]
            assert (rec["da_state"][d, p] == rec["state"][24 * d, p]).all()
            for i in range(S):
                x = rec["da_x"][d, p, i]
                P, fs, pda, u = dl.day_ahead_lp(cf, da_f[i], rt_f[i], float(soc), float(thr))
                extra = [(pda[t], x[maps["da_pda"]][t]) for t in range(Tda)] + [(u[t], x[maps["da_u"]][t]) for t in range(Tda)]
                seen["worst"] = max(seen["worst"], _feasible_and_optimal(P, _mapped(P, fs, maps["da"], x, extra), ("da", k, d, i)))
                seen["lps"] += 1
            for t in range(24):
                power = rec["da_x"][d, p, :, maps["da_pda"][t]]
                U, M = reference_curve(power, da_f[:, t], [True] * S)
                assert (U, M) == curve_of(rec["da_curve"][d, p, t], rec["da_count"][d, p, t]), ("day-ahead curve", k, d, t)
                assert numpy_path_agrees(power, da_f[:, t], [True] * S, U, M)
                want = clear(U, M, realised[t], market)
                assert rec["da_dispatch"][d, p, t] == want, ("day-ahead dispatch", k, d, t)
                seen["below"] += want < U[-1] / 100.0
                seen["equal"] += want == U[-1] / 100.0
                seen["curves"] += 1
        for i_hour in range(H):
            d, h = divmod(i_hour, 24)
            offer, prices = rec["da_dispatch"][d, p], dl.window(da_s, start, 24 * d, 24)
            soc, thr = (float(v) for v in rec["state"][i_hour, p])
            if i_hour > 0:
                prev = rec["tr_x"][i_hour - 1, p]
                for got, col in ((soc, 4), (thr, 5)):
                    real = float(prev[maps["tr"][0, col]])
                    assert abs(got - real) <= 0.005 + 1e-9 * max(1.0, abs(real)), ("state hand-off", k, i_hour)
            rt_f, da_f = scenarios_at(rt_s, start, i_hour, T), scenarios_at(da_s, start, i_hour, T)
            rt_real, cf = dl.window(rt_s, start, i_hour, T), dl.window(cf_s, start, i_hour, T)
            known = min(T, 24 - h)
            cleared = np.zeros(T)
            cleared[:known] = offer[h:h + known]
            powers = np.zeros((S, T))
            for i in range(S):
                daw = da_f[i].copy()
                daw[:known] = prices[h:h + known]
                x = rec["rt_x"][i_hour, p, i]
                P, fs, u, pda = dl.real_time_lp(cf, rt_f[i], daw, cleared, known, soc, thr)
                xp, xu = x[maps["rt_pda"]], x[maps["rt_u"]]
                assert np.abs(xp[:known] - cleared[:known]).max() <= 1e-9 * 225, ("cleared day-ahead position", k, i_hour, i)
                extra = [(u[t], xu[t]) for t in range(T)] + [(pda[t], xp[t]) for t in range(known, T)]
                seen["worst"] = max(seen["worst"], _feasible_and_optimal(P, _mapped(P, fs, maps["rt"], x, extra), ("rt", k, i_hour, i)))
                seen["lps"] += 1
                powers[i] = pt(maps["rt"], x)
            dispatch = rec["rt_dispatch"][i_hour, p]
            for t in range(Ttr):
                U, M = reference_curve(powers[:, t], rt_f[:, t], [True] * S)
                assert (U, M) == curve_of(rec["rt_curve"][i_hour, p, t], rec["rt_count"][i_hour, p, t]), ("real-time curve", k, i_hour, t)
                lmp = rt_real[0] if t == 0 else rt_f[0, t]
                assert dispatch[t] == clear(U, M, lmp, market), ("real-time dispatch", k, i_hour, t)
                seen["curves"] += 1
            x = rec["tr_x"][i_hour, p]
            P, fs, under, over = dl.tracking_lp(cf[:Ttr], dispatch, soc, thr)
            ptt = pt(maps["tr"], x)
            extra = [(under[t], max(0.0, dispatch[t] - ptt[t])) for t in range(Ttr)] + [(over[t], max(0.0, ptt[t] - dispatch[t])) for t in range(Ttr)]
            seen["worst"] = max(seen["worst"], _feasible_and_optimal(P, _mapped(P, fs, maps["tr"], x, extra), ("tr", k, i_hour)))
            seen["lps"] += 1
            total += ptt[0] * rt_real[0] + offer[h] * (prices[h] - rt_real[0])
        assert abs(total - revenue[p]) <= 1e-9 * max(1.0, abs(total)), ("revenue", k, total, revenue[p])
    return seen
