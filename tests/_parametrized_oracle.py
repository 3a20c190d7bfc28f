"""Plain-Python statement of the parametrized mode of dispatches_amd/rolling_flowsheets.py::BatchedDoubleLoop (bidder="parametrized") and
a teacher-forced walk that checks a running loop against it, shared by the CPU and the GPU tests: every curve against the host
bidders (workflow/parametrized_bidder.py on a PerfectForecaster over the plant's own window), every clearing against
clear_price_taker, every tracking LP against the oracle's own LP (oracle/dispatch_lp_oracle.py, HiGHS) of the loop's state and
dispatch, and state hand-off, revenue and hydrogen recomputed from the tracker solutions."""
import numpy as np
import pandas as pd

from tests._flowsheet_stochastic_oracle import clear, curve_of, reference_curve


def host_bidder(loop, b):
    """the reference-shaped host bidder of plant b on a PerfectForecaster whose DataFrame is the plant's own year: row 0 is hour
    start[b] of the circular series"""
    from dispatches_amd.workflow import PerfectForecaster
    from dispatches_amd.workflow.parametrized_bidder import FixedParametrizedBidder, PEMParametrizedBidder
    mo = loop.bidder.bidding_model_object
    gen = mo.model_data.gen_name
    start = int(loop.start[b].item())
    roll = lambda t: np.roll(t.cpu().numpy(), -start)
    df = pd.DataFrame({f"{gen}-DACF": roll(loop.da_cf_series), f"{gen}-RTCF": roll(loop.cf_series)},
                      index=pd.date_range("2020-01-01", periods=loop.N, freq="h"))
    cls, kw = ((PEMParametrizedBidder, dict(pem_marginal_cost=float(loop.bid_price[b].item()), pem_mw=float(loop.storage_mw[b].item())))
               if loop.flowsheet == "wind_pem" else
               (FixedParametrizedBidder, dict(storage_marginal_cost=float(loop.bid_price[b].item()), storage_mw=float(loop.storage_mw[b].item()))))
    return cls(bidding_model_object=mo, day_ahead_horizon=24, real_time_horizon=loop.tr.T, solver=None, forecaster=PerfectForecaster(df), **kw), gen


def host_curve(bidder, p_cost, cf):
    """(U cents, M cents) of ONE host bid.  `p_cost` is what the host bidder hands to the market: costs, in which a tier of zero width
    has lost its price.  So the bid is first tied to the bidder's own tiers (p_cost == convert_marginal_costs_to_actual_costs(tiers),
    exactly), then the tiers' powers and marginal costs are rounded to cents and duplicate powers merged by the curve rule (the highest
    price per distinct power, running maximum), written here from the rule - not through workflow/market.py."""
    from dispatches_amd.workflow.utils import convert_marginal_costs_to_actual_costs
    tiers, p_max = bidder._tiers(cf * bidder.wind_mw)
    assert list(p_cost) == convert_marginal_costs_to_actual_costs(tiers)
    U, M = reference_curve([p for p, _ in tiers], [c for _, c in tiers], [True] * len(tiers), 0)
    assert U[-1] == int(round(round(float(p_max), 2) * 100))
    return U, M


def cost_pairs(U, M):
    from dispatches_amd.workflow.utils import convert_marginal_costs_to_actual_costs
    return convert_marginal_costs_to_actual_costs([(u / 100.0, m / 100.0) for u, m in zip(U, M)])


def _tracking_lp(loop):
    from oracle import dispatch_lp_oracle as orc
    kw = loop.tr.wind[1]
    if loop.flowsheet == "wind_pem":
        return lambda T, cf, disp, st: orc.wind_pem_track(T, cf, disp, wind_kw=kw)[0]
    return lambda T, cf, disp, st: orc.wind_battery_track(T, cf, disp, wind_kw=kw, soc0=float(st[0]), e0=float(st[1]))[0]


def parametrized_walk(loop, days, tol=1e-6, bidders=True):
    """Steps `loop` (at hour 0 of a day) through `days` days with day_ahead() / hour_step() and checks every step.
    -> dict of what was seen (for the non-vacuity assertions)."""
    from dispatches_amd.flowsheets.wind_pem import MultiPeriodWindPEM
    tr_lp = _tracking_lp(loop)
    B, N, Ttr = loop.B, loop.N, loop.tr.T
    num = lambda t: t.cpu().numpy().copy()
    da_s, rt_s, cf_s, dacf_s = num(loop.da_series), num(loop.rt_series), num(loop.cf_series), num(loop.da_cf_series)
    start = num(loop.start)
    tr_PT, tr_const = num(loop.tr.PT), num(loop.tr.PT_const)
    scale = list(loop.scale)
    hosts = [host_bidder(loop, b) for b in range(B)] if bidders else None
    seen = dict(worst=0.0, lps=0, curves=0, below=0, equal=0, points={1: 0, 2: 0, 3: 0}, ties=0, all_optimal=True, dacf_differs=0)
    revenue, energy, state = num(loop.revenue), num(loop.energy_mwh), num(loop.state)
    h2 = num(loop.h2_kg) if loop.h2_kg is not None else None
    da_energy, offered = num(loop.da_energy_mwh), num(loop.offered_mwh)
    hour_abs = loop.hour
    assert hour_abs % 24 == 0

    def check_curve(b, cf, lmp, curve, count, dispatch, bid, what):
        U, M = curve_of(curve, count)
        if bid is not None:
            hu, hm = host_curve(hosts[b][0], bid[hosts[b][1]]["p_cost"], cf)
            assert (hu, hm) == (U, M) and cost_pairs(hu, hm) == cost_pairs(U, M), (what, b, hu, hm, U, M)
        want = clear(U, M, lmp, loop.market)
        assert want == float(dispatch), (what, b, want, float(dispatch))
        seen["curves"] += 1
        seen["points"][len(U)] += 1
        seen["ties"] += any(m == int(round(round(float(lmp), 2) * 100)) and m > 0 for m in M)      # the bid equals the price to the cent
        seen["below" if want < U[-1] / 100.0 else "equal"] += 1

    for _ in range(days):
        date = pd.Timestamp("2020-01-01") + pd.Timedelta(hours=hour_abs)
        loop.day_ahead()
        offer, da_prices = num(loop.da_offer), num(loop.da_prices)
        curve, count = num(loop.da_curve), num(loop.da_count)
        for b in range(B):
            idx = (start[b] + hour_abs + np.arange(24)) % N
            assert np.array_equal(da_prices[b], da_s[idx])
            seen["dacf_differs"] += int((dacf_s[idx] != cf_s[idx]).sum())
            bids = hosts[b][0].compute_day_ahead_bids(date, 0) if bidders else None
            for t in range(24):
                check_curve(b, dacf_s[idx][t], da_s[idx][t], curve[b, t], count[b, t], offer[b, t], bids[t] if bidders else None, "da")
            da_energy[b] += offer[b].sum()
            offered[b] += sum(curve[b, t, count[b, t] - 1, 0] / 100.0 for t in range(24))
        for h in range(24):
            state0 = state.copy()
            assert np.array_equal(num(loop.state), state0)
            loop.hour_step()
            x_tr = num(loop.tr.out["x"])
            obj_tr = num(loop.tr.out["obj"]) + num(loop.tr.c0)
            seen["all_optimal"] &= not num(loop.tr.out["status"]).any()
            curve, count, dispatch = num(loop.rt_curve), num(loop.rt_count), num(loop.rt_dispatch)
            delivered = num(loop.delivered)
            for b in range(B):
                idx = (start[b] + hour_abs + np.arange(Ttr)) % N
                bids = hosts[b][0].compute_real_time_bids(date, h, None, None) if bidders else None
                for t in range(Ttr):
                    check_curve(b, cf_s[idx][t], rt_s[idx][t], curve[b, t], count[b, t], dispatch[b, t], bids[t + h] if bidders else None, ("rt", h))
                ref = tr_lp(Ttr, cf_s[idx], dispatch[b], state0[b]).solve(tight=True)[1]
                g = abs(obj_tr[b] - ref) / max(1.0, abs(ref))
                seen["worst"], seen["lps"] = max(seen["worst"], g), seen["lps"] + 1
                assert g <= tol, (loop.flowsheet, "track", b, h, obj_tr[b], ref, g)
                got = float(x_tr[b] @ tr_PT[0] + tr_const[0])
                assert abs(got - delivered[b]) <= 1e-9 * max(1.0, abs(got))
                for j, col in enumerate(loop.tr.state_real):                  # update_model: the realised state, rounded
                    state[b, j] = round(x_tr[b, col] * scale[j]) / scale[j]
                revenue[b] += delivered[b] * rt_s[idx][0] + offer[b, h] * (da_prices[b, h] - rt_s[idx][0])
                energy[b] += delivered[b]
                if h2 is not None:
                    h2[b] += MultiPeriodWindPEM._h2_kg_per_hr(x_tr[b, loop.pem_col])
            hour_abs += 1
        loop._warm = True                              # (as run_day: later days replay from graphs where the loop uses them)
    res, _ = loop.results()
    np.testing.assert_allclose(num(res["obj"]), revenue, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(num(res["energy_mwh"]), energy, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(num(res["da_energy_mwh"]), da_energy, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(num(res["offered_mwh"]), offered, rtol=1e-12, atol=1e-9)
    assert np.array_equal(num(res["state"]), state)
    if h2 is not None:
        np.testing.assert_allclose(num(res["h2_kg"]), h2, rtol=1e-12, atol=1e-9)
        seen["h2_kg"] = float(h2.sum())
    return seen
