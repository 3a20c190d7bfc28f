"""GPU tests of BatchedDoubleLoop(..., past_midnight="coupled") (csrc/dsp_market.hip: dsp_loop_midnight_prepare; dsp_loop_market_clear on
the coupled real-time rows with k >= 0): the new entry point alone against the tensor form, the kernels against the tensor form over two
days and graph replay against the eager loop bit for bit, the oracle walk on the device, the entry point's refusals, and the default."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
MODES = {"monotone": dict(scenario_coupling="monotone"), "self_schedule": dict(bidder="self_schedule")}


def _loop(flowsheet, B, S, mode, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    args = dict(device=0, n_price_scenarios=S, forecaster="backcast", max_historical_days=3, market="price_taker", day_ahead_horizon=24,
                past_midnight="coupled")
    args.update(MODES[mode])
    args.update(kw)
    if args["past_midnight"] is None:
        del args["past_midnight"]
    return BatchedDoubleLoop(flowsheet, B, **args)


def _snapshot(loop):
    res, ok = loop.results()
    out = {k: v.cpu().numpy().copy() for k, v in res.items()}
    models = [("da", loop.da), ("rt", loop.rt), ("tr", loop.tr)] + ([("rtc", loop.rtc)] if loop.past_midnight == "coupled" else [])
    for name, m in models:
        for key in ("c", "lb", "ub", "rlo", "rhi", "c0"):
            out[name + "_" + key] = getattr(m, key).cpu().numpy().copy()
        out[name + "_status"] = m.out["status"].cpu().numpy().copy()
    for key in ("da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch", "da_offer", "da_prices", "delivered"):
        out[key] = getattr(loop, key).cpu().numpy().copy()
    out["uncertified"] = np.array(int(loop.uncertified.item()))
    return out, ok


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k].astype(float) - b[k].astype(float)).max()))


def _prepare(loop, k):
    m = loop.rtc
    bounds = (C.c_void_p(m.rlo.data_ptr()), C.c_void_p(m.rhi.data_ptr())) if loop.monotone else (None, None)
    loop._call(loop._lib.dsp_loop_midnight_prepare, C.byref(loop._mk_coupled if loop.monotone else loop._mk_sched), C.byref(loop._mk_rtc), *bounds,
               m.lp.m, m.first_coupling_row, k)


@gpu
@pytest.mark.parametrize("mode,flowsheet", [("monotone", "nuclear"), ("self_schedule", "wind_pem")])
def test_the_entry_point_is_the_tensor_form_bit_for_bit(mode, flowsheet):
    """B = 4, S = 3, no solve: dsp_loop_midnight_prepare against BatchedDoubleLoop._tied_blocks from sentinel-filled buffers, at the first
    late hour of a day and at hour 23 of day 2, on a cleared offer, realised prices and a state set by hand - c, lb, ub, rlo, rhi, c0
    bit for bit.  Monotone: every pair row of all T periods is written, each of -inf, 0 and +inf occurs, no block row is touched.
    Self-schedule (NULL rlo): no row bound is touched."""
    import torch
    B, S = 4, 3
    for k_of in (lambda T: 24 - T + 1, lambda T: 23):
        got = {}
        for fused in (False, True):
            loop = _loop(flowsheet, B, S, mode, use_fused=fused, use_graphs=False)
            m, T = loop.rtc, loop.rt.T
            k = k_of(T)
            grid = torch.arange(B * 24, dtype=torch.float64, device=loop.dev).view(B, 24)
            loop.da_offer.copy_(400.0 + 0.37 * grid)
            loop.da_prices.copy_(11.0 + 0.53 * grid)
            if loop.state.shape[1]:
                loop.state.copy_(torch.tensor([[3.0 * b + 1.0] * loop.state.shape[1] for b in range(B)], dtype=torch.float64, device=loop.dev))
            loop.hour_t.fill_(48 + k)
            for t in (m.c, m.lb, m.ub, m.rlo, m.rhi, m.c0):
                t.fill_(-7.0)
            if fused:
                _prepare(loop, k)
            else:
                loop._tied_blocks(k)
            torch.cuda.synchronize()
            got[fused] = {key: getattr(m, key).cpu().numpy().copy() for key in ("c", "lb", "ub", "rlo", "rhi", "c0")}
        first, pda = m.first_coupling_row, loop.rt.pda_cols.cpu().numpy()
        known = 24 - k
        ours = got[True]
        assert not (ours["c0"] == -7.0).any() and (ours["rlo"][:, :first] == -7.0).all() and (ours["rhi"][:, :first] == -7.0).all()
        lb, ub = ours["lb"].reshape(B, S, -1)[:, :, pda], ours["ub"].reshape(B, S, -1)[:, :, pda]
        assert (lb[:, :, :known] == ub[:, :, :known]).all() and (lb[:, :, known:] == 0).all() and np.isinf(ub[:, :, known:]).all()
        assert (lb[:, :, 0] == loop.da_offer[:, k].cpu().numpy()[:, None]).all()
        pair = np.concatenate([ours["rlo"][:, first:], ours["rhi"][:, first:]], axis=1)
        if mode == "monotone":
            assert pair.shape[1] == 2 * 3 * T and not (pair == -7.0).any()
            assert (pair == -np.inf).any() and (pair == 0).any() and (pair == np.inf).any()
        else:
            assert (pair == -7.0).all()
        _same(got[False], ours, (mode, flowsheet, k))


@gpu
@pytest.mark.parametrize("mode,flowsheet,B,S", [("monotone", "nuclear", 4, 3), ("monotone", "wind_battery", 6, 2), ("self_schedule", "nuclear", 4, 3)])
def test_kernels_are_the_tensor_form_bit_for_bit(mode, flowsheet, B, S):
    """use_fused True against False over two days, eager: the coupled real-time rows, the other three LPs, curves, counts, offers,
    dispatches, state, revenue, energy.  Every late-hour real-time solve and every tracking solve ends with status 0; both runs go
    through the same solver and agree on every status (wind + battery's day-ahead solve: as the monotone mode's own GPU tests - its
    iteration-limit plants are the day-ahead LP's matter, the two runs must agree on them)."""
    runs, oks = {}, {}
    for fused in (False, True):
        loop = _loop(flowsheet, B, S, mode, use_fused=fused, use_graphs=False, health=True)
        assert loop.use_fused == fused and loop.rtc.c.shape == (B, S * loop.rt.lp.n)
        T = loop.rt.T
        for day in range(2):
            loop.day_ahead()
            for k in range(24):
                loop.hour_step()
                if 24 - k < T:
                    assert not loop.rtc.out["status"].any().item() and not loop.tr.out["status"].any().item(), (day, k)
        assert not loop.rtc.dlp.last_stats.streaming and int(loop.hour_t.item()) == 48
        runs[fused], oks[fused] = _snapshot(loop)
        per = 1 if mode == "self_schedule" else S
        assert loop.health_solves[1].tolist() == [2 * ((24 - (T - 1)) * per + T - 1)] * B and not loop.health_fail[1:3].any().item()
        assert loop.solves == 2 * (B + (24 - (T - 1)) * (B * per + B) + (T - 1) * 2 * B)
    assert oks[False] == oks[True] and (flowsheet == "wind_battery" or oks[True])
    _same(runs[False], runs[True], (mode, flowsheet, B, S))


@gpu
@pytest.mark.parametrize("mode,flowsheet,B,S", [("monotone", "nuclear", 4, 3), ("monotone", "wind_battery", 6, 2)])
def test_oracle_walk_on_the_device(mode, flowsheet, B, S):
    """two days with kernels and graphs (the second day's steps replay; the late hours' steps are captured per k like the others)
    against the oracle's own LPs at 1e-6, the project's device parity bar: curves and dispatches exact from the read-back solutions,
    every late-hour solve optimal, the coupled solutions inside their rows to 1e-6 MW"""
    from tests._past_midnight_oracle import oracle_walk
    loop = _loop(flowsheet, B, S, mode)
    assert loop.use_fused and loop.use_graphs
    seen = oracle_walk(loop, 2, tol=1e-6)
    print("past midnight", mode, flowsheet, "worst relative gap", seen["worst"], "over", seen["lps"], "LPs; late margins",
          sorted(e[3] for e in seen["late"])[-3:], "iterations", loop.rtc.out["iters"].cpu().tolist())
    assert not loop.rtc.dlp.last_stats.streaming and len(loop._graphs) == 25
    assert seen["worst"] <= 1e-6 and all(not s.any() for s in seen["late_status"])
    assert max(e[5] for e in seen["late"]) <= 1e-6 and int(loop.uncertified.item()) == 0
    assert flowsheet == "wind_battery" or (seen["all_optimal"] and loop.results()[1])


@gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_graph_replay_is_the_eager_loop_bit_for_bit(mode):
    """three days, nuclear B = 4 x S = 3, with ledger, health, record and profiles: the steps of the third day are replays of graphs
    captured on the second - the day-ahead step, the 13 early hours and the 11 late ones"""
    runs = {}
    for graphs in (False, True):
        loop = _loop("nuclear", 4, 3, mode, use_graphs=graphs, ledger=True, health=True, record=([0, 3], 3), profiles=3)
        for _ in range(3):
            loop.run_day()
        assert int(loop.hour_t.item()) == 72 and len(loop._graphs) == (25 if graphs else 0)
        runs[graphs], ok = _snapshot(loop)
        assert ok
        runs[graphs].update({"rec_" + k: v for k, v in loop.recorded().items()})
        runs[graphs]["profile"] = loop.profile.cpu().numpy().copy()
        runs[graphs]["health_solves"] = loop.health_solves.cpu().numpy().copy()
    _same(runs[False], runs[True], mode)


@gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_simplex_options_ride_along(mode):
    """simplex_warm=False and simplex_certify=True reach the coupled handle too: two days (the second from graphs) end with every solve
    optimal and nothing uncertified; under simplex_certify the coupled model carries its certificates"""
    for kw in (dict(simplex_warm=False), dict(simplex_certify=True)):
        loop = _loop("nuclear", 4, 3, mode, **kw)
        loop.run_day(), loop.run_day()
        assert loop.results()[1] and not loop.rtc.out["status"].any().item() and int(loop.uncertified.item()) == 0
        assert ("kkt" in loop.rtc.out) == bool(kw.get("simplex_certify")) and loop.rtc.opts.simplex_certify == int(bool(kw.get("simplex_certify")))


@gpu
def test_refusals_of_the_entry_point_on_the_host():
    """dsp_loop_midnight_prepare on the descriptors of a real loop (nuclear, B = 3, S = 3) over sentinel-filled buffers: with ONE thing
    broken DSP_ERR_INVALID and nothing written; the unedited call is accepted"""
    import torch
    from dispatches_amd.hip_solver import DspLoopMarketModel, DspLoopMarketState
    loop = _loop("nuclear", 3, 3, "monotone")
    lib, m0, s0, m = loop._lib, loop._mk_rtc, loop._mk_coupled, loop.rtc
    T, rows, first = m0.T, m.lp.m, m.first_coupling_row
    bufs = (m.c, m.lb, m.ub, m.c0, m.rlo, m.rhi)
    stream = C.c_void_p(torch.cuda.current_stream(loop.dev).cuda_stream)

    def call(edit=None, **args):
        for t in bufs:
            t.fill_(-7.0)
        st, md = DspLoopMarketState.from_buffer_copy(s0), DspLoopMarketModel.from_buffer_copy(m0)
        if edit is not None:
            edit(st, md)
        a = dict(rlo=m.rlo.data_ptr(), rhi=m.rhi.data_ptr(), m_rows=rows, first=first, k=23)
        a.update(args)
        rc = lib.dsp_loop_midnight_prepare(C.byref(st), C.byref(md), C.c_void_p(a["rlo"]) if a["rlo"] else None,
                                           C.c_void_p(a["rhi"]) if a["rhi"] else None, a["m_rows"], a["first"], a["k"], stream)
        torch.cuda.synchronize()
        return rc, all(bool((t == -7.0).all()) for t in bufs)

    st_field = lambda name, value: (lambda st, md: setattr(st, name, value))
    m_field = lambda name, value: (lambda st, md: setattr(md, name, value))
    edits = [m_field("c", None), m_field("lb", None), m_field("ub", None), m_field("base_c", None), m_field("c0", None),
             st_field("start", None), st_field("hour", None), st_field("rt_series", None), st_field("state", None),
             st_field("da_offer", None), st_field("da_prices", None), st_field("S", 0), st_field("S", 17), st_field("S", 4),
             m_field("T", 0), m_field("T", 49), m_field("n", 0), m_field("row_stride", 3 * m0.n - 1), m_field("row_stride", 0),
             m_field("wind_kw_plant", m.c0.data_ptr()), st_field("coupled", 2)]
    for q, edit in enumerate(edits):
        rc, untouched = call(edit)
        assert rc == -1 and untouched, q
    for args in (dict(k=-1), dict(k=24), dict(k=24 - T), dict(rlo=None), dict(rhi=None), dict(first=-1), dict(first=first + 1),
                 dict(m_rows=rows - 1)):
        rc, untouched = call(**args)
        assert rc == -1 and untouched, args
    assert lib.dsp_loop_midnight_prepare(None, None, None, None, 0, 0, 23, None) == -1
    rc, untouched = call(k=24 - T + 1)
    assert rc == 0 and not untouched and bool((m.c0 != -7.0).all())
    rc, untouched = call(rlo=None, rhi=None)                             # a self-schedule's call: the blocks, no row bound
    assert rc == 0 and bool((m.rlo == -7.0).all()) and bool((m.c0 != -7.0).all())


@gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_default_is_left_alone(mode):
    """past_midnight="free" against the argument left out - the path of the loop as it was: results(), curves, state and every LP
    buffer bit for bit after two days from graphs, and no coupled real-time model"""
    runs = {}
    for given in ("free", None):
        loop = _loop("nuclear", 16, 3, mode, past_midnight=given)
        assert not hasattr(loop, "rtc") and "past_midnight" not in vars(loop)
        loop.run_day(), loop.run_day()
        assert len(loop._graphs) == 25
        runs[given], ok = _snapshot(loop)
        assert ok
    _same(runs["free"], runs[None], mode)
