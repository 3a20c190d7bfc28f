"""GPU tests of BatchedDoubleLoop(..., bidder="self_schedule") (csrc/dsp_market.hip: dsp_loop_schedule_prepare; dsp_loop_market_clear with
row_stride / self_schedule / curve_slots; ABI 18): the kernels against the tensor form and graph replay against the eager loop bit for
bit, the oracle walk on the device, the new entry point's refusals, the old clearing path with the new fields at 0, and the default
loop left alone."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
FLOWSHEETS = ("wind_battery", "wind_pem", "nuclear")


def _loop(flowsheet, B, S=3, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    args = dict(device=0, bidder="self_schedule", n_price_scenarios=S, forecaster="backcast", max_historical_days=3, market="price_taker",
                day_ahead_horizon=24)
    args.update(kw)
    return BatchedDoubleLoop(flowsheet, B, **args)


def _snapshot(loop):
    res, ok = loop.results()
    out = {k: v.cpu().numpy().copy() for k, v in res.items()}
    for name, m in (("da", loop.da), ("rt", loop.rt), ("tr", loop.tr)):
        for key in ("c", "lb", "ub", "rlo", "rhi", "c0"):
            out[name + "_" + key] = getattr(m, key).cpu().numpy().copy()
    for key in ("da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch", "da_offer", "da_prices", "delivered"):
        out[key] = getattr(loop, key).cpu().numpy().copy()
    out["uncertified"] = np.array(int(loop.uncertified.item()))
    return out, ok


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k].astype(float) - b[k].astype(float)).max()))


@gpu
@pytest.mark.parametrize("B,S", [(90, 3), (5, 2)])
@pytest.mark.parametrize("market", ["price_taker", "stub"])
@pytest.mark.parametrize("flowsheet", FLOWSHEETS)
def test_kernels_are_the_tensor_form_bit_for_bit(flowsheet, market, B, S):
    """use_fused True against False over one day and two hours of the next (the second day-ahead step starts from a realised state):
    c, lb, ub, c0 of the coupled rows, the hourly and the tracker's LPs, curves, counts, offers, dispatches, state, revenue and
    energy.  B = 90 x S = 3: 270 (plant, scenario) lanes cross the 64- and the 256-lane boundaries, blocks S * n1 apart; B = 5 x S = 2:
    an odd, tiny grid."""
    runs = {}
    for fused in (False, True):
        loop = _loop(flowsheet, B, S, market=market, use_fused=fused, use_graphs=False)
        assert loop.use_fused == fused and loop.da.c.shape == (B, S * loop.da.n1) and loop.rt.c.shape[0] == B
        loop.run_day()
        loop.day_ahead()
        loop.hour_step(), loop.hour_step()
        runs[fused], ok = _snapshot(loop)
        assert ok and int(loop.hour_t.item()) == 26
    base = runs[False]
    assert np.abs(base["obj"]).max() > 0 and (base["da_count"] >= 1).all() and (base["da_count"] <= 2).all() and (base["da_count"] == 2).any()
    assert not base["da_curve"][:, :, 2:].any() and not base["da_curve"][:, :, :, 1].any()
    _same(base, runs[True], (flowsheet, market, B, S))


@gpu
@pytest.mark.parametrize("flowsheet", ["wind_battery", "nuclear"])
def test_graph_replay_is_the_eager_loop_bit_for_bit(flowsheet):
    """three days, B = 90 x S = 3: the steps of the third day are replays of graphs captured on the second - the 24 hourly steps, and
    the day-ahead step where the coupled LP stays in the fused kernels (a streamed coupled solve is host-driven and stays eager)"""
    runs = {}
    for graphs in (False, True):
        loop = _loop(flowsheet, 90, use_graphs=graphs)
        assert loop.use_fused
        for _ in range(3):
            loop.run_day()
        streamed = bool(loop.da.dlp.last_stats.streaming)
        assert streamed == (flowsheet == "wind_battery")                  # 582 x 408 streams; the nuclear coupled LP fits the fused kernels
        assert int(loop.hour_t.item()) == 72 and len(loop._graphs) == ((24 if streamed else 25) if graphs else 0)
        runs[graphs], ok = _snapshot(loop)
        assert ok
    _same(runs[False], runs[True], flowsheet)


@gpu
@pytest.mark.parametrize("flowsheet,B", [("wind_battery", 6), ("nuclear", 4)])
def test_oracle_walk_on_the_device(flowsheet, B):
    """S = 3, D = 3, two days (the second day's hours from graphs): every coupled day-ahead LP, hourly LP and tracking LP against the
    oracle's own at 1e-6 (the project's device parity bar), curves and dispatches exact from the read-back solutions, all optimal,
    nothing uncertified; the coupling binds (as on the CPU)"""
    from tests._self_schedule_oracle import oracle_walk
    loop = _loop(flowsheet, B)
    assert loop.use_fused and loop.use_graphs
    seen = oracle_walk(loop, 2)
    stats = loop.da.dlp.last_stats
    print("self-schedule", flowsheet, "loop on the device: worst relative gap", seen["worst"], "over", seen["lps"], "LPs; coupled solve streaming",
          stats.streaming, "stream_form", stats.stream_form, "iterations", loop.da.out["iters"].cpu().tolist())
    res, ok = loop.results()
    assert ok and seen["all_optimal"] and int(loop.uncertified.item()) == 0 and len(loop._graphs) == (24 if stats.streaming else 25)
    assert seen["worst"] <= 1e-6
    assert min(seen["coupling_margin"]) > 1e-3 and min(seen["schedule_distance"]) > 1.0 and seen["two_points"] > 0


@gpu
def test_schedule_prepare_refuses_malformed_descriptors_on_the_host():
    """dsp_loop_schedule_prepare on the descriptors of a real loop (wind + battery: wind columns, two state columns; B = 3, S = 3) over
    buffers filled with a sentinel: with ONE field broken - a NULL buffer that is used; S, D, T or n_state out of range; a column index
    outside the BLOCK (inside the row); a stride below S * n; per-plant size pointers - DSP_ERR_INVALID and nothing written.  The
    unedited descriptors are accepted and write every block."""
    import torch
    from dispatches_amd.hip_solver import DspLoopMarketModel, DspLoopMarketState
    loop = _loop("wind_battery", 3)
    lib, m0, s0 = loop._lib, loop._mk_da, loop._mk_sched
    n, S = m0.n, s0.S
    assert m0.row_stride == S * n and loop._mk_state.S == 1 and loop._mk_state.self_schedule == 1 and loop._mk_state.curve_slots == S + 1
    bufs = (loop.da.c, loop.da.lb, loop.da.ub, loop.da.c0)
    stream = C.c_void_p(torch.cuda.current_stream(loop.dev).cuda_stream)

    def call(edit=None):
        for t in bufs:
            t.fill_(-7.0)
        st, m = DspLoopMarketState.from_buffer_copy(s0), DspLoopMarketModel.from_buffer_copy(m0)
        if edit is not None:
            edit(st, m)
        rc = lib.dsp_loop_schedule_prepare(C.byref(st), C.byref(m), stream)
        torch.cuda.synchronize()
        return rc, all(bool((t == -7.0).all()) for t in bufs)

    st_field = lambda name, value: (lambda st, m: setattr(st, name, value))
    m_field = lambda name, value: (lambda st, m: setattr(m, name, value))

    def item(name, at, value):
        def edit(st, m):
            target = getattr(m, name)
            if isinstance(at, tuple):
                target[at[0]][at[1]] = value
            else:
                target[at] = value
        return edit
    some = loop.da.c0.data_ptr()
    edits = [m_field("c", None), m_field("lb", None), m_field("ub", None), m_field("base_c", None), m_field("c0", None),
             st_field("start", None), st_field("hour", None), st_field("da_series", None), st_field("rt_series", None), st_field("state", None),
             st_field("cf_series", None),
             st_field("S", 0), st_field("S", 17), st_field("S", 4), st_field("D", 0), st_field("D", 2), st_field("D", 400), m_field("T", 0), m_field("T", 49),
             m_field("n_state", 3), m_field("n_state", -1), m_field("n", 0),
             item("pda_cols", 3, n), item("pda_cols", 3, -1), item("pt_cols", (2, 0), n), item("pt_cols", (2, 1), -2), item("state_init", 0, n),
             item("state_init", 1, -1), item("wind_cols", 1, n), item("wind_cols", 5, 2 * n),
             m_field("row_stride", S * n - 1), m_field("row_stride", n), m_field("row_stride", 0), m_field("row_stride", -1),
             m_field("wind_kw_plant", some), m_field("c0_base_plant", some)]
    for k, edit in enumerate(edits):
        rc, untouched = call(edit)
        assert rc == -1 and untouched, k
    assert lib.dsp_loop_schedule_prepare(None, None, None) == -1
    assert lib.dsp_loop_schedule_prepare(C.byref(DspLoopMarketState()), C.byref(DspLoopMarketModel()), None) == -1
    rc, untouched = call()
    assert rc == 0 and not untouched and bool((loop.da.c0 != -7.0).all())
    pda = loop.da.pda_cols.cpu().numpy()
    ub = loop.da.ub.cpu().numpy().reshape(3, S, n)
    assert np.isinf(ub[:, :, pda]).all() and (loop.da.lb.cpu().numpy().reshape(3, S, n)[:, :, pda] == 0).all()
    # dsp_loop_market_prepare keeps its rows n apart: a stride of its own is refused, 0 and n are the same call
    loop.rt.c0.fill_(-7.0)
    m = DspLoopMarketModel.from_buffer_copy(loop._mk_rt)
    m.row_stride = 2 * m.n
    assert lib.dsp_loop_market_prepare(C.byref(loop._mk_state), C.byref(m), 0, stream) == -1
    torch.cuda.synchronize()
    assert bool((loop.rt.c0 == -7.0).all())
    # ... and the clearing refuses a stride inside a row, a curve stride below S + 1 points and a flag that is not 0 / 1
    for obj, name, value in (("m", "row_stride", n - 1), ("st", "curve_slots", 1), ("st", "curve_slots", 18), ("st", "self_schedule", 2)):
        st, m = DspLoopMarketState.from_buffer_copy(loop._mk_state), DspLoopMarketModel.from_buffer_copy(m0)
        setattr(m if obj == "m" else st, name, value)
        loop.da_count.fill_(-1)
        rc = lib.dsp_loop_market_clear(C.byref(st), C.byref(m), None, -1, 24, C.c_void_p(loop.da_offer.data_ptr()), C.c_void_p(loop.da_curve.data_ptr()),
                                       C.c_void_p(loop.da_count.data_ptr()), stream)
        torch.cuda.synchronize()
        assert rc == -1 and bool((loop.da_count == -1).all()), (name, value)


@gpu
def test_clearing_with_the_new_fields_at_zero_is_the_old_path():
    """a stochastic loop (bidder left at "lp") builds its descriptors with row_stride = 0, self_schedule = 0, curve_slots = 0, and its
    kernels give the curves and dispatches of the tensor form, as before ABI 18"""
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    runs = {}
    for fused in (False, True):
        loop = BatchedDoubleLoop("nuclear", 70, device=0, use_fused=fused, use_graphs=False, n_price_scenarios=3, forecaster="backcast",
                                 max_historical_days=3, market="price_taker", day_ahead_horizon=24)
        if fused:
            assert loop._mk_da.row_stride == loop._mk_rt.row_stride == 0 and loop._mk_state.self_schedule == 0 and loop._mk_state.curve_slots == 0
        loop.day_ahead()
        loop.hour_step(), loop.hour_step()
        runs[fused] = {k: getattr(loop, k).cpu().numpy().copy() for k in ("da_curve", "da_count", "da_offer", "da_prices", "rt_curve", "rt_count", "rt_dispatch")}
        assert loop.results()[1]
    assert (runs[False]["da_count"] > 2).any()
    _same(runs[False], runs[True], "lp")


@gpu
def test_the_default_loop_is_left_alone():
    """BatchedDoubleLoop(flowsheet, 64, n_price_scenarios=3, forecaster="backcast", market="price_taker") with the bidder left at its
    default: bit-identical after two days whether or not a self-schedule loop was built and run in the same process before it"""
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    for flowsheet in FLOWSHEETS:
        def default():
            loop = BatchedDoubleLoop(flowsheet, 64, device=0, n_price_scenarios=3, forecaster="backcast", market="price_taker")
            assert not loop.self_schedule
            loop.run_day(), loop.run_day()
            out, ok = _snapshot(loop)
            assert ok
            return out
        before = default()
        other = _loop(flowsheet, 16)
        other.run_day()
        assert other.results()[1]
        _same(before, default(), flowsheet)
