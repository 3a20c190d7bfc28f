"""GPU tests of the parametrized mode of the descriptor loop (dispatches_amd/rolling_flowsheets.py::BatchedDoubleLoop with
bidder="parametrized"; csrc/dsp_param.hip: dsp_loop_param_step): the entry point alone on synthetic inputs against the tensor form, its
refusals on the host, kernels against tensor operations and graph replay against the eager loop bit for bit, the oracle walk on the
device, and the reference-shaped sweep over 30 days."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
FLOWSHEETS = ("wind_pem", "wind_battery")
PEM_BIDS = [15.0, 20.0, 25.0, 30.0, 35.0, 40.0, 45.0]                   # run_double_loop_PEM.py --pem_bid
PEM_SIZES = [847.0 * f for f in (0.05, 0.1, 0.25, 0.5, 1.0)]            # --pem_pmax; 0.25 * 847 = 211.75, the reference's default


def _pair(flowsheet, B, market, seed):
    """a tensor-form loop and a kernel loop (no graphs) on the SAME synthetic data: capacity factors that put the wind exactly on, a cent
    below and a cent above the storage sizes and on x.xx5 rounding boundaries, prices that tie the bids to the cent, starts next to the
    end of the circular series"""
    import torch
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    rng = np.random.default_rng(seed)
    sizes = np.array([0.0, 50.0, 100.0, 100.005, 0.004, 1e4])
    bids = np.array([0.0, 12.345, 30.0, 30.01, 0.004, 45.0])
    storage, bid = sizes[rng.integers(0, len(sizes), B)], bids[rng.integers(0, len(bids), B)]
    loops = [BatchedDoubleLoop(flowsheet, B, device=0, use_graphs=False, use_fused=fused, bidder="parametrized", bid_price=bid, storage_mw=storage,
                               market=market) for fused in (False, True)]
    a, k = loops
    assert not a.use_fused and k.use_fused
    N, wind = a.N, a.wind_mw
    w = np.array([0.0, 100.0, 100.004, 100.005, 100.006, 100.01, 99.995, 50.0, 50.005, 49.995, 0.004, 0.005, 0.0051, 150.0, 1e-9, 30.0])
    prices = np.concatenate([bids, bids + 0.005, bids - 0.005, [0.0, 500.0, 29.999999, 30.000001, 12.35, 12.34]]).clip(0.0)
    cf = lambda: np.where(rng.random(N) < 0.8, w[rng.integers(0, len(w), N)] / wind, rng.random(N))
    price = lambda: np.where(rng.random(N) < 0.8, prices[rng.integers(0, len(prices), N)], np.round(rng.uniform(0, 60, N), 3))
    data = dict(cf_series=cf(), da_cf_series=cf(), da_series=price(), rt_series=price())
    start = rng.integers(0, N, B)
    start[:4] = [N - 1, N - 3, N - 30, 0]
    state = np.round(rng.uniform(0, 20000, (B, len(a.scale))), 2)
    x = rng.uniform(0, 1e5, tuple(a.tr.out["x"].shape))
    for loop in loops:
        for name, v in data.items():
            getattr(loop, name).copy_(torch.as_tensor(v, device=loop.dev))
        loop.start.copy_(torch.as_tensor(start, device=loop.dev))
        loop.state.copy_(torch.as_tensor(state, device=loop.dev))
        loop.tr.out["x"].copy_(torch.as_tensor(x, device=loop.dev))
    return a, k, dict(start=start, storage=storage, bid=bid, **data)


def _outputs(loop, names):
    import torch
    torch.cuda.synchronize()
    out = {}
    for name in names:
        t = getattr(loop.tr, name[3:]) if name.startswith("tr_") else getattr(loop, name)
        out[name] = t.cpu().numpy().copy()
    return out


DA_OUT = ("da_offer", "da_prices", "da_curve", "da_count")
RT_OUT = ("rt_dispatch", "rt_curve", "rt_count", "tr_rlo", "tr_rhi", "tr_lb", "tr_ub", "tr_c0")


@gpu
@pytest.mark.parametrize("market", ["price_taker", "stub"])
@pytest.mark.parametrize("flowsheet", FLOWSHEETS)
def test_param_step_alone_is_the_tensor_form(flowsheet, market):
    """dsp_loop_param_step through ctypes, B = 60 (lanes not a multiple of 64), phases 0, 1, 2 on synthetic series: adversarial ties and
    duplicate powers, storage on both sides of the wind, windows that wrap the circular series.  Every output equals the tensor form bit
    for bit; the curves are also checked against the rule in plain Python, so that the two cannot be wrong together."""
    import torch
    from tests._flowsheet_stochastic_oracle import clear, reference_curve
    B = 60
    a, k, inp = _pair(flowsheet, B, market, seed=11)
    lib, N = k._lib, a.N
    stream = lambda: C.c_void_p(torch.cuda.current_stream(k.dev).cuda_stream)
    for hour in (48, N - 7):                                                # (the second clock wraps every window)
        for loop in (a, k):
            loop.hour_t.fill_(hour)
        a._day_ahead_step_parametrized()
        assert lib.dsp_loop_param_step(C.byref(k._param_state), C.byref(k._loop_tr), 0, -1, stream()) == 0
        want, got = _outputs(a, DA_OUT), _outputs(k, DA_OUT)
        for name in DA_OUT:
            assert np.array_equal(want[name], got[name]), (hour, name)
        seen = {1: 0, 2: 0, 3: 0}
        below = 0
        for b in range(B):
            for t in range(24):
                at = (inp["start"][b] + hour + t) % N
                wv = inp["da_cf_series"][at] * a.wind_mw
                hi = max(wv, inp["storage"][b]) if flowsheet == "wind_battery" else wv
                U, M = reference_curve([0.0, max(0.0, wv - inp["storage"][b]), hi], [0.0, 0.0, inp["bid"][b]], [True] * 3, 0)
                c = int(got["da_count"][b, t])
                assert (got["da_curve"][b, t, :c, 0].tolist(), got["da_curve"][b, t, :c, 1].tolist()) == (U, M), (b, t)
                assert not got["da_curve"][b, t, c:].any()
                d = clear(U, M, inp["da_series"][at], market)
                assert got["da_offer"][b, t] == d and got["da_prices"][b, t] == inp["da_series"][at], (b, t)
                seen[c] += 1
                below += d < U[-1] / 100.0
        assert min(seen.values()) >= 1 and (below > 0) == (market == "price_taker"), (seen, below)
    for hour, kk in ((24 * 2 + 5, 5), (N - 2, (N - 2) % 24)):
        for loop in (a, k):
            loop.hour_t.fill_(hour)
        a._param_dispatch(kk)
        assert lib.dsp_loop_param_step(C.byref(k._param_state), C.byref(k._loop_tr), 1, kk, stream()) == 0
        want, got = _outputs(a, RT_OUT), _outputs(k, RT_OUT)
        for name in RT_OUT:
            assert np.array_equal(want[name], got[name]), (hour, name)
        assert (got["rt_count"] >= 1).all() and (got["rt_count"] == 3).any() and np.abs(got["tr_rlo"]).max() > 0
        if a.h2_kg is not None:
            for _ in range(2):                                              # (accumulates)
                a._param_hydrogen(kk)
                assert lib.dsp_loop_param_step(C.byref(k._param_state), C.byref(k._loop_tr), 2, kk, stream()) == 0
            want, got = _outputs(a, ("h2_kg",)), _outputs(k, ("h2_kg",))
            assert np.array_equal(want["h2_kg"], got["h2_kg"]) and (got["h2_kg"] > 0).all()


@gpu
def test_param_step_refuses_malformed_descriptors_on_the_host():
    """DSP_ERR_INVALID and nothing written for B < 1, N < 24, a tracker horizon outside 1 .. 16, a NULL series / parameter array /
    output, a dispatch row, wind column or state column out of range, a phase or k out of range - each refused BEFORE any launch"""
    import torch
    from dispatches_amd.hip_solver import DspLoopModel, DspLoopParamState, load_library
    lib = load_library()
    for flowsheet in FLOWSHEETS:
        _, k, _ = _pair(flowsheet, 8, "price_taker", seed=3)
        k.hour_t.fill_(29)
        names = DA_OUT + RT_OUT + (("h2_kg",) if k.h2_kg is not None else ())
        for name in names:
            (getattr(k.tr, name[3:]) if name.startswith("tr_") else getattr(k, name)).fill_(-7)
        before = _outputs(k, names)
        stream = C.c_void_p(torch.cuda.current_stream(k.dev).cuda_stream)

        def refused(phase, kk, st_edit=None, tr_edit=None):
            st, tr = DspLoopParamState.from_buffer_copy(k._param_state), DspLoopModel.from_buffer_copy(k._loop_tr)
            if st_edit is not None:
                setattr(st, *st_edit)
            if tr_edit is not None:
                name, value = tr_edit
                if isinstance(name, tuple):
                    getattr(tr, name[0])[name[1]] = value
                else:
                    setattr(tr, name, value)
            return lib.dsp_loop_param_step(C.byref(st), C.byref(tr), phase, kk, stream)
        common = [("B", 0), ("B", -3), ("N", 23), ("N", 0), ("start", None), ("hour", None), ("da_series", None), ("rt_series", None),
                  ("da_cf_series", None), ("rt_cf_series", None), ("bid_price", None), ("storage_mw", None)]
        for phase, kk in ((0, -1), (1, 5), (2, 5)):
            if phase == 2 and k.h2_kg is None:
                assert refused(2, 5) == -1                                  # no electrolyser: no hydrogen phase
                continue
            for edit in common:
                assert refused(phase, kk, st_edit=edit) == -1, (phase, edit)
            for T in (0, 17, -1):
                assert refused(phase, kk, tr_edit=("T", T)) == -1, (phase, T)
        for phase, kk in ((0, 0), (0, 5), (0, -2), (1, -1), (1, 24), (2, -1), (2, 24), (3, 0), (-1, 0)):
            assert refused(phase, kk) == -1, (phase, kk)
        for edit in (("da_offer", None), ("da_prices", None), ("da_curve", None), ("da_count", None)):
            assert refused(0, -1, st_edit=edit) == -1, edit
        for edit in (("rt_dispatch", None), ("rt_curve", None), ("rt_count", None)) + ((("state", None),) if len(k.scale) else ()):
            assert refused(1, 5, st_edit=edit) == -1, edit
        n, m = k.tr.lp.n, k.tr.lp.m
        tr_edits = [("rlo", None), ("rhi", None), ("lb", None), ("ub", None), ("c0", None), ("n", 0), ("m", 0), ("n_state", 3), ("n_state", -1),
                    (("track_rows", 1), m), (("track_rows", 0), -1), (("wind_cols", 2), n), (("wind_cols", 1), -1)]
        if len(k.scale):
            tr_edits += [(("state_init", 0), n), (("state_init", 1), -1)]
        for edit in tr_edits:
            assert refused(1, 5, tr_edit=edit) == -1, edit
        if k.h2_kg is not None:
            for edit in (("h2_kg", None), ("pem_col", n), ("pem_col", -1)):
                assert refused(2, 5, st_edit=edit) == -1, edit
            assert refused(2, 5, tr_edit=("x", None)) == -1
        after = _outputs(k, names)
        for name in names:
            assert np.array_equal(before[name], after[name]), name
        assert refused(0, -1) == 0 and refused(1, 5) == 0                   # (the unedited descriptors are accepted, and write)
        after = _outputs(k, names)
        assert (after["da_count"] >= 1).all() and (after["rt_count"] >= 1).all()
    assert lib.dsp_loop_param_step(None, None, 0, -1, None) == -1
    assert lib.dsp_loop_param_step(C.byref(DspLoopParamState()), C.byref(DspLoopModel()), 0, -1, None) == -1


def _snapshot(loop):
    res, ok = loop.results()
    out = {k: v.cpu().numpy().copy() for k, v in res.items()}
    for key in ("c", "lb", "ub", "rlo", "rhi", "c0"):
        out["tr_" + key] = getattr(loop.tr, key).cpu().numpy().copy()
    for key in ("da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch", "da_offer", "da_prices"):
        out[key] = getattr(loop, key).cpu().numpy().copy()
    return out, ok


@gpu
@pytest.mark.parametrize("market", ["price_taker", "stub"])
@pytest.mark.parametrize("flowsheet", FLOWSHEETS)
def test_kernels_tensor_operations_and_graph_replay_agree_bit_for_bit(flowsheet, market):
    """use_fused True / False and graph replay / eager, B = 64 on 16 windows x 4 parameter points, three days (the third is a replay of
    graphs captured on the second): da_offer, curves, counts, rt_dispatch, the tracker's rows and bounds, state, revenue and h2_kg bit
    for bit"""
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    B, days = 64, 3
    wind = 847.0 if flowsheet == "wind_pem" else 200.0
    bid = np.tile([0.0, 20.0, 30.0, 45.0], B // 4)
    storage = np.tile([0.25 * wind, 0.0, 0.5 * wind, 2.0 * wind], B // 4)
    windows = np.repeat(np.arange(B // 4), 4)
    runs = {}
    for fused, graphs in ((False, False), (True, False), (True, True)):
        loop = BatchedDoubleLoop(flowsheet, B, device=0, use_graphs=graphs, use_fused=fused, bidder="parametrized", bid_price=bid, storage_mw=storage,
                                 plant_windows=windows, market=market)
        assert loop.use_fused == fused and loop.parametrized
        for _ in range(days):
            loop.run_day()
        assert int(loop.hour_t.item()) == 24 * days and len(loop._graphs) == (25 if graphs else 0) and loop.solves == days * 24 * B
        runs[fused, graphs], ok = _snapshot(loop)
        assert ok and int(loop.uncertified.item()) == 0
    base = runs[False, False]
    assert np.abs(base["obj"]).max() > 0 and (base["da_count"] >= 1).all() and (base["da_count"] == 3).any()
    worst = {}
    for k in base:
        for key, other in runs.items():
            if not np.array_equal(base[k], other[k]):
                worst[k, key] = float(np.abs(base[k] - other[k]).max() / max(1.0, np.abs(base[k]).max()))
    print("parametrized", flowsheet, market, "kernel / graph runs that differ from the tensor form (relative):", worst)
    for k in base:
        for key, other in runs.items():
            assert np.array_equal(base[k], other[k]), (key, k, worst)


@gpu
@pytest.mark.parametrize("flowsheet", FLOWSHEETS)
def test_parametrized_oracle_walk_on_the_device(flowsheet):
    """B = 12, two days, the second replayed from graphs: curves against the host bidders, clearing exact, every tracking LP against
    the oracle's own at 1e-6 relative, every status optimal; the worst gap is printed"""
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from tests._parametrized_oracle import parametrized_walk
    B = 12
    wind = 847.0 if flowsheet == "wind_pem" else 200.0
    bid = np.array([0.0, 15.0, 20.0, 25.0, 30.0, 35.0, 40.0, 45.0, 30.0, 30.0, 30.0, 30.0])
    storage = np.array([0.25 * wind] * 8 + [0.0, 0.05 * wind, 0.5 * wind, 10.0 * wind])
    loop = BatchedDoubleLoop(flowsheet, B, device=0, first_scenario=40, bidder="parametrized", bid_price=bid, storage_mw=storage, market="price_taker")
    assert loop.use_fused and loop.use_graphs
    seen = parametrized_walk(loop, 2)
    print("parametrized", flowsheet, "loop on the device: worst relative objective gap of", seen["lps"], "tracking LPs =", seen["worst"], seen)
    res, ok = loop.results()
    assert ok and seen["all_optimal"] and int(loop.uncertified.item()) == 0 and len(loop._graphs) == 25
    assert seen["worst"] <= 1e-6
    assert seen["lps"] == 2 * 24 * B and seen["below"] >= 1 and seen["equal"] >= 1 and seen["points"][3] >= 1, seen


@gpu
def test_reference_shaped_sweep_over_thirty_days():
    """wind + PEM, pem_bid 15 .. 45 step 5 (and 0) x five PEM sizes x 8 windows = 320 plants, 30 days from graphs: all optimal; for a fixed
    window and size the cleared day-ahead energy does not increase with the bid price (a higher bid only ever loses hours); with a bid
    of 0 everything offered clears"""
    from dispatches_amd import sweeps
    bids = [0.0] + PEM_BIDS
    out = sweeps.parametrized_sweep("wind_pem", bids, PEM_SIZES, 8, 30, device=0, market="price_taker")
    assert out["all_optimal"] is True
    for key in ("revenue", "energy_mwh", "da_energy_mwh", "offered_mwh", "h2_kg"):
        assert out[key].shape == (len(bids), len(PEM_SIZES), 8) and np.isfinite(out[key]).all()
    da = out["da_energy_mwh"]
    print("sweep: cleared day-ahead energy by bid price (mean over sizes and windows):", da.mean(axis=(1, 2)).round(1).tolist(),
          "hydrogen [t]:", (out["h2_kg"].mean(axis=(1, 2)) / 1e3).round(1).tolist())
    assert (np.diff(da, axis=0) <= 0).all() and (np.diff(da, axis=0) < 0).any()
    assert np.array_equal(da[0], out["offered_mwh"][0])
    assert (da <= out["offered_mwh"]).all() and (out["h2_kg"] >= 0).all() and out["h2_kg"].max() > 0
    assert (out["offered_mwh"] == out["offered_mwh"][:1]).all()                # the offer's last point is the wind: no parameter moves it
