"""GPU tests of the stochastic mode of the device-resident double loop (dispatches_amd/rolling.py: backcast scenarios, bid curves, market
clearing; csrc/dsp_market.hip): the curve + clearing kernel alone against the plain-Python statement, the fused kernels against the tensor
operations and graph replay against the eager loop bit for bit, every recorded LP against the oracle's own, a longer run."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu


def _market_call(S, B, k, T, backcast=True, price_taker=True, fail=(), seed=0, D=16, with_tracker=False, edit=None):
    """dsp_market_clear through ctypes on a synthetic solution -> (rc, inputs, outputs)"""
    import torch
    from dispatches_amd.hip_solver import DspMarketModel, DspMarketState, DspWbModel, load_library
    from tests.test_market_cpu import adversarial_pairs
    lib = load_library()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed)
    n, N = 40, 24 * 20
    # prices: a series of adversarial values; powers: columns of x (day-ahead: column 2 t; real time: 1e-3 (x[2 t] + x[2 t + 1]))
    _, series = adversarial_pairs(rng, 1, N)
    series = series[0]
    power, _ = adversarial_pairs(rng, B * S, T)
    x = rng.uniform(0, 100, (B * S, n))
    for t in range(T):
        if k < 0:
            x[:, t] = power[:, t]
        else:
            x[:, 2 * t] = np.round(power[:, t] * 600.0)
            x[:, 2 * t + 1] = np.round(power[:, t] * 400.0)
    status = np.zeros(B * S, np.int32)
    status[list(fail)] = 1
    x[list(fail)] = np.nan
    start = rng.integers(0, N, B)
    hour = 24 * 3 + max(k, 0)
    t_ = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    keep = dict(x=t_(x, torch.float64), status=t_(status, torch.int32), start=t_(start, torch.int64), hour=t_([hour], torch.int64)[0],
                series=t_(series, torch.float64), da_prices=torch.zeros((B, 24), dtype=torch.float64, device=dev),
                bad=torch.zeros((), dtype=torch.bool, device=dev),
                dispatch=torch.full((B, T), -1.0, dtype=torch.float64, device=dev), curve=torch.full((B, T, S + 1, 2), -7, dtype=torch.int32, device=dev),
                count=torch.full((B, T), -1, dtype=torch.int32, device=dev))
    st = DspMarketState()
    st.B, st.S, st.D, st.N, st.backcast, st.price_taker = B, S, D, N, int(backcast), int(price_taker)
    st.start, st.hour = keep["start"].data_ptr(), keep["hour"].data_ptr()
    st.da_series = st.rt_series = st.cf_series = keep["series"].data_ptr()
    st.da_prices, st.bad = keep["da_prices"].data_ptr(), keep["bad"].data_ptr()
    m = DspMarketModel()
    m.x, m.status, m.n, m.T = keep["x"].data_ptr(), keep["status"].data_ptr(), n, max(T, 4)
    for t in range(m.T):
        m.pda_cols[t] = t
        m.pt_cols[t][0], m.pt_cols[t][1] = (2 * t) % n, (2 * t + 1) % n
    args = dict(dispatch=keep["dispatch"].data_ptr(), curve=keep["curve"].data_ptr(), count=keep["count"].data_ptr(), T=T, k=k)
    if edit is not None:
        edit(st, m, args)
    rc = lib.dsp_market_clear(C.byref(st), C.byref(m), None, args["k"], args["T"], C.c_void_p(args["dispatch"]), C.c_void_p(args["curve"]),
                              C.c_void_p(args["count"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    out = {key: keep[key].cpu().numpy() for key in ("dispatch", "curve", "count", "da_prices", "bad")}
    return rc, dict(x=x, status=status, start=start, hour=hour, series=series, N=N), out


@gpu
@pytest.mark.parametrize("k", [-1, 5])
@pytest.mark.parametrize("S", [1, 2, 3, 16])
def test_curve_and_clearing_kernel_is_the_plain_python_statement(S, k):
    """dsp_market_clear alone on synthetic solutions - exact ties in power and in price, duplicates, x.xx5 rounding boundaries, rows that
    are not optimal, B not a multiple of 64: curves, counts and dispatches equal the plain-Python / numpy statement exactly"""
    from dispatches_amd.workflow.market import clear_price_taker
    from tests._stochastic_oracle import host_backcast, numpy_path_agrees, reference_curve
    B, T, D = 70, (24 if k < 0 else 4), 16
    fail = tuple(range(S)) + (S * 5, S * 9 + S - 1)                  # plant 0: no row optimal; plants 5 and 9: one row missing
    for price_taker in (True, False):
        rc, inp, out = _market_call(S, B, k, T, price_taker=price_taker, fail=set(fail), seed=10 * S + k + 1, D=D)
        assert rc == 0 and bool(out["bad"])
        hod, day = max(k, 0), inp["hour"] // 24
        below = 0
        for b in range(B):
            fc = host_backcast(inp["series"], int(inp["start"][b]), day, hod, T, S, D)
            real = inp["series"][(inp["start"][b] + inp["hour"] + np.arange(T)) % inp["N"]]
            ok = inp["status"][b * S:(b + 1) * S] == 0
            for t in range(T):
                xs = inp["x"][b * S:(b + 1) * S]
                power = xs[:, t] if k < 0 else 1e-3 * (xs[:, 2 * t] + xs[:, 2 * t + 1])
                U, M = reference_curve(power, fc[:, t], ok)
                c = int(out["count"][b, t])
                assert (out["curve"][b, t, :c, 0].tolist(), out["curve"][b, t, :c, 1].tolist()) == (U, M), (b, t)
                assert not out["curve"][b, t, c:].any()
                assert numpy_path_agrees(np.where(ok, power, 0.0), fc[:, t], ok, U, M)
                lmp = real[t] if (k < 0 or t == 0) else fc[0, t]
                want = clear_price_taker(np.array(U) / 100.0, np.array(M) / 100.0, lmp) if price_taker else U[-1] / 100.0
                assert out["dispatch"][b, t] == want, (b, t)
                below += want < U[-1] / 100.0
            if k < 0:
                assert np.array_equal(out["da_prices"][b, :T], real)
        assert not out["curve"][0].any() and (out["count"][0] == 1).all() and not out["dispatch"][0].any()
        assert (below > 0) == price_taker


@gpu
def test_market_entry_points_refuse_bad_arguments_on_the_host():
    from dispatches_amd.hip_solver import DspMarketModel, DspMarketState, load_library
    def field(obj, name, value):
        return lambda st, m, a: setattr(st if obj == "st" else m, name, value)
    def arg(name, value):
        return lambda st, m, a: a.__setitem__(name, value)
    def col(st, m, a):
        m.pda_cols[3] = -1
    def col_big(st, m, a):
        m.pda_cols[3] = 40
    for edit in (field("st", "S", 17), field("st", "S", 0), field("st", "D", 2), field("st", "D", 0), field("st", "N", 24), field("st", "start", None),
                 field("st", "hour", None), field("st", "da_series", None), field("st", "da_prices", None), field("m", "x", None),
                 field("m", "status", None), field("m", "n", 0), field("m", "T", 49), arg("curve", None), arg("count", None), arg("dispatch", None),
                 arg("T", 25), arg("T", 0), arg("k", 24), arg("k", -2), col, col_big):
        rc, _, out = _market_call(3, 8, -1, 24, edit=edit)
        assert rc == -1 and (out["count"] == -1).all() and (out["dispatch"] == -1.0).all()          # DSP_ERR_INVALID, nothing written
    rc, _, _ = _market_call(3, 8, 5, 4, edit=arg("T", 9))
    assert rc == -1
    rc, _, _ = _market_call(2, 8, -1, 24, backcast=False)                                          # the perfect forecaster knows one scenario
    assert rc == -1
    lib = load_library()
    assert lib.dsp_market_prepare(None, None, 0, None) == -1
    assert lib.dsp_market_prepare(C.byref(DspMarketState()), C.byref(DspMarketModel()), 0, None) == -1
    assert lib.dsp_market_clear(None, None, None, 0, 4, None, None, None, None) == -1


def _snapshot(loop):
    res, ok = loop.results()
    out = {k: v.cpu().numpy().copy() for k, v in res.items()}
    for name, m in (("da", loop.da), ("rt", loop.rt), ("tr", loop.tr)):
        for key in ("c", "lb", "ub", "rlo", "rhi", "c0"):
            out[name + "_" + key] = getattr(m, key).cpu().numpy().copy()
    for key in ("da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch", "da_offer", "da_prices", "delivered"):
        if hasattr(loop, key):
            out[key] = getattr(loop, key).cpu().numpy().copy()
    out["uncertified"] = np.array(int(loop.uncertified.item()))
    return out, ok


@gpu
@pytest.mark.parametrize("market", ["price_taker", "stub"])
def test_stochastic_kernels_and_graphs_are_bit_identical_to_the_tensor_operations(market):
    """use_fused True / False and graph replay / eager, S = 3, three days (the third is a replay of graphs captured on the second):
    objective vectors, bounds, curves, dispatches, state and revenue bit for bit"""
    from dispatches_amd.rolling import BatchedWindBatteryDoubleLoop
    B, days = 96, 3
    runs = {}
    for fused, graphs in ((False, False), (True, False), (True, True)):
        loop = BatchedWindBatteryDoubleLoop(B, device=0, use_graphs=graphs, use_fused=fused, n_price_scenarios=3, forecaster="backcast", market=market)
        assert loop.use_fused == fused and loop.stochastic
        for _ in range(days):
            loop.run_day()
        assert int(loop.hour_t.item()) == 24 * days and (len(loop._graphs) == 25) == graphs
        runs[fused, graphs], ok = _snapshot(loop)
        assert ok
    base = runs[False, False]
    assert np.abs(base["obj"]).max() > 0 and (base["da_count"] > 1).any()
    for key, other in runs.items():
        for k in base:
            assert np.array_equal(base[k], other[k]), (key, k)


@gpu
def test_every_recorded_lp_curve_and_dispatch_of_the_stochastic_loop_on_the_device():
    """12 plants, S = 3, two days (the second replayed from graphs): every recorded LP against the oracle's own at 1e-6, curves and
    dispatches exact from the recorded solutions, revenue re-added, nothing uncertified, all optimal"""
    from dispatches_amd.rolling import BatchedWindBatteryDoubleLoop
    from tests._rolling_oracle import column_maps
    from tests._stochastic_oracle import check_recorded
    B, S, D, days = 12, 3, 10, 2
    loop = BatchedWindBatteryDoubleLoop(B, device=0, stride=17, n_price_scenarios=S, forecaster="backcast", max_historical_days=D,
                                        market="price_taker", record=(list(range(B)), days))
    for _ in range(days):
        loop.run_day()
    res, ok = loop.results()
    assert ok and int(loop.uncertified.item()) == 0
    seen = check_recorded(dict(S=S, D=D, forecaster="backcast", market="price_taker"), column_maps(loop), loop.recorded(),
                          res["obj"].cpu().numpy(), stride=17)
    print("stochastic loop on the device:", seen)
    assert seen["lps"] == B * days * S + B * 24 * days * (S + 1) and seen["worst"] <= 1e-6
    assert seen["forecast_differs"] > 0.5 * seen["forecast_hours"] and seen["below"] >= 1 and seen["equal"] >= 1, seen


@gpu
def test_longer_stochastic_run_leaves_the_deterministic_loop_alone():
    """1024 plants, S = 3, 30 days from graphs (two pipelined groups): all optimal; a default-argument loop run in the same process before
    and after it gives bit-identical results"""
    from dispatches_amd.rolling import BatchedWindBatteryDoubleLoop, PipelinedDoubleLoops

    def deterministic():
        loop = BatchedWindBatteryDoubleLoop(256, device=0)
        for _ in range(3):
            loop.run_day()
        out, ok = _snapshot(loop)
        assert ok and not loop.stochastic
        return out
    before = deterministic()
    loop = PipelinedDoubleLoops(1024, device=0, n_price_scenarios=3, forecaster="backcast", market="price_taker")
    assert loop.groups == 2
    loop.run_days(30)
    res, ok = loop.results()
    assert ok and loop.hour == 24 * 30 and int(loop.uncertified.item()) == 0
    assert (res["da_energy_mwh"] <= res["offered_mwh"]).all() and (res["da_energy_mwh"] < res["offered_mwh"]).any()
    assert float(res["obj"].abs().max().item()) > 0
    after = deterministic()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
