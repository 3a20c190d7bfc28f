"""GPU tests of the stochastic mode of the descriptor loop (dispatches_amd/rolling_flowsheets.py::BatchedDoubleLoop; csrc/dsp_market.hip:
dsp_loop_market_prepare / dsp_loop_market_clear): the curve + clearing kernel alone against the plain-Python statement (minimum power,
coefficient / constant form of the power, tracker rows), refusals on the host, the kernels against the tensor operations and graph
replay against the eager loop bit for bit for all three flowsheets, the oracle walk on the device, a longer nuclear run."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
FLOWSHEETS = ("wind_battery", "wind_pem", "nuclear")
CA, CB = 1.25e-3, 2e-3                                          # coefficients of the synthetic power output (not the wind plants' 1e-3)


def _consts(T):
    return np.array([0.0, 0.37, -1.5, 12.345, 400.0, 0.005][:T] + [0.25] * max(0, T - 6))


def _clear_call(S, B, k, T, p_min_cents=0, backcast=True, price_taker=True, fail=(), seed=0, D=16, with_tracker=False, edit=None, prepare=False):
    """dsp_loop_market_clear (or _prepare) through ctypes on a synthetic solution -> (rc, inputs, outputs)"""
    import torch
    from dispatches_amd.hip_solver import DspLoopMarketModel, DspLoopMarketState, DspLoopModel, load_library
    from tests.test_market_cpu import adversarial_pairs
    lib = load_library()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed)
    n, N, m_tr = 40, 24 * 20, 9
    _, series = adversarial_pairs(rng, 1, N)
    series = series[0]
    power, _ = adversarial_pairs(rng, B * S, T)
    if p_min_cents:                                             # pairs on both sides of the minimum power, some exactly on it
        power = np.round(power + p_min_cents / 100.0 - 110.0, 3)
        power[rng.random(power.shape) < 0.15] = p_min_cents / 100.0
    x = rng.uniform(0, 100, (B * S, n))
    consts = _consts(T)
    cols = np.array([[(2 * t) % n, -1 if t == 1 else (2 * t + 1) % n] for t in range(T)])      # period 1 has ONE term
    for t in range(T):
        if k < 0:
            x[:, t] = power[:, t]
        else:                                                   # about half of the power from each term (all of it in the one-term period)
            x[:, cols[t, 0]] = np.round((power[:, t] - consts[t]) * (800.0 if t == 1 else 400.0))
            if cols[t, 1] >= 0:
                x[:, cols[t, 1]] = np.round((power[:, t] - consts[t]) * 250.0)
    status = np.zeros(B * S, np.int32)
    status[list(fail)] = 1
    x[list(fail)] = np.nan
    start = rng.integers(0, N, B)
    hour = 24 * 3 + max(k, 0)
    state = np.round(rng.uniform(0, 50, (B, 1)))
    t_ = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    f64 = lambda *shape, fill=-1.0: torch.full(shape, fill, dtype=torch.float64, device=dev)
    keep = dict(x=t_(x, torch.float64), status=t_(status, torch.int32), start=t_(start, torch.int64), hour=t_([hour], torch.int64)[0],
                series=t_(series, torch.float64), da_prices=torch.zeros((B, 24), dtype=torch.float64, device=dev), da_offer=f64(B, 24, fill=3.0),
                bad=torch.zeros((), dtype=torch.bool, device=dev), state=t_(state, torch.float64), base_c=f64(n, fill=0.5),
                c=f64(B * S, n), lb=f64(B * S, n), ub=f64(B * S, n), c0=f64(B * S),
                dispatch=f64(B, T), curve=torch.full((B, T, S + 1, 2), -7, dtype=torch.int32, device=dev),
                count=torch.full((B, T), -1, dtype=torch.int32, device=dev),
                tr_lb=f64(B, n), tr_ub=f64(B, n), tr_rlo=f64(B, m_tr), tr_rhi=f64(B, m_tr), tr_c0=f64(B))
    st = DspLoopMarketState()
    st.B, st.S, st.D, st.N, st.backcast, st.price_taker, st.p_min_cents = B, S, D, N, int(backcast), int(price_taker), p_min_cents
    st.start, st.hour = keep["start"].data_ptr(), keep["hour"].data_ptr()
    st.da_series = st.rt_series = st.cf_series = keep["series"].data_ptr()
    st.da_prices, st.da_offer, st.bad, st.state = keep["da_prices"].data_ptr(), keep["da_offer"].data_ptr(), keep["bad"].data_ptr(), keep["state"].data_ptr()
    m = DspLoopMarketModel()
    m.x, m.status, m.n, m.T, m.n_state = keep["x"].data_ptr(), keep["status"].data_ptr(), n, max(T, 4), 1
    m.c, m.lb, m.ub, m.c0, m.base_c = (keep[key].data_ptr() for key in ("c", "lb", "ub", "c0", "base_c"))
    m.state_init[0] = 38
    for t in range(len(m.pda_cols)):
        live = t < m.T
        m.pda_cols[t] = (t if k < 0 else 24 + t) if live else -1
        m.wind_cols[t] = -1
        for e in range(2):
            m.pt_cols[t][e] = int(cols[t, e]) if t < T else -1
        m.pt_coef[t][0], m.pt_coef[t][1] = CA, CB
        m.pt_const[t] = float(consts[t]) if t < T else 0.0
    tr = DspLoopModel()
    tr.lb, tr.ub, tr.rlo, tr.rhi, tr.c0 = (keep["tr_" + key].data_ptr() for key in ("lb", "ub", "rlo", "rhi", "c0"))
    tr.n, tr.m, tr.T, tr.n_state, tr.c0_base = n, m_tr, T, 1, 17.5
    tr.state_init[0] = 7
    for t in range(16):
        tr.track_rows[t] = 2 * t if t < T else -1
        tr.wind_cols[t] = -1
        tr.pt_const[t] = float(consts[t]) if t < T else 0.0
    args = dict(dispatch=keep["dispatch"].data_ptr(), curve=keep["curve"].data_ptr(), count=keep["count"].data_ptr(), T=T, k=k,
                tr=tr if with_tracker else None)
    if edit is not None:
        edit(st, m, args)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if prepare:
        rc = lib.dsp_loop_market_prepare(C.byref(st), C.byref(m), args["k"], stream)
    else:
        rc = lib.dsp_loop_market_clear(C.byref(st), C.byref(m), C.byref(args["tr"]) if args["tr"] is not None else None, args["k"], args["T"],
                                       C.c_void_p(args["dispatch"]), C.c_void_p(args["curve"]), C.c_void_p(args["count"]), stream)
    torch.cuda.synchronize()
    out = {key: keep[key].cpu().numpy() for key in ("dispatch", "curve", "count", "da_prices", "bad", "c", "lb", "ub", "c0",
                                                    "tr_lb", "tr_ub", "tr_rlo", "tr_rhi", "tr_c0")}
    return rc, dict(x=x, status=status, start=start, hour=hour, series=series, N=N, cols=cols, consts=consts, state=state), out


@gpu
@pytest.mark.parametrize("p_min_cents", [0, 40000])
@pytest.mark.parametrize("k", [-1, 5])
@pytest.mark.parametrize("S", [1, 2, 3, 16])
def test_curve_and_clearing_kernel_is_the_plain_python_statement(S, k, p_min_cents):
    """dsp_loop_market_clear alone on synthetic solutions - ties, duplicates, rounding boundaries, pairs on both sides of the minimum
    power, coefficients other than 1e-3, a non-zero constant, a one-term period, rows that are not optimal, B not a multiple of 64:
    curves, counts and dispatches equal the plain-Python statement exactly; `bad` is set; the tracker's rows are dispatch - pt_const"""
    from tests._flowsheet_stochastic_oracle import _power, clear, reference_curve
    from tests._stochastic_oracle import host_backcast
    B, T, D = 70, (24 if k < 0 else 4), 16
    fail = tuple(range(S)) + (S * 5, S * 9 + S - 1)                  # plant 0: no row optimal; plants 5 and 9: one row missing
    coef = np.array([[CA, CB]] * T)
    for price_taker in (True, False):
        rc, inp, out = _clear_call(S, B, k, T, p_min_cents=p_min_cents, price_taker=price_taker, fail=set(fail), seed=10 * S + k + 1, D=D,
                                   with_tracker=k >= 0)
        assert rc == 0 and bool(out["bad"])
        hod, day = max(k, 0), inp["hour"] // 24
        below = dropped = 0
        for b in range(B):
            fc = host_backcast(inp["series"], int(inp["start"][b]), day, hod, T, S, D)
            real = inp["series"][(inp["start"][b] + inp["hour"] + np.arange(T)) % inp["N"]]
            ok = inp["status"][b * S:(b + 1) * S] == 0
            xs = inp["x"][b * S:(b + 1) * S]
            for t in range(T):
                power = xs[:, t] if k < 0 else np.array([_power((inp["cols"], coef), inp["consts"], xr, t) for xr in xs])
                U, M = reference_curve(power, fc[:, t], ok, p_min_cents)
                c = int(out["count"][b, t])
                assert (out["curve"][b, t, :c, 0].tolist(), out["curve"][b, t, :c, 1].tolist()) == (U, M), (b, t)
                assert not out["curve"][b, t, c:].any() and U[0] == p_min_cents
                lmp = real[t] if (k < 0 or t == 0) else fc[0, t]
                want = clear(U, M, lmp, "price_taker" if price_taker else "stub")
                assert out["dispatch"][b, t] == want, (b, t)
                below += want < U[-1] / 100.0
                dropped += int((np.round(power[ok] * 100) < p_min_cents - 1).sum())
                if k >= 0:
                    assert out["tr_rlo"][b, 2 * t] == out["tr_rhi"][b, 2 * t] == want - inp["consts"][t], (b, t)
            if k < 0:
                assert np.array_equal(out["da_prices"][b, :T], real)
            else:
                assert out["tr_lb"][b, 7] == out["tr_ub"][b, 7] == inp["state"][b, 0] and out["tr_c0"][b] == 17.5
                assert (out["tr_rlo"][b, 1::2] == -1.0).all() and (np.delete(out["tr_lb"][b], 7) == -1.0).all()
        assert (out["count"][0] == 1).all() and (out["curve"][0, :, 0, 0] == p_min_cents).all() and not out["curve"][0, :, :, 1].any()
        assert (out["dispatch"][0] == p_min_cents / 100.0).all()
        assert (below > 0) == price_taker
        assert p_min_cents == 0 or dropped > 0
        if k < 0:
            assert (out["tr_rlo"] == -1.0).all()


@gpu
def test_entry_points_refuse_malformed_descriptors_on_the_host():
    """DSP_ERR_INVALID and nothing written for a NULL buffer, S / D / T / k out of range, a column outside [0, n), a dispatch row outside
    [0, m), a state column with a NULL state, wind columns with a NULL cf_series - every case is refused BEFORE any launch"""
    from dispatches_amd.hip_solver import DspLoopMarketModel, DspLoopMarketState, load_library

    def field(obj, name, value):
        return lambda st, m, a: setattr(st if obj == "st" else (m if obj == "m" else a["tr"]), name, value)

    def arg(name, value):
        return lambda st, m, a: a.__setitem__(name, value)

    def item(obj, name, at, value):
        def edit(st, m, a):
            target = getattr(m if obj == "m" else a["tr"], name)
            if isinstance(at, tuple):
                target[at[0]][at[1]] = value
            else:
                target[at] = value
        return edit

    def wind_without_series(obj):
        def edit(st, m, a):
            target = m if obj == "m" else a["tr"]
            for t in range(4):
                target.wind_cols[t] = 30 + t
            st.cf_series = None
        return edit

    def untouched(out, keys):
        return all((out[key] == (-7 if key == "curve" else -1)).all() for key in keys)
    common = [field("st", "S", 17), field("st", "S", 0), field("st", "D", 2), field("st", "D", 0), field("st", "N", 24), field("st", "start", None),
              field("st", "hour", None), field("st", "da_series", None), field("st", "rt_series", None), field("st", "p_min_cents", -1),
              field("m", "n", 0), field("m", "T", 49), field("m", "T", 0), field("m", "n_state", 3), field("m", "n_state", -1),
              arg("k", 24), arg("k", -2)]
    clear_only = [field("st", "da_prices", None), field("m", "x", None), field("m", "status", None), arg("curve", None), arg("count", None),
                  arg("dispatch", None), arg("T", 25), arg("T", 0), item("m", "pda_cols", 3, -1), item("m", "pda_cols", 3, 40)]
    for edit in common + clear_only:
        rc, _, out = _clear_call(3, 8, -1, 24, edit=edit)
        assert rc == -1 and untouched(out, ("count", "dispatch", "curve")), edit
    rt_only = [arg("T", 17), arg("T", 5), item("m", "pt_cols", (2, 0), 40), item("m", "pt_cols", (2, 1), -2), field("tr", "T", 3), field("tr", "m", 0),
               field("tr", "n", 0), field("tr", "rlo", None), field("tr", "rhi", None), field("tr", "lb", None), field("tr", "ub", None),
               field("tr", "c0", None), field("tr", "n_state", 2), item("tr", "track_rows", 1, 9), item("tr", "track_rows", 1, -1),
               item("tr", "state_init", 0, 40), item("tr", "state_init", 0, -1), field("st", "state", None), wind_without_series("tr"),
               item("tr", "wind_cols", 0, 40)]
    for edit in rt_only:
        rc, _, out = _clear_call(3, 8, 5, 4, with_tracker=True, edit=edit)
        assert rc == -1 and untouched(out, ("count", "dispatch", "curve", "tr_rlo", "tr_rhi", "tr_lb", "tr_ub", "tr_c0")), edit
    rc, _, _ = _clear_call(3, 8, -1, 24, with_tracker=True)                                        # the day-ahead clearing has no tracker
    assert rc == -1
    rc, _, _ = _clear_call(2, 8, -1, 24, backcast=False)                                           # the perfect forecaster knows one scenario
    assert rc == -1
    prepare_only = [field("m", "c", None), field("m", "lb", None), field("m", "ub", None), field("m", "base_c", None), field("m", "c0", None),
                    field("st", "da_offer", None), field("st", "da_prices", None), field("st", "state", None), item("m", "state_init", 0, 40),
                    item("m", "state_init", 0, -1), item("m", "pda_cols", 3, 40), item("m", "pda_cols", 3, -1), item("m", "pt_cols", (2, 0), 40),
                    item("m", "pt_cols", (2, 1), -2), wind_without_series("m"), item("m", "wind_cols", 0, 40)]
    for edit in common + prepare_only:
        rc, _, out = _clear_call(3, 8, 5, 4, edit=edit, prepare=True)
        assert rc == -1 and untouched(out, ("c", "lb", "ub", "c0")), edit
    rc, _, out = _clear_call(3, 8, 5, 4, prepare=True)                                            # (the unedited descriptor is accepted, and writes)
    assert rc == 0 and (out["c0"] != -1).all() and (out["lb"][:, 38] != -1).all()
    lib = load_library()
    assert lib.dsp_loop_market_prepare(None, None, 0, None) == -1
    assert lib.dsp_loop_market_prepare(C.byref(DspLoopMarketState()), C.byref(DspLoopMarketModel()), 0, None) == -1
    assert lib.dsp_loop_market_clear(None, None, None, 0, 4, None, None, None, None) == -1


@gpu
def test_loop_update_refuses_malformed_descriptors_on_the_host():
    """dsp_loop_update on descriptors of B = 3, rt.T = 4, tr.T = 2, n_state = 1 over buffers filled with a sentinel: with ONE field broken -
    the documented "no such column" -1 in pda_cols, a power term, a dispatch row, a state or wind column outside its buffer, a state
    column with a NULL state - every phase returns DSP_ERR_INVALID and every buffer is still all sentinel (nothing is launched).  A
    tracker of rt.T + 1 periods whose every index is valid (the offer of its last period would silently be pt_const): phases 0 and 1
    refuse it the same way; phase 2, which reads the tracker alone, accepts it.  The unbroken descriptors are accepted by every phase,
    and write"""
    import torch
    from dispatches_amd.hip_solver import DspLoopModel, DspLoopState, load_library
    lib = load_library()
    dev = torch.device("cuda", 0)
    B, n, m, N, SENTINEL = 3, 16, 5, 48, -7.0      # (m = 5 dispatch rows: room for a tracker of rt.T + 1 periods)
    f64 = lambda *shape, fill=SENTINEL: torch.full(shape, fill, dtype=torch.float64, device=dev)

    def call(edit=None, phases=(0, 1, 2)):
        written = {f"{name}_{key}": f64(B, n if key in ("c", "lb", "ub") else m) for name in ("rt", "tr") for key in ("c", "lb", "ub", "rlo", "rhi")}
        written.update(rt_c0=f64(B), tr_c0=f64(B), state=f64(B, 1), delivered=f64(B), revenue=f64(B), energy_mwh=f64(B))
        read = dict(x=f64(B, n, fill=2.0), base_c=f64(n, fill=0.5), series=f64(N, fill=0.25), offers=f64(B, 24, fill=3.0),
                    start=torch.arange(B, dtype=torch.int64, device=dev), hour=torch.zeros((), dtype=torch.int64, device=dev),
                    bad=torch.zeros((), dtype=torch.bool, device=dev), uncertified=torch.zeros((), dtype=torch.int64, device=dev))
        st = DspLoopState()
        st.B, st.N, st.start, st.hour = B, N, read["start"].data_ptr(), read["hour"].data_ptr()
        st.da_series = st.rt_series = st.cf_series = read["series"].data_ptr()
        st.state, st.da_offer, st.da_prices = written["state"].data_ptr(), read["offers"].data_ptr(), read["offers"].data_ptr()
        st.state_scale[0] = st.state_scale[1] = 100.0
        st.delivered, st.revenue, st.energy_mwh = (written[key].data_ptr() for key in ("delivered", "revenue", "energy_mwh"))
        st.bad, st.uncertified = read["bad"].data_ptr(), read["uncertified"].data_ptr()
        rt, tr = DspLoopModel(), DspLoopModel()
        for name, w, T in (("rt", rt, 4), ("tr", tr, 2)):
            w.c, w.lb, w.ub, w.rlo, w.rhi, w.c0 = (written[f"{name}_{key}"].data_ptr() for key in ("c", "lb", "ub", "rlo", "rhi", "c0"))
            w.base_c, w.x = read["base_c"].data_ptr(), read["x"].data_ptr()
            w.n, w.m, w.T, w.n_state = n, m, T, 1
            for t in range(16):
                live = t < T
                w.pt_cols[t][0], w.pt_cols[t][1] = (t if live else -1), (4 + t if live and t % 2 == 0 else -1)     # odd periods have ONE term
                w.pt_coef[t][0], w.pt_coef[t][1], w.pt_const[t] = CA, CB, 0.5
                w.pda_cols[t] = 6 + t if live and name == "rt" else -1
                w.track_rows[t] = 2 * t if live and name == "tr" else -1
                w.wind_cols[t] = 10 + t if live else -1
            w.state_init[0], w.state_real[0] = 14, 15
            w.wind_kw, w.waste_per_kw, w.c0_base = 100.0, 1e-3, 17.5
        if edit is not None:
            edit(st, rt, tr)
        rcs = [lib.dsp_loop_update(C.byref(st), C.byref(rt), C.byref(tr), phase, 5, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
               for phase in phases]
        torch.cuda.synchronize()
        return rcs, {key: v.cpu().numpy() for key, v in written.items()}, int(read["hour"].item())

    def item(which, name, at, value):
        def edit(st, rt, tr):
            target = getattr(rt if which == "rt" else tr, name)
            if isinstance(at, tuple):
                target[at[0]][at[1]] = value
            else:
                target[at] = value
        return edit
    broken = [item("rt", "pda_cols", 1, -1), item("rt", "pt_cols", (2, 1), n), item("tr", "pt_cols", (0, 0), n), item("tr", "track_rows", 0, m),
              item("rt", "state_init", 0, -1), item("tr", "state_init", 0, -1), item("tr", "state_real", 0, n),
              lambda st, rt, tr: setattr(st, "state", None),
              item("tr", "wind_cols", 1, n), item("rt", "wind_cols", 3, -1), lambda st, rt, tr: setattr(st, "cf_series", None)]
    for at, edit in enumerate(broken):
        rcs, out, hour = call(edit)
        assert rcs == [-1, -1, -1] and hour == 0 and all((v == SENTINEL).all() for v in out.values()), at

    def longer_tracker(st, rt, tr):                 # tr.T = rt.T + 1 = 5 and NOTHING else wrong: distinct dispatch rows, columns in range
        tr.T = rt.T + 1
        for t, (row, wind) in enumerate(((0, 10), (2, 11), (1, 12), (3, 13), (4, 9))):
            tr.track_rows[t], tr.wind_cols[t] = row, wind
            tr.pt_cols[t][0], tr.pt_cols[t][1] = t, -1
    rcs, out, hour = call(longer_tracker, phases=(0, 1))
    assert rcs == [-1, -1] and hour == 0 and all((v == SENTINEL).all() for v in out.values())
    rcs, out, hour = call(longer_tracker, phases=(2,))
    assert rcs == [0] and hour == 1 and all((out[key] != SENTINEL).all() for key in ("state", "delivered", "revenue", "energy_mwh"))
    rcs, out, hour = call()
    assert rcs == [0, 0, 0] and hour == 1
    assert all((out[key] != SENTINEL).all() for key in ("rt_c0", "tr_c0", "state", "delivered", "revenue", "energy_mwh"))
    assert (out["rt_ub"][:, 10:14] == 25.0).all() and (out["tr_rlo"][:, [0, 2]] != SENTINEL).all() and (out["tr_rlo"][:, [1, 3, 4]] == SENTINEL).all()


def _snapshot(loop):
    res, ok = loop.results()
    out = {k: v.cpu().numpy().copy() for k, v in res.items()}
    for name, m in (("da", loop.da), ("rt", loop.rt), ("tr", loop.tr)):
        for key in ("c", "lb", "ub", "rlo", "rhi", "c0"):
            out[name + "_" + key] = getattr(m, key).cpu().numpy().copy()
    for key in ("da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch", "da_offer", "da_prices"):
        if hasattr(loop, key):
            out[key] = getattr(loop, key).cpu().numpy().copy()
    out["uncertified"] = np.array(int(loop.uncertified.item()))
    return out, ok


SUMS = ("obj", "energy_mwh", "offered_mwh", "da_energy_mwh")       # accumulated by phase 2 of dsp_loop_update / sums of cleared dispatches


@gpu
@pytest.mark.parametrize("market", ["price_taker", "stub"])
@pytest.mark.parametrize("flowsheet", FLOWSHEETS)
def test_stochastic_kernels_and_graphs_are_bit_identical_to_the_tensor_operations(flowsheet, market):
    """use_fused True / False and graph replay / eager, B = 96, S = 3, three days (the third is a replay of graphs captured on the
    second): objective vectors, constants, bounds, tracker rows, curves, counts, dispatches, day-ahead offers and prices and the state
    bit for bit; the accumulated sums identical between graph and eager, and to rtol 1e-12 / atol 1e-9 between kernels and tensor
    operations (phase 2 of dsp_loop_update associates its sums differently: the tolerance of the deterministic loop's test)"""
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    B, days = 96, 3
    runs = {}
    for fused, graphs in ((False, False), (True, False), (True, True)):
        loop = BatchedDoubleLoop(flowsheet, B, device=0, use_graphs=graphs, use_fused=fused, n_price_scenarios=3, forecaster="backcast", market=market)
        assert loop.use_fused == fused and loop.stochastic
        for _ in range(days):
            loop.run_day()
        assert int(loop.hour_t.item()) == 24 * days and len(loop._graphs) == (25 if graphs else 0)
        runs[fused, graphs], ok = _snapshot(loop)
        assert ok and int(loop.uncertified.item()) == 0
    base = runs[False, False]
    assert np.abs(base["obj"]).max() > 0 and (base["da_count"] >= 1).all() and (flowsheet == "wind_pem" or (base["da_count"] > 2).any())
    for k in base:
        if k in SUMS:
            assert np.array_equal(runs[True, False][k], runs[True, True][k]), k
            np.testing.assert_allclose(runs[True, False][k], base[k], rtol=1e-12, atol=1e-9, err_msg=k)
        else:
            for key, other in runs.items():
                assert np.array_equal(base[k], other[k]), (key, k)


@gpu
@pytest.mark.parametrize("flowsheet", ["nuclear", "wind_pem"])
def test_oracle_walk_on_the_device(flowsheet):
    """B = 12, S = 3, D = 10, two days, the second replayed from graphs: every LP against the oracle's own at 1e-6, curves and
    dispatches exact from the read-back solutions, all optimal, not vacuous"""
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from tests._flowsheet_stochastic_oracle import oracle_walk
    loop = BatchedDoubleLoop(flowsheet, 12, device=0, n_price_scenarios=3, forecaster="backcast", max_historical_days=10, market="price_taker")
    assert loop.use_fused and loop.use_graphs
    seen = oracle_walk(loop, 2)
    print("stochastic", flowsheet, "loop on the device:", {k: v for k, v in seen.items() if k != "first_powers"})
    res, ok = loop.results()
    assert ok and seen["all_optimal"] and int(loop.uncertified.item()) == 0 and len(loop._graphs) == 25
    assert seen["worst"] <= 1e-6
    assert seen["forecast_differs"] > 0.5 * seen["forecast_hours"] and seen["below"] >= 1 and seen["equal"] >= 1, seen
    if flowsheet == "nuclear":
        assert seen["three"] >= 1 and seen["first_powers"] == {40000}, seen


@gpu
def test_longer_nuclear_run_leaves_the_deterministic_loop_alone():
    """256 nuclear plants x S = 3, 10 days from graphs: all optimal, the market leaves offered energy on the table; a default-argument
    loop of 64 plants run in the same process before and after it gives identical results"""
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop

    def deterministic():
        loop = BatchedDoubleLoop("nuclear", 64, device=0)
        for _ in range(3):
            loop.run_day()
        out, ok = _snapshot(loop)
        assert ok and not loop.stochastic and sorted(loop.results()[0]) == ["energy_mwh", "obj", "state"]
        return out
    before = deterministic()
    loop = BatchedDoubleLoop("nuclear", 256, device=0, n_price_scenarios=3, forecaster="backcast", market="price_taker")
    for _ in range(10):
        loop.run_day()
    res, ok = loop.results()
    assert ok and loop.hour == 240 and int(loop.hour_t.item()) == 240
    assert (res["da_energy_mwh"] <= res["offered_mwh"]).all() and (res["da_energy_mwh"] < res["offered_mwh"]).any()
    assert float(res["obj"].abs().max().item()) > 0
    after = deterministic()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
