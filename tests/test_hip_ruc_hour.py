"""GPU tests of BatchedDoubleLoop(..., ruc_hour=H) (dsp_loop_project, dsp_loop_market_state::rt_history_lag_days; ABI 17): the new entry
point alone on synthetic inputs against its statement in numpy, the kernels against the tensor form and graph replay against the eager
loop bit for bit, the chain and the bid walked against the oracle on the device, day 0 and the stateless wind + PEM loop against the
default loop, and a sized wind + battery batch."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
MODES = {"S1": dict(n_price_scenarios=1, forecaster="perfect"), "S3": dict(n_price_scenarios=3, forecaster="backcast")}
B70 = 70                                                                   # 280 tracker lanes (T = 4): across the 256-lane block edge


# ---- dsp_loop_project alone ---------------------------------------------------------------------------------------------------------------
def _project_case(B, H, wind, n_state, sized, seed):
    """synthetic descriptors on live device buffers and the same inputs on the host"""
    import torch
    from dispatches_amd.hip_solver import DspLoopModel, DspLoopProjectState
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", 0)
    n, m, T, N, L, slots = 23, 11, 4, 97, 24 - H, 4
    host = dict(start=rng.integers(0, N, B), hour=np.array(24 * 3 + H), cf=rng.random(N), state=np.round(rng.random((B, n_state)) * 1e5, 2),
                da_offer=np.round(rng.random((B, 24)) * 300, 2), x=rng.random((L, B, n)) * 1e5, obj=rng.standard_normal((L, B)) * 1e4,
                status=(rng.random((L, B)) < 0.02).astype(np.int32), flags=(rng.random((L, B)) < 0.05).astype(np.int32),
                kw_plant=rng.uniform(5e4, 4e5, B), c0_plant=rng.uniform(10, 500, B), pt_const=rng.standard_normal(T),
                pend_offer=rng.random((B, 24)), pend_prices=rng.random((B, 24)), pend_curve=rng.integers(0, 9999, (B, 24, slots, 2)).astype(np.int32),
                pend_count=rng.integers(1, slots + 1, (B, 24)).astype(np.int32))
    host["status"][:, 0], host["flags"][0, -1] = 0, 1
    cols = rng.permutation(n)
    host.update(track_rows=rng.permutation(m)[:T], wind_cols=cols[:T], state_init=cols[T:T + 2], state_real=cols[T + 2:T + 4],
                scale=[100.0, 1.0], wind_kw=2e5, c0_base=123.25, waste=1e-3 * 1e3 + 0.125)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    d = {k: t(host[k]) for k in ("start", "hour", "cf", "state", "da_offer", "kw_plant", "c0_plant", "pend_offer", "pend_prices", "pend_curve", "pend_count")}
    z = lambda *shape, dtype=torch.float64: torch.full(shape, -7, dtype=dtype, device=dev)
    d.update(lb=z(B, n), ub=z(B, n), rlo=z(B, m), rhi=z(B, m), c0=z(B), x=z(B, n), obj=z(B), status=z(B, dtype=torch.int32), flags=z(B, dtype=torch.int32),
             proj_state=z(L + 1, B, n_state), proj_real=z(L, B, n_state), proj_obj=z(L, B), bad=torch.zeros((), dtype=torch.uint8, device=dev),
             uncertified=torch.zeros((), dtype=torch.int64, device=dev), cur_offer=d["da_offer"].clone(), da_prices=z(B, 24),
             da_curve=z(B, 24, slots, 2, dtype=torch.int32), da_count=z(B, 24, dtype=torch.int32))
    pj = DspLoopModel()
    for name in ("lb", "ub", "rlo", "rhi", "c0", "x", "status", "flags"):
        setattr(pj, name, d[name].data_ptr())
    pj.n, pj.m, pj.T, pj.n_state = n, m, T, n_state
    for q in range(16):
        pj.track_rows[q] = int(host["track_rows"][q]) if q < T else -1
        pj.wind_cols[q] = int(host["wind_cols"][q]) if wind and q < T else -1
        pj.pt_const[q] = float(host["pt_const"][q]) if q < T else 0.0
        pj.pt_cols[q][0] = pj.pt_cols[q][1] = pj.pda_cols[q] = -1
    for e in range(2):
        pj.state_init[e], pj.state_real[e] = int(host["state_init"][e]), int(host["state_real"][e])
    pj.wind_kw, pj.c0_base, pj.waste_per_kw = host["wind_kw"], host["c0_base"], host["waste"]
    if sized:
        pj.wind_kw_plant, pj.c0_base_plant = d["kw_plant"].data_ptr(), d["c0_plant"].data_ptr()
    st = DspLoopProjectState()
    st.B, st.N, st.ruc_hour, st.slots = B, N, H, slots
    st.start, st.hour, st.cf_series = d["start"].data_ptr(), d["hour"].data_ptr(), d["cf"].data_ptr() if wind else None
    st.state = d["state"].data_ptr() if n_state else None
    st.state_scale[0], st.state_scale[1] = host["scale"]
    st.obj, st.proj_state, st.proj_real, st.proj_obj = (d[k].data_ptr() for k in ("obj", "proj_state", "proj_real", "proj_obj"))
    st.bad, st.uncertified = d["bad"].data_ptr(), d["uncertified"].data_ptr()
    st.da_offer, st.da_prices, st.pend_offer, st.pend_prices = (d[k].data_ptr() for k in ("cur_offer", "da_prices", "pend_offer", "pend_prices"))
    st.da_curve, st.da_count, st.pend_curve, st.pend_count = (d[k].data_ptr() for k in ("da_curve", "da_count", "pend_curve", "pend_count"))
    return host, d, st, pj, dict(n=n, m=m, T=T, N=N, L=L)


@gpu
@pytest.mark.parametrize("H", [16, 23])
@pytest.mark.parametrize("B", [1, B70, 257])
def test_dsp_loop_project_is_its_statement(B, H):
    """every phase of the entry point on synthetic inputs against numpy, bit for bit: B = 70 x T = 4 crosses the 256-lane block edge in
    the write phase, B = 257 in the per-plant phase; H = 23 is one window with one dispatch and three free rows; with and without wind
    columns, 0 / 1 / 2 state columns, scalar and per-plant sizes.  What a phase does not own keeps its fill value."""
    import torch
    from dispatches_amd.hip_solver import load_library
    lib = load_library()
    seed = 0
    for wind, sized in ((True, False), (True, True), (False, False)):
        for n_state in (0, 1, 2):
            seed += 1
            host, d, st, pj, dim = _project_case(B, H, wind, n_state, sized, 1000 * H + 10 * B + seed)
            T, N, L = dim["T"], dim["N"], dim["L"]
            kw = host["kw_plant"] if sized else np.full(B, host["wind_kw"])
            base = host["c0_plant"] if sized else np.full(B, host["c0_base"])
            scale = np.array(host["scale"][:n_state])
            ps = np.full((L + 1, B, n_state), -7.0)
            ps[0] = host["state"]
            bad, uncertified = 0, 0
            for j in range(L):
                assert lib.dsp_loop_project(C.byref(st), C.byref(pj), 0, j, None) == 0
                got = {k: d[k].cpu().numpy() for k in ("lb", "ub", "rlo", "rhi", "c0")}
                rlo, rhi = np.full((B, dim["m"]), -7.0), np.full((B, dim["m"]), -7.0)
                for t in range(T):
                    at = H + j + t
                    rhs = host["da_offer"][:, at] - host["pt_const"][t] if at < 24 else None
                    rlo[:, host["track_rows"][t]] = rhs if at < 24 else -np.inf
                    rhi[:, host["track_rows"][t]] = rhs if at < 24 else np.inf
                assert np.array_equal(got["rlo"], rlo) and np.array_equal(got["rhi"], rhi), (wind, n_state, sized, j)
                lb, ub = np.full((B, dim["n"]), -7.0), np.full((B, dim["n"]), -7.0)
                c0 = base.copy()
                if wind:
                    avail = kw[:, None] * host["cf"][(host["start"][:, None] + int(host["hour"]) + j + np.arange(T)[None, :]) % N]
                    ub[:, host["wind_cols"]] = avail
                    total = avail[:, 0].copy()
                    for t in range(1, T):
                        total = total + avail[:, t]
                    c0 = c0 + host["waste"] * total
                for e in range(n_state):
                    lb[:, host["state_init"][e]] = ps[j, :, e]
                    ub[:, host["state_init"][e]] = ps[j, :, e]
                assert np.array_equal(got["lb"], lb) and np.array_equal(got["ub"], ub) and np.array_equal(got["c0"], c0), (wind, n_state, sized, j)
                # the "solve": this step's synthetic outputs
                for k in ("x", "obj", "status", "flags"):
                    d[k].copy_(torch.as_tensor(host[k][j], device=d[k].device))
                assert lib.dsp_loop_project(C.byref(st), C.byref(pj), 1, j, None) == 0
                real = host["x"][j][:, host["state_real"][:n_state]]
                ps[j + 1] = np.round(real * scale) / scale
                bad |= int(host["status"][j].any())
                uncertified += int((host["flags"][j] & 1).sum())
                assert np.array_equal(d["proj_real"].cpu().numpy()[j], real) and np.array_equal(d["proj_obj"].cpu().numpy()[j], host["obj"][j] + c0)
                assert np.array_equal(d["proj_state"].cpu().numpy()[:j + 2], ps[:j + 2])
                assert int(d["bad"].item()) == bad and int(d["uncertified"].item()) == uncertified
            assert uncertified > 0
            assert (d["da_prices"] == -7).all() and (d["da_count"] == -7).all() and np.array_equal(d["cur_offer"].cpu().numpy(), host["da_offer"])
            assert lib.dsp_loop_project(C.byref(st), None, 2, 0, None) == 0
            for cur, pend in (("cur_offer", "pend_offer"), ("da_prices", "pend_prices"), ("da_curve", "pend_curve"), ("da_count", "pend_count")):
                assert np.array_equal(d[cur].cpu().numpy(), host[pend]), cur
            st.slots = 0                             # a loop without curves: offers and prices only
            d["da_count"].fill_(-7), d["cur_offer"].fill_(-7)
            assert lib.dsp_loop_project(C.byref(st), None, 2, 0, None) == 0
            assert (d["da_count"] == -7).all() and np.array_equal(d["cur_offer"].cpu().numpy(), host["pend_offer"])
            # a refused call writes nothing
            d["c0"].fill_(-7)
            pj.track_rows[T - 1] = dim["m"]
            assert lib.dsp_loop_project(C.byref(st), C.byref(pj), 0, 0, None) == -1 and (d["c0"] == -7).all()


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def _loop(flowsheet, market, mode, H=16, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    return BatchedDoubleLoop(flowsheet, kw.pop("B", B70), device=0, market=market, ruc_hour=H, **MODES[mode], **kw)


def _snap(loop):
    """what the mode writes (and the state it starts from), as host copies"""
    out = {k: getattr(loop, k).cpu().numpy().copy() for k in ("proj_state", "pend_offer", "pend_prices", "da_offer", "da_prices", "state", "bid_hour_t")}
    for key in ("lb", "ub", "rlo", "rhi", "c0"):
        out["pj_" + key] = getattr(loop.pj, key).cpu().numpy().copy()
    if loop.stochastic:
        for key in ("pend_curve", "pend_count", "da_curve", "da_count", "da_energy_mwh", "offered_mwh"):
            out[key] = getattr(loop, key).cpu().numpy().copy()
    ok = loop.results()[1]
    assert ok and int(loop.uncertified.item()) == 0
    return out


class _Once:
    """one run per key for the whole module; a run that failed is not started again - its exception is raised to every test that asks"""

    def __init__(self, run):
        self.run, self.done = run, {}

    def __call__(self, *key):
        if key not in self.done:
            try:
                self.done[key] = (self.run(*key), None)
            except BaseException as exc:                  # noqa: B902 (kept, and raised again below)
                self.done[key] = (None, exc)
        value, exc = self.done[key]
        if exc is not None:
            raise exc
        return value


def _run_eager(flowsheet, market, mode):
    loop = _loop(flowsheet, market, mode, use_graphs=False, use_fused=True)
    assert loop.use_fused and not loop._graphs
    snaps = {}
    for day in (1, 2, 3):
        loop.run_day()
        if day >= 2:
            snaps[day] = _snap(loop)
    return snaps


@pytest.fixture(scope="module")
def eager_fused():
    """(flowsheet, market, mode) -> {2: snapshot after two days, 3: after three} of the eager kernels: run once, shared, not modified"""
    return _Once(_run_eager)


@gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("market", ["price_taker", "stub"])
@pytest.mark.parametrize("flowsheet", ["wind_battery", "wind_pem", "nuclear"])
def test_kernels_are_bit_identical_to_the_tensor_form(flowsheet, market, mode, eager_fused):
    """70 plants, two days without graphs, use_fused True / False: the trace, the projection model's bounds, rows and constants, the
    pending and the current offers, prices, curves and counts, the bid clock - bit for bit"""
    fused = eager_fused(flowsheet, market, mode)[2]
    loop = _loop(flowsheet, market, mode, use_graphs=False, use_fused=False)
    assert not loop.use_fused
    for _ in range(2):
        loop.run_day()
    base = _snap(loop)
    assert set(base) == set(fused) and int(base["bid_hour_t"]) == 48
    for k in base:
        assert np.array_equal(base[k], fused[k]), (flowsheet, market, mode, k)
    assert np.abs(base["pend_offer"]).max() > 0 and (base["pend_offer"] != base["da_offer"]).any()
    if flowsheet != "wind_pem":
        rows = loop.pj.track_rows.cpu().numpy()
        assert np.isneginf(base["pj_rlo"][:, rows[1:]]).all() and np.isposinf(base["pj_rhi"][:, rows[1:]]).all()     # the last window: one dispatch
        assert np.isfinite(base["pj_rlo"][:, rows[0]]).all() and (base["proj_state"][-1] != base["proj_state"][0]).any()


@gpu
@pytest.mark.parametrize("market,mode", [("price_taker", "S3"), ("stub", "S1")])
@pytest.mark.parametrize("flowsheet", ["wind_battery", "wind_pem", "nuclear"])
def test_graph_replay_is_the_eager_loop(flowsheet, market, mode, eager_fused):
    """three days: day 0 eager, day 1 captured (the chain, the bid and the activation among the graphs), day 2 replayed - bit for bit"""
    eager = eager_fused(flowsheet, market, mode)[3]
    loop = _loop(flowsheet, market, mode, use_graphs=True, use_fused=True)
    for _ in range(3):
        loop.run_day()
    assert sorted(loop._graphs, key=str) == sorted(list(range(24)) + ["activate"], key=str) and int(loop.hour_t.item()) == 72
    replay = _snap(loop)
    assert set(replay) == set(eager)
    for k in eager:
        assert np.array_equal(eager[k], replay[k]), (flowsheet, market, mode, k)


@gpu
@pytest.mark.parametrize("H", [16, 23])
@pytest.mark.parametrize("flowsheet", ["wind_battery", "nuclear"])
def test_walk_on_the_device(flowsheet, H):
    """the CPU walk on the device (1e-6, the parity contract of every device walk): 70 plants, S = 3, price taker, two days, plants 0, 1,
    63, 64 (both sides of a wave edge) and 69 - every chain LP, with its free rows, every LP of the pending bid, curves and dispatches
    exactly; all optimal, nothing uncertified"""
    from tests._projection_oracle import ruc_walk
    loop = _loop(flowsheet, "price_taker", "S3", H=H)
    assert loop.use_fused and loop.use_graphs
    plants = [0, 1, 63, 64, 69]
    seen = ruc_walk(loop, 2, plants=plants, tol=1e-6)
    print("ruc_hour walk on the device:", flowsheet, H, {k: seen[k] for k in ("worst", "lps", "curves", "free_rows", "midnight_windows")})
    assert loop.results()[1] and seen["all_optimal"] and int(loop.uncertified.item()) == 0
    assert seen["worst"] <= 1e-6 and seen["lps"] == 2 * len(plants) * (24 - H + 3) and seen["curves"] == 2 * len(plants) * 24
    free = sum(loop.tr.T - min(loop.tr.T, 24 - H - j) for j in range(24 - H))       # 1 + 2 + 3 at H = 16, one window with 3 at H = 23
    assert seen["projected_moves"] and seen["free_rows"] == 2 * len(plants) * free and free == (6 if H == 16 else 3) and seen["rt_lag_differs"] > 0


@gpu
@pytest.mark.parametrize("mode,market", [("S1", "stub"), ("S3", "price_taker")])
@pytest.mark.parametrize("flowsheet", ["wind_battery", "wind_pem", "nuclear"])
def test_day_0_is_the_default_loops_on_the_device(flowsheet, mode, market):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    a = _loop(flowsheet, market, mode)
    b = BatchedDoubleLoop(flowsheet, B70, device=0, market=market, **MODES[mode])
    a.run_day(), b.run_day()
    for name in ("state", "revenue", "energy_mwh", "delivered", "da_offer", "da_prices"):
        assert np.array_equal(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()), name
    assert a.results()[1] and b.results()[1] and int(a.uncertified.item()) == 0


@gpu
@pytest.mark.parametrize("market", ["stub", "price_taker"])
def test_wind_pem_on_a_perfect_forecast_is_invariant_on_the_device(market):
    """no state, the same windows, the solves in the same order: three days (eager, captured, replayed) of results() bit for bit"""
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    a = _loop("wind_pem", market, "S1")
    b = BatchedDoubleLoop("wind_pem", B70, device=0, market=market, **MODES["S1"])
    for _ in range(3):
        a.run_day(), b.run_day()
    (ra, oka), (rb, okb) = a.results(), b.results()
    assert oka and okb and sorted(ra) == sorted(rb)
    for key in ra:
        assert np.array_equal(ra[key].cpu().numpy(), rb[key].cpu().numpy()), key
    assert np.array_equal(a.da_offer.cpu().numpy(), b.da_offer.cpu().numpy())


@gpu
def test_sized_batch():
    """3 wind x 3 battery x 2 durations x 5 windows = 90 plants of their own size, S = 3, ruc_hour = 16: kernels = tensor form after two
    days, and the walk on the smallest and the largest battery (the projection tracker carries each plant's own bounds and constants)"""
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from dispatches_amd.sweeps import design_layout
    from tests._projection_oracle import ruc_walk
    wind, batt, mwh, win = design_layout([50.0, 200.0, 400.0], [5.0, 25.0, 100.0], [2.0, 4.0], 5)
    kw = dict(device=0, market="price_taker", ruc_hour=16, plant_windows=win, wind_mw=wind, battery_mw=batt, battery_mwh=mwh, **MODES["S3"])
    fused = BatchedDoubleLoop("wind_battery", 90, use_graphs=False, **kw)
    plain = BatchedDoubleLoop("wind_battery", 90, use_graphs=False, use_fused=False, **kw)
    assert fused.use_fused and fused.sized and bool(fused._loop_pj.wind_kw_plant) and mwh[0] == mwh.min() and mwh[89] == mwh.max()
    for _ in range(2):
        fused.run_day(), plain.run_day()
    a, b = _snap(fused), _snap(plain)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    soc = a["proj_state"][-1, :, 0]
    assert (soc <= mwh * 1e3).all() and len(set(a["pj_c0"].tolist())) > 3
    loop = BatchedDoubleLoop("wind_battery", 90, **kw)
    seen = ruc_walk(loop, 2, plants=[0, 89], tol=1e-6)
    print("sized ruc_hour walk on the device:", {k: seen[k] for k in ("worst", "lps", "curves")})
    assert loop.results()[1] and seen["all_optimal"] and int(loop.uncertified.item()) == 0 and seen["worst"] <= 1e-6
    assert seen["lps"] == 2 * 2 * (8 + 3) and seen["projected_moves"]
