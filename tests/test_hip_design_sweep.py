"""GPU tests of the per-plant sizes of the LP-bidding double loop (BatchedDoubleLoop(wind_mw=, battery_mw=, battery_mwh=); dsp_loop_model /
dsp_loop_market_model: wind_kw_plant, c0_base_plant, ABI 16): the kernels against the tensor form bit for bit on a design grid of 90
different plants, graph replay against the eager loop, the oracle walk on the device, the default loop against the same plant passed as
arrays (NULL branch = pointer branch), the refusals of the entry points on the host; and the DETERMINISTIC sized loop (the class defaults:
perfect forecaster, stub market), the only path on which phases 0 and 1 of dsp_loop_update read the per-plant pointers."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast")
DETERMINISTIC = dict(n_price_scenarios=1, forecaster="perfect")
WINDS, BATTS, DURS, WINDOWS = [50.0, 200.0, 400.0], [5.0, 25.0, 100.0], [2.0, 4.0], 5      # 90 plants, 270 bidding rows: more than one
#                                                                                          256-thread block, not a multiple of 64


def _grid_loop(flowsheet, market, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from dispatches_amd.sweeps import design_layout
    if flowsheet == "wind_pem":                                       # the wind axis only: 3 sizes x 30 windows
        wind, _, _, win = design_layout([300.0, 847.0, 1200.0], [0.0], [0.0], 30)
        sizes = dict(wind_mw=wind)
    else:
        wind, batt, mwh, win = design_layout(WINDS, BATTS, DURS, WINDOWS)
        sizes = dict(wind_mw=wind, battery_mw=batt, battery_mwh=mwh)
    mode = {k: kw.pop(k, v) for k, v in STOCHASTIC.items()}
    loop = BatchedDoubleLoop(flowsheet, 90, device=0, market=market, plant_windows=win, **sizes, **mode, **kw)
    assert loop.B == 90 and loop.sized and (loop.S == 1 or loop.B * loop.S == 270)
    return loop


def _snap(loop):
    """everything a step writes, as host copies"""
    res, ok = loop.results()
    out = {k: v.cpu().numpy().copy() for k, v in res.items()}
    for name, m in (("da", loop.da), ("rt", loop.rt), ("tr", loop.tr)):
        for key in ("c", "lb", "ub", "rlo", "rhi", "c0"):
            out[name + "_" + key] = getattr(m, key).cpu().numpy().copy()
    for key in ("da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch", "da_offer", "da_prices", "delivered"):
        if hasattr(loop, key):
            out[key] = getattr(loop, key).cpu().numpy().copy()
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


def _run_eager(flowsheet, market, **mode):
    """the kernels without graphs on the 90-plant grid: snapshots after two and after three days"""
    loop = _grid_loop(flowsheet, market, use_graphs=False, use_fused=True, **mode)
    assert loop.use_fused and not loop._graphs
    snaps = {}
    for day in (1, 2, 3):
        loop.run_day()
        if day >= 2:
            snaps[day] = _snap(loop)
    return snaps


@pytest.fixture(scope="module")
def eager_fused():
    """(flowsheet, market) -> {2: snapshot after two days, 3: after three} of the eager kernels: run once, shared, not modified"""
    return _Once(_run_eager)


@pytest.fixture(scope="module")
def eager_deterministic():
    """flowsheet -> the same for the deterministic sized loop"""
    return _Once(lambda flowsheet: _run_eager(flowsheet, "stub", **DETERMINISTIC))


@gpu
@pytest.mark.parametrize("market", ["price_taker", "stub"])
@pytest.mark.parametrize("flowsheet", ["wind_battery", "wind_pem"])
def test_sized_kernels_are_bit_identical_to_the_tensor_form(flowsheet, market, eager_fused):
    """90 plants of different sizes, S = 3, two days without graphs, use_fused True / False: every plant's objective vectors, constants,
    bounds (the static battery bounds among them), tracker rows, curves, counts, dispatches, offers, state, delivered power AND the
    accumulated revenue and energies bit for bit (a sized batch's tensor form states phase 2 of dsp_loop_update in its fused arithmetic)"""
    fused = eager_fused(flowsheet, market)[2]
    loop = _grid_loop(flowsheet, market, use_graphs=False, use_fused=False)
    assert not loop.use_fused
    for _ in range(2):
        loop.run_day()
    base = _snap(loop)
    assert np.abs(base["obj"]).max() > 0 and (base["da_count"] >= 1).all() and set(base) == set(fused)
    for k in base:
        assert np.array_equal(base[k], fused[k]), (flowsheet, market, k)
    # not vacuous: the plants differ where the sizes enter
    kw = loop.wind_mw * 1e3
    assert len(set(base["tr_c0"].tolist())) > 3 and len(set(base["da_c0"].tolist())) > 3
    wind_cols = loop.tr.wind[0].cpu().numpy()
    cf = loop.cf_series.cpu().numpy()[(loop.start.cpu().numpy()[:, None] + 47 + np.arange(loop.tr.T)[None, :]) % loop.N]      # the last hour's window
    assert cf.max() > 0 and np.array_equal(base["tr_ub"][:, wind_cols], kw[:, None] * cf) and len(set(kw.tolist())) == 3
    if flowsheet == "wind_battery":
        for name, m, per in (("da", loop.da, 3), ("rt", loop.rt, 3), ("tr", loop.tr, 1)):
            assert np.array_equal(base[name + "_ub"][:, m.batt_cols], np.repeat(loop.battery_mw * 1e3, per)[:, None] * np.ones(len(m.batt_cols)))
            assert np.array_equal(base[name + "_rhi"][:, m.soc_rows], np.repeat(loop.battery_mwh * 1e3, per)[:, None] * np.ones(len(m.soc_rows)))
        assert len(set(np.round(base["obj"], 6).tolist())) > 30            # the grid is not one plant repeated
        assert (base["state"][:, 0] <= loop.battery_mwh * 1e3 + 1e-6).all()


@gpu
@pytest.mark.parametrize("market", ["price_taker", "stub"])
@pytest.mark.parametrize("flowsheet", ["wind_battery", "wind_pem"])
def test_sized_graph_replay_is_the_eager_loop(flowsheet, market, eager_fused):
    """the same batch, three days: captured on the second day, replayed on the third - everything bit for bit, sums included"""
    eager = eager_fused(flowsheet, market)[3]
    loop = _grid_loop(flowsheet, market, use_graphs=True, use_fused=True)
    for _ in range(3):
        loop.run_day()
    assert len(loop._graphs) == 25 and int(loop.hour_t.item()) == 72
    replay = _snap(loop)
    assert set(replay) == set(eager)
    for k in eager:
        assert np.array_equal(eager[k], replay[k]), (flowsheet, market, k)


@gpu
@pytest.mark.parametrize("flowsheet", ["wind_battery", "wind_pem"])
def test_sized_deterministic_kernels_match_the_tensor_form(flowsheet, eager_deterministic):
    """The sized loop with the class defaults (perfect forecaster, stub market): phases 0 and 1 of dsp_loop_update read c0_base_plant[b]
    and wind_kw_plant[b] (loop_update_kernel, loop_state_and_wind) - no other path does.  90 plants of three wind sizes, two days,
    use_fused True / False as tests/test_hip_rolling.py does for the default loop: the realised states equal, revenue, energy and the
    objective constants to 1e-12 (the kernel adds with fma), and what the kernel writes WITHOUT a sum exactly: the wind columns' upper
    bounds kw[b] * cf and the state columns' bounds.  Then per plant, from the plant's own numbers: the tracker's constant is
    c0_plant[b] + per_kw * sum_t kw[b] cf[t] - a wrong index or the other model's pointer would show here."""
    fused = eager_deterministic(flowsheet)[2]
    loop = _grid_loop(flowsheet, "stub", use_graphs=False, use_fused=False, **DETERMINISTIC)
    assert not loop.use_fused and not loop.stochastic and loop.S == 1
    for _ in range(2):
        loop.run_day()
    base = _snap(loop)
    assert set(base) == set(fused) and np.abs(base["obj"]).max() > 0
    assert np.array_equal(base["state"], fused["state"])
    for k in ("obj", "energy_mwh"):
        np.testing.assert_allclose(fused[k], base[k], rtol=1e-12, atol=1e-9, err_msg=k)
    kw = loop.wind_mw * 1e3
    start = loop.start.cpu().numpy()
    for name, m in (("rt", loop.rt), ("tr", loop.tr)):
        np.testing.assert_allclose(fused[name + "_c0"], base[name + "_c0"], rtol=1e-12, err_msg=name)
        wind_cols = m.wind[0].cpu().numpy()
        cf = loop.cf_series.cpu().numpy()[(start[:, None] + 47 + np.arange(m.T)[None, :]) % loop.N]        # the window of the last hour
        assert cf.max() > 0 and np.array_equal(fused[name + "_ub"][:, wind_cols], kw[:, None] * cf), name
        assert np.array_equal(fused[name + "_ub"][:, wind_cols], base[name + "_ub"][:, wind_cols]), name
        for key in ("_lb", "_ub"):
            assert np.array_equal(fused[name + key][:, m.state_init], base[name + key][:, m.state_init]), (name, key)
        if name == "tr":                                  # (the real-time constant also carries the prices' share: compared above)
            want = m.c0_plant.cpu().numpy() + m.wind[2] * (kw[:, None] * cf).sum(1)
            np.testing.assert_allclose(fused["tr_c0"], want, rtol=1e-12)
            assert len(set(m.c0_plant.cpu().numpy().tolist())) == 3 and len(set(kw.tolist())) == 3
    # the two models' constants differ per plant (T differs for the day-ahead one only; rt and tr share T = 4, so compare with da)
    assert not np.array_equal(loop.da.c0_plant.cpu().numpy(), loop.tr.c0_plant.cpu().numpy())
    if flowsheet == "wind_battery":
        for name, m in (("da", loop.da), ("rt", loop.rt), ("tr", loop.tr)):
            assert np.array_equal(fused[name + "_ub"][:, m.batt_cols], (loop.battery_mw * 1e3)[:, None] * np.ones(len(m.batt_cols)))
            assert np.array_equal(fused[name + "_rhi"][:, m.soc_rows], (loop.battery_mwh * 1e3)[:, None] * np.ones(len(m.soc_rows)))


@gpu
@pytest.mark.parametrize("flowsheet", ["wind_battery", "wind_pem"])
def test_sized_deterministic_graph_replay_is_the_eager_loop(flowsheet, eager_deterministic):
    """the plainest sized call, BatchedDoubleLoop(flowsheet, B, wind_mw=...), three days: captured on the second, replayed on the third -
    bit for bit with the eager kernels (the graphs hold the per-plant pointers by value in the descriptors)"""
    eager = eager_deterministic(flowsheet)[3]
    loop = _grid_loop(flowsheet, "stub", use_graphs=True, use_fused=True, **DETERMINISTIC)
    for _ in range(3):
        loop.run_day()
    assert len(loop._graphs) == 25 and int(loop.hour_t.item()) == 72
    replay = _snap(loop)
    assert set(replay) == set(eager)
    for k in eager:
        assert np.array_equal(eager[k], replay[k]), (flowsheet, k)


@gpu
@pytest.mark.parametrize("flowsheet", ["wind_battery", "wind_pem"])
def test_deterministic_walk_on_the_device(flowsheet):
    """the deterministic sized loop on the device, six hours, six plants (first, last, both neighbours of a wind-size boundary, smallest
    and largest battery): the day-ahead and every hourly real-time and tracking objective against the oracle's LP of THAT plant's size"""
    from tests._design_oracle import deterministic_walk
    loop = _grid_loop(flowsheet, "stub", **DETERMINISTIC)
    assert loop.use_fused and not loop.stochastic
    plants = [0, 4, 29, 30, 85, 89]
    assert loop.wind_mw[29] != loop.wind_mw[30]
    seen = deterministic_walk(loop, 6, plants=plants)
    print("deterministic sized", flowsheet, "loop on the device:", {k: v for k, v in seen.items() if k in ("worst", "lps")})
    assert loop.results()[1] and seen["all_optimal"] and int(loop.uncertified.item()) == 0
    assert seen["worst"] <= 1e-6 and seen["lps"] == len(plants) * (1 + 2 * 6)
    assert len({seen["da_c0"][b] for b in (0, 30, 89)}) == 3


@gpu
def test_design_walk_on_the_device():
    """one day on the device, six plants of the 90-plant grid walked against the oracle's LPs of THEIR size: the first, the last, the three
    whose bidding rows lie around row 256 (plant 85 holds rows 255 .. 257: both blocks), the smallest and the largest battery - every
    LP within 1e-6, curves and dispatches exact, all optimal, nothing uncertified"""
    from tests._design_oracle import design_walk
    loop = _grid_loop("wind_battery", "price_taker")
    assert loop.use_fused and loop.use_graphs
    plants = [0, 4, 84, 85, 86, 89]
    assert loop.battery_mwh[0] == loop.battery_mwh.min() and loop.battery_mwh[89] == loop.battery_mwh.max() and 85 * 3 <= 256 < 86 * 3
    seen = design_walk(loop, 1, plants=plants)
    print("sized loop on the device:", {k: v for k, v in seen.items() if k in ("worst", "lps", "curves", "below", "equal", "battery_kw")})
    res, ok = loop.results()
    assert ok and seen["all_optimal"] and int(loop.uncertified.item()) == 0
    assert seen["worst"] <= 1e-6 and seen["lps"] == len(plants) * (3 + 21 * 3 + 24)
    assert seen["battery_kw"][0] <= 5e3 * (1 + 1e-6) and seen["battery_kw"][89] > 5e3 + 1.0 and seen["below"] >= 1 and seen["equal"] >= 1


@gpu
def test_default_loop_is_the_default_plant_passed_as_arrays():
    """BatchedDoubleLoop("wind_battery", 64, S = 3, backcast, price taker) against the same call with the default sizes as arrays: all
    outputs bit for bit after two days - the NULL branch and the pointer branch of the kernels compute the same thing"""
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    kw = dict(n_price_scenarios=3, forecaster="backcast", market="price_taker")
    runs = []
    for sizes in ({}, dict(wind_mw=np.full(64, 200.0), battery_mw=np.full(64, 25.0), battery_mwh=np.full(64, 100.0))):
        loop = BatchedDoubleLoop("wind_battery", 64, device=0, **kw, **sizes)
        assert loop.sized == bool(sizes) and loop.use_fused and bool(loop._loop_tr.wind_kw_plant) == bool(sizes)
        assert bool(loop._mk_da.c0_base_plant) == bool(loop._mk_rt.wind_kw_plant) == bool(sizes)
        for _ in range(2):
            loop.run_day()
        runs.append(_snap(loop))
    assert set(runs[0]) == set(runs[1]) and np.abs(runs[0]["obj"]).max() > 0
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


@gpu
def test_entry_points_refuse_inconsistent_per_plant_pointers_on_the_host():
    """dsp_loop_market_prepare / dsp_loop_market_clear / dsp_loop_update: one of wind_kw_plant / c0_base_plant without the other, per-plant
    pointers on a model without wind columns, the bidding model and the tracker not carrying them together -> DSP_ERR_INVALID and
    nothing written.  Every pointer handed over is a live device buffer of B doubles: only the host's check is exercised."""
    import torch
    from dispatches_amd.hip_solver import DspLoopModel, DspLoopState, load_library
    from tests.test_hip_flowsheet_stochastic import _clear_call
    B = 8
    dev = torch.device("cuda", 0)
    per_plant = torch.full((2, B), 3.0, dtype=torch.float64, device=dev)
    kw_ptr, c0_ptr = per_plant[0].data_ptr(), per_plant[1].data_ptr()

    def with_wind(target):
        for t in range(4):
            target.wind_cols[t] = 30 + t

    def edit(which, kw, c0, wind=()):
        def apply(st, m, a):
            for name in wind:
                with_wind(m if name == "m" else a["tr"])
            target = m if which == "m" else a["tr"]
            target.wind_kw_plant, target.c0_base_plant = kw, c0
        return apply

    def untouched(out, keys):
        return all((out[key] == (-7 if key == "curve" else -1)).all() for key in keys)
    for e in (edit("m", kw_ptr, None, wind=("m",)), edit("m", None, c0_ptr, wind=("m",)), edit("m", kw_ptr, c0_ptr)):      # (last: no wind columns)
        rc, _, out = _clear_call(3, B, 5, 4, edit=e, prepare=True)
        assert rc == -1 and untouched(out, ("c", "lb", "ub", "c0"))
        rc, _, out = _clear_call(3, B, -1, 24, edit=e)
        assert rc == -1 and untouched(out, ("count", "dispatch", "curve"))
    for e in (edit("tr", kw_ptr, None, wind=("m", "tr")), edit("tr", None, c0_ptr, wind=("m", "tr")), edit("tr", kw_ptr, c0_ptr, wind=("m",)),
              edit("tr", kw_ptr, c0_ptr, wind=("m", "tr")),                # the tracker with, the bidding model without
              edit("m", kw_ptr, c0_ptr, wind=("m", "tr"))):                # the bidding model with, the tracker without
        rc, _, out = _clear_call(3, B, 5, 4, with_tracker=True, edit=e)
        assert rc == -1 and untouched(out, ("count", "dispatch", "curve", "tr_rlo", "tr_rhi", "tr_lb", "tr_ub", "tr_c0"))
    # consistent per-plant pointers are accepted, and read: the tracker's constant is the plant's, not the scalar 17.5
    def both(st, m, a):
        with_wind(m), with_wind(a["tr"])
        for target in (m, a["tr"]):
            target.wind_kw_plant, target.c0_base_plant, target.waste_per_kw = kw_ptr, c0_ptr, 0.0
    rc, _, out = _clear_call(3, B, 5, 4, with_tracker=True, edit=both)
    assert rc == 0 and (out["tr_c0"] == 3.0).all()
    # dsp_loop_update: B = 0 (a call that passes the check launches nothing), every other field in range
    lib = load_library()
    c0 = torch.zeros(B, dtype=torch.float64, device=dev)
    series = torch.zeros(48, dtype=torch.float64, device=dev)

    def update(rt_kw, rt_c0, tr_kw, tr_c0, rt_wind=True, tr_wind=True):
        st, rt, tr = DspLoopState(), DspLoopModel(), DspLoopModel()
        st.B, st.N, st.cf_series = 0, 48, series.data_ptr()
        for m, wind, kw, base in ((rt, rt_wind, rt_kw, rt_c0), (tr, tr_wind, tr_kw, tr_c0)):
            m.T, m.n, m.m, m.n_state, m.c0 = 4, 40, 9, 0, c0.data_ptr()
            for t in range(16):
                m.wind_cols[t] = 30 + t if wind and t < 4 else -1
            m.wind_kw_plant, m.c0_base_plant = kw, base
        return lib.dsp_loop_update(C.byref(st), C.byref(rt), C.byref(tr), 0, 0, None)
    assert update(None, None, None, None) == 0 and update(kw_ptr, c0_ptr, kw_ptr, c0_ptr) == 0
    for args in ((kw_ptr, None, kw_ptr, c0_ptr), (kw_ptr, c0_ptr, None, c0_ptr), (kw_ptr, c0_ptr, None, None), (None, None, kw_ptr, c0_ptr)):
        assert update(*args) == -1, args
    assert update(kw_ptr, c0_ptr, kw_ptr, c0_ptr, rt_wind=False) == -1 and update(kw_ptr, c0_ptr, kw_ptr, c0_ptr, tr_wind=False) == -1
