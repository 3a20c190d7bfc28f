"""GPU tests of the ledger of the implemented hour (BatchedDoubleLoop(ledger=True); dsp_loop_ledger / dsp_loop_ledger_desc, ABI 20): the
kernel against the tensor statement bit for bit below one wave and across two blocks, the refusals of the entry point on the host, graph
replay against the eager loop, and the default loops next to a loop that keeps a ledger."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast", market="price_taker")
DSP_ERR_INVALID = -1


def _loop(flowsheet, B, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    return BatchedDoubleLoop(flowsheet, B, device=0, **{**STOCHASTIC, **kw})


def _sizes(B):
    """plants of three wind sizes and three batteries, B of them"""
    k = np.arange(B)
    batt = np.array([5.0, 25.0, 100.0])[(k // 3) % 3]
    return dict(wind_mw=np.array([50.0, 200.0, 400.0])[k % 3], battery_mw=batt, battery_mwh=4.0 * batt, plant_windows=k // 9)


def _snap(loop):
    res, ok = loop.results()
    out = {k: v.cpu().numpy().copy() for k, v in res.items()}
    for key in ("ledger_acc", "ledger_hour", "delivered", "da_offer", "rt_dispatch"):
        if hasattr(loop, key):
            out[key] = getattr(loop, key).cpu().numpy().copy()
    out["x"] = loop.tr.out["x"].cpu().numpy().copy()
    assert ok and int(loop.uncertified.item()) == 0
    return out


def _day_and_two_hours(loop):
    """a midnight is crossed: the first day runs eagerly, the two hours after it are day 2's"""
    loop.run_day()
    loop.day_ahead()
    loop.hour_step()
    loop.hour_step()
    return _snap(loop)


def _priced(B):
    """nuclear plants with their own hydrogen price and PEM size"""
    k = np.arange(B)
    return dict(h2_price=0.75 + 0.25 * (k % 6), pem_mw=25.0 * (1 + k % 10), plant_windows=k // 10)


def _parametrized(B):
    k = np.arange(B)
    return dict(bidder="parametrized", bid_price=10.0 + 5.0 * (k % 4), storage_mw=50.0 * (1 + k % 5), n_price_scenarios=1, forecaster="perfect")


CASES = {"wind_battery": ("wind_battery", lambda B: {}), "wind_pem": ("wind_pem", lambda B: {}), "nuclear": ("nuclear", lambda B: {}),
         "wind_battery_sized": ("wind_battery", _sizes), "nuclear_priced": ("nuclear", _priced), "wind_pem_parametrized": ("wind_pem", _parametrized)}


@gpu
@pytest.mark.parametrize("B", [5, 257])
@pytest.mark.parametrize("case", list(CASES))
def test_ledger_kernel_is_bit_identical_to_the_tensor_statement(case, B):
    """B = 5 (less than one wave) and B = 257 (the second block of every form has one live lane), stochastic bidder, one day and two
    hours, use_fused True (loop_ledger_kernel) against False (_ledger_book, exact_fma): the accumulators and the last hour's values of
    every key bit for bit - all three flowsheets (shared coefficients and constants, with and without the hour's available wind) and a
    sized wind + battery batch (per-plant constants, wind_kw_plant), a nuclear batch of different hydrogen prices and PEM sizes (per-plant
    coefficients, built by the loop) and the parametrized wind + PEM loop (the fused parametrized hour, one form fewer)."""
    flowsheet, extra = CASES[case]
    fused = _loop(flowsheet, B, ledger=True, use_graphs=False, use_fused=True, **extra(B))
    tensor = _loop(flowsheet, B, ledger=True, use_graphs=False, use_fused=False, **extra(B))
    assert fused.use_fused and not tensor.use_fused and fused.ledger_acc.shape == (len(fused.ledger_keys), B)
    if case.endswith("sized"):
        assert fused._loop_ledger.const_stride == len(fused.ledger_keys) and fused._loop_tr.wind_kw_plant
        assert len(set(fused._ledger["const"][:, 0].cpu().tolist())) == 3            # fixed O&M of three wind sizes
    elif case == "nuclear_priced":
        F = len(fused.ledger_keys)
        assert fused._loop_ledger.coef_stride == F * 8 and fused._loop_ledger.const_stride == 0 and fused.nuclear_sized
        assert len(set(fused._ledger["coef"][:, F - 1, 0].cpu().tolist())) == min(B, 6)      # h2_revenue at six hydrogen prices
    else:
        assert fused._loop_ledger.const_stride == 0 and fused._loop_ledger.coef_stride == 0
        if flowsheet == "wind_pem":
            assert ("h2_kg" in fused.ledger_keys) == (case != "wind_pem_parametrized")
    a, b = _day_and_two_hours(fused), _day_and_two_hours(tensor)
    assert np.array_equal(a["x"], b["x"])                                            # the same tracker solutions went in
    for key in ["ledger_acc", "ledger_hour", "state"] + fused.ledger_keys + (["obj", "profit"] if fused.exact else []):
        assert np.array_equal(a[key], b[key]), (case, B, key)      # (the revenue, and with it the profit, is bit-identical where the tensor form states phase 2 exactly: the sized batch)
    assert np.array_equal(b["profit"], b["obj"] - b["tot_cost"])
    assert np.abs(a["ledger_acc"][0]).min() > 0                                      # every plant has booked a cost
    assert np.array_equal(a["profit"], a["obj"] - a["tot_cost"])
    if flowsheet != "nuclear":
        f = fused.ledger_keys.index("curtailed_mwh")
        assert fused._loop_ledger.per_avail[f] != 0.0 and fused._loop_ledger.per_avail[0] != 0.0


@gpu
@pytest.mark.parametrize("B", [5, 257])
def test_per_plant_coefficients_and_constants(B):
    """coef_stride / const_stride != 0 (what a batch of plants with different hydrogen prices will carry): the nuclear loop's descriptor
    with every plant's own coefficients [B, F, 8] and constants [B, F], padded to strides LONGER than one plant's set, on the tracker's
    solution of a real hour - the kernel against the tensor statement on the same arrays, bit for bit, and not the shared result"""
    import torch
    from dispatches_amd.hip_solver import DspLoopLedgerDesc
    loop = _loop("nuclear", B, ledger=True, use_graphs=False)
    loop.day_ahead()
    loop.hour_step()
    L, F = loop._ledger, len(loop.ledger_keys)
    shared = loop.ledger_hour.clone()
    scale = 1.0 + torch.arange(B, dtype=torch.float64, device=loop.dev) / 7.0             # plant b: 1 + b / 7 times the shared numbers
    coef_pad = torch.full((B, F + 1, 8), float("nan"), dtype=torch.float64, device=loop.dev)
    const_pad = torch.full((B, F + 2), float("nan"), dtype=torch.float64, device=loop.dev)
    coef_pad[:, :F] = L["coef"][None] * scale[:, None, None]
    const_pad[:, :F] = L["const"][None] * scale[:, None]
    g = DspLoopLedgerDesc.from_buffer_copy(loop._loop_ledger)
    g.coef, g.coef_stride, g.constant, g.const_stride = coef_pad.data_ptr(), (F + 1) * 8, const_pad.data_ptr(), F + 2
    loop.ledger_acc.zero_()
    rc = loop._lib.dsp_loop_ledger(C.byref(loop._loop_state), C.byref(loop._loop_tr), C.byref(g), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    kernel = loop.ledger_hour.clone()
    assert torch.equal(loop.ledger_acc, kernel) and torch.isfinite(kernel).all().item()
    L["coef"], L["const"] = coef_pad[:, :F], const_pad[:, :F]                              # the tensor statement on the same per-plant arrays
    loop.ledger_acc.zero_()
    loop.hour_t -= 1                                                                        # (the hand-off has advanced the clock; nuclear reads no capacity factor anyway)
    loop._ledger_book(loop.tr.out["x"])
    assert torch.equal(loop.ledger_hour, kernel) and torch.equal(loop.ledger_acc, kernel)
    assert torch.equal(kernel[:, 0], shared[:, 0]) and not torch.equal(kernel[0, 1:], shared[0, 1:])      # plant 0 has scale 1, the others their own


def _filled(loop, value=-7.25):
    loop.ledger_acc.fill_(value)
    loop.ledger_hour.fill_(value)


@gpu
def test_dsp_loop_ledger_refusals():
    """every refusal the header lists, on sentinel-filled accumulators: DSP_ERR_INVALID and nothing written; the untouched descriptor
    is accepted and writes"""
    import torch
    from dispatches_amd.hip_solver import DspLoopLedgerDesc, DspLoopModel, DspLoopState
    nuc, wb = _loop("nuclear", 5, ledger=True, use_graphs=False), _loop("wind_battery", 5, ledger=True, use_graphs=False)
    for loop in (nuc, wb):
        loop.day_ahead()
        loop.hour_step()
    lib = nuc._lib
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(loop, g=None, st=None, tr=None):
        return lib.dsp_loop_ledger(C.byref(st or loop._loop_state), C.byref(tr or loop._loop_tr), C.byref(g or loop._loop_ledger), stream())

    def refused(loop, **fields):
        """a copy of the loop's descriptor / state / tracker with `fields` set (g_*, st_*, tr_*) is refused and writes nothing"""
        g, st, tr = DspLoopLedgerDesc.from_buffer_copy(loop._loop_ledger), DspLoopState.from_buffer_copy(loop._loop_state), DspLoopModel.from_buffer_copy(loop._loop_tr)
        for name, value in fields.items():
            target, field = {"g": g, "st": st, "tr": tr}[name.split("_", 1)[0]], name.split("_", 1)[1]
            if callable(value):
                value(target)
            else:
                setattr(target, field, value)
        _filled(loop)
        rc = call(loop, g, st, tr)
        torch.cuda.synchronize()
        assert rc == DSP_ERR_INVALID, (fields, rc)
        assert (loop.ledger_acc == -7.25).all().item() and (loop.ledger_hour == -7.25).all().item(), fields

    def set_col(f, e, col):
        def apply(g):
            g.cols[f][e] = col
        return apply

    def set_terms(f, count):
        def apply(g):
            g.n_terms[f] = count
        return apply

    def set_per_avail(f, v):
        def apply(g):
            g.per_avail[f] = v
        return apply
    n = nuc.tr.lp.n
    refused(nuc, g_cols=set_col(0, 0, n))                    # a column outside [0, n)
    refused(nuc, g_cols=set_col(3, 0, -1))
    refused(nuc, g_n_forms=9)                                 # more forms / terms than the limits
    refused(nuc, g_n_forms=0)
    refused(nuc, g_n_terms=set_terms(0, 9))
    refused(nuc, g_n_terms=set_terms(1, -1))
    refused(nuc, g_acc=None)                                  # NULL buffers
    refused(nuc, g_hour_value=None)
    refused(nuc, g_coef=None)
    refused(nuc, g_constant=None)
    refused(nuc, g_reserved=1)
    refused(nuc, g_coef_stride=8)                             # shorter than one plant's set of 6 forms x 8
    refused(nuc, g_const_stride=-1)
    refused(nuc, tr_x=None)
    refused(nuc, g_per_avail=set_per_avail(0, 1.0))           # per_avail without wind columns (and without capacity factors)
    refused(wb, st_cf_series=None)                            # ... with wind columns but no capacity factors
    refused(wb, g_per_avail=set_per_avail(1, float("nan")))
    assert lib.dsp_loop_ledger(None, C.byref(nuc._loop_tr), C.byref(nuc._loop_ledger), stream()) == DSP_ERR_INVALID
    for loop in (nuc, wb):                                    # the descriptor as the loop built it is accepted, and writes every entry
        _filled(loop)
        assert call(loop) == 0
        torch.cuda.synchronize()
        assert not (loop.ledger_hour == -7.25).any().item() and torch.equal(loop.ledger_acc, loop.ledger_hour - 7.25)
        assert (loop.ledger_hour[0] != 0).all().item()
    empty = DspLoopState.from_buffer_copy(nuc._loop_state)    # B = 0: nothing to do, no launch
    empty.B = 0
    _filled(nuc)
    assert call(nuc, st=empty) == 0
    torch.cuda.synchronize()
    assert (nuc.ledger_acc == -7.25).all().item()


@gpu
def test_graph_replay_is_the_eager_loop_and_the_ledger_changes_nothing_else():
    """nuclear, B = 90 x S = 3, three days with ledger=True: eager against graphs (day 2 captured, day 3 replayed) bit for bit, the
    ledger included; and against the same loop with ledger=False in everything that loop has (the booking sits in the captured hour
    graphs: 24 + 1 graphs as before)"""
    snaps = {}
    for name, kw in (("eager", dict(ledger=True, use_graphs=False)), ("graphs", dict(ledger=True)), ("off", dict(ledger=False))):
        loop = _loop("nuclear", 90, **kw)
        for _ in range(3):
            loop.run_day()
        assert loop.use_fused and int(loop.hour_t.item()) == 72 and len(loop._graphs) == (0 if name == "eager" else 25)
        snaps[name] = _snap(loop)
    assert set(snaps["eager"]) == set(snaps["graphs"]) and "ledger_acc" not in snaps["off"] and "profit" not in snaps["off"]
    for key in snaps["eager"]:
        assert np.array_equal(snaps["eager"][key], snaps["graphs"][key]), key
    for key in snaps["off"]:
        assert np.array_equal(snaps["off"][key], snaps["graphs"][key]), key
    assert snaps["graphs"]["h2_kg"].min() > 0 and snaps["graphs"]["over_mwh"].max() > 0


@gpu
@pytest.mark.parametrize("mode", ["stochastic", "deterministic"])
def test_default_loops_around_a_ledger_loop(mode):
    """the default loop (ledger=False) before and after a loop that keeps a ledger ran in the same process: bit-identical"""
    kw = {} if mode == "stochastic" else dict(n_price_scenarios=1, forecaster="perfect", market="stub")

    def default_day():
        loop = _loop("nuclear", 5, **kw)
        loop.run_day()
        return _snap(loop)
    before = default_day()
    with_ledger = _loop("nuclear", 5, ledger=True, **kw)
    with_ledger.run_day()
    booked = _snap(with_ledger)
    after = default_day()
    assert set(before) == set(after) and "ledger_acc" not in before
    for key in before:
        assert np.array_equal(before[key], after[key]), key
        assert np.array_equal(before[key], booked[key]), key
    assert booked["h2_revenue"].min() > 0
