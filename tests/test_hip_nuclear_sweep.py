"""GPU tests of the per-plant nuclear operands (BatchedDoubleLoop("nuclear", pem_mw=, tank_kg=, h2_price=, h2_demand=);
dsp_loop_market_state::p_min_cents_plant, ABI 20): dsp_loop_market_clear with a per-plant minimum power against the tensor form bit for
bit, its refusal of an out-of-range entry, the oracle walk of the mixed batch on the device, and the sweep."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
DSP_ERR_INVALID = -1


def _operands(B):
    """plants that differ in all four operands; ten PEM sizes, so ten minimum powers"""
    k = np.arange(B)
    return dict(pem_mw=25.0 * (1 + k % 10), tank_kg=2000.0 + 1000.0 * (k % 5), h2_price=0.75 + 0.25 * (k % 6), h2_demand=0.2 + 0.05 * (k % 4),
                plant_windows=k // 10)


def _loop(B, market="price_taker", **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    return BatchedDoubleLoop("nuclear", B, device=0, n_price_scenarios=3, forecaster="backcast", market=market, **kw)


def _snap(loop):
    res, ok = loop.results()
    out = {k: v.cpu().numpy().copy() for k, v in res.items()}
    for name, m in (("da", loop.da), ("rt", loop.rt), ("tr", loop.tr)):
        for key in ("c", "lb", "ub", "rlo", "rhi", "c0"):
            out[name + "_" + key] = getattr(m, key).cpu().numpy().copy()
    for key in ("da_curve", "da_count", "rt_curve", "rt_count", "rt_dispatch", "da_offer", "da_prices", "delivered"):
        out[key] = getattr(loop, key).cpu().numpy().copy()
    assert ok and int(loop.uncertified.item()) == 0
    return out


@gpu
@pytest.mark.parametrize("market", ["price_taker", "stub"])
@pytest.mark.parametrize("B", [5, 90])
def test_per_plant_p_min_kernels_are_bit_identical_to_the_tensor_form(B, market):
    """nuclear, B = 5 and B = 90, S = 3, both markets, one day and two hours without graphs, use_fused True (loop_market_clear_kernel
    reading p_min_cents_plant) against False (plant_curves with a per-lane minimum): curves, counts, offers, dispatches, the tracker's
    rows, every objective vector, bound and constant, state, revenue and energies bit for bit.  Not vacuous: the curves of plants
    with different PEM sizes start at different powers, 500 MW - pem_mw each."""
    snaps = {}
    for fused in (True, False):
        loop = _loop(B, market, use_graphs=False, use_fused=fused, **_operands(B))
        assert loop.use_fused == fused and loop.nuclear_sized and (not fused or loop._mk_state.p_min_cents_plant)
        loop.run_day()
        loop.day_ahead()
        loop.hour_step()
        loop.hour_step()
        snaps[fused] = _snap(loop)
    assert set(snaps[True]) == set(snaps[False])
    for key in snaps[True]:
        assert np.array_equal(snaps[True][key], snaps[False][key]), (B, market, key)
    first = snaps[True]["da_curve"][:, :, 0, 0]                                  # the first point of every day-ahead curve, cents
    want = np.round((500.0 - _operands(B)["pem_mw"]) * 100.0).astype(np.int64)
    assert np.array_equal(first, np.repeat(want[:, None], 24, axis=1)) and len(set(want.tolist())) == min(B, 10)
    assert snaps[True]["da_offer"].min() < 400.0                                 # a larger PEM is cleared below the 400 MW of the default plant


@gpu
def test_out_of_range_p_min_entry_is_refused():
    """an entry of p_min_cents_plant outside 0 .. 2e9 (bounded like the scalar): DSP_ERR_INVALID and nothing written; NULL and the
    loop's own array are accepted"""
    import torch
    from dispatches_amd.hip_solver import DspLoopMarketState
    loop = _loop(5, use_graphs=False, **_operands(5))
    loop.day_ahead()
    loop.hour_step()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outputs = (loop.rt_dispatch, loop.rt_curve, loop.rt_count)

    def clear(state):
        return loop._lib.dsp_loop_market_clear(C.byref(state), C.byref(loop._mk_rt), None, 0, loop.tr.T, *(C.c_void_p(v.data_ptr()) for v in outputs), stream())
    for bad in (-1, 2000000001):
        entries = loop.p_min_cents_plant.clone()
        entries[3] = bad
        state = DspLoopMarketState.from_buffer_copy(loop._mk_state)
        state.p_min_cents_plant = entries.data_ptr()
        before = [v.clone() for v in outputs]
        for v in outputs:
            v.fill_(-7)
        rc = clear(state)
        torch.cuda.synchronize()
        assert rc == DSP_ERR_INVALID, (bad, rc)
        assert all((v == -7).all().item() for v in outputs)
        for v, keep in zip(outputs, before):
            v.copy_(keep)
    assert clear(loop._mk_state) == 0                                            # the loop's own array: every curve from its plant's minimum
    torch.cuda.synchronize()
    assert torch.equal(loop.rt_curve[:, :, 0, 0].to(torch.int64), loop.p_min_cents_plant[:, None].expand(-1, loop.tr.T))
    state = DspLoopMarketState.from_buffer_copy(loop._mk_state)
    state.p_min_cents_plant = None                                               # NULL: the scalar, every curve from 400 MW
    assert clear(state) == 0
    torch.cuda.synchronize()
    assert (loop.rt_curve[:, :, 0, 0] == 40000).all().item()


@gpu
def test_oracle_walk_of_the_mixed_batch_on_the_device(monkeypatch):
    """the walk of tests/test_nuclear_sweep_cpu.py on the device: B = 4 x S = 3, two days, the second from graphs; every LP against the
    oracle at its plant's operands to 1e-6, curves and dispatches exact, all optimal, nothing uncertified"""
    from tests._nuclear_size_oracle import nuclear_walk
    from tests.test_nuclear_sweep_cpu import MIXED
    loop = _loop(4, ledger=True, **MIXED)
    seen = nuclear_walk(loop, 2, monkeypatch)
    res, ok = loop.results()
    print("mixed nuclear batch on the device, worst relative objective gap:", seen["worst"], "over", seen["lps"], "LPs")
    assert ok and seen["all_optimal"] and seen["worst"] <= 1e-6 and int(loop.uncertified.item()) == 0
    assert len(loop._graphs) == 25 and seen["lps"] == 2 * 4 * (3 + (24 - loop.rt.T + 1) * 3 + 24)
    assert seen["lowest_offer_mw"][1] == 300.0 and seen["lowest_offer_mw"][0] == 400.0
    h2 = res["h2_kg"].cpu().numpy()
    assert np.allclose(res["h2_revenue"].cpu().numpy(), h2 * np.array(MIXED["h2_price"]), rtol=1e-12) and h2.min() > 0


@gpu
def test_nuclear_sweep_on_the_device():
    """a 2 x 2 x 2 grid, two days (the second from graphs): all optimal, shapes, profit = revenue - tot_cost exactly, the capacity
    factor inside (0, 1], and the larger PEM delivers less electricity at every price and window (cell against own-loop equality is
    the CPU test's: HiGHS gives one vertex, the device solvers' choice among degenerate optima may depend on the shared template)"""
    from dispatches_amd.sweeps import nuclear_sweep
    out = nuclear_sweep([0.75, 2.0], [50.0, 250.0], 2, 2)
    assert out["all_optimal"] and all(out[k].shape == (2, 2, 2) for k in out if k != "all_optimal")
    assert np.array_equal(out["profit"], out["revenue"] - out["tot_cost"])
    assert (out["pem_capacity_factor"] > 0).all() and (out["pem_capacity_factor"] <= 1.0 + 1e-9).all()
    assert (out["energy_mwh"][:, 1] < out["energy_mwh"][:, 0]).all() and (out["h2_kg"] > 0).all()
