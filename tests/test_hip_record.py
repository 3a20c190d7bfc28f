"""GPU tests of the recorder of the descriptor double loop (BatchedDoubleLoop(record=(plants, days)); dsp_loop_record /
dsp_loop_record_desc, ABI 21): the gather kernel against the tensor form bit for bit in every participation mode, graph replay against
the eager loop, the refusals of the entry point on sentinel-filled buffers, and the default loops next to a recording loop."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast", market="price_taker")
DSP_ERR_INVALID = -1

CASES = {"nuclear_stochastic": ("nuclear", STOCHASTIC),
         "wind_pem_monotone": ("wind_pem", dict(STOCHASTIC, scenario_coupling="monotone")),
         "wind_battery_self_schedule": ("wind_battery", dict(n_price_scenarios=2, forecaster="backcast", market="price_taker", bidder="self_schedule")),
         "wind_pem_parametrized": ("wind_pem", dict(bidder="parametrized", bid_price=20.0, storage_mw=100.0, market="price_taker")),
         "nuclear_ruc_ledger": ("nuclear", dict(STOCHASTIC, ruc_hour=16, ledger=True))}
BATCHES = {70: [0, 63, 64, 69], 5: [4]}               # indices on both sides of the 64-lane boundary; R = 1, an odd tiny grid


def _loop(flowsheet, B, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    return BatchedDoubleLoop(flowsheet, B, device=0, **kw)


def _day_and_two_hours(loop):
    loop.run_day()
    loop.day_ahead()
    loop.hour_step()
    loop.hour_step()


def _twin(loop):
    """a second recorder on the same loop that writes the TENSOR form into buffers of its own whenever the loop's recorder writes: both
    read the same live buffers at the same moment"""
    from dispatches_amd.loop_record import LoopRecorder
    rec = loop._rec
    twin = LoopRecorder(loop, rec.plants, rec.days, 2 ** 30)
    twin._desc = None
    write = rec.write

    def both(name):
        write(name)
        twin._write_tensors(name)
    rec.write = both
    return twin


@gpu
@pytest.mark.parametrize("B", list(BATCHES))
@pytest.mark.parametrize("case", list(CASES))
def test_record_kernel_is_bit_identical_to_the_tensor_form(case, B):
    """One day and two hours (a midnight is crossed; days = 1: the second day's rows go to the spare row), use_graphs=False.
    (a) in the fused loop, the kernel's record against the tensor form of the same writes on the same live buffers: every buffer,
    spare rows included, bit for bit.  (b) use_fused True against False: recorded() bit for bit - except `delivered` where the loop's
    tensor form states the hand-off in matrix arithmetic (loops that are not `exact`; _hand_off), which is compared to 1e-12."""
    flowsheet, kw = CASES[case]
    plants = BATCHES[B]
    fused = _loop(flowsheet, B, record=(plants, 1), use_graphs=False, use_fused=True, **kw)
    tensor = _loop(flowsheet, B, record=(plants, 1), use_graphs=False, use_fused=False, **kw)
    assert fused.use_fused and fused._rec._desc is not None and not tensor.use_fused and tensor._rec._desc is None
    twin = _twin(fused)
    _day_and_two_hours(fused)
    _day_and_two_hours(tensor)
    assert fused.results()[1] and tensor.results()[1]
    for key, buf in fused._rec.buf.items():
        assert np.array_equal(buf.cpu().numpy(), twin.buf[key].cpu().numpy()), (case, B, key)
    a, b = fused.recorded(), tensor.recorded()
    assert sorted(a) == sorted(b) and a["plants"].tolist() == plants and a["delivered"].shape == (24, len(plants))
    assert a["da_offer"].shape == (1, len(plants), 24)
    for key in a:
        if key == "delivered" and not fused.exact:
            np.testing.assert_allclose(a[key], b[key], rtol=1e-12, atol=0)
        else:
            assert np.array_equal(a[key], b[key]), (case, B, key)
    # what the cases are there for
    widths = {s.width for d in fused._rec._desc.values() for s in d.segments[:d.n_segments]}
    assert any(w % 64 for w in widths) and a["tr_x"].any() and a["delivered"].any()
    if case == "wind_pem_monotone":
        seg = fused._rec._desc["daily"].segments[0]                       # da_x: the one coupled row of S * n1 columns
        assert seg.plant_stride == fused.da.lp.n == 3 * fused.da.n1 and a["da_x"].shape[2:] == (3, fused.da.n1)
    if case == "wind_battery_self_schedule":
        assert a["rt_x"].shape[2] == 1 and a["rt_curve"].shape[2:] == (fused.tr.T, 3, 2)
    if case == "wind_pem_parametrized":
        assert "rt_x" not in a and "da_x" not in a and a["rt_count"].dtype == np.int32 and a["rt_count"].any()
    if case == "nuclear_ruc_ledger":
        assert "bid" in fused._rec._desc and a["ledger_hour"].shape == (24, len(plants), 6) and a["ledger_hour"][..., 0].all()
        seg = [s for s in fused._rec._desc["hour"].segments[:fused._rec._desc["hour"].n_segments] if s.elem_stride == B]
        assert len(seg) == 1 and seg[0].plant_stride == 1                 # the ledger's [F, B] source
        # the bid made at hour 16 of day 0 is for day 1: past days = 1, so it sits in the spare row, and row 0 is day 0's bid
        spare = fused._rec.buf["da_offer"][1].cpu().numpy()
        assert np.array_equal(spare, fused.da_offer.cpu().numpy()[plants]) and spare.any() and a["da_offer"][0].any()


@gpu
def test_graph_replay_records_what_the_eager_loop_records():
    """nuclear, B = 70 x S = 3, three days: eager against graphs (day 2 captured, day 3 replayed) - recorded() bit for bit, and the
    recorder's launches sit inside the captured steps: 24 + 1 graphs as without it"""
    out = {}
    for graphs in (False, True):
        loop = _loop("nuclear", 70, record=(BATCHES[70], 3), use_graphs=graphs, **STOCHASTIC)
        for _ in range(3):
            loop.run_day()
        assert loop.use_fused and int(loop.hour_t.item()) == 72 and len(loop._graphs) == (25 if graphs else 0)
        assert loop.results()[1]
        out[graphs] = loop.recorded()
    assert out[True]["delivered"].shape == (72, 4) and out[True]["da_x"].shape[0] == 3
    for key in out[False]:
        assert np.array_equal(out[False][key], out[True][key]), key
    assert out[True]["delivered"][48:].all() and out[True]["da_offer"][2].any()      # the replayed day is there


@gpu
def test_dsp_loop_record_refusals():
    """every refusal the header lists, one broken field at a time, on sentinel-filled destinations: DSP_ERR_INVALID and nothing written;
    the unedited call returns 0 and writes exactly n_plants x sum(width) elements of one row; a clock of 0 with offset -1 and a clock
    past the span touch the spare row only"""
    import torch
    from dispatches_amd.hip_solver import DspLoopRecordDesc, load_library
    lib = load_library()
    dev = torch.device("cuda", 0)
    B, rows, plants = 9, 3, [1, 4, 8]
    src64 = torch.arange(B * 5, dtype=torch.float64, device=dev).reshape(B, 5) + 0.5           # plant-major, width 5
    src32 = (torch.arange(3 * B, dtype=torch.int32, device=dev) + 100).reshape(3, B)           # plant-minor [F, B], width 3
    dst64 = torch.empty((rows + 1, len(plants), 5), dtype=torch.float64, device=dev)
    dst32 = torch.empty((rows + 1, len(plants), 3), dtype=torch.int32, device=dev)
    clock = torch.zeros((), dtype=torch.int64, device=dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def descriptor():
        d = DspLoopRecordDesc()
        d.n_plants, d.n_segments = len(plants), 2
        for q, b in enumerate(plants):
            d.plants[q] = b
        d.clock, d.divisor, d.offset, d.rows = clock.data_ptr(), 1, 0, rows
        a, b = d.segments[0], d.segments[1]
        a.src, a.dst, a.plant_stride, a.elem_stride, a.width, a.elem_bytes = src64.data_ptr(), dst64.data_ptr(), 5, 1, 5, 8
        b.src, b.dst, b.plant_stride, b.elem_stride, b.width, b.elem_bytes = src32.data_ptr(), dst32.data_ptr(), 1, B, 3, 4
        return d

    def fill():
        dst64.fill_(-7.25)
        dst32.fill_(-7)

    def untouched():
        torch.cuda.synchronize()
        return bool((dst64 == -7.25).all().item() and (dst32 == -7).all().item())

    def refused(edit, batch=B):
        d = descriptor()
        edit(d)
        fill()
        rc = lib.dsp_loop_record(C.byref(d), batch, stream())
        assert rc == DSP_ERR_INVALID and untouched(), edit.__doc__

    def field(name, value, segment=None):
        def edit(d):
            setattr(d if segment is None else d.segments[segment], name, value)
        edit.__doc__ = f"{name}={value!r} segment={segment}"
        return edit

    def plant(q, value):
        def edit(d):
            d.plants[q] = value
        edit.__doc__ = f"plants[{q}]={value}"
        return edit
    fill()
    assert lib.dsp_loop_record(None, B, stream()) == DSP_ERR_INVALID and untouched()
    refused(field("clock", None))
    for name, values in dict(n_plants=[0, 65], n_segments=[0, 17], rows=[0, (1 << 24) + 1], divisor=[0, 8785], offset=[1, -2], reserved=[1]).items():
        for v in values:
            refused(field(name, v))
    refused(plant(1, 1))                               # not strictly increasing: equal, then decreasing
    refused(plant(2, 3))
    refused(plant(0, -1))                              # outside [0, B)
    refused(plant(2, B))
    refused(lambda d: None, batch=8)                   # ... the same descriptor on a batch of 8 plants: plants[2] = 8 is not below B
    refused(lambda d: None, batch=0)
    for s in (0, 1):
        refused(field("src", None, s))
        refused(field("dst", None, s))
        for name, values in dict(width=[0, (1 << 20) + 1], elem_bytes=[0, 2, 16], plant_stride=[0, -1, (1 << 40) + 1], elem_stride=[0, -5, (1 << 40) + 1]).items():
            for v in values:
                refused(field(name, v, s))

    def written_rows():
        torch.cuda.synchronize()
        return sorted(set(torch.nonzero((dst64 != -7.25).any(2).any(1)).flatten().tolist()) | set(torch.nonzero((dst32 != -7).any(2).any(1)).flatten().tolist()))
    # the unedited call: row = clock, exactly n_plants x (5 + 3) elements, each the source's
    clock.fill_(2)
    fill()
    assert lib.dsp_loop_record(C.byref(descriptor()), B, stream()) == 0
    assert written_rows() == [2]
    assert int((dst64 != -7.25).sum().item()) + int((dst32 != -7).sum().item()) == len(plants) * (5 + 3)
    assert torch.equal(dst64[2], src64[plants]) and torch.equal(dst32[2], src32.t()[plants])
    # a daily record: row = clock // 24
    clock.fill_(49)
    fill()
    d = descriptor()
    d.divisor = 24
    assert lib.dsp_loop_record(C.byref(d), B, stream()) == 0
    assert written_rows() == [2] and torch.equal(dst64[2], src64[plants])
    # the spare row: the hour before hour 0, with both divisors (-1 // 24 is not day 0), and clocks past the span
    for value, divisor, offset in ((0, 1, -1), (0, 24, -1), (rows, 1, 0), (rows + 1, 1, -1), (24 * rows, 24, 0), (10 ** 12, 1, 0)):
        clock.fill_(value)
        fill()
        d = descriptor()
        d.divisor, d.offset = divisor, offset
        assert lib.dsp_loop_record(C.byref(d), B, stream()) == 0
        assert written_rows() == [rows], (value, divisor, offset)
        assert torch.equal(dst64[rows], src64[plants]) and torch.equal(dst32[rows], src32.t()[plants])
    clock.fill_(rows)                                  # ... and the last row of the span, reached by offset -1
    fill()
    d = descriptor()
    d.offset = -1
    assert lib.dsp_loop_record(C.byref(d), B, stream()) == 0
    assert written_rows() == [rows - 1]


@gpu
def test_default_loops_around_a_recording_loop():
    """the default loop (record=None) before and after a recording loop was built and run in the same process: two days, bit-identical"""
    def default_days():
        loop = _loop("nuclear", 5, **STOCHASTIC)
        loop.run_day()
        loop.run_day()
        res, ok = loop.results()
        assert ok and loop._rec is None
        out = {k: v.cpu().numpy().copy() for k, v in res.items()}
        for key in ("delivered", "da_offer", "da_curve", "rt_dispatch", "rt_curve"):
            out[key] = getattr(loop, key).cpu().numpy().copy()
        out["x"] = loop.tr.out["x"].cpu().numpy().copy()
        return out
    before = default_days()
    rec = _loop("nuclear", 5, record=([1, 3], 2), **STOCHASTIC)
    rec.run_day()
    rec.run_day()
    got = rec.recorded()
    assert got["delivered"].shape == (48, 2) and np.array_equal(got["delivered"][-1], rec.delivered.cpu().numpy()[[1, 3]])
    after = default_days()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    for key in ("obj", "energy_mwh", "state"):       # ... and recording itself changes nothing the loop computes
        assert np.array_equal(before[key], rec.results()[0][key].cpu().numpy()), key
