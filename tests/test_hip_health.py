"""GPU tests of the per-plant solve health of the descriptor double loop (BatchedDoubleLoop(health=True); dsp_loop_health /
dsp_loop_health_state, added under ABI 22): the kernel alone against its numpy statement at every size edge, the refusals of the entry
point on the host, the kernels against the tensor form inside the loop - with an iteration limit that makes part of the day-ahead batch
fail, so that non-zero counters are compared -, graph replay against the eager loop, the shape whose coupled LPs are known to end at the
iteration limit, and health=True next to health=False.  Integers throughout: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast", market="price_taker")
MONOTONE = dict(scenario_coupling="monotone", forecaster="backcast", max_historical_days=3, market="price_taker", day_ahead_horizon=24)
DSP_ERR_INVALID = -1
COUNTERS = ("solves", "fail", "status_mask", "waived", "iters", "iters_max", "first")
TENSORS = ("health_solves", "health_fail", "health_status", "health_waived", "health_iters", "health_iters_max", "health_first")


def _loop(flowsheet, B, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    return BatchedDoubleLoop(flowsheet, B, device=0, **kw)


class _Counters:
    """sentinel-filled counters [4, B] / [B], a clock and the descriptor over them"""

    def __init__(self, B, sentinel):
        import torch
        from dispatches_amd.hip_solver import DspLoopHealthState
        dev = torch.device("cuda", 0)
        full = lambda dtype, *shape: torch.full(shape, sentinel, dtype=dtype, device=dev)
        self.t = dict(solves=full(torch.int32, 4, B), fail=full(torch.int32, 4, B), status_mask=full(torch.int32, 4, B), waived=full(torch.int32, 4, B),
                      iters=full(torch.int64, 4, B), iters_max=full(torch.int32, 4, B), first=full(torch.int64, B))
        self.clock = torch.zeros((), dtype=torch.int64, device=dev)
        self.h = DspLoopHealthState()
        self.h.B, self.h.clock = B, self.clock.data_ptr()
        for name in COUNTERS:
            setattr(self.h, name, self.t[name].data_ptr())

    def numpy(self):
        return {name: v.cpu().numpy().copy() for name, v in self.t.items()}


def _book_numpy(c, status, flags, iters, R, kind, clock):
    """the statement of dsp_loop_health on host arrays c (in place)"""
    B = c["first"].shape[0]
    s = status.reshape(B, R)
    failed = s != 0
    c["solves"][kind] += R
    c["fail"][kind] += failed.sum(1).astype(np.int32)
    bits = np.where(failed, np.left_shift(1, np.where((s >= 1) & (s <= 29), s, 30)), 0)
    c["status_mask"][kind] |= np.bitwise_or.reduce(bits, axis=1).astype(np.int32)
    if flags is not None:
        c["waived"][kind] += (~failed & ((flags.reshape(B, R) & 1) != 0)).sum(1).astype(np.int32)
    if iters is not None:
        it = iters.reshape(B, R)
        c["iters"][kind] += it.sum(1, dtype=np.int64)
        c["iters_max"][kind] = np.maximum(c["iters_max"][kind], np.maximum(it.max(1), 0))
    c["first"][:] = np.where(failed.any(1) & (c["first"] == 0), clock + 1, c["first"])


def _call(lib, h, status, flags, iters, R, kind):
    import torch
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = lib.dsp_loop_health(None if h is None else C.byref(h), ptr(status), ptr(flags), ptr(iters), R, kind, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@gpu
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("R", [1, 3, 16])
@pytest.mark.parametrize("B", [1, 70, 257])
def test_kernel_alone_against_its_numpy_statement(B, R, kind):
    """synthetic status / flags / iters, three consecutive calls with a moving clock (5, 6, 30): sums, maxima, the status mask and "the
    first failure stays the first"; B = 257 crosses the 256-lane block edge, 70 a wave edge; the counter rows of the other kinds keep
    their sentinel; a fourth call with flags = NULL and iters = NULL leaves the waived and iteration counters as they were"""
    import torch
    from dispatches_amd.hip_solver import load_library
    lib = load_library()
    rng = np.random.default_rng(1000 * B + 10 * R + kind)
    c = _Counters(B, 3)
    c.t["first"].zero_()
    if B > 1:
        c.t["first"][B // 2] = 2                                          # a plant that failed at hour 1, before these calls: stays
    want = c.numpy()
    dev = c.clock.device
    for call, clock in enumerate((5, 6, 30)):
        status = rng.choice(np.array([0, 0, 0, 0, 1, 2, 3, 4], np.int32), size=B * R)
        if call == 0:
            status.reshape(B, R)[::2] = 0                                 # every other plant fails later, if at all
        if call == 1:
            status.reshape(B, R)[0] = 0                                   # (plant 0: a call without a failure; its small iters keep the earlier maximum)
        flags = rng.integers(0, 4, size=B * R).astype(np.int32)          # bit 0 = DSP_FLAG_OBJ_WAIVED, bit 1 another flag
        iters = rng.integers(0, 200001, size=B * R).astype(np.int32)
        if call == 1:
            iters.reshape(B, R)[0] = 1
        c.clock.fill_(clock)
        args = [torch.as_tensor(a, device=dev) for a in (status, flags, iters)]
        assert _call(lib, c.h, *args, R, kind) == 0
        _book_numpy(want, status, flags, iters, R, kind, clock)
        got = c.numpy()
        for name in COUNTERS:
            assert np.array_equal(got[name], want[name]), (name, call)
    for name in COUNTERS[:-1]:                                            # the rows of the other kinds: never touched
        others = np.delete(got[name], kind, axis=0)
        assert (others == 3).all(), name
    assert got["solves"][kind][0] == 3 + 3 * R
    status = torch.ones(B * R, dtype=torch.int32, device=dev)             # flags = NULL, iters = NULL: every row fails with status 1
    c.clock.fill_(99)
    assert _call(lib, c.h, status, None, None, R, kind) == 0
    last = c.numpy()
    for name in ("waived", "iters", "iters_max"):
        assert np.array_equal(last[name], got[name]), name
    assert np.array_equal(last["fail"][kind], got["fail"][kind] + R) and (last["status_mask"][kind] & 2 == 2).all()
    assert np.array_equal(last["first"], np.where(got["first"] == 0, 100, got["first"]))


@gpu
def test_dsp_loop_health_refusals():
    """every refusal the header lists, on sentinel-filled counters: DSP_ERR_INVALID and nothing written; the untouched call is accepted"""
    import torch
    from dispatches_amd.hip_solver import DspLoopHealthState, load_library
    lib = load_library()
    B, R = 70, 3
    c = _Counters(B, -7)
    dev = c.clock.device
    status, flags, iters = (torch.ones(B * R, dtype=torch.int32, device=dev) for _ in range(3))

    def refused(R=R, kind=1, no_status=False, **fields):
        h = DspLoopHealthState.from_buffer_copy(c.h)
        for name, value in fields.items():
            setattr(h, name, value)
        rc = _call(lib, h, None if no_status else status, flags, iters, R, kind)
        assert rc == DSP_ERR_INVALID, (fields, R, kind, rc)
        for name, v in c.t.items():
            assert (v == -7).all().item(), (fields, R, kind, name)
    refused(B=0)
    refused(B=-1)
    refused(R=0)
    refused(R=17)
    refused(kind=-1)
    refused(kind=4)
    refused(no_status=True)
    refused(clock=None)
    for name in COUNTERS:
        refused(**{name: None})
    refused(reserved=1)
    assert _call(lib, None, status, flags, iters, R, 1) == DSP_ERR_INVALID
    c.t["first"].zero_()
    assert _call(lib, c.h, status, flags, iters, R, 1) == 0               # the descriptor as built is accepted and books kind 1 only
    got = c.numpy()
    assert (got["solves"][1] == -7 + R).all() and (got["fail"][1] == -7 + R).all() and (got["first"] == 1).all()
    assert (np.delete(got["solves"], 1, axis=0) == -7).all()


def _health(loop):
    res, ok = loop.results()
    out = {k: v.cpu().numpy().copy() for k, v in res.items()}
    out.update((name, getattr(loop, name).cpu().numpy().copy()) for name in TENSORS)
    out["ok"], out["uncertified"] = np.array(ok), np.array(int(loop.uncertified.item()))
    return out


def _invariants(loop):
    assert bool(loop.bad.item()) == bool((loop.health_fail.sum() > 0).item())
    assert int(loop.uncertified.item()) == int(loop.health_waived.sum().item())


def _parametrized(B):
    k = np.arange(B)
    return dict(bidder="parametrized", bid_price=10.0 + 5.0 * (k % 4), storage_mw=50.0 * (1 + k % 5), market="price_taker")


# the iteration limits on the day-ahead handle: what about half of the batch needs, a multiple of the handle's check period, so that
# some rows end at status 1 and others at 0.  Measured on an MI355X under the default limit of 200 000: the 210 nuclear 48-h rows take
# 640 .. 2352 iterations (median 880 on day 0, 848 for the pending bid; checks every 16), the 5 coupled wind + PEM rows 216 .. 264
# (228, 228, 240, 264, 264 on day 0; checks every 12).  The test asserts that its limit still splits the batch.
CASES = {
    "nuclear_ruc": ("nuclear", 70, dict(STOCHASTIC, ruc_hour=16), 880),
    "wind_pem_monotone": ("wind_pem", 5, dict(MONOTONE, n_price_scenarios=2), 240),
    "wind_battery_parametrized": ("wind_battery", 5, None, None),
}


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_kernels_against_the_tensor_form(case):
    """use_fused True (dsp_loop_health) against False (_health_book), use_graphs=False, one day and two hours: all health_* tensors and
    results() equal exactly.  Both runs use the same solver under the same options, so they agree on every status - an iteration limit
    on the day-ahead handle makes part of the batch end at status 1, so that non-zero failure counters are what is compared."""
    flowsheet, B, kw, limit = CASES[case]
    runs = {}
    for fused in (True, False):
        loop = _loop(flowsheet, B, health=True, use_graphs=False, use_fused=fused, **(_parametrized(B) if kw is None else kw))
        assert loop.use_fused == fused
        if limit is not None:
            loop.da.opts.max_iter = limit
        loop.run_day()
        loop.day_ahead()
        loop.hour_step()
        loop.hour_step()
        _invariants(loop)
        runs[fused] = _health(loop)
    a, b = runs[True], runs[False]
    print(case, "failed rows per kind:", a["health_fail"].sum(1), "solves per plant:", a["health_solves"][:, 0], "largest iteration count per kind:",
          a["health_iters_max"].max(1))
    assert a.keys() == b.keys()
    for key in a:
        if key in ("obj", "energy_mwh") and not loop.exact:               # (delivered power and revenue of this mode: the tensor form sums in matrix
            np.testing.assert_allclose(a[key], b[key], rtol=1e-9, atol=1e-9, err_msg=key)      # order - the same solutions, another summation order)
        else:
            assert np.array_equal(a[key], b[key]), (case, key)
    S = loop.S
    if case == "nuclear_ruc":                                             # day 0: the bid of hour 0 and the pending bid of hour 16, 8 projection steps
        assert a["health_solves"][:, 0].tolist() == [2 * S, 26 * S, 26, 8]
    elif case == "wind_pem_monotone":
        assert a["health_solves"][:, 0].tolist() == [2, 26 * S, 26, 0]
    else:
        assert a["health_solves"][:, 0].tolist() == [0, 0, 26, 0] and a["valid"].all()
    if limit is not None:
        fail = a["health_fail"][0]
        assert 0 < fail.sum() < a["health_solves"][0].sum(), "the limit no longer splits the batch"
        assert (a["health_status"][0][fail > 0] == 2).all() and (a["health_iters_max"][0][fail > 0] == limit).all()
        assert not a["ok"] and not a["valid"].all()
        assert np.array_equal(a["first_failure_hour"] >= 0, ~a["valid"])
    assert (a["health_iters"][2] > 0).all() and (a["health_iters_max"][2] <= a["health_iters"][2]).all()


@gpu
def test_graph_replay_against_the_eager_loop():
    """nuclear B = 8, S = 3, three days: the counters from graphs (day 2 captured, day 3 replayed) equal the eager loop's, and
    health_solves shows that days 2 and 3 were booked - the booking is a kernel inside the captured steps, no memset"""
    runs = {}
    for graphs in (False, True):
        loop = _loop("nuclear", 8, health=True, use_graphs=graphs, **STOCHASTIC)
        for _ in range(3):
            loop.run_day()
        assert loop.use_fused and len(loop._graphs) == (25 if graphs else 0)
        _invariants(loop)
        runs[graphs] = _health(loop)
    for key in runs[False]:
        assert np.array_equal(runs[False][key], runs[True][key]), key
    assert np.array_equal(runs[True]["health_solves"], np.repeat(np.array([[9], [72 * 3], [72], [0]], np.int32), 8, axis=1))
    assert int(runs[True]["health_solves"].sum()) == loop.solves
    assert (runs[True]["health_iters"][:3] > 0).all() and runs[True]["valid"].all()


@gpu
def test_the_known_failing_shape():
    """wind + battery B = 90, S = 2 monotone, one day: the shape for which test_hip_monotone_loop.py documents coupled day-ahead rows at
    the iteration limit.  valid is False exactly where that day's day-ahead status is not 0 - whichever plants those are -, both
    invariants hold, and those plants' largest day-ahead iteration count is the limit.  If no row fails on the machine at hand, the
    equalities are still checked and the output says so."""
    loop = _loop("wind_battery", 90, health=True, use_graphs=False, **dict(MONOTONE, n_price_scenarios=2))
    loop.run_day()
    h = _health(loop)
    status = loop.da.out["status"].cpu().numpy()
    failed = status != 0
    limit = int(loop.da.opts.max_iter)
    print("known failing shape: plants at the iteration limit:", np.nonzero(failed)[0].tolist() or "NONE on this machine", "limit", limit,
          "day-ahead iterations: median", int(np.median(h["health_iters_max"][0])), "max", int(h["health_iters_max"][0].max()))
    _invariants(loop)
    assert not h["health_fail"][1:].any(), "an hourly or tracking LP failed"
    assert np.array_equal(h["valid"], ~failed) and np.array_equal(h["health_fail"][0], failed.astype(np.int32))
    assert np.array_equal(h["failed_solves"], failed.astype(np.int64)) and bool(h["ok"]) == (not failed.any())
    assert np.array_equal(h["first_failure_hour"], np.where(failed, 0, -1))
    assert (h["health_iters_max"][0][failed] == limit).all()
    assert np.array_equal(h["health_iters_max"][0], loop.da.out["iters"].cpu().numpy())
    assert np.array_equal(h["health_status"][0], np.where(failed, 1 << np.clip(status, 0, 29), 0))


@gpu
def test_health_changes_nothing_else():
    """nuclear B = 8, S = 3, two days from graphs, health=True against False: every other result and the trackers' solutions are
    bit-identical, as many graphs; health=False has no health_* attribute"""
    snaps = {}
    for health in (True, False):
        loop = _loop("nuclear", 8, use_graphs=True, **STOCHASTIC, **({"health": True} if health else {}))
        for _ in range(2):
            loop.run_day()
        assert loop.use_fused and len(loop._graphs) == 25
        res, ok = loop.results()
        assert ok
        snaps[health] = {k: v.cpu().numpy().copy() for k, v in res.items()}
        for name, m in (("da", loop.da), ("rt", loop.rt), ("tr", loop.tr)):
            for key in ("x", "obj", "status", "iters"):
                snaps[health][name + "_" + key] = m.out[key].cpu().numpy().copy()
        if not health:
            assert not [name for name in vars(loop) if name.startswith("health_")]
    assert set(snaps[True]) - set(snaps[False]) == {"valid", "failed_solves", "uncertified_solves", "first_failure_hour"}
    for key in snaps[False]:
        assert np.array_equal(snaps[False][key], snaps[True][key]), key
