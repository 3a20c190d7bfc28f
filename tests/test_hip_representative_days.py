"""GPU tests of the day profiles and the representative days (BatchedDoubleLoop(profiles=days); representative_days.py; dsp_loop_profile,
dsp_days_assign, dsp_days_update, dsp_days_frequency of csrc/dsp_days.hip, added under ABI 22): the profile kernel against the tensor
form inside the loop, eager and from graphs; each clustering kernel against the numpy statement at every size edge - labels, squared
distances and frequencies bit for bit, sums against math.fsum within the bound of a sum of n terms -; fit on planted data; the sweep end
to end; and every refusal of the entry points over sentinel-filled outputs."""
import ctypes as C
import math
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast", market="price_taker")
PARAMETRIZED = dict(bidder="parametrized", bid_price=[15.0, 20.0, 25.0, 30.0, 35.0], storage_mw=[50.0, 100.0, 200.0, 25.0, 150.0], market="price_taker")
DSP_ERR_INVALID = -1
U = 2.0 ** -53


def _loop(flowsheet, B, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    return BatchedDoubleLoop(flowsheet, B, device=0, **kw)


def _twin(loop):
    """a second profile buffer on the same loop that takes the TENSOR form whenever the loop's kernel writes: both read the same live
    `delivered` and the same clock at the same moment"""
    import torch
    twin = torch.zeros_like(loop.profile)
    write = loop._profile_write

    def both():
        write()
        loop._profile_write_tensors(twin)
    loop._profile_write = both
    return twin


@gpu
@pytest.mark.parametrize("case", ["nuclear_70x3", "wind_pem_parametrized_5"])
def test_profile_kernel_is_bit_identical_to_the_tensor_form(case):
    """Two days, use_graphs=False.  (a) in the fused loop, the kernel's profile against the tensor form of the same writes on the same
    live buffers, bit for bit, spare row included, and row (d, h) is the delivered power seen after that hour.  (b) use_fused True
    against False: the profiles bit for bit where the loop's tensor form states the hand-off exactly (`exact`), else to 1e-12, as the
    recorder's test compares `delivered`.  B = 70 crosses a wave."""
    flowsheet, B, kw = ("nuclear", 70, STOCHASTIC) if case == "nuclear_70x3" else ("wind_pem", 5, PARAMETRIZED)
    fused = _loop(flowsheet, B, profiles=2, use_graphs=False, use_fused=True, **kw)
    tensor = _loop(flowsheet, B, profiles=2, use_graphs=False, use_fused=False, **kw)
    assert fused.use_fused and not tensor.use_fused and fused.profile.shape == (3, 24, B)
    twin = _twin(fused)
    seen = np.zeros((2, 24, B))
    for day in range(2):
        fused.day_ahead()
        for h in range(24):
            seen[day, h] = fused.hour_step().cpu().numpy()
        tensor.run_day()
    assert fused.results()[1] and tensor.results()[1]
    got = fused.profile.cpu().numpy()
    assert np.array_equal(got, twin.cpu().numpy()) and np.array_equal(got[:2], seen) and seen.any() and not got[2].any()
    assert np.array_equal(fused.profiles_host(), seen.transpose(2, 0, 1))
    if fused.exact:
        assert np.array_equal(got, tensor.profile.cpu().numpy())
    else:
        np.testing.assert_allclose(got, tensor.profile.cpu().numpy(), rtol=1e-12, atol=0)
    fused.reset()
    assert not fused.profile.any().item()


@gpu
def test_graph_replay_writes_the_profile_the_eager_loop_writes():
    """nuclear, B = 70 x S = 3, three days: eager against graphs (day 2 captured, day 3 replayed) - the profiles bit for bit, and the
    launch sits inside the captured steps: 24 + 1 graphs, as many as a loop without profiles has"""
    out = {}
    for graphs in (False, True):
        loop = _loop("nuclear", 70, profiles=3, use_graphs=graphs, **STOCHASTIC)
        for _ in range(3):
            loop.run_day()
        assert loop.use_fused and int(loop.hour_t.item()) == 72 and loop.results()[1]
        assert len(loop._graphs) == (25 if graphs else 0)
        out[graphs] = loop.profile.cpu().numpy()
    plain = _loop("nuclear", 70, use_graphs=True, **STOCHASTIC)
    for _ in range(2):
        plain.run_day()
    assert len(plain._graphs) == 25 and not hasattr(plain, "profile")
    assert np.array_equal(out[False], out[True]) and out[True][:3].all() and not out[True][3].any()


@gpu
def test_days_past_the_span_land_in_the_spare_row():
    """profiles=1 over two days (the second from graphs): day 2 sits in the spare row hour by hour and row 0 is untouched"""
    loop = _loop("wind_pem", 5, profiles=1, **PARAMETRIZED)
    loop.run_day()
    first = loop.profile[0].cpu().numpy().copy()
    assert first.any() and not loop.profile[1].any().item()
    loop.day_ahead()
    second = np.stack([loop.hour_step().cpu().numpy() for _ in range(24)])
    assert np.array_equal(loop.profile[0].cpu().numpy(), first) and np.array_equal(loop.profile[1].cpu().numpy(), second)
    assert not np.array_equal(first, second) and loop.profiles_host().shape == (5, 1, 24)


@gpu
def test_profile_kernel_alone_at_the_clock_edges():
    """dsp_loop_profile on buffers of its own, B = 257 (past one block), days = 2: clocks 1, 24, 25, 48, 49 and one far past the span write
    exactly the row the header states - the spare row from day 2 on -, a clock of 0 writes hour 0 of the spare row, nothing else moves"""
    import torch
    from dispatches_amd.hip_solver import DspLoopProfileDesc, load_library
    lib, dev = load_library(), torch.device("cuda", 0)
    B, days = 257, 2
    profile = torch.full((days + 1, 24, B), -7.0, dtype=torch.float64, device=dev)
    delivered, clock = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    d = DspLoopProfileDesc()
    d.B, d.days, d.clock, d.delivered, d.profile = B, days, clock.data_ptr(), delivered.data_ptr(), profile.data_ptr()
    want = profile.cpu().numpy().copy()
    for call, (now, row) in enumerate([(1, (0, 0)), (24, (0, 23)), (25, (1, 0)), (48, (1, 23)), (49, (2, 0)), (24 * 1000 + 6, (2, 5)), (0, (2, 0))]):
        clock.fill_(now)
        delivered.copy_(torch.arange(B, dtype=torch.float64, device=dev) + 1000.0 * call)
        assert lib.dsp_loop_profile(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        want[row] = delivered.cpu().numpy()
        assert np.array_equal(profile.cpu().numpy(), want), (now, row)


# ---- the clustering kernels against the numpy statement ---------------------------------------------------------------------------------
def _case(B, days, K, channels, seed):
    """profile [days, 24, B] with zero days, full days and random days over per-plant scaling ranges; K centres of which 0 and 1 are
    identical (K >= 2) and, with K >= 3, centre 2 = centre 0 + 1/8 and point (day 0, plant 0) = centre 0 + 1/16 in every feature, all
    dyadic: exactly between the two, so that the accumulated squares tie bit for bit; a series of N = 24 days + 5 hours that the
    plants' windows wrap"""
    rng = np.random.default_rng(seed)
    F, N = 24 * channels, 24 * days + 5
    p_min, p_max = rng.integers(0, 300, size=B).astype(np.float64), rng.integers(301, 900, size=B).astype(np.float64)
    if K >= 3:
        p_min[0], p_max[0] = 0.0, 1.0                    # cf = (p - 0) / (1 - 0) = p exactly
    kind = rng.integers(0, 5, size=(days, B))            # 0: a zero day, 1: a full day, else random
    profile = p_min + rng.random((days, 24, B)) * (p_max - p_min)
    profile = np.where(kind[:, None, :] == 0, p_min, np.where(kind[:, None, :] == 1, p_max, profile))
    series, start = rng.random(N), rng.integers(0, N, size=B)
    start[0] = N - 7
    centers = rng.random((K, F))
    if K >= 2:
        centers[0] = rng.integers(8, 48, size=F) / 64.0
        centers[1] = centers[0]
    if K >= 3:
        centers[2] = centers[0] + 0.125
        profile[0, :, 0] = centers[0, :24] + 0.0625
        if channels == 2:
            series[(start[0] + np.arange(24)) % N] = centers[0, 24:] + 0.0625
    return dict(profile=np.ascontiguousarray(profile), p_min=p_min, p_max=p_max, series=series, start=start, centers=centers, kind=kind)


def _points(case, channels, filter_days=True):
    import torch
    from dispatches_amd import representative_days as rd
    dev = torch.device("cuda", 0)
    two = channels == 2
    view = rd.Profiles(torch.as_tensor(case["profile"], device=dev), torch.as_tensor(case["series"], device=dev) if two else None,
                       torch.as_tensor(case["start"], device=dev) if two else None)
    points = rd.DayPoints(view, channels=channels, filter_days=filter_days, p_min=case["p_min"], p_max=case["p_max"])
    assert points.kernels
    X = rd.points(case["profile"], case["p_min"], case["p_max"], channels, case["series"] if two else None, case["start"] if two else None)
    return points, X


@gpu
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("K", [1, 2, 20, 64])
@pytest.mark.parametrize("days", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_assign_against_the_numpy_statement(B, days, K, channels):
    """labels and dist2 bit for bit; B = 63 / 65 sit on either side of a wave, 257 past a block; the inputs hold zero days, full days,
    two identical centres (the lower index wins) and a point exactly between two centres (the lower index wins); the plants' windows
    of the second channel wrap the series.  Without the filter the same days are clustered like any other."""
    from dispatches_amd import representative_days as rd
    case = _case(B, days, K, channels, 1000 * B + 100 * days + 2 * K + channels)
    points, X = _points(case, channels)
    label, dist2 = points.assign(case["centers"])
    want_label, want_dist2 = rd.assign(X, case["centers"])
    label, dist2 = label.cpu().numpy(), dist2.cpu().numpy()
    assert label.shape == (days, B) and label.dtype == np.int32 and dist2.dtype == np.float64
    assert np.array_equal(label.reshape(-1), want_label) and np.array_equal(dist2.reshape(-1), want_dist2)
    kind = case["kind"].copy()
    if K >= 3:
        kind[0, 0] = 2
        assert label[0, 0] == 0 and dist2[0, 0] == 24 * channels / 256.0      # the tie: 1/16 from centres 0, 1 and 2
    assert np.array_equal(label == -1, kind == 0) and np.array_equal(label == -2, kind == 1) and not (label == 1).any()
    plain, _ = _points(case, channels, filter_days=False)
    label, dist2 = plain.assign(case["centers"])
    want_label, want_dist2 = rd.assign(X, case["centers"], filter_days=False)
    assert np.array_equal(label.cpu().numpy().reshape(-1), want_label) and np.array_equal(dist2.cpu().numpy().reshape(-1), want_dist2)
    assert (want_label >= 0).all()


def _fsum_bounds(X, label, dist2, centers, count, inertia, old):
    """the derived bound on a sum of n terms taken in any order, n * 2^-53 * max|x|, for every centre entry and the inertia against
    math.fsum; an empty cluster keeps its centre"""
    for k in range(len(centers)):
        rows = X[label == k]
        assert count[k] == len(rows)
        if len(rows) == 0:
            assert np.array_equal(centers[k], old[k])
            continue
        for j in range(X.shape[1]):
            assert abs(centers[k, j] - math.fsum(rows[:, j]) / len(rows)) <= len(rows) * U * np.abs(rows[:, j]).max(), (k, j)
    keep = label >= 0
    assert abs(inertia - math.fsum(dist2[keep]) / keep.sum()) <= keep.sum() * U * dist2[keep].max()


@gpu
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("B, days", [(65, 3), (257, 9)])
def test_update_counts_order_and_bounds(B, days, channels):
    """K = 6 with one centre far away (no member): counts exact, two calls on the same input give the same bits, the empty cluster keeps
    its centre, every centre entry and the inertia within n * 2^-53 * max|x| of math.fsum's mean; and the kernels' fixed order is the
    numpy statement's, bit for bit.  257 x 9 = 2313 points are three chunks, 65 x 3 part of one."""
    from dispatches_amd import representative_days as rd
    case = _case(B, days, 6, channels, 77 * B + channels)
    case["centers"][5] = 50.0
    points, X = _points(case, channels)
    label, dist2 = points.assign(case["centers"])
    first = points.update(label, dist2, case["centers"])
    again = points.update(label, dist2, case["centers"])
    for a, b in zip(first, again):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    centers, count, inertia = first
    label_h, dist2_h = label.cpu().numpy().reshape(-1), dist2.cpu().numpy().reshape(-1)
    assert count.dtype == np.int64 and count[5] == 0 and count.sum() == (label_h >= 0).sum() > 0 and (label_h < 0).any()
    _fsum_bounds(X, label_h, dist2_h, centers, count, inertia, case["centers"])
    want = rd.update(X, label_h, dist2_h, case["centers"])
    assert np.array_equal(centers, want[0]) and np.array_equal(count, want[1]) and inertia == want[2]


@gpu
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("B, days, K", [(1, 1, 1), (63, 3, 2), (65, 7, 20), (257, 3, 64)])
def test_frequency_against_the_numpy_statement(B, days, K, channels):
    """freq [B, K + 2] equals the numpy statement exactly and every row sums to 1 within 4 ulp; without the filter [B, K]"""
    from dispatches_amd import representative_days as rd
    case = _case(B, days, K, channels, 31 * B + K)
    for filter_days in (True, False):
        points, X = _points(case, channels, filter_days)
        freq = points.frequency(case["centers"]).cpu().numpy()
        want = rd.frequency(rd.assign(X, case["centers"], filter_days)[0].reshape(days, B), K, filter_days)
        assert freq.shape == (B, K + 2 if filter_days else K) and np.array_equal(freq, want)
        assert np.abs(freq.sum(1) - 1.0).max() <= 4 * np.finfo(float).eps


def _planted(seed=8):
    """5 well separated 24-value shapes plus noise 0.01, 3 days x 257 plants"""
    rng = np.random.default_rng(seed)
    days, B = 3, 257
    shapes = np.repeat(np.array([0.1, 0.3, 0.5, 0.7, 0.9]), 24).reshape(5, 24) + 0.05 * rng.random((5, 24))
    member = rng.integers(0, 5, size=(days, B))
    cf = shapes[member] + 0.01 * rng.standard_normal((days, B, 24))
    case = dict(profile=np.ascontiguousarray(cf.transpose(0, 2, 1)), p_min=np.zeros(B), p_max=np.ones(B), series=None, start=None)
    return case, shapes, member


def _same_partition(a, b, groups):
    pairs = {(int(x), int(y)) for x, y in zip(np.ravel(a), np.ravel(b))}
    return len(pairs) == groups and len({x for x, _ in pairs}) == groups and len({y for _, y in pairs}) == groups


@gpu
def test_fit_on_planted_data():
    """init given: labels and n_iter equal the numpy statement's Lloyd run from the same init, the centres within the bound of
    test_update_counts_order_and_bounds against math.fsum's means; init="k-means++" with a seed recovers the 5 planted groups, compared
    as partitions"""
    from dispatches_amd import representative_days as rd
    case, shapes, member = _planted()
    points, X = _points(case, 1)
    init = shapes[::-1] + 0.03
    fit = points.fit(5, init=init)
    centers, inertia, n_iter = rd.lloyd(lambda c: rd.assign(X, c), lambda lab, d2, c: rd.update(X, lab, d2, c), init)
    labels = fit.labels.cpu().numpy()
    assert fit.n_iter == n_iter and 2 <= n_iter < 50 and np.array_equal(labels.reshape(-1), rd.assign(X, centers)[0])
    assert np.array_equal(labels, 4 - member)             # (init is the shapes in reverse order)
    for k in range(5):
        rows = X[labels.reshape(-1) == k]
        for j in range(24):
            assert abs(fit.centers[k, j] - math.fsum(rows[:, j]) / len(rows)) <= len(rows) * U * np.abs(rows[:, j]).max()
    d2 = rd.assign(X, fit.centers)[1]                     # (the last iteration changed no centre: its distances are these)
    assert abs(fit.inertia - math.fsum(d2) / len(d2)) <= len(d2) * U * d2.max() and fit.inertia == inertia
    seeded = points.fit(5, seed=42)
    assert _same_partition(member, seeded.labels.cpu().numpy(), 5) and seeded.n_iter < 50
    assert np.array_equal(points.fit(5, seed=42).centers, seeded.centers)


@gpu
def test_nuclear_sweep_returns_the_dispatch_frequency(monkeypatch):
    """nuclear_sweep([1, 2] $/kg x [100, 200] MW x 3 windows, 3 days) under the reference's 30 x 24 centres: dispatch_frequency is
    [2, 2, 3, 32], equals the numpy statement applied to profiles_host() with p_min = p_max - pem_mw, and all_optimal holds"""
    from dispatches_amd import representative_days as rd
    from dispatches_amd import sweeps
    with np.load(os.path.join(ROOT, "tests", "golden", "representative_days_reference.npz")) as f:
        centers = f["ne_centers"].copy()
    seen, real = {}, sweeps._representative_days

    def spy(loop, *args):
        seen["loop"] = loop
        return real(loop, *args)
    monkeypatch.setattr(sweeps, "_representative_days", spy)
    out = sweeps.nuclear_sweep([1.0, 2.0], [100.0, 200.0], 3, 3, representative_days=centers)
    loop = seen["loop"]
    assert out["all_optimal"] and loop.use_fused and out["dispatch_frequency"].shape == (2, 2, 3, 32) and np.array_equal(out["day_centers"], centers)
    host = loop.profiles_host()
    assert host.shape == (12, 3, 24) and host.all()
    top = float(loop.bidder.bidding_model_object.model_data.p_max)
    pem = sweeps.nuclear_layout([1.0, 2.0], [100.0, 200.0], 3)[1]
    X = rd.points(host.transpose(1, 2, 0), top - pem, np.full(12, top))
    want = rd.frequency(rd.assign(X, centers)[0].reshape(3, 12), 30)
    assert np.array_equal(out["dispatch_frequency"].reshape(12, 32), want)
    assert np.abs(out["dispatch_frequency"].sum(-1) - 1.0).max() <= 4 * np.finfo(float).eps


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_malformed_descriptors_are_refused_and_nothing_is_written():
    """every entry point, one broken field or argument at a time, over sentinel-filled outputs: DSP_ERR_INVALID and nothing written; the
    unedited calls return 0 and write; B == 0 returns 0 and writes nothing"""
    import torch
    from dispatches_amd.hip_solver import DspDaysDesc, DspLoopProfileDesc, load_library
    lib, dev = load_library(), torch.device("cuda", 0)
    B, days, K, N = 9, 2, 3, 53
    f64 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    profile, p_min, p_max, series = f64(days + 1, 24, B), torch.zeros(B, dtype=torch.float64, device=dev), f64(B).fill_(2.0), f64(N).fill_(0.5)
    start, clock, delivered = torch.arange(B, dtype=torch.int64, device=dev), torch.ones((), dtype=torch.int64, device=dev), f64(B).fill_(1.0)
    centers, label, dist2 = f64(K, 48).fill_(0.25), torch.full((days, B), -7, dtype=torch.int32, device=dev), f64(days, B)
    count, inertia, freq = torch.full((K,), -7, dtype=torch.int64, device=dev), f64(1), f64(B, K + 2)
    n_work = lib.dsp_days_work_doubles(B * days, K, 2)
    work = f64(n_work)
    outputs = [profile, label, dist2, count, inertia, freq, work, centers]
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def sound():
        d = DspDaysDesc()
        d.B, d.days, d.channels, d.filter, d.N = B, days, 2, 1, N
        d.profile, d.p_min, d.p_max, d.cf_series, d.start = (t.data_ptr() for t in (profile, p_min, p_max, series, start))
        p = DspLoopProfileDesc()
        p.B, p.days, p.clock, p.delivered, p.profile = B, days, clock.data_ptr(), delivered.data_ptr(), profile.data_ptr()
        return d, p

    def calls(d, p, K=K, c=centers, lab=label, d2=dist2, cnt=count, ine=inertia, fr=freq, wk=work, n=n_work):
        return dict(profile=lambda: lib.dsp_loop_profile(None if p is None else C.byref(p), stream()),
                    assign=lambda: lib.dsp_days_assign(None if d is None else C.byref(d), ptr(c), K, ptr(lab), ptr(d2), stream()),
                    update=lambda: lib.dsp_days_update(None if d is None else C.byref(d), ptr(lab), ptr(d2), K, ptr(c), ptr(cnt), ptr(ine), ptr(wk), n, stream()),
                    frequency=lambda: lib.dsp_days_frequency(None if d is None else C.byref(d), ptr(lab), K, ptr(fr), stream()))

    before = [t.clone() for t in outputs]

    def refused(which, **kw):
        d, p = sound()
        edit = kw.pop("edit", None)
        if edit:
            edit(d, p)
        if kw.pop("null", False):
            d, p = None, None
        table = calls(d, p, **kw)
        for name in which:
            assert table[name]() == DSP_ERR_INVALID, (name, kw)
        torch.cuda.synchronize()
        for t, keep in zip(outputs, before):
            assert torch.equal(t, keep)
    days_calls, every = ("assign", "update", "frequency"), ("profile", "assign", "update", "frequency")
    refused(every, null=True)
    for field, values in (("B", (-1, 2 ** 24 + 1, -2 ** 31)), ("days", (0, -1, 65537, 2 ** 31 - 1))):
        for v in values:
            refused(every, edit=lambda d, p, f=field, v=v: (setattr(d, f, v), setattr(p, f, v)))
    for field in ("profile", "p_min", "p_max", "cf_series", "start"):
        refused(days_calls, edit=lambda d, p, f=field: setattr(d, f, None))
    for field in ("clock", "delivered", "profile"):
        refused(("profile",), edit=lambda d, p, f=field: setattr(p, f, None))
    for field, values in (("channels", (0, 3, -1)), ("filter", (2, -1)), ("N", (0, -1))):
        for v in values:
            refused(days_calls, edit=lambda d, p, f=field, v=v: setattr(d, f, v))
    refused(days_calls, edit=lambda d, p: (setattr(d, "B", 32768), setattr(d, "days", 65536)))          # 2^31 points
    for q in range(4):
        refused(every, edit=lambda d, p, q=q: (d.reserved.__setitem__(q, 1), p.reserved.__setitem__(q, 1)))
    for bad_K in (0, -1, 65, 2 ** 31 - 1):
        refused(days_calls, K=bad_K)
    refused(("assign", "update"), c=None)
    refused(days_calls, lab=None)
    refused(("assign", "update"), d2=None)
    refused(("update",), cnt=None)
    refused(("update",), ine=None)
    refused(("update",), wk=None)
    refused(("update",), n=n_work - 1)
    refused(("frequency",), fr=None)
    # B == 0: DSP_OK, nothing launched, nothing written
    d, p = sound()
    d.B = p.B = 0
    assert [fn() for fn in calls(d, p).values()] == [0, 0, 0, 0]
    torch.cuda.synchronize()
    for t, keep in zip(outputs, before):
        assert torch.equal(t, keep)
    # the unedited calls: the profile row of clock 1, every label and distance, the centres' counts, the frequencies
    d, p = sound()
    table = calls(d, p)
    assert table["profile"]() == 0
    profile[:days].fill_(1.0)                               # cf = 0.5 everywhere, the series too
    assert table["assign"]() == 0 and table["update"]() == 0 and table["frequency"]() == 0
    torch.cuda.synchronize()
    assert (profile[0, 0] == 1.0).all().item() and (profile[2] == -7.0).all().item()
    assert (label == 0).all().item() and torch.equal(dist2, torch.full_like(dist2, 48 * 0.0625))
    assert count.tolist() == [B * days, 0, 0] and inertia.item() == 3.0 and (centers[0] == 0.5).all().item() and (centers[1:] == 0.25).all().item()
    assert torch.equal(freq[:, 1], torch.ones(B, dtype=torch.float64, device=dev)) and freq.sum().item() == B
