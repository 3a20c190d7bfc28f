"""Representative days without a GPU (dispatches_amd/representative_days.py; BatchedDoubleLoop(profiles=days)): the reference's own label
test, the numpy statement against an independent restatement of Train_NN_Surrogates._generate_label_data under both of the reference's
shipped centre sets, the loop's profile buffer on the CPU backend of the tests (HiGHS per LP) against the delivered power seen hour by
hour, the refusals by their messages, the C ABI's mirror, and the entry points' host checks as a stand-alone program under the host
sanitizers."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOCHASTIC = dict(n_price_scenarios=3, forecaster="backcast", max_historical_days=10, market="price_taker")
PARAMETRIZED = dict(bidder="parametrized", bid_price=[15.0, 25.0], storage_mw=[50.0, 200.0], market="price_taker")


def _loop(flowsheet, B, **kw):
    from dispatches_amd.rolling_flowsheets import BatchedDoubleLoop
    from tests._highs_solver import HighsTensorLP
    return BatchedDoubleLoop(flowsheet, B, lp_backend=HighsTensorLP, **kw)


@pytest.fixture(scope="module")
def reference_centers():
    with np.load(os.path.join(ROOT, "tests", "golden", "representative_days_reference.npz")) as f:
        return {"re": f["re_centers"].copy(), "ne": f["ne_centers"].copy()}


def test_reference_centers_fixture(reference_centers):
    """tools/extract_reference_clusters.py: the centres of the reference's two shipped clusterings, and nothing else"""
    assert reference_centers["re"].shape == (20, 48) and reference_centers["ne"].shape == (30, 24)
    assert np.isfinite(reference_centers["re"]).all() and np.isfinite(reference_centers["ne"]).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "representative_days_reference.npz")) < 64 * 1024


def test_reference_pin_generate_label_data():
    """the reference's own test_generate_label_data: three plants held for a year of 366 days at p_min, at p_min + 0.25 (p_max - p_min)
    and at p_max (200 / 340 / 400 MW with p_min 200 / 320 / 120, p_max 400), one centre 24 x 0.25: the frequencies are exactly
    [1, 0, 0], [0, 1, 0], [0, 0, 1] - by the numpy statement and through DayPoints over the same profile"""
    import torch
    from dispatches_amd import representative_days as rd
    p_min, p_max = np.array([200.0, 320.0, 120.0]), np.array([400.0, 400.0, 400.0])
    profile = np.broadcast_to(np.array([200.0, 340.0, 400.0]), (366, 24, 3)).copy()
    centers = np.full((1, 24), 0.25)
    X = rd.points(profile, p_min, p_max)
    label, dist2 = rd.assign(X, centers)
    want = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    assert np.array_equal(rd.frequency(label.reshape(366, 3), 1), want)
    assert np.array_equal(label.reshape(366, 3)[0], [-1, 0, -2]) and not dist2.any()
    points = rd.DayPoints(rd.Profiles(torch.as_tensor(profile)), p_min=p_min, p_max=p_max)
    assert not points.kernels and points.days == 366
    assert np.array_equal(points.frequency(centers).numpy(), want)
    # without the filter there is one column, and every day is nearest to the only centre
    plain = rd.DayPoints(rd.Profiles(torch.as_tensor(profile)), filter_days=False, p_min=p_min, p_max=p_max)
    assert np.array_equal(plain.frequency(centers).numpy(), np.ones((3, 1)))


def _generate_label_data(dispatch, p_min, p_max, centers, wind=None):
    """Train_NN_Surrogates._generate_label_data (filter_opt=True) restated independently of representative_days.py: Python floats and
    Python's sum for the scaling and the day classes, scipy's cdist(...).argmin for clustering_model.predict, numpy.unique for the counts.
    dispatch [B][D * 24] MW; wind [B][D * 24] the second channel or None.  -> (frequencies [B][K + 2], smallest gap between the best and
    the second-best distance over all clustered days)"""
    from scipy.spatial.distance import cdist
    K, out, gap = len(centers), [], np.inf
    for b in range(len(dispatch)):
        year = [(float(p) - float(p_min[b])) / (float(p_max[b]) - float(p_min[b])) for p in dispatch[b]]
        day_num = int(len(year) / 24)
        zero_day = full_day = 0
        kept = []
        for day in range(day_num):
            sim_day_data = year[day * 24:(day + 1) * 24]
            if sum(sim_day_data) == 0:
                zero_day += 1
            elif sum(sim_day_data) == 24:
                full_day += 1
            else:
                kept.append(sim_day_data + ([float(w) for w in wind[b][day * 24:(day + 1) * 24]] if wind is not None else []))
        if kept:
            dist = cdist(np.array(kept), centers)
            labels = dist.argmin(1)
            if K > 1:
                two = np.sort(dist, axis=1)[:, :2]
                gap = min(gap, float((two[:, 1] - two[:, 0]).min()))
        else:
            labels = np.array([])
        elements, count = np.unique(labels, return_counts=True)
        found = dict(zip(elements, count))
        out.append([zero_day / day_num] + [found[j] / day_num if j in found else 0 for j in range(K)] + [full_day / day_num])
    return np.array(out, np.float64), gap


@pytest.mark.parametrize("case", ["re", "ne"])
def test_numpy_statement_against_the_restated_reference(case, reference_centers):
    """seeded random profiles mixed with zero and full days, B = 7 plants of different scaling ranges over 40 days; channels=2 under the
    reference's 20 x 48 centres (wind + PEM) and channels=1 under its 30 x 24 (nuclear): frequencies equal exactly.  The seed is such that
    for every clustered day the best and the second-best distance differ by more than 1e-9 - asserted -, so the squared and the rooted
    argmin cannot part."""
    from dispatches_amd import representative_days as rd
    centers = reference_centers[case]
    channels = centers.shape[1] // 24
    rng = np.random.default_rng(20260 + channels)
    B, D, N = 7, 40, 24 * 55 + 7
    p_min = np.array([0.0, 0.0, 400.0, 300.0, 12.5, 0.0, 100.0])
    p_max = np.array([847.0, 120.0, 500.0, 500.0, 50.0, 1.0, 400.0])
    cf = rng.random((D, 24, B))
    shape = rng.integers(0, 4, size=(D, B))              # 0: a zero day, 1: a full day, else: a day to cluster
    cf = np.where(shape[:, None, :] == 0, 0.0, np.where(shape[:, None, :] == 1, 1.0, cf))
    profile = p_min + cf * (p_max - p_min)
    profile = np.where(shape[:, None, :] == 0, p_min, np.where(shape[:, None, :] == 1, p_max, profile))     # the two ends exactly
    series, start = rng.random(N), rng.integers(0, N, size=B)
    start[0], start[1] = N - 5, N - 24 * D + 3           # windows that wrap the series
    X = rd.points(profile, p_min, p_max, channels, series, start)
    label, _ = rd.assign(X, centers)
    got = rd.frequency(label.reshape(D, B), len(centers))
    dispatch = profile.transpose(2, 0, 1).reshape(B, D * 24)
    wind = np.array([[series[(start[b] + t) % N] for t in range(D * 24)] for b in range(B)]) if channels == 2 else None
    want, gap = _generate_label_data(dispatch, p_min, p_max, centers, wind)
    assert gap > 1e-9, gap
    assert (got[:, 0] > 0).all() and (got[:, -1] > 0).all() and (got[:, 1:-1].sum(1) > 0).all()      # every plant has days of all three kinds
    assert np.array_equal(got, want)
    assert np.abs(got.sum(1) - 1.0).max() <= 4 * np.finfo(float).eps


def test_numpy_update_and_lloyd_on_planted_groups():
    """the numpy statement's update: exact counts, means within n_k * 2^-53 * max|x| of math.fsum's, an empty cluster keeps its centre,
    labels outside 0 .. K - 1 are skipped; and Lloyd from a given init recovers three planted groups and stops on an unchanged inertia"""
    import math
    from dispatches_amd import representative_days as rd
    rng = np.random.default_rng(5)
    shapes = rng.random((3, 24))
    member = rng.integers(0, 3, size=2500)
    X = shapes[member] + 0.01 * rng.standard_normal((2500, 24))
    label, dist2 = rd.assign(X, shapes, filter_days=False)
    assert np.array_equal(label, member)
    label = label.copy()
    label[::50] = -1                                     # a set-aside day does not move a centre
    old = np.vstack([shapes, np.full((1, 24), 7.0)])      # centre 3 has no member
    new, count, inertia = rd.update(X, label, dist2, old)
    keep = label >= 0
    assert np.array_equal(count, [np.sum(label == k) for k in range(4)]) and count[3] == 0 and np.array_equal(new[3], old[3])
    for k in range(3):
        rows = X[label == k]
        for j in range(24):
            assert abs(new[k, j] - math.fsum(rows[:, j]) / len(rows)) <= len(rows) * 2.0 ** -53 * np.abs(rows[:, j]).max()
    assert abs(inertia - math.fsum(dist2[keep]) / keep.sum()) <= keep.sum() * 2.0 ** -53 * dist2[keep].max()
    start = shapes + 0.05
    centers, last, n_iter = rd.lloyd(lambda c: rd.assign(X, c, False), lambda lab, d2, c: rd.update(X, lab, d2, c), start)
    assert n_iter == 3 and np.array_equal(rd.assign(X, centers, False)[0], member) and np.abs(centers - shapes).max() < 0.005
    assert last < 24 * 0.01 ** 2 * 1.5


def test_fit_with_seeded_kmeans_plus_plus_on_the_numpy_path():
    """DayPoints.fit over a profile on the CPU (the numpy statement): k-means++ from a seed recovers four planted groups as a partition,
    the same seed gives the same centres, and the returned labels are the assignment under the returned centres"""
    import torch
    from dispatches_amd import representative_days as rd
    rng = np.random.default_rng(11)
    D, B = 30, 41
    shapes = np.repeat(np.array([0.1, 0.35, 0.6, 0.85]), 24).reshape(4, 24) + 0.05 * rng.random((4, 24))
    member = rng.integers(0, 4, size=(D, B))
    cf = shapes[member] + 0.01 * rng.standard_normal((D, B, 24))
    points = rd.DayPoints(rd.Profiles(torch.as_tensor(np.ascontiguousarray(cf.transpose(0, 2, 1)))), p_min=0.0, p_max=1.0)
    fit = points.fit(4, seed=3)
    labels = fit.labels.numpy()
    assert fit.n_iter <= 50 and fit.centers.shape == (4, 24) and labels.shape == (D, B)
    pairs = {(int(a), int(b)) for a, b in zip(member.reshape(-1), labels.reshape(-1))}
    assert len(pairs) == 4 and len({a for a, _ in pairs}) == 4 and len({b for _, b in pairs}) == 4       # a bijection of the groups
    assert np.array_equal(points.fit(4, seed=3).centers, fit.centers)
    assert np.array_equal(points.assign(fit.centers)[0].numpy(), labels)


# mode -> (flowsheet, plants, constructor arguments)
LOOPS = {"nuclear_stochastic": ("nuclear", 3, STOCHASTIC), "wind_pem_parametrized": ("wind_pem", 2, PARAMETRIZED)}


@pytest.mark.parametrize("mode", list(LOOPS))
def test_loop_profile_equals_delivered_hour_by_hour(mode):
    """profiles=2, three days stepped by hand: profile[d, h, b] is the delivered power seen after hour h of day d, day 3 sits in the spare
    row, profiles_host() is [B, whole days run, 24] cut to the span, DayPoints over the loop equals the numpy statement on
    profiles_host(), and reset() zeroes the buffer"""
    from dispatches_amd import representative_days as rd
    flowsheet, B, kw = LOOPS[mode]
    loop = _loop(flowsheet, B, profiles=2, **kw)
    assert loop.profile.shape == (3, 24, B) and loop.profile_bytes == 3 * 24 * B * 8 and not loop.profile.numpy().any()
    seen = np.zeros((3, 24, B))
    for day in range(3):
        loop.day_ahead()
        for h in range(24):
            delivered = loop.hour_step().numpy()
            seen[day, h] = delivered
            assert np.array_equal(loop.profile[min(day, 2), h].numpy(), delivered), (day, h)
        assert loop.profiles_host().shape == (B, min(day + 1, 2), 24)
    assert seen.any() and np.array_equal(loop.profile.numpy(), seen)
    assert np.array_equal(loop.profiles_host(), seen[:2].transpose(2, 0, 1))
    points = rd.DayPoints(loop)
    assert not points.kernels and points.days == 2
    centers = np.stack([np.full(24, 0.2), np.full(24, 0.9)])
    X = rd.points(loop.profiles_host().transpose(1, 2, 0), points.p_min, points.p_max)
    label, dist2 = points.assign(centers)
    want_label, want_dist2 = rd.assign(X, centers)
    assert np.array_equal(label.numpy().reshape(-1), want_label) and np.array_equal(dist2.numpy().reshape(-1), want_dist2)
    freq = points.frequency(centers).numpy()
    assert freq.shape == (B, 4) and np.array_equal(freq, rd.frequency(want_label.reshape(2, B), 2))
    if flowsheet == "nuclear":                           # Simulation_Data._read_NE_pmin: p_max - PEM size .. p_max
        assert np.array_equal(points.p_max - points.p_min, np.full(B, 100.0)) and (points.p_max == points.p_max[0]).all()
    else:
        assert not points.p_min.any() and np.array_equal(points.p_max, np.full(B, loop.wind_mw))
    loop.reset()
    assert not loop.profile.numpy().any() and loop.profiles_host().shape == (B, 0, 24)


def test_profiles_none_is_the_loop_as_it_was():
    """profiles=None against a loop built without the argument against profiles=2, one day: results() bit for bit, same keys, and no
    `profile` attribute without profiles"""
    flowsheet, B, kw = LOOPS["wind_pem_parametrized"]
    loops = [_loop(flowsheet, B, **kw), _loop(flowsheet, B, profiles=None, **kw), _loop(flowsheet, B, profiles=2, **kw)]
    for loop in loops:
        loop.run_day()
    assert not hasattr(loops[0], "profile") and not hasattr(loops[1], "profile") and hasattr(loops[2], "profile")
    (plain, ok), others = loops[0].results(), [loop.results() for loop in loops[1:]]
    for res, ok_other in others:
        assert ok_other == ok and list(res) == list(plain)
        for key in plain:
            assert np.array_equal(res[key].numpy(), plain[key].numpy()), key
    with pytest.raises(RuntimeError, match="keeps no profiles"):
        loops[1].profiles_host()


@pytest.mark.parametrize("profiles, kw, match", [
    (0, {}, "integer number of days >= 1"),
    (-3, {}, "integer number of days >= 1"),
    (True, {}, "integer number of days >= 1"),
    (1.5, {}, "integer number of days >= 1"),
    ("2", {}, "integer number of days >= 1"),
    (366, dict(profile_max_bytes=1000), "more than profile_max_bytes = 1000"),
])
def test_profile_refusals(profiles, kw, match):
    with pytest.raises(ValueError, match=match):
        _loop("nuclear", 2, profiles=profiles, **kw)


def test_day_points_refusals():
    """every refusal of DayPoints by its message, next to the construction that succeeds"""
    import torch
    from dispatches_amd import representative_days as rd
    with pytest.raises(ValueError, match="needs a loop that keeps profiles"):
        rd.DayPoints(_loop("nuclear", 2))
    loop = _loop("nuclear", 2, profiles=1)
    assert rd.DayPoints(loop).F == 24
    with pytest.raises(RuntimeError, match="no whole day has been run"):
        rd.DayPoints(loop).assign(np.zeros((1, 24)))
    for channels in (0, 3, "2"):
        with pytest.raises(ValueError, match="channels is 1 or 2"):
            rd.DayPoints(loop, channels=channels)
    with pytest.raises(ValueError, match="needs a capacity-factor series"):
        rd.DayPoints(loop, channels=2)
    with pytest.raises(ValueError, match="p_max must be greater than p_min"):
        rd.DayPoints(loop, p_min=[0.0, 400.0], p_max=[400.0, 400.0])
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="must be finite"):
            rd.DayPoints(loop, p_min=0.0, p_max=[400.0, bad])
    view = rd.Profiles(torch.zeros((2, 24, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="give p_min and p_max"):
        rd.DayPoints(view)
    points = rd.DayPoints(view, p_min=0.0, p_max=1.0)
    for centers in (np.zeros((1, 48)), np.zeros(24), np.zeros((65, 24)), np.zeros((0, 24))):
        with pytest.raises(ValueError, match=r"centres are \[K, 24\]"):
            points.assign(centers)
    with pytest.raises(ValueError, match="every day is a zero or a full day"):
        points.fit(2)
    with pytest.raises(ValueError, match="K is an integer in 1 .. 64"):
        points.fit(65)
    with pytest.raises(ValueError, match="init is 'k-means\\+\\+'"):
        points.fit(2, init="random")
    with pytest.raises(ValueError, match="contiguous float64 tensor"):
        rd.Profiles(torch.zeros((2, 23, 3), dtype=torch.float64))


def test_fit_and_sweep_on_the_cpu_backend(reference_centers):
    """nuclear_sweep with representative_days on the stand-in backend, one day of a 1 x 2 x 2 grid: a centre array only labels -
    dispatch_frequency is grid shape + (32,), every entry a share of the one day; a malformed argument is refused before anything runs"""
    from dispatches_amd import sweeps
    from tests._highs_solver import HighsTensorLP
    out = sweeps.nuclear_sweep([2.0], [100.0, 200.0], 2, 1, lp_backend=HighsTensorLP, representative_days=reference_centers["ne"])
    freq = out["dispatch_frequency"]
    assert freq.shape == (1, 2, 2, 32) and np.array_equal(out["day_centers"], reference_centers["ne"])
    assert set(np.unique(freq)) <= {0.0, 1.0} and np.array_equal(freq.sum(-1), np.ones((1, 2, 2)))
    plain = sweeps.nuclear_sweep([2.0], [100.0], 1, 1, lp_backend=HighsTensorLP)
    assert "dispatch_frequency" not in plain and "day_centers" not in plain
    with pytest.raises(ValueError, match="number of clusters K or centres"):
        sweeps.nuclear_sweep([2.0], [100.0], 1, 1, lp_backend=HighsTensorLP, representative_days=np.zeros((3, 7)))


def test_c_abi_declares_and_exports_the_entry_points():
    """the header declares the two structs and the five symbols, the library exports them, the ctypes mirrors match the header field for
    field, the limits are the header's, and DSP_VERSION is still 22: new symbols, no changed struct"""
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from dispatches_amd import hip_solver
    from dispatches_amd import representative_days as rd
    lib = hip_solver.load_library()
    hdr = open(os.path.join(ROOT, "include", "dsp_hip.h")).read()
    for name in ("dsp_loop_profile", "dsp_days_assign", "dsp_days_update", "dsp_days_frequency", "dsp_days_work_doubles"):
        assert re.search(r"\b(int|int64_t) %s\s*\(" % name, hdr) and hasattr(lib, name) and name in hip_solver.EXPORTED_SYMBOLS, name
    assert int(re.search(r"#define DSP_VERSION (\d+)", hdr).group(1)) == 22 == hip_solver.ABI_VERSION == lib.dsp_version()
    for struct, mirror, size in (("dsp_loop_profile_desc", hip_solver.DspLoopProfileDesc, 8 + 3 * 8 + 32),
                                 ("dsp_days_desc", hip_solver.DspDaysDesc, 16 + 5 * 8 + 8 + 32)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        body = re.sub(r"\[[0-9\]\[]*\]", "", body)                     # array extents
        fields = [f for decl in body.split(";") for f in re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", decl.strip().split(" ", 1)[-1] if decl.strip() else "")]
        fields = [f for f in fields if f not in ("const", "double", "int32_t", "int64_t")]
        assert fields == [f[0] for f in mirror._fields_], (struct, fields)
        assert C.sizeof(mirror) == size, struct
    define = lambda name: eval(re.search(r"#define %s (\(?[0-9 <]+\)?)" % name, hdr).group(1))      # noqa: S307 - digits, spaces and <<
    assert hip_solver.DAYS_MAX_K == define("DSP_DAYS_MAX_K") == rd.MAX_K and hip_solver.DAYS_CHUNK == define("DSP_DAYS_CHUNK") == rd.CHUNK
    assert hip_solver.DAYS_MAX_DAYS == define("DSP_DAYS_MAX_DAYS") and hip_solver.DAYS_MAX_PLANTS == define("DSP_DAYS_MAX_PLANTS")
    assert hip_solver.DAYS_MAX_POINTS == define("DSP_DAYS_MAX_POINTS")
    assert lib.dsp_days_work_doubles(1025, 3, 2) == 2 * (3 * 48 + 3 + 2) and lib.dsp_days_work_doubles(1025, 65, 2) == -1
    # the entry points refuse a NULL descriptor on the host, without a GPU
    assert lib.dsp_loop_profile(None, None) == -1 and lib.dsp_days_assign(None, None, 3, None, None, None) == -1
    assert lib.dsp_days_frequency(None, None, 3, None, None) == -1 and lib.dsp_days_update(None, None, None, 3, None, None, None, None, 0, None) == -1


def test_host_checks_run_clean_under_the_host_sanitizers(tmp_path):
    """the host-side checks of dsp_loop_profile and the three dsp_days entry points (csrc/dsp_days_check.hpp, the functions dsp_days.hip
    calls before it launches) compiled into the stand-alone program tools/days_check_main.cpp with AddressSanitizer and
    UndefinedBehaviorSanitizer on the host side: the sound descriptors accepted, every malformed one refused, no report.  A stand-alone
    program: nothing is preloaded into python."""
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "days_check")
    subprocess.run([hipcc if os.path.exists(hipcc) else "hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-g", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "days_check_main.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "0 failures" in run.stdout and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout, run.stderr)
