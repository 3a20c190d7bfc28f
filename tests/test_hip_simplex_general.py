"""GPU tests of the in-wave simplex kernels (csrc/dsp_simplex.hip) on GENERAL small LPs: free columns, upper-bounded-only columns,
negative lower bounds, ranges and one-sided rows of either side, NULL bound pointers, every shape edge of the three kernels
(simplex_reg_kernel<1, 24>, simplex_kernel<1>, simplex_kernel<2>), the grid-stride loop with failing neighbours, unbounded LPs and
warm starts from bases that no longer fit.

Generator, references and tolerances: tests/_small_lp_cases.py (every LP feasible and bounded by construction; HiGHS objectives and a
solver-free KKT certificate in long double; tolerances = min(100 x the floor of the numpy specification, 1e-9), measured by
tests/test_simplex_spec_cpu.py).  The share of scenarios that may come back non-optimal is ZERO: the specification solves all of them.

Masking: the feasible families are solved with max_iter = 64, so the PDLP pass that follows the simplex cannot rescue a scenario the
simplex handed over (as tests/test_hip_batch_parity.py::test_simplex_certificate_regression does), and the objective tolerance is one no
first-order solve of 64 iterations meets.

MEASURED on an MI355X (worst over all cases of this file; tolerance in brackets):
    objective vs HiGHS 2.6e-12 (3.6e-10)   kkt primal 1.4e-15 (8.0e-12)   dual_col 4.6e-14 (5.1e-12)   dual_row 4.2e-14 (1.1e-12)
    gap 6.5e-12 (4.1e-10)   duals vs HiGHS's row duals 3.8e-12 (5.2e-11)
No scenario was handed over or came back non-optimal in any kernel.  Mean pivots per shape (generic / degenerate family, cold):
    1x1 1.0 / 0.7   3x1 1.4 / 0.8   5x3 3.1 / 3.8   7x6 6.8 / 9.2   40x23 85.8 / 80.0   40x24 74.4 / 70.5   39x25 90.2 / 76.3
    32x32 102.9 / 80.5   33x32 101.6 / 97.9   63x1 1.1 / 1.7   1x63 24.1 / 3.4   64x64 400.4 / 348.7   100x28 147.3 / 132.4
    70x57 327.1 / 340.9 (register and LDS kernel give the same counts); warm starts: after a few percent 1.0 - 7.3, after the rough
    change about 55 % of the cold count.
"""
import functools

import numpy as np
import pytest

from tests import _small_lp_cases as slc

gpu = pytest.mark.gpu
B = 48
NUMERICAL = 4            # DSP_STATUS_NUMERICAL of include/dsp_hip.h


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")


def _in_register_kernel(n, m, batch=B):
    """launch_simplex: the register-tableau kernel takes m <= 24, n + m <= 64, B <= 2048 without a warm start."""
    return m <= 24 and n + m <= 64 and batch <= 2048


@functools.lru_cache(maxsize=None)
def _reference(key, batch=B):
    """(A, batch dict, [B, .] data, HiGHS obj, x, y) of a case, computed once and never modified."""
    if key in slc.EXTRA:
        A, bt = slc.make_extra(key, batch)
    else:
        n, m, fam = key
        A, bt = slc.make_batch(n, m, fam, batch)
    data = slc.expand(A, bt)
    for a in data:
        a.flags.writeable = False
    return (A, bt, data) + slc.highs_solve(A, *data)


def _check(label, A, data, res, ref_obj, keep=None):
    """Every scenario (of `keep`) optimal and equal to its references at the tolerances of the helper.  -> the figures."""
    keep = np.ones(len(ref_obj), bool) if keep is None else keep
    st, it = res["status"], res["iters"]
    bad = np.nonzero(keep & (st != 0))[0]
    assert bad.size == 0, (f"{label} A {A.shape[1]} x {A.shape[0]}: {bad.size} of {int(keep.sum())} scenarios not optimal: "
                           f"scenario / status / iters {[(int(k), int(st[k]), int(it[k])) for k in bad[:12]]}")
    sel = lambda a: a[keep]
    fig = dict(objective=slc.objective_error(sel(res["obj"]), sel(ref_obj)),
               **slc.kkt_residuals(A, *(sel(a) for a in data), sel(res["x"]), sel(res["y"])))
    worst = {k: float(v.max()) for k, v in fig.items()}
    print(f"\n[simplex] {label}: pivots mean {sel(it).mean():.1f} max {int(sel(it).max())}  " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in fig.items():
        w = int(np.argmax(v))
        assert v[w] <= slc.TOL[k], (f"{label} A {A.shape[1]} x {A.shape[0]}: {k} {v[w]:.3e} > {slc.TOL[k]:.1e} at kept scenario {w} "
                                     f"(iters {int(sel(it)[w])}, obj {sel(res['obj'])[w]!r} vs {sel(ref_obj)[w]!r})")
    return worst


@functools.lru_cache(maxsize=None)
def _cold(n, m, fam):
    """The cold solve of a shape as the handle routes it, PDLP capped at 64 iterations."""
    A, bt, data, ref_obj, ref_x, ref_y = _reference((n, m, fam))
    return slc.device_solve(A, bt, max_iter=64)


# ---- shapes x kernels ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fam", slc.FAMILIES)
@pytest.mark.parametrize("n,m", slc.SHAPES)
def test_every_shape_in_every_kernel_that_takes_it(n, m, fam):
    """48 LPs of every shape edge (m % 4 != 0, m = 24 / 25, n + m = 64 / 65 / 128, m = 64, n = 1, m = 1) against HiGHS and the KKT
    certificate.  A shape the register kernel takes runs a second time in the LDS kernel (simplex_warm = 1 on a fresh handle: every warm
    call goes there and the first one starts cold): both agree with the references and with each other."""
    _need_gpu()
    A, bt, data, ref_obj, ref_x, ref_y = _reference((n, m, fam))
    res = _cold(n, m, fam)
    assert res["stats"].simplex == 1
    kernel = "reg" if _in_register_kernel(n, m) else f"lds<{(n + m + 63) // 64}>"
    _check(f"{n}x{m} {fam} {kernel} seed {slc.seed_of(n, m, fam)}", A, data, res, ref_obj)
    if _in_register_kernel(n, m):
        lds = slc.device_solve(A, bt, max_iter=64, simplex_warm=1)
        assert lds["stats"].simplex == 1
        _check(f"{n}x{m} {fam} lds<1> (cold, warm mode) seed {slc.seed_of(n, m, fam)}", A, data, lds, ref_obj)
        both = slc.objective_error(lds["obj"], res["obj"])
        assert both.max() <= slc.TOL["objective"], (n, m, fam, both.max(), int(both.argmax()))


@gpu
@pytest.mark.parametrize("n,m", [s for s in slc.SHAPES if s != (1, 63)])      # (one column, ~19 equalities through x0: always degenerate)
def test_duals_equal_highs_where_they_are_unique(n, m):
    """Generic family: where HiGHS's vertex is non-degenerate the multipliers are unique, and the kernel's y equals HiGHS's row duals entry
    by entry (sign convention of HiGHS checked on the CPU: tests/test_simplex_spec_cpu.py)."""
    _need_gpu()
    A, bt, data, ref_obj, ref_x, ref_y = _reference((n, m, "generic"))
    res = _cold(n, m, "generic")
    unique = slc.nondegenerate(A, *data, ref_x) & (res["status"] == 0)
    assert unique.sum() >= B // 2, (n, m, int(unique.sum()))
    err = np.where(unique, slc.dual_error(res["y"], ref_y), 0.0)
    print(f"\n[simplex] {n}x{m} duals vs HiGHS on {int(unique.sum())} non-degenerate scenarios: {err.max():.1e}")
    assert err.max() <= slc.TOL["duals"], (n, m, err.max(), int(err.argmax()))


# ---- the gate -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", [(65, 64), (10, 65)])
def test_shapes_next_to_the_limit_go_to_pdlp(n, m):
    """n + m = 129 and m = 65 are beyond what the kernels hold: no simplex pass, and PDLP still solves them at default options to the
    project's 1e-6 on the objective."""
    _need_gpu()
    A, bt = slc.make_batch(n, m, "generic", 8)
    data = slc.expand(A, bt)
    res = slc.device_solve(A, bt)
    assert res["stats"].simplex == 0
    assert (res["status"] == 0).all(), (res["status"], res["iters"])
    err = slc.objective_error(res["obj"], slc.highs_objective(A, *data))
    print(f"\n[simplex] gate {n}x{m}: PDLP iterations max {int(res['iters'].max())}, objective error {err.max():.1e}")
    assert err.max() <= 1e-6, err


# ---- NULL bound pointers, broadcast bounds ---------------------------------------------------------------------------------------------
def _same_bits(a, b, what):
    for k in ("x", "y", "obj", "status", "iters"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, np.nonzero(np.asarray(a[k] != b[k]).reshape(len(a[k]), -1).any(1))[0][:8])


@gpu
@pytest.mark.parametrize("name", ["free_cols_20x12", "free_cols_45x30", "no_rlo_20x12", "no_rlo_45x30"])
def test_null_bound_pointers_mean_no_bound(name):
    """lb = ub = None (every column free) and rlo = None (no row has a lower side): the NULL pointers give the results of explicit
    arrays of infinities, bit for bit, and those are the optima."""
    _need_gpu()
    A, bt, data, ref_obj, ref_x, ref_y = _reference(name)
    explicit = slc.device_solve(A, bt, max_iter=64)
    assert explicit["stats"].simplex == 1
    _check(f"{name} explicit infinities", A, data, explicit, ref_obj)
    if name.startswith("free_cols"):
        assert np.isinf(bt["lb"]).all() and np.isinf(bt["ub"]).all()
        null = dict(bt, lb=None, ub=None)
    else:
        assert np.isinf(bt["rlo"]).all()
        null = dict(bt, rlo=None)
    res = slc.device_solve(A, null, max_iter=64)
    _check(f"{name} NULL pointers", A, data, res, ref_obj)
    _same_bits(res, explicit, name)


@gpu
@pytest.mark.parametrize("name", ["shared_20x12", "shared_45x30"])
def test_broadcast_bounds_equal_per_scenario_copies(name):
    """[n] / [m] bound vectors (scenario stride 0) against [B, n] / [B, m] copies of the same numbers: the same arithmetic read through
    another stride, bit for bit."""
    _need_gpu()
    A, bt, data, ref_obj, ref_x, ref_y = _reference(name)
    full = slc.device_solve(A, bt, max_iter=64)
    assert full["stats"].simplex == 1
    _check(f"{name} per-scenario bounds", A, data, full, ref_obj)
    for k in ("lb", "ub", "rlo", "rhi"):
        assert (bt[k] == bt[k][0]).all()
    res = slc.device_solve(A, dict(bt, **{k: bt[k][0].copy() for k in ("lb", "ub", "rlo", "rhi")}), max_iter=64)
    _same_bits(res, full, name)


# ---- grid stride with failing neighbours ----------------------------------------------------------------------------------------------
def _simplex_grid_bound(n, m):
    """Upper bound of the simplex launch's grid (dsp_solve: min(B, CUs x min(32, LDS per CU / LDS per block))) with the largest LDS of
    any CDNA part, 160 KiB per CU: a device with less launches fewer blocks and strides more."""
    import torch
    N = n + m
    lds = (m * (N | 1) + 2 * ((m + 1) & ~1) + ((N + 1) & ~1) + 16) * 8
    return torch.cuda.get_device_properties(0).multi_processor_count * max(1, min(32, (160 * 1024) // lds))


@gpu
@pytest.mark.parametrize("name,batch", [("stride_32x32", 2600), ("stride_64x64", 700)])
def test_grid_stride_with_failing_neighbours(name, batch):
    """More scenarios than blocks: every wave takes further scenarios on the same LDS after its earlier ones ended - some of them through
    the early exits (NaN cost, crossed bounds, row-infeasible).  200 distinct LPs tiled in a seeded permutation, 2 % broken in seeded
    places of the first and the later rounds.  Broken ones get their verdict, EVERY healthy one equals its reference, and copies of one LP
    agree bit for bit wherever they ran.  Default max_iter here, so that a row-infeasible LP the simplex passes on still ends in PDLP's
    certificate (the healthy ones are held to a tolerance PDLP does not reach, and to simplex-sized iteration counts)."""
    _need_gpu()
    pool = 200
    A, bt, data, ref_obj, ref_x, ref_y = _reference(name, pool)
    m, n = A.shape
    grid = _simplex_grid_bound(n, m)
    assert batch > grid, (batch, grid)
    rng = np.random.default_rng(slc.seed_of(n, m, "generic", 77))
    idx = rng.permutation(np.resize(np.arange(pool), batch))
    c, lb, ub, rlo, rhi = (a[idx].copy() for a in data)
    n_bad = batch // 50
    first = rng.choice(min(grid, batch) // 2, n_bad // 2, replace=False)                      # first round of every device
    later = grid + rng.choice(batch - grid, n_bad - n_bad // 2, replace=False)                # a later round of every device
    broken = np.concatenate([first, later])
    kind = np.arange(broken.size) % 3
    nan_cost, crossed, row_inf = broken[kind == 0], broken[kind == 1], broken[kind == 2]
    c[nan_cost, rng.integers(0, n, nan_cost.size)] = np.nan
    j = rng.integers(0, n, crossed.size)
    lb[crossed, j], ub[crossed, j] = 1.0, -1.0
    r = bt["x0"][idx[row_inf]] @ A[m - 1]
    assert np.array_equal(A[m - 1], A[m - 2])
    rlo[row_inf, m - 2], rhi[row_inf, m - 2] = r + 1.0, r + 2.0                               # two copies of one row, disjoint ranges
    rlo[row_inf, m - 1], rhi[row_inf, m - 1] = r - 2.0, r - 1.0
    res = slc.device_solve(A, dict(c=c, lb=lb, ub=ub, rlo=rlo, rhi=rhi))
    assert res["stats"].simplex == 1
    st = res["status"]
    assert (st[nan_cost] == NUMERICAL).all() and (st[crossed] == 2).all(), (st[nan_cost], st[crossed])
    for k in np.concatenate([nan_cost, crossed]):
        assert np.isnan(res["x"][k]).all() and np.isnan(res["y"][k]).all() and np.isnan(res["obj"][k]), k
    assert (st[row_inf] == 2).all(), (st[row_inf], res["iters"][row_inf])
    for k in row_inf[:2]:
        assert slc.highs_verdict(A, c[k], lb[k], ub[k], rlo[k], rhi[k]) == 2
    healthy = np.ones(batch, bool)
    healthy[broken] = False
    assert (res["iters"][healthy] <= 20 * (n + m)).all(), res["iters"][healthy].max()
    _check(f"{name} B {batch} (grid <= {grid})", A, (c, lb, ub, rlo, rhi), res, ref_obj[idx], keep=healthy)
    # copies of one distinct LP: identical bits, whichever block and round solved them
    first_copy = np.full(pool, -1)
    for k in np.nonzero(healthy)[0][::-1]:
        first_copy[idx[k]] = k
    twin = first_copy[idx]
    for key in ("x", "y", "obj", "iters"):
        differ = healthy & (np.asarray(res[key] != res[key][twin]).reshape(batch, -1).any(1))
        assert not differ.any(), (key, np.nonzero(differ)[0][:8], twin[differ][:8])


# ---- unbounded ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_unbounded_lps_are_reported_dual_infeasible():
    """40 x 24 LPs with one column whose entries (positive, in <= rows only) never block its way down: made free and given a positive cost
    it is an unbounded ray.  The simplex meets the empty ratio test and passes the scenario on; default options, so PDLP's certificate
    ends it: status 3, confirmed by HiGHS; the neighbours are the optima they were."""
    _need_gpu()
    A, bt, data, ref_obj, ref_x, ref_y = _reference("ray_40x24", 16)
    m, n = A.shape
    c, lb, ub, rlo, rhi = (a.copy() for a in data)
    bad = np.array([2, 7, 8, 13])
    lb[bad, n - 1], ub[bad, n - 1], c[bad, n - 1] = -np.inf, np.inf, 1.5
    res = slc.device_solve(A, dict(c=c, lb=lb, ub=ub, rlo=rlo, rhi=rhi))
    assert res["stats"].simplex == 1
    assert (res["status"][bad] == 3).all(), (res["status"], res["iters"])
    for k in bad[:2]:
        assert slc.highs_verdict(A, c[k], lb[k], ub[k], rlo[k], rhi[k]) == 3
    keep = np.ones(16, bool)
    keep[bad] = False
    assert (res["iters"][keep] <= 20 * (n + m)).all()
    _check("ray_40x24 neighbours of unbounded LPs", A, (c, lb, ub, rlo, rhi), res, ref_obj, keep=keep)


# ---- warm starts ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fam", slc.FAMILIES)
@pytest.mark.parametrize("n,m", slc.WARM_SHAPES)
def test_warm_starts_from_bases_that_no_longer_fit(n, m, fam):
    """simplex_warm = 1, three solves on one handle: data D; D with costs, bounds and row sides moved by a few percent; a rough change
    (finite bounds become infinite, fixed columns are released and others fixed, row sides move far: the saved basis is primal infeasible
    and some of its nonbasic sides no longer exist).  Every solve is held to its own references; the second needs fewer pivots than the
    first on average, which is what the warm start is for."""
    _need_gpu()
    seq = slc.warm_sequence(n, m, fam, B)
    handle = slc.make_handle(seq[0][0], max_iter=64, simplex_warm=1)
    pivots = []
    for step, (A, bt) in enumerate(seq):
        data = slc.expand(A, bt)
        res = slc.device_solve(A, bt, handle=handle, max_iter=64, simplex_warm=1)
        assert res["stats"].simplex == 1
        _check(f"warm {n}x{m} {fam} solve {step}", A, data, res, slc.highs_objective(A, *data))
        pivots.append(float(res["iters"].mean()))
    print(f"\n[simplex] warm {n}x{m} {fam}: mean pivots cold {pivots[0]:.1f}, after a few percent {pivots[1]:.1f}, after the rough change {pivots[2]:.1f}")
    assert pivots[1] < pivots[0], pivots
