"""Seeded batches of GENERAL small LPs for the in-wave simplex kernels (csrc/dsp_simplex.hip), with their references.

Helper module of tests/test_simplex_spec_cpu.py (the numpy specification tools/simplex_proto.py, no GPU) and
tests/test_hip_simplex_general.py (the HIP kernels).  No tests in here.

    min c.x   s.t.  rlo <= A x <= rhi,  lb <= x <= ub          one dense A [m, n] per batch, c / lb / ub / rlo / rhi per scenario

Every LP is feasible and bounded BY CONSTRUCTION, no solver is asked: the bounds and row sides are laid around a point x0
(feasible), and c = A^T y0 + r0 with y0 of the sign its row's finite sides allow and r0 of the sign its column's finite bounds
allow, 0 on free columns (a dual feasible point, so the LP is bounded).  Two families:
  "generic"     A = integers in [-3, 3] x uniform(0.5, 2), x0 uniform in [0, 3], continuous slacks: the optimal vertex is almost
                surely unique and non-degenerate (so HiGHS's row duals can be compared entry by entry);
  "degenerate"  A, x0, slacks, y0 and r0 all small integers, a third of the slacks 0: x0 sits on many bounds, rows are active
                at x0, the ratio test ties all the time.
Columns (per scenario): 40 % lb = 0 with a finite ub >= x0, 10 % free, 10 % lb = -2, 5 % fixed at x0, 10 % with only an upper
bound (lb = -inf), the rest lb = 0, ub = inf.  Rows (one pattern per batch): 30 % equalities, 30 % >= with slack, 20 % <= with
slack, 20 % ranges.  Density about min(1, 6 / n + 0.15), no empty row.

References:
  highs_solve / highs_objective   HiGHS (the library scipy vendors, through oracle.highs_direct) per scenario;
  kkt_residuals                   solver-free optimality certificate of a pair (x, y) in np.longdouble - needs no unique solution, so it
                                  holds on the degenerate family too.

MEASURED FLOORS (tests/test_simplex_spec_cpu.py: the numpy specification with the kernel's tolerances tol_p = 1e-10, tol_d = 1e-12,
tol_piv = 1e-9 on every committed seed of SHAPES x FAMILIES and of the two grid-stride pools, raw data and Ruiz/Pock-Chambolle scaled
data, B = 32; worst over all of them, printed by that file's test_floors_are_the_recorded_ones):
    objective vs HiGHS, |obj - ref| / max(1, |ref|)   3.6e-12     -> GPU tolerance 3.6e-10
    kkt primal (bounds and rows)                      8.0e-14     -> 8.0e-12
    kkt dual_col (signs of c - A^T y)                 5.1e-14     -> 5.1e-12
    kkt dual_row (signs of y)                         1.1e-14     -> 1.1e-12
    kkt gap (primal - dual objective)                 4.1e-12     -> 4.1e-10
    duals vs HiGHS's row duals, |y - ref| / (1 + |ref|_inf), generic family, non-degenerate vertices only
                                                      5.2e-13     -> 5.2e-11
(all 1568 LPs optimal; most pivots 20 (n + m) is never reached: the worst mean is 398 of 2560 on 64 x 64 scaled)
GPU tolerances = min(100 x floor, 1e-9) (the factor covers FMA contraction and the handle's own scaling against the numpy run; 1e-9 is
the kernel's own certificate level): see TOL below, which is computed from FLOOR by exactly that rule.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LD = np.longdouble

# (n, m): m % 4 != 0, the register / LDS switch at m = 24 / 25, N = n + m = 64 / 65 / 128, m = 64 (every lane owns a row), n = 1, m = 1
SHAPES = [(1, 1), (3, 1), (5, 3), (7, 6), (40, 23), (40, 24), (39, 25), (32, 32), (33, 32), (63, 1), (1, 63), (64, 64), (100, 28), (70, 57)]
FAMILIES = ("generic", "degenerate")

# worst figures of the numpy specification over all committed seeds (see the docstring); the CPU tier asserts that they still hold
FLOOR = dict(objective=3.6e-12, primal=8.0e-14, dual_col=5.1e-14, dual_row=1.1e-14, gap=4.1e-12, duals=5.2e-13)
TOL = {k: min(100.0 * v, 1e-9) for k, v in FLOOR.items()}


# further batches: name -> make_batch arguments.  The grid-stride pools (a duplicated row, so that a test can make a scenario
# row-infeasible), the modes that stay bounded under NULL bound pointers, batch-wide bounds (broadcast vectors), a column that can
# be turned into an unbounded ray.  One register-kernel shape and one LDS-kernel shape with two columns per lane for each.
EXTRA = {
    "stride_32x32": dict(n=32, m=32, family="degenerate", dup_row=True),
    "stride_64x64": dict(n=64, m=64, family="generic", dup_row=True),
    "free_cols_20x12": dict(n=20, m=12, family="generic", mode="free_cols"),
    "free_cols_45x30": dict(n=45, m=30, family="degenerate", mode="free_cols"),
    "no_rlo_20x12": dict(n=20, m=12, family="degenerate", mode="no_rlo"),
    "no_rlo_45x30": dict(n=45, m=30, family="generic", mode="no_rlo"),
    "shared_20x12": dict(n=20, m=12, family="degenerate", shared_bounds=True),
    "shared_45x30": dict(n=45, m=30, family="generic", shared_bounds=True),
    "ray_40x24": dict(n=40, m=24, family="generic", ray_col=True),
}


WARM_SHAPES = [(40, 24), (39, 25), (70, 57)]


def warm_sequence(n, m, family, B):
    """[(A, D), (A, D perturbed by a few percent), (A, a rough change of that)]: three solves on one handle."""
    A, d0 = make_batch(n, m, family, B)
    d1 = perturbed(A, d0, seed_of(n, m, family, 101))
    d2 = rough_change(A, d1, seed_of(n, m, family, 102))
    return [(A, d0), (A, d1), (A, d2)]


def make_extra(name, B):
    kw = dict(EXTRA[name])
    n, m, family = kw.pop("n"), kw.pop("m"), kw.pop("family")
    return make_batch(n, m, family, B, seed=seed_of(n, m, family, 1 + sorted(EXTRA).index(name)), **kw)


def seed_of(n, m, family, extra=0):
    return 100003 * n + 1009 * m + 7 * FAMILIES.index(family) + 1000003 * extra


def make_batch(n, m, family, B, seed=None, mode="mixed", shared_bounds=False, dup_row=False, ray_col=False):
    """-> A [m, n], dict(c [B, n], lb, ub [B, n], rlo, rhi [B, m], x0, y0).

    mode "mixed"      the column / row mix of the module docstring
         "free_cols"  every column free (lb = -inf, ub = inf: what lb = ub = None means to the solver); r0 = 0, so c = A^T y0
         "no_rlo"     no row has a lower side (rlo = -inf: what rlo = None means); rows are <= rows, y0 <= 0
    shared_bounds     one x0 and one set of bounds and row sides for the whole batch (only the costs differ): every array but c has
                      identical rows, so the batch can be handed over as [n] / [m] vectors as well
    dup_row           the last row of A repeats the one before it (sides still laid around x0: healthy as generated; a test makes a
                      scenario infeasible by giving the two copies disjoint ranges)
    ray_col           column n - 1 has entries (positive) only in <= rows, at least one; as generated it is a bounded column
                      (lb = 0, finite ub); set free with a positive cost it runs to -inf without any row blocking it"""
    degenerate = family == "degenerate"
    rng = np.random.default_rng(seed_of(n, m, family) if seed is None else seed)
    dens = min(1.0, 6.0 / n + 0.15)
    A = np.where(rng.random((m, n)) < dens, rng.choice([-3, -2, -1, 1, 2, 3], (m, n)), 0).astype(float)
    for i in np.nonzero(~A.any(1))[0]:
        A[i, rng.integers(n)] = rng.choice([-3, -2, -1, 1, 2, 3])
    if not degenerate:
        A *= rng.uniform(0.5, 2.0, (m, n))
    # rows: 0 equality, 1 >=, 2 <=, 3 range (one pattern per batch)
    rtype = rng.choice(4, m, p=[0.3, 0.3, 0.2, 0.2])
    if mode == "no_rlo":
        rtype[:] = 2
    if dup_row:
        assert m >= 2
        A[m - 1] = A[m - 2]
    if ray_col:
        if not (rtype == 2).any():
            rtype[rng.integers(m)] = 2
        le = rtype == 2
        A[:, n - 1] = np.where(le, np.where(rng.random(m) < 0.6, np.abs(A[:, n - 1]) + 1.0, 0.0), 0.0)
        if not A[:, n - 1].any():
            A[np.nonzero(le)[0][0], n - 1] = 2.0
    Bg = 1 if shared_bounds else B
    x0 = rng.integers(0, 4, (Bg, n)).astype(float) if degenerate else rng.uniform(0.0, 3.0, (Bg, n))
    slack = (lambda shape: rng.integers(0, 3, shape).astype(float)) if degenerate else (lambda shape: rng.uniform(0.1, 2.0, shape))
    # columns: 0 lb = 0 and finite ub, 1 free, 2 lb = -2, 3 fixed, 4 only an upper bound, 5 lb = 0 only
    ctype = rng.choice(6, (Bg, n), p=[0.40, 0.10, 0.10, 0.05, 0.10, 0.25])
    if mode == "free_cols":
        ctype[:] = 1
    if ray_col:
        ctype[:, n - 1] = 0
    up = x0 + slack((Bg, n))
    lb = np.select([ctype == 0, ctype == 1, ctype == 2, ctype == 3, ctype == 4], [0.0, -np.inf, -2.0, x0, -np.inf], 0.0)
    ub = np.select([ctype == 0, ctype == 1, ctype == 2, ctype == 3, ctype == 4], [up, np.inf, np.inf, x0, up], np.inf)
    r = x0 @ A.T
    s1, s2 = slack((Bg, m)), slack((Bg, m))
    rlo = np.select([rtype == 0, rtype == 1, rtype == 2], [r, r - s1, -np.inf], r - s1)
    rhi = np.select([rtype == 0, rtype == 1, rtype == 2], [r, np.inf, r + s2], r + s2)
    if shared_bounds:
        x0, lb, ub, rlo, rhi, ctype = (np.repeat(a, B, 0) for a in (x0, lb, ub, rlo, rhi, ctype))
    # a dual feasible point: y0 >= 0 on >= rows, <= 0 on <= rows, any sign on equalities and ranges; r0 >= 0 where only lb is finite,
    # <= 0 where only ub is, any sign where both are, 0 on free columns
    y0 = rng.standard_normal((B, m)) * (rng.random((B, m)) < 0.7) * 2.0
    y0 = np.select([rtype == 1, rtype == 2], [np.abs(y0), -np.abs(y0)], y0)
    r0 = rng.standard_normal((B, n)) * (rng.random((B, n)) < 0.7) * 2.0
    r0 = np.select([ctype == 1, (ctype == 2) | (ctype == 5), ctype == 4], [0.0, np.abs(r0), -np.abs(r0)], r0)
    if degenerate:
        y0, r0 = np.round(y0), np.round(r0)
    c = y0 @ A + r0
    return A, dict(c=c, lb=lb, ub=ub, rlo=rlo, rhi=rhi, x0=x0, y0=y0, r0=r0, ctype=ctype, rtype=rtype, degenerate=degenerate)


def _rows_around(A, bt, x0, rng, s1, s2):
    r = x0 @ A.T
    rtype = bt["rtype"]
    rlo = np.select([rtype == 0, rtype == 1, rtype == 2], [r, r - s1, -np.inf], r - s1)
    rhi = np.select([rtype == 0, rtype == 1, rtype == 2], [r, np.inf, r + s2], r + s2)
    return rlo, rhi


def perturbed(A, bt, seed, rel=0.03):
    """The batch with costs, bounds and row sides moved by a few percent - still feasible and bounded by construction: the finite bounds
    keep x0 inside, x0 itself then moves a little within them and the row sides are laid around the new A x0 with slacks of
    (1 +- rel) x the old ones; y0 and r0 are scaled by (1 +- rel) entry by entry, which keeps their signs."""
    rng = np.random.default_rng(seed)
    u = lambda a: 1.0 + rel * rng.uniform(-1.0, 1.0, a.shape)
    x0, lb, ub = bt["x0"], bt["lb"], bt["ub"]
    fixed = lb == ub
    with np.errstate(invalid="ignore"):
        lb2 = np.where(fixed | ~np.isfinite(lb), lb, x0 - (x0 - lb) * u(x0))
        ub2 = np.where(fixed | ~np.isfinite(ub), ub, x0 + (ub - x0) * u(x0))
    x1 = np.clip(x0 + rel * rng.uniform(-1.0, 1.0, x0.shape) * (1.0 + np.abs(x0)), lb2, ub2)
    r = x0 @ A.T
    with np.errstate(invalid="ignore"):
        s1 = np.where(np.isfinite(bt["rlo"]), r - bt["rlo"], 0.0) * u(r)
        s2 = np.where(np.isfinite(bt["rhi"]), bt["rhi"] - r, 0.0) * u(r)
    rlo2, rhi2 = _rows_around(A, bt, x1, rng, s1, s2)
    y1, r1 = bt["y0"] * u(bt["y0"]), bt["r0"] * u(bt["r0"])
    return dict(bt, c=y1 @ A + r1, lb=lb2, ub=ub2, rlo=rlo2, rhi=rhi2, x0=x1, y0=y1, r0=r1)


def rough_change(A, bt, seed):
    """A change no hour-to-hour step of a rolling loop makes, still feasible and bounded by construction:
      * a quarter of the finite upper bounds become infinite (lb = 0 columns lose their ub, upper-bounded-only columns become free; r0
        is given the sign, or the 0, that the remaining bounds allow);
      * half of the fixed columns are released to [x0 - 1, x0 + 2], and a tenth of the lb = 0, ub = inf columns are fixed at x0;
      * x0 moves by up to 1.5 within the column bounds and every row's sides are laid anew around the new A x0, which leaves the old
        optimal basis primal infeasible on most scenarios."""
    rng = np.random.default_rng(seed)
    deg = bt["degenerate"]
    x0, lb, ub, r0, ctype = (bt[k].copy() for k in ("x0", "lb", "ub", "r0", "ctype"))
    pick = lambda t, share: (ctype == t) & (rng.random(ctype.shape) < share)
    drop0, drop4, release, fix = pick(0, 0.25), pick(4, 0.25), pick(3, 0.5), pick(5, 0.1)
    ub[drop0 | drop4] = np.inf
    r0[drop0] = np.abs(r0[drop0]); r0[drop4] = 0.0
    lb[release] = x0[release] - 1.0; ub[release] = x0[release] + 2.0
    lb[fix] = x0[fix]; ub[fix] = x0[fix]
    ctype[drop0] = 5; ctype[drop4] = 1; ctype[release] = 0; ctype[fix] = 3
    step = rng.integers(-1, 2, x0.shape).astype(float) if deg else rng.uniform(-1.5, 1.5, x0.shape)
    x1 = np.clip(x0 + step, lb, ub)
    slack = (lambda: rng.integers(0, 3, bt["rlo"].shape).astype(float)) if deg else (lambda: rng.uniform(0.1, 2.0, bt["rlo"].shape))
    rlo, rhi = _rows_around(A, bt, x1, rng, slack(), slack())
    return dict(bt, c=bt["y0"] @ A + r0, lb=lb, ub=ub, rlo=rlo, rhi=rhi, x0=x1, r0=r0, ctype=ctype)


def _full(a, B, w):
    """[B, w] float64 view of a per-scenario array, a broadcast vector or None (None = the infinite side `fill`)."""
    return np.broadcast_to(np.asarray(a, float), (B, w))


def expand(A, batch):
    """c, lb, ub, rlo, rhi as [B, .] arrays: None becomes the infinite bound it stands for, a vector is repeated."""
    m, n = A.shape
    c = np.atleast_2d(np.asarray(batch["c"], float))
    B = c.shape[0]
    get = lambda k, fill, w: _full(fill if batch.get(k) is None else batch[k], B, w)
    return c, get("lb", -np.inf, n), get("ub", np.inf, n), get("rlo", -np.inf, m), get("rhi", np.inf, m)


def highs_solve(A, c, lb, ub, rlo, rhi):
    """HiGHS per scenario -> obj [B], x [B, n], y [B, m] (HiGHS's row duals: the sign convention of kkt_residuals, checked on the
    CPU by tests/test_simplex_spec_cpu.py)."""
    from oracle.highs_direct import HighsModel
    B = c.shape[0]
    m, n = A.shape
    obj, X, Y = np.empty(B), np.empty((B, n)), np.empty((B, m))
    for k in range(B):
        X[k], obj[k], Y[k] = HighsModel(c[k], A, rlo[k], rhi[k], lb[k], ub[k]).solve()
    return obj, X, Y


def highs_objective(A, c, lb, ub, rlo, rhi):
    return highs_solve(A, c, lb, ub, rlo, rhi)[0]


def highs_verdict(A, c, lb, ub, rlo, rhi):
    """HiGHS's verdict on ONE LP without presolve (which would answer "unbounded or infeasible"): 0 optimal, 2 infeasible, 3 unbounded."""
    from oracle.highs_direct import HighsModel, _hc
    h = HighsModel(c, A, rlo, rhi, lb, ub).h
    h.setOptionValue("presolve", "off")
    h.run()
    S = _hc.HighsModelStatus
    return {S.kOptimal: 0, S.kInfeasible: 2, S.kUnbounded: 3}.get(h.getModelStatus(), -1)


def kkt_residuals(A, c, lb, ub, rlo, rhi, x, y):
    """Solver-free optimality certificate of (x, y) per scenario, in np.longdouble.  -> dict of [B] arrays:
      "primal"    largest violation of lb <= x <= ub and rlo <= A x <= rhi
      "dual_col"  largest violation of the sign conditions of r = c - A^T y: r_j < 0 needs a finite ub_j, r_j > 0 a finite lb_j
      "dual_row"  largest violation of the sign conditions of y: y_i > 0 needs a finite rlo_i, y_i < 0 a finite rhi_i
      "gap"       |primal objective - dual objective|, the dual objective y+.rlo - y-.rhi + r+.lb - r-.ub over the finite sides
    each relative to 1 + the largest magnitude among the numbers it compares (x, A x and the finite bounds; c and A^T y; y; the two
    objectives).  All four are 0 exactly at an optimal pair; a NaN anywhere gives inf."""
    A, c, x, y = (np.asarray(a, LD) for a in (A, c, x, y))
    lb, ub, rlo, rhi = (np.asarray(a, LD) for a in (lb, ub, rlo, rhi))
    fin = lambda a: np.where(np.isfinite(a), a, LD(0))
    pos = lambda a: np.maximum(a, LD(0))
    Ax = x @ A.T
    pv = np.maximum(np.max(np.maximum(pos(lb - x), pos(x - ub)), 1), np.max(np.maximum(pos(rlo - Ax), pos(Ax - rhi)), 1))
    pmag = np.max(np.abs(np.concatenate([x, Ax, fin(lb), fin(ub), fin(rlo), fin(rhi)], 1)), 1)
    ATy = y @ A
    r = c - ATy
    dc = np.max(np.maximum(np.where(np.isfinite(lb), 0, pos(r)), np.where(np.isfinite(ub), 0, pos(-r))), 1)
    dcmag = np.max(np.abs(np.concatenate([c, ATy], 1)), 1)
    dr = np.max(np.maximum(np.where(np.isfinite(rlo), 0, pos(y)), np.where(np.isfinite(rhi), 0, pos(-y))), 1)
    drmag = np.max(np.abs(y), 1)
    pobj = np.sum(c * x, 1)
    dobj = np.sum(pos(y) * fin(rlo) - pos(-y) * fin(rhi), 1) + np.sum(pos(r) * fin(lb) - pos(-r) * fin(ub), 1)
    out = dict(primal=pv / (1 + pmag), dual_col=dc / (1 + dcmag), dual_row=dr / (1 + drmag),
               gap=np.abs(pobj - dobj) / (1 + np.maximum(np.abs(pobj), np.abs(dobj))))
    return {k: np.where(np.isnan(v), np.inf, v).astype(float) for k, v in out.items()}


def nondegenerate(A, c, lb, ub, rlo, rhi, x, tol=1e-7):
    """[B] bool: exactly m of the n + m variables (x, A x) lie strictly inside their bounds at x (a free column at exactly 0 is a
    nonbasic one and does not count) - a non-degenerate basic solution, whose multipliers y are unique."""
    Ax = x @ A.T
    inside = ((x > lb + tol) & (x < ub - tol) & ~(np.isinf(lb) & np.isinf(ub) & (x == 0.0))).sum(1) + ((Ax > rlo + tol) & (Ax < rhi - tol)).sum(1)
    return inside == A.shape[0]


def dual_error(y, ref):
    return np.abs(y - ref).max(1) / (1.0 + np.abs(ref).max(1))


def objective_error(obj, ref):
    return np.abs(obj - ref) / np.maximum(1.0, np.abs(ref))


def handle_scaling(A):
    """The handle's equilibration of a dense A (csrc/dsp_prepare.hpp::equilibrate at the default options: 10 Ruiz passes, then Pock-Chambolle
    with alpha = 1; an empty row or column keeps scale 1) -> scaled A, dr [m], dc [n].  tools/pdlp_proto.py::ruiz_pc_scaling is the same
    wherever no column is empty."""
    As, dr, dc = np.abs(A).astype(float), np.ones(A.shape[0]), np.ones(A.shape[1])
    inv = lambda v: np.where(v > 0, 1.0 / np.sqrt(np.where(v > 0, v, 1.0)), 1.0)
    for it in range(11):
        rs, cs = (inv(As.max(1)), inv(As.max(0))) if it < 10 else (inv(As.sum(1)), inv(As.sum(0)))
        As = As * rs[:, None] * cs[None, :]
        dr, dc = dr * rs, dc * cs
    return A * dr[:, None] * dc[None, :], dr, dc


def spec_module():
    """tools/simplex_proto.py, the executable specification of the kernels."""
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import simplex_proto
    return simplex_proto


def spec_solve(A, c, lb, ub, rlo, rhi, scaled):
    """The numpy specification (tools/simplex_proto.py) with the kernel's tolerances, on the raw data or on data scaled the way the
    handle scales it (as tools/simplex_proto.py::solve_model does).  -> x, y, obj, status, pivots in the original space."""
    sx = spec_module()
    kw = dict(tol_p=1e-10, tol_d=1e-12, tol_piv=1e-9)
    if scaled:
        As, dr, dc = handle_scaling(A)
        x, y, st, piv = sx.simplex_batch(As, c * dc, lb / dc, ub / dc, rlo * dr, rhi * dr, **kw)
        x, y = x * dc, y * dr
    else:
        x, y, st, piv = sx.simplex_batch(A, c, lb, ub, rlo, rhi, **kw)
    return x, y, np.sum(c * x, 1), st, piv


def make_handle(A, **options):
    """DeviceLP of the dense matrix: CSR, c = zeros, no col_scale, no row_compliance."""
    import scipy.sparse as sp
    from dispatches_amd.hip_solver import DeviceLP, default_options
    from dispatches_amd.lp import StandardFormLP
    m, n = A.shape
    S = sp.csr_matrix(A)
    S.sort_indices()
    lp = StandardFormLP(n=n, m=m, indptr=S.indptr.astype(np.int32), indices=S.indices.astype(np.int32), data=S.data.astype(np.float64),
                        c=np.zeros(n), c0=0.0, lb=np.full(n, -np.inf), ub=np.full(n, np.inf), rlo=np.full(m, -np.inf), rhi=np.full(m, np.inf))
    return DeviceLP(lp, 0, default_options(**options))


def device_solve(A, batch, handle=None, **options):
    """Upload, solve on the GPU, download.  batch: dict with c [B, n] and lb / ub [B, n] or [n] or None, rlo / rhi [B, m] or [m] or
    None (None = a NULL pointer: no bound on that side).  handle: a make_handle() result to solve on again (warm starts); the options
    then apply to this call.  -> numpy x, y, obj, status, iters and the call's dsp_stats."""
    import torch
    from dispatches_amd.hip_solver import default_options
    dlp = make_handle(A, **options) if handle is None else handle
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float64)).cuda()
    c = np.atleast_2d(np.asarray(batch["c"], float))
    out = dlp.solve(c.shape[0], up(c), up(batch.get("lb")), up(batch.get("ub")), up(batch.get("rlo")), up(batch.get("rhi")),
                    options=None if handle is None else default_options(**options))
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy().copy() for k in ("x", "y", "obj", "status", "iters")}
    res["stats"] = out["stats"]
    return res
