"""CPU tests of the in-wave simplex' KKT certificate (dsp_options::simplex_certify, csrc/dsp_simplex.hip) through its numpy specification,
tools/simplex_proto.py::kkt_certificate and simplex_batch(certify=True), and of the option / structure plumbing that needs no GPU.

The certificate is four numbers per scenario - primal, dual_col, dual_row, gap - with the definitions of
tests/_small_lp_cases.py::kkt_residuals (long double).  Agreement bound 1.4e-13 absolute: at most 128 terms x 2^-53 x 10 on quantities
that are already relative to 1 + magnitude.  The dsp_solve refusals (they need a handle, hence a device) are in
tests/test_hip_simplex_certificate.py.

MEASURED (this file, every SHAPES x FAMILIES batch of 48): kkt_certificate vs kkt_residuals 4.4e-14 worst (bound 1.4e-13), the four numbers
at the specification's optima primal 3.3e-14, dual_col 6.0e-14, dual_row 1.4e-14, gap 3.1e-12 (slc.TOL 8.0e-12, 5.1e-12, 1.1e-12, 4.1e-10);
the rejected points: max of the named components at least 1.5e-4 (non-optimal vertex), 6.7e-4 (negated multiplier), 0.59 (y = 0).
"""
import functools
import os
import re

import numpy as np
import pytest

from tests import _small_lp_cases as slc

B = 48
AGREE = 1.4e-13
KEYS = ("primal", "dual_col", "dual_row", "gap")
KW = dict(tol_p=1e-10, tol_d=1e-12, tol_piv=1e-9)         # the kernels' tolerances (slc.spec_solve)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, m, fam) for n, m in slc.SHAPES for fam in slc.FAMILIES]


@functools.lru_cache(maxsize=None)
def _optimum(n, m, fam):
    """(A, data, x, y, status, pivots) of the specification's plain solve of a batch: computed once, never modified."""
    A, bt = slc.make_batch(n, m, fam, B)
    data = slc.expand(A, bt)
    x, y, st, piv = slc.spec_module().simplex_batch(A, *data, **KW)
    for a in data + (x, y, st, piv):
        a.flags.writeable = False
    return A, data, x, y, st, piv


def _long_double(A, data, x, y):
    r = slc.kkt_residuals(A, *data, x, y)
    return np.stack([r[k] for k in KEYS], 1)


@pytest.mark.parametrize("n,m,fam", CASES)
def test_certificate_equals_the_long_double_one_at_every_optimum(n, m, fam):
    A, data, x, y, st, piv = _optimum(n, m, fam)
    assert (st == 0).all()
    kkt = slc.spec_module().kkt_certificate(A, *data, x, y)
    ref = _long_double(A, data, x, y)
    assert kkt.shape == (B, 4)
    print(f"\n[certificate] {n}x{m} {fam}: vs long double {np.abs(kkt - ref).max():.1e}  worst " + "  ".join(f"{k} {kkt[:, e].max():.1e}" for e, k in enumerate(KEYS)))
    assert np.abs(kkt - ref).max() <= AGREE, (np.abs(kkt - ref).max(), np.unravel_index(np.abs(kkt - ref).argmax(), kkt.shape))
    for e, k in enumerate(KEYS):
        assert kkt[:, e].max() <= slc.TOL[k], (k, kkt[:, e].max(), int(kkt[:, e].argmax()))


# ---- points today's check (bounds and rows of x) accepts and the certificate rejects --------------------------------------------------
REJECT_SHAPES = [(40, 24), (39, 25), (70, 57)]


def _judge(A, data, x, y, named):
    """-> max of the named components per scenario; primal stays at the optimum's level"""
    kkt = slc.spec_module().kkt_certificate(A, *data, x, y)
    assert np.abs(kkt - _long_double(A, data, x, y)).max() <= AGREE
    assert kkt[:, 0].max() <= slc.TOL["primal"], kkt[:, 0].max()
    return kkt[:, [KEYS.index(k) for k in named]].max(1)


@pytest.mark.parametrize("n,m", REJECT_SHAPES)
def test_a_feasible_vertex_that_is_not_optimal_is_rejected(n, m):
    """The optimum of the LP with ONE nonbasic column's cost changed (a column with two finite bounds that sits at its lower bound with a
    positive reduced cost gets a cost that makes it attractive), judged under the ORIGINAL cost: a feasible vertex, its rows and bounds
    are fine, it is not optimal - what a drifted tableau can stop at."""
    A, data, x, y, st, piv = _optimum(n, m, "generic")
    c, lb, ub, rlo, rhi = data
    r = c - y @ A
    cand = np.isfinite(lb) & np.isfinite(ub) & (ub > lb + 0.1) & (x <= lb + 1e-12) & (r > 1e-3)
    assert cand.any(1).sum() >= B // 2
    j = cand.argmax(1)
    rows = np.nonzero(cand.any(1))[0]
    c2 = c.copy()
    c2[rows, j[rows]] -= 2.0 * r[rows, j[rows]] + 1.0
    x2, y2, st2, _ = slc.spec_module().simplex_batch(A, c2, lb, ub, rlo, rhi, **KW)
    assert (st2 == 0).all()
    worse = np.zeros(B, bool)
    worse[rows] = ((c * x2).sum(1) - (c * x).sum(1))[rows] > 1e-6 * (1.0 + np.abs((c * x).sum(1)))[rows]      # (else it is still an optimum)
    assert worse.sum() >= B // 4, int(worse.sum())
    comp = _judge(A, data, x2, y2, ("dual_col", "gap"))
    print(f"\n[certificate] {n}x{m} non-optimal vertices: {int(worse.sum())}, smallest max(dual_col, gap) {comp[worse].min():.1e}")
    assert (comp[worse] > 1e-9).all(), comp[worse].min()


@pytest.mark.parametrize("n,m", REJECT_SHAPES)
def test_a_multiplier_of_the_wrong_sign_is_rejected(n, m):
    """The optimum with one ACTIVE row's y_i negated."""
    A, data, x, y, st, piv = _optimum(n, m, "generic")
    active = np.abs(y) > 1e-3
    assert active.any(1).all()
    i = active.argmax(1)
    y2 = y.copy()
    y2[np.arange(B), i] *= -1.0
    comp = _judge(A, data, x, y2, ("dual_row", "gap"))
    print(f"\n[certificate] {n}x{m} negated multiplier: smallest max(dual_row, gap) {comp.min():.1e}")
    assert (comp > 1e-9).all(), comp.min()


@pytest.mark.parametrize("n,m", REJECT_SHAPES)
def test_zero_multipliers_are_rejected(n, m):
    """The optimum with y = 0 (the y of a tableau that prices nothing)."""
    A, data, x, y, st, piv = _optimum(n, m, "generic")
    comp = _judge(A, data, x, np.zeros_like(y), ("dual_col", "gap"))
    print(f"\n[certificate] {n}x{m} y = 0: smallest max(dual_col, gap) {comp.min():.1e}")
    assert (comp > 1e-9).all(), comp.min()


# ---- simplex_batch(certify=True) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,fam", CASES)
def test_certify_changes_no_solution_and_rejects_by_its_tolerance(n, m, fam):
    A, data, x, y, st, piv = _optimum(n, m, fam)
    sx = slc.spec_module()
    x1, y1, st1, piv1, kkt = sx.simplex_batch(A, *data, certify=True, **KW)
    assert np.array_equal(x1, x) and np.array_equal(y1, y) and np.array_equal(piv1, piv) and np.array_equal(st1, st)
    assert np.array_equal(kkt, sx.kkt_certificate(A, *data, x, y))
    x2, y2, st2, piv2, kkt2 = sx.simplex_batch(A, *data, certify=True, kkt_tol=1e-300, **KW)
    assert np.array_equal(x2, x) and np.array_equal(y2, y) and np.array_equal(piv2, piv) and np.array_equal(kkt2, kkt)
    assert np.array_equal(st2 == 4, kkt.max(1) > 0.0) and np.array_equal(st2 == 0, kkt.max(1) == 0.0)


def test_no_vertex_no_certificate():
    """pivot limit: status 1, four NaNs"""
    A, data, x, y, st, piv = _optimum(40, 24, "generic")
    out = slc.spec_module().simplex_batch(A, *data, certify=True, max_pivots=3, **KW)
    assert (out[2] == 1).all() and np.isnan(out[4]).all()


# ---- options and structures -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dispatches_amd import hip_solver
    return hip_solver.load_library()


def test_options_flag_and_structures(lib):
    import ctypes as C
    from dispatches_amd import hip_solver
    o = hip_solver.default_options()
    assert o.simplex_certify == 0 and o.simplex_kkt_tol == 0.0
    hdr = open(os.path.join(ROOT, "include", "dsp_hip.h")).read()
    assert int(re.search(r"#define DSP_FLAG_SIMPLEX_KKT\s+(\d+)", hdr).group(1)) == 8 == hip_solver.FLAG_SIMPLEX_KKT
    assert int(re.search(r"#define DSP_VERSION (\d+)", hdr).group(1)) == 22 == hip_solver.ABI_VERSION == lib.dsp_version()
    assert hip_solver.DspBatch._fields_[-1] == ("kkt", C.c_void_p)
    assert hip_solver.DspStats._fields_[-1] == ("simplex_unsolved", C.c_int32)
    assert [f[0] for f in hip_solver.DspOptions._fields_[-2:]] == ["simplex_certify", "simplex_kkt_tol"]
    assert hip_solver.default_options(simplex_certify=1, simplex_kkt_tol=1e-8).simplex_kkt_tol == 1e-8
