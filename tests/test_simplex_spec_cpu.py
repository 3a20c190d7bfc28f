"""CPU tier of the general small-LP tests: the numpy specification of the in-wave simplex (tools/simplex_proto.py) with the kernel's
tolerances, on the generator of tests/_small_lp_cases.py, raw and scaled the way the handle scales.

It proves the generator (every LP feasible and bounded: HiGHS and the specification both end optimal), pins the specification's rules
for free columns and upper-bounded-only columns, and measures the floors from which tests/test_hip_simplex_general.py takes its
tolerances (recorded in tests/_small_lp_cases.py::FLOOR)."""
import functools

import numpy as np
import pytest

from tests import _small_lp_cases as slc

B = 32
WARM = [f"warm{step}-{n}x{m}-{fam}" for (n, m) in slc.WARM_SHAPES for fam in slc.FAMILIES for step in (1, 2)]
CASES = [f"{n}x{m}-{fam}" for (n, m) in slc.SHAPES for fam in slc.FAMILIES] + sorted(slc.EXTRA) + WARM


@functools.lru_cache(maxsize=None)
def _case(name):
    """Batch, HiGHS reference and both runs of the specification for one case, computed once."""
    if name in slc.EXTRA:
        A, bt = slc.make_extra(name, B)
    elif name.startswith("warm"):
        step, shape, fam = name.split("-")
        n, m = map(int, shape.split("x"))
        A, bt = slc.warm_sequence(n, m, fam, B)[int(step[4:])]
    else:
        shape, fam = name.split("-")
        n, m = map(int, shape.split("x"))
        A, bt = slc.make_batch(n, m, fam, B)
    data = slc.expand(A, bt)
    ref_obj, ref_x, ref_y = slc.highs_solve(A, *data)
    runs = {scaled: slc.spec_solve(A, *data, scaled=scaled) for scaled in (False, True)}
    return A, bt, data, (ref_obj, ref_x, ref_y), runs


def _figures(name):
    A, bt, data, (ref_obj, ref_x, ref_y), runs = _case(name)
    unique = slc.nondegenerate(A, *data, ref_x) if name.endswith("-generic") and not name.startswith("warm") else None
    out = {}
    for scaled, (x, y, obj, st, piv) in runs.items():
        assert (st == 0).all(), (name, scaled, st.tolist(), piv.tolist())
        assert piv.max() <= 20 * sum(A.shape), (name, piv.max())
        fig = dict(objective=slc.objective_error(obj, ref_obj), **slc.kkt_residuals(A, *data, x, y))
        if unique is not None:
            fig["duals"] = np.where(unique, slc.dual_error(y, ref_y), 0.0)
        out[scaled] = {k: float(v.max()) for k, v in fig.items()}
        out[scaled]["unique"] = 0 if unique is None else int(unique.sum())
        out[scaled]["pivots"] = float(piv.mean())
    return out


@pytest.mark.parametrize("name", CASES)
def test_specification_solves_every_generated_lp(name):
    """All 32 LPs optimal within the kernel's pivot limit, objective = HiGHS's, (x, y) a KKT pair - on raw and on scaled data."""
    figs = _figures(name)
    for scaled, fig in figs.items():
        print(f"\n[spec] {name} {'scaled' if scaled else 'raw'}: pivots mean {fig['pivots']:.1f}  " + "  ".join(f"{k} {fig[k]:.1e}" for k in slc.FLOOR if k in fig)
              + f"  ({fig['unique']} non-degenerate)")
        for k in slc.FLOOR:
            if k in fig:
                    assert fig[k] <= slc.TOL[k], (name, scaled, k, fig[k])


def test_floors_are_the_recorded_ones():
    """The worst figure of each kind over all cases stays within the floor recorded in the helper (x 10: the order of summation of
    another BLAS), so the GPU tolerances derived from the floors are not stale."""
    worst = {k: 0.0 for k in slc.FLOOR}
    for name in CASES:
        for fig in _figures(name).values():
            for k in worst:
                worst[k] = max(worst[k], fig.get(k, 0.0))
    print("\n[spec] floors: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 10.0 * slc.FLOOR[k], (k, v, slc.FLOOR[k])


def test_generator_points_are_feasible_and_dual_feasible():
    """The construction itself: x0 within all bounds and rows, (y0, c - A^T y0) of the allowed signs - feasible and bounded without a solver."""
    for name in CASES:
        A, bt, data, _, _ = _case(name)
        res = slc.kkt_residuals(A, *data, bt["x0"], bt["y0"])
        assert max(res["primal"].max(), res["dual_col"].max(), res["dual_row"].max()) <= 1e-14, (name, res)


def test_highs_row_duals_follow_the_kkt_sign_convention():
    """HiGHS's row duals are multipliers in the convention of kkt_residuals (y_i > 0 on an active lower side), and on the generic family
    the specification's y equals them entry by entry (a unique non-degenerate vertex): the direct comparison of the GPU tier is sound."""
    for name in ("40x24-generic", "39x25-generic", "5x3-generic"):
        A, bt, data, (ref_obj, ref_x, ref_y), runs = _case(name)
        res = slc.kkt_residuals(A, *data, ref_x, ref_y)
        assert max(v.max() for v in res.values()) <= 1e-8, (name, {k: v.max() for k, v in res.items()})
        flipped = slc.kkt_residuals(A, *data, ref_x, -ref_y)
        assert max(flipped["dual_col"].max(), flipped["dual_row"].max()) > 1e-3
        for x, y, *_ in runs.values():
            assert np.abs(y - ref_y).max() <= 1e-8 * (1 + np.abs(ref_y).max()), name


def test_kkt_residuals_notice_each_kind_of_error():
    A, bt, data, (ref_obj, ref_x, ref_y), runs = _case("40x24-generic")
    c, lb, ub, rlo, rhi = data
    x, y = runs[False][0], runs[False][1]
    assert slc.kkt_residuals(A, *data, x + 1e-6, y)["primal"].max() > 1e-8
    assert slc.kkt_residuals(A, *data, x, -y)["dual_row"].max() > 1e-3
    assert slc.kkt_residuals(A, *data, x, 0.5 * y)["dual_col"].max() > 1e-3
    assert slc.kkt_residuals(A, *data, bt["x0"], y)["gap"].max() > 1e-3
    assert np.isinf(slc.kkt_residuals(A, *data, x * np.nan, y)["primal"]).all()


def test_free_and_upper_only_column_rules():
    """The two rules the specification shares with the kernel beyond lower-bounded columns, on LPs small enough to solve by hand."""
    sx = slc.spec_module()
    # a free column is eligible on |d| and moves against the sign of d: min 2 x, -x <= 3 -> x = -3 (DOWN from 0), y = -2
    x, y, st, piv = sx.simplex_batch(np.array([[-1.0]]), np.array([[2.0]]), np.array([[-np.inf]]), np.array([[np.inf]]),
                                     np.array([[-np.inf]]), np.array([[3.0]]), tol_p=1e-10, tol_d=1e-12, tol_piv=1e-9)
    assert st[0] == 0 and x[0, 0] == -3.0 and y[0, 0] == -2.0
    # a column with only an upper bound starts AT it, on its upper side, and stays there when its cost pays for it
    x, y, st, piv = sx.simplex_batch(np.array([[1.0]]), np.array([[-1.0]]), np.array([[-np.inf]]), np.array([[4.0]]),
                                     np.array([[-np.inf]]), np.array([[10.0]]), tol_p=1e-10, tol_d=1e-12, tol_piv=1e-9)
    assert st[0] == 0 and piv[0] == 0 and x[0, 0] == 4.0
