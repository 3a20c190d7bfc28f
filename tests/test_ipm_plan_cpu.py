"""CPU tests of the interior-point form's plan (csrc/dsp_ipm_plan.hpp: what ipm_create of csrc/dsp_ipm.hip uploads): the band's
product lists against  A_narrow diag(theta) A_narrow'  computed densely, the two ELLs and the wide columns' CSR against the matrix'
own products, the padding, the refusals each at its edge, the rounding of the half-bandwidth and the partition geometry.
tests/ipm_plan_harness.cpp builds the time-banded matrices and does the dense arithmetic.  GPU side: tests/test_hip_ipm_forms.py."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipm_plan") / "ipm_plan_harness")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "ipm_plan_harness.cpp")], check=True)

    def run(T, rows, band, wide, seed=7, parts=0, row_entries=0, Lp=0):
        args = [str(v) for v in (T, rows, band, wide, seed, parts, row_entries, Lp)]
        return json.loads(subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout)
    return run


@pytest.mark.parametrize("T,rows,band,wide,seed", [
    (40, 2, 6, 1, 1),        # the wind + battery shape in small: half-bandwidth 6, one wide column
    (33, 3, 8, 0, 2),        # the nuclear shape: half-bandwidth 8, none
    (25, 4, 3, 4, 3),        # a narrow band, as many wide columns as the form carries
    (64, 1, 7, 2, 4),        # band 7 is carried as 8
    (101, 1, 1, 3, 5),       # bidiagonal
])
def test_plan_reproduces_the_matrix(harness, T, rows, band, wide, seed):
    res = harness(T, rows, band, wide, seed)
    assert res["ok"] == 1 and res["m"] == T * rows and res["K"] == wide, res
    assert res["W"] == (6 if band <= 6 else 8), res
    assert 0 <= res["band_err"] <= 1e-12 and res["beyond_band"] == 0.0, res           # B(t, t - k), every t, k <= W; nothing beyond W
    assert 0 <= res["ax_err"] <= 1e-12 and 0 <= res["aty_err"] <= 1e-12, res           # (entries of magnitude 0.5 .. 2, at most 16 per sum)
    assert res["padding_ok"] == 1 and res["wide_ok"] == 1, res
    assert res["rw"] % 4 == 0 and res["cw"] % 4 == 0 and res["bw"] % 4 == 0 and max(res["rw"], res["cw"], res["bw"]) <= 16, res


def test_refusals_each_at_its_edge(harness):
    assert harness(63, 1, 6, 1)["ok"] == 0 and harness(64, 1, 6, 1)["ok"] == 1         # fewer than 64 rows
    assert harness(80, 1, 6, 4)["ok"] == 1 and harness(80, 1, 6, 5)["ok"] == 0         # more than four wide columns
    assert harness(80, 1, 8, 1)["ok"] == 1 and harness(80, 1, 9, 1)["ok"] == 0         # a half-bandwidth above 8
    full = harness(80, 1, 6, 0, row_entries=16)
    assert full["ok"] == 1 and full["rw"] == 16 and full["bw"] == 16, full              # 16 entries in a row fit
    assert full["band_err"] <= 1e-12 and full["ax_err"] <= 1e-12 and full["padding_ok"] == 1, full
    assert harness(80, 1, 6, 0, row_entries=17)["ok"] == 0                              # 17 do not


@pytest.mark.parametrize("band", range(1, 9))
def test_half_bandwidth_is_carried_as_6_or_8(harness, band):
    assert harness(70, 1, band, 1)["W"] == (6 if band <= 6 else 8)


def test_partition_geometry(harness):
    """The rows of the table in tests/test_ipm_par_cpu.py, out of the planner."""
    auto = harness(505, 2, 6, 1)
    assert (auto["m"], auto["W"], auto["P"], auto["Lp"]) == (1010, 6, 3, 337), auto    # the one-week price-taker LP: automatic
    finer = harness(505, 2, 8, 1, parts=8)
    assert (finer["W"], finer["P"], finer["Lp"]) == (8, 8, 127), finer
    nine = harness(333, 1, 6, 1, parts=9, Lp=40)
    assert nine["P"] == 9 and nine["Lp"] == 37, nine                                    # asked for 9: keeps 9
    assert (nine["rows_P"], nine["rows_Lp"]) == (9, 40), nine                           # partitions of 40 rows: a tail of 13 is one of its own
    joined = harness(330, 1, 6, 1, Lp=40)
    assert (joined["rows_P"], joined["rows_Lp"]) == (8, 40), joined                     # a tail of 10 joins the partition before it
    assert joined["P"] == 1 and joined["Lp"] == 330, joined                             # below 512 rows without a request: one
    asked = harness(330, 1, 8, 1, parts=20)
    assert (asked["P"], asked["Lp"]) == (10, 32), asked                                 # 4 W rows at least; the tail of 10 joins
    assert harness(333, 1, 6, 1)["P"] == 1 and harness(333, 1, 6, 1, parts=1)["P"] == 1
    assert harness(600, 1, 6, 1)["P"] == 2                                              # from 512 rows on
    ten = harness(2560, 1, 6, 1)
    assert (ten["P"], ten["Lp"]) == (10, 256), ten                                      # partitions of 256 rows at least
