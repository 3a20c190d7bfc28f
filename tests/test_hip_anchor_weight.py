"""The fused PDLP kernel's results are BIT-IDENTICAL to the recorded ones on both sides of every edge of the anchor-weight table
(tools/make_anchor_weight_fixture.py): the metric kernel reads the Halpern weight 1 / (k + 2) of a plain segment from a device
table of K = 4096 entries where the whole segment lies below K and computes it as before where it does not.

The table holds what the kernel's own expression gives, so no FP64 operand changes: status, iteration count, jumps and flags are
equal, obj is bitwise equal, and so is every scenario's x row and y row (compared through a wrap-around sum of their bit
patterns).  Cases, 4 scenarios each: the default cadence under limits 1, 17 and 400; the default options to the end (restarts and a
ray jump take k back to 0 and the table is entered again); cadence 4000 under a limit of 8200 with every restart and jump
switched off (first segment from the table, second across K, third beyond it); cadences 4097 and 4098 (a segment that ends on K,
and one past it); cadence 3 on another register-resident shape and on the generic kernel, whose loops are unchanged.  The fixture
was recorded with the build before the table."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "anchor_weight_parent.npz")


def _cases():
    from tools.make_anchor_weight_fixture import CASES
    return list(CASES)


@gpu
@pytest.mark.parametrize("name", _cases())
def test_anchor_weight_results_are_bit_identical(name):
    from tools.make_anchor_weight_fixture import path_misses, solve_case
    from dispatches_amd.hip_solver import load_library
    fx = np.load(FIXTURE)
    # the reference is the build BEFORE the change under test: a fixture re-recorded with the loaded library would prove nothing
    assert str(fx["source_hash"]) != load_library().dsp_source_hash().decode()
    row = fx["cases"].tolist().index(name)
    res, stats = solve_case(name)
    assert path_misses(name, res, stats) == []
    for key in ("status", "iters", "jumps", "flags"):
        ref = fx[key][row]
        assert res[key].dtype == ref.dtype and np.array_equal(res[key], ref), \
            (name, key, res[key].tolist(), ref.tolist())
    for key in ("obj", "xsum", "ysum"):
        ref, got = fx[key][row], res[key]
        assert got.dtype == ref.dtype and got.shape == ref.shape, (name, key, got.dtype, got.shape)
        same = got.view(np.uint64) == ref.view(np.uint64)
        assert same.all(), (name, key, f"{int((~same).sum())} of {same.size} scenarios differ", np.nonzero(~same)[0].tolist())


def test_fixture_covers_every_case_and_is_small():
    """No GPU: the committed fixture has every array of every case, its recorded iteration counts and jumps walk the paths the cases
    are there for (to the limit without an event; solved with a ray jump), it names the sources it was recorded from, and stays small."""
    fx = np.load(FIXTURE)
    from tools.make_anchor_weight_fixture import B, CASES, KEYS, TABLE, shape_misses
    assert fx["cases"].tolist() == list(CASES)
    for key in KEYS:
        assert fx[key].shape == (len(CASES), B), key
    for row, name in enumerate(CASES):
        assert shape_misses(name, fx["iters"][row], fx["jumps"][row], fx["status"][row]) == [], name
    # the cases around the table's end: a first segment of exactly TABLE plain iterations, and one of TABLE + 1
    assert CASES[f"wind_battery_24h_ce{TABLE + 1}_mi4200"][1]["check_every"] - 1 == TABLE
    assert CASES[f"wind_battery_24h_ce{TABLE + 2}_mi4200"][1]["check_every"] - 1 == TABLE + 1
    assert len(str(fx["source_hash"])) == 16
    assert os.path.getsize(FIXTURE) < 64 * 1024
