"""The fused PDLP kernel's results are BIT-IDENTICAL to the recorded ones at the edges of its segment loop
(tools/make_cadence_fixture.py): check cadences 1, 2, 3 and 16 - no, one, two, fifteen plain iterations between checks - under
iteration limits that end the solve before the first check, inside a segment or on a check, on the 24-h metric shape; cadences 1
and 3 on another register-resident shape, the 4-h kernel, the generic LDS-matrix kernel, the QP and the run-time compiled kernel.

Changes to how the kernel is compiled or scheduled (the metric kernel's three waves per SIMD, the order of independent work in
the plain-iteration loop) leave the FP64 operations and their operands alone: status, iteration count, jumps and flags are
equal, obj is bitwise equal, and so is every scenario's x row and y row (compared through a wrap-around sum of their bit
patterns).  The fixture was recorded with the build before the three-wave change; tests/test_hip_check_path.py holds the same at
the default cadence on the cases that reach every block of the check."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "hot_loop_cadence_parent.npz")


def _cases():
    from tools.make_cadence_fixture import CASES
    return list(CASES)


@gpu
@pytest.mark.parametrize("name", _cases())
def test_cadence_results_are_bit_identical(name):
    from tools.make_cadence_fixture import path_misses, solve_case
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
            (name, key, np.nonzero(res[key] != ref)[0][:8].tolist())
    for key in ("obj", "xsum", "ysum"):
        ref, got = fx[key][row], res[key]
        assert got.dtype == ref.dtype and got.shape == ref.shape, (name, key, got.dtype, got.shape)
        same = got.view(np.uint64) == ref.view(np.uint64)
        assert same.all(), (name, key, f"{int((~same).sum())} of {same.size} scenarios differ", np.nonzero(~same)[0][:8].tolist())


def test_fixture_covers_every_case_and_is_small():
    """No GPU: the committed fixture has every array of every case, names the sources it was recorded from, and stays small."""
    fx = np.load(FIXTURE)
    from tools.make_cadence_fixture import B, CADENCES, CASES, KEYS, LIMITS
    assert len(CASES) == len(CADENCES) * len(LIMITS) + 2 * 5
    assert fx["cases"].tolist() == list(CASES)
    for key in KEYS:
        assert fx[key].shape == (len(CASES), B), key
    assert len(str(fx["source_hash"])) == 16
    assert os.path.getsize(FIXTURE) < 64 * 1024
