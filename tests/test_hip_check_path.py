"""The fused PDLP kernel's results are BIT-IDENTICAL to the recorded ones on the small cases that reach every path of its check
iteration (tools/make_check_path_fixture.py: KKT test, restart, ray jump, warm start given up, iteration-limit epilogue; the
register-resident kernels of four shapes, the generic, QP and run-time compiled instantiations).

The check path is restructured for speed (uniform values on the scalar unit, no spills on the common path, the restart's matrix
re-read issued early), never for other numbers: status, iteration count, jumps and flags are equal, obj is bitwise equal, and
so is every scenario's x row and y row (compared through a wrap-around sum of their bit patterns).  The fixture was recorded
with the build before that restructuring; the infeasible / suspect path is covered by tests/test_hip_infeasible.py."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "check_path_parent.npz")


def _cases():
    from tools.make_check_path_fixture import CASES
    return list(CASES)


@gpu
@pytest.mark.parametrize("name", _cases())
def test_check_path_results_are_bit_identical(name):
    from tools.make_check_path_fixture import path_misses, solve_case
    fx = np.load(FIXTURE)
    res, stats = solve_case(name)
    assert path_misses(name, res, stats) == []
    for key in ("status", "iters", "jumps", "flags"):
        ref = fx[f"{name}/{key}"]
        assert res[key].dtype == ref.dtype and np.array_equal(res[key], ref), \
            (name, key, np.nonzero(res[key] != ref)[0][:8].tolist())
    for key in ("obj", "xsum", "ysum") + (("pw",) if f"{name}/pw" in fx.files else ()):
        ref, got = fx[f"{name}/{key}"], res[key]
        assert got.dtype == ref.dtype and got.shape == ref.shape, (name, key, got.dtype, got.shape)
        same = got.view(np.uint64) == ref.view(np.uint64)
        assert same.all(), (name, key, f"{int((~same).sum())} of {same.size} scenarios differ", np.nonzero(~same)[0][:8].tolist())


def test_fixture_covers_every_case_and_is_small():
    """No GPU: the committed fixture has every array of every case, names the sources it was recorded from, and stays a few KB."""
    fx = np.load(FIXTURE)
    from tools.make_check_path_fixture import CASES
    for name, (_, B, _, _) in CASES.items():
        for key in ("status", "iters", "jumps", "flags", "obj", "xsum", "ysum"):
            assert fx[f"{name}/{key}"].shape == (B,), (name, key)
    assert len(str(fx["source_hash"])) == 16
    assert os.path.getsize(FIXTURE) < 64 * 1024
