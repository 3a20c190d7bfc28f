"""The fused PDLP kernel's results are BIT-IDENTICAL to the recorded ones when one block of its check iteration at a time moves the
state (tools/make_check_blocks_fixture.py).  The three-wave metric kernel reads the options of its gate, restart, steady and
ray-jump tests from the kernel-argument segment where they are used and packs its wave-uniform flags into one word; no FP64
operation, operand or order changes, so status, iteration count, jumps and flags are equal, obj is bitwise equal, and so is every
scenario's x row and y row (compared through a wrap-around sum of their bit patterns).

Cases, the first 4 scenarios of `wind_battery_24h` each: quiet checks only (limits 17 and 33); a KKT test that fails and re-arms
its gate; restarts with and without a weight change; a restart through polish_patience; a stall rescue; a ray jump taken (the
default options to the end) and refused; a warm start given up; the default options on the nuclear 24-h kernel and on the generic
kernel, which share the source and keep their code.  The fixture was recorded with the build before the change."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "check_blocks_parent.npz")


def _cases():
    from tools.make_check_blocks_fixture import CASES
    return list(CASES)


@gpu
@pytest.mark.parametrize("name", _cases())
def test_check_block_results_are_bit_identical(name):
    from tools.make_check_blocks_fixture import path_misses, solve_case
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


def test_fixture_shows_every_block_was_walked():
    """No GPU: the committed fixture has every array of every case, its recorded iteration counts, jumps, flags and row sums show that
    each case walked the block it is there for (tools/make_check_blocks_fixture.py, shape_misses), it names the sources it was
    recorded from, and stays small."""
    fx = np.load(FIXTURE)
    from tools.make_check_blocks_fixture import B, CASES, KEYS, shape_misses
    assert fx["cases"].tolist() == list(CASES)
    for key in KEYS:
        assert fx[key].shape == (len(CASES), B), key
    rec = {key: {name: fx[key][row] for row, name in enumerate(CASES)} for key in KEYS}
    for name in CASES:
        assert shape_misses(name, rec) == [], name
    assert len(str(fx["source_hash"])) == 16
    assert os.path.getsize(FIXTURE) < 64 * 1024
