"""The follow-up passes of the fused PDLP solve - the certificate pass behind a register-resident first pass, the
re-certification passes of dsp_options::recertify_passes - give BIT-IDENTICAL results however they are compiled and launched
(tools/make_followup_fixture.py).

Behind the three-wave metric kernel the passes run a light instantiation of the generic kernel in blocks of one wave; that is a
change of launch bounds and geometry, not of an FP64 operation.  The batch: 8 scenarios of the 24-h wind + battery LP, scenarios
1, 4 and 6 infeasible (initial state of charge 1e6 kWh, as in tests/test_hip_infeasible.py), through DeviceLP.solve with
sync_stats (the pass is sized by the suspect count the host reads), without it on a side stream (the fixed launch of 8 blocks) and
without it on four streams at once, each with its own outputs; all of it again with recertify_passes = 3, which changes nothing
because nothing is flagged; and one case whose options provoke DSP_FLAG_OBJ_WAIVED as
tests/test_hip_parity.py::test_device_side_recertification_passes does, with the three passes on.  Status, iteration count, jumps
and flags are equal, obj and every scenario's x row and y row (through a wrap-around sum of their bit patterns) bitwise equal to
a fixture recorded with the build before the change."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "followup_parent.npz")


def _cases():
    from tools.make_followup_fixture import CASES
    return list(CASES)


def _assert_bitwise(leg, res, fx, ref_leg):
    for key in ("status", "iters", "jumps", "flags"):
        ref = fx[f"{ref_leg}/{key}"]
        assert res[key].dtype == ref.dtype and np.array_equal(res[key], ref), \
            (leg, ref_leg, key, np.nonzero(res[key] != ref)[0][:8].tolist())
    for key in ("obj", "xsum", "ysum"):
        ref, got = fx[f"{ref_leg}/{key}"], res[key]
        assert got.dtype == ref.dtype and got.shape == ref.shape, (leg, ref_leg, key, got.dtype, got.shape)
        same = got.view(np.uint64) == ref.view(np.uint64)
        assert same.all(), (leg, ref_leg, key, f"{int((~same).sum())} of {same.size} scenarios differ", np.nonzero(~same)[0][:8].tolist())


@gpu
@pytest.mark.parametrize("name", _cases())
def test_followup_results_are_bit_identical(name):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    from tools.make_followup_fixture import CASES, INFEASIBLE_LEGS, STATUSES, path_misses, solve_case
    from dispatches_amd.hip_solver import load_library
    fx = np.load(FIXTURE)
    # the reference is the build BEFORE the change under test: a fixture re-recorded with the loaded library would prove nothing
    assert str(fx["source_hash"]) != load_library().dsp_source_hash().decode()
    res, stats = solve_case(name)
    assert path_misses(name, stats) == []
    assert list(res) == CASES[name][4]
    for leg, r in res.items():
        if leg in INFEASIBLE_LEGS:
            assert r["status"].tolist() == STATUSES, (leg, r["status"], r["iters"])
        _assert_bitwise(leg, r, fx, leg)
        if leg.startswith("waived_"):
            # the passes had work: without them the same options leave scenarios flagged (6 of 256 when the fixture was recorded), and
            # every one of those comes back certified - from a pass, with the iterations of its re-solve on top
            plain, _ = solve_case(name, options={k: v for k, v in CASES[name][2].items() if k != "recertify_passes"})
            flagged = (plain[leg]["flags"] & 1) != 0
            assert flagged.any(), "the provocation flags no scenario of this LP: the re-certification passes are not exercised"
            assert not (r["flags"] & 1)[flagged].any() and (r["iters"][flagged] > plain[leg]["iters"][flagged]).all(), \
                (np.nonzero(flagged)[0].tolist(), r["flags"][flagged], r["iters"][flagged], plain[leg]["iters"][flagged])
            assert np.array_equal(r["obj"][~flagged].view(np.uint64), plain[leg]["obj"][~flagged].view(np.uint64))
        if leg.startswith("recertify3_"):
            # no scenario is flagged: the three passes return at their first line and the arrays are those of the run without them
            assert not (r["flags"] & 1).any(), (leg, r["flags"])
            _assert_bitwise(leg, r, fx, leg[len("recertify3_"):])


def test_fixture_covers_every_leg_and_is_small():
    """No GPU: the committed fixture has every array of every leg, names the sources it was recorded from, and stays small."""
    fx = np.load(FIXTURE)
    from tools.make_followup_fixture import B, B_WAIVED, CASES, INFEASIBLE_LEGS, KEYS, LEGS, N_STREAMS, STATUSES
    assert len(CASES) == 7 and len(LEGS) == 2 * (2 + N_STREAMS) + 1 and len(INFEASIBLE_LEGS) == len(LEGS) - 1
    assert fx["legs"].tolist() == LEGS
    assert sorted(fx.files) == sorted(["source_hash", "legs"] + [f"{leg}/{k}" for leg in LEGS for k in KEYS])
    for leg in LEGS:
        for key in KEYS:
            assert fx[f"{leg}/{key}"].shape == ((B,) if leg in INFEASIBLE_LEGS else (B_WAIVED,)), (leg, key)
            assert fx[f"{leg}/{key}"].dtype == (np.int32 if key in ("status", "iters", "jumps", "flags") else
                                                np.float64 if key == "obj" else np.uint64), (leg, key)
        if leg in INFEASIBLE_LEGS:
            assert fx[f"{leg}/status"].tolist() == STATUSES, leg
    assert len(str(fx["source_hash"])) == 16
    assert os.path.getsize(FIXTURE) < 64 * 1024
