"""Every branch of the interior-point form's host layer (csrc/dsp_ipm.hip: plan, workspace, settings, launch geometry, Newton loop,
lane packing) returns what the build before that layer was cut into steps returned (tools/make_ipm_forms_fixture.py): half-bandwidth
6 with a wide column at the automatic geometry, as sequential walks and in nine ragged partitions; half-bandwidth 8 without a wide
column (the one-wave reduced solve) at the automatic geometry and in 31 partitions; the lanes packed into fewer groups, told not to
pack, two lane groups of which the second is ragged; a member the form gives up on; every member handed over warm at the iteration
limit; one handle whose workspace grows and is reused; and the default case under the trace, which changes nothing but prints.

Per solve: status, iteration count, jumps, flags and every field of dsp_stats but kernel_ms are equal, obj is bitwise equal and so is
every scenario's x row and y row (compared through a wrap-around sum of their bit patterns).  A traced solve also printed the
recorded `steps taken back` and `lanes` lines and packed its lanes as often.  A solve that the recording build itself did not
reproduce bit for bit is marked `loose` in the fixture; its objectives are then compared at rtol = atol = 1e-9 (the recorded
fixture marks none).

Steps taken back (k_ipm_undo): the recorder found no one-week or four-week LP on which the recording build takes a step back
(DSP_IPM_REFTOL_END = 1e-7, 1e-5, 1e-3 on 64 members of the wide family at T = 168 and 672: none), and the fixture says so
(`taken_back_found` = 0); that branch stays with tests/test_hip_ipm.py::test_year_long_batch_of_256_distinct_lps[steps_taken_back]."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ipm_forms_parent.npz")


def _cases():
    from tools.make_ipm_forms_fixture import CASES
    return list(CASES)


@gpu
@pytest.mark.parametrize("name", _cases())
def test_ipm_forms_results_are_those_of_the_parent(name):
    from tools.make_ipm_forms_fixture import CASES, ENV, INTS, KEYS, TEXT, form_misses, recorded_keys, solve_case
    from dispatches_amd.hip_solver import load_library
    fx = np.load(FIXTURE)
    # the reference is the build BEFORE the change under test: a fixture re-recorded with the loaded library would prove nothing
    assert str(fx["source_hash"]) != load_library().dsp_source_hash().decode()
    before = {k: os.environ.get(k) for k in ENV}
    results = solve_case(name)
    assert before == {k: os.environ.get(k) for k in before}              # the case's environment is gone again
    assert form_misses(name, results) == []
    traced = "DSP_IPM_TRACE" in CASES[name]["env"]
    for label, res in results.items():
        ref = {k: fx[f"{name}/{label}/{k}"] for k in recorded_keys(CASES[name])}
        for key in INTS + (TEXT if traced else ()):
            assert res[key].dtype == ref[key].dtype and np.array_equal(res[key], ref[key]), \
                (name, label, key, res[key].tolist(), ref[key].tolist())
        if int(fx[f"{name}/{label}/loose"]):
            assert np.allclose(res["obj"], ref["obj"], rtol=1e-9, atol=1e-9, equal_nan=True), (name, label, res["obj"], ref["obj"])
            continue
        for key in ("obj", "xsum", "ysum"):
            got = res[key]
            assert got.dtype == ref[key].dtype and got.shape == ref[key].shape, (name, label, key, got.dtype, got.shape)
            same = got.view(np.uint64) == ref[key].view(np.uint64)
            assert same.all(), (name, label, key, f"{int((~same).sum())} of {same.size} scenarios differ", np.nonzero(~same)[0].tolist())
    if name == "trace":                                                   # the trace prints, and changes no bit of the default case
        for key in KEYS:
            assert results["solve0"][key].tobytes() == fx[f"default/solve0/{key}"].tobytes(), key


def test_fixture_covers_every_case_and_is_small():
    """No GPU: the committed fixture holds every array of every solve of every case, each solve's recorded dsp_stats and printed lines
    show the branch it is there for, it names the sources it was recorded from and what the recorder found, and it stays small."""
    from tools.make_ipm_forms_fixture import CASES, KEYS, PACK_B, STATS, TAKEN_BACK, form_misses, recorded_keys
    fx = np.load(FIXTURE)
    assert fx["stats_fields"].tolist() == list(STATS)
    assert int(fx["pack_B"]) == PACK_B == CASES["lane_packing"]["steps"][0] == CASES["no_packing"]["steps"][0]
    assert int(fx["taken_back_found"]) == int(TAKEN_BACK is not None) == int("steps_taken_back" in CASES)
    assert fx["taken_back_setting"].tolist() == list(map(str, TAKEN_BACK or ()))
    want = {"source_hash", "stats_fields", "pack_B", "taken_back_found", "taken_back_setting"}
    for name, c in CASES.items():
        results = {}
        for k, B in enumerate(c["steps"]):
            label = f"solve{k}"
            results[label] = {key: fx[f"{name}/{label}/{key}"] for key in recorded_keys(c)}
            want |= {f"{name}/{label}/{key}" for key in recorded_keys(c) + ("loose",)}
            for key in ("status", "iters", "jumps", "flags", "obj", "xsum", "ysum"):
                assert results[label][key].shape == (B,), (name, label, key)
            assert results[label]["stats"].shape == (len(STATS),) and results[label]["stats"].dtype == np.int64
            assert int(fx[f"{name}/{label}/loose"]) in (0, 1)
        assert form_misses(name, results) == [], name
    for key in KEYS:
        assert fx[f"trace/solve0/{key}"].tobytes() == fx[f"default/solve0/{key}"].tobytes(), key
    assert set(fx.files) == want
    assert len(str(fx["source_hash"])) == 16
    assert os.path.getsize(FIXTURE) < 64 * 1024
