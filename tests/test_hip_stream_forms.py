"""Every form of the HBM-resident ("streaming") path and every branch of its host layer returns what the build before the host layer
was cut into steps returned (tools/make_stream_forms_fixture.py): the two-launch form without and with long columns, the tile form
with its deferred and its staged kernel, small tiles and per-scenario bounds, the lane form in one phase, repacking, told not to
repack and with per-scenario bounds, the block form, the certificate sequence from the period loop, from the lane form's
certify-then-repack and in the block form's kernel, the iteration limit in the tile and the lane form, and the interior-point form
leaving one member to the forms behind it.

Per solve: status, iteration count, jumps, flags and every field of dsp_stats but kernel_ms are equal, obj is bitwise equal and so is
every scenario's x row and y row (compared through a wrap-around sum of their bit patterns).  A solve that the recording build
itself did not reproduce bit for bit is marked `loose` in the fixture; its objectives are then compared at rtol = atol = 1e-9, what
tests/test_hip_stream.py allows between two runs of the same arithmetic (the recorded fixture marks none).

The one difference the change was allowed: what a solve reports no longer depends on what the handle solved before.  A handle has one
matrix, hence one form per batch size and bounds, so the fixture cannot show a stale figure; the block form's report is asserted
directly (test_block_form_reports_the_two_launch_figure_on_every_solve)."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "stream_forms_parent.npz")


def _cases():
    from tools.make_stream_forms_fixture import CASES
    return list(CASES)


@gpu
@pytest.mark.parametrize("name", _cases())
def test_stream_forms_results_are_those_of_the_parent(name):
    from tools.make_stream_forms_fixture import RECORDED, form_misses, solve_case
    from dispatches_amd.hip_solver import load_library
    fx = np.load(FIXTURE)
    # the reference is the build BEFORE the change under test: a fixture re-recorded with the loaded library would prove nothing
    assert str(fx["source_hash"]) != load_library().dsp_source_hash().decode()
    before = {k: os.environ.get(k) for k in ("DSP_NO_IPM", "DSP_STREAM_NO_LANE", "DSP_LANE_MIN_B")}
    results = solve_case(name)
    assert before == {k: os.environ.get(k) for k in before}              # the case's environment is gone again
    assert form_misses(name, results) == []
    for label, res in results.items():
        ref = {k: fx[f"{name}/{label}/{k}"] for k in RECORDED}
        for key in ("status", "iters", "jumps", "flags", "stats", "nm"):
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


@gpu
def test_block_form_reports_the_two_launch_figure_on_every_solve():
    """A block-form solve reports stream_bytes_per_iteration = 8 (8 n + 6 m) on a fresh handle, and the same on the handle's second solve."""
    from tools.make_stream_forms_fixture import BLOCK, STATS, solve_case
    results = solve_case("block")
    assert list(results) == ["solve0", "solve1"]
    for label, res in results.items():
        stats = dict(zip(STATS, res["stats"].tolist()))
        n, m = (int(v) for v in res["nm"])
        assert stats["stream_form"] == BLOCK and stats["stream_bytes_per_iteration"] == 8 * (8 * n + 6 * m), (label, stats)
        assert stats["stream_phases"] == 0 and stats["ipm_solved"] == 0, (label, stats)


def test_fixture_covers_every_case_and_is_small():
    """No GPU: the committed fixture holds every array of every solve of every case, each solve's recorded dsp_stats show the form and
    the branch it is there for, it names the sources it was recorded from, and it stays small."""
    from tools.make_stream_forms_fixture import CASES, LANE_REPACK_B, RECORDED, STATS, form_misses
    fx = np.load(FIXTURE)
    assert fx["stats_fields"].tolist() == list(STATS)
    assert int(fx["lane_repack_B"]) == LANE_REPACK_B == CASES["lane_repacking"]["B"] == CASES["lane_no_repacking"]["B"]
    want = {"source_hash", "stats_fields", "lane_repack_B"}
    for name, c in CASES.items():
        results = {}
        for k in range(c["solves"]):
            label = f"solve{k}"
            results[label] = {key: fx[f"{name}/{label}/{key}"] for key in RECORDED}
            want |= {f"{name}/{label}/{key}" for key in RECORDED + ("loose",)}
            for key in ("status", "iters", "jumps", "flags", "obj", "xsum", "ysum"):
                assert results[label][key].shape == (c["B"],), (name, label, key)
            assert results[label]["stats"].shape == (len(STATS),) and results[label]["stats"].dtype == np.int64
            assert int(fx[f"{name}/{label}/loose"]) in (0, 1)
        assert form_misses(name, results) == [], name
    assert set(fx.files) == want
    assert len(str(fx["source_hash"])) == 16
    assert os.path.getsize(FIXTURE) < 64 * 1024
