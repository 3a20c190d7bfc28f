"""dsp_solve and dsp_create return BIT-IDENTICAL results on the branches that the other bit-equality fixtures do not reach
(tools/make_solve_paths_fixture.py): the fused path with a requested block size between two default solves, the generic kernel, the
simplex pass with its warm buffers grown and reused, the QP in float64 and the float32 solves, the run-time compiled shape with the lazy
compile of its QP instantiation, the streaming path at its iteration limit and to the end, the certificate pass with the host's
suspect count and with the fixed 8-block launch - and what dsp_solve refuses, it refuses without touching an output.

Per solve: status, iteration count, jumps, flags and every field of dsp_stats but kernel_ms are equal, obj is bitwise equal and so is
every scenario's x row and y row (compared through a wrap-around sum of their bit patterns).  A streaming solve that the recording
build itself did not reproduce bit for bit is marked `loose` in the fixture; its objectives are then compared at rtol = atol = 1e-9,
what tests/test_hip_stream.py allows between two runs of the same arithmetic.  The fixture was recorded with the build before the
host layer was split into passes."""
import ctypes as C
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "solve_paths_parent.npz")
SENTINEL = -12345.0


def _cases():
    from tools.make_solve_paths_fixture import CASES
    return list(CASES)


@gpu
@pytest.mark.parametrize("name", _cases())
def test_solve_paths_results_are_bit_identical(name):
    from tools.make_solve_paths_fixture import path_misses, solve_case
    from dispatches_amd.hip_solver import load_library
    fx = np.load(FIXTURE)
    # the reference is the build BEFORE the change under test: a fixture re-recorded with the loaded library would prove nothing
    assert str(fx["source_hash"]) != load_library().dsp_source_hash().decode()
    results = solve_case(name)
    assert path_misses(name, results) == []
    for label, res in results.items():
        ref = {k: fx[f"{name}/{label}/{k}"] for k in res}
        for key in ("status", "iters", "jumps", "flags", "stats"):
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


def _refusal_cases():
    """(what, batch of the handle, options of the solve, soft rows): everything dsp_solve refuses with DSP_ERR_INVALID."""
    bad = [dict(max_iter=0), dict(check_every=-1), dict(kkt_every=-1), dict(kkt_gate=-1.0), dict(stall_rescue=-1),
           dict(polish_patience=-1), dict(jump_rel=-1.0), dict(eps_rel=0.0), dict(eps_obj=-1.0), dict(eps_infeasible=-1.0), dict(pid_kp=-1.0),
           dict(restart_artificial=-1.0), dict(step_scale=0.0), dict(precision=2)]
    # the floating-point checks are written `!(x >= 0)` / `!(x > 0)`, so that a NaN is refused as well
    bad += [{k: float("nan")} for k in ("kkt_gate", "jump_rel", "eps_rel", "eps_obj", "eps_infeasible", "pid_kp", "restart_artificial", "step_scale")]
    cases = [(",".join(f"{k}={v}" for k, v in o.items()), "wind_battery_24h", o, False) for o in bad]
    # float32 iterates and soft rows exist for shapes without long vectors only (wind + PEM 48 h has them); float32 not when streaming
    cases += [("precision=1 with long vectors", "wind_pem_48h", dict(precision=1), False),
              ("row_compliance with long vectors", "wind_pem_48h", {}, True),
              ("precision=1 on a streaming handle", "price_taker_168", dict(precision=1), False)]
    return cases


@gpu
def test_refusals_leave_the_outputs_untouched_and_an_empty_batch_is_ok():
    import torch
    from dispatches_amd.hip_solver import DeviceLP, DspBatch, DspStats, default_options
    from tools.make_solve_paths_fixture import build_batch
    dev = torch.device("cuda", 0)
    handles = {}
    for what, kind, options, soft in _refusal_cases():
        if kind not in handles:
            lp, host = build_batch(kind)
            handles[kind] = (DeviceLP(lp, 0, default_options()), lp, {k: torch.as_tensor(v, device=dev) for k, v in host.items()})
        dlp, lp, t = handles[kind]
        B = t["c"].shape[0]
        out = dict(x=torch.full((B, lp.n), SENTINEL, dtype=torch.float64, device=dev), y=torch.full((B, lp.m), SENTINEL, dtype=torch.float64, device=dev),
                   obj=torch.full((B,), SENTINEL, dtype=torch.float64, device=dev), **{k: torch.full((B,), -77, dtype=torch.int32, device=dev)
                                                                                      for k in ("status", "iters", "jumps", "flags")})
        before = {k: v.clone() for k, v in out.items()}
        bt = DspBatch()
        bt.B = B
        bt.c, bt.c_stride = t["c"].data_ptr(), lp.n
        bt.var_lb, bt.var_lb_stride, bt.var_ub, bt.var_ub_stride = t["lb"].data_ptr(), lp.n, t["ub"].data_ptr(), lp.n
        bt.row_lb, bt.row_lb_stride, bt.row_ub, bt.row_ub_stride = t["rlo"].data_ptr(), lp.m, t["rhi"].data_ptr(), lp.m
        kappa = torch.zeros(lp.m, dtype=torch.float64, device=dev)
        if soft:
            bt.row_compliance, bt.row_compliance_stride = kappa.data_ptr(), 0
        bt.x, bt.y, bt.obj = out["x"].data_ptr(), out["y"].data_ptr(), out["obj"].data_ptr()
        bt.status, bt.iters, bt.jumps, bt.flags = (out[k].data_ptr() for k in ("status", "iters", "jumps", "flags"))
        opts = default_options(**options)
        stats = DspStats()
        rc = dlp.lib.dsp_solve(dlp.handle, C.byref(bt), C.byref(opts), C.byref(stats), 1, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
        assert rc == -1, (what, rc)                                  # DSP_ERR_INVALID
        for k, v in out.items():
            assert torch.equal(v, before[k]), (what, k)
    # an empty batch with a stats struct: DSP_OK, every field zeroed, nothing read
    dlp = handles["wind_battery_24h"][0]
    bt = DspBatch()
    bt.B = 0
    stats = DspStats()
    C.memset(C.byref(stats), 0xFF, C.sizeof(stats))
    assert dlp.lib.dsp_solve(dlp.handle, C.byref(bt), None, C.byref(stats), 1, None) == 0
    assert bytes(stats) == bytes(C.sizeof(stats))
    for dlp, _, _ in handles.values():
        dlp.close()


def test_fixture_covers_every_case_and_is_small():
    """No GPU: the committed fixture holds every array of every solve of every case, each solve's recorded dsp_stats show the branch it
    is there for, the statuses are the ones the case needs, it names the sources it was recorded from, and it stays small."""
    from tools.make_solve_paths_fixture import CASES, KEYS, STATS, STREAMING, path_misses
    fx = np.load(FIXTURE)
    assert fx["stats_fields"].tolist() == list(STATS)
    want = {"source_hash", "stats_fields"}
    for name, (_, _, steps, expect) in CASES.items():
        results = {}
        for label, B, options, soft, sync in steps:
            results[label] = {k: fx[f"{name}/{label}/{k}"] for k in KEYS}
            want |= {f"{name}/{label}/{k}" for k in KEYS + ("loose",)}
            for k in ("status", "iters", "jumps", "flags", "obj", "xsum", "ysum"):
                assert results[label][k].shape == (B,), (name, label, k)
            assert results[label]["stats"].shape == (len(STATS),) and results[label]["stats"].dtype == np.int64
            assert name in STREAMING or int(fx[f"{name}/{label}/loose"]) == 0, (name, label)
        assert path_misses(name, results) == [], name
        assert set(expect) <= {"matreg", "rtc", "simplex", "streaming", "precision", "quadratic"}
    assert set(fx.files) == want
    assert len(str(fx["source_hash"])) == 16
    assert os.path.getsize(FIXTURE) < 64 * 1024
