"""The recorder of the descriptor double loop (rolling_flowsheets.py::BatchedDoubleLoop(record=(plants, days))) and the writer that turns
a record into the reference's four result files per generator.

What a run of the reference leaves behind is bidder_detail.csv, bidding_model_detail.csv, tracker_detail.csv and
tracking_model_detail.csv (its post-processing, case_studies/renewables_case/double_loop_utils.py:212-221, reads them by name); the
host objects of this project write them with the reference's column names.  The device loop keeps, for up to 64 chosen plants, what
those files are made of - the state every LP was built from, every solution, curve, dispatch and delivered power - hour by hour in
device buffers:

    group    clock                 row                          launched
    daily    hour_t                day the bid is for           at the end of the day-ahead step
    bid      bid_hour_t (ruc_hour) day the bid is for (d + 1)   at the end of the day-ahead step made at the RUC hour
    hour     hour_t                the hour                     after the tracking solve (and the ledger), before the hand-off
    after    hour_t - 1            the hour that just ended     after the hand-off

Each group is ONE launch of dsp_loop_record (include/dsp_hip.h, ABI 21: a gather of strided segments into the row the device clock
names), so the record is written by the replayed hipGraphs too; the tensor form (`LoopRecorder._write_tensors`: index_select /
index_copy_ at the same row rule) is the specification and the CPU backend of the tests, bit for bit.  Rows outside the recorded span
land in a spare last row of every buffer (the rule of rolling.py::_record)."""
from __future__ import annotations

import numpy as np

RECORD_MAX_PLANTS, RECORD_MAX_SEGMENTS = 64, 16        # DSP_RECORD_MAX_PLANTS / DSP_RECORD_MAX_SEGMENTS of include/dsp_hip.h


def check_record(record, B):
    """record=(plants, days) -> (list of plant indices, days); ValueError as BatchedDoubleLoop's docstring states"""
    try:
        plants, days = record
        plants = list(plants)
    except (TypeError, ValueError):
        raise ValueError(f"record is None or (plants, days), not {record!r}") from None
    if not plants or any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) for p in plants):
        raise ValueError("record: plants is a non-empty list of integer plant indices")
    plants = [int(p) for p in plants]
    if len(plants) > RECORD_MAX_PLANTS:
        raise ValueError(f"record: at most {RECORD_MAX_PLANTS} plants can be recorded, not {len(plants)}")
    if len(set(plants)) != len(plants):
        raise ValueError(f"record: plants must be distinct, not {plants}")
    if any(b <= a for a, b in zip(plants, plants[1:])):
        raise ValueError(f"record: plants must be increasing, not {plants}")
    if plants[0] < 0 or plants[-1] >= B:
        raise ValueError(f"record: plants must lie in [0, {B}), not {plants}")
    if isinstance(days, bool) or not isinstance(days, (int, np.integer)) or days < 1:
        raise ValueError(f"record: days must be an integer >= 1, not {days!r}")
    return plants, int(days)


class LoopRecorder:
    """The record of one BatchedDoubleLoop: buffers [rows + 1, plants, ...], the groups' segments, the two forms of a write."""

    def __init__(self, loop, plants, days, max_bytes):
        import torch
        self.loop, self.plants, self.days = loop, plants, days
        self.days_bid = 0                              # days for which a bid has been recorded (host count, like loop.hour)
        L, dev = loop, loop.dev
        B, S, ns, R = L.B, L.S, len(L.scale), len(plants)
        f64, i32 = torch.float64, torch.int32
        self.plants_t = torch.as_tensor(plants, dtype=torch.int64, device=dev)
        has_lp, curves = not L.parametrized, L.stochastic                    # bidding LPs; curves and cleared dispatches
        self.has_lp, self.has_curves = has_lp, curves

        def daily(bid):
            offer, curve, count, prices = L._day_ahead_buffers(bid) if curves else \
                ((L.pend_offer, None, None, L.pend_prices) if bid else (L.da_offer, None, None, L.da_prices))
            segs = []
            if has_lp:
                rows = 1 if L.coupled_da else S                              # rows of the day-ahead batch per plant
                n1 = L.da.n1 if L.coupled_da else L.da.lp.n
                if L.coupled_da and L.da.lp.n != S * n1:
                    raise RuntimeError("the coupled day-ahead LP is not S blocks of the template's columns")
                if ns:                                                        # the state the bid was built on (ruc_hour: the projected one)
                    segs.append(("da_state", (lambda: L.proj_state[-1]) if bid else (lambda: L.state), (ns,), f64))
                segs += [("da_x", lambda: L.da.out["x"], (S, n1), f64), ("da_obj", lambda: L.da.out["obj"], (rows,), f64),
                         ("da_c0", lambda: L.da.c0, (rows,), f64), ("da_status", lambda: L.da.out["status"], (rows,), i32),
                         ("da_iters", lambda: L.da.out["iters"], (rows,), i32)]
            if curves:
                segs += [("da_curve", lambda: curve, tuple(curve.shape[1:]), i32), ("da_count", lambda: count, (24,), i32)]
            return segs + [("da_offer", lambda: offer, (24,), f64), ("da_prices", lambda: prices, (24,), f64)]

        hourly = [("state", lambda: L.state, (ns,), f64)] if ns else []
        if has_lp:
            per = L.rt.per_plant or S                                        # rows of the real-time batch per plant
            hourly += [("rt_x", lambda: L.rt.out["x"], (per, L.rt.lp.n), f64), ("rt_obj", lambda: L.rt.out["obj"], (per,), f64),
                       ("rt_c0", lambda: L.rt.c0, (per,), f64), ("rt_status", lambda: L.rt.out["status"], (per,), i32)]
        if curves:
            hourly += [("rt_curve", lambda: L.rt_curve, tuple(L.rt_curve.shape[1:]), i32), ("rt_count", lambda: L.rt_count, (L.tr.T,), i32),
                       ("rt_dispatch", lambda: L.rt_dispatch, (L.tr.T,), f64)]
        hourly += [("tr_x", lambda: L.tr.out["x"], (L.tr.lp.n,), f64), ("tr_obj", lambda: L.tr.out["obj"], (), f64),
                   ("tr_c0", lambda: L.tr.c0, (), f64), ("tr_status", lambda: L.tr.out["status"], (), i32)]
        if L.ledger:                                                          # [F, B]: plant-minor, the reason segments carry two strides
            hourly.append(("ledger_hour", lambda: L.ledger_hour.t(), (len(L.ledger_keys),), f64))
        H = 24 * days
        self.groups = {"daily": dict(clock=L.hour_t, divisor=24, offset=0, rows=days, segments=daily(False)),
                       "hour": dict(clock=L.hour_t, divisor=1, offset=0, rows=H, segments=hourly),
                       "after": dict(clock=L.hour_t, divisor=1, offset=-1, rows=H, segments=[("delivered", lambda: L.delivered, (), f64)])}
        if L.ruc_hour is not None:                     # the bid made at the RUC hour: its own clock, the projected state, the pending buffers
            self.groups["bid"] = dict(clock=L.bid_hour_t, divisor=24, offset=0, rows=days, segments=daily(True))
        self.buf, self.hourly_keys, self.daily_keys = {}, [], []
        total = 0
        for name in ("daily", "hour", "after"):
            g = self.groups[name]
            if len(g["segments"]) > RECORD_MAX_SEGMENTS:
                raise RuntimeError(f"the {name} record has {len(g['segments'])} segments: the kernel takes {RECORD_MAX_SEGMENTS}")
            for key, _, trail, dtype in g["segments"]:
                shape = (g["rows"] + 1, R) + tuple(trail)
                total += int(np.prod(shape)) * (8 if dtype == f64 else 4)
                (self.daily_keys if name == "daily" else self.hourly_keys).append(key)
        self.bytes = total
        if total > max_bytes:
            raise ValueError(f"record: the buffers of {R} plants over {days} days take {total} bytes, more than record_max_bytes = {max_bytes}")
        for name in ("daily", "hour", "after"):
            g = self.groups[name]
            for key, _, trail, dtype in g["segments"]:
                self.buf[key] = torch.zeros((g["rows"] + 1, R) + tuple(trail), dtype=dtype, device=dev)
            g["rows_t"] = torch.full((), g["rows"], dtype=torch.int64, device=dev)
        if "bid" in self.groups:
            self.groups["bid"]["rows_t"] = self.groups["daily"]["rows_t"]
        self._desc = {name: self._describe(g) for name, g in self.groups.items()} if L.use_fused else None

    @staticmethod
    def _plant_rows(t, B):
        """a source -> its [B, width] view, no copy: [B * rows, n] / [B, ...] contiguous, [B], or a strided 2-d view such as [F, B].t()"""
        if t.dim() == 1 and t.shape[0] == B:
            return t.unsqueeze(1)
        if t.is_contiguous():
            return t.view(B, -1)
        if t.dim() != 2 or t.shape[0] != B:
            raise RuntimeError("a recorded source is a contiguous tensor or a strided [B, width] view")
        return t

    def _describe(self, g):
        """-> the DspLoopRecordDesc (hip_solver.py) of a group: pointers and strides of the live buffers, taken once (they are persistent)"""
        from .hip_solver import DspLoopRecordDesc
        B, R = self.loop.B, len(self.plants)
        d = DspLoopRecordDesc()
        d.n_plants, d.n_segments = R, len(g["segments"])
        for q, b in enumerate(self.plants):
            d.plants[q] = b
        d.clock, d.divisor, d.offset, d.rows = g["clock"].data_ptr(), g["divisor"], g["offset"], g["rows"]
        for s, (key, source, trail, dtype) in enumerate(g["segments"]):
            v, dst = self._plant_rows(source(), B), self.buf[key]
            width = int(np.prod(trail)) if trail else 1
            if v.shape[1] != width or v.dtype != dst.dtype:
                raise RuntimeError(f"recorded source {key!r} is [{B}, {v.shape[1]}] {v.dtype}, the record holds {width} {dst.dtype} per plant")
            seg = d.segments[s]
            seg.src, seg.dst = v.data_ptr(), dst.data_ptr()
            seg.plant_stride, seg.elem_stride = v.stride(0), v.stride(1) if width > 1 else 1
            seg.width, seg.elem_bytes = width, v.element_size()
        return d

    def write(self, name):
        """record group `name` now (capturable in both forms: the row is computed from the device clock)"""
        if self._desc is not None:
            import ctypes as C
            self.loop._call(self.loop._lib.dsp_loop_record, C.byref(self._desc[name]), self.loop.B)
        else:
            self._write_tensors(name)

    def _write_tensors(self, name):
        """the specification of dsp_loop_record: t = clock + offset; row = t // divisor if 0 <= t and t // divisor < rows, else the spare
        row `rows`; buffer[row, q] = source[plants[q]]"""
        import torch
        g, B = self.groups[name], self.loop.B
        t = g["clock"] + g["offset"] if g["offset"] else g["clock"]
        r = torch.div(t, g["divisor"], rounding_mode="floor") if g["divisor"] != 1 else t
        row = torch.where((t < 0) | (r >= g["rows_t"]), g["rows_t"], r).view(1)
        for key, source, _, _ in g["segments"]:
            dst = self.buf[key]
            value = source().reshape(B, -1).index_select(0, self.plants_t).to(dst.dtype)
            dst.view(dst.shape[0], dst.shape[1], -1).index_copy_(0, row, value.unsqueeze(0))

    def recorded(self):
        H, D = min(self.loop.hour, 24 * self.days), min(self.days_bid, self.days)
        out = {key: self.buf[key][:H].cpu().numpy() for key in self.hourly_keys}
        out.update({key: self.buf[key][:D].cpu().numpy() for key in self.daily_keys})
        out["plants"] = np.asarray(self.plants, dtype=np.int64)
        return out

    def reset(self):
        for t in self.buf.values():
            t.zero_()
        self.days_bid = 0


# ---- the writer: a record -> the reference's four files per generator, through the host classes' own row builders ------------------------
def _plant_model_object(loop, b):
    """-> a factory of the flowsheet's model object for plant b: its own window of the capacity factors (hour 0 = its start), its sizes"""
    mo = loop.bidder.bidding_model_object
    cls = mo.__class__
    if loop.flowsheet == "nuclear":
        kw = {}
        if loop.nuclear_sized:
            kw = dict(pem_mw=float(loop.pem_mw[b]), tank_kg=float(loop.tank_kg[b]), h2_price=float(loop.h2_price[b]), h2_demand=float(loop.h2_demand[b]))
        return lambda: cls(mo.model_data, **kw)
    cfs = list(np.roll(loop.cf_series.cpu().numpy(), -int(loop.start[b].item())))
    wind = float(loop.wind_mw[b]) if loop.sized else float(mo._wind_pmax_mw)
    if loop.flowsheet == "wind_pem":
        return lambda: cls(mo.model_data, wind_capacity_factors=cfs, wind_pmax_mw=wind, pem_pmax_mw=mo._pem_pmax_mw)
    batt = (float(loop.battery_mw[b]), float(loop.battery_mwh[b])) if loop.sized else (mo._battery_pmax_mw, mo._battery_energy_capacity_mwh)
    return lambda: cls(model_data=mo.model_data, wind_capacity_factors=cfs, wind_pmax_mw=wind, battery_pmax_mw=batt[0], battery_energy_capacity_mwh=batt[1])


class _HourBlock:
    """A populated block of one horizon of one plant whose expressions are moved to the window that starts at a given hour - what
    update_model leaves after that many implemented hours - so that the model object's own _result_columns reads a recorded solution"""

    def __init__(self, model_object, horizon, n_series):
        from .lp import LinearBlock
        self.mo, self.block, self.N = model_object, LinearBlock("fs"), n_series
        model_object.populate_model(self.block, horizon)

    def at(self, hour, x):
        b = self.block
        if hasattr(b, "_time_idx"):                    # the wind flowsheets: the constants of wind_waste / tot_cost follow the window
            b._time_idx = int(hour) % self.N
            self.mo._write_expressions(b, self.mo._get_capacity_factors(b))
        b.solution = np.asarray(x)
        return b


def curve_bids(curve, count, first_hour, gen, p_min):
    """a stored curve [T, slots, 2] (integer cents: power, marginal price) with count [T] points used -> the bids dictionary the
    bidders' _record_bids take: p_cost = the cumulative cost of the marginal curve (convert_marginal_costs_to_actual_costs), p_max its
    last power"""
    from .workflow.utils import convert_marginal_costs_to_actual_costs
    bids = {}
    for t in range(curve.shape[0]):
        k = int(count[t])
        pairs = [(int(curve[t, i, 0]) / 100.0, int(curve[t, i, 1]) / 100.0) for i in range(k)]
        p_max = pairs[-1][0] if pairs else None
        bids[first_hour + t] = {gen: {"p_cost": convert_marginal_costs_to_actual_costs(pairs), "p_min": p_min, "p_max": p_max,
                                      "startup_capacity": p_max, "shutdown_capacity": p_max}}
    return bids


def write_results(loop, path, start_date="2020-01-02"):
    """path/plant_<index>/{bidder_detail, bidding_model_detail, tracker_detail, tracking_model_detail}.csv for every recorded plant of
    `loop` (BatchedDoubleLoop.write_results).  bidding_model_detail.csv is left out in parametrized mode, which has no bidding LP (the
    host's parametrized bidders write none either)."""
    import datetime
    import os
    import types
    import pandas as pd
    from .workflow import Tracker
    from .workflow.bidder import Bidder, SelfScheduler
    from .workflow.parametrized_bidder import ParametrizedBidder
    rec = loop.recorded()
    day0 = datetime.date.fromisoformat(str(start_date))
    date = lambda d: (day0 + datetime.timedelta(days=int(d))).isoformat()
    H = rec["delivered"].shape[0]
    D = rec["da_offer"].shape[0]
    S, Tc = loop.S, loop.tr.T
    layout = ParametrizedBidder if loop.parametrized else SelfScheduler if loop.self_schedule else Bidder
    tr_const = loop.tr.PT_const.cpu().numpy()
    for q, b in enumerate(rec["plants"].tolist()):
        out = os.path.join(path, f"plant_{b}")
        os.makedirs(out, exist_ok=True)
        make = _plant_model_object(loop, b)
        bid_mo, tr_mo = make(), make()
        gen, md = bid_mo.model_data.gen_name, bid_mo.model_data
        p_min = md.p_min if loop.p_min_cents_plant is None else float(loop.p_min_cents_plant[b].item()) / 100.0
        book = types.SimpleNamespace(n_scenario=S, bids_result_list=[])      # what the three _record_bids read and fill of a bidder
        tr_blk = _HourBlock(tr_mo, Tc, loop.N)
        if not loop.parametrized:
            da_blk, rt_blk = _HourBlock(bid_mo, loop.da.T, loop.N), _HourBlock(bid_mo, loop.rt.T, loop.N)
        tracker_rows = []

        def bids_of(curve, count, offer, first_hour):
            if loop.stochastic:
                bids = curve_bids(curve, count, first_hour, gen, p_min)
            else:                                      # the deterministic loop offers its power output at no price: one point per hour
                bids = curve_bids(np.stack([np.round(offer * 100.0), np.zeros_like(offer)], 1)[:, None, :].astype(np.int64), np.ones(len(offer), int),
                                  first_hour, gen, p_min)
            return bids

        def model_rows(blk, clock, x, d, k, market):
            """the bidding model object's detail rows of the scenarios' solutions x [scenarios, n] (Bidder.record_bids' two routes)"""
            if x.shape[0] > 1:
                bid_mo.record_results_many(blk.at(clock, x), list(range(x.shape[0])), date=date(d), hour=k, Market=market)
            else:
                bid_mo.record_results(blk.at(clock, x[0]), date=date(d), hour=k, Scenario=0, Market=market)

        def day_ahead(d):
            if d >= D:
                return
            if not loop.parametrized:
                model_rows(da_blk, 24 * d, rec["da_x"][d, q], d, 0, "Day-ahead")
            bids = bids_of(rec["da_curve"][d, q] if loop.stochastic else None, rec["da_count"][d, q] if loop.stochastic else None, rec["da_offer"][d, q], 0)
            layout._record_bids(book, bids, date(d), 0, Market="Day-ahead")

        for h in range(H):
            d, k = divmod(h, 24)
            if k == 0:
                day_ahead(d)
            if not loop.parametrized:
                model_rows(rt_blk, h, rec["rt_x"][h, q], d, k, "Real-time")
            if loop.stochastic:
                dispatch = rec["rt_dispatch"][h, q]
                bids = bids_of(rec["rt_curve"][h, q], rec["rt_count"][h, q], None, k)
            else:                                      # the stub market of the deterministic loop: the real-time offer IS the dispatch
                dispatch = rt_blk.at(h, rec["rt_x"][h, q, 0]).family_values(bid_mo.power_output)[:Tc]
                bids = bids_of(None, None, dispatch, k)
            layout._record_bids(book, bids, date(d), k, Market="Real-time")
            blk = tr_blk.at(h, rec["tr_x"][h, q])
            tr_mo.record_results(blk, date=date(d), hour=k)
            P_T = blk.expressions[tr_mo.power_output]
            under, over = (loop.tracker_template.model.power_underdelivered, loop.tracker_template.model.power_overdelivered)
            tracker_rows += Tracker.detail_rows(date(d), k, [float(dispatch[t]) - tr_const[t] for t in range(Tc)], tr_const,
                                                [blk.value(P_T[t]) for t in range(Tc)], [blk.solution[under[t].index] for t in range(Tc)],
                                                [blk.solution[over[t].index] for t in range(Tc)])
        frames = [f() if callable(f) else f for f in book.bids_result_list]
        pd.concat(frames).to_csv(os.path.join(out, "bidder_detail.csv"), index=False)
        if not loop.parametrized:
            bid_mo.write_results(path=os.path.join(out, "bidding_model_detail.csv"))
        pd.DataFrame(tracker_rows).to_csv(os.path.join(out, "tracker_detail.csv"), index=False)
        tr_mo.write_results(path=os.path.join(out, "tracking_model_detail.csv"))
