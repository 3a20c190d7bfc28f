"""What the two device double loops share on the host (BatchedWindBatteryDoubleLoop, rolling.py; BatchedDoubleLoop, rolling_flowsheets.py):
the solver attachment of a device model, the market arguments' validation, price windows and backcast scenarios read at the device clock,
bid curves / clearing / their storage, the day's sums, the C ABI call, and the capture-and-replay of a step.  Everything here is written
for the general case - clock `self._clk`, a history lag, curves from p_min, padded curve slots - of which the wind + battery loop is the
special one: its clock is hour_t, it has no lag, p_min = 0 and S + 1 slots.  The kernels and structs stay each loop's own."""
from __future__ import annotations

from .hip_solver import DeviceLP, default_options


class _NoSolver:
    def solve(self, *a, **k):
        raise RuntimeError("template model: never solved on the host")


def attach_solver(m, B, dev, device_index, extra_options, lp_backend, solved=True, simplex_certify=False):
    """m.opts / opts_warm / opts_first, m.dlp and m.out of a device model m (m.lp, m.T set) with B rows.
    recertify: the loop never reads a flag back between solves (its days are hipGraph replays), so a solve accepted without a certified
    objective accuracy is re-solved on the device under other settings (dsp_options::recertify_passes) - three passes for a day-ahead LP,
    which the PDLP kernel solves.  The hourly LPs (T <= 16) get neither that nor an infeasibility test: they carry slack columns (always
    feasible - and the simplex reports an infeasible input itself), a first-order fallback has not been needed once, and should one ever
    come back flagged, the loop's `uncertified` count says so.  They share one matrix from hour to hour: the simplex starts hour k from
    hour k - 1's final basis (dsp_options::simplex_warm = 1: 2 - 4 pivots instead of ~26) and from the slack basis in the first hour
    of every day (= 2).  The output buffers have fixed addresses from the start: the fused kernels and the hipGraphs hold pointers.
    simplex_certify: the hourly LPs (T <= 16) are solved under dsp_options::simplex_certify = 1 - the simplex stores status 0 only for a pair
    (x, y) that passed the full KKT certificate against the original LP and flags it DSP_FLAG_SIMPLEX_KKT; what it rejects reaches the PDLP
    pass, whose status and flags feed `bad` / `uncertified` as ever.  m.out then carries the certificates, kkt [B, 4].
    lp_backend: tests pass a stand-in with DeviceLP.solve's signature (CPU tensors + HiGHS); solved=False: a template never solved."""
    import torch
    if lp_backend is not None:
        m.opts, m.dlp, m.out = None, lp_backend(m.lp), None
        return
    from .hip_solver import DspOptions
    extra = {"recertify_passes": 3} if m.T > 16 else {"recertify_passes": 0, "eps_infeasible": 0.0}
    if simplex_certify and m.T <= 16:
        extra["simplex_certify"] = 1
    m.opts = default_options(**{**extra, **(extra_options or {})})
    m.opts_warm, m.opts_first = DspOptions.from_buffer_copy(m.opts), DspOptions.from_buffer_copy(m.opts)
    if m.T <= 16:
        m.opts_warm.simplex_warm, m.opts_first.simplex_warm = 1, 2
    m.dlp = DeviceLP(m.lp, device_index, m.opts) if solved else None
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    i32 = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
    m.out = dict(x=f64(B, m.lp.n), y=f64(B, max(m.lp.m, 1)), obj=f64(B), status=i32(), iters=i32(), jumps=i32(), flags=i32())
    if m.opts.simplex_certify == 1:
        m.out["kkt"] = torch.full((B, 4), float("nan"), dtype=torch.float64, device=dev)


class _DeviceLoop:
    """Base of the two loops.  A subclass provides B, S, D, N, dev, forecaster, market, start, _clk (the device clock a step reads),
    da_offer, da_curve / da_count, da_energy_mwh / offered_mwh, _hundred, bad, uncertified, use_graphs, _graphs, day_ahead(), hour_step()."""

    _warm = False          # the first day runs eagerly (handles, output buffers and kernels get created), then graphs

    @staticmethod
    def _check_market_arguments(forecaster, market, S, D):
        if forecaster not in ("perfect", "backcast") or market not in ("stub", "price_taker"):
            raise ValueError(f"forecaster is 'perfect' or 'backcast' and market 'stub' or 'price_taker', not {forecaster!r} / {market!r}")
        if forecaster == "backcast" and not 1 <= S <= min(16, D):
            raise ValueError(f"forecaster='backcast' needs 1 <= n_price_scenarios <= min(16, max_historical_days), not {S} (max_historical_days={D})")
        if forecaster == "perfect" and S != 1:
            raise ValueError("forecaster='perfect' knows one price scenario: n_price_scenarios must be 1")

    def _call(self, fn, *args):
        """one C ABI call on the current stream"""
        import ctypes as C
        import torch
        rc = fn(*args, C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        if rc != 0:
            raise RuntimeError(f"{fn.__name__} failed ({rc})")

    # -- windows (capturable: the clock is read on the device) ----------------------------------------------------------------------------
    def _window(self, series, T, offset=0):
        """[B, T] window of `series` that starts `offset` hours after the current hour of every plant"""
        import torch
        clock = self._clk + offset if offset else self._clk
        return series[(self.start[:, None] + clock + torch.arange(T, device=self.dev)[None, :]) % self.N]

    def _forecast(self, series, T, hod, lag_days=0):
        """[B, S, T] price scenarios asked at hour-of-day `hod` of the current day.  Backcast: exactly Backcaster._forecast over the D
        whole days before the current day of every plant's own circular series - pos = (24 (D - 1 - i) + hod + t) mod 24 D into that
        history, i.e. series[(start + 24 (d - D) + pos) mod N].  lag_days: the history ends that many days earlier (the real-time prices
        of a bid made at the RUC hour)"""
        import torch
        if self.forecaster == "perfect":
            return self._window(series, T)[:, None, :]
        D = self.D
        d = torch.div(self._clk, 24, rounding_mode="floor")
        if lag_days:
            d = d - lag_days
        i, t = torch.arange(self.S, device=self.dev)[:, None], torch.arange(T, device=self.dev)[None, :]
        pos = (24 * (D - 1 - i) + hod + t) % (24 * D)
        return series[(self.start[:, None, None] + 24 * (d - D) + pos[None]) % self.N]

    def _rows(self, v, m=None):
        """per-plant values [B, ...] -> per-row [B * S, ...] (a plant's S rows are adjacent; m.per_plant: that model's rows per plant)"""
        per = self.S if m is None or m.per_plant is None else m.per_plant
        return v if per == 1 else v.repeat_interleave(per, dim=0)

    def _free_day_ahead_power(self, m, k=None, per=1):
        """day_ahead_power free in every row of bidding model m; k: hour k of the day - the `known` periods of the horizon inside the
        cleared day are fixed to the cleared offer instead (per: rows per plant)"""
        m.lb.index_fill_(1, m.pda_cols, 0.0)          # (index_fill_, not lb[:, cols] = 0.0: a Python scalar on the right-hand
        m.ub.index_fill_(1, m.pda_cols, float("inf"))  #  side becomes a host-to-device copy, which a graph capture refuses)
        if k is None:
            return
        known = min(m.T, 24 - k)
        rows = lambda v: v if per == 1 else v.repeat_interleave(per, dim=0)
        m.lb[:, m.pda_cols[:known]] = rows(self.da_offer[:, k:k + known])
        m.ub[:, m.pda_cols[:known]] = rows(self.da_offer[:, k:k + known])

    # -- bid curves, market clearing --------------------------------------------------------------------------------------------------------
    def _curves(self, power, price, status):
        """power, price [B, S, Tc]; status [B * S] -> (U, M [S + 1, B * Tc] int64 cents, count [B * Tc]) - workflow/market.py::plant_curves"""
        import torch
        from .workflow.market import plant_curves
        B, S, Tc = power.shape
        lanes = lambda a: a.expand(B, S, Tc).permute(1, 0, 2).reshape(S, B * Tc)
        p_min = getattr(self, "p_min_cents", 0)
        if getattr(self, "p_min_cents_plant", None) is not None:          # plants of different minimum power: lane (b, t) reads plant b's
            p_min = self.p_min_cents_plant.repeat_interleave(Tc)
        return plant_curves(torch, lanes(power), lanes(price), lanes((status == 0).reshape(B, S, 1)), p_min_cents=p_min)

    def _clear(self, U, M, count, lmp):
        import torch
        from .workflow.market import clear_curves
        return clear_curves(torch, U, M, count, lmp.reshape(-1), self._hundred, price_taker=self.market == "price_taker").reshape(lmp.shape)

    def _store_curves(self, curve, cnt, U, M, count):
        import torch
        B, Tc, slots, _ = curve.shape
        if U.shape[0] < slots:                        # (a self-schedule's one-pair curve in the loop's S + 1 slots: the rest stays 0)
            pad = torch.zeros((slots - U.shape[0], U.shape[1]), dtype=U.dtype, device=U.device)
            U, M = torch.cat([U, pad]), torch.cat([M, pad])
        curve.copy_(torch.stack([U.t().reshape(B, Tc, slots), M.t().reshape(B, Tc, slots)], dim=3))
        cnt.copy_(count.reshape(B, Tc))

    def _check(self, out):
        self.bad |= (out["status"] != 0).any()
        # accepted without a certified objective accuracy (DSP_FLAG_OBJ_WAIVED): counted, on the device (the loop is replayed
        # from hipGraphs: no host round trip to re-solve them here); results() reports the count next to `ok`
        if out.get("flags") is not None:
            self.uncertified += ((out["flags"] & 1) != 0).sum()

    def _account_day_ahead(self):
        """the day's sums of the bid that is current: cleared and offered day-ahead energy (ruc_hour: when the bid BECOMES current)"""
        import torch
        self.da_energy_mwh += self.da_offer.sum(1)
        last = torch.gather(self.da_curve[:, :, :, 0], 2, (self.da_count.to(torch.int64) - 1)[:, :, None])[:, :, 0]
        self.offered_mwh += (last.to(torch.float64) / self._hundred).sum(1)

    # -- one simulated day ----------------------------------------------------------------------------------------------------------------
    def _run(self, key, fn):
        """Run one step: eagerly, or - with use_graphs - captured once into a hipGraph and replayed from then on."""
        import torch
        if not self.use_graphs or not self._warm:
            fn()
            return
        g = self._graphs.get(key)
        if g is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            self._graphs[key] = g
        g.replay()

    def run_day(self):
        self.day_ahead()
        for _ in range(24):
            self.hour_step()
        self._warm = True
