"""Representative days of a double-loop sweep: day points, k-means, dispatch frequencies - the second label of the reference's market
surrogates (annual revenue is the first), computed where the sweep's data already sits.

The reference's workflow downstream of its double-loop sweeps is dispatches/workflow/train_market_surrogates/dynamic/:
Simulation_Data.py:305-366 scales every simulated year's hourly dispatch to a capacity factor, Time_Series_Clustering.py:226-385 cuts it
into days, sets aside all-zero and all-full days and clusters the rest into K representative days (tslearn TimeSeriesKMeans, euclidean,
max_iter=50, tol=1e-6, k-means++; one channel of 24 values for the nuclear case, dispatch and the day's wind capacity factor - 48 values -
for wind + PEM), and Train_NN_Surrogates.py:208-320 labels every simulation with its dispatch frequency [ws0, f_0 .. f_{K-1}, ws1]: the
share of zero days, of days nearest to each centre, and of full days.  The surrogates' training itself (Keras) is out of scope here.

BatchedDoubleLoop(profiles=days) keeps every plant's delivered power, `profile` [days + 1, 24, B], plant-minor.  A POINT is one (day,
plant) pair, p = day * B + b, with F = 24 * channels features; its arithmetic is written down so that numpy restates the kernels bit for
bit - every operation rounded on its own, nothing contracted into an fma:

    scaling     cf[h] = (profile[day, h, b] - p_min[b]) / (p_max[b] - p_min[b])      (Simulation_Data.py:351; :363 with p_min = 0)
    channel 2   w[h]  = cf_series[(start[b] + 24 * day + h) % N], the realised window, computed on the fly
    class       with filter_days: s = ((cf[0] + cf[1]) + ...) + cf[23], Python's sum; s == 0.0 a zero day (label -1), s == 24.0 a full
                day (label -2)
    distance    for k in order: acc = 0; for j in order: d = x[j] - c[k][j]; acc = acc + d * d.  The label is the first k with the
                smallest acc (strict <): cdist(...).argmin without the monotone square root.  A zero or full day gets dist2 = 0.
    update      centre k = sum of its members / their number; the points of chunk q = [1024 q, 1024 (q + 1)) are added in the order of p,
                then the chunks in the order of q.  A cluster without a member KEEPS its centre - our choice: tslearn re-initialises
                such a run instead.  inertia = sum(dist2 of labelled points) / their number.
    frequency   freq[b] = [#zero days, #days at centre 0 .. K - 1, #full days] / days  ([B, K] without the filter, the reference's
                filter_opt=False branch).

The functions `points`, `classify`, `assign`, `update`, `frequency`, `lloyd` below are that statement in numpy: the specification the
kernels of csrc/dsp_days.hip are tested against, and what DayPoints runs for a loop on the CPU stand-in or with use_fused=False.  With the
kernels, DayPoints calls dsp_days_assign / dsp_days_update / dsp_days_frequency (include/dsp_hip.h) on the loop's own buffers.

fit() is Lloyd's iteration with tslearn's stopping rule.  It does NOT claim tslearn's centres for a seed: tslearn is not a dependency
here, its k-means++ draws candidates in an order of its own, and it handles empty clusters differently.  Given the same centres,
assignment and frequencies are the reference's (tests/test_representative_days_cpu.py restates _generate_label_data independently)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

CHUNK = 1024                                  # DSP_DAYS_CHUNK of include/dsp_hip.h
MAX_K = 64                                    # DSP_DAYS_MAX_K
Fit = namedtuple("Fit", "centers labels inertia n_iter")


# ---- the numpy statement ------------------------------------------------------------------------------------------------------------------
def points(profile, p_min, p_max, channels=1, cf_series=None, start=None):
    """profile [D, 24, B] MW, p_min / p_max [B] -> X [D * B, 24 * channels], point p = d * B + b"""
    profile = np.asarray(profile, np.float64)
    D, _, B = profile.shape
    cf = (profile - np.asarray(p_min, np.float64)) / (np.asarray(p_max, np.float64) - np.asarray(p_min, np.float64))
    X = cf.transpose(0, 2, 1).reshape(D * B, 24)
    if channels == 2:
        cf_series, start = np.asarray(cf_series, np.float64), np.asarray(start, np.int64)
        at = (start[None, :, None] + 24 * np.arange(D)[:, None, None] + np.arange(24)[None, None, :]) % len(cf_series)
        X = np.concatenate([X, cf_series[at].reshape(D * B, 24)], axis=1)
    return np.ascontiguousarray(X)


def classify(X):
    """-> int32 [P]: -1 a zero day, -2 a full day, 0 a day to cluster; the sum runs in hour order over the first 24 features"""
    s = X[:, 0].copy()
    for h in range(1, 24):
        s = s + X[:, h]
    return np.where(s == 0.0, -1, np.where(s == 24.0, -2, 0)).astype(np.int32)


def assign(X, centers, filter_days=True):
    """-> (label int32 [P], dist2 [P])"""
    centers = np.asarray(centers, np.float64)
    P = X.shape[0]
    label, best = np.zeros(P, np.int32), np.zeros(P)
    for k in range(centers.shape[0]):
        acc = np.zeros(P)
        for j in range(X.shape[1]):
            d = X[:, j] - centers[k, j]
            acc = acc + d * d
        if k == 0:
            best = acc
        else:
            closer = acc < best
            best, label = np.where(closer, acc, best), np.where(closer, np.int32(k), label)
    if filter_days:
        cls = classify(X)
        label, best = np.where(cls < 0, cls, label), np.where(cls < 0, 0.0, best)
    return label.astype(np.int32), best


def update(X, label, dist2, centers):
    """-> (new centres [K, F], count int64 [K], inertia): chunked sums in the kernels' order (module docstring)"""
    centers = np.asarray(centers, np.float64)
    (P, F), K = X.shape, centers.shape[0]
    chunks = (P + CHUNK - 1) // CHUNK
    keep = np.flatnonzero((label >= 0) & (label < K))
    q, lab = keep // CHUNK, label[keep].astype(np.int64)
    part, cnt = np.zeros((chunks, K, F)), np.zeros((chunks, K))
    d2, n_lab = np.zeros(chunks), np.zeros(chunks)
    np.add.at(part, (q, lab), X[keep])                 # unbuffered: in the order of p
    np.add.at(cnt, (q, lab), 1.0)
    np.add.at(d2, q, dist2[keep])
    np.add.at(n_lab, q, 1.0)
    total, n, d2_total, n_total = np.zeros((K, F)), np.zeros(K), 0.0, 0.0
    for c in range(chunks):                            # the chunks in the order of q
        total, n, d2_total, n_total = total + part[c], n + cnt[c], d2_total + d2[c], n_total + n_lab[c]
    with np.errstate(invalid="ignore", divide="ignore"):
        new = np.where(n[:, None] > 0, total / n[:, None], centers)
    return new, n.astype(np.int64), float(d2_total / n_total) if n_total > 0 else 0.0


def frequency(label, K, filter_days=True):
    """label [D, B] -> [B, K + 2] = [zero, f_0 .. f_{K-1}, full] / D  ([B, K] without the filter)"""
    label = np.asarray(label)
    D = label.shape[0]
    slots = ([-1] if filter_days else []) + list(range(K)) + ([-2] if filter_days else [])
    return np.stack([(label == s).sum(0) for s in slots], axis=1) / float(D)


def lloyd(step_assign, step_update, centers, max_iter=50, tol=1e-6):
    """Lloyd's iteration under tslearn's rule (TimeSeriesKMeans._fit_one_init): assign, update, stop once |inertia_prev - inertia| < tol or
    at max_iter.  step_assign(centers) -> (label, dist2); step_update(label, dist2, centers) -> (centres, count, inertia).
    -> (centres, inertia, n_iter)"""
    previous, inertia, n_iter = None, 0.0, 0
    for it in range(int(max_iter)):
        label, dist2 = step_assign(centers)
        centers, _, inertia = step_update(label, dist2, centers)
        inertia, n_iter = float(inertia), it + 1
        if previous is not None and abs(previous - inertia) < tol:
            break
        previous = inertia
    return centers, inertia, n_iter


# ---- the host API -------------------------------------------------------------------------------------------------------------------------
def _scaling_range(loop, p_min, p_max):
    """the defaults of the module docstring's scaling, per plant, and their checks"""
    B = loop.B
    mo = loop.bidder.bidding_model_object if loop.bidder is not None else None
    if mo is None:
        if p_min is None or p_max is None:
            raise ValueError("profiles outside a loop carry no plant sizes: give p_min and p_max")
        lo_default = hi_default = None
    elif loop.flowsheet == "nuclear":
        from .flowsheets import parameters as prm
        top = float(mo.model_data.p_max)                                   # Simulation_Data._read_NE_pmin: p_min = p_max - PEM size
        pem = loop.pem_mw if loop.nuclear_sized else float(prm.nuclear_pem_capacity_mw)
        lo_default, hi_default = top - np.broadcast_to(np.asarray(pem, np.float64), (B,)), np.full(B, top)
    else:
        wind = getattr(loop, "wind_mw", None)
        wind = float(mo._wind_pmax_mw) if wind is None else wind
        lo_default, hi_default = np.zeros(B), np.broadcast_to(np.asarray(wind, np.float64), (B,))
    lo = lo_default if p_min is None else np.broadcast_to(np.asarray(p_min, np.float64), (B,))
    hi = hi_default if p_max is None else np.broadcast_to(np.asarray(p_max, np.float64), (B,))
    lo, hi = np.array(lo, np.float64), np.array(hi, np.float64)          # (own, writable copies)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("p_min and p_max must be finite")
    if (hi <= lo).any():
        raise ValueError("p_max must be greater than p_min for every plant")
    return lo, hi


class Profiles:
    """A profile buffer outside a loop, in the place of DayPoints' `loop` (tools and the kernels' tests: any year of hourly dispatch, from
    wherever it comes, can be clustered).  profile: torch float64 [days, 24, B], plant-minor, MW; cf_series [N] / start int64 [B]: the
    second channel's series and every plant's first hour in it.  On a GPU tensor the kernels run, on a CPU tensor the numpy statement;
    p_min and p_max have no defaults here."""
    flowsheet, bidder, nuclear_sized = "profiles", None, False

    def __init__(self, profile, cf_series=None, start=None, kernels=None):
        import torch
        if profile.dim() != 3 or profile.shape[1] != 24 or profile.dtype != torch.float64 or not profile.is_contiguous():
            raise ValueError("profile is a contiguous float64 tensor [days, 24, B]")
        self.profile, self.B, self.dev = profile, profile.shape[2], profile.device
        self._profile_days = profile.shape[0]
        self.hour = 24 * profile.shape[0]
        self.cf_series, self.start, self.N = cf_series, start, 0 if cf_series is None else cf_series.shape[0]
        if cf_series is not None and (start is None or start.dtype != torch.int64 or start.shape != (self.B,) or cf_series.dtype != torch.float64):
            raise ValueError("a second channel needs cf_series float64 [N] and start int64 [B]")
        self.use_fused = profile.is_cuda if kernels is None else bool(kernels)
        if self.use_fused:
            from .hip_solver import load_library
            self._lib = load_library()

    def _call(self, fn, *args):
        import ctypes as C
        import torch
        rc = fn(*args, C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        if rc != 0:
            raise RuntimeError(f"{fn.__name__} failed ({rc})")


class DayPoints:
    """The day points over a loop's profile (module docstring).  loop: a BatchedDoubleLoop built with profiles=days; the points are its
    whole days run so far.  channels: 1 (dispatch) or 2 (dispatch, then the day's realised capacity factors: wind flowsheets only).
    filter_days: zero and full days are set aside (labels -1 / -2) - the reference's filter_opt.  p_min, p_max [B] or scalars, MW: the
    scaling range; defaults: wind + PEM and wind + battery 0 .. the plant's own wind_mw (for wind + battery our choice: a discharging
    battery may push a capacity factor above 1, as in the reference's FE case), nuclear p_max - pem_mw .. p_max per plant
    (Simulation_Data._read_NE_pmin).  Refused (ValueError): a loop without profiles, channels outside 1 .. 2 or a second channel without
    a capacity-factor series, p_max <= p_min, non-finite values.  With the loop's kernels (use_fused) everything runs on the device;
    otherwise the numpy statement of this module - the same bits."""

    def __init__(self, loop, channels=1, filter_days=True, p_min=None, p_max=None):
        import torch
        if getattr(loop, "_profile_days", None) is None:
            raise ValueError("DayPoints needs a loop that keeps profiles: construct it with profiles=days")
        if channels not in (1, 2):
            raise ValueError(f"channels is 1 or 2, not {channels!r}")
        if channels == 2 and loop.cf_series is None:
            raise ValueError(f"channels=2 needs a capacity-factor series: the {loop.flowsheet!r} flowsheet has none")
        self.loop, self.B, self.channels, self.F, self.filter_days = loop, loop.B, int(channels), 24 * int(channels), bool(filter_days)
        self.p_min, self.p_max = _scaling_range(loop, p_min, p_max)
        self.kernels = bool(loop.use_fused)
        self.dev = loop.dev
        if self.kernels:
            from .hip_solver import DspDaysDesc
            self._p_min_t, self._p_max_t = torch.as_tensor(self.p_min, device=self.dev), torch.as_tensor(self.p_max, device=self.dev)
            d = DspDaysDesc()
            d.B, d.channels, d.filter = self.B, self.channels, int(self.filter_days)
            d.profile, d.p_min, d.p_max = loop.profile.data_ptr(), self._p_min_t.data_ptr(), self._p_max_t.data_ptr()
            if self.channels == 2:
                d.cf_series, d.start, d.N = loop.cf_series.data_ptr(), loop.start.data_ptr(), loop.N
            self._desc = d

    # -- pieces ---------------------------------------------------------------------------------------------------------------------------
    @property
    def days(self):
        """whole days run so far, at most the profile's span"""
        return min(self.loop.hour // 24, self.loop._profile_days)

    def _described(self):
        D = self.days
        if D < 1:
            raise RuntimeError("no whole day has been run yet")
        self._desc.days = D
        return self._desc, D

    def points(self):
        """-> numpy [days * B, F], the numpy statement on the profile read back (what the CPU paths work on)"""
        D = self.days
        if D < 1:
            raise RuntimeError("no whole day has been run yet")
        two = self.channels == 2
        return points(self.loop.profile[:D].cpu().numpy(), self.p_min, self.p_max, self.channels,
                      self.loop.cf_series.cpu().numpy() if two else None, self.loop.start.cpu().numpy() if two else None)

    def _centers(self, centers):
        c = np.ascontiguousarray(centers.cpu().numpy() if hasattr(centers, "cpu") else centers, np.float64)
        if c.ndim != 2 or c.shape[1] != self.F or not 1 <= c.shape[0] <= MAX_K:
            raise ValueError(f"centres are [K, {self.F}] with 1 <= K <= {MAX_K}, not {list(c.shape)}")
        return c

    def _ptr(self, t):
        import ctypes as C
        return C.c_void_p(t.data_ptr())

    def assign(self, centers):
        """-> (label int32 [days, B], dist2 float64 [days, B]) on the loop's device"""
        import torch
        c = self._centers(centers)
        if not self.kernels:
            label, dist2 = assign(self.points(), c, self.filter_days)
            D = self.days
            return torch.as_tensor(label.reshape(D, self.B), device=self.dev), torch.as_tensor(dist2.reshape(D, self.B), device=self.dev)
        import ctypes as C
        desc, D = self._described()
        c_t = torch.as_tensor(c, device=self.dev)
        label = torch.empty((D, self.B), dtype=torch.int32, device=self.dev)
        dist2 = torch.empty((D, self.B), dtype=torch.float64, device=self.dev)
        self.loop._call(self.loop._lib.dsp_days_assign, C.byref(desc), self._ptr(c_t), c.shape[0], self._ptr(label), self._ptr(dist2))
        return label, dist2

    def update(self, label, dist2, centers):
        """-> (new centres numpy [K, F], count numpy int64 [K], inertia float): the means of the members, an empty cluster keeps its centre"""
        import torch
        c = self._centers(centers)
        if not self.kernels:
            return update(self.points(), label.cpu().numpy().reshape(-1), dist2.cpu().numpy().reshape(-1), c)
        import ctypes as C
        desc, D = self._described()
        K = c.shape[0]
        c_t = torch.as_tensor(c, device=self.dev).clone()
        count, inertia = torch.zeros(K, dtype=torch.int64, device=self.dev), torch.zeros((), dtype=torch.float64, device=self.dev)
        n_work = self.loop._lib.dsp_days_work_doubles(D * self.B, K, self.channels)
        work = torch.empty(n_work, dtype=torch.float64, device=self.dev)
        label, dist2 = label.contiguous(), dist2.contiguous()
        if label.dtype != torch.int32 or dist2.dtype != torch.float64 or label.numel() != D * self.B or dist2.numel() != D * self.B:
            raise ValueError(f"label is int32 and dist2 float64, both [{D}, {self.B}]")
        self.loop._call(self.loop._lib.dsp_days_update, C.byref(desc), self._ptr(label), self._ptr(dist2), K, self._ptr(c_t), self._ptr(count),
                        self._ptr(inertia), self._ptr(work), n_work)
        return c_t.cpu().numpy(), count.cpu().numpy(), float(inertia.item())

    def label_frequency(self, label, K):
        """label [days, B] -> freq [B, K + 2] (filter_days) or [B, K] on the loop's device"""
        import torch
        if not self.kernels:
            return torch.as_tensor(frequency(label.cpu().numpy(), K, self.filter_days), device=self.dev)
        import ctypes as C
        desc, D = self._described()
        label = label.contiguous()
        if label.dtype != torch.int32 or label.numel() != D * self.B or not 1 <= K <= MAX_K:
            raise ValueError(f"label is int32 [{D}, {self.B}] and 1 <= K <= {MAX_K}")
        freq = torch.empty((self.B, K + 2 if self.filter_days else K), dtype=torch.float64, device=self.dev)
        self.loop._call(self.loop._lib.dsp_days_frequency, C.byref(desc), self._ptr(label), K, self._ptr(freq))
        return freq

    def frequency(self, centers):
        """-> the dispatch frequency of every plant under these centres, [B, K + 2] = [zero, f_0 .. f_{K-1}, full] / days"""
        c = self._centers(centers)
        return self.label_frequency(self.assign(c)[0], c.shape[0])

    def point(self, p):
        """the features of point p = day * B + b -> numpy [F]"""
        d, b = divmod(int(p), self.B)
        two = self.channels == 2
        return points(self.loop.profile[d:d + 1, :, b:b + 1].cpu().numpy(), self.p_min[b:b + 1], self.p_max[b:b + 1], self.channels,
                      self.loop.cf_series.cpu().numpy() if two else None,
                      (self.loop.start[b:b + 1].cpu().numpy() + 24 * d) if two else None)[0]

    # -- k-means ---------------------------------------------------------------------------------------------------------------------------
    def _seed_centers(self, K, seed):
        """k-means++: the first centre uniformly among the days to cluster, every next one with probability proportional to the squared
        distance to the nearest centre so far (dsp_days_assign's dist2; zero and full days carry 0 and are never drawn).  The draws are
        made on the host from numpy.random.RandomState(seed)."""
        rs = np.random.RandomState(seed)
        label, _ = self.assign(np.zeros((1, self.F)))
        candidates = np.flatnonzero(label.cpu().numpy().reshape(-1) >= 0)
        if len(candidates) == 0:
            raise ValueError("no day left to cluster: every day is a zero or a full day")
        centers = [self.point(candidates[rs.randint(len(candidates))])]
        while len(centers) < K:
            cum = np.cumsum(self.assign(np.stack(centers))[1].cpu().numpy().reshape(-1))
            if cum[-1] > 0:
                pick = min(int(np.searchsorted(cum, rs.random_sample() * cum[-1], side="right")), len(cum) - 1)
            else:                                                          # every day sits on a centre already
                pick = candidates[rs.randint(len(candidates))]
            centers.append(self.point(pick))
        return np.stack(centers)

    def fit(self, K, seed=42, max_iter=50, tol=1e-6, init="k-means++"):
        """K representative days of the loop's points by Lloyd's iteration from the two kernels (module docstring: `lloyd`).
        init: "k-means++" (seeded, _seed_centers) or a [K, F] array.  -> Fit(centers numpy [K, F], labels int32 [days, B] on the device -
        the assignment under the returned centres -, inertia, n_iter).  Not tslearn's centres for a seed (module docstring)."""
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= MAX_K:
            raise ValueError(f"K is an integer in 1 .. {MAX_K}, not {K!r}")
        if isinstance(init, str):
            if init != "k-means++":
                raise ValueError(f"init is 'k-means++' or a [K, {self.F}] array, not {init!r}")
            centers = self._seed_centers(int(K), seed)
        else:
            centers = self._centers(init)
            if centers.shape[0] != K:
                raise ValueError(f"init has {centers.shape[0]} centres, K = {K}")
        centers, inertia, n_iter = lloyd(self.assign, self.update, centers, max_iter, tol)
        return Fit(centers, self.assign(centers)[0], inertia, n_iter)
