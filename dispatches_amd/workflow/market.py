"""Price-taker clearing of a bid curve, and the per-plant curves of the stochastic double loop as tensor operations.

A bid curve is what `bid_curves.curves` leaves of an hour's (power, marginal price) pairs: powers `U_0 < U_1 < ...`, marginal prices
`M_0 <= M_1 <= ...`.  A cost-minimising market facing a price-taking unit with that curve (cost = the integral `curves` builds)
dispatches it at the largest breakpoint whose marginal price the LMP covers: `clear_price_taker`.  It is the statement the device kernel
(`csrc/dsp_market.hip`) and the tensor form below (`plant_curves` / `clear_curves`, used by `rolling.py`) are tested against.
"""
from __future__ import annotations

import numpy as np

from .bid_curves import _DROP, _KEY_OFF, cents


def clear_price_taker(U, M, lmp):
    """U, M: the points of ONE curve (powers ascending, marginal prices non-decreasing), lmp: the price that occurs.
    Dispatch = max{ U_j : M_j <= lmp }, U_0 if no j qualifies (ties in M go to the larger power).  Compared as doubles."""
    U, M = np.asarray(U, float), np.asarray(M, float)
    if len(U) == 0 or len(U) != len(M):
        raise ValueError("a curve has at least one point, and as many prices as powers")
    covered = M <= float(lmp)
    return float(U[covered].max()) if covered.any() else float(U[0])


def plant_curves(torch, power, price, ok, p_min_cents=0):
    """power, price: [S, L] float64 - the S scenarios' pairs of L independent (plant, period) lanes; ok [S, L] bool (False: the row's
    solve was not optimal, it offers nothing); p_min_cents: the generator's minimum power in integer cents (0 for the wind + battery
    plant, 40000 for the 400 MW nuclear unit), an int or - plants of different minimum - an int64 tensor [L], one per lane.  The arithmetic of `bid_curves.sorted_pairs` + `bid_curves.curves`, per lane: integer
    cents, pairs with power below p_min dropped, sorted by power ascending / price descending, the highest price per distinct power, the
    point (p_min, lowest price seen or 0) in front if no pair sits at p_min, running maximum over the prices.
    -> (U [S + 1, L], M [S + 1, L] int64 cents, unused slots 0; count [L])."""
    S, L = power.shape
    pc, cc = cents(torch, power), cents(torch, price)
    keep = (pc >= p_min_cents) & ok & torch.isfinite(power) & torch.isfinite(price)
    key = torch.where(keep, pc * (1 << 32) + ((_KEY_OFF - 1) - cc), torch.full_like(pc, _DROP))
    key, _ = torch.sort(key, dim=0)
    live = key != _DROP
    ps = key >> 32
    cs = (_KEY_OFF - 1) - (key & 0xFFFFFFFF)
    first = live.clone()
    first[1:] &= ps[1:] != ps[:-1]
    n = first.sum(dim=0)
    ins = ~(first & (ps == p_min_cents)).any(dim=0)                         # no point at p_min: one is inserted in front
    lowest = torch.where(first, cs, torch.full_like(cs, _DROP)).min(dim=0).values
    lowest = torch.where(n == 0, torch.zeros_like(lowest), lowest)
    dest = torch.where(first, torch.cumsum(first.to(torch.int64), dim=0) - 1 + ins.to(torch.int64), torch.full_like(ps, S + 1))
    U = torch.zeros((S + 2, L), dtype=torch.int64, device=power.device)     # (row S + 1 takes what is not a point)
    M = torch.zeros_like(U)
    U.scatter_(0, dest, ps)
    M.scatter_(0, dest, cs)
    U, M = U[:S + 1], M[:S + 1]
    U[0] = torch.where(ins, p_min_cents if torch.is_tensor(p_min_cents) else torch.full_like(U[0], p_min_cents), U[0])
    M[0] = torch.where(ins, lowest, M[0])
    count = n + ins.to(torch.int64)
    valid = torch.arange(S + 1, device=power.device)[:, None] < count[None, :]
    M = torch.cummax(torch.where(valid, M, torch.full_like(M, -_DROP)), dim=0).values
    zero = torch.zeros_like(U)
    return torch.where(valid, U, zero), torch.where(valid, M, zero), count


def clear_curves(torch, U, M, count, lmp, hundred, price_taker=True):
    """U, M, count of `plant_curves`; lmp [L] float64; hundred: a 0-d float64 tensor holding 100 (a tensor divisor: torch multiplies by
    the rounded reciprocal of a Python scalar on the GPU).  -> dispatch [L] float64: `clear_price_taker` per lane, or - stub market -
    the curve's last point."""
    if price_taker:
        valid = torch.arange(U.shape[0], device=U.device)[:, None] < count[None, :]
        covered = ((M.to(torch.float64) / hundred) <= lmp[None, :]) & valid
        j = torch.clamp(covered.sum(dim=0) - 1, min=0)                      # M is non-decreasing: the covered points are a prefix
    else:
        j = count - 1
    return U.gather(0, j[None, :])[0].to(torch.float64) / hundred
