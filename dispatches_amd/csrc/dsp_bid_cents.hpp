// dsp_bid_cents.hpp — the exact decimal rounding and the composite sort key of the bid curves, shared by dsp_bids.hip (one curve per
// hour over thousands of scenarios) and dsp_market.hip (one curve per plant and period over <= 16 scenarios).
#pragma once
#include <hip/hip_runtime.h>

namespace dsp {

constexpr long long kBidDrop = 0x7fffffffffffffffll;        // key of a pair that takes no part: sorts behind every real key
constexpr long long kBidOff = 1ll << 31;

// round(a, 2) * 100 as an integer, for finite |a| < 2e7 (anything else: 0, and the caller drops the pair).
__device__ __forceinline__ long long bid_cents(double a) {
#pragma clang fp contract(off)
  const double p = a * 200.0;                      // rounded product
  const double c = a * 134217729.0;                // Veltkamp split (2^27 + 1)
  const double hi = c - (c - a);
  const double lo = a - hi;
  const double err = (hi * 200.0 - p) + lo * 200.0;   // exact: a * 200 = p + err
  double r = floor(a * 100.0);                     // the exact floor is r or r +- 1
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (((p - 2.0 * r) + err) < 0.0) r -= 1.0;
    if (((p - (2.0 * r + 2.0)) + err) >= 0.0) r += 1.0;
  }
  const double d = (p - (2.0 * r + 1.0)) + err;    // sign of a * 100 - (r + 1/2), exact
  const bool odd = fmod(r, 2.0) != 0.0;
  if (d > 0.0 || (d == 0.0 && odd)) r += 1.0;      // above the midpoint, or on it with an odd floor: ties to even
  const bool ok = (fabs(a) < 2.0e7);               // false for NaN / inf too
  return ok ? (long long)r : 0ll;
}

// (power cents, price cents) as ONE signed 64-bit key: power ascending, price DESCENDING inside a power (low half in [0, 2^32))
__device__ __forceinline__ long long bid_key(long long pc, long long cc) { return pc * 4294967296ll + ((kBidOff - 1) - cc); }
__device__ __forceinline__ long long bid_key_power(long long key) { return key >> 32; }
__device__ __forceinline__ long long bid_key_price(long long key) { return (kBidOff - 1) - (key & 0xffffffffll); }

}  // namespace dsp
