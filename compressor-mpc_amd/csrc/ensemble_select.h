// Exact ensemble quantiles (cmpc_quantile_*, cmpc_score_quantiles,
// cmpc_envelope_*): the order-statistic arithmetic, shared by
// the host entry points (cmpc_abi.cpp) and the device kernels
// (ensemble_quantiles.hip).  Everything is integer counting on keys; the only
// floating-point operations are the rank's one product and the value rule.
//
//   key     a double's bits u as a uint64_t whose unsigned order is the total
//           order  -inf < negatives < -0 < +0 < positives < +inf < NaN:
//           sign clear: u | 2^63;  sign set: ~u;  every NaN: 2^64 - 1, which
//           decodes to the one quiet NaN 0x7ff8000000000000
//   rank    h = q (double)(B - 1) (one product), k_lo = floor(h), g = h - k_lo
//           (exact), k_hi = k_lo + 1 where g > 0, else k_lo
//   value   x_lo where x_lo == x_hi; else with d = x_hi - x_lo:
//           x_lo + d g for g < 0.5, x_hi - d (1 - g) otherwise (products and
//           sums separate: the tree builds with -ffp-contract=off)
//   select  MSB-first radix selection with 8-bit digits: given the counts of
//           the next digit among the keys that share a target's prefix, the
//           digit that holds the target's remaining rank, and the rank left
//           inside that digit (cmpc_select_narrow)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CMPC_SELECT_HD __host__ __device__
#else
#define CMPC_SELECT_HD
#endif

constexpr int kSelectDigits = 256, kSelectPasses = 8;
constexpr uint64_t kSelectNanKey = ~(uint64_t)0;

CMPC_SELECT_HD inline uint64_t cmpc_select_key(double v) {
  uint64_t u;
  __builtin_memcpy(&u, &v, sizeof u);
  if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return kSelectNanKey;
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

CMPC_SELECT_HD inline double cmpc_select_value_of(uint64_t key) {
  uint64_t u = key == kSelectNanKey ? 0x7ff8000000000000ull : (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  double v;
  __builtin_memcpy(&v, &u, sizeof v);
  return v;
}

// digit `pass` (0: the most significant) of a key, and the digits above it
CMPC_SELECT_HD inline uint32_t cmpc_select_digit(uint64_t key, int pass) {
  return (uint32_t)(key >> (56 - 8 * pass)) & 255u;
}
CMPC_SELECT_HD inline uint64_t cmpc_select_prefix(uint64_t key, int pass) {
  return pass ? key >> (64 - 8 * pass) : 0;
}

// the ranks of level q among B values (q inside [0, 1], B >= 1)
CMPC_SELECT_HD inline void cmpc_select_rank(int B, double q, uint32_t* k_lo, uint32_t* k_hi, double* g) {
  const double h = q * (double)(B - 1);
  uint32_t lo = (uint32_t)h;  // h >= 0: the floor
  if (lo > (uint32_t)(B - 1)) lo = (uint32_t)(B - 1);
  const double frac = h - (double)lo;
  *k_lo = lo;
  *k_hi = frac > 0.0 && lo + 1 < (uint32_t)B ? lo + 1 : lo;
  *g = frac;
}

CMPC_SELECT_HD inline double cmpc_select_interpolate(double x_lo, double x_hi, double g) {
  if (x_lo == x_hi) return x_lo;
  const double d = x_hi - x_lo;
  if (g < 0.5) {
    const double t = d * g;
    return x_lo + t;
  }
  const double t = d * (1.0 - g);
  return x_hi - t;
}

// counts[0..255]: the keys with the target's prefix, by their next digit;
// rank: the target's position among those keys.  Returns the digit that holds
// it and leaves the position inside that digit in *rank.  (rank below the
// counts' total, which holds for a rank below B.)
CMPC_SELECT_HD inline uint32_t cmpc_select_narrow(const uint32_t* counts, uint32_t* rank) {
  uint32_t r = *rank, d = 0;
  while (d < (uint32_t)kSelectDigits - 1 && r >= counts[d]) {
    r -= counts[d];
    ++d;
  }
  *rank = r;
  return d;
}

// x_hi from the last pass's results: position k_hi holds key_lo again while
// k_hi is below the number of keys <= key_lo, and the smallest key above it
// otherwise
CMPC_SELECT_HD inline uint64_t cmpc_select_key_hi(uint64_t key_lo, uint32_t k_hi, uint32_t n_le, uint64_t next) {
  return k_hi < n_le ? key_lo : next;
}

// The host form of the whole selection for one row of B values x[b * stride]:
// per level l, out[3 l] = x_lo, out[3 l + 1] = x_hi, out[3 l + 2] = the lowest
// b whose key is x_lo's.  The same passes the kernels make, on one histogram.
inline void cmpc_select_row_host(const double* x, size_t stride, int B, int n_levels, const uint32_t* k_lo,
                                 const uint32_t* k_hi, double* out) {
  for (int l = 0; l < n_levels; ++l) {
    uint64_t prefix = 0;
    uint32_t rank = k_lo[l];
    for (int pass = 0; pass < kSelectPasses; ++pass) {
      uint32_t counts[kSelectDigits] = {};
      for (int b = 0; b < B; ++b) {
        const uint64_t key = cmpc_select_key(x[(size_t)b * stride]);
        if (cmpc_select_prefix(key, pass) == prefix) counts[cmpc_select_digit(key, pass)]++;
      }
      prefix = (prefix << 8) | cmpc_select_narrow(counts, &rank);
    }
    uint32_t n_le = 0;
    int32_t arg = INT32_MAX;
    uint64_t next = kSelectNanKey;
    for (int b = 0; b < B; ++b) {
      const uint64_t key = cmpc_select_key(x[(size_t)b * stride]);
      if (key <= prefix) {
        ++n_le;
        if (key == prefix && b < arg) arg = b;
      } else if (key < next) {
        next = key;
      }
    }
    out[3 * l] = cmpc_select_value_of(prefix);
    out[3 * l + 1] = cmpc_select_value_of(cmpc_select_key_hi(prefix, k_hi[l], n_le, next));
    out[3 * l + 2] = (double)arg;
  }
}
