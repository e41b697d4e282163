"""A numpy model of the exact ensemble quantiles (include/cmpc.h, DESIGN.md
§3.18), written from the specification and not from the library: the key map,
a full sort of the keys, the rank rule and the value rule.

  key    a double's bits u as a uint64 in the total order -inf < negatives < -0
         < +0 < positives < +inf < NaN: u | 2^63 with the sign clear, ~u with it
         set, every NaN 2^64 - 1 (back: the quiet NaN 0x7ff8000000000000)
  rank   h = q (B - 1) in float64, k_lo = floor(h), g = h - k_lo, k_hi = k_lo +
         1 where g > 0
  value  x_lo where x_lo == x_hi, else x_lo + d g for g < 0.5 and x_hi - d (1 -
         g) otherwise, d = x_hi - x_lo
"""
import numpy as np

TOP = np.uint64(1) << np.uint64(63)
NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
QUIET_NAN = np.uint64(0x7FF8000000000000)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def keys(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    u = x.view(np.uint64)
    k = np.where((u & TOP) != 0, ~u, u | TOP)
    return np.where(np.isnan(x), NAN_KEY, k)


def values(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    u = np.where((k & TOP) != 0, k & ~TOP, ~k)
    u = np.where(k == NAN_KEY, QUIET_NAN, u)
    return np.ascontiguousarray(u).view(np.float64)


def rank(B, q):
    h = np.float64(q) * np.float64(B - 1)
    k_lo = int(np.floor(h))
    g = float(h - np.float64(k_lo))
    return k_lo, (k_lo + 1 if g > 0 else k_lo), g


def value(x_lo, x_hi, g):
    x_lo, x_hi = np.asarray(x_lo, dtype=np.float64), np.asarray(x_hi, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x_hi - x_lo
        v = np.where(g < 0.5, x_lo + d * g, x_hi - d * (1.0 - g))
    return np.where(x_lo == x_hi, x_lo, v)


def model(X, levels):
    """X (len, B, S): lo, hi, value (n_levels, len, S) float64 and arg (int64),
    the lowest b whose key is lo's, by a sort of the keys over axis 1."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, B, S = X.shape
    K = keys(X)
    Ks = np.sort(K, axis=1)
    out = {k: [] for k in ("lo", "hi", "arg", "value")}
    for q in levels:
        k_lo, k_hi, g = rank(B, q)
        key_lo = Ks[:, k_lo, :]
        lo, hi = values(key_lo), values(Ks[:, k_hi, :])
        out["lo"].append(lo)
        out["hi"].append(hi)
        out["arg"].append(np.argmax(K == key_lo[:, None, :], axis=1).astype(np.int64))   # (the first: the lowest)
        out["value"].append(value(lo, hi, g))
    return {k: np.stack(v) for k, v in out.items()}


def same(a, b):
    """Equal by value with NaN equal to NaN (the two zeros compare equal)."""
    return np.array_equal(a, b, equal_nan=True)
