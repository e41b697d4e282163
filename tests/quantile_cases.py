"""The data and the levels the quantile tests share (tests/test_quantiles.py on
the host, tests/test_gpu_quantiles.py on the device).  Every kind is a (len, B,
S) float64 array; FINITE are the kinds on which the interpolated value is
compared with numpy.quantile bit for bit (no infinity, no NaN, no -0)."""
import functools

import numpy as np

LEVELS = (0.0, 1.0, 0.5, 0.95, 0.05, 1.0 / 3.0, 0.999)
ALL8 = LEVELS + (0.25,)
# the single-level calls and the call with all eight
LEVEL_CALLS = tuple((q,) for q in LEVELS) + (ALL8,)

FINITE = ("normal", "ties", "equal", "spread", "subnormal", "lowbit", "topbits")
KINDS = FINITE + ("mixed",)


def _flip(x, mask):
    return (np.ascontiguousarray(x).view(np.uint64) ^ np.uint64(mask)).view(np.float64)


@functools.lru_cache(maxsize=None)
def cases(n, B, S):
    """{kind: (n, B, S) array}, read-only."""
    rng = np.random.default_rng(1000 * B + 10 * S + n)
    shape = (n, B, S)
    out = {}
    out["normal"] = rng.normal(size=shape)
    out["ties"] = rng.integers(0, 4, size=shape).astype(np.float64)              # heavy ties
    out["equal"] = np.full(shape, 7.25)
    out["spread"] = rng.normal(size=shape) * 10.0 ** rng.integers(-300, 301, size=shape)
    out["subnormal"] = (rng.integers(-2 ** 40, 2 ** 40, size=shape) * 5e-324).astype(np.float64)
    # neighbours that differ in the lowest mantissa bit only: the last digit pass decides
    base = rng.choice([1.5, -2.75, 1e10], size=(n, 1, S))
    low =np.broadcast_to(base, shape).copy()
    pick = rng.integers(0, 2, size=shape).astype(bool)
    low[pick] = _flip(low[pick], 1)
    out["lowbit"] = low
    # neighbours that differ in the sign or in the top exponent bit only: the first pass decides
    v = np.full(shape, 2.0 ** -511 * 1.25)                                        # exponent field 0x200
    top = v.copy()
    which = rng.integers(0, 4, size=shape)
    top[which == 1] = _flip(v[which == 1], 1 << 63)                               # the sign
    top[which == 2] = _flip(v[which == 2], 1 << 62)                               # 2^513 * 1.25
    top[which == 3] = _flip(v[which == 3], (1 << 63) | (1 << 62))
    out["topbits"] = top
    mixed = rng.normal(size=shape)
    special = np.array([np.inf, -np.inf, 0.0, -0.0, np.nan, -np.nan, 1.0], dtype=np.float64)
    nan_payload = _flip(np.array([np.nan]), 0x800000000000BEEF)[0]                # a negative NaN with a payload
    special = np.append(special, nan_payload)
    sel = rng.integers(0, 2 * special.size, size=shape)
    hit = sel < special.size
    mixed[hit] = special[sel[hit]]
    out["mixed"] = mixed
    for a in out.values():
        a.setflags(write=False)
    assert set(out) == set(KINDS)
    return out


def record(n, B, S):
    """(n, B, S): row r is row r of kind r mod len(KINDS); and the rows that
    are finite (FINITE kinds)."""
    c = cases(n, B, S)
    rec = np.stack([c[KINDS[r % len(KINDS)]][r] for r in range(n)])
    finite = np.array([KINDS[r % len(KINDS)] in FINITE for r in range(n)])
    return rec, finite
