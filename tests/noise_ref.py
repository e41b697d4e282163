"""Reference models of the seeded noise (include/cmpc.h) —
TEST INFRASTRUCTURE ONLY (the checker; the product never imports this).

Written from the published constants of Philox4x32-10 and the formulas of the
header, not from the library:
  philox4x32_10   pure-Python integers, one call
  uniforms        the (B, ceil(n/2), 2) uniforms of a step, float64, exact
  normals_ld      the Box-Muller pairs in numpy longdouble (the yardstick)
  normals_f64     a float64 numpy evaluation that forms cos(2 pi u2) (the
                  plain model whose distance to the yardstick sets the scale)
  step_model      w and out of the element update from given z, float64, in
                  the header's operation order
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# Known answers of Philox4x32-10 (counter, key, output): the Random123
# distribution's kat_vectors.
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = (int(v) & MASK for v in ctr)
    k0, k1 = (int(v) & MASK for v in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
    return c0, c1, c2, c3


def words_to_k(x):
    """(k1, k2) of the four output words."""
    return ((x[0] >> 5) << 26) + (x[1] >> 6), ((x[2] >> 5) << 26) + (x[3] >> 6)


def uniforms(seed, step, B, n, stream=0, scenario0=0):
    """(B, ceil(n/2), 2) float64: [u1, u2] per pair, exact."""
    key = (seed & MASK, (seed >> 32) & MASK)
    npair = (n + 1) // 2
    u = np.zeros((B, npair, 2))
    for b in range(B):
        for j in range(npair):
            k1, k2 = words_to_k(philox4x32_10((scenario0 + b, step, j, stream), key))
            u[b, j, 0] = float(k1 + 1) * 2.0 ** -53     # (k1 + 1 <= 2^53: exact)
            u[b, j, 1] = float(k2) * 2.0 ** -53
    return u


def _pairs_to_channels(c, s, n):
    """(B, npair) cosine and sine branches to (B, n) channels: 2j the cosine,
    2j + 1 the sine, the last sine dropped with n odd."""
    B, npair = c.shape
    z = np.empty((B, 2 * npair), dtype=c.dtype)
    z[:, 0::2], z[:, 1::2] = c, s
    return z[:, :n]


def normals_ld(u, n):
    """(z (B, n) longdouble, r (B, n) float64): the yardstick and each
    channel's radius r = sqrt(-2 ln u1), the unit of the error count."""
    ld = np.longdouble
    u1, u2 = u[:, :, 0].astype(ld), u[:, :, 1].astype(ld)
    r = np.sqrt(ld(-2) * np.log(u1))
    # 2 u2 = q / 2 + t exactly (u2 is a multiple of 2^-53), so the argument of
    # sin and cos stays inside [-pi/4, pi/4] in longdouble
    x = ld(2) * u2
    q = np.rint(ld(2) * x)
    a = (x - q / ld(2)) * ld("3.14159265358979323846264338327950288")
    sa, ca = np.sin(a), np.cos(a)
    k = q.astype(np.int64) & 3
    s = np.choose(k, [sa, ca, -sa, -ca])
    c = np.choose(k, [ca, -sa, -ca, sa])
    rr = r.astype(np.float64)
    return _pairs_to_channels(r * c, r * s, n), _pairs_to_channels(rr, rr, n)


def normals_f64(u, n):
    """The plain float64 evaluation: r cos(2 pi u2), r sin(2 pi u2)."""
    u1, u2 = u[:, :, 0], u[:, :, 1]
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * np.pi * u2
    return _pairs_to_channels(r * np.cos(a), r * np.sin(a), n)


def error_units(z, z_ld, r):
    """max |z - z_ld| / (eps r) over the channels with r > 0."""
    eps = np.finfo(np.float64).eps
    d = np.abs(z.astype(np.longdouble) - z_ld)
    ok = r > 0
    return float(np.max(d[ok] / (eps * r[ok].astype(np.longdouble))))


def step_model(z, sigma=None, rho=None, w=None, base=None):
    """(w', out) of the element update from the normals z (B, n), float64, in
    the header's operation order: products and sums separately rounded."""
    z = np.asarray(z, dtype=np.float64)
    s = np.ones_like(z) if sigma is None else np.broadcast_to(np.asarray(sigma, dtype=np.float64), z.shape)
    if rho is not None:
        rh = np.broadcast_to(np.asarray(rho, dtype=np.float64), z.shape)
        g = np.sqrt(1.0 - rh * rh) * s
        t1 = rh * np.asarray(w, dtype=np.float64)
        t2 = g * z
        w = t1 + t2
        d = w
    else:
        d = s * z
    b = np.zeros_like(z) if base is None else np.broadcast_to(np.asarray(base, dtype=np.float64), z.shape)
    out = np.where(d == 0.0, b, b + d)
    return w, out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
