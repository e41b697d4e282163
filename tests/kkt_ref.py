"""Long-double numpy model of the multipliers and the KKT certificate
(include/cmpc.h, cmpc_certify) — TEST INFRASTRUCTURE ONLY (the checker; the
product never imports this).  Written from the definitions, not from the
kernel: per QP slot, with n = nV, x the plan, d the other controllers' plans,

  C = [I; A],  A = I,  A[i][i - nu] = -1 for i >= nu          (2n rows)
  W: bit j of the working-set word, row j active; bit 16 + j, its upper side;
     empty where status != 0
  g = H x + f + G d,  cx = C x,  t[j] = hi[j] on an upper side, lo[j] on a lower
  lam_W: (C_W C_W') lam_W = C_W g, by LDL' elimination in the rows' order; a
     pivot <= 2^-20 (the matrix has integer entries, its true pivots are
     >= 1/64) means dependent normals: rank_def = 1, lam = 0
  r_stat = max|g - C' lam|;  r_prim = max_j max(lo - cx, cx - hi, 0)
  r_dual = largest wrong-signed |lam| over W;  r_comp = max_W |lam| |cx - t|
  obj = 1/2 x'Hx + (f + G d)'x;  scale = max|H| max(1, max|x|) + max|f + G d| + 1

The whole working set is eliminated at once (the kernel works per input).
dtype = numpy.longdouble is the reference; dtype = numpy.float64 is the plain
evaluation of the same formulas whose distance from the reference sets the
device's tolerance (units()).
"""
import numpy as np

FIELDS = ("lam", "r_stat", "r_prim", "r_dual", "r_comp", "obj", "scale", "n_active", "status", "rank_def")
EXACT = ("n_active", "status", "rank_def")
PIVOT_MIN = 2.0 ** -20
EPS = float(np.finfo(np.float64).eps)


def rows(n, nu, dtype=np.longdouble):
    """The 2n constraint rows: bounds (j < n), then the rate rows."""
    A = np.eye(n, dtype=dtype)
    for i in range(nu, n):
        A[i, i - nu] = -1
    return np.vstack([np.eye(n, dtype=dtype), A])


def slot_limits(lim, u_old, nu, m, dtype=np.longdouble):
    """lo, hi (2n) of one slot from its [lower | upper | rate_lower | rate_upper]
    (4, nu) and u_old[:nu]: lo[j] = lower[c] - u_old[c] ... with c = j mod nu."""
    lim = np.asarray(lim, dtype=dtype).reshape(4, nu)
    uo = np.asarray(u_old, dtype=dtype)[:nu]
    lo = np.concatenate([np.tile(lim[0] - uo, m), np.tile(lim[2], m)])
    hi = np.concatenate([np.tile(lim[1] - uo, m), np.tile(lim[3], m)])
    return lo, hi


def _ldl_solve(Nm, rhs, dtype):
    """lam with Nm lam = rhs by LDL' without pivoting; None where a pivot is
    not above PIVOT_MIN."""
    k = len(rhs)
    Lm = np.eye(k, dtype=dtype)
    dg = np.zeros(k, dtype=dtype)
    for j in range(k):
        p = Nm[j, j]
        for t in range(j):
            p = p - Lm[j, t] * Lm[j, t] * dg[t]
        if not p > PIVOT_MIN:
            return None
        dg[j] = p
        for i in range(j + 1, k):
            v = Nm[i, j]
            for t in range(j):
                v = v - Lm[i, t] * Lm[j, t] * dg[t]
            Lm[i, j] = v / p
    y = np.array(rhs, dtype=dtype)
    for i in range(k):
        for t in range(i):
            y[i] = y[i] - Lm[i, t] * y[t]
    lam = np.zeros(k, dtype=dtype)
    for i in range(k - 1, -1, -1):
        v = y[i] / dg[i]
        for t in range(i + 1, k):
            v = v - Lm[t, i] * lam[t]
        lam[i] = v
    return lam


def certify_slot(H, f, G, d, x, ws, status, lo, hi, nu, dtype=np.longdouble):
    """The record of one slot as a dict (lam (2n,), the other fields scalars)."""
    n = len(f)
    c = lambda a: np.asarray(a, dtype=dtype)
    H, f, x, lo, hi = c(H).reshape(n, n), c(f), c(x), c(lo), c(hi)
    C = rows(n, nu, dtype)
    gd = f.copy()
    if G is not None and np.size(G):
        gd = gd + c(G).reshape(n, -1) @ c(d)
    hx = H @ x
    g = hx + gd
    cx = C @ x
    ws = int(ws) if int(status) == 0 else 0
    act = [j for j in range(2 * n) if (ws >> j) & 1]
    upper = {j: bool((ws >> (16 + j)) & 1) for j in act}
    lam = np.zeros(2 * n, dtype=dtype)
    rank_def = 0
    if act:
        CW = C[act]
        sol = _ldl_solve(CW @ CW.T, CW @ g, dtype)
        if sol is None:
            rank_def = 1
        else:
            lam[act] = sol
    r_stat = np.abs(g - C.T @ lam).max()
    r_prim = max(np.maximum(lo - cx, cx - hi).max(), dtype(0))
    r_dual = dtype(0)
    r_comp = dtype(0)
    for j in act:
        if (lam[j] > 0) if upper[j] else (lam[j] < 0):
            r_dual = max(r_dual, abs(lam[j]))
        t = hi[j] if upper[j] else lo[j]
        r_comp = max(r_comp, abs(lam[j]) * abs(cx[j] - t))
    obj = dtype(0.5) * (x @ hx) + gd @ x
    scale = np.abs(H).max() * max(dtype(1), np.abs(x).max()) + np.abs(gd).max() + dtype(1)
    return {"lam": lam, "r_stat": r_stat, "r_prim": r_prim, "r_dual": r_dual, "r_comp": r_comp, "obj": obj,
            "scale": scale, "n_active": float(len(act)), "status": float(int(status)), "rank_def": float(rank_def)}


def certify_batch(H, f, G, d, x, ws, status, lim, u_old, nu, dtype=np.longdouble):
    """The records of nq slots: {field: array}, lam (nq, 2n), the rest (nq,).
    lim (nq, 4, nu) per slot [lower | upper | rate_lower | rate_upper]; lo and
    hi are formed in float64 as the solver forms them (lower - u_old, one
    rounding), then carried in dtype."""
    nq, n = f.shape
    m = n // nu
    out = {k: np.zeros((nq, 2 * n) if k == "lam" else nq, dtype=dtype) for k in FIELDS}
    for q in range(nq):
        lo, hi = slot_limits(lim[q], u_old[q], nu, m, np.float64)
        r = certify_slot(H[q], f[q], G[q] if G is not None and G.shape[-1] else None,
                         d[q] if d is not None and d.shape[-1] else None, x[q], ws[q], status[q], lo, hi, nu, dtype)
        for k in FIELDS:
            out[k][q] = r[k]
    return out


def units(H, f, G, d, x, lim, u_old, nu):
    """Per slot and field, the magnitude that one float64 rounding of the
    field's inputs is measured against (multiply by EPS for the unit):
      mag = max_i (sum_j |H_ij x_j| + |f_i| + sum_k |G_ik d_k|)   the summed magnitudes of g
      lam, r_stat, r_dual: mag;  obj: mag * sum|x|;  scale: the scale's own size
      r_prim: max|x| + max|limit| + max|u_old|;  r_comp: mag * that."""
    nq, n = f.shape
    u = {}
    mag = np.abs(H * x[:, None, :]).sum(axis=2) + np.abs(f)
    if G is not None and G.shape[-1]:
        mag = mag + np.abs(G * d[:, None, :]).sum(axis=2)
    mag = mag.max(axis=1)
    xs = np.abs(x).max(axis=1)
    span = xs + np.abs(np.asarray(lim).reshape(nq, -1)).max(axis=1) + np.abs(u_old[:, :nu]).max(axis=1)
    u["lam"] = u["r_stat"] = u["r_dual"] = mag
    u["obj"] = mag * np.abs(x).sum(axis=1)
    u["scale"] = np.abs(H).reshape(nq, -1).max(axis=1) * np.maximum(1.0, xs) + mag + 1.0
    u["r_prim"] = span
    u["r_comp"] = mag * span
    return u


def deviation(a, b, unit):
    """max over slots and fields of |a - b| / (EPS unit), and the field it is at"""
    worst, where = 0.0, None
    for k in FIELDS:
        if k in EXACT:
            continue
        da = np.abs(np.asarray(a[k], dtype=np.longdouble) - np.asarray(b[k], dtype=np.longdouble))
        un = np.maximum(unit[k], np.finfo(np.float64).tiny)   # (obj of a zero plan: 0 against 0)
        un = un[:, None] if da.ndim == 2 else un
        r = float((da / (EPS * un)).max())
        if r > worst:
            worst, where = r, k
    return worst, where


def host_summary(rec, fields, tol):
    """cmpc_certify_summary's reduction on a downloaded (len, nq) record, in
    float64: the same divisions, maxima with the lowest slot on ties, counts."""
    row = lambda k: rec[fields[k].start]
    ok = row("status") == 0.0
    idx = np.nonzero(ok)[0]
    out = {"n_not_ok": int((~ok).sum())}
    vals = {"stat": row("r_stat") / row("scale"), "prim": row("r_prim"), "dual": row("r_dual") / row("scale"),
            "comp": row("r_comp") / row("scale")}
    above = np.zeros(rec.shape[1], bool)
    for k, v in vals.items():
        if idx.size:
            best = idx[np.argmax(v[idx])]          # (argmax: the first, i.e. lowest, slot of the maximum)
            out["r_" + k], out["slot_" + k] = float(v[best]), int(best)
        else:
            out["r_" + k], out["slot_" + k] = 0.0, -1
        above |= ok & (v > tol)
    out["n_above"] = int(above.sum())
    return out
