"""Float64 numpy model of the closed-loop performance indices (include/cmpc.h,
cmpc_score_*) — TEST INFRASTRUCTURE ONLY (the checker; the product never
imports this).  Written from the field table, not from the kernel: per step k
and QP slot q = b*S + s, with e[o] = y[b][out_idx[s][o]] - target[q][o],

  n += 1; ise += (e e) Ts; iae += |e| Ts; peak = max(peak, |e|)
  last_out = k where |e| > band[s][o]           (starts at -1)
  j_track += 1/2 e' ywt[q] e;  j_move += 1/2 du' uwt[q] du;  tv += |du|
  sat_bound[c] += 1 when status == 0 and bit c of ws is set
  sat_rate[c]  += 1 when status == 0 and bit nV + c of ws is set
  n_fail += 1 when status != 0;  nwsr_sum += nwsr
  plant_fail_step = first k with a non-zero plant status   (starts at -1)

Every sum is one numpy multiply or add per term in the order written, so all
fields but j_track and j_move are what the kernel's FP64 gives bit for bit.
"""
import numpy as np

FIELDS = ("n", "ise", "iae", "peak", "last_out", "j_track", "j_move", "tv", "sat_bound", "sat_rate",
          "n_fail", "nwsr_sum", "plant_fail_step")
EXACT = tuple(f for f in FIELDS if f not in ("j_track", "j_move"))


class ScoreMirror:
    def __init__(self, B, S, ny, nu, nV, out_idx, Ts, band=None):
        self.B, self.S, self.ny, self.nu, self.nV, self.Ts = B, S, ny, nu, nV, float(Ts)
        self.oi = np.asarray(out_idx, dtype=np.int64)[:, :ny]
        self.band = np.zeros((S, ny)) if band is None else np.asarray(band, dtype=np.float64).reshape(S, ny)
        nq = B * S
        z = lambda *s: np.zeros((nq,) + s)
        self.k = 0
        self.f = {"n": z(), "ise": z(ny), "iae": z(ny), "peak": z(ny), "last_out": z(ny) - 1.0,
                  "j_track": z(), "j_move": z(), "tv": z(nu), "sat_bound": z(nu), "sat_rate": z(nu),
                  "n_fail": z(), "nwsr_sum": z(), "plant_fail_step": z() - 1.0}

    def step(self, y, target, du, status, nwsr, ws, ywt, uwt, plant_status=None):
        """y (B, n_outputs); target (B*S, ny); du (B*S, >= nu) plans (the first
        move is read); status, nwsr, ws (B*S,); ywt (B*S, ny, ny) and uwt
        (B*S, nu, nu) the weights in force per slot; plant_status (B,) or None."""
        B, S, ny, nu, f, k = self.B, self.S, self.ny, self.nu, self.f, float(self.k)
        y = np.asarray(y, dtype=np.float64)
        ys = y[:, self.oi].reshape(B * S, ny)                    # y[b][out_idx[s][o]]
        e = ys - np.asarray(target, dtype=np.float64).reshape(B * S, ny)
        ae = np.abs(e)
        d = np.asarray(du, dtype=np.float64)[:, :nu]
        band = np.tile(self.band, (B, 1))
        f["n"] = f["n"] + 1.0
        f["ise"] = f["ise"] + (e * e) * self.Ts
        f["iae"] = f["iae"] + ae * self.Ts
        f["peak"] = np.maximum(f["peak"], ae)
        f["last_out"] = np.where(ae > band, k, f["last_out"])
        f["j_track"] = f["j_track"] + 0.5 * np.einsum("qi,qij,qj->q", e, np.asarray(ywt, dtype=np.float64), e)
        f["j_move"] = f["j_move"] + 0.5 * np.einsum("qi,qij,qj->q", d, np.asarray(uwt, dtype=np.float64), d)
        f["tv"] = f["tv"] + np.abs(d)
        ok = np.asarray(status) == 0
        w = np.asarray(ws, dtype=np.uint32).astype(np.int64)
        c = np.arange(nu)
        f["sat_bound"] = f["sat_bound"] + (ok[:, None] & (((w[:, None] >> c) & 1) == 1)).astype(np.float64)
        f["sat_rate"] = f["sat_rate"] + (ok[:, None] & (((w[:, None] >> (self.nV + c)) & 1) == 1)).astype(np.float64)
        f["n_fail"] = f["n_fail"] + (~ok).astype(np.float64)
        f["nwsr_sum"] = f["nwsr_sum"] + np.asarray(nwsr).astype(np.float64)
        if plant_status is not None:
            bad = np.repeat(np.asarray(plant_status) != 0, S)
            f["plant_fail_step"] = np.where(bad & (f["plant_fail_step"] < 0), k, f["plant_fail_step"])
        self.k += 1

    def record(self, fields):
        """The record as the library lays it out: (len, B*S) field-major, rows
        placed by `fields` = {name: slice} (cmpc.score_fields)."""
        n = max(sl.stop for sl in fields.values())
        out = np.zeros((n, self.B * self.S))
        for name, sl in fields.items():
            out[sl] = self.f[name].reshape(self.B * self.S, -1).T
        return out
