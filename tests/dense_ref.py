"""Dense test problems and a long-double reference of the condensed QP and of
the prediction.  TEST INFRASTRUCTURE ONLY.

The reference is written from the record contract of include/cmpc.h (the
"lin record" and its dx_aug tail) and from the model stated at the top of
csrc/predict.hip, not from the oracle's block loop (oracle/or_condense.c): it
steps the plant model forward in numpy.longdouble,

    x_{k+1} = A x_k + fd + sum_c Bin[:, c] v_c(k)          x_0 = 0
    y_k     = y_prev + C_dist x_dist + C_x x_{k+1}          k = 0 .. p-1

with v_c(k) what input c feeds the plant at step k: its move-blocked plan
entry min(k - D_c, m - 1) once k >= D_c, and before that the stored delay
state of that step less u_old[c] (AdjustAllDelayedStates): the delayed-input
slot at k = 0, then the input's shift block front to back.  The free response
is the run with zero plans, column j of Su (Su_other) the run with the unit
plan e_j minus the free response, and

    H = Su' W Su + kron(I_m, uwt)      W = blkdiag_p(ywt)
    f = Su' W (y_free - y_ref)
    G = Su' W Su_other

in the oracle's sign and ordering conventions (own plans mv*nu + c, the other
controllers' mv*nuo + c).  Nothing here forms powers of A or touches a
Cholesky factor, so a misreading of the contract shared by the oracle and the
kernels does not carry over.

dense_problem draws records in which no entry is zero and nothing is
structured: the plant data of cmpc/synthetic.py has exact zeros in A, Bin and
Csel, diagonal weights and a reference that is constant over the horizon, all
of which hide index errors.

The per-scenario settings of include/cmpc.h enter the model where the header
puts them: slot q's own ywt[q] and uwt[q] in place of the sub-controller's,
and the reference y_ref[s] + dy[q] + dref[q]; ref_shift is the amount
g = Su' W dref a profile takes off f.  The draw has per-slot limits and a
paired form for build pairing (scenario_case and the builders after it).
"""
import numpy as np

import cmpc
from cmpc._abi import CmpcDims

LD = np.longdouble

# (ns, ny, nu, m) of csrc/kernel_dims.h, each as the reference configuration
# that has those dimensions
DIM_SETS = {(11, 3, 2, 2): ("par", "coop", 2), (11, 2, 2, 2): ("par", "ncoop", 2),
            (11, 3, 4, 2): ("par", "cent", 2), (10, 2, 2, 2): ("ser", "ncoop", 2),
            (10, 4, 2, 2): ("ser", "coop", 2), (10, 4, 4, 2): ("ser", "cent", 2),
            (11, 3, 2, 1): ("par", "coop", 1), (11, 3, 2, 3): ("par", "coop", 3)}


def config_for(dimset, p, delays=None):
    import dataclasses
    plant, ctype, m = DIM_SETS[tuple(dimset)]
    cfg = cmpc.reference_config(plant, ctype, p=p, m=m)
    if delays is not None:
        cfg = dataclasses.replace(cfg, delays=tuple(delays))
    assert (cfg.ns, cfg.ny, cfg.nu, cfg.m) == tuple(dimset)
    return cfg


class Layout:
    """Offsets of one lin record, from the comment above cmpc_layout in
    include/cmpc.h (test_dense_reference.py checks it against or_layout_of)."""

    def __init__(self, cfg):
        d = cfg.delays[:cfg.nu_tot]
        self.nd = sum(1 for D in d if D)
        self.naug = cfg.ndist + sum(d)
        self.nobs = cfg.ns + cfg.ndist
        self.nV, self.nuo = cfg.m * cfg.nu, cfg.nu_tot - cfg.nu
        self.nVo = cfg.m * self.nuo
        self.off_A = 0
        self.off_B = self.off_A + cfg.ns * cfg.ns
        self.off_C = self.off_B + cfg.ns * cfg.nu_tot
        self.off_f = self.off_C + cfg.ny * self.nobs
        self.off_x = self.off_f + cfg.ns
        self.off_y = self.off_x + self.naug
        self.rec_len = (self.off_y + cfg.ny + 7) // 8 * 8
        # per input: its delayed-input slot and the start of its shift block in dx_aug
        self.dslot, self.dblk = [-1] * cfg.nu_tot, [-1] * cfg.nu_tot
        slot, blk = cfg.ndist, cfg.ndist + self.nd
        for c, D in enumerate(d):
            if D:
                self.dslot[c], self.dblk[c] = slot, blk
                slot += 1
                blk += D - 1


# ---------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------

def _spd_dense(rng, n):
    """QQ' + I with every off-diagonal entry non-zero"""
    while True:
        Q = rng.standard_normal((n, n))
        W = Q @ Q.T + np.eye(n)
        W = 0.5 * (W + W.T)
        if np.all(W != 0.0):
            return W


def _nonzero(a):
    assert np.all(a != 0.0)   # a Gaussian draw is zero with probability 0
    return a


def dense_problem(cfg, B, seed, rho=0.95, scale=1.0, paired=False, limit_scale=None):
    """(lin [B*S, rec_len], u_old [B*S, nu_tot], arrays) from one seeded
    generator.  Per slot: A dense Gaussian rescaled to spectral radius rho;
    Bin, every column of Csel (the disturbance columns too), fd, dx_aug and
    y_prev dense Gaussian; u_old non-zero in every input, strictly inside the
    setup file's limits (one plant-level draw per scenario, mapped to each
    sub-controller's input order).  Per sub-controller: ywt = QQ' + I and
    uwt = QQ' + I, y_ref independent Gaussian at every horizon row and output,
    the setup file's limits.  Nothing is zero and everything is O(1).

    scale multiplies the affine data (fd, dx_aug's deviations, y_prev, y_ref),
    and with it the QP's linear term f: at 1 the unconstrained optimum lies far
    outside the limits (0.1 to 1) and every QP ends at a vertex of them; the
    step tests choose a smaller one (H and G do not depend on it).

    limit_scale (B*S, 1): slot q's limits are the setup file's times
    limit_scale[q] (slot_limits), and u_old is drawn strictly inside them.
    paired (S = 2, nu_tot = 2 nu): after the draw, slot 1's A, C and fd become
    slot 0's bit for bit, its Bin slot 0's rolled by -nu columns and
    arr.ywt[1] = arr.ywt[0], which is what build pairing assumes
    (include/cmpc.h); dx_aug, y_prev, u_old, uwt and y_ref stay each slot's own
    (assert_paired).  With neither the draw is what it was without them."""
    rng = np.random.default_rng(seed)
    L = Layout(cfg)
    S, ns, nut, ny, nu, p = cfg.S, cfg.ns, cfg.nu_tot, cfg.ny, cfg.nu, cfg.p
    plant = "par" if cfg.plant == 0 else "ser"
    arr = cmpc.controller_arrays(cfg, cmpc.reference_setup(plant, cfg.controller))
    arr.ywt = np.ascontiguousarray(np.stack([_spd_dense(rng, ny) for _ in range(S)]))
    arr.uwt = np.ascontiguousarray(np.stack([_spd_dense(rng, nu) for _ in range(S)]))
    arr.y_ref = np.ascontiguousarray(_nonzero(scale * rng.standard_normal((S, p * ny))))
    nq = B * S
    lin = np.zeros((nq, L.rec_len))
    for q in range(nq):
        A = rng.standard_normal((ns, ns))
        A *= rho / np.abs(np.linalg.eigvals(A)).max()
        lin[q, L.off_A:L.off_B] = A.ravel()
        lin[q, L.off_B:L.off_y + ny] = rng.standard_normal(L.off_y + ny - L.off_B)
        lin[q, L.off_f:L.off_y + ny] *= scale
    _nonzero(lin[:, :L.off_y + ny])
    # u_old: plant-level, at 10 % .. 90 % of each input's range
    lo, hi = np.zeros((B, nut)), np.zeros((B, nut))
    ls = np.ones((B, S)) if limit_scale is None else np.asarray(limit_scale, dtype=np.float64).reshape(B, S)
    for s in range(S):
        for c in range(nu):
            k = cfg.input_order[s][c]
            lo[:, k], hi[:, k] = arr.lower[s][c] * ls[:, s], arr.upper[s][c] * ls[:, s]
    u_plant = lo + (hi - lo) * rng.uniform(0.1, 0.9, (B, nut))
    u_old = np.zeros((B, S, nut))
    for s in range(S):
        u_old[:, s, :] = u_plant[:, cfg.input_order[s]]
    u_old = np.ascontiguousarray(u_old.reshape(nq, nut))
    _nonzero(u_old)
    # the delay states hold past inputs: the Gaussian draw is their deviation
    # from u_old (what AdjustAllDelayedStates leaves), the record stores the sum
    for c in range(nut):
        D = cfg.delays[c]
        if D:
            lin[:, L.off_x + L.dslot[c]] += u_old[:, c]
            lin[:, L.off_x + L.dblk[c]:L.off_x + L.dblk[c] + D - 1] += u_old[:, c:c + 1]
    _nonzero(lin[:, :L.off_y + ny])
    if paired:
        assert S == 2 and nut == 2 * nu
        lin[1::2, :L.off_B] = lin[0::2, :L.off_B]
        lin[1::2, L.off_C:L.off_x] = lin[0::2, L.off_C:L.off_x]
        B0 = lin[0::2, L.off_B:L.off_C].reshape(B, ns, nut)
        lin[1::2, L.off_B:L.off_C] = np.roll(B0, -nu, axis=2).reshape(B, ns * nut)
        arr.ywt[1] = arr.ywt[0]
    return np.ascontiguousarray(lin), u_old, arr


def slot_limits(cfg, arr, limit_scale):
    """(lower, upper, rate_lower, rate_upper), each (B*S, nu): the setup file's
    limits of the slot's sub-controller times limit_scale[q]"""
    nq = np.asarray(limit_scale).shape[0]
    sc = np.asarray(limit_scale, dtype=np.float64).reshape(nq, 1)
    return tuple(np.ascontiguousarray(np.tile(getattr(arr, n), (nq // cfg.S, 1)) * sc)
                 for n in ("lower", "upper", "rate_lower", "rate_upper"))


def assert_paired(cfg, lin, u_old, arr):
    """The premises of build pairing, as test_gpu_build_pairing.problem checks
    them on plant records, and what has to stay different for the pair to be a
    test: equal plants up to Bin's column rotation and equal ywt, bit for bit;
    distinct tails, u_old, uwt and y_ref."""
    L = Layout(cfg)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    for b in range(lin.shape[0] // 2):
        r0, r1 = lin[2 * b], lin[2 * b + 1]
        B0 = r0[L.off_B:L.off_C].reshape(cfg.ns, cfg.nu_tot)
        B1 = r1[L.off_B:L.off_C].reshape(cfg.ns, cfg.nu_tot)
        assert np.array_equal(bits(r0[:L.off_B]), bits(r1[:L.off_B]))
        assert np.array_equal(bits(r0[L.off_C:L.off_x]), bits(r1[L.off_C:L.off_x]))
        assert np.array_equal(bits(np.roll(B0, -cfg.nu, axis=1)), bits(B1))
        assert not np.array_equal(B0, B1)
        assert np.all(r0[L.off_x:L.off_y + cfg.ny] != r1[L.off_x:L.off_y + cfg.ny])
        assert np.all(u_old[2 * b] != u_old[2 * b + 1])
    assert np.array_equal(bits(arr.ywt[0]), bits(arr.ywt[1]))
    assert np.all(arr.uwt[0] != arr.uwt[1]) and np.all(arr.y_ref[0] != arr.y_ref[1])


def assert_dense(cfg, lin, u_old, arr):
    """The draw's own properties: no zero entry in any record field, u_old or
    reference; weights symmetric positive definite with non-zero off-diagonals."""
    L = Layout(cfg)
    assert np.all(lin[:, :L.off_y + cfg.ny] != 0.0), "a zero entry in a lin record"
    assert np.all(u_old != 0.0) and np.all(arr.y_ref != 0.0)
    for W in list(arr.ywt) + list(arr.uwt):
        assert np.all(W != 0.0) and np.array_equal(W, W.T)
        assert np.linalg.eigvalsh(W).min() >= 1.0 - 1e-12
    ns = cfg.ns
    for q in range(lin.shape[0]):
        r = np.abs(np.linalg.eigvals(lin[q, :ns * ns].reshape(ns, ns))).max()
        assert r < 1.0


# ---------------------------------------------------------------------------
# the long-double model
# ---------------------------------------------------------------------------

def _fields(cfg, L, lin):
    Q, ns, nut, ny = lin.shape[0], cfg.ns, cfg.nu_tot, cfg.ny
    x = np.asarray(lin, dtype=np.float64).astype(LD)
    A = x[:, L.off_A:L.off_B].reshape(Q, ns, ns)
    Bin = x[:, L.off_B:L.off_C].reshape(Q, ns, nut)
    C = x[:, L.off_C:L.off_f].reshape(Q, ny, L.nobs)
    return A, Bin, C[:, :, :ns], C[:, :, ns:], x[:, L.off_f:L.off_x], x[:, L.off_x:L.off_y], x[:, L.off_y:L.off_y + ny]


def simulate(cfg, lin, u_old, plans):
    """Outputs of the model for R runs per slot.  lin (Q, rec_len), u_old
    (Q, nu_tot), plans (Q, R, m, nu_tot): per run the move-blocked plan of
    every input in the slot's input order.  Returns (Q, R, p, ny) longdouble."""
    L = Layout(cfg)
    A, Bin, Cx, Cd, fd, xa, yprev = _fields(cfg, L, lin)
    Q, R = plans.shape[0], plans.shape[1]
    p, m, nut = cfg.p, cfg.m, cfg.nu_tot
    uo = np.asarray(u_old, dtype=np.float64).astype(LD)
    plans = np.asarray(plans).astype(LD)
    ybase = yprev + np.einsum("qod,qd->qo", Cd, xa[:, :cfg.ndist])
    x = np.zeros((Q, cfg.ns, R), dtype=LD)
    Y = np.zeros((Q, R, p, cfg.ny), dtype=LD)
    v = np.zeros((Q, nut, R), dtype=LD)
    for k in range(p):
        for c in range(nut):
            D = cfg.delays[c]
            if k >= D:
                v[:, c, :] = plans[:, :, min(k - D, m - 1), c]
            else:
                stored = xa[:, L.dslot[c]] if k == 0 else xa[:, L.dblk[c] + k - 1]
                v[:, c, :] = (stored - uo[:, c])[:, None]
        x = np.matmul(A, x) + fd[:, :, None] + np.matmul(Bin, v)
        Y[:, :, k, :] = np.transpose(np.matmul(Cx, x), (0, 2, 1)) + ybase[:, None, :]
    return Y


def _plan_slots(cfg, du, d):
    """(Q, nV) own and (Q, nVo) other plans -> (Q, m, nu_tot) per-input plans"""
    Q, m, nu, nuo = du.shape[0], cfg.m, cfg.nu, cfg.nu_tot - cfg.nu
    out = np.zeros((Q, m, cfg.nu_tot), dtype=LD)
    out[:, :, :nu] = np.asarray(du).reshape(Q, m, nu)
    if nuo:
        out[:, :, nu:] = np.asarray(d).reshape(Q, m, nuo)
    return out


def ref_matrices(cfg, lin, u_old):
    """(y_free (Q, p*ny), Su (Q, p*ny, nV), Su_other (Q, p*ny, nVo)), longdouble"""
    L = Layout(cfg)
    Q, m, nu, nut = lin.shape[0], cfg.m, cfg.nu, cfg.nu_tot
    R = 1 + L.nV + L.nVo
    plans = np.zeros((Q, R, m, nut), dtype=LD)
    for mv in range(m):
        for c in range(nu):
            plans[:, 1 + mv * nu + c, mv, c] = 1
        for c in range(L.nuo):
            plans[:, 1 + L.nV + mv * L.nuo + c, mv, nu + c] = 1
    Y = simulate(cfg, lin, u_old, plans).reshape(Q, R, cfg.p * cfg.ny)
    resp = np.transpose(Y[:, 1:, :] - Y[:, :1, :], (0, 2, 1))
    return Y[:, 0, :], resp[:, :, :L.nV], resp[:, :, L.nV:]


def _slot_settings(cfg, Q, arr, ywt, uwt, dy, dref):
    """Per slot q = b*S + s in long double: ywt (Q, ny, ny) and uwt (Q, nu, nu),
    the slot's own where given, else arr's of s; the reference (Q, p*ny)
    y_ref[s] + dy[q] + dref[q] with whichever of the two is given
    (include/cmpc.h: cmpc_set_scenario_reference, _reference_profile, _weights)."""
    ld = lambda a: np.asarray(a, dtype=np.float64).astype(LD)
    s_of = np.arange(Q) % cfg.S
    W = ld(arr.ywt)[s_of] if ywt is None else ld(ywt).reshape(Q, cfg.ny, cfg.ny)
    R = ld(arr.uwt)[s_of] if uwt is None else ld(uwt).reshape(Q, cfg.nu, cfg.nu)
    yref = ld(arr.y_ref)[s_of]                                            # (Q, p*ny)
    if dy is not None:
        yref = (yref.reshape(Q, cfg.p, cfg.ny) + ld(dy).reshape(Q, 1, cfg.ny)).reshape(Q, -1)
    if dref is not None:
        yref = yref + ld(dref).reshape(Q, -1)
    return W, R, yref


def ref_qp(cfg, lin, u_old, arr, ywt=None, uwt=None, dy=None, dref=None):
    """Long-double H (Q, nV, nV), f (Q, nV), G (Q, nV, nVo) and the Gram part
    H - R, for slots q = b*S + s with the weights and reference of arr[s], or
    with the slot's own ywt (Q, ny, ny), uwt (Q, nu, nu) and the reference
    y_ref[s] + dy[q] + dref[q] (dy (Q, ny), dref (Q, p, ny)) where given."""
    Q, S, p, ny, nu, m = lin.shape[0], cfg.S, cfg.p, cfg.ny, cfg.nu, cfg.m
    yfree, Su, Suo = ref_matrices(cfg, lin, u_old)
    ywt, uwt, yref = _slot_settings(cfg, Q, arr, ywt, uwt, dy, dref)
    nV = m * nu
    WSu = np.einsum("qab,qrbc->qrac", ywt, Su.reshape(Q, p, ny, nV)).reshape(Q, p * ny, nV)
    gram = np.einsum("qra,qrb->qab", Su, WSu)
    Rm = np.zeros((Q, nV, nV), dtype=LD)
    for mv in range(m):
        Rm[:, mv * nu:(mv + 1) * nu, mv * nu:(mv + 1) * nu] = uwt
    f = np.einsum("qra,qr->qa", WSu, yfree - yref)
    G = np.einsum("qra,qrc->qac", WSu, Suo)
    return gram + Rm, f, G, gram


def ref_shift(cfg, lin, u_old, arr, dref, ywt=None):
    """Long-double g (Q, nV) = Su' W dref, the amount a reference profile takes
    off f (include/cmpc.h), from the model's Su and the slot's ywt (arr's of s
    where none is given): computed directly, not as a difference of two f's."""
    Q, p, ny = lin.shape[0], cfg.p, cfg.ny
    _, Su, _ = ref_matrices(cfg, lin, u_old)
    W, _, _ = _slot_settings(cfg, Q, arr, ywt, None, None, None)
    w = np.einsum("qab,qrb->qra", W, np.asarray(dref, dtype=np.float64).astype(LD).reshape(Q, p, ny))
    return np.einsum("qra,qr->qa", Su, w.reshape(Q, p * ny))


def ref_prediction(cfg, lin, u_old, arr, du, d, ywt=None, uwt=None, dy=None, dref=None):
    """Long-double y_pred (Q, p, ny) and cost (Q, 2) = [J_track, J_move] of the
    plans du (Q, nV) and d (Q, nVo), as predict_ref.costs defines them; per-slot
    weights and reference as in ref_qp."""
    Q, S, p, ny, nu, m = lin.shape[0], cfg.S, cfg.p, cfg.ny, cfg.nu, cfg.m
    Y = simulate(cfg, lin, u_old, _plan_slots(cfg, du, d)[:, None])[:, 0]
    ywt, uwt, yref = _slot_settings(cfg, Q, arr, ywt, uwt, dy, dref)
    e = Y - yref.reshape(Q, p, ny)
    dm = np.asarray(du, dtype=np.float64).astype(LD).reshape(Q, m, nu)
    J = np.zeros((Q, 2), dtype=LD)
    J[:, 0] = np.einsum("qri,qij,qrj->q", e, ywt, e) / 2
    J[:, 1] = np.einsum("qki,qij,qkj->q", dm, uwt, dm) / 2
    return Y, J


# ---------------------------------------------------------------------------
# the bound (the project's form, scaled by the Gram part)
# ---------------------------------------------------------------------------

def qp_error_ratios(H, f, G, Href, fref, Gref, gram_ref):
    """Worst error of (H, f, G) over the slots as a fraction of the bound
      |H - Href| <= 1e-11 sH,  sH = max|Href - R|
      |f - fref| <= 1e-10 max(max|fref|, 1e-6 sH)
      |G - Gref| <= 1e-11 max(max|Gref|, 1e-6 sH)
    (test_gpu_build_matches_oracle's, with the Gram part in place of max|H|);
    <= 1 passes."""
    worst = {"H": 0.0, "f": 0.0, "G": 0.0}
    for q in range(Href.shape[0]):
        sH = float(np.abs(gram_ref[q]).max())
        worst["H"] = max(worst["H"], float(np.abs(H[q] - Href[q]).max()) / (1e-11 * sH))
        sf = max(float(np.abs(fref[q]).max()), 1e-6 * sH)
        worst["f"] = max(worst["f"], float(np.abs(f[q] - fref[q]).max()) / (1e-10 * sf))
        if Gref.shape[2]:
            sG = max(float(np.abs(Gref[q]).max()), 1e-6 * sH)
            worst["G"] = max(worst["G"], float(np.abs(G[q] - Gref[q]).max()) / (1e-11 * sG))
    return worst


def dims_of(cfg, B):
    return CmpcDims.from_config(cfg, B)


# ---------------------------------------------------------------------------
# shared cases: each computed once per process and left unchanged
# ---------------------------------------------------------------------------

REF_DELAYS = (0, 40, 0, 40)
Y_TOL = 1e-11   # test_gpu_predict.py: |y - y_ref| <= 1e-11 max|y_ref| per slot, costs 1e-11 relative


def case_seed(dimset, p, delays):
    return 5000 + 100 * list(DIM_SETS).index(tuple(dimset)) + p + sum(delays)


def oracle_qps(cfg, arr, lin, u_old):
    import _oracle as O
    dims = dims_of(cfg, 1)
    out = [O.build_qp(dims, lin[q], u_old[q], arr.y_ref[q % cfg.S], arr.ywt[q % cfg.S], arr.uwt[q % cfg.S])
           for q in range(lin.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[4] for o in out])


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


_cache = {}


def build_case(dimset, p, delays=REF_DELAYS, B=47):
    """A dense problem with the oracle's and the long-double QPs:
    dict(cfg, arr, lin, u_old, oracle=(H, f, G), ref=(H, f, G), gram, ratios),
    ratios = the oracle's error against the long-double reference as a
    fraction of the bound (qp_error_ratios)."""
    key = ("build", tuple(dimset), p, tuple(delays), B)
    if key not in _cache:
        cfg = config_for(dimset, p, delays)
        lin, u_old, arr = dense_problem(cfg, B, case_seed(dimset, p, delays))
        Hr, fr, Gr, gram = ref_qp(cfg, lin, u_old, arr)
        Ho, fo, Go = oracle_qps(cfg, arr, lin, u_old)
        _freeze(lin, u_old, Hr, fr, Gr, gram, Ho, fo, Go)
        _cache[key] = dict(cfg=cfg, arr=arr, lin=lin, u_old=u_old, oracle=(Ho, fo, Go), ref=(Hr, fr, Gr),
                           gram=gram, ratios=qp_error_ratios(Ho, fo, Go, Hr, fr, Gr, gram))
    return _cache[key]


def predict_case(dimset, p, delays=REF_DELAYS, B=47):
    """The problem of build_case with Gaussian plans du (nq, nV) and d (nq, nVo),
    d_gathered (the scenario's other slots' du in the Jacobi order) and the
    long-double predictions and costs for (du, d) and (du, d_gathered)."""
    import predict_ref as PR
    key = ("predict", tuple(dimset), p, tuple(delays), B)
    if key not in _cache:
        c = build_case(dimset, p, delays, B)
        cfg, L = c["cfg"], Layout(c["cfg"])
        nq = B * cfg.S
        rng = np.random.default_rng(case_seed(dimset, p, delays) + 1)
        du = np.ascontiguousarray(rng.standard_normal((nq, L.nV)))
        d = np.ascontiguousarray(rng.standard_normal((nq, L.nVo)))
        dg = np.ascontiguousarray(PR.gather_other(cfg, du))
        Y, J = ref_prediction(cfg, c["lin"], c["u_old"], c["arr"], du, d)
        Yg, Jg = ref_prediction(cfg, c["lin"], c["u_old"], c["arr"], du, dg) if L.nVo else (Y, J)
        _freeze(du, d, dg, Y, J, Yg, Jg)
        _cache[key] = dict(c, du=du, d=d, d_gathered=dg, given=(Y, J), gathered=(Yg, Jg))
    return _cache[key]


def prediction_error_ratios(Y, J, Yref, Jref):
    """Worst |Y - Yref| / (Y_TOL max|Yref[q]|) and worst relative cost error /
    Y_TOL over the slots; <= 1 passes test_gpu_predict.py's tolerances."""
    wy = wj = 0.0
    for q in range(Yref.shape[0]):
        wy = max(wy, float(np.abs(Y[q] - Yref[q]).max() / (Y_TOL * np.abs(Yref[q]).max())))
        wj = max(wj, float((np.abs(J[q] - Jref[q]) / (Y_TOL * np.abs(Jref[q]))).max()))
    return wy, wj


# The GPU file's cases, (dimension set, p, delays), all at B = 47: every
# dimension set at p = 7, 23, 50 with the reference delays, at p = 50 with two
# different delays inside the horizon and at p = 64 with the shortest delay
# beside one of p - 1; par-coop p = 100 runs the row kernel's ring lines.
GPU_BUILD_CASES = [(ds, p, dl) for ds in DIM_SETS
                   for p, dl in [(7, REF_DELAYS), (23, REF_DELAYS), (50, REF_DELAYS), (50, (0, 10, 0, 25)),
                                 (64, (0, 2, 0, 63))]] + [((11, 3, 2, 2), 100, REF_DELAYS)]
# predict: one partial chunk of 16 steps, one exact chunk, a chunk plus one step, three chunks and two steps
GPU_PREDICT_CASES = [(ds, p, REF_DELAYS) for ds in DIM_SETS for p in (7, 16, 17, 50)]


# The step cases (cmpc_step, K = 3): the draw's scale and seed are chosen so
# that a quarter or more of the QPs end with an active constraint, no oracle
# solve comes within NEAR_TIE of a tie and every status is 0
# (test_dense_reference.py checks all three on the CPU).
STEP_K = 3
STEP_SCALE = 0.03
STEP_CASES = {"coop-par": ((11, 3, 2, 2), 50, 3001), "cent-par": ((11, 3, 4, 2), 50, 3001)}


def step_case(name, B=47):
    """dict(cfg, arr, lin, u_old, oracle=(du, status, nwsr, ws, trace, ntrace),
    u_after, margin): one oracle step of K = 3 iterations from zero plans and
    empty working sets, the first move applied."""
    import _oracle as O
    key = ("step", name, B)
    if key not in _cache:
        dimset, p, seed = STEP_CASES[name]
        cfg = config_for(dimset, p)
        lin, u_old, arr = dense_problem(cfg, B, seed, scale=STEP_SCALE)
        nq = B * cfg.S
        u, du_old, ws, margin = u_old.copy(), np.zeros((nq, cfg.nV)), np.zeros(nq, np.uint32), np.zeros(nq)
        du, st, nw, tr, ntr = O.step(dims_of(cfg, B), arr, lin, STEP_K, u, du_old, ws, flags=cmpc.CMPC_APPLY_MOVE,
                                     init=False, want_trace=True, margin=margin)
        _freeze(lin, u_old, du, st, nw, ws, tr, ntr, u, margin)
        _cache[key] = dict(cfg=cfg, arr=arr, lin=lin, u_old=u_old, oracle=(du, st, nw, ws, tr, ntr), u_after=u,
                           margin=margin)
    return _cache[key]


# ---------------------------------------------------------------------------
# per-scenario settings on dense data: offsets dy, profiles dref, per-slot
# weights and limits, the paired draw (tests/test_gpu_dense_scenarios.py;
# every condition the GPU file relies on is checked in test_dense_reference.py)
# ---------------------------------------------------------------------------

B_WAVE, B_ROWS = 5, 9    # 10 / 5 and 18 / 9 slots: refshift's workgroup of four rows and the row build's
#                          group of four scenarios both end partly filled
# The affine data's scale where a profile is in force: dref is Gaussian of unit
# size whatever the scale, so the shift g = Su' W dref keeps its size while f
# shrinks with the scale.  At 1 max|g| falls to 3e-4 max|f| in some slot and
# the subtraction f_unset - f_profile loses what the shift test is after;
# 0.12 at 1e-3 and 0.8 at 1e-4, so that max|g| >= 0.1 max|f| in every slot of
# every case (checked on the CPU).
SHIFT_SCALE = 1e-4

SCN_OFFSET_CASES = [(ds, 23, REF_DELAYS) for ds in DIM_SETS] + [((11, 3, 2, 2), 50, (0, 10, 0, 25))]
# a partial chunk of 16 steps, one exact chunk, a chunk plus one step, three chunks and two steps
SCN_PROFILE_CASES = ([(ds, p, REF_DELAYS) for ds in DIM_SETS for p in (7, 16, 17, 50)]
                     + [((11, 2, 2, 2), 64, (0, 2, 0, 63))])
SCN_WEIGHT_CASES = [(ds, p, REF_DELAYS) for ds in DIM_SETS for p in (7, 50)]
SCN_PREDICT_CASES = [(ds, p, REF_DELAYS) for ds in DIM_SETS for p in (16, 17)]
PAIR_DIMSET = (11, 3, 2, 2)
PAIR_HORIZONS = (50, 20, 45)   # test_gpu_build_pairing's three loop shapes


def scenario_case(dimset, p, delays=REF_DELAYS, B=B_WAVE, weights=False, paired=False, limits=False,
                  scale=SHIFT_SCALE, dref_scale=1.0, seed=None):
    """A dense problem with per-slot settings, everything read-only:
    dict(cfg, arr, lin, u_old, dy (nq, ny), dref (nq, p, ny), ywt, uwt (per
    slot, or None: the shared ones), limits (four (nq, nu), or None), key).
    dy is Gaussian times scale like the other affine data, dref Gaussian times
    dref_scale; per-slot weights are _spd_dense draws; per-slot limits are the
    setup file's times U(0.3, 1) per slot with u_old inside the slot's own."""
    seed = case_seed(dimset, p, delays) if seed is None else seed
    key = ("scenario", tuple(dimset), p, tuple(delays), B, weights, paired, limits, scale, dref_scale, seed)
    if key not in _cache:
        cfg = config_for(dimset, p, delays)
        nq = B * cfg.S
        rng = np.random.default_rng(seed + 70001)     # the settings' own generator: the records are dense_problem's
        lscale = rng.uniform(0.3, 1.0, (nq, 1)) if limits else None
        lin, u_old, arr = dense_problem(cfg, B, seed, scale=scale, paired=paired, limit_scale=lscale)
        assert_dense(cfg, lin, u_old, arr)
        if paired:
            assert_paired(cfg, lin, u_old, arr)
        dy = np.ascontiguousarray(_nonzero(scale * rng.standard_normal((nq, cfg.ny))))
        dref = np.ascontiguousarray(_nonzero(dref_scale * rng.standard_normal((nq, p, cfg.ny))))
        ywt = uwt = lim = None
        if weights:
            ywt = np.ascontiguousarray(np.stack([_spd_dense(rng, cfg.ny) for _ in range(nq)]))
            uwt = np.ascontiguousarray(np.stack([_spd_dense(rng, cfg.nu) for _ in range(nq)]))
            _freeze(ywt, uwt)
        if limits:
            lim = slot_limits(cfg, arr, lscale)
            _freeze(*lim)
            own = u_old[:, :cfg.nu]
            assert np.all(own > lim[0]) and np.all(own < lim[1]), "u_old outside the slot's own limits"
        _freeze(lin, u_old, dy, dref, arr.ywt, arr.uwt, arr.y_ref)
        _cache[key] = dict(cfg=cfg, arr=arr, lin=lin, u_old=u_old, dy=dy, dref=dref, ywt=ywt, uwt=uwt, limits=lim,
                           key=key)
    return _cache[key]


def slot_oracle_qps(cfg, arr, lin, u_old, ywt=None, uwt=None, dy=None, dref=None):
    """The oracle's H, f, G slot by slot with the slot's weights and y_ref + dy + dref"""
    import weights_ref as WR
    uw, yw = WR.shared_weights(cfg, arr, lin.shape[0])
    return WR.oracle_qps(cfg, arr, lin, u_old, uw if uwt is None else uwt, yw if ywt is None else ywt, dy, dref)


def scenario_refs(c, dy=False, dref=False, weights=True):
    """The long-double and the oracle's QPs of a scenario_case with its weights
    (weights=False: the shared ones) and the chosen parts of the reference in
    force: dict(ref=(H, f, G), gram, oracle=(H, f, G), ratios)."""
    key = ("refs", c["key"], dy, dref, weights)
    if key not in _cache:
        kw = dict(ywt=c["ywt"] if weights else None, uwt=c["uwt"] if weights else None,
                  dy=c["dy"] if dy else None, dref=c["dref"] if dref else None)
        Hr, fr, Gr, gram = ref_qp(c["cfg"], c["lin"], c["u_old"], c["arr"], **kw)
        Ho, fo, Go = slot_oracle_qps(c["cfg"], c["arr"], c["lin"], c["u_old"], **kw)
        _freeze(Hr, fr, Gr, gram, Ho, fo, Go)
        _cache[key] = dict(ref=(Hr, fr, Gr), gram=gram, oracle=(Ho, fo, Go),
                           ratios=qp_error_ratios(Ho, fo, Go, Hr, fr, Gr, gram))
    return _cache[key]


def scenario_shift(c, weights=True):
    """g = Su' W dref of a scenario_case three ways, each (nq, nV): the
    long-double ref_shift, the oracle's Su' w (refprofile_ref.oracle_g) and the
    numpy backward sweep refshift.hip is modelled on (refprofile_ref.sweep_g)."""
    import refprofile_ref as RP
    key = ("shift", c["key"], weights)
    if key not in _cache:
        cfg, lin = c["cfg"], c["lin"]
        nq = lin.shape[0]
        ywt = c["ywt"] if weights and c["ywt"] is not None else c["arr"].ywt[np.arange(nq) % cfg.S]
        g = ref_shift(cfg, lin, c["u_old"], c["arr"], c["dref"], ywt)
        dims, L = dims_of(cfg, 1), Layout(cfg)
        go = np.stack([RP.oracle_g(cfg, dims, lin[q], ywt[q], c["dref"][q]) for q in range(nq)])
        gs = np.stack([RP.sweep_g(cfg, dims, L, lin[q], ywt[q], c["dref"][q]) for q in range(nq)])
        _freeze(g, go, gs)
        _cache[key] = dict(g=g, oracle_g=go, sweep_g=gs)
    return _cache[key]


def shift_error_ratio(g, gref):
    """Worst |g - gref| / (1e-11 max|gref[q]|) over the slots (the bar of
    test_gpu_reference_profile.py); <= 1 passes"""
    return max(float(np.abs(g[q] - gref[q]).max() / (1e-11 * np.abs(gref[q]).max())) for q in range(gref.shape[0]))


def shift_to_f(fref, g):
    """Smallest max|g[q]| / max|f[q]| over the slots, f the larger of the linear
    term with and without the profile: what the shift test's subtraction of two
    f's keeps of g"""
    out = np.inf
    for q in range(g.shape[0]):
        sf = max(float(np.abs(fref[q]).max()), float(np.abs(fref[q] + g[q]).max()))
        out = min(out, float(np.abs(g[q]).max()) / sf)
    return out


def pair_case(p, B=B_ROWS):
    """The paired draw (par-coop, reference delays) with dy, dref and per-slot limits"""
    return scenario_case(PAIR_DIMSET, p, B=B, paired=True, limits=True)


PAIR_ALTERED = (2, 8)


def pair_altered_case(p=50, B=B_ROWS):
    """pair_case with one entry of slot 1's A raised by one ulp in the scenarios
    PAIR_ALTERED, and the long-double and oracle's QPs of the altered records:
    dict(lin, ref=(H, f, G), gram, oracle)"""
    key = ("pair-altered", p, B)
    if key not in _cache:
        c = pair_case(p, B)
        cfg = c["cfg"]
        lin = c["lin"].copy()
        for i, b in enumerate(PAIR_ALTERED):
            e = 7 + 13 * i    # some entry of A (ns * ns = 121 of them)
            lin[2 * b + 1, e] = np.nextafter(lin[2 * b + 1, e], np.inf)
        assert (lin != c["lin"]).sum() == len(PAIR_ALTERED)
        Hr, fr, Gr, gram = ref_qp(cfg, lin, c["u_old"], c["arr"])
        ora = slot_oracle_qps(cfg, c["arr"], lin, c["u_old"])
        _freeze(lin, Hr, fr, Gr, gram, *ora)
        _cache[key] = dict(lin=lin, ref=(Hr, fr, Gr), gram=gram, oracle=ora)
    return _cache[key]


def scenario_predict_case(dimset, p, delays=REF_DELAYS, B=B_WAVE, weights=True):
    """A scenario_case (weights, dy and dref all in force) with predict_case's
    plans and the long-double predictions and costs of (du, d) and
    (du, d_gathered) under the slot's weights and y_ref + dy + dref."""
    import predict_ref as PR
    key = ("scenario-predict", tuple(dimset), p, tuple(delays), B, weights)
    if key not in _cache:
        c = scenario_case(dimset, p, delays, B, weights=weights)
        cfg, L = c["cfg"], Layout(c["cfg"])
        nq = B * cfg.S
        rng = np.random.default_rng(case_seed(dimset, p, delays) + 1)    # predict_case's draw
        du = np.ascontiguousarray(rng.standard_normal((nq, L.nV)))
        d = np.ascontiguousarray(rng.standard_normal((nq, L.nVo)))
        dg = np.ascontiguousarray(PR.gather_other(cfg, du))
        kw = dict(ywt=c["ywt"], uwt=c["uwt"], dy=c["dy"], dref=c["dref"])
        Y, J = ref_prediction(cfg, c["lin"], c["u_old"], c["arr"], du, d, **kw)
        Yg, Jg = ref_prediction(cfg, c["lin"], c["u_old"], c["arr"], du, dg, **kw) if L.nVo else (Y, J)
        _freeze(du, d, dg, Y, J, Yg, Jg)
        _cache[key] = dict(c, du=du, d=d, d_gathered=dg, given=(Y, J), gathered=(Yg, Jg))
    return _cache[key]


def slot_oracle_predictions(c, du, d):
    """The oracle's y_pred (nq, p, ny) and costs (nq, 2) with the slot's weights
    and y_ref + dy + dref (predict_ref.oracle_batch takes the shared weights)"""
    import _oracle as O
    import predict_ref as PR
    cfg, arr, lin = c["cfg"], c["arr"], c["lin"]
    dims = dims_of(cfg, 1)
    Lo = O.layout(dims)
    nq = lin.shape[0]
    Y, J = np.zeros((nq, cfg.p, cfg.ny)), np.zeros((nq, 2))
    for q in range(nq):
        s = q % cfg.S
        Y[q] = PR.oracle_prediction(dims, Lo, lin[q], c["u_old"][q], du[q], d[q])
        yr = np.asarray(arr.y_ref[s]).reshape(cfg.p, cfg.ny) + c["dy"][q] + c["dref"][q]
        J[q] = PR.costs(cfg, Y[q], du[q], yr, arr.ywt[s] if c["ywt"] is None else c["ywt"][q],
                        arr.uwt[s] if c["uwt"] is None else c["uwt"][q])
    return Y, J


# The step cases with per-slot settings (cmpc_step, K = 3, B = 9): per-slot
# limits and dy everywhere, the paired draw with dref as well.  Seed and scale
# are chosen so that step_case's conditions hold (test_dense_reference.py): a
# quarter or more of the QPs end with an active constraint, no oracle decision
# within NEAR_TIE, every status 0, and at least one slot ends on a limit of its
# own that differs from the shared one.
SCN_STEP_SCALE = 0.03
SCN_STEP_CASES = {"pair": ((11, 3, 2, 2), 50, 4006, True), "coop-par": ((11, 3, 2, 2), 50, 4007, False),
                  "cent-par": ((11, 3, 4, 2), 50, 4010, False)}


def scenario_step_case(name, B=B_ROWS):
    """dict(scenario_case..., profile (whether dref is in force), oracle=(du,
    status, nwsr, ws, trace, ntrace), u_after, margin): the oracle's step of
    K = 3 iterations from zero plans and empty working sets, the first move
    applied, run scenario by scenario with the scenario's own reference
    y_ref + dy (+ dref) and limits as its shared ones."""
    import dataclasses
    import _oracle as O
    key = ("scenario-step", name, B)
    if key not in _cache:
        dimset, p, seed, paired = SCN_STEP_CASES[name]
        c = scenario_case(dimset, p, B=B, paired=paired, limits=True, scale=SCN_STEP_SCALE,
                          dref_scale=SCN_STEP_SCALE, seed=seed)
        cfg, arr, lin = c["cfg"], c["arr"], c["lin"]
        S, nq = cfg.S, B * cfg.S
        dims = dims_of(cfg, 1)
        u, ws, margin = c["u_old"].copy(), np.zeros(nq, np.uint32), np.zeros(nq)
        out = []
        for b in range(B):
            sl = slice(b * S, (b + 1) * S)
            yr = arr.y_ref.reshape(S, p, cfg.ny) + c["dy"][sl][:, None, :]
            if paired:
                yr = yr + c["dref"][sl]
            lim = [np.ascontiguousarray(a[sl]) for a in c["limits"]]
            a_b = dataclasses.replace(arr, y_ref=np.ascontiguousarray(yr.reshape(S, -1)), lower=lim[0], upper=lim[1],
                                      rate_lower=lim[2], rate_upper=lim[3])
            u_b, ws_b, mg_b = np.ascontiguousarray(u[sl]), np.zeros(S, np.uint32), np.zeros(S)
            out.append(O.step(dims, a_b, np.ascontiguousarray(lin[sl]), STEP_K, u_b, np.zeros((S, cfg.nV)), ws_b,
                              flags=cmpc.CMPC_APPLY_MOVE, init=False, want_trace=True, margin=mg_b))
            u[sl], ws[sl], margin[sl] = u_b, ws_b, mg_b
        du, st, nw, tr, ntr = (np.concatenate([o[i] for o in out]) for i in range(5))
        _freeze(du, st, nw, ws, tr, ntr, u, margin)
        _cache[key] = dict(c, profile=paired, oracle=(du, st, nw, ws, tr, ntr), u_after=u, margin=margin)
    return _cache[key]


def on_own_limit(cfg, c, du):
    """Per slot: whether the plan du (nq, nV) sits on one of the slot's own
    limits whose value differs from the sub-controller's shared one: a move
    block at lower - u_old or upper - u_old (the solver sets those exactly), or
    a rate row (the first block, or a block less the one before it) at a rate
    limit to 1e-12."""
    nq, nu, m, arr = du.shape[0], cfg.nu, cfg.m, c["arr"]
    lo, up, rlo, rup = c["limits"]
    s_of = np.arange(nq) % cfg.S
    x = du.reshape(nq, m, nu)
    own = c["u_old"][:, None, :nu]
    rows = x - np.concatenate([np.zeros((nq, 1, nu)), x[:, :-1, :]], axis=1)
    hit = np.zeros(nq, bool)
    for mine, shared in ((lo, arr.lower), (up, arr.upper)):
        at = x == mine[:, None, :] - own
        hit |= (at & (mine != shared[s_of])[:, None, :]).any(axis=(1, 2))
    for mine, shared in ((rlo, arr.rate_lower), (rup, arr.rate_upper)):
        at = np.abs(rows - mine[:, None, :]) <= 1e-12 * np.abs(mine[:, None, :])
        hit |= (at & (mine != shared[s_of])[:, None, :]).any(axis=(1, 2))
    return hit
