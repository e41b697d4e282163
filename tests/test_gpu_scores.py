"""Closed-loop performance indices on the device (include/cmpc.h, cmpc_score_*;
score.hip) against the float64 numpy model tests/score_ref.py.  Marked gpu;
runs on an MI355X.

Every field but j_track and j_move must equal the model bit for bit (plain
FP64 multiplies and adds in the written order on both sides).  j_track and
j_move are compared at rtol 1e-12 with 1/2 e' ywt e and 1/2 du' uwt du
evaluated directly in numpy: both are sums of non-negative terms over at most
30 steps, so the forward error is a few dozen ulp (~1e-14); 1e-12 leaves two
to three orders of margin and is 1e4 below any indexing mistake.

The batch of the kernel tests (problem()): B scenarios of cmpc.synthetic
records, 6 steps of build + iterate (K = 3, CMPC_APPLY_MOVE) on the same
records, so u_old moves and the QPs change from step to step.  What each slot
or scenario carries:
  limits (bound per slot, not validated), by slot q:
    q % 7 == 1   position window [u_old0 + 0.02, u_old0 + 0.0201] on both own
                 inputs, wide rates: the first move sits on a bound (bit c)
    q % 7 == 2   wide positions, rate window [1e-3, 1.1e-3]: the first move
                 sits on its rate row (bit nV + c)
    q % 23 == 5  lower = 1 > upper = -1: CMPC_QP_INFEASIBLE, a zero move
    else         the sub-controller's own limits
  measured outputs y[k][b] = target centre + amp[k][b] * U(-1, 1), by scenario:
    b % 3 == 0   amp 1 for k < 3, 1e-3 after: last_out ends in 0..2
    b % 3 == 1   amp 1e-3 throughout: no output ever leaves its band (>= 0.1)
    b % 3 == 2   amp 1 throughout
  plant status: scenario 2 fails (1) from step 3 on, the last scenario (3)
  from step 0 on, the rest never."""
import functools
import types

import numpy as np
import pytest

import cmpc
import golden_cases as GC
from cmpc.synthetic import synthetic_batch
from score_ref import EXACT, FIELDS, ScoreMirror
from weights_ref import draw_weights

pytestmark = pytest.mark.gpu

STEPS, K, TS = 6, 3, 0.05
N_OUT = 4
CASES = ["coop-par", "cent-ser"]     # S = 2, ny = 3, nu = 2 and S = 1, ny = 4, nu = 4
SENTINEL = np.array([0x5EA1ED0FF1CEB0B0], dtype=np.uint64).view(np.float64)[0]   # a finite double


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")   # (a copy: the inputs are read-only)


@functools.lru_cache(maxsize=None)
def problem(name, B):
    """The host data of one batch (module docstring); everything read-only."""
    cfg, setup, arr, g = GC.case(name, p=50)
    S, ny, nu, p = cfg.S, cfg.ny, cfg.nu, cfg.p
    nq = B * S
    lin, u_old, du_old, ws = synthetic_batch(cfg, B, seed=2100 + B, n_distinct=min(B, 7))
    rng = np.random.default_rng(4242 + B)
    yref0 = np.stack([np.asarray(arr.y_ref[s]).reshape(p, ny)[0] for s in range(S)])    # (S, ny)
    full = np.zeros(N_OUT)
    for s in range(S):
        full[list(cfg.out_idx[s][:ny])] = yref0[s]
    dyb = rng.uniform(-0.05, 0.05, (B, N_OUT)) * np.maximum(np.abs(full), 0.1)
    dy = cmpc.scenario_reference_offsets(cfg, dyb)                                      # (nq, ny)
    target = np.ascontiguousarray(yref0[np.arange(nq) % S] + dy)                        # y_ref[s][0] + dy_ref[q]
    amp = np.ones((STEPS, B))
    amp[3:, np.arange(B) % 3 == 0] = 1e-3
    amp[:, np.arange(B) % 3 == 1] = 1e-3
    y = (full + dyb)[None] + amp[:, :, None] * rng.uniform(-1.0, 1.0, (STEPS, B, N_OUT))
    band = 0.1 * (1.0 + 0.5 * np.arange(ny))[None, :] + 0.01 * np.arange(S)[:, None]    # (S, ny), all distinct
    lim = np.zeros((nq, 4, nu))
    for q in range(nq):
        s = q % S
        lim[q] = [arr.lower[s], arr.upper[s], arr.rate_lower[s], arr.rate_upper[s]]
        if q % 7 == 1:
            lim[q] = [u_old[q, :nu] + 0.02, u_old[q, :nu] + 0.0201, np.full(nu, -1.0), np.full(nu, 1.0)]
        elif q % 7 == 2:
            lim[q] = [np.full(nu, -10.0), np.full(nu, 10.0), np.full(nu, 1e-3), np.full(nu, 1.1e-3)]
        if q % 23 == 5:
            lim[q, 0], lim[q, 1] = 1.0, -1.0
    plant = np.zeros((STEPS, B), np.int32)
    if B > 2:
        plant[3:, 2] = 1
    plant[:, B - 1] = 3
    P = types.SimpleNamespace(
        name=name, cfg=cfg, arr=arr, B=B, nq=nq, lin=lin, u_old=u_old, du_old=du_old, ws=ws, dy=dy, target=target,
        y=np.ascontiguousarray(y), band=np.ascontiguousarray(band), lim=np.ascontiguousarray(lim), plant=plant,
        u_ctrl=rng.uniform(-1, 1, (STEPS, B, cfg.nu_tot)), x=rng.uniform(-1, 1, (STEPS, B, cfg.ns)),
        ywt=np.ascontiguousarray(arr.ywt[np.arange(nq) % S]), uwt=np.ascontiguousarray(arr.uwt[np.arange(nq) % S]))
    for a in vars(P).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return P


def subset(P, bs):
    """The scenarios bs of P as a batch of their own."""
    S = P.cfg.S
    bs = np.asarray(bs)
    qs = (bs[:, None] * S + np.arange(S)).ravel()
    Q = types.SimpleNamespace(**vars(P))
    Q.B, Q.nq = len(bs), len(qs)
    for k in ("lin", "u_old", "du_old", "ws", "dy", "target", "lim", "ywt", "uwt"):
        setattr(Q, k, np.ascontiguousarray(getattr(P, k)[qs]))
    for k in ("y", "plant", "u_ctrl", "x"):
        setattr(Q, k, np.ascontiguousarray(getattr(P, k)[:, bs]))
    return Q


def run_gpu(P, n_steps=STEPS, weights=None, targets=None, capture=None, t_cap=0, guard=0, bound_state=False,
            again=False, then=None):
    """n_steps of build + iterate + score_step on a fresh context.  weights:
    (uwt, ywt) per slot; targets: (n_steps, nq, ny) explicit targets; capture:
    scenario list; guard: doubles of sentinel on either side of a bound score
    record (and capture buffer); again: restore the state, reset and run the
    same steps once more; then(ctx): called before the context closes.
    Returns the final record (len, nq), the per-step downloads, the capture
    and whether the guard words survived."""
    import torch
    cfg = P.cfg
    out = types.SimpleNamespace(steps=[], cap=None, guard_ok=None)
    with cmpc.Context(cfg, P.B) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.configure(P.arr)
        ctx.upload_lin(P.lin)
        ctx.set_scenario_reference(P.dy)
        lim_d = dev(P.lim)
        ctx.bind_scenario_constraints(lim_d.data_ptr())
        if weights is not None:
            ctx.set_scenario_weights(*weights)
        state = None
        if bound_state:   # the working-set words are then read from the caller's array
            state = (dev(P.u_old), dev(P.du_old), torch.from_numpy(P.ws.astype(np.int32)).to("cuda:0"))
            ctx.bind_state(*[t.data_ptr() for t in state])
        ctx.score_enable(N_OUT, band=P.band, Ts=TS)
        n = cmpc.score_len(ctx.dims) * P.nq
        big = cbig = None
        if guard:
            big = torch.full((guard + n + guard,), float(SENTINEL), dtype=torch.float64, device="cuda:0")
            ctx.score_bind(big.data_ptr() + 8 * guard)
        if capture is not None:
            ctx.score_capture(capture, t_cap)
            if guard:
                nc = t_cap * len(capture) * (N_OUT + cfg.nu_tot + cfg.ns)
                cbig = torch.full((guard + nc + guard,), float(SENTINEL), dtype=torch.float64, device="cuda:0")
                cbig[guard:guard + nc] = 0.0
                ctx.score_bind_capture(cbig.data_ptr() + 8 * guard)
        y_d, pl_d, u_d, x_d = dev(P.y), dev(P.plant), dev(P.u_ctrl), dev(P.x)
        tg_d = None if targets is None else dev(targets)
        for rep in range(2 if again else 1):
            if state is None:
                ctx.set_state(P.u_old, P.du_old, P.ws)
            else:
                for t, a in zip(state, (P.u_old, P.du_old, P.ws.astype(np.int32))):
                    t.copy_(torch.from_numpy(np.array(a, order="C")))
            ctx.score_reset()
            out.steps = []
            for k in range(n_steps):
                ctx.build()
                ctx.iterate(K, cmpc.CMPC_APPLY_MOVE)
                ctx.score_step(y_d[k].data_ptr(), 0 if tg_d is None else tg_d[k].data_ptr(), pl_d[k].data_ptr(),
                               u_d[k].data_ptr(), x_d[k].data_ptr())
                du, st, nw = ctx.download()
                ws = ctx.get_state()[2] if state is None else state[2].cpu().numpy().view(np.uint32)
                out.steps.append((du, st, nw, ws.copy()))
            rec = ctx.score_download()
            if rep == 0:
                out.rec = rec
            else:
                out.rec_again = rec
        if capture is not None:
            out.cap = ctx.score_download_capture()
        if guard:
            iv = lambda t: t.view(torch.int64).cpu().numpy()
            sent = np.array([SENTINEL]).view(np.int64)[0]
            b = iv(big)
            out.guard_ok = bool((b[:guard] == sent).all() and (b[guard + n:] == sent).all())
            assert np.array_equal(b[guard:guard + n].view(np.float64), out.rec.ravel())
            if cbig is not None:
                c = iv(cbig)
                out.guard_ok = out.guard_ok and bool((c[:guard] == sent).all() and (c[-guard:] == sent).all())
        if then is not None:
            then(ctx)
    return out


def mirror_of(P, steps, targets=None, ywt=None, uwt=None):
    cfg = P.cfg
    m = ScoreMirror(P.B, cfg.S, cfg.ny, cfg.nu, cfg.nV, cfg.out_idx, TS, P.band)
    for k, (du, st, nw, ws) in enumerate(steps):
        m.step(P.y[k], P.target if targets is None else targets[k], du, st, nw, ws,
               P.ywt if ywt is None else ywt, P.uwt if uwt is None else uwt, plant_status=P.plant[k])
    return m


def assert_record(rec, m, fields, what=""):
    """rec (len, nq) against the model under the module docstring's rules;
    prints each field's worst figure before asserting."""
    want = m.record(fields)
    for name in FIELDS:
        a, b = rec[fields[name]], want[fields[name]]
        if name in EXACT:
            nbad = int((a.view(np.int64) != b.view(np.int64)).sum())
            print(f"{what}{name}: {nbad} of {a.size} values differ from the model")
            assert nbad == 0, name
        else:
            rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
            rel[(a == 0) & (b == 0)] = 0.0
            print(f"{what}{name}: max relative difference {rel.max():.3e}")
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, err_msg=name)


# ---- 1. the kernel against the model --------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_gpu_scores_match_model(name):
    """B = 70: 140 or 70 slots, two full waves and a partial one; with S = 2 a
    scenario's two slots straddle each wave boundary (slots 63 | 64, 127 | 128)."""
    P = problem(name, 70)
    cfg = P.cfg
    r = run_gpu(P)
    m = mirror_of(P, r.steps)
    nu, nV = cfg.nu, cfg.nV
    st = np.stack([s[1] for s in r.steps])
    ws = np.stack([s[3] for s in r.steps]).astype(np.int64)
    ok = st == 0
    own = (1 << nu) - 1
    lo = m.f["last_out"]
    print(f"{name}: slots with a bound bit {int((ok & ((ws & own) != 0)).any(0).sum())}, a rate bit "
          f"{int((ok & (((ws >> nV) & own) != 0)).any(0).sum())}, a failed solve {int((~ok).any(0).sum())}, "
          f"last_out inside the run {int(((lo > -1) & (lo < STEPS - 1)).any(1).sum())}, "
          f"never out of band {int((lo == -1).any(1).sum())}")
    # the case is not vacuous (module docstring: which slots carry which case)
    assert (ok & ((ws & own) != 0)).any(), "no bound bit"
    assert (ok & (((ws >> nV) & own) != 0)).any(), "no rate bit"
    assert (~ok).any() and (st[:, 5] == cmpc.CMPC_QP_INFEASIBLE).all(), "no failed solve"
    assert ((lo > -1) & (lo < STEPS - 1)).any(), "no last_out inside the run"
    assert (lo == -1).any(), "every output left its band"
    assert (m.f["sat_bound"] > 0).any() and (m.f["sat_rate"] > 0).any() and (m.f["n_fail"] == STEPS).any()
    assert set(np.unique(m.f["plant_fail_step"])) == {-1.0, 0.0, 3.0}
    assert (m.f["j_move"] > 0).any() and (m.f["j_track"] > 0).all()
    assert_record(r.rec, m, cmpc.score_fields(cmpc.CmpcDims.from_config(cfg, P.B)), what=name + " ")


# ---- 2. weights and targets -------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_gpu_scores_follow_slot_weights_and_targets(name):
    P = problem(name, 9)
    cfg = P.cfg
    fields = cmpc.score_fields(cmpc.CmpcDims.from_config(cfg, P.B))
    base = run_gpu(P, bound_state=True)      # ws read from a bound state array
    assert_record(base.rec, mirror_of(P, base.steps), fields, what=name + " shared ")
    # per-slot weights: dense SPD ywt, symmetric uwt
    uwt, ywt = draw_weights(np.random.default_rng(31), cfg, P.arr, P.nq)
    w = run_gpu(P, weights=(uwt, ywt))
    mw = mirror_of(P, w.steps, ywt=ywt, uwt=uwt)
    assert_record(w.rec, mw, fields, what=name + " per-slot weights ")
    # ... and not the shared ones: the same steps' data under the shared weights
    ms = mirror_of(P, w.steps)
    for f in ("j_track", "j_move"):
        a, b = mw.f[f], ms.f[f]
        live = b > 0     # (a failed solve's zero moves cost nothing under any weight)
        rel = np.abs(a - b)[live] / b[live]
        print(f"{name} {f}: per-slot against shared weights, min relative difference {rel.min():.3e}")
        assert live.any() and (rel > 1e-6).all(), f
    # an explicit target: the errors follow it, not y_ref + dy_ref
    tg = np.ascontiguousarray(P.target[None] + np.random.default_rng(32).uniform(0.05, 0.3, (STEPS,) + P.target.shape))
    t = run_gpu(P, targets=tg)
    mt = mirror_of(P, t.steps, targets=tg)
    assert_record(t.rec, mt, fields, what=name + " explicit target ")
    m0 = mirror_of(P, t.steps)
    assert (mt.f["ise"] != m0.f["ise"]).all() and (mt.f["peak"] != m0.f["peak"]).all()


# ---- 3. guard band ------------------------------------------------------------------

@pytest.mark.parametrize("B", [70, 1])
@pytest.mark.parametrize("name", CASES)
def test_gpu_scores_stay_inside_their_buffers(name, B):
    """The record bound into the middle of a sentinel-filled tensor, 3 steps;
    the capture buffer likewise through t_cap = 2 with 5 steps."""
    P = problem(name, 70) if B == 70 else subset(problem(name, 70), [37])
    cfg = P.cfg
    r = run_gpu(P, n_steps=3, guard=64)
    assert r.guard_ok
    assert (r.rec[cmpc.score_fields(cmpc.CmpcDims.from_config(cfg, P.B))["n"]] == 3).all()
    sel = [0] if B == 1 else [69, 0, 37]
    c = run_gpu(P, n_steps=5, guard=64, capture=sel, t_cap=2)
    assert c.guard_ok
    rows, n = c.cap
    assert n == 2 and rows.shape == (2, len(sel), N_OUT + cfg.nu_tot + cfg.ns)
    want = np.concatenate([P.y[:2][:, sel], P.u_ctrl[:2][:, sel], P.x[:2][:, sel]], axis=2)
    assert np.array_equal(rows, want)


# ---- 4. independence and reset -----------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_gpu_scores_scenario_alone_and_reset(name):
    P = problem(name, 70)
    S = P.cfg.S
    refused = []

    def disabled(ctx):
        ctx.score_disable()
        with pytest.raises(RuntimeError, match="not enabled"):
            ctx.score_step(1)
        with pytest.raises(RuntimeError, match="not enabled"):
            ctx.score_download()
        refused.append(True)

    full = run_gpu(P, again=True, then=disabled)
    assert refused
    assert np.array_equal(full.rec.view(np.int64), full.rec_again.view(np.int64))   # reset + the same steps
    one = run_gpu(subset(P, [37]))
    assert one.rec.shape[1] == S
    assert np.array_equal(one.rec.view(np.int64), full.rec[:, 37 * S:38 * S].view(np.int64))
    fields = cmpc.score_fields(cmpc.CmpcDims.from_config(P.cfg, 1))
    assert (one.rec[fields["ise"]] > 0).all() and (one.rec[fields["n"]] == STEPS).all()   # (a live record)


def test_gpu_score_step_needs_a_solve_and_y():
    P = problem("coop-par", 9)
    with cmpc.Context(P.cfg, P.B) as ctx:
        ctx.configure(P.arr)
        with pytest.raises(RuntimeError, match="not enabled"):
            ctx.score_step(1)
        ctx.score_enable(N_OUT, Ts=TS)
        y = dev(P.y[0])
        with pytest.raises(RuntimeError, match="no solve"):
            ctx.score_step(y.data_ptr())
        with pytest.raises(RuntimeError, match="null y"):
            ctx.score_step(0)
        host = np.zeros(cmpc.score_len(ctx.dims) * P.nq)
        with pytest.raises(RuntimeError, match="cmpc_score_bind"):
            ctx.score_bind(host.ctypes.data)                 # host memory
        buf = dev(np.zeros(host.size + 1))
        with pytest.raises(RuntimeError, match="misaligned"):
            ctx.score_bind(buf.data_ptr() + 4)
        ctx.score_bind(buf.data_ptr() + 8)
        ctx.score_bind(0)
        with pytest.raises(RuntimeError, match="capture"):
            ctx.score_download_capture()


# ---- 5. the closed loop ----------------------------------------------------------------

def loop_inputs(name, B=6, n=30):
    cfg, setup, arr, g = GC.case(name, p=50)
    x0, u_def = cmpc.plant_default(cfg.plant)
    S, nu, nut = cfg.S, cfg.nu, cfg.nu_tot
    lim = np.zeros((4, B, nut))
    for s in range(S):
        own = cfg.input_order[s][:nu]
        for i, a in enumerate((arr.lower, arr.upper, arr.rate_lower, arr.rate_upper)):
            lim[i][:, own] = a[s]
    lim[2:, 1] *= 0.02          # scenarios 1 and 4: rates tight enough to saturate
    lim[2:, 4] *= 0.05
    lim[1, 2] = 0.002           # scenario 2: a low ceiling on every input
    sched = np.zeros((B, n + 5, N_OUT))
    sched[:, 10:, 3] = 0.02 * (1.0 + 0.25 * np.arange(B))[:, None]    # output 3 steps at instant 10
    yo = np.zeros((B, N_OUT))
    yo[:, 3] = 0.005 * np.arange(B)
    return cfg, arr, g["n_iterations"], x0, u_def, lim, sched, yo


@pytest.mark.parametrize("name", CASES)
def test_gpu_closed_loop_scores(name):
    from cmpc.driver import ClosedLoop
    B, n = 6, 30
    cfg, arr, Kl, x0, u_def, lim, sched, yo = loop_inputs(name, B, n)
    S, ny, p = cfg.S, cfg.ny, cfg.p
    M = cmpc.reference_observer_gain(cfg)
    band = np.full((S, ny), 1e-3)
    sel = [0, 5, 3]

    def make(scored):
        loop = ClosedLoop(cfg, arr, [M] * S, np.tile(x0, (B, 1)), np.tile(u_def, (B, 1)), Kl, y_offset=yo,
                          limits=tuple(lim))
        loop.set_setpoint_schedule(sched)
        if scored:
            loop.enable_scores(band=band, capture=sel, capture_steps=n)
        loop.initialize()
        return loop

    a, b = make(True), make(False)
    try:
        yref0 = np.stack([np.asarray(arr.y_ref[s]).reshape(p, ny)[0] for s in range(S)])
        dy = cmpc.scenario_reference_offsets(cfg, yo)
        base = yref0[np.arange(B * S) % S] + dy
        oi = np.asarray(cfg.out_idx)[:, :ny]
        m = ScoreMirror(B, S, ny, cfg.nu, cfg.nV, cfg.out_idx, a.Ts, band)
        ywt, uwt = arr.ywt[np.arange(B * S) % S], arr.uwt[np.arange(B * S) % S]
        ys, us, xs = [], [], []
        for k in range(n):
            xb, _, _, pst = b.sim.download()           # the instant's state and status, before the step
            _, ya = a.step()
            ua = a.u_ctrl.cpu().numpy()
            ya = ya.cpu().numpy().copy()
            _, yb = b.step()
            yb, ub = yb.cpu().numpy().copy(), b.u_ctrl.cpu().numpy()
            # scoring changes nothing the loop computes
            assert np.array_equal(ya.view(np.int64), yb.view(np.int64)), k
            assert np.array_equal(ua.view(np.int64), ub.view(np.int64)), k
            du, st, nw = b.ctx.download()
            ws = b.ctx.get_state()[2]
            tgt = base + sched[:, min(k, sched.shape[1] - 1)][:, oi].reshape(B * S, ny)
            m.step(yb, tgt, du, st, nw, ws, ywt, uwt, plant_status=pst)
            ys.append(yb); us.append(ub); xs.append(xb)
        sc = a.scores()
        fields = a.ctx.score_fields()
        assert_record(a.ctx.score_download(), m, fields, what=name + " loop ")
        for f in FIELDS:
            want = m.f[f].reshape((B, S) + m.f[f].shape[1:])
            assert sc[f].shape == want.shape, f
            if f in EXACT:
                assert np.array_equal(sc[f], want), f
        assert np.array_equal(sc["settling_time"], (sc["last_out"] + 1.0) * a.Ts)
        print(f"{name}: saturated steps per scenario {sc['sat_bound'].sum((1, 2)) + sc['sat_rate'].sum((1, 2))}, "
              f"settling time of the stepped output {sc['settling_time'][:, :, -1].ravel()}")
        assert (sc["n"] == n).all()
        assert (sc["sat_bound"].sum((1, 2)) + sc["sat_rate"].sum((1, 2)) > 0).any(), "no scenario saturates"
        o3 = [list(cfg.out_idx[s][:ny]).index(3) for s in range(S)]
        for s in range(S):
            stl = sc["settling_time"][:, s, o3[s]]
            assert np.isfinite(stl).all() and (stl > 10 * a.Ts).all(), stl
        t, yc, uc, xc = a.captured()
        assert np.array_equal(t, np.arange(n) * a.Ts)
        assert np.array_equal(yc, np.stack(ys)[:, sel]) and np.array_equal(uc, np.stack(us)[:, sel])
        assert np.array_equal(xc, np.stack(xs)[:, sel])
        # initialize resets the record
        a.initialize()
        assert (a.scores()["n"] == 0).all() and (a.scores()["last_out"] == -1).all()
        assert a.captured()[0].size == 0
    finally:
        a.close()
        b.close()


# ---- 6. enable_scores refuses bad arguments ----------------------------------------------

def test_gpu_enable_scores_argument_refusals():
    from cmpc.driver import ClosedLoop
    cfg, arr, Kl, x0, u_def, lim, sched, yo = loop_inputs("coop-par")
    B = 6
    M = cmpc.reference_observer_gain(cfg)
    loop = ClosedLoop(cfg, arr, [M] * cfg.S, np.tile(x0, (B, 1)), np.tile(u_def, (B, 1)), Kl)
    try:
        bad = [dict(band=np.zeros((cfg.S, cfg.ny + 1))), dict(band=np.zeros(cfg.ny)),
               dict(band=-np.ones((cfg.S, cfg.ny))), dict(band=np.full((cfg.S, cfg.ny), np.nan)),
               dict(capture=[0, 3, 0], capture_steps=4), dict(capture=[0, 6], capture_steps=4),
               dict(capture=[-1], capture_steps=4), dict(capture=[1, 2], capture_steps=0),
               dict(capture=[[1, 2]], capture_steps=4), dict(capture=[0.5], capture_steps=4)]
        for kw in bad:
            with pytest.raises(ValueError):
                loop.enable_scores(**kw)
            with pytest.raises(RuntimeError, match="not enabled"):    # nothing was enabled or allocated
                loop.ctx.score_reset()
        loop.initialize()
        loop.step()          # a loop that never enables scoring steps as before
        with pytest.raises(RuntimeError, match="not enabled"):
            loop.scores()
        loop.enable_scores()
        loop.initialize()
        loop.step()
        assert (loop.scores()["n"] == 1).all()
        with pytest.raises(RuntimeError, match="capture"):
            loop.captured()
    finally:
        loop.close()
