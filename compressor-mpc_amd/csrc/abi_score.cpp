// Closed-loop performance indices of the C ABI (include/cmpc.h): the score
// record, its ensemble statistics and exact quantiles, and the envelope.
#include "abi_ctx.h"

#include <algorithm>
#include <cmath>

#include "ensemble_select.h"

using namespace cmpc_abi;

extern "C" {

// Closed-loop performance indices (include/cmpc.h, score.hip).
static const struct {
  const char* name;
  int ScoreFields::*row;
  int per;  // rows: 0 one, 1 ny, 2 nu
} kScoreFields[] = {
    {"n", &ScoreFields::n, 0},           {"ise", &ScoreFields::ise, 1},
    {"iae", &ScoreFields::iae, 1},       {"peak", &ScoreFields::peak, 1},
    {"last_out", &ScoreFields::last_out, 1}, {"j_track", &ScoreFields::j_track, 0},
    {"j_move", &ScoreFields::j_move, 0}, {"tv", &ScoreFields::tv, 2},
    {"sat_bound", &ScoreFields::sat_bound, 2}, {"sat_rate", &ScoreFields::sat_rate, 2},
    {"n_fail", &ScoreFields::n_fail, 0}, {"nwsr_sum", &ScoreFields::nwsr_sum, 0},
    {"plant_fail_step", &ScoreFields::plant_fail_step, 0},
};

int cmpc_score_len(const cmpc_dims* dims) {
  cmpc_layout L;
  if (!dims) return fail("null argument");
  if (layout_of(dims, &L)) return -1;
  return cmpc_score_fields(dims->ny, dims->nu).len;
}

int cmpc_score_field(const cmpc_dims* dims, const char* name, int* offset, int* count) {
  cmpc_layout L;
  if (!dims || !name) return fail("null argument");
  if (layout_of(dims, &L)) return -1;
  const ScoreFields F = cmpc_score_fields(dims->ny, dims->nu);
  for (const auto& f : kScoreFields)
    if (!std::strcmp(name, f.name)) {
      if (offset) *offset = F.*(f.row);
      if (count) *count = f.per == 0 ? 1 : f.per == 1 ? dims->ny : dims->nu;
      return 0;
    }
  return fail(std::string("cmpc_score_field: no field named '") + name + "'");
}

int cmpc_score_check(const cmpc_dims* dims, int n_outputs, const int32_t* out_idx, double Ts, const double* band) {
  cmpc_layout L;
  if (!dims || !out_idx) return fail("cmpc_score_enable: null argument");
  if (layout_of(dims, &L)) return -1;
  if (!cmpc_score_instance(dims->ny, dims->nu))
    return fail("cmpc_score_enable: score kernel not instantiated for these dimensions (ny, nu)");
  if (n_outputs < 1) return fail("cmpc_score_enable: n_outputs must be >= 1");
  if (!std::isfinite(Ts) || Ts < 0) return fail("cmpc_score_enable: Ts must be finite and >= 0");
  for (int i = 0; i < dims->S * dims->ny; ++i) {
    if (out_idx[i] < 0 || out_idx[i] >= n_outputs)
      return fail("cmpc_score_enable: sub-controller " + std::to_string(i / dims->ny) +
                  ": out_idx outside [0, n_outputs)");
    if (band && (!std::isfinite(band[i]) || band[i] < 0))
      return fail("cmpc_score_enable: sub-controller " + std::to_string(i / dims->ny) +
                  ": band must be finite and >= 0");
  }
  return 0;
}

int cmpc_score_capture_check(const cmpc_dims* dims, int n_sel, const int32_t* scenarios, int t_cap) {
  cmpc_layout L;
  if (!dims) return fail("cmpc_score_capture: null argument");
  if (layout_of(dims, &L)) return -1;
  if (n_sel < 0) return fail("cmpc_score_capture: n_sel must be >= 0");
  if (n_sel == 0) return 0;
  if (!scenarios) return fail("cmpc_score_capture: null scenario list");
  if (t_cap < 1) return fail("cmpc_score_capture: t_cap must be >= 1");
  if (n_sel > dims->B) return fail("cmpc_score_capture: more scenarios than the batch holds");
  for (int i = 0; i < n_sel; ++i) {
    if (scenarios[i] < 0 || scenarios[i] >= dims->B)
      return fail("cmpc_score_capture: scenario " + std::to_string(scenarios[i]) + " outside [0, B)");
    for (int j = 0; j < i; ++j)
      if (scenarios[j] == scenarios[i])
        return fail("cmpc_score_capture: scenario " + std::to_string(scenarios[i]) + " given twice");
  }
  return 0;
}

static int score_cap_width(const cmpc_ctx* c) { return c->score_nout + c->d.nu_tot + c->d.ns; }

static void score_capture_free(cmpc_ctx* c) {
  if (c->score_map) (void)hipFree(c->score_map);
  if (c->score_cap_own) (void)hipFree(c->score_cap_own);
  c->score_map = nullptr;
  c->score_cap_own = c->score_cap = nullptr;
  c->score_nsel = c->score_tcap = 0;
}

int cmpc_score_reset(cmpc_ctx* c) {
  if (!c) return fail("null context");
  if (!c->score_on) return fail("cmpc_score_reset: scoring is not enabled (cmpc_score_enable)");
  HIP_TRY(hipSetDevice(c->device));
  if (cmpc_launch_score_reset(c->score_rec, c->nqp, c->d.ny, c->d.nu, c->stream))
    return fail("cmpc_score_reset: launch failed");
  if (check_launch("score reset kernel")) return -1;
  if (c->score_cap_own && c->score_cap == c->score_cap_own)
    HIP_TRY(hipMemsetAsync(c->score_cap_own, 0,
                           sizeof(double) * (size_t)c->score_tcap * c->score_nsel * score_cap_width(c), c->stream));
  c->score_k = 0;
  return 0;
}

int cmpc_score_enable(cmpc_ctx* c, int n_outputs, const int32_t* out_idx, double Ts, const double* band) {
  if (!c) return fail("null context");
  if (cmpc_score_check(&c->d, n_outputs, out_idx, Ts, band)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  const size_t m = (size_t)c->d.S * c->d.ny;
  if (c->score_on && n_outputs != c->score_nout) score_capture_free(c);  // (its row width has changed)
  if (!c->score_band) HIP_TRY(hipMalloc(&c->score_band, sizeof(double) * m));
  if (!c->score_oi) HIP_TRY(hipMalloc(&c->score_oi, sizeof(int32_t) * m));
  if (!c->score_own)
    HIP_TRY(hipMalloc(&c->score_own, sizeof(double) * (size_t)cmpc_score_fields(c->d.ny, c->d.nu).len * c->nqp));
  if (ensure_yref(c)) return -1;
  std::vector<double> hb(m, 0.0);
  if (band) std::copy(band, band + m, hb.begin());
  HIP_TRY(hipMemcpyAsync(c->score_band, hb.data(), sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->score_oi, out_idx, sizeof(int32_t) * m, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!c->score_rec) c->score_rec = c->score_own;
  c->score_nout = n_outputs;
  c->score_Ts = Ts;
  c->score_on = true;
  return cmpc_score_reset(c);
}

int cmpc_score_bind(cmpc_ctx* c, double* scores_device) {
  if (!c) return fail("null context");
  if (!c->score_on) return fail("cmpc_score_bind: scoring is not enabled (cmpc_score_enable)");
  if (scores_device &&
      bound_array_check(c, scores_device, "cmpc_score_bind",
                        (size_t)cmpc_score_fields(c->d.ny, c->d.nu).len * c->nqp, "len * nqp"))
    return -1;
  c->score_rec = scores_device ? scores_device : c->score_own;
  return 0;
}

int cmpc_score_capture(cmpc_ctx* c, int n_sel, const int32_t* scenarios, int t_cap) {
  if (!c) return fail("null context");
  if (!c->score_on) return fail("cmpc_score_capture: scoring is not enabled (cmpc_score_enable)");
  if (cmpc_score_capture_check(&c->d, n_sel, scenarios, t_cap)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  score_capture_free(c);
  if (n_sel == 0) return 0;
  std::vector<int32_t> map((size_t)c->d.B, -1);
  for (int i = 0; i < n_sel; ++i) map[scenarios[i]] = i;
  const size_t rows = sizeof(double) * (size_t)t_cap * n_sel * score_cap_width(c);
  HIP_TRY(hipMalloc(&c->score_map, sizeof(int32_t) * map.size()));
  HIP_TRY(hipMalloc(&c->score_cap_own, rows));
  HIP_TRY(hipMemcpyAsync(c->score_map, map.data(), sizeof(int32_t) * map.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->score_cap_own, 0, rows, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->score_cap = c->score_cap_own;
  c->score_nsel = n_sel;
  c->score_tcap = t_cap;
  return 0;
}

int cmpc_score_bind_capture(cmpc_ctx* c, double* rows_device) {
  if (!c) return fail("null context");
  if (!c->score_on || !c->score_nsel)
    return fail("cmpc_score_bind_capture: no capture is enabled (cmpc_score_capture)");
  if (rows_device &&
      bound_array_check(c, rows_device, "cmpc_score_bind_capture",
                        (size_t)c->score_tcap * c->score_nsel * score_cap_width(c), "t_cap * n_sel * width"))
    return -1;
  c->score_cap = rows_device ? rows_device : c->score_cap_own;
  return 0;
}

int cmpc_score_step(cmpc_ctx* c, const double* y, const double* target, const int32_t* plant_status,
                    const double* u_control, const double* x) {
  if (!c) return fail("null context");
  if (!c->score_on) return fail("cmpc_score_step: scoring is not enabled (cmpc_score_enable)");
  if (!y) return fail("cmpc_score_step: null y");
  if (!c->last_solve) return fail("cmpc_score_step: no solve has run (cmpc_iterate, cmpc_step, cmpc_control_step)");
  if (c->score_k >= INT32_MAX) return fail("cmpc_score_step: step count overflow (cmpc_score_reset)");
  if (ensure_cfg(c)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  if (!target && ensure_yref(c)) return -1;  // (allocated by cmpc_score_enable; a copy when the references changed)
  ScoreParams P;
  std::memset(&P, 0, sizeof P);
  P.rec = c->score_rec;
  P.y = y;
  P.target = target;
  P.cfg = c->cfg;
  P.yref = c->d_yref;
  P.dy_ref = c->sc_dy;
  P.sc_w = c->sc_w;
  P.du = c->du;  // (page-locked host memory up to CMPC_HOST_OUT_MAX_QP slots: its device address)
  P.status = c->status;
  P.nwsr = c->nwsr;
  P.ws = c->ws;
  P.plant_status = plant_status;
  P.out_idx = c->score_oi;
  P.band = c->score_band;
  if (c->score_nsel) {
    P.cap_map = c->score_map;
    P.cap = c->score_cap;
    P.u_control = u_control;
    P.x = x;
    P.n_sel = c->score_nsel;
    P.t_cap = c->score_tcap;
    P.cap_w = score_cap_width(c);
  }
  P.n_out = c->score_nout;
  P.nu_tot = c->d.nu_tot;
  P.ns = c->d.ns;
  P.nqp = c->nqp;
  P.S = c->d.S;
  P.p = c->d.p;
  P.nV = c->L.nV;
  P.k = (int)c->score_k;
  P.Ts = c->score_Ts;
  P.co = c->co;
  if (cmpc_launch_score(P, c->d.ny, c->d.nu, c->stream)) return plan_mismatch("score");
  if (check_launch("score kernel")) return -1;
  c->score_k++;
  return 0;
}

int cmpc_score_download(cmpc_ctx* c, double* scores) {
  if (!c || !scores) return fail("null argument");
  if (!c->score_on) return fail("cmpc_score_download: scoring is not enabled (cmpc_score_enable)");
  HIP_TRY(hipSetDevice(c->device));
  return direct_download(
      c->stream, {{c->score_rec, scores, sizeof(double) * (size_t)cmpc_score_fields(c->d.ny, c->d.nu).len * c->nqp}});
}

int cmpc_score_download_capture(cmpc_ctx* c, double* rows, int32_t* n_rows) {
  if (!c) return fail("null context");
  if (!c->score_on || !c->score_nsel)
    return fail("cmpc_score_download_capture: no capture is enabled (cmpc_score_capture)");
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = sizeof(double) * (size_t)c->score_tcap * c->score_nsel * score_cap_width(c);
  if (direct_download(c->stream, {{c->score_cap, rows, bytes}})) return -1;
  if (n_rows) *n_rows = (int32_t)std::min<int64_t>(c->score_k, c->score_tcap);
  return 0;
}

int cmpc_score_disable(cmpc_ctx* c) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  score_capture_free(c);
  if (c->score_band) (void)hipFree(c->score_band);
  if (c->score_oi) (void)hipFree(c->score_oi);
  if (c->score_own) (void)hipFree(c->score_own);
  c->score_band = nullptr;
  c->score_oi = nullptr;
  c->score_own = c->score_rec = nullptr;
  c->score_on = false;
  c->score_k = 0;
  return 0;
}

// Ensemble statistics of the score record (include/cmpc.h, score_ensemble.hip).
int cmpc_score_ensemble(cmpc_ctx* c, const double* thresholds, double* out) {
  if (!c || !out) return fail("cmpc_score_ensemble: null argument");
  if (!c->score_on) return fail("cmpc_score_ensemble: scoring is not enabled (cmpc_score_enable)");
  const int len = cmpc_score_fields(c->d.ny, c->d.nu).len, S = c->d.S;
  if (thresholds)
    for (int f = 0; f < len; ++f)
      if (std::isnan(thresholds[f]))
        return fail("cmpc_score_ensemble: threshold of row " + std::to_string(f) + " is not a number");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->score_ens_work.p) HIP_TRY(hipMalloc(&c->score_ens_work.p, cmpc_score_ensemble_bytes(len, S)));
  void* work = c->score_ens_work.p;
  if (thresholds)
    HIP_TRY(hipMemcpyAsync(cmpc_score_ensemble_thresholds(work, len, S), thresholds, sizeof(double) * len,
                           hipMemcpyHostToDevice, c->stream));
  if (cmpc_launch_score_ensemble(c->score_rec, len, c->d.B, S, thresholds != nullptr, work, c->stream))
    return plan_mismatch("score ensemble");
  if (check_launch("score ensemble kernels")) return -1;
  return direct_download(c->stream, {{work, out, sizeof(double) * (size_t)len * S * kScoreEnsembleStats}});
}

// Exact ensemble quantiles and the envelope (include/cmpc.h, ensemble_select.h,
// ensemble_quantiles.hip).
static int quantile_levels_check(const char* who, int n_levels, int n_min, const double* levels) {
  if (n_levels < n_min || n_levels > CMPC_QUANTILE_MAX_LEVELS)
    return fail(std::string(who) + ": n_levels must be inside [" + std::to_string(n_min) + ", " +
                std::to_string(CMPC_QUANTILE_MAX_LEVELS) + "]");
  if (n_levels > 0 && !levels) return fail(std::string(who) + ": null levels");
  for (int l = 0; l < n_levels; ++l)
    if (!(levels[l] >= 0.0 && levels[l] <= 1.0))
      return fail(std::string(who) + ": level " + std::to_string(l) + " must be inside [0, 1]");
  return 0;
}

static QuantileRanks quantile_ranks(int B, int n_levels, const double* levels, double* g) {
  QuantileRanks R{};
  R.n = n_levels;
  for (int l = 0; l < n_levels; ++l) {
    double gl;
    cmpc_select_rank(B, levels[l], &R.k_lo[l], &R.k_hi[l], &gl);
    if (g) g[l] = gl;
  }
  return R;
}

int cmpc_quantile_check(int B, int n_levels, const double* levels) {
  if (B < 1) return fail("cmpc_quantile: B must be >= 1");
  return quantile_levels_check("cmpc_quantile", n_levels, 1, levels);
}

int cmpc_quantile_rank(int B, double level, int32_t* k_lo, int32_t* k_hi, double* g) {
  if (!k_lo || !k_hi || !g) return fail("cmpc_quantile_rank: null argument");
  if (cmpc_quantile_check(B, 1, &level)) return -1;
  uint32_t lo, hi;
  cmpc_select_rank(B, level, &lo, &hi, g);
  *k_lo = (int32_t)lo;
  *k_hi = (int32_t)hi;
  return 0;
}

double cmpc_quantile_value(double x_lo, double x_hi, double g) { return cmpc_select_interpolate(x_lo, x_hi, g); }

int cmpc_quantiles_host(const double* x, int len, int B, int S, int n_levels, const double* levels, double* out) {
  if (!x || !out) return fail("cmpc_quantiles_host: null argument");
  if (cmpc_quantile_check(B, n_levels, levels)) return -1;
  if (len < 1 || S < 1) return fail("cmpc_quantiles_host: len and S must be >= 1");
  const QuantileRanks R = quantile_ranks(B, n_levels, levels, nullptr);
  for (int f = 0; f < len; ++f)
    for (int s = 0; s < S; ++s)
      cmpc_select_row_host(x + (size_t)f * B * S + s, (size_t)S, B, n_levels, R.k_lo, R.k_hi,
                           out + ((size_t)f * S + s) * n_levels * 3);
  return 0;
}

int cmpc_score_quantiles(cmpc_ctx* c, int n_levels, const double* levels, double* out) {
  if (!c || !out) return fail("cmpc_score_quantiles: null argument");
  if (!c->score_on) return fail("cmpc_score_quantiles: scoring is not enabled (cmpc_score_enable)");
  if (cmpc_quantile_check(c->d.B, n_levels, levels)) return -1;
  const int len = cmpc_score_fields(c->d.ny, c->d.nu).len, S = c->d.S, B = c->d.B;
  if ((size_t)len * S > 65535) return fail("cmpc_score_quantiles: more rows than one launch covers");
  const int rows = len * S;
  HIP_TRY(hipSetDevice(c->device));
  if (!c->quant_work.p)
    HIP_TRY(hipMalloc(&c->quant_work.p, cmpc_quantile_work_bytes(rows, B, CMPC_QUANTILE_MAX_LEVELS)));
  void* work = c->quant_work.p;
  EnsRowMap M{};
  M.p0 = c->score_rec;
  M.fstride0 = (int64_t)B * S;
  M.rows0 = rows;
  M.S0 = S;
  const QuantileRanks R = quantile_ranks(B, n_levels, levels, nullptr);
  const QuantileOut O{static_cast<double*>(work), (int64_t)n_levels * 3, 3};
  if (cmpc_launch_quantiles(M, B, R, O, work, c->stream)) return plan_mismatch("score quantiles");
  if (check_launch("quantile kernels")) return -1;
  return direct_download(c->stream, {{O.out, out, sizeof(double) * (size_t)rows * n_levels * 3}});
}

static int envelope_width(int n_levels) { return kScoreEnsembleStats + 2 * n_levels; }

int cmpc_envelope_check(const cmpc_dims* dims, int n_outputs, int t_cap, int n_levels, const double* levels,
                        const double* thresholds) {
  cmpc_layout L;
  if (!dims) return fail("cmpc_envelope_enable: null argument");
  if (layout_of(dims, &L)) return -1;
  if (n_outputs < 1) return fail("cmpc_envelope_enable: n_outputs must be >= 1");
  if (t_cap < 1) return fail("cmpc_envelope_enable: t_cap must be >= 1");
  if (quantile_levels_check("cmpc_envelope_enable", n_levels, 0, levels)) return -1;
  if ((int64_t)n_outputs + dims->nu_tot > 65535)
    return fail("cmpc_envelope_enable: more channels than one launch covers");
  for (int ch = 0; thresholds && ch < n_outputs + dims->nu_tot; ++ch)
    if (std::isnan(thresholds[ch]))
      return fail("cmpc_envelope_enable: threshold of channel " + std::to_string(ch) + " is not a number");
  return 0;
}

int cmpc_envelope_len(const cmpc_dims* dims, int n_outputs, int n_levels) {
  cmpc_layout L;
  if (!dims) return fail("cmpc_envelope_len: null argument");
  if (layout_of(dims, &L)) return -1;
  if (n_outputs < 1 || n_levels < 0 || n_levels > CMPC_QUANTILE_MAX_LEVELS ||
      (int64_t)n_outputs + dims->nu_tot > 65535)
    return fail("cmpc_envelope_len: n_outputs or n_levels outside the limits");
  return (n_outputs + dims->nu_tot) * envelope_width(n_levels);
}

static size_t envelope_row_len(const cmpc_ctx* c) {
  return (size_t)(c->env_nout + c->d.nu_tot) * envelope_width(c->env_ranks.n);
}

static void envelope_free(cmpc_ctx* c) {
  for (auto* b : {&c->env_thr, &c->env_mom_work, &c->env_quant_work, &c->env_own}) {
    if (b->p) (void)hipFree(b->p);
    b->p = nullptr;
  }
  c->env_rows = nullptr;
  c->env_on = false;
  c->env_k = 0;
}

int cmpc_envelope_disable(cmpc_ctx* c) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  envelope_free(c);
  return 0;
}

int cmpc_envelope_enable(cmpc_ctx* c, int n_outputs, int t_cap, int n_levels, const double* levels,
                         const double* thresholds) {
  if (!c) return fail("null context");
  if (cmpc_envelope_check(&c->d, n_outputs, t_cap, n_levels, levels, thresholds)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  envelope_free(c);
  const int chans = n_outputs + c->d.nu_tot, B = c->d.B;
  c->env_nout = n_outputs;
  c->env_tcap = t_cap;
  c->env_ranks = quantile_ranks(B, n_levels, levels, nullptr);
  const size_t rows = sizeof(double) * (size_t)t_cap * envelope_row_len(c);
  HIP_TRY(hipMalloc(&c->env_own.p, rows));
  HIP_TRY(hipMemsetAsync(c->env_own.p, 0, rows, c->stream));
  HIP_TRY(hipMalloc(&c->env_mom_work.p, cmpc_envelope_moments_bytes(chans)));
  if (thresholds) {
    HIP_TRY(hipMalloc(&c->env_thr.p, sizeof(double) * chans));
    HIP_TRY(hipMemcpyAsync(c->env_thr.p, thresholds, sizeof(double) * chans, hipMemcpyHostToDevice, c->stream));
  }
  if (n_levels > 0) {
    // (a step without u_control covers n_outputs rows, with its own block count)
    const size_t bytes = std::max(cmpc_quantile_work_bytes(chans, B, n_levels),
                                  cmpc_quantile_work_bytes(n_outputs, B, n_levels));
    HIP_TRY(hipMalloc(&c->env_quant_work.p, bytes));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->env_rows = static_cast<double*>(c->env_own.p);
  c->env_k = 0;
  c->env_on = true;
  return 0;
}

int cmpc_envelope_reset(cmpc_ctx* c) {
  if (!c) return fail("null context");
  if (!c->env_on) return fail("cmpc_envelope_reset: no envelope is enabled (cmpc_envelope_enable)");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemsetAsync(c->env_own.p, 0, sizeof(double) * (size_t)c->env_tcap * envelope_row_len(c), c->stream));
  c->env_k = 0;
  return 0;
}

int cmpc_envelope_bind(cmpc_ctx* c, double* rows_device) {
  if (!c) return fail("null context");
  if (!c->env_on) return fail("cmpc_envelope_bind: no envelope is enabled (cmpc_envelope_enable)");
  if (rows_device && bound_array_check(c, rows_device, "cmpc_envelope_bind",
                                       (size_t)c->env_tcap * envelope_row_len(c), "t_cap * cmpc_envelope_len"))
    return -1;
  c->env_rows = rows_device ? rows_device : static_cast<double*>(c->env_own.p);
  return 0;
}

int cmpc_envelope_step(cmpc_ctx* c, const double* y, const double* u_control) {
  if (!c) return fail("null context");
  if (!c->env_on) return fail("cmpc_envelope_step: no envelope is enabled (cmpc_envelope_enable)");
  if (!y) return fail("cmpc_envelope_step: null y");
  if (c->env_k >= c->env_tcap) {  // dropped, as the capture drops its steps
    if (c->env_k < INT32_MAX) c->env_k++;
    return 0;
  }
  HIP_TRY(hipSetDevice(c->device));
  const int W = envelope_width(c->env_ranks.n);
  EnsRowMap M{};
  M.p0 = y;
  M.rows0 = M.S0 = c->env_nout;
  M.fstride0 = 0;
  if (u_control) {
    M.p1 = u_control;
    M.rows1 = M.S1 = c->d.nu_tot;
  }
  double* row = c->env_rows + (size_t)c->env_k * envelope_row_len(c);
  if (cmpc_launch_envelope_moments(M, c->d.B, static_cast<const double*>(c->env_thr.p), row, W, c->env_mom_work.p,
                                   c->stream))
    return plan_mismatch("envelope statistics");
  if (c->env_ranks.n > 0) {
    const QuantileOut O{row + kScoreEnsembleStats, W, 2};
    if (cmpc_launch_quantiles(M, c->d.B, c->env_ranks, O, c->env_quant_work.p, c->stream))
      return plan_mismatch("envelope quantiles");
  }
  if (check_launch("envelope kernels")) return -1;
  c->env_k++;
  return 0;
}

int cmpc_envelope_download(cmpc_ctx* c, double* rows, int32_t* n_rows) {
  if (!c) return fail("null context");
  if (!c->env_on) return fail("cmpc_envelope_download: no envelope is enabled (cmpc_envelope_enable)");
  HIP_TRY(hipSetDevice(c->device));
  if (direct_download(c->stream, {{c->env_rows, rows, sizeof(double) * (size_t)c->env_tcap * envelope_row_len(c)}}))
    return -1;
  if (n_rows) *n_rows = (int32_t)std::min<int64_t>(c->env_k, c->env_tcap);
  return 0;
}

}  // extern "C"
