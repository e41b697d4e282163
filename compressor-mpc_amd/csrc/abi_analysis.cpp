// Plant analysis of the C ABI (include/cmpc.h): equilibrium, steady-state
// target, gains, frequency responses, eigenvalues and modes.  Each has a host form over arrays, a
// device form over a simulator's scenarios (cmpc_sim_*) and that form's
// download.  The only translation unit of the ABI that includes the solvers'
// shared bodies (*_body.h); its host forms need no device.
#include <cmath>
#include <type_traits>

#include "abi_sim.h"
#include "eig_body.h"
#include "equilibrium_body.h"
#include "freq_body.h"
#include "gains_body.h"
#include "target_body.h"

using namespace cmpc_abi;

namespace {

// f(std::integral_constant<int, PLANT>) for the plant's template instance
template <class F>
auto for_plant(int plant, F&& f) {
  return plant == CMPC_PLANT_PARALLEL ? f(std::integral_constant<int, CMPC_PLANT_PARALLEL>{})
                                      : f(std::integral_constant<int, CMPC_PLANT_SERIAL>{});
}

// what every cmpc_plant_*_host checks of its batch: a known plant (its state
// and input counts returned), B >= 1, no null array
int plant_host_args(const char* who, int plant, int B, bool arrays, int* ns, int* ni) {
  int no = 0, nci = 0;
  if (cmpc_plant_dims(plant, ns, ni, &no, &nci)) return fail(std::string(who) + ": unknown plant");
  if (B < 1) return fail(std::string(who) + ": B must be >= 1");
  if (!arrays) return fail(std::string(who) + ": null argument");
  return 0;
}

// entry j of an index list: inside [0, 4) and none of the entries before it
int index_check(const char* who, const char* name, bool output, const int32_t* idx, int j) {
  if (idx[j] < 0 || idx[j] >= 4)
    return fail(std::string(who) + ": " + name + "[" + std::to_string(j) + "] is not a " +
                (output ? "plant output" : "control input") + " in [0, 4)");
  for (int i = 0; i < j; ++i)
    if (idx[i] == idx[j])
      return fail(std::string(who) + ": " + name + " repeats " + (output ? "output " : "control input ") +
                  std::to_string(idx[j]));
  return 0;
}

// the simulator's part of a launch parameter struct (the per-scenario
// instance reads scenario b's pressure pair at the launch)
template <class P>
void sim_fields(const cmpc_sim* m, P* p) {
  std::memset(p, 0, sizeof *p);
  p->x = m->x;
  p->u_full = m->u_full;
  p->sim_status = m->status;
  p->pressures = m->pr;
  p->B = m->B;
  p->p_in = m->p_in;
  p->p_out = m->p_out;
}

int equilibrium_check(const char* who, int max_iter, double tol) {
  if (max_iter < 0 || max_iter > CMPC_EQ_MAX_ITER)
    return fail(std::string(who) + ": max_iter must be in [0, " + std::to_string(CMPC_EQ_MAX_ITER) + "]");
  if (!std::isfinite(tol) || !(tol > 0)) return fail(std::string(who) + ": tol must be finite and positive");
  return 0;
}

int eig_check(const char* who, int max_iter) {
  if (max_iter < 1 || max_iter > CMPC_EIG_MAX_ITER)
    return fail(std::string(who) + ": max_iter must be in [1, " + std::to_string(CMPC_EIG_MAX_ITER) + "]");
  return 0;
}

template <int PLANT>
int plant_modes_one(double p_in, double p_out, const double* u, const double* x, int max_iter, double* wr,
                    double* wi, double* summary, int32_t* iters) {
  constexpr int ns = cmpc_eq::Dims<PLANT>::ns;
  double A[ns * ns], Bm[ns * 4], C[4 * ns], f[ns];
  cmpc_eq::eq_linearize<PLANT>(p_in, p_out, x, u, A, Bm, C, f);
  return cmpc_eig::eig_host_one<ns>(A, max_iter, wr, wi, iters, summary);
}

}  // namespace

extern "C" {

// Plant equilibrium (include/cmpc.h, equilibrium_body.h, equilibrium.hip)
int cmpc_plant_equilibrium_host(int plant, int B, const double* pressures, const double* u_full, double* x,
                                int max_iter, double tol, int32_t* status, int32_t* iters, double* resid) {
  int ns = 0, ni = 0;
  if (plant_host_args("cmpc_plant_equilibrium_host", plant, B, pressures && u_full && x && status && iters && resid,
                      &ns, &ni))
    return -1;
  if (equilibrium_check("cmpc_plant_equilibrium_host", max_iter, tol)) return -1;
  for (size_t b = 0; b < (size_t)B; ++b)
    status[b] = for_plant(plant, [&](auto pl) {
      return cmpc_eq::eq_solve<decltype(pl)::value>(pressures[2 * b], pressures[2 * b + 1], u_full + b * ni, x + b * ns,
                                         max_iter, tol, iters + b, resid + b);
    });
  return 0;
}

int cmpc_sim_equilibrium(cmpc_sim* m, int max_iter, double tol) {
  if (!m) return fail("cmpc_sim_equilibrium: null simulator");
  if (equilibrium_check("cmpc_sim_equilibrium", max_iter, tol)) return -1;
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  if (ensure_device(&m->eq_status, sizeof(int32_t) * Bz) || ensure_device(&m->eq_iters, sizeof(int32_t) * Bz) ||
      ensure_device(&m->eq_resid, sizeof(double) * Bz))
    return -1;
  EquilibriumParams P;
  sim_fields(m, &P);
  P.status = m->eq_status;
  P.iters = m->eq_iters;
  P.resid = m->eq_resid;
  P.max_iter = max_iter;
  P.tol = tol;
  if (cmpc_launch_equilibrium(P, m->plant, m->stream)) return fail("equilibrium launch failed");
  return check_launch("equilibrium kernel");
}

int cmpc_sim_equilibrium_download(cmpc_sim* m, int32_t* status, int32_t* iters, double* resid) {
  if (!m) return fail("cmpc_sim_equilibrium_download: null simulator");
  if (!m->eq_status) return fail("cmpc_sim_equilibrium_download: call cmpc_sim_equilibrium first");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  return pinned_download(m->pin_out, m->stream,
                         {{m->eq_resid, resid, sizeof(double) * Bz},
                          {m->eq_iters, iters, sizeof(int32_t) * Bz},
                          {m->eq_status, status, sizeof(int32_t) * Bz}});
}

int32_t* cmpc_sim_equilibrium_status(cmpc_sim* m) { return m ? m->eq_status : nullptr; }
int32_t* cmpc_sim_equilibrium_iters(cmpc_sim* m) { return m ? m->eq_iters : nullptr; }
double* cmpc_sim_equilibrium_resid(cmpc_sim* m) { return m ? m->eq_resid : nullptr; }

// Steady-state target solve (include/cmpc.h, target_body.h, target.hip)
int cmpc_target_check(int plant, int nh, const int32_t* hold_idx, const int32_t* free_idx, int max_iter,
                      double tol_f, double tol_y) {
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail("cmpc_target_check: unknown plant");
  if (nh < 0 || nh > cmpc_tg::kMaxHold)
    return fail("cmpc_target_check: nh must be in [0, " + std::to_string(cmpc_tg::kMaxHold) + "]");
  if (nh > 0 && (!hold_idx || !free_idx)) return fail("cmpc_target_check: null index array");
  for (int j = 0; j < nh; ++j)
    if (index_check("cmpc_target_check", "hold_idx", true, hold_idx, j) ||
        index_check("cmpc_target_check", "free_idx", false, free_idx, j))
      return -1;
  if (max_iter < 0 || max_iter > CMPC_EQ_MAX_ITER)
    return fail("cmpc_target_check: max_iter must be in [0, " + std::to_string(CMPC_EQ_MAX_ITER) + "]");
  if (!std::isfinite(tol_f) || !(tol_f > 0)) return fail("cmpc_target_check: tol_f must be finite and positive");
  if (!std::isfinite(tol_y) || !(tol_y > 0)) return fail("cmpc_target_check: tol_y must be finite and positive");
  return 0;
}

int cmpc_plant_target_host(int plant, int B, const double* pressures, int nh, const int32_t* hold_idx,
                           const int32_t* free_idx, const double* targets, double* u_full, double* x, int max_iter,
                           double tol_f, double tol_y, int32_t* status, int32_t* iters, double* resid) {
  if (cmpc_target_check(plant, nh, hold_idx, free_idx, max_iter, tol_f, tol_y)) return -1;
  int ns = 0, ni = 0;
  if (plant_host_args("cmpc_plant_target_host", plant, B,
                      pressures && u_full && x && status && iters && resid && (nh == 0 || targets), &ns, &ni))
    return -1;
  for (size_t b = 0; b < (size_t)B; ++b)
    status[b] = for_plant(plant, [&](auto pl) {
      return cmpc_tg::tg_solve<decltype(pl)::value>(pressures[2 * b], pressures[2 * b + 1], nh, hold_idx, free_idx,
                                         nh > 0 ? targets + b * nh : nullptr, u_full + b * ni, x + b * ns, max_iter,
                                         tol_f, tol_y, iters + b, resid + 2 * b);
    });
  return 0;
}

int cmpc_sim_target(cmpc_sim* m, int nh, const int32_t* hold_idx, const int32_t* free_idx,
                    const double* targets_device, int max_iter, double tol_f, double tol_y) {
  if (!m) return fail("cmpc_sim_target: null simulator");
  if (cmpc_target_check(m->plant, nh, hold_idx, free_idx, max_iter, tol_f, tol_y)) return -1;
  if (nh > 0 && !targets_device) return fail("cmpc_sim_target: null targets");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  if (ensure_device(&m->tg_status, sizeof(int32_t) * Bz) || ensure_device(&m->tg_iters, sizeof(int32_t) * Bz) ||
      ensure_device(&m->tg_resid, sizeof(double) * 2 * Bz))
    return -1;
  TargetParams P;
  sim_fields(m, &P);
  P.u_offset = m->u_offset;
  P.targets = nh > 0 ? targets_device : nullptr;
  P.status = m->tg_status;
  P.iters = m->tg_iters;
  P.resid = m->tg_resid;
  P.max_iter = max_iter;
  P.nh = nh;
  for (int j = 0; j < nh; ++j) {
    P.hold[j] = hold_idx[j];
    P.fre[j] = free_idx[j];
  }
  P.tol_f = tol_f;
  P.tol_y = tol_y;
  if (cmpc_launch_target(P, m->plant, m->stream)) return fail("target launch failed");
  return check_launch("target kernel");
}

int cmpc_sim_target_host(cmpc_sim* m, int nh, const int32_t* hold_idx, const int32_t* free_idx,
                         const double* targets, int max_iter, double tol_f, double tol_y) {
  if (!m) return fail("cmpc_sim_target_host: null simulator");
  if (cmpc_target_check(m->plant, nh, hold_idx, free_idx, max_iter, tol_f, tol_y)) return -1;
  if (nh > 0 && !targets) return fail("cmpc_sim_target_host: null targets");
  HIP_TRY(hipSetDevice(m->device));
  // the staging buffer holds 2 * max(ns, ni, no, nc) >= nh doubles per scenario
  if (nh > 0)
    HIP_TRY(hipMemcpyAsync(m->stage, targets, sizeof(double) * (size_t)m->B * nh, hipMemcpyHostToDevice, m->stream));
  const int rc = cmpc_sim_target(m, nh, hold_idx, free_idx, m->stage, max_iter, tol_f, tol_y);
  HIP_TRY(hipStreamSynchronize(m->stream));  // (the host array is free again)
  return rc;
}

int cmpc_sim_target_download(cmpc_sim* m, int32_t* status, int32_t* iters, double* resid) {
  if (!m) return fail("cmpc_sim_target_download: null simulator");
  if (!m->tg_status) return fail("cmpc_sim_target_download: call cmpc_sim_target first");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  return pinned_download(m->pin_out, m->stream,
                         {{m->tg_resid, resid, sizeof(double) * 2 * Bz},
                          {m->tg_iters, iters, sizeof(int32_t) * Bz},
                          {m->tg_status, status, sizeof(int32_t) * Bz}});
}

int32_t* cmpc_sim_target_status(cmpc_sim* m) { return m ? m->tg_status : nullptr; }
int32_t* cmpc_sim_target_iters(cmpc_sim* m) { return m ? m->tg_iters : nullptr; }
double* cmpc_sim_target_resid(cmpc_sim* m) { return m ? m->tg_resid : nullptr; }

// Steady-state gains, RGA and pressure feed-forward (include/cmpc.h, gains_body.h, gains.hip)
int cmpc_gain_check(int plant, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx) {
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail("cmpc_gain_check: unknown plant");
  if (ny < 1 || ny > cmpc_gn::kMaxSel)
    return fail("cmpc_gain_check: ny must be in [1, " + std::to_string(cmpc_gn::kMaxSel) + "]");
  if (nu < 1 || nu > cmpc_gn::kMaxSel)
    return fail("cmpc_gain_check: nu must be in [1, " + std::to_string(cmpc_gn::kMaxSel) + "]");
  if (!out_idx || !in_idx) return fail("cmpc_gain_check: null index array");
  for (int j = 0; j < ny; ++j)
    if (index_check("cmpc_gain_check", "out_idx", true, out_idx, j)) return -1;
  for (int j = 0; j < nu; ++j)
    if (index_check("cmpc_gain_check", "in_idx", false, in_idx, j)) return -1;
  return 0;
}

int cmpc_plant_gains_host(int plant, int B, const double* pressures, const double* u_full, const double* x, int ny,
                          const int32_t* out_idx, int nu, const int32_t* in_idx, double* record, int32_t* status) {
  if (cmpc_gain_check(plant, ny, out_idx, nu, in_idx)) return -1;
  int ns = 0, ni = 0;
  if (plant_host_args("cmpc_plant_gains_host", plant, B, pressures && u_full && x && record && status, &ns, &ni))
    return -1;
  for (size_t b = 0; b < (size_t)B; ++b)
    status[b] = for_plant(plant, [&](auto pl) {
      return cmpc_gn::gn_solve<decltype(pl)::value>(pressures[2 * b], pressures[2 * b + 1], ny, out_idx, nu, in_idx,
                                         u_full + b * ni, x + b * ns, record + b * CMPC_GAIN_LEN);
    });
  return 0;
}

int cmpc_sim_gains(cmpc_sim* m, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx) {
  if (!m) return fail("cmpc_sim_gains: null simulator");
  if (cmpc_gain_check(m->plant, ny, out_idx, nu, in_idx)) return -1;
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  if (ensure_device(&m->gn_record, sizeof(double) * CMPC_GAIN_LEN * Bz) ||
      ensure_device(&m->gn_status, sizeof(int32_t) * Bz))
    return -1;
  GainsParams P;
  sim_fields(m, &P);
  P.record = m->gn_record;
  P.status = m->gn_status;
  P.ny = ny;
  P.nu = nu;
  for (int j = 0; j < ny; ++j) P.out[j] = out_idx[j];
  for (int j = 0; j < nu; ++j) P.in[j] = in_idx[j];
  if (cmpc_launch_gains(P, m->plant, m->stream)) return fail("gains launch failed");
  return check_launch("gains kernel");
}

int cmpc_sim_gains_download(cmpc_sim* m, double* record, int32_t* status) {
  if (!m) return fail("cmpc_sim_gains_download: null simulator");
  if (!m->gn_status) return fail("cmpc_sim_gains_download: call cmpc_sim_gains first");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  return pinned_download(m->pin_out, m->stream,
                         {{m->gn_record, record, sizeof(double) * CMPC_GAIN_LEN * Bz},
                          {m->gn_status, status, sizeof(int32_t) * Bz}});
}

double* cmpc_sim_gains_record(cmpc_sim* m) { return m ? m->gn_record : nullptr; }
int32_t* cmpc_sim_gains_status(cmpc_sim* m) { return m ? m->gn_status : nullptr; }

// Plant frequency responses (include/cmpc.h, freq_body.h, freq.hip)
static int freq_list_check(const char* who, int nw, const double* omega) {
  if (nw < 1 || nw > cmpc_fq::kMaxNw)
    return fail(std::string(who) + ": nw must be in [1, " + std::to_string(cmpc_fq::kMaxNw) + "]");
  if (!omega) return fail(std::string(who) + ": null omega");
  for (int k = 0; k < nw; ++k)
    if (!std::isfinite(omega[k]) || omega[k] < 0)
      return fail(std::string(who) + ": omega[" + std::to_string(k) + "] must be finite and >= 0");
  return 0;
}

int cmpc_freq_check(int plant, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx, int nw,
                    const double* omega) {
  if (cmpc_gain_check(plant, ny, out_idx, nu, in_idx)) return fail("cmpc_freq_check: " + g_err);
  return freq_list_check("cmpc_freq_check", nw, omega);
}

int cmpc_plant_freq_host(int plant, int B, const double* pressures, const double* u_full, const double* x, int ny,
                         const int32_t* out_idx, int nu, const int32_t* in_idx, int nw, const double* omega,
                         double* record, double* summary, int32_t* status) {
  if (cmpc_freq_check(plant, ny, out_idx, nu, in_idx, nw, omega)) return -1;
  int ns = 0, ni = 0;
  if (plant_host_args("cmpc_plant_freq_host", plant, B, pressures && u_full && x && record && summary && status, &ns,
                      &ni))
    return -1;
  for (size_t b = 0; b < (size_t)B; ++b)
    status[b] = for_plant(plant, [&](auto pl) {
      return cmpc_fq::fq_solve<decltype(pl)::value>(pressures[2 * b], pressures[2 * b + 1], ny, out_idx, nu, in_idx,
                                         u_full + b * ni, x + b * ns, nw, omega, record + b * nw * CMPC_FREQ_LEN,
                                         summary + b * CMPC_FREQ_NSUM);
    });
  return 0;
}

int cmpc_freq_host(int n, int B, const double* A, const double* Bm, const double* C, const double* E, int ny, int nu,
                   int nw, const double* omega, double* record, double* summary, int32_t* status) {
  if (n < 1 || n > CMPC_FREQ_MAX_N)
    return fail("cmpc_freq_host: n must be in [1, " + std::to_string(CMPC_FREQ_MAX_N) + "]");
  if (B < 1) return fail("cmpc_freq_host: B must be >= 1");
  if (ny < 1 || ny > cmpc_gn::kMaxSel || nu < 1 || nu > cmpc_gn::kMaxSel)
    return fail("cmpc_freq_host: ny and nu must be in [1, " + std::to_string(cmpc_gn::kMaxSel) + "]");
  if (freq_list_check("cmpc_freq_host", nw, omega)) return -1;
  if (!A || !Bm || !C || !E || !record || !summary || !status) return fail("cmpc_freq_host: null argument");
  const size_t nz = (size_t)n;
  for (size_t b = 0; b < (size_t)B; ++b)
    status[b] = cmpc_fq::fq_host(n, A + b * nz * nz, Bm + b * nz * 4, C + b * 4 * nz, E + b * nz * 2, ny, nu, nw, omega,
                                 record + b * nw * CMPC_FREQ_LEN, summary + b * CMPC_FREQ_NSUM);
  return 0;
}

int cmpc_sim_freq(cmpc_sim* m, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx, int nw,
                  const double* omega_host) {
  if (!m) return fail("cmpc_sim_freq: null simulator");
  if (cmpc_freq_check(m->plant, ny, out_idx, nu, in_idx, nw, omega_host)) return -1;
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  if (ensure_device(&m->fq_omega, sizeof(double) * CMPC_FREQ_MAX_NW) ||
      ensure_device(&m->fq_summary, sizeof(double) * CMPC_FREQ_NSUM * Bz) ||
      ensure_device(&m->fq_status, sizeof(int32_t) * Bz))
    return -1;
  if (nw > m->fq_cap) {  // (hipFree waits for the work that may still read the old record)
    if (m->fq_record) HIP_TRY(hipFree(m->fq_record));
    m->fq_record = nullptr;
    m->fq_cap = m->fq_nw = 0;
    HIP_TRY(hipMalloc(&m->fq_record, sizeof(double) * CMPC_FREQ_LEN * Bz * nw));
    m->fq_cap = nw;
  }
  const size_t count = (size_t)nw;
  if (pinned_upload(m->pin_in, m->stream, m->fq_omega, &omega_host, &count, 1, nullptr)) return -1;
  FreqParams P;
  sim_fields(m, &P);
  P.omega = m->fq_omega;
  P.record = m->fq_record;
  P.summary = m->fq_summary;
  P.status = m->fq_status;
  P.ny = ny;
  P.nu = nu;
  P.nw = nw;
  for (int j = 0; j < ny; ++j) P.out[j] = out_idx[j];
  for (int j = 0; j < nu; ++j) P.in[j] = in_idx[j];
  m->fq_nw = nw;
  if (cmpc_launch_freq(P, m->plant, m->stream)) return fail("freq launch failed");
  return check_launch("freq kernel");
}

int cmpc_sim_freq_download(cmpc_sim* m, double* record, double* summary, int32_t* status) {
  if (!m) return fail("cmpc_sim_freq_download: null simulator");
  if (!m->fq_status || m->fq_nw < 1) return fail("cmpc_sim_freq_download: call cmpc_sim_freq first");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  // (a span without a host array takes no staging room: the record is the large one)
  return pinned_download(m->pin_out, m->stream,
                         {{m->fq_record, record, record ? sizeof(double) * CMPC_FREQ_LEN * Bz * m->fq_nw : 0},
                          {m->fq_summary, summary, sizeof(double) * CMPC_FREQ_NSUM * Bz},
                          {m->fq_status, status, sizeof(int32_t) * Bz}});
}

double* cmpc_sim_freq_record(cmpc_sim* m) { return m ? m->fq_record : nullptr; }
double* cmpc_sim_freq_summary(cmpc_sim* m) { return m ? m->fq_summary : nullptr; }
int32_t* cmpc_sim_freq_status(cmpc_sim* m) { return m ? m->fq_status : nullptr; }

// Eigenvalues and plant modes (include/cmpc.h, eig_body.h, eig.hip)
int cmpc_eig_host(int n, int B, const double* A, int max_iter, double* wr, double* wi, int32_t* status,
                  int32_t* iters) {
  if (n < 1 || n > CMPC_EIG_MAX_N)
    return fail("cmpc_eig_host: n must be in [1, " + std::to_string(CMPC_EIG_MAX_N) + "]");
  if (B < 1) return fail("cmpc_eig_host: B must be >= 1");
  if (!A || !wr || !wi || !status || !iters) return fail("cmpc_eig_host: null argument");
  if (eig_check("cmpc_eig_host", max_iter)) return -1;
  const size_t nz = (size_t)n;
  for (size_t b = 0; b < (size_t)B; ++b)
    status[b] = cmpc_eig::eig_host(n, A + b * nz * nz, max_iter, wr + b * nz, wi + b * nz, iters + b, nullptr);
  return 0;
}

int cmpc_eig_device(int n, int B, const double* A, int max_iter, double* wr, double* wi, int32_t* status,
                    int32_t* iters, void* stream) {
  if (n != 10 && n != 11) return fail("cmpc_eig_device: n must be 10 or 11");
  if (B < 1) return fail("cmpc_eig_device: B must be >= 1");
  if (!A || !wr || !wi || !status || !iters) return fail("cmpc_eig_device: null argument");
  if (eig_check("cmpc_eig_device", max_iter)) return -1;
  EigParams P;
  std::memset(&P, 0, sizeof P);
  P.A = A;
  P.wr = wr;
  P.wi = wi;
  P.status = status;
  P.iters = iters;
  P.B = B;
  P.max_iter = max_iter;
  if (cmpc_launch_eig(P, n, stream)) return fail("cmpc_eig_device: launch failed");
  return check_launch("eig kernel");
}

int cmpc_modes_summary_host(int n, int B, const double* wr, const double* wi, const int32_t* status,
                            double* summary) {
  if (n < 1 || n > CMPC_EIG_MAX_N)
    return fail("cmpc_modes_summary_host: n must be in [1, " + std::to_string(CMPC_EIG_MAX_N) + "]");
  if (B < 1) return fail("cmpc_modes_summary_host: B must be >= 1");
  if (!wr || !wi || !status || !summary) return fail("cmpc_modes_summary_host: null argument");
  for (size_t b = 0; b < (size_t)B; ++b)
    cmpc_eig::eig_summary(n, wr + b * n, wi + b * n, status[b] == CMPC_EIG_OK, summary + b * CMPC_MODES_NSUM);
  return 0;
}

int cmpc_plant_modes_host(int plant, int B, const double* pressures, const double* u_full, const double* x,
                          int max_iter, double* wr, double* wi, double* summary, int32_t* status, int32_t* iters) {
  int ns = 0, ni = 0;
  if (plant_host_args("cmpc_plant_modes_host", plant, B,
                      pressures && u_full && x && wr && wi && summary && status && iters, &ns, &ni))
    return -1;
  if (eig_check("cmpc_plant_modes_host", max_iter)) return -1;
  for (size_t b = 0; b < (size_t)B; ++b)
    status[b] = for_plant(plant, [&](auto pl) {
      return plant_modes_one<decltype(pl)::value>(pressures[2 * b], pressures[2 * b + 1], u_full + b * ni, x + b * ns, max_iter,
                                       wr + b * ns, wi + b * ns, summary + b * CMPC_MODES_NSUM, iters + b);
    });
  return 0;
}

int cmpc_sim_modes(cmpc_sim* m, int max_iter) {
  if (!m) return fail("cmpc_sim_modes: null simulator");
  if (eig_check("cmpc_sim_modes", max_iter)) return -1;
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  if (ensure_device(&m->md_wr, sizeof(double) * Bz * m->ns) || ensure_device(&m->md_wi, sizeof(double) * Bz * m->ns) ||
      ensure_device(&m->md_summary, sizeof(double) * Bz * CMPC_MODES_NSUM) ||
      ensure_device(&m->md_status, sizeof(int32_t) * Bz) || ensure_device(&m->md_iters, sizeof(int32_t) * Bz))
    return -1;
  ModesParams P;
  sim_fields(m, &P);
  P.wr = m->md_wr;
  P.wi = m->md_wi;
  P.summary = m->md_summary;
  P.status = m->md_status;
  P.iters = m->md_iters;
  P.max_iter = max_iter;
  if (cmpc_launch_modes(P, m->plant, m->stream)) return fail("modes launch failed");
  return check_launch("modes kernel");
}

int cmpc_sim_modes_download(cmpc_sim* m, double* wr, double* wi, double* summary, int32_t* status,
                            int32_t* iters) {
  if (!m) return fail("cmpc_sim_modes_download: null simulator");
  if (!m->md_status) return fail("cmpc_sim_modes_download: call cmpc_sim_modes first");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B, bw = sizeof(double) * Bz * m->ns;
  return pinned_download(m->pin_out, m->stream,
                         {{m->md_wr, wr, bw},
                          {m->md_wi, wi, bw},
                          {m->md_summary, summary, sizeof(double) * Bz * CMPC_MODES_NSUM},
                          {m->md_status, status, sizeof(int32_t) * Bz},
                          {m->md_iters, iters, sizeof(int32_t) * Bz}});
}

double* cmpc_sim_modes_wr(cmpc_sim* m) { return m ? m->md_wr : nullptr; }
double* cmpc_sim_modes_wi(cmpc_sim* m) { return m ? m->md_wi : nullptr; }
double* cmpc_sim_modes_summary(cmpc_sim* m) { return m ? m->md_summary : nullptr; }
int32_t* cmpc_sim_modes_status(cmpc_sim* m) { return m ? m->md_status : nullptr; }
int32_t* cmpc_sim_modes_iters(cmpc_sim* m) { return m ? m->md_iters : nullptr; }

}  // extern "C"
