// The plant simulator of the C ABI (include/cmpc.h): life, inputs, integration,
// pressures, outputs and downloads, with the host-array variants.
#include "abi_sim.h"

#include <algorithm>
#include <vector>

using namespace cmpc_abi;

extern "C" {

// releases everything the simulator owns: every device buffer, the staging
// buffers, its own stream (cmpc_sim_create's failure path and cmpc_sim_destroy)
static void sim_release(cmpc_sim* m) {
  pinned_free(m->pin_in);
  pinned_free(m->pin_out);
  void* bufs[] = {m->x, m->dt, m->u_full, m->u_offset, m->ring, m->scratch, m->stage, m->status, m->own_pr,
                  m->eq_status, m->eq_iters, m->eq_resid, m->tg_status, m->tg_iters, m->tg_resid, m->gn_record,
                  m->gn_status, m->fq_omega, m->fq_record, m->fq_summary, m->fq_status, m->md_wr, m->md_wi,
                  m->md_summary, m->md_status, m->md_iters};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
}

int cmpc_sim_create(cmpc_sim** out, int plant, int B, int device, double p_in, double p_out,
                    int n_control, const int32_t* delays, const int32_t* control_index) {
  if (!out || !delays || !control_index) return fail("null argument");
  *out = nullptr;
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail("cmpc_sim_create: unknown plant");
  if (B < 1 || B > (1 << 28)) return fail("cmpc_sim_create: bad batch");
  if (n_control < 1 || n_control > CMPC_MAX_INPUTS) return fail("cmpc_sim_create: bad n_control");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail("no such HIP device");
  cmpc_sim* m = new cmpc_sim();
  m->plant = plant; m->B = B; m->device = device; m->ns = ns; m->ni = ni; m->no = no;
  m->nc = n_control; m->p_in = p_in; m->p_out = p_out;
  for (int i = 0; i < n_control; ++i) {
    if (delays[i] < 0 || control_index[i] < 0 || control_index[i] >= ni) {
      delete m;
      return fail("cmpc_sim_create: bad delay or control index");
    }
    m->delay[i] = delays[i];
    m->cidx[i] = control_index[i];
    m->ring_len += delays[i];
  }
  if (m->ring_len == 0) m->ring_len = 1;
  auto bail = [&](hipError_t e) {
    (void)e;
    sim_release(m);
    return fail("cmpc_sim_create: device allocation failed");
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return bail(e);
  if ((e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e);
  m->own_stream = true;
  const size_t Bz = (size_t)B;
  if ((e = hipMalloc(&m->x, sizeof(double) * Bz * ns)) != hipSuccess ||
      (e = hipMalloc(&m->dt, sizeof(double) * Bz)) != hipSuccess ||
      (e = hipMalloc(&m->u_full, sizeof(double) * Bz * ni)) != hipSuccess ||
      (e = hipMalloc(&m->u_offset, sizeof(double) * Bz * ni)) != hipSuccess ||
      (e = hipMalloc(&m->ring, sizeof(double) * Bz * m->ring_len)) != hipSuccess ||
      (e = hipMalloc(&m->scratch, sizeof(double) * Bz * (ni > n_control ? ni : n_control))) != hipSuccess ||
      (e = hipMalloc(&m->stage, sizeof(double) * Bz * 2 * std::max(std::max(ns, ni), std::max(no, n_control)))) !=
          hipSuccess ||
      (e = hipMalloc(&m->status, sizeof(int32_t) * Bz)) != hipSuccess ||
      (e = hipMemsetAsync(m->status, 0, sizeof(int32_t) * Bz, m->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(m->stream)) != hipSuccess)
    return bail(e);
  *out = m;
  return 0;
}

int cmpc_sim_destroy(cmpc_sim* m) {
  if (!m) return 0;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  sim_release(m);
  return 0;
}

int cmpc_sim_set_stream(cmpc_sim* m, void* stream) {
  if (!m) return fail("null simulator");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (m->own_stream) (void)hipStreamDestroy(m->stream);
  m->stream = (hipStream_t)stream;
  m->own_stream = false;
  return 0;
}

static SimInputParams sim_input_params(cmpc_sim* m, const double* u_control, int use_delay) {
  SimInputParams P;
  std::memset(&P, 0, sizeof P);
  P.u_control = u_control;
  P.u_offset = m->u_offset;
  P.u_full = m->u_full;
  P.ring = m->ring;
  P.B = m->B;
  P.nc = m->nc;
  P.ni = m->ni;
  P.ring_len = m->ring_len;
  P.use_delay = use_delay;
  for (int i = 0; i < m->nc; ++i) {
    P.delay[i] = m->delay[i];
    P.cidx[i] = m->cidx[i];
    P.cur[i] = m->cur[i];
  }
  return P;
}

int cmpc_sim_reset(cmpc_sim* m, const double* x0, const double* u_offset, double dt0) {
  if (!m || !x0 || !u_offset) return fail("null argument");
  if (!(dt0 > 0)) return fail("cmpc_sim_reset: dt0 must be positive");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  HIP_TRY(hipMemcpyAsync(m->x, x0, sizeof(double) * Bz * m->ns, hipMemcpyDeviceToDevice, m->stream));
  HIP_TRY(hipMemcpyAsync(m->u_offset, u_offset, sizeof(double) * Bz * m->ni, hipMemcpyDeviceToDevice,
                         m->stream));
  std::vector<double> dts(Bz, dt0);
  HIP_TRY(hipMemcpyAsync(m->dt, dts.data(), sizeof(double) * Bz, hipMemcpyHostToDevice, m->stream));
  // TimeDelay(): zero memory, cursor of input i at the sum of the delays before it
  HIP_TRY(hipMemsetAsync(m->ring, 0, sizeof(double) * Bz * m->ring_len, m->stream));
  HIP_TRY(hipMemsetAsync(m->status, 0, sizeof(int32_t) * Bz, m->stream));  // failures are sticky until here
  for (int i = 0, sum = 0; i < m->nc; ++i) {
    m->cur[i] = sum;
    sum += m->delay[i];
  }
  // u_ = GetPlantInput(u_init = 0) = u_offset
  HIP_TRY(hipMemcpyAsync(m->u_full, u_offset, sizeof(double) * Bz * m->ni, hipMemcpyDeviceToDevice,
                         m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));  // (host staging buffers above)
  return 0;
}

int cmpc_sim_set_input(cmpc_sim* m, const double* u_control) {
  if (!m || !u_control) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  const SimInputParams P = sim_input_params(m, u_control, 1);
  if (cmpc_launch_sim_input(P, m->stream)) return fail("sim input launch failed");
  if (check_launch("sim input kernel")) return -1;
  // TimeDelay::GetDelayedInput's cursor step (time_delay.h:41-58), on the host
  for (int i = 0, end = 0; i < m->nc; ++i) {
    if (m->delay[i] == 0) continue;
    end += m->delay[i];
    if (++m->cur[i] == end) m->cur[i] -= m->delay[i];
  }
  return 0;
}

int cmpc_sim_set_offset(cmpc_sim* m, const double* u_offset) {
  if (!m || !u_offset) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(m->u_offset, u_offset, sizeof(double) * (size_t)m->B * m->ni,
                         hipMemcpyDeviceToDevice, m->stream));
  return 0;
}

int cmpc_sim_plant_input_offset(cmpc_sim* m, const double* u_control, const double* u_offset,
                                double* u_full_out) {
  if (!m || !u_control || !u_offset || !u_full_out) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  SimInputParams P = sim_input_params(m, u_control, 0);
  P.u_offset = u_offset;
  P.u_full = u_full_out;
  if (cmpc_launch_sim_input(P, m->stream)) return fail("sim input launch failed");
  return check_launch("sim input kernel");
}

int cmpc_sim_plant_input(cmpc_sim* m, const double* u_control, double* u_full_out) {
  if (!m) return fail("null argument");
  return cmpc_sim_plant_input_offset(m, u_control, m->u_offset, u_full_out);  // (the simulator's own offsets)
}

int cmpc_sim_restart(cmpc_sim* m, double dt0) {
  if (!m) return fail("null simulator");
  if (!(dt0 > 0)) return fail("cmpc_sim_restart: dt0 must be positive");
  HIP_TRY(hipSetDevice(m->device));
  std::vector<double> dts((size_t)m->B, dt0);
  HIP_TRY(hipMemcpyAsync(m->dt, dts.data(), sizeof(double) * dts.size(), hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));  // (host staging buffer)
  return 0;
}

int cmpc_sim_integrate(cmpc_sim* m, double t, double t_end, double eps_abs, double eps_rel) {
  if (!m) return fail("null simulator");
  if (!(t_end >= t)) return fail("cmpc_sim_integrate: t_end < t");
  HIP_TRY(hipSetDevice(m->device));
  SimParams P;
  std::memset(&P, 0, sizeof P);
  P.x = m->x;
  P.dt = m->dt;
  P.u_full = m->u_full;
  P.status = m->status;
  P.B = m->B;
  P.t = t;
  P.t_end = t_end;
  P.eps_abs = eps_abs;
  P.eps_rel = eps_rel;
  P.p_in = m->p_in;
  P.p_out = m->p_out;
  if (m->pr) {  // the per-scenario instance reads scenario b's pair at this launch
    SimParamsP Q;
    std::memset(&Q, 0, sizeof Q);
    static_cast<SimParams&>(Q) = P;
    Q.pressures = m->pr;
    if (cmpc_launch_sim_pressures(Q, m->plant, m->stream)) return fail("sim launch failed");
    return check_launch("sim kernel (per-scenario pressures)");
  }
  if (cmpc_launch_sim(P, m->plant, m->stream)) return fail("sim launch failed");
  return check_launch("sim kernel");
}

// Per-scenario boundary pressures of the plant (include/cmpc.h)
int cmpc_sim_set_pressures(cmpc_sim* m, const double* pressures_device) {
  if (!m) return fail("null simulator");
  if (!pressures_device) {
    m->pr = nullptr;
    return 0;
  }
  HIP_TRY(hipSetDevice(m->device));
  if (ensure_device(&m->own_pr, sizeof(double) * 2 * (size_t)m->B)) return -1;
  HIP_TRY(hipMemcpyAsync(m->own_pr, pressures_device, sizeof(double) * 2 * (size_t)m->B, hipMemcpyDeviceToDevice,
                         m->stream));
  m->pr = m->own_pr;
  return 0;
}

int cmpc_sim_set_pressures_host(cmpc_sim* m, const double* pressures) {
  if (!m) return fail("null simulator");
  if (!pressures) {
    m->pr = nullptr;
    return 0;
  }
  if (pressures_check("cmpc_sim_set_pressures_host", pressures, (size_t)m->B)) return -1;
  HIP_TRY(hipSetDevice(m->device));
  if (ensure_device(&m->own_pr, sizeof(double) * 2 * (size_t)m->B)) return -1;
  HIP_TRY(hipMemcpyAsync(m->own_pr, pressures, sizeof(double) * 2 * (size_t)m->B, hipMemcpyHostToDevice,
                         m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));  // (the host array is free again)
  m->pr = m->own_pr;
  return 0;
}

int cmpc_sim_bind_pressures(cmpc_sim* m, const double* pressures_device) {
  if (!m) return fail("null simulator");
  if (pressures_device) {
    if (!device_range_ok(m->device, pressures_device, sizeof(double) * 2 * (size_t)m->B))
      return fail("cmpc_sim_bind_pressures: not a device allocation of B * 2 doubles on the simulator's device");
    // one 16-byte load per scenario
    if (reinterpret_cast<uintptr_t>(pressures_device) % 16)
      return fail("cmpc_sim_bind_pressures: the array must be 16-byte aligned");
  }
  m->pr = pressures_device;
  return 0;
}

int cmpc_sim_get_pressures(cmpc_sim* m, double* pressures) {
  if (!m || !pressures) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  if (!m->pr) {  // the scalars of cmpc_sim_create hold for every scenario
    for (int b = 0; b < m->B; ++b) {
      pressures[2 * b] = m->p_in;
      pressures[2 * b + 1] = m->p_out;
    }
    return 0;
  }
  return direct_download(m->stream, {{m->pr, pressures, sizeof(double) * 2 * (size_t)m->B}});
}

int cmpc_sim_output(cmpc_sim* m, double* y) {
  if (!m || !y) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  if (cmpc_launch_sim_output(m->plant, m->x, y, m->B, m->stream)) return fail("sim output launch failed");
  return check_launch("sim output kernel");
}

int cmpc_sim_download(cmpc_sim* m, double* x, double* u_full, double* dt, int32_t* status) {
  if (!m) return fail("null simulator");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  return pinned_download(m->pin_out, m->stream,
                         {{m->x, x, sizeof(double) * Bz * m->ns},
                          {m->u_full, u_full, sizeof(double) * Bz * m->ni},
                          {m->dt, dt, sizeof(double) * Bz},
                          {m->status, status, sizeof(int32_t) * Bz}});
}

// Host-array variants: stage through the simulator's device buffer; each
// returns once the call's work is done (the host arrays are free again).
static int sim_stage(cmpc_sim* m, const double* h0, size_t n0, const double* h1, size_t n1) {
  HIP_TRY(hipSetDevice(m->device));
  const size_t half = (size_t)m->B * std::max(std::max(m->ns, m->ni), std::max(m->no, m->nc));
  // one DMA from page-locked memory: h0 at stage, h1 at stage + half
  const size_t tot = n1 ? half + n1 : n0;
  if (pinned_acquire(m->pin_in, sizeof(double) * std::max<size_t>(tot, 1))) return -1;
  double* h = reinterpret_cast<double*>(m->pin_in.buf);
  if (n0) std::memcpy(h, h0, sizeof(double) * n0);
  if (n1) std::memcpy(h + half, h1, sizeof(double) * n1);
  if (tot) HIP_TRY(hipMemcpyAsync(m->stage, h, sizeof(double) * tot, hipMemcpyHostToDevice, m->stream));
  return pinned_release(m->pin_in, m->stream);
}

int cmpc_sim_reset_host(cmpc_sim* m, const double* x0, const double* u_offset, double dt0) {
  if (!m || !x0 || !u_offset) return fail("null argument");
  const size_t half = (size_t)m->B * std::max(std::max(m->ns, m->ni), std::max(m->no, m->nc));
  if (sim_stage(m, x0, (size_t)m->B * m->ns, u_offset, (size_t)m->B * m->ni)) return -1;
  return cmpc_sim_reset(m, m->stage, m->stage + half, dt0);  // (synchronises)
}

int cmpc_sim_set_input_host(cmpc_sim* m, const double* u_control) {
  if (!m || !u_control) return fail("null argument");
  if (sim_stage(m, u_control, (size_t)m->B * m->nc, nullptr, 0)) return -1;
  if (cmpc_sim_set_input(m, m->stage)) return -1;
  return cmpc_sim_synchronize(m);
}

int cmpc_sim_set_offset_host(cmpc_sim* m, const double* u_offset) {
  if (!m || !u_offset) return fail("null argument");
  if (sim_stage(m, u_offset, (size_t)m->B * m->ni, nullptr, 0)) return -1;
  if (cmpc_sim_set_offset(m, m->stage)) return -1;
  return cmpc_sim_synchronize(m);
}

int cmpc_sim_output_host(cmpc_sim* m, double* y) {
  if (!m || !y) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  const size_t by = sizeof(double) * (size_t)m->B * m->no;
  if (pinned_acquire(m->pin_out, by)) return -1;
  if (cmpc_sim_output(m, m->stage)) return -1;
  HIP_TRY(hipMemcpyAsync(m->pin_out.buf, m->stage, by, hipMemcpyDeviceToHost, m->stream));
  if (cmpc_sim_synchronize(m)) return -1;
  std::memcpy(y, m->pin_out.buf, by);
  return 0;
}

double* cmpc_sim_state(cmpc_sim* m) { return m ? m->x : nullptr; }
double* cmpc_sim_input(cmpc_sim* m) { return m ? m->u_full : nullptr; }
double* cmpc_sim_step_size(cmpc_sim* m) { return m ? m->dt : nullptr; }
int32_t* cmpc_sim_status(cmpc_sim* m) { return m ? m->status : nullptr; }
int cmpc_sim_delay_len(cmpc_sim* m) { return m ? m->ring_len : -1; }

int cmpc_sim_download_inputs(cmpc_sim* m, double* u_offset, double* delay_line) {
  if (!m) return fail("null simulator");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (u_offset) HIP_TRY(hipMemcpy(u_offset, m->u_offset, sizeof(double) * Bz * m->ni, hipMemcpyDeviceToHost));
  if (delay_line) HIP_TRY(hipMemcpy(delay_line, m->ring, sizeof(double) * Bz * m->ring_len, hipMemcpyDeviceToHost));
  return 0;
}

int cmpc_sim_synchronize(cmpc_sim* m) {
  if (!m) return fail("null simulator");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return 0;
}

}  // extern "C"
