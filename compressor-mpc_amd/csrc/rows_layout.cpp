// LDS layout of the row-layout build kernel (build_rows.hip), chosen by a
// bank-conflict model of its horizon loop.
//
// The kernel's LDS offsets are all runtime parameters (RowsLayout), so the
// host can place every region freely.  The horizon loop issues, per step and
// wave (tools/lds_rows_sim.py is the same model in Python):
//   ds_read_b64   yh   = yp[u]                 (zeros / L_W'y_ref / carriers)
//   ds_write_b64  wq[u*NY + o], o < NY          (Markov writers, 4 lanes a row)
//   ds_write_b64  zq[u*NY]                      (free-response writers)
//   ds_read2_b64 + ds_read_b64  rq[u*NY + o]    (gather lanes)
//   per unrolled group: ds_write_b64 tq[o]      (ring history)
// and MI355X_MICROARCH.md §LDS gives their banking: ds_read_b64 in two
// 32-lane groups on 32 double-wide banks, ds_read2_b64 / ds_write_b64 in four
// 16-lane groups on 16; every extra distinct address on a bank costs one LDS
// cycle.  Packed naively (regions back to back) the loop takes ≈ 28 extra
// LDS cycles per wave-step at coop p = 50, which PMC confirmed
// (SQ_LDS_BANK_CONFLICT ≈ 30 per wave-step).  A deterministic search over the
// order of the per-input lines and a few doubles of padding between regions,
// within the LDS budget that keeps the resident waves per CU of the packed layout,
// brings the model to ≈ 2.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "cmpc_internal.h"

namespace {


constexpr int kLdsBytes = 160 * 1024;

struct Pads {
  int order[CMPC_MAX_INPUTS];
  int pad_c[CMPC_MAX_INPUTS];
  int dump, z, zr, LQ, yl, yls, w, WL;
  int ring;  // ring lines where p > 2 D + 1 (only when that keeps more waves resident)
};

int up(int v, int a) { return (v + a - 1) / a * a; }

// Wrap steps of a ring line of R entries (entry e holds the value of step
// e - (m - 1), the first m - 1 entries start as history zeros): the writer of
// step t stores entry m - 1 + t, so it steps back by R entries at t = R - m + 1;
// the move-k reader reads entry (m - 1 - k) + s - D at step s >= D, so it steps
// back at s = R + D - (m - 1 - k).
int rows_ring_writer_wrap(int R, int M) { return R - (M - 1); }
int rows_ring_reader_wrap(int R, int D, int M, int k) { return R + D - (M - 1 - k); }

// The layout for given paddings (all offsets in doubles).  Returns the LDS
// bytes per workgroup.
size_t make_layout(const cmpc_dims& d, int nd, int rec_len, const Pads& pd, RowsLayout* R) {
  std::memset(R, 0, sizeof *R);
  const int M = d.m, ny = d.ny, U = cmpc_rows_unroll(d.ny);
  int o = 0;
  for (int i = 0; i < d.nu_tot; ++i) {
    const int c = pd.order[i];
    o += pd.pad_c[c];
    R->lo[c] = o;
    int len = (d.delay[c] == 0) ? U + 1 : (M - 1) + std::max(0, d.p - d.delay[c]);
    // a value written at step t is read until step t + D + m - 1: a ring of
    // D + m entries holds every value still to be read (rows_ring_* below)
    if (pd.ring && d.delay[c] > 0 && len > d.delay[c] + M) {
      len = d.delay[c] + M;
      R->ring[c] = len;
    }
    o += ny * len;
  }
  o += pd.dump;
  R->dump_off = o;
  o += U * ny;
  o += pd.z;
  R->z_off = o;
  o += U * ny;
  o += pd.zr;
  R->zr_off = o;
  o += U * ny;
  R->LQ = up(o, 2) + 2 * pd.LQ;
  R->U = U;
  // the C_hat rows overlay the hand-off areas when those are large enough
  // (build_rows.hip reads them in the prologue, before any area is written)
  const int chs = 4 * ny * 16;
  R->ch_off = (4 * R->LQ >= chs) ? 0 : 4 * R->LQ;
  R->w_off = std::max(4 * R->LQ, R->ch_off + chs) + pd.w;
  // w lines: the carriers read entries 3 + r (r < p) until the segment r = D
  // of their input, then the zero slots (build_rows.hip): D + 3 entries
  int dmax = 0;
  for (int c = 0; c < d.nu_tot; ++c) dmax = std::max(dmax, d.delay[c]);
  R->WL = up(std::min(d.p + 2 + U, dmax + 3), 2) + pd.WL;
  // the group's four records are staged over the wave's region first
  R->per_wave = std::max(up(R->w_off + 4 * nd * R->WL, 2), up(4 * rec_len, 2));
  R->yls = d.p + U + pd.yls;
  R->yl_off = 16 + pd.yl;
  R->lw_off = R->yl_off + d.S * ny * R->yls;
  R->uw_off = R->lw_off + d.S * ny * ny;
  R->lds_block = up(R->uw_off + d.S * d.nu * d.nu, 2);
  // loop segments: distinct D (delayed readers start) and p - D (delayed
  // writers stop) inside (0, p), ascending
  R->nseg = 0;
  bool fits = true;
  auto add = [&](int v) {
    if (v <= 0 || v >= d.p) return;
    for (int i = 0; i < R->nseg; ++i)
      if (R->seg[i] == v) return;
    if (R->nseg == CMPC_ROWS_NSEG) {
      fits = false;
      return;
    }
    R->seg[R->nseg++] = v;
  };
  for (int c = 0; c < d.nu_tot; ++c)
    if (d.delay[c] > 0) {
      add(d.delay[c]);
      add(d.p - d.delay[c]);
      if (R->ring[c]) {  // wrap steps: the writer's (while it writes), each move's gather reader's
        for (int t = rows_ring_writer_wrap(R->ring[c], M); t < d.p - d.delay[c]; t += R->ring[c]) add(t);
        for (int k = 0; k < M; ++k)
          for (int t = rows_ring_reader_wrap(R->ring[c], d.delay[c], M, k); t < d.p; t += R->ring[c]) add(t);
      }
    }
  std::sort(R->seg, R->seg + R->nseg);
  if (!fits) R->nseg = -1;  // too many segments: not usable (make_layout's caller checks)
  return sizeof(double) * ((size_t)R->lds_block + (size_t)R->per_wave * CMPC_BUILD_WAVES);
}

// max over banks of the distinct addresses on a bank, for lanes [g0, g0+n)
int group_cycles(const int* a, const bool* act, int g0, int n, int nbank) {
  int seen[64], ns = 0, cnt[64] = {0}, mx = 1;
  for (int i = g0; i < g0 + n; ++i) {
    if (!act[i]) continue;
    bool dup = false;
    for (int k = 0; k < ns && !dup; ++k) dup = seen[k] == a[i];
    if (dup) continue;
    seen[ns++] = a[i];
    const int b = ((a[i] % nbank) + nbank) % nbank;
    mx = std::max(mx, ++cnt[b]);
  }
  return mx;
}

// Extra LDS cycles per wave-step of the horizon loop for wave `wave`; the
// per-lane pointer arithmetic is the kernel's (build_rows.hip).
double loop_conflicts(const cmpc_dims& d, int nd, const RowsLayout& R, int wave) {
  const int NS = d.ns, NY = d.ny, NUT = d.nu_tot, M = d.m, ND = nd, S = d.S, p = d.p, U = R.U;
  const int NG = M * NUT + 1;
  const int wreg = R.lds_block + wave * R.per_wave;
  int rq[64], rinc[64], rline[64], rsw[64], wq[64], winc[64], wsw[64], dump[64], yp[64], yinc[64];
  int zq[64], tq[64], ysw[64], rwr[64], wwr[64], rback[64], wback[64];
  int kdelay[CMPC_ND_MAX] = {0};  // delay of the k-th delayed input (ascending input index)
  for (int c = 0, k = 0; c < d.nu_tot && k < CMPC_ND_MAX; ++c)
    if (d.delay[c] > 0) kdelay[k++] = d.delay[c];
  bool mk[64], ol[64], tl[64], all[64];
  for (int lane = 0; lane < 64; ++lane) {
    const int Rw = lane >> 4, j = lane & 15, s = Rw % S;
    const int ql = wreg + Rw * R.LQ;
    const bool st = j < NS;
    mk[lane] = j >= NS && j < NS + NUT;
    const int cm = mk[lane] ? j - NS : 0;
    ol[lane] = j >= NS && j < NS + NY;
    const int oo = ol[lane] ? j - NS : 0;
    const bool cl = ND > 0 && j >= 16 - ND;
    const int kc = cl ? j - (16 - ND) : 0;
    const bool gl = j < NG, zl = j == NG - 1;
    const int gk = (gl && !zl) ? j / NUT : 0;
    const int gc = (gl && !zl) ? j - gk * NUT : 0;
    const int dg = d.delay[gc], dm = d.delay[cm];
    const int zrow = ql + R.zr_off;
    rq[lane] = !gl ? zrow : zl ? ql + R.z_off : (dg == 0) ? ql + R.lo[gc] + (1 - gk) * NY : zrow;
    rinc[lane] = 0;
    rline[lane] = ql + R.lo[gc] + (M - 1 - gk) * NY;
    const bool rdel = gl && !zl && dg > 0;
    rsw[lane] = (rdel && dg < p) ? dg : -1;
    const bool wdel = mk[lane] && dm > 0;
    dump[lane] = ql + R.dump_off;
    wq[lane] = !mk[lane] ? dump[lane]
               : (dm == 0) ? ql + R.lo[cm] + NY
               : (p - dm > 0) ? ql + R.lo[cm] + (M - 1) * NY
                              : dump[lane];
    winc[lane] = (wdel && p - dm > 0) ? NY : 0;
    wsw[lane] = (wdel && p - dm > 0) ? p - dm : -1;
    const int rgw = mk[lane] ? R.ring[cm] : 0, rgr = (gl && !zl) ? R.ring[gc] : 0;
    wwr[lane] = (wdel && rgw) ? rows_ring_writer_wrap(rgw, M) : -1;
    wback[lane] = rgw * NY;
    rwr[lane] = (rdel && rgr) ? rows_ring_reader_wrap(rgr, dg, M, gk) : -1;
    rback[lane] = rgr * NY;
    tl[lane] = M > 1 && mk[lane] && dm == 0;
    tq[lane] = ql + R.lo[cm];
    zq[lane] = ol[lane] ? ql + R.z_off + oo : dump[lane];  // every lane stores (build_rows.hip)
    if (st) {
      yp[lane] = 0; yinc[lane] = 0;
    } else if (ol[lane]) {
      yp[lane] = R.yl_off + (s * NY + oo) * R.yls + 1; yinc[lane] = 1;
    } else if (cl) {
      yp[lane] = wreg + R.w_off + (Rw * ND + kc) * R.WL + 3; yinc[lane] = 1;
    } else {
      yp[lane] = 0; yinc[lane] = 0;
    }
    ysw[lane] = (cl && kdelay[kc] < p) ? kdelay[kc] : -1;
    all[lane] = true;
  }
  long extra = 0, steps = 0;
  int a[64], b[64];
  auto read_b64 = [&](const int* x) {
    extra += group_cycles(x, all, 0, 32, 32) - 1 + group_cycles(x, all, 32, 32, 32) - 1;
  };
  auto by16 = [&](const int* x, const bool* act) {
    for (int g = 0; g < 64; g += 16) extra += group_cycles(x, act, g, 16, 16) - 1;
  };
  auto step = [&](int u) {
    ++steps;
    for (int l = 0; l < 64; ++l) a[l] = yp[l] + u;
    read_b64(a);
    for (int o = 0; o < NY; ++o) {
      for (int l = 0; l < 64; ++l) a[l] = wq[l] + u * NY + o;
      by16(a, all);  // lanes without a Markov role store into the dump area
    }
    for (int l = 0; l < 64; ++l) a[l] = zq[l] + u * NY;
    by16(a, all);
    for (int o = 0; o < NY;) {
      for (int l = 0; l < 64; ++l) a[l] = rq[l] + u * NY + o;
      if (o + 1 < NY) {  // the compiler pairs the reads into ds_read2_b64
        for (int l = 0; l < 64; ++l) b[l] = a[l] + 1;
        by16(a, all);
        by16(b, all);
        o += 2;
      } else {
        read_b64(a);
        o += 1;
      }
    }
  };
  auto tail = [&]() {
    for (int o = 0; o < NY; ++o) {
      for (int l = 0; l < 64; ++l) a[l] = tq[l] + o;
      by16(a, tl);
    }
  };
  auto advance = [&](int k) {
    for (int l = 0; l < 64; ++l) {
      wq[l] += k * winc[l];
      rq[l] += k * rinc[l];
      yp[l] += k * yinc[l];
    }
  };
  int r = 0;
  for (int sg = 0; sg <= R.nseg; ++sg) {
    const int r_end = sg < R.nseg ? R.seg[sg] : p;
    for (; r + U <= r_end; r += U) {
      for (int u = 0; u < U; ++u) step(u);
      tail();
      advance(U);
    }
    while (U > 2 && r + 2 <= r_end) {  // the kernel's two-step remainder blocks
      step(0);
      step(1);
      tail();
      advance(2);
      r += 2;
    }
    for (; r < r_end; ++r) {
      step(0);
      tail();
      advance(1);
    }
    for (int l = 0; l < 64; ++l) {
      if (r == rsw[l]) { rq[l] = rline[l]; rinc[l] = NY; }
      if (r == rwr[l]) { rq[l] -= rback[l]; rwr[l] += rback[l] / NY; }
      if (r == wwr[l]) { wq[l] -= wback[l]; wwr[l] += wback[l] / NY; }
      if (r == wsw[l]) { wq[l] = dump[l]; winc[l] = 0; wwr[l] = -1; }
      if (r == ysw[l]) { yp[l] = 0; yinc[l] = 0; }  // the zero slots
    }
  }
  return steps ? (double)extra / steps : 0.0;
}

// resident waves per CU of layout R with w waves per workgroup, at most 12
// (3 waves/SIMD: the kernel's register budget)
int waves_with(const RowsLayout& R, int w) {
  // A workgroup takes more LDS than it asks for.  Measured residency: 54 240 B
  // per workgroup runs as 2 per CU (ser-coop p = 50: 3 requested by the
  // occupancy query, 0.382 ms; 2 forced, 0.350 ms), 53 408 B as 3 (ser-cent
  // p = 50), 81 168 B as 2 (par-coop p = 100), 54 693 B as 2.  Model: the
  // request rounded up to 512 B, plus 512 B.
  const size_t req = sizeof(double) * ((size_t)R.lds_block + (size_t)R.per_wave * w);
  const size_t lds = (req + 511) / 512 * 512 + 512;
  return lds <= (size_t)kLdsBytes ? std::min(12, (int)(kLdsBytes / lds) * w) : 0;
}

int resident_waves(const RowsLayout& R) {
  const int w = cmpc_rows_waves_per_group(R);
  return w ? waves_with(R, w) : 0;
}

uint64_t lcg(uint64_t& s) {
  s = s * 6364136223846793005ULL + 1442695040888963407ULL;
  return s >> 33;
}


}  // namespace

// Workgroup size of the row kernel for layout R: four waves wherever at
// least one four-wave workgroup per CU fits; two-wave workgroups only where
// they hold twice the resident waves.  A workgroup's waves go to SIMDs in a
// fixed cyclic order, so small workgroups pile onto some SIMDs: at p = 100
// (round 2, w tables of D + 3 entries) four-wave workgroups measured as fast
// or faster in every case (par-coop 8 vs 6 waves 0.52 vs 0.68 ms, par-cent
// 8 vs 8 waves 0.290 vs 0.290 ms, ser-coop 4 vs 6 waves 0.89 vs 1.41 ms,
// ser-cent 4 vs 6 waves 0.49 vs 0.80 ms; tools/gpu_wpg_sweep.sh).  0 when
// not even one two-wave workgroup per SIMD fits: the one-QP-per-wave kernel
// runs.  CMPC_ROWS_WPG=4|2 overrides it for timing.
int cmpc_rows_resident_groups(const RowsLayout& R, int w) { return w > 0 ? waves_with(R, w) / w : 0; }

int cmpc_rows_waves_per_group(const RowsLayout& R) {
  if (const char* e = std::getenv("CMPC_ROWS_WPG")) {
    const int w = std::atoi(e);
    if ((w == 4 || w == 2) && waves_with(R, w) > 0) return w;
  }
  const int w4 = waves_with(R, 4), w2 = waves_with(R, 2);
  if (w2 >= 2 * w4 && w2 >= 4) return 2;
  if (w4 >= 4) return 4;
  return w2 >= 4 ? 2 : 0;
}

void cmpc_rows_layout(const cmpc_dims& d, int nd, int nobs, int rec_len, RowsLayout* out) {
  std::memset(out, 0, sizeof *out);
  if (d.m < 1 || d.m > 2 || nobs > 16) return;
  static std::mutex mu;
  static std::map<std::vector<int>, RowsLayout> cache;
  std::vector<int> key{d.ns, d.ny, d.nu, d.nu_tot, d.m, d.p, d.S, nd, nobs, rec_len};
  for (int c = 0; c < CMPC_MAX_INPUTS; ++c) key.push_back(d.delay[c]);
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) {
      *out = it->second;
      return;
    }
  }
  Pads base{};
  for (int c = 0; c < CMPC_MAX_INPUTS; ++c) base.order[c] = c;
  RowsLayout best;
  make_layout(d, nd, rec_len, base, &best);
  {
    // ring lines (and the kernel's RING instantiation, whose wrap bookkeeping
    // costs registers) only where they let more waves share a CU: ser-coop /
    // ser-cent p = 100 go from one four-wave workgroup per CU to two, while
    // par-coop p = 100 has two either way and keeps its plain lines
    Pads rb = base;
    rb.ring = 1;
    RowsLayout rl;
    make_layout(d, nd, rec_len, rb, &rl);
    if (rl.nseg >= 0 && (best.nseg < 0 || resident_waves(rl) > resident_waves(best))) {
      base = rb;
      best = rl;
    }
  }
  if (best.nseg < 0) {  // more loop segments than the kernel unrolls over: not usable
    best.ok = 0;
    std::lock_guard<std::mutex> lk(mu);
    cache[key] = best;
    *out = best;
    return;
  }
  const int base_waves = resident_waves(best);
  // CMPC_ROWS_LAYOUT=packed: regions back to back (diagnostic A/B timing)
  const char* env = std::getenv("CMPC_ROWS_LAYOUT");
  const bool packed = env && std::strcmp(env, "packed") == 0;
  if (packed) {
    best.ok = base_waves > 0;
  } else if (base_waves > 0) {
    // keep the resident waves per CU of the packed layout (over the
    // launcher's workgroup sizes, capped by the kernel's register budget)
    double best_cost = loop_conflicts(d, nd, best, 0);
    Pads bp = base;
    uint64_t seed = 0x5eedULL;
    if (const char* e = std::getenv("CMPC_ROWS_SEED")) seed = std::strtoull(e, nullptr, 0);  // layout A/B
    for (int it = 0; it < 400 && best_cost > 0.0; ++it) {
      Pads cand = bp;
      const int nchg = 1 + (int)(lcg(seed) % 3);
      for (int k = 0; k < nchg; ++k) {
        const int which = (int)(lcg(seed) % (d.nu_tot + 8));
        const int v = (int)(lcg(seed) % 16);
        if (which < d.nu_tot) cand.pad_c[which] = v;
        else {
          int* f[8] = {&cand.dump, &cand.z, &cand.zr, &cand.LQ, &cand.yl, &cand.yls, &cand.w, &cand.WL};
          *f[which - d.nu_tot] = (which - d.nu_tot == 3) ? v % 4 : v;
        }
      }
      if (lcg(seed) % 10 < 3) {
        for (int i = d.nu_tot - 1; i > 0; --i) std::swap(cand.order[i], cand.order[lcg(seed) % (i + 1)]);
      }
      RowsLayout R;
      make_layout(d, nd, rec_len, cand, &R);
      if (resident_waves(R) < base_waves) continue;
      const double cost = loop_conflicts(d, nd, R, 0);
      if (cost < best_cost) {
        best_cost = cost;
        best = R;
        bp = cand;
      }
    }
    make_layout(d, nd, rec_len, bp, &best);
    best.ok = resident_waves(best) > 0;
  }
  std::lock_guard<std::mutex> lk(mu);
  cache[key] = best;
  *out = best;
}

// The shared form's wave region on top of layout R (PairLayout,
// cmpc_internal.h).  The hand-off areas keep R's offsets, so their accesses
// keep R's modelled bank conflicts; slot 1's z entries and the second set of w
// tables follow them, the w tables at R's residue mod 32.  ok: two four-wave
// workgroups per CU fit (the kernel is compiled for two waves per SIMD) and
// the group's staging fits the kernel's chunk counts.
void cmpc_pair_layout(const cmpc_dims& d, const RowsLayout& R, int nd, int rec_len, int off_x, PairLayout* out) {
  std::memset(out, 0, sizeof *out);
  if (!R.ok || rec_len % 2) return;
  const int zlen = 4 * R.U * d.ny;
  out->z1_off = up(R.w_off, 2);
  out->tail0 = off_x & ~1;
  const int stage = 4 * (2 * rec_len - out->tail0);
  int w = std::max(out->z1_off + zlen, stage);  // behind the staged records
  while ((w - R.w_off) % 32) ++w;
  out->w_off = w;
  // w lines of D + 3 entries (make_layout), without the row layout's padding
  int dmax = 0;
  for (int c = 0; c < d.nu_tot; ++c) dmax = std::max(dmax, d.delay[c]);
  out->WL = up(std::min(d.p + 2 + R.U, dmax + 3), 2);
  out->per_wave = up(out->w_off + 4 * 2 * nd * out->WL, 2);
  const size_t req = sizeof(double) * ((size_t)R.lds_block + (size_t)out->per_wave * CMPC_BUILD_WAVES);
  const size_t lds = (req + 511) / 512 * 512 + 512;  // waves_with's allocation model
  // the kernel stages a record in three 1 KiB blocks and its tail in one, and
  // compares the record's head in CMPC_PAIR_CMP blocks of 64 entries
  out->ok = 2 * lds <= (size_t)kLdsBytes && rec_len <= 384 && rec_len - out->tail0 <= 128 &&
            off_x <= 64 * CMPC_PAIR_CMP && rec_len >= 64 * CMPC_PAIR_CMP && out->WL <= 64;
}

double cmpc_rows_layout_conflicts(const cmpc_dims& d, int nd, const RowsLayout& R, int wave) {
  return loop_conflicts(d, nd, R, wave);
}

extern "C" int cmpc_rows_lds_model(const cmpc_dims* d, double* packed_cycles, double* chosen_cycles,
                                   int32_t* lds_bytes) {
  if (!d) return -1;
  cmpc_layout L;
  if (cmpc_layout_of(d, &L)) return -1;
  RowsLayout R;
  cmpc_rows_layout(*d, L.nd, L.nobs, L.rec_len, &R);
  if (!R.ok) return -1;
  Pads base{};
  for (int c = 0; c < CMPC_MAX_INPUTS; ++c) base.order[c] = c;
  for (int c = 0; c < CMPC_MAX_INPUTS; ++c) base.ring = base.ring || R.ring[c] > 0;
  RowsLayout P0;
  make_layout(*d, L.nd, L.rec_len, base, &P0);
  if (packed_cycles) *packed_cycles = loop_conflicts(*d, L.nd, P0, 0);
  if (chosen_cycles) *chosen_cycles = loop_conflicts(*d, L.nd, R, 0);
  if (lds_bytes)
    *lds_bytes = (int32_t)(sizeof(double) * ((size_t)R.lds_block + (size_t)R.per_wave * CMPC_BUILD_WAVES));
  return 0;
}
