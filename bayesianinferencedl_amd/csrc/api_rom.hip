// The reduced-order model behind the C ABI: every finrom_rom_* entry point, finrom_subfin_avg, the FINROM_TRACE dump,
// and finrom_solve_pairs, which runs the FOM half through api_fom.hip's stages.
#include "api_private.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace finrom;

extern "C" {

// ---------------------------------------------------------------------------------------
// ROM
// ---------------------------------------------------------------------------------------
int finrom_rom_create(const finrom_rom_desc* a, finrom_rom_t* out) {
  if (!a || !out) { set_error("rom_create: null argument"); return FINROM_ERR_ARG; }
  *out = nullptr;
  if (int rc = validate_rom_desc(a)) return rc;
  const int r = a->r, NB = (r + 15) / 16, rp = 16 * NB;
  if (NB > 13) { set_error("rom_create: basis size > 208 not supported"); return FINROM_ERR_UNSUPPORTED; }

  auto cnt = [&](int row) { return a->row_ptr[row + 1] - a->row_ptr[row]; };
  const std::vector<int> order = rows_by_term_count(a);
  auto* h = new finrom_rom_s();
  RomDev& d = h->d;
  d.n = a->n; d.r = r; d.rp = rp; d.NB = NB; d.P = a->P; d.n_obs = a->n_obs;
  d.solve_in_lds = rp <= 176 ? 1 : 0;
  d.trace = nullptr;
  auto push_slot = [&](std::vector<double>& T, std::vector<int>& Pi, const std::vector<int>& rows4, int t) {
    for (int q = 0; q < 4; ++q) {
      const size_t base = T.size();
      T.resize(base + rp, 0.0);
      int pi = 0;
      if (q < (int)rows4.size() && rows4[q] >= 0) {
        const int row = rows4[q], tt = a->row_ptr[row] + t;
        if (tt < a->row_ptr[row + 1]) { std::memcpy(&T[base], a->term_val + (size_t)tt * r, r * sizeof(double)); pi = a->term_p[tt]; }
      }
      Pi.push_back(pi);
    }
  };
  // ---- pattern-uniform k-steps for the single-wave kernels (see RomDev::tvu) ----------------------------------------------
  std::vector<double> tvu; std::vector<int> kmeta;
  {
    std::vector<KStep> ksteps = uniform_ksteps(a, order);
    // every term-count group gets an even number of k-steps (a k-step of zero rows pads it): the multi-wave main loop is
    // unrolled twice and specialised by term count, so that its phases start at even k-steps
    for (size_t k = 0; k < ksteps.size();) {
      size_t k1 = k;
      while (k1 < ksteps.size() && ksteps[k1].pat.size() == ksteps[k].pat.size()) ++k1;
      if ((k1 - k) % 2) { ksteps.insert(ksteps.begin() + k1, KStep{ksteps[k].pat, {-1, -1, -1, -1}}); ++k1; }
      k = k1;
    }
    for (int t = 0; t < 4; ++t) {
      d.uend[t] = 0;
      for (const KStep& ks : ksteps) if ((int)ks.pat.size() > t) ++d.uend[t];
    }
    int uslots = 0;
    for (size_t k = 0; k < ksteps.size(); ++k) {
      const int nt = (int)ksteps[k].pat.size();
      if (nt > 4) { delete h; set_error("rom_create: a row of psi has more than 4 terms"); return FINROM_ERR_UNSUPPORTED; }
      for (int t = 0; t < nt; ++t) {
        const int pp = ksteps[k].pat[t];
        for (int q = 0; q < 4; ++q) {
          const size_t base = tvu.size();
          tvu.resize(base + rp, 0.0);
          const int row = ksteps[k].rows[q];
          if (row < 0) continue;
          for (int tt = a->row_ptr[row]; tt < a->row_ptr[row + 1]; ++tt)
            if (a->term_p[tt] == pp) for (int col = 0; col < r; ++col) tvu[base + col] += a->term_val[(size_t)tt * r + col];
        }
      }
      uslots += nt;
    }
    // per-k-step records for the interleaved main loop: {first slot, term count, -, -, theta index of slots 0..3}; eight padding
    // k-steps point at the zero slots behind the table
    d.nku = (int)ksteps.size();
    {
      int sl = 0;
      for (size_t k = 0; k < ksteps.size(); ++k) {
        const int nt = (int)ksteps[k].pat.size();
        int rec[8] = {sl, nt, 0, 0, 0, 0, 0, 0};
        for (int t = 0; t < nt; ++t) rec[4 + t] = ksteps[k].pat[t];
        kmeta.insert(kmeta.end(), rec, rec + 8);
        sl += nt;
      }
      for (int k = 0; k < 8; ++k) { int rec[8] = {uslots, 1, 0, 0, 0, 0, 0, 0}; kmeta.insert(kmeta.end(), rec, rec + 8); }
    }
    tvu.resize(tvu.size() + (size_t)4 * 4 * rp, 0.0);       // one k-step of padding for the prefetch
    d.tvu_bytes = (int)std::min<size_t>(tvu.size() * sizeof(double), (size_t)0x7FFFFFF0);

    // ---- the same k-steps grouped by their leading parameter (build_grouped_tables above; proj_main_grouped, NB <= 5) ------
    d.n_ext = 0; d.nkg = 0; d.ext_final = 0; d.ext = nullptr;
    d.nkg_m = 0; d.kmg_m = 0; d.ext_final_m = 0; d.twin = nullptr;
    d.nkg_s = 0; d.kmg_s = 0; d.ext_final_s = 0; d.short_lo = 0.0; d.short_hi = 0.0;
    if (NB <= 5 && getenv("FINROM_PROJ_UNGROUPED") == nullptr) {
      GroupedTables gt;
      if (build_grouped_tables(a, ksteps, rp, gt)) {
        d.nkg = gt.nkg; d.n_ext = gt.n_ext; d.ext_final = gt.ext_final;
        h->tvg_host = gt.tvg; h->kmg_host = gt.kmg; h->def_host = gt.def;      // (finrom_rom_set_mirror appends the half list)
        d.tvg_bytes = (int)std::min<size_t>(gt.tvg.size() * sizeof(double), (size_t)0x7FFFFFF0);
        int grc = up(h->owned, &d.tvg, gt.tvg.data(), gt.tvg.size());
        if (!grc) grc = up(h->owned, &d.kmg, gt.kmg.data(), gt.kmg.size());
        if (!grc) grc = up(h->owned, &d.ext_def, gt.def.data(), gt.def.size());
        if (grc) { finrom_rom_destroy(h); return grc; }
      }
    }
  }
  // root rows (F != 0) for B_r = psi^T F
  std::vector<int> frows;
  for (int i = 0; i < a->n; ++i) if (a->rhs[i] != 0.0 && cnt(i) > 0) frows.push_back(i);
  d.rhs_nk = ((int)frows.size() + 3) / 4;
  d.rhs_nt = 0;
  for (int row : frows) d.rhs_nt = std::max(d.rhs_nt, cnt(row));
  std::vector<double> rtv, rf; std::vector<int> rpi;
  for (int ks = 0; ks < d.rhs_nk; ++ks) {
    std::vector<int> rows4;
    for (int q = 0; q < 4; ++q) {
      const int idx = ks * 4 + q;
      rows4.push_back(idx < (int)frows.size() ? frows[idx] : -1);
      rf.push_back(idx < (int)frows.size() ? a->rhs[frows[idx]] : 0.0);
    }
    for (int t = 0; t < d.rhs_nt; ++t) push_slot(rtv, rpi, rows4, t);
  }
  if (rtv.empty()) { rtv.assign(4 * rp, 0.0); rpi.assign(4, 0); rf.assign(4, 0.0); }

  // h_p = Psi_p^T F for the offline/online form of B_r
  std::vector<double> hp((size_t)(a->P + 1) * rp, 0.0);
  for (int i = 0; i < a->n; ++i) {
    if (a->rhs[i] == 0.0) continue;
    for (int t = a->row_ptr[i]; t < a->row_ptr[i + 1]; ++t)
      for (int col = 0; col < r; ++col) hp[(size_t)a->term_p[t] * rp + col] += a->rhs[i] * a->term_val[(size_t)t * r + col];
  }

  int rc = 0;
  if (!rc) rc = up(h->owned, &h->gram.h, hp.data(), hp.size());
  if (!rc) rc = up(h->owned, &d.tvu, tvu.data(), tvu.size());
  if (!rc) rc = up(h->owned, &d.kmeta, kmeta.data(), kmeta.size());
  if (!rc) rc = up(h->owned, &d.rhs_tv, rtv.data(), rtv.size());
  if (!rc) rc = up(h->owned, &d.rhs_pidx, rpi.data(), rpi.size());
  if (!rc) rc = up(h->owned, &d.rhs_f, rf.data(), rf.size());
  if (!rc) rc = up(h->owned, &d.obs_phi, a->obs_phi, (size_t)a->n_obs * r);
  if (rc) { finrom_rom_destroy(h); return rc; }
  *out = h;
  return 0;
}

}  // extern "C"
// a half list (finrom_rom_set_mirror / _short) appended behind the handle's grouped tables: records, rows and factors go behind
// what is there, everything is uploaded again; nd gets the new arrays and n_ext, kmg0 = where the list's records start
struct HostTables { std::vector<double> tvg; std::vector<int> kmg, def; };
static int append_half_list(finrom_rom_t h, const finrom_rom_desc* a, const double* row_weight, RomDev& nd, GroupedTables& g, int& kmg0,
                            HostTables& next, const char* who) {
  std::vector<int> kclass;
  const std::vector<KStep> ksteps = mirror_ksteps(a, row_weight, kclass);
  const int slot0 = (int)(h->tvg_host.size() / ((size_t)4 * nd.rp));
  if (!build_grouped_tables(a, ksteps, nd.rp, g, &kclass, slot0, nd.n_ext, short_scale_free(a, h->short_grouped))) { set_error(std::string(who) + ": the half descriptor has no grouped form"); return FINROM_ERR_UNSUPPORTED; }
  std::vector<double> tvg(h->tvg_host); tvg.insert(tvg.end(), g.tvg.begin(), g.tvg.end());
  std::vector<int> kmg(h->kmg_host); kmg.insert(kmg.end(), g.kmg.begin(), g.kmg.end());
  std::vector<int> def(h->def_host); def.insert(def.end(), g.def.begin(), g.def.end());
  if (tvg.size() * sizeof(double) > (size_t)0x7FFFFFF0) { set_error(std::string(who) + ": tables too large"); return FINROM_ERR_UNSUPPORTED; }
  int rc = up(h->owned, &nd.tvg, tvg.data(), tvg.size());
  if (!rc) rc = up(h->owned, &nd.kmg, kmg.data(), kmg.size());
  if (!rc) rc = up(h->owned, &nd.ext_def, def.data(), def.size());
  if (rc) return rc;
  kmg0 = (int)h->kmg_host.size();
  nd.tvg_bytes = (int)(tvg.size() * sizeof(double)); nd.n_ext = g.n_ext;
  next.tvg.swap(tvg); next.kmg.swap(kmg); next.def.swap(def);      // (the caller commits them with nd once nothing can fail any more)
  return 0;
}
extern "C" {

int finrom_rom_set_mirror(finrom_rom_t h, const finrom_rom_desc* a, const int32_t* row_node, const double* row_weight,
                          const int32_t* theta_twin) {
  if (!h || !a) { set_error("rom_set_mirror: null argument"); return FINROM_ERR_ARG; }
  RomDev& d = h->d;
  if (int rc = validate_rom_mirror(a, d.n, row_node, row_weight, theta_twin)) return rc;
  if (a->r != d.r || a->P != d.P) { set_error("rom_set_mirror: basis size / parameter count differ from the handle's"); return FINROM_ERR_ARG; }
  if (d.nkg_m > 0) { set_error("rom_set_mirror: already installed"); return FINROM_ERR_ARG; }
  // the one-wave grouped kernel is the only form that walks the half list
  if (d.NB > 5 || d.nkg == 0) { set_error("rom_set_mirror: the handle has no grouped form (r > 80, FINROM_PROJ_UNGROUPED, nothing to group)"); return FINROM_ERR_UNSUPPORTED; }
  GroupedTables g;
  int kmg0 = 0;
  RomDev nd = d;
  HostTables next;
  if (int rc = append_half_list(h, a, row_weight, nd, g, kmg0, next, "rom_set_mirror")) return rc;
  if (int rc = up(h->owned, &nd.twin, theta_twin, (size_t)d.P)) return rc;      // (the handle keeps its tables; what was uploaded is freed with it)
  nd.kmg_m = kmg0; nd.nkg_m = g.nkg; nd.ext_final_m = g.ext_final;
  d = nd;
  h->tvg_host.swap(next.tvg); h->kmg_host.swap(next.kmg); h->def_host.swap(next.def);
  h->mirror_n = a->n;
  h->mirror_counts[0][0] = (int)rows_by_term_count(a).size(); h->mirror_counts[0][1] = g.live; h->mirror_counts[0][2] = g.fma_ksteps;
  return 0;
}

int finrom_rom_set_mirror_short(finrom_rom_t h, const finrom_rom_desc* a, const double* row_weight, double theta_lo, double theta_hi) {
  if (!h || !a || !row_weight) { set_error("rom_set_mirror_short: null argument"); return FINROM_ERR_ARG; }
  RomDev& d = h->d;
  if (d.nkg_m == 0) { set_error("rom_set_mirror_short: finrom_rom_set_mirror comes first"); return FINROM_ERR_ARG; }
  if (d.nkg_s > 0) { set_error("rom_set_mirror_short: already installed"); return FINROM_ERR_ARG; }
  if (int rc = validate_rom_desc(a)) return rc;
  if (a->r != d.r || a->P != d.P || a->n != h->mirror_n) { set_error("rom_set_mirror_short: sizes differ from the half descriptor's"); return FINROM_ERR_ARG; }
  if (!(theta_lo > 0.0 && theta_lo <= theta_hi)) { set_error("rom_set_mirror_short: need 0 < theta_lo <= theta_hi"); return FINROM_ERR_ARG; }
  if (int rc = validate_row_weights(a, row_weight)) return rc;
  GroupedTables g;
  int kmg0 = 0;
  RomDev nd = d;
  HostTables next;
  if (int rc = append_half_list(h, a, row_weight, nd, g, kmg0, next, "rom_set_mirror_short")) return rc;
  nd.kmg_s = kmg0; nd.nkg_s = g.nkg; nd.ext_final_s = g.ext_final; nd.short_lo = theta_lo; nd.short_hi = theta_hi;
  d = nd;
  h->tvg_host.swap(next.tvg); h->kmg_host.swap(next.kmg); h->def_host.swap(next.def);
  h->mirror_counts[1][0] = (int)rows_by_term_count(a).size(); h->mirror_counts[1][1] = g.live; h->mirror_counts[1][2] = g.fma_ksteps;
  return 0;
}

// the compact list (DESIGN 4b''): a fourth list behind the short one, from the short descriptor's rows rotated per pattern class
// (finrom_rom_compact_rows) with the rows below the caller's threshold left out.  No kernel knows it: a launch that offers it
// (rom_project) hands the kernel its records in the short list's place, so the samples that pass the short list's tests walk it.
int finrom_rom_set_mirror_compact(finrom_rom_t h, const finrom_rom_desc* a, const double* row_weight) {
  if (!h || !a || !row_weight) { set_error("rom_set_mirror_compact: null argument"); return FINROM_ERR_ARG; }
  RomDev& d = h->d;
  if (d.nkg_s == 0) { set_error("rom_set_mirror_compact: finrom_rom_set_mirror_short comes first"); return FINROM_ERR_ARG; }
  if (h->nkg_c > 0) { set_error("rom_set_mirror_compact: already installed"); return FINROM_ERR_ARG; }
  if (int rc = validate_rom_desc(a)) return rc;
  if (a->r != d.r || a->P != d.P || a->n != h->mirror_n) { set_error("rom_set_mirror_compact: sizes differ from the half descriptor's"); return FINROM_ERR_ARG; }
  if (int rc = validate_row_weights(a, row_weight)) return rc;
  GroupedTables g;
  int kmg0 = 0;
  RomDev nd = d;
  HostTables next;
  if (int rc = append_half_list(h, a, row_weight, nd, g, kmg0, next, "rom_set_mirror_compact")) return rc;
  d = nd;
  h->kmg_c = kmg0; h->nkg_c = g.nkg; h->ext_final_c = g.ext_final;
  h->tvg_host.swap(next.tvg); h->kmg_host.swap(next.kmg); h->def_host.swap(next.def);
  h->mirror_counts[2][0] = (int)rows_by_term_count(a).size(); h->mirror_counts[2][1] = g.live; h->mirror_counts[2][2] = g.fma_ksteps;
  return 0;
}

int finrom_rom_mirror_info(finrom_rom_t h, int32_t which, int32_t* live_rows, int32_t* ksteps, int32_t* fma_ksteps) {
  if (!h || !live_rows || !ksteps || !fma_ksteps || which < 0 || which > 2) { set_error("rom_mirror_info: bad argument"); return FINROM_ERR_ARG; }
  *live_rows = h->mirror_counts[which][0]; *ksteps = h->mirror_counts[which][1]; *fma_ksteps = h->mirror_counts[which][2];      // (zeros: not installed)
  return 0;
}

int finrom_rom_last_form(finrom_rom_t h) {
  if (!h) { set_error("rom_last_form: null handle"); return FINROM_ERR_ARG; }
  return h->last_form;
}

int finrom_rom_last_epilogue(finrom_rom_t h) {
  if (!h) { set_error("rom_last_epilogue: null handle"); return FINROM_ERR_ARG; }
  return h->last_epilogue;
}

void finrom_rom_destroy(finrom_rom_t h) {
  if (!h) return;
  for (void* p : h->owned) dev_free(p);
  h->Ar.release(); h->Br.release(); h->theta.release(); h->qtmp.release(); h->vw.release(); h->grad_ticket.release();
  h->part.release(); h->ext.release();
  if (h->side) defer_or_run([](void* s) { (void)hipStreamDestroy((hipStream_t)s); }, h->side);
  if (h->fom_side) defer_or_run([](void* s) { (void)hipStreamDestroy((hipStream_t)s); }, h->fom_side);
  if (h->ev_join_fom) defer_or_run([](void* e) { (void)hipEventDestroy((hipEvent_t)e); }, h->ev_join_fom);
  if (h->ev_fork) defer_or_run([](void* e) { (void)hipEventDestroy((hipEvent_t)e); }, h->ev_fork);
  if (h->ev_join) defer_or_run([](void* e) { (void)hipEventDestroy((hipEvent_t)e); }, h->ev_join);
  delete h;
}

int finrom_rom_set_gram(finrom_rom_t h, int32_t npairs, const int32_t* pair_p, const int32_t* pair_q, const double* G) {
  if (!h || npairs <= 0 || !pair_p || !pair_q || !G) { set_error("rom_set_gram: bad argument"); return FINROM_ERR_ARG; }
  if (npairs > ROM_GRAM_MAX_PAIRS) { set_error("rom_set_gram: more than 64 pairs"); return FINROM_ERR_UNSUPPORTED; }
  const RomDev& d = h->d;
  const int r = d.r, R = d.rp, NB = d.NB;
  for (int t = 0; t < npairs; ++t)
    if (pair_p[t] < 0 || pair_q[t] > d.P || pair_p[t] > pair_q[t]) { set_error("rom_set_gram: invalid pair (need 0 <= p <= q <= P)"); return FINROM_ERR_ARG; }
  for (int t = 0; t < npairs; ++t)
    for (int u = 0; u < t; ++u)
      if (pair_p[t] == pair_p[u] && pair_q[t] == pair_q[u]) { set_error("rom_set_gram: duplicate pair"); return FINROM_ERR_ARG; }
  auto at = [&](int t, int i, int j) { return (i < r && j < r) ? G[((size_t)t * r + i) * r + j] : 0.0; };
  for (int t = 0; t < npairs; ++t)
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < i; ++j) {
        const double x = at(t, i, j), y = at(t, j, i);
        if (!(std::fabs(x - y) <= 1e-12 * (std::fabs(x) + std::fabs(y)) + 1e-300)) { set_error("rom_set_gram: block is not symmetric"); return FINROM_ERR_ARG; }
      }
  int rc = 0;
  RomGramDev gm = h->gram;
  if (!rc) rc = up(h->owned, &gm.pair_p, pair_p, npairs);
  if (!rc) rc = up(h->owned, &gm.pair_q, pair_q, npairs);
  if (NB <= 6) {       // tile images: lane (q, c), register g of tile (ti <= tj) holds entry (16 ti + q + 4 g, 16 tj + c)
    const int NT = NB * (NB + 1) / 2;
    std::vector<double> Gt((size_t)npairs * NT * 256, 0.0);
    for (int t = 0; t < npairs; ++t) {
      int tile = 0;
      for (int ti = 0; ti < NB; ++ti)
        for (int tj = ti; tj < NB; ++tj, ++tile)
          for (int lane = 0; lane < 64; ++lane)
            for (int g = 0; g < 4; ++g)
              Gt[(((size_t)t * NT + tile) * 64 + lane) * 4 + g] = at(t, 16 * ti + (lane >> 4) + 4 * g, 16 * tj + (lane & 15));
    }
    if (!rc) rc = up(h->owned, &gm.Gt, Gt.data(), Gt.size());
  } else {             // packed upper triangle, row by row (= the lower triangle by columns the Cholesky kernels read)
    const size_t np = (size_t)R * (R + 1) / 2;
    std::vector<double> Gp((size_t)npairs * np, 0.0);
    for (int t = 0; t < npairs; ++t)
      for (int row = 0; row < r; ++row)
        for (int col = row; col < r; ++col) Gp[t * np + (size_t)row * R - ((size_t)row * (row - 1)) / 2 + col - row] = at(t, row, col);
    if (!rc) rc = up(h->owned, &gm.Gp, Gp.data(), Gp.size());
  }
  if (rc) return rc;
  gm.npairs = npairs;
  h->gram = gm;
  return 0;
}

int finrom_rom_set_projection(finrom_rom_t h, int32_t mode) {
  if (!h || (mode != FINROM_PROJECTION_DIRECT && mode != FINROM_PROJECTION_GRAM)) { set_error("rom_set_projection: bad argument"); return FINROM_ERR_ARG; }
  if (mode == FINROM_PROJECTION_GRAM && h->gram.npairs == 0) { set_error("rom_set_projection: finrom_rom_set_gram has not been called"); return FINROM_ERR_ARG; }
  h->projection = mode;
  return 0;
}

}  // extern "C"
// A_r, B_r (or, with factor > 0, the factor / the solution) by the form of the reduced operator the handle is set to
// (mirror: the call may offer the half list of finrom_rom_set_mirror to its samples -- finrom_rom_solve only)
static int rom_project(finrom_rom_t h, const double* theta, int64_t S, int factor, int* info, hipStream_t st,
                       double* w_r = nullptr, double* qoi_r = nullptr, bool mirror = false, bool roomy = false, bool short_waits = false,
                       bool block_row = false, bool compact = false) {
  h->last_form = FINROM_ROM_FORM_FULL;
  roomy = roomy && h->projection == FINROM_PROJECTION_DIRECT && rom_roomy_applies(h->d, factor, w_r, qoi_r);
  block_row = roomy && block_row;
  short_waits = roomy && (short_waits || block_row);      // (the block-row elimination is a form of the short-waits epilogue)
  h->last_epilogue = !roomy ? FINROM_ROM_EPILOGUE_STANDARD : block_row ? FINROM_ROM_EPILOGUE_ROOMY_BLOCK_ROW :
                     short_waits ? FINROM_ROM_EPILOGUE_ROOMY_SHORT_WAITS : FINROM_ROM_EPILOGUE_ROOMY;
  if (h->projection == FINROM_PROJECTION_GRAM)
    return launch_rom_gram(h->d, h->gram, theta, S, (double*)h->Ar.p, (double*)h->Br.p, factor, info, st, w_r, qoi_r);
  RomDev d = h->d;
  d.ext = nullptr;
  if (!mirror) d.nkg_m = d.nkg_s = 0;
  // (compact: the call offers the compact list -- the samples that would walk the short list walk it instead, same tests, same kernel)
  if (compact && d.nkg_s > 0 && h->nkg_c > 0) { d.kmg_s = h->kmg_c; d.nkg_s = h->nkg_c; d.ext_final_s = h->ext_final_c; }
  if (d.nkg > 0 && S > 0 && (roomy || !rom_splitk_applies(d, S))) {      // the grouped main loop: room for the samples' scalars
    if (int rc = h->ext.reserve((size_t)S * d.n_ext * sizeof(double))) return rc;
    d.ext = (double*)h->ext.p;
    if (d.nkg_m > 0) h->last_form = FINROM_ROM_FORM_HALF;
  }
  return launch_rom_proj(d, theta, S, (double*)h->Ar.p, (double*)h->Br.p, factor, info, st, w_r, qoi_r, roomy, short_waits, block_row);
}

// the workspace bound of one piece of a batch (the packed A_r and B_r of its samples): 16 GiB; FINROM_ROM_WORKSPACE_BYTES=<n>, read
// per call, puts another bound in its place so that a test can make a small batch run in pieces (the shape of api_fom.hip's
// fom_piece_samples).  Pieces are multiples of four samples, four at the least.  rom_solve_impl then makes its pieces equal (a piece
// chooses its form by its own size); finrom_rom_grad cuts whole pieces and leaves the rest to the last one.
// NOT for finrom_romml_grad: its one-sample form needs finrom_rom_grad to run the batch in one piece (defer_sum) and says so with an
// error when the switch cuts a batch of <= 64 samples; include/finrom.h says the switch is not supported there.
static int64_t rom_piece_samples(size_t per_sample) {
  const char* env_ws = getenv("FINROM_ROM_WORKSPACE_BYTES");
  const int64_t env_bound = env_ws != nullptr ? (int64_t)atoll(env_ws) : 0;
  const int64_t bound = env_bound > 0 ? env_bound : (int64_t)((size_t)16 << 30);
  return std::max<int64_t>(4, bound / (int64_t)per_sample / 4 * 4);
}

// roomy: finrom_solve_pairs beside the FOM's half sweep -- QoI-only calls at r <= 80 then take the 256-register one-wave kernel at
// every batch size (rom_roomy_applies); finrom_rom_solve itself never does.  short_waits: that kernel's form without the fixed waits
// between accumulate-chained MFMAs (finrom_rom_s::short_waits says where).  block_row: the short-waits form that eliminates each block
// row in place instead of forming U_kk^-T (finrom_rom_s::block_row says where)
static int rom_solve_impl(finrom_rom_t h, const double* theta, int64_t S, double* w_r, double* qoi_r, double* A_r,
                          double* B_r, int32_t* info, void* stream, bool roomy, bool short_waits = false, bool block_row = false,
                          bool compact = false) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!theta || (!qoi_r && h->d.n_obs > 0)))) { set_error("rom_solve: bad argument"); return FINROM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const RomDev& d = h->d;
  const size_t per_sample = ((size_t)d.rp * (d.rp + 1) / 2 + d.rp) * sizeof(double);
  int64_t chunk = rom_piece_samples(per_sample);
  if (S > chunk) { const int64_t np = (S + chunk - 1) / chunk; chunk = ((S + np - 1) / np + 3) / 4 * 4; }      // equal pieces
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t Sc = std::min(chunk, S - s0);
    int rc;
    // one-sample call patterns (MAP / HMC: a handful of samples, latency): contraction over several workgroups per sample, then
    // the MFMA-form factorisation + substitutions (rom_onesample.hip)
    const bool rm = roomy && A_r == nullptr && B_r == nullptr && h->projection == FINROM_PROJECTION_DIRECT && rom_roomy_applies(d, 2, w_r, qoi_r);
    if (!rm && A_r == nullptr && B_r == nullptr && h->projection == FINROM_PROJECTION_DIRECT && rom_onesample_applies(d, Sc)) {
      h->last_epilogue = FINROM_ROM_EPILOGUE_STANDARD;
      if ((rc = h->part.reserve(rom_onesample_scratch_bytes(d, Sc)))) return rc;
      h->last_form = FINROM_ROM_FORM_FULL;
      if ((rc = launch_rom_onesample(d, theta + s0 * d.P, Sc, (double*)h->part.p, 0, RomGradArgs(), w_r ? w_r + s0 * d.r : nullptr,
                                     qoi_r ? qoi_r + s0 * d.n_obs : nullptr, info ? info + s0 : nullptr, st))) return rc;
      continue;
    }
    if ((rc = h->Ar.reserve((size_t)Sc * (d.rp * (d.rp + 1) / 2) * sizeof(double)))) return rc;
    if ((rc = h->Br.reserve((size_t)Sc * d.rp * sizeof(double)))) return rc;
    // A_r is factored inside the projection kernel (in registers, MFMA trailing updates) unless the caller
    // wants A_r itself back (the state the reference's gradients use) or the basis needs more than one wave
    const bool want_factor = A_r == nullptr;
    int factor = (want_factor && d.NB <= 6) ? 1 : 0;                  // in-register, inside the projection kernel
    // ... and when neither A_r nor B_r is wanted back (r <= 80), the two substitutions and the reduced QoI happen there
    // as well: no packed factor in memory, no second kernel
    if (factor && (d.NB <= 5 || (d.NB == 6 && h->projection == FINROM_PROJECTION_DIRECT && rom_splitk_applies(d, Sc))) && A_r == nullptr && B_r == nullptr)
      factor = 2;
    // wider bases, only the reduced QoI wanted (the sample-pair path): factorisation and QoI stay in the registers of the
    // projection kernel's waves (fused_solve_mw); A_r never reaches memory
    if (d.NB > 6 && want_factor && h->projection == FINROM_PROJECTION_DIRECT && A_r == nullptr && B_r == nullptr && w_r == nullptr &&
        qoi_r != nullptr && d.n_obs + 1 <= 16 * 3) factor = 3;
    if ((rc = rom_project(h, theta + s0 * d.P, Sc, factor, info ? info + s0 : nullptr, st,
                          w_r ? w_r + s0 * d.r : nullptr, qoi_r ? qoi_r + s0 * d.n_obs : nullptr, true, rm, short_waits, block_row, compact))) return rc;
    if (factor >= 2) continue;
    int factored = factor;
    if (want_factor && d.NB > 6) {                                     // wider bases: blocked MFMA Cholesky kernel
      if ((rc = launch_rom_chol_blocked(d, (double*)h->Ar.p, Sc, info ? info + s0 : nullptr, st))) return rc;
      factored = 1;
    }
    if ((rc = launch_rom_solve(d, (const double*)h->Ar.p, (const double*)h->Br.p, Sc, w_r ? w_r + s0 * d.r : nullptr,
                               qoi_r ? qoi_r + s0 * d.n_obs : nullptr, A_r ? A_r + s0 * (int64_t)d.r * d.r : nullptr,
                               B_r ? B_r + s0 * d.r : nullptr, info ? info + s0 : nullptr, factored, st))) return rc;
  }
  return 0;
}
extern "C" {

int finrom_rom_solve(finrom_rom_t h, const double* theta, int64_t S, double* w_r, double* qoi_r, double* A_r,
                     double* B_r, int32_t* info, void* stream) {
  return rom_solve_impl(h, theta, S, w_r, qoi_r, A_r, B_r, info, stream, false, false, false, h ? h->compact(false) : false);
}

int finrom_rom_set_gradient(finrom_rom_t h, int32_t npairs, const int32_t* pair_p, const int32_t* pair_i, const double* G) {
  if (!h || npairs < 0 || (npairs > 0 && (!pair_p || !pair_i || !G))) { set_error("rom_set_gradient: bad argument"); return FINROM_ERR_ARG; }
  for (int t = 0; t < npairs; ++t)
    if (pair_p[t] < 0 || pair_p[t] > h->d.P || pair_i[t] < 0 || pair_i[t] >= h->d.P) { set_error("rom_set_gradient: invalid pair"); return FINROM_ERR_ARG; }
  int rc = 0;
  if (!rc) rc = up(h->owned, &h->g_pair_p, pair_p, npairs);
  if (!rc) rc = up(h->owned, &h->g_pair_i, pair_i, npairs);
  if (!rc) rc = up(h->owned, &h->g_Gt, G, (size_t)npairs * h->d.r * h->d.r);
  if (rc) return rc;
  h->g_npairs = npairs;
  return 0;
}

int finrom_rom_grad(finrom_rom_t h, const double* theta, const double* data, int32_t data_per_sample, int64_t S,
                    double* J, double* g, double* w_r, double* qoi_r, int32_t* info, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!theta || !data || !J || !g))) { set_error("rom_grad: bad argument"); return FINROM_ERR_ARG; }
  if (h->g_npairs == 0) { set_error("rom_grad: finrom_rom_set_gradient has not been called"); return FINROM_ERR_ARG; }
  const RomDev& d = h->d;
  hipStream_t st = (hipStream_t)stream;
  const size_t per_sample = ((size_t)d.rp * (d.rp + 1) / 2 + d.rp) * sizeof(double);
  const int64_t chunk = rom_piece_samples(per_sample);
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t Sc = std::min(chunk, S - s0);
    int rc;
    if ((rc = h->Ar.reserve((size_t)Sc * (d.rp * (d.rp + 1) / 2) * sizeof(double)))) return rc;
    if ((rc = h->Br.reserve((size_t)Sc * d.rp * sizeof(double)))) return rc;
    double* q = qoi_r ? qoi_r + s0 * d.n_obs : nullptr;
    if (!q) { if ((rc = h->qtmp.reserve((size_t)Sc * d.n_obs * sizeof(double)))) return rc; q = (double*)h->qtmp.p; }
    // one-sample call patterns (MAP / HMC), 48 < r <= 96, the per-sample contraction: projection split over four waves, both
    // solves in registers, the gradient contraction dealt over the same waves -- one kernel, nothing but the outputs written
    if (h->projection == FINROM_PROJECTION_DIRECT && rom_onesample_applies(d, Sc)) {
      // contraction over several workgroups per sample, MFMA-form factorisation + forward / adjoint solves (rom_onesample.hip),
      // then the gradient contraction dealt over 36 workgroups per sample
      h->last_form = FINROM_ROM_FORM_FULL; h->last_epilogue = FINROM_ROM_EPILOGUE_STANDARD;      // (this branch's own projection launch)
      RomGradArgs ga;
      ga.data = data + (data_per_sample ? s0 * d.n_obs : 0); ga.data_stride = data_per_sample ? d.n_obs : 0;
      ga.theta = theta + s0 * d.P; ga.J = J + s0; ga.g = g + s0 * d.P;
      ga.npairs = h->g_npairs; ga.pair_p = h->g_pair_p; ga.pair_i = h->g_pair_i; ga.Gt = h->g_Gt;
      const size_t vw_bytes = (size_t)Sc * 2 * d.rp * sizeof(double), gp_bytes = (size_t)Sc * ROM_GRAD_SMALL_NG * 32 * sizeof(double);
      if ((rc = h->vw.reserve(vw_bytes + gp_bytes))) return rc;
      if ((rc = h->part.reserve(rom_onesample_scratch_bytes(d, Sc)))) return rc;
      if (!h->grad_ticket.p) {                          // arrival counters: zero once, the kernel leaves them zero
        if ((rc = h->grad_ticket.reserve(ROM_SPLITK_MAX_S * sizeof(int)))) return rc;
        FR_HIP(hipMemset(h->grad_ticket.p, 0, ROM_SPLITK_MAX_S * sizeof(int)));
      }
      ga.vw = (double*)h->vw.p; ga.gpart = (double*)((char*)h->vw.p + vw_bytes); ga.ticket = (int*)h->grad_ticket.p;
      ga.defer_sum = h->defer_gsum && s0 == 0 && Sc == S;
      ga.info_store = ga.defer_sum && h->info_store;
      h->last_gpart = ga.defer_sum ? ga.gpart : nullptr;
      if ((rc = launch_rom_onesample(d, theta + s0 * d.P, Sc, (double*)h->part.p, 1, ga, w_r ? w_r + s0 * d.r : nullptr, q,
                                     info ? info + s0 : nullptr, st, ga.defer_sum ? h->fuse : nullptr))) return rc;
      if ((rc = launch_rom_grad_contract_small(d, Sc, ga, st, ga.defer_sum ? h->back : nullptr))) return rc;
      continue;
    }
    if (h->projection == FINROM_PROJECTION_DIRECT && rom_splitk_applies(d, Sc) && d.n_obs <= 64) {
      h->last_form = FINROM_ROM_FORM_FULL; h->last_epilogue = FINROM_ROM_EPILOGUE_STANDARD;      // (this branch's own projection launch)
      RomGradArgs ga;
      ga.data = data + (data_per_sample ? s0 * d.n_obs : 0); ga.data_stride = data_per_sample ? d.n_obs : 0;
      ga.theta = theta + s0 * d.P; ga.J = J + s0; ga.g = g + s0 * d.P;
      ga.npairs = h->g_npairs; ga.pair_p = h->g_pair_p; ga.pair_i = h->g_pair_i; ga.Gt = h->g_Gt;
      const size_t vw_bytes = (size_t)Sc * 2 * d.rp * sizeof(double), gp_bytes = (size_t)Sc * ROM_GRAD_SMALL_NG * 32 * sizeof(double);
      if ((rc = h->vw.reserve(vw_bytes + gp_bytes))) return rc;
      if (!h->grad_ticket.p) {                          // arrival counters: zero once, the kernel leaves them zero
        if ((rc = h->grad_ticket.reserve(ROM_SPLITK_MAX_S * sizeof(int)))) return rc;
        FR_HIP(hipMemset(h->grad_ticket.p, 0, ROM_SPLITK_MAX_S * sizeof(int)));      // synchronous: ordered before ANY stream's first use
      }
      ga.vw = (double*)h->vw.p; ga.gpart = (double*)((char*)h->vw.p + vw_bytes); ga.ticket = (int*)h->grad_ticket.p;
      {
        ScopedKernelTimer t(K_ROM_PROJ, st);
        if ((rc = launch_rom_proj_splitk(d, theta + s0 * d.P, Sc, (double*)h->Ar.p, (double*)h->Br.p, 4, info ? info + s0 : nullptr, st,
                                         w_r ? w_r + s0 * d.r : nullptr, q, ga))) return rc;
      }
      if ((rc = launch_rom_grad_contract_small(d, Sc, ga, st))) return rc;
      continue;
    }
    // the factor of A_r: inside the projection kernel for r <= 96, by the blocked MFMA Cholesky kernel for wider bases
    if ((rc = rom_project(h, theta + s0 * d.P, Sc, d.NB <= 6 ? 1 : 0, info ? info + s0 : nullptr, st))) return rc;
    if (d.NB > 6 && (rc = launch_rom_chol_blocked(d, (double*)h->Ar.p, Sc, info ? info + s0 : nullptr, st))) return rc;
    RomGradArgs ga;
    ga.data = data + (data_per_sample ? s0 * d.n_obs : 0); ga.data_stride = data_per_sample ? d.n_obs : 0;
    ga.theta = theta + s0 * d.P; ga.J = J + s0; ga.g = g + s0 * d.P;
    ga.npairs = h->g_npairs; ga.pair_p = h->g_pair_p; ga.pair_i = h->g_pair_i; ga.Gt = h->g_Gt;
    // batches: the contraction with the blocks G_pi runs on the matrix cores for 16 samples at a time; a handful of samples
    // (the one-sample call pattern) keep it inside the substitution kernel (one launch less)
    const bool batched = Sc >= 64 && d.n_obs <= 64;
    if (batched) {
      if ((rc = h->vw.reserve((size_t)Sc * 2 * d.rp * sizeof(double)))) return rc;
      ga.vw = (double*)h->vw.p;
    }
    if ((rc = launch_rom_grad(d, (const double*)h->Ar.p, (const double*)h->Br.p, Sc, w_r ? w_r + s0 * d.r : nullptr, q,
                              info ? info + s0 : nullptr, ga, st))) return rc;
    if (batched && (rc = launch_rom_grad_contract(d, Sc, ga, st))) return rc;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
int finrom_subfin_avg(const double* Sop, int32_t P, int32_t n, const double* k, int64_t S, double* theta, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!Sop || P <= 0 || n <= 0 || S < 0 || (S > 0 && (!k || !theta))) { set_error("subfin_avg: bad argument"); return FINROM_ERR_ARG; }
  return launch_subfin_avg(Sop, P, n, k, S, theta, (hipStream_t)stream);
}

}  // extern "C"
// FINROM_TRACE=<prefix>: every finrom_solve_pairs call records, per workgroup of the FOM interpreter and of the
// projection kernel, {start, end, HW_ID, XCC_ID} and rewrites <prefix>.fom.bin / <prefix>.proj.bin (int64 x 6 per
// workgroup) after a device synchronisation.  Diagnostic for the co-residency of the two halves.
static long long* g_trace_buf[2] = {nullptr, nullptr};
static constexpr size_t kTraceWg = 1u << 18;
static const char* trace_prefix() { static const char* p = getenv("FINROM_TRACE"); return p; }
static int trace_dump(const char* kind, long long* dbuf, size_t nwg) {
  std::vector<long long> h(nwg * 6);
  FR_HIP(hipDeviceSynchronize());
  FR_HIP(hipMemcpy(h.data(), dbuf, nwg * 6 * sizeof(long long), hipMemcpyDeviceToHost));
  const std::string path = std::string(trace_prefix()) + "." + kind + ".bin";
  if (FILE* f = fopen(path.c_str(), "wb")) { fwrite(h.data(), sizeof(long long), h.size(), f); fclose(f); }
  return 0;
}
extern "C" {

int finrom_solve_pairs(finrom_fom_t fom, finrom_rom_t rom, const double* Sop, const double* x, int64_t S,
                       double* qoi, double* qoi_r, double* err, double* w, double* w_r, double* theta,
                       int32_t* info, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!fom || !rom || !Sop || S < 0 || (S > 0 && (!x || !qoi || !qoi_r))) { set_error("solve_pairs: bad argument"); return FINROM_ERR_ARG; }
  if (fom->d.n_obs != rom->d.n_obs) { set_error("solve_pairs: FOM and ROM observation operators differ in size"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = rom->ensure_side())) return rc;
  if (!theta) {
    if ((rc = rom->theta.reserve((size_t)S * rom->d.P * sizeof(double)))) return rc;
    theta = (double*)rom->theta.p;
  }
  // The two halves run on two streams (FINROM_NO_OVERLAP / finrom_set_overlap(0): in turn, for per-kernel profiling).  With the
  // band sweep as the FOM half (HBM-bound, one 300-register wave per SIMD, vector units 80 % idle) a projection wave fits beside
  // every sweep wave, and since the projection hides its non-MFMA work behind its own MFMAs a lone wave per SIMD is efficient:
  // measured 26.3 ms side by side against 29.1 ms in turn per 100k samples (r = 80).
  static const bool env_no_overlap = getenv("FINROM_NO_OVERLAP") != nullptr;      // (read once, not per call)
  // (The four-wave band sweep of m = 16, 20 takes a whole CU's LDS -- 157 KB per workgroup -- and the wide-basis projection 43 KB
  // per workgroup: the two kernels cannot share a CU, side by side they take turns CU by CU at the dispatcher's discretion.  That
  // still beats running them in turn by 1-5 % (r = 200: 68.6 against 72.0 ms per 20k samples, 420 against 425 ms per 125k), so
  // those sizes fork too; their event-timed kernel durations then include waiting for CUs -- FINROM_NO_OVERLAP=1 gives clean ones.)
  const bool overlap = overlap_enabled() && !env_no_overlap;
  hipStream_t side = overlap ? rom->side : st;
  const bool tracing = trace_prefix() != nullptr;
  if (tracing) {
    for (int i = 0; i < 2; ++i)
      if (!g_trace_buf[i]) FR_HIP(hipMalloc((void**)&g_trace_buf[i], kTraceWg * 6 * sizeof(long long)));
    FR_HIP(hipMemset(g_trace_buf[0], 0, kTraceWg * 6 * sizeof(long long)));
    FR_HIP(hipMemset(g_trace_buf[1], 0, kTraceWg * 6 * sizeof(long long)));
    FR_HIP(hipDeviceSynchronize());
    fom->d.trace = (size_t)((S + 63) / 64) <= kTraceWg ? g_trace_buf[0] : nullptr;
    rom->d.trace = (size_t)S <= kTraceWg ? g_trace_buf[1] : nullptr;
  }
  // (the fork below: everything already queued on the caller's stream -- inputs, zeroed info -- precedes both halves)
  // ROM half first, on a high-priority stream: its 4-wave, 160-VGPR workgroups need large contiguous
  // register ranges, so they claim their slots before the small FOM waves fill the remaining ones
  // The FOM's short bandwidth-bound pre-pass (pack + assembly) used to run first, alone: beside the projection kernel it crawls and
  // the interpreter of round 1, whose waves then started late, WAS the critical path.  Since the band sweep the FOM half ends
  // long before the ROM half (6.8 against 21.8 ms side by side at the headline), so the pre-pass now runs after the fork, on the
  // FOM side, and only the sub-fin averages -- the head of the ROM half -- precede it.
  // Every workspace the two halves need is reserved BEFORE the fork: an allocation failure after it would return while the
  // side stream still writes the caller's outputs.  Any other failure after the fork joins the side stream first.
  const BandDev& fband = fom->band_for(w != nullptr);
  const bool split = S <= fom_chunk_samples(fom->d, &fband);
  // Round 4: beside the ONE-WAVE projection kernel (r <= 80, two 200-register waves per SIMD) the register band sweep (m <= 12, one
  // 312-register wave per SIMD) runs on a stream masked to THREE CUs of every shader engine (96 of 256): what the projection loses is
  // proportional to the CU-time it shares with sweep waves, and confined to fewer CUs the sweep's waves -- fewer at a time, less
  // contention for HBM -- need less of it in total (256 CUs x 6.9 ms -> 96 x 15.3 ms; the sweep still ends long before the projection).
  // Measured, headline: step 21.54 -> 20.92 ms; two CUs per engine make the sweep the longer half (22.4), four give 21.06.  NOT for the
  // multi-wave projection kernels (r = 120: 49.7 -> 56.7 ms, their workgroups leave the confined sweep too few slots), the four-wave
  // sweep (LDS-exclusive: no change) or the offline/online form (FOM-bound: 9.1 -> 14.3).  FINROM_FOM_CUS=<n> forces n CUs (0: off).
  static const int env_fom_cus = getenv("FINROM_FOM_CUS") != nullptr ? atoi(getenv("FINROM_FOM_CUS")) : -1;
  const bool no_band = env_no_band();
  int fom_cus = env_fom_cus;
  // The half plan of a mirror-symmetric operator (finrom_fom_set_band_mirror: a 154-register wave, 60 KB per sample, 1.3 ms alone)
  // is confined to ONE CU of every shader engine: it then lives 6.1 ms on 32 CUs instead of 3.1 ms on 96, still a third of the
  // projection's time, and the projection loses least.  Headline, step in ms: unmasked 19.48, one CU per engine 19.06, two 19.20,
  // three 19.32 (the full plan with three: 20.11-20.15).
  const bool half_plan = &fband == &fom->band_m;
  // (what the default is, whatever FINROM_FOM_CUS, the caller's stream or the overlap switch then make of it: the block-row epilogue
  // below follows THIS, because it returns other bits than the kernels beside it and a call's bits must not depend on the mask)
  const bool mask_by_default = rom->projection == FINROM_PROJECTION_DIRECT && rom->d.NB <= 5 && fom->band.on && fom->band.NSP <= 14 && !no_band &&
                               w == nullptr && S >= 16384;
  if (fom_cus < 0) fom_cus = mask_by_default ? (half_plan ? -1 : -3) : 0;
  hipStream_t fst = st;
  if (overlap && fom_cus != 0) {
    if ((rc = rom->ensure_fom_side(fom_cus))) return rc;
    if (rom->fom_side) fst = rom->fom_side;
  }
  // With the sweep on its masked stream and its pre-pass off it (below), the ROM half can stay on the CALLER's stream: sub-fin
  // averages, per-sample scalars, projection and the difference kernel then follow each other in stream order, and the library's
  // unmasked side stream carries the pre-pass instead -- no cross-stream wait on the step's critical path (each costs 40-80 us:
  // between two steps of the headline the GPU waited 0.33 ms).  FINROM_ROM_ON_SIDE=1: the ROM half on the side stream, as for
  // every other caller's stream.
  static const bool env_rom_on_side = getenv("FINROM_ROM_ON_SIDE") != nullptr;
  static const bool env_pre_masked = getenv("FINROM_FOM_PREPASS_MASKED") != nullptr;
  const bool pre_unmasked = fst != st && split && !env_pre_masked;
  // Only when the caller's stream is a non-blocking one: hipExtStreamCreateWithCUMask has no flags argument, the masked stream is a
  // BLOCKING stream, and the null stream (torch's default) serialises with it -- measured: the sweep then starts when the
  // projection ends (29.0 instead of 20.2 ms per step).
  unsigned st_flags = 0;
  const bool st_nonblocking = st != nullptr && hipStreamGetFlags(st, &st_flags) == hipSuccess && (st_flags & hipStreamNonBlocking);
  const bool rom_on_caller = pre_unmasked && !env_rom_on_side && st_nonblocking;
  const hipStream_t rst = rom_on_caller ? st : side;      // the ROM half
  const hipStream_t pst = rom_on_caller ? side : st;      // the FOM half's unmasked pre-pass
  auto join = [&]() {
    if (overlap && !rom_on_caller && hipEventRecord(rom->ev_join, side) == hipSuccess) (void)hipStreamWaitEvent(st, rom->ev_join, 0);
    if (fst != st && hipEventRecord(rom->ev_join_fom, fst) == hipSuccess) (void)hipStreamWaitEvent(st, rom->ev_join_fom, 0);      // (the sweep waited for the pre-pass)
  };
  auto fail = [&](int code) { if (overlap) (void)hipStreamSynchronize(side); if (fst != st) (void)hipStreamSynchronize(fst); return code; };
  if (split && (rc = fom_solve_stages(fom, x, S, qoi, w, info, st, 4))) return rc;          // (reserves the FOM workspace)
  // the sub-fin averages (bandwidth-bound, short) run BEFORE the fork, alone: beside the sweep they were starved (0.19 -> 0.39 ms
  // at the headline, 0.6 -> 5.8 ms at m = 20) and they head the ROM half's critical path
  if ((rc = launch_subfin_avg(Sop, rom->d.P, fom->d.xdim, x, S, theta, st))) return fail(rc);
  if (overlap) {                          // the ROM half starts after the averages
    FR_HIP(hipEventRecord(rom->ev_fork, st));
    FR_HIP(hipStreamWaitEvent(side, rom->ev_fork, 0));
    if (fst != st) FR_HIP(hipStreamWaitEvent(fst, rom->ev_fork, 0));
  }
  // Beside the HALF sweep (154 registers, 11.8 KB of LDS per wave) a QoI-only projection at r <= 80 takes the roomy one-wave kernel:
  // 256 + 154 registers still share a SIMD.  Whether the roomy kernel runs depends on the two handles and on what the caller wants
  // back, never on batch size, stream or mask.  FINROM_PROJ_NO_ROOMY=1 at handle creation: the 200-register kernel, as everywhere else.
  // WHICH of its two forms runs does depend on the mask: the epilogue drops the fixed waits between accumulate-chained MFMAs (same
  // bits) only beside a sweep on its masked stream, for the reason the pivot records below have: a batch too small for
  // the mask is bounded from BELOW by the benchmark's contract (0.662 ms at 4096 samples; with the short waits the step measured
  // 0.660 and 0.678 ms there, with the fixed ones 0.69).  The batches whose sweep is masked BY DEFAULT eliminate their block rows in
  // place (round 15: no U_kk^-T; qoi_r differs at rounding level) at the basis widths where that measured faster -- also where
  // FINROM_FOM_CUS, a blocking stream or the overlap switch then keep the mask away: same bits wherever the kernels run.  The same
  // batches offer the COMPACT list (round 16, DESIGN 4b'') in the short list's place, for the same reason: other bits, at rounding level.
  if ((rc = rom_solve_impl(rom, theta, S, w_r, qoi_r, nullptr, nullptr, info, rst, half_plan && !rom->no_roomy, rom->short_waits(fst != st),
                           rom->block_row(mask_by_default), rom->compact(mask_by_default))))
    return fail(rc);
  // With a masked FOM stream only the SWEEP runs on it: pack + assembly go to an unmasked stream (they take 0.1 ms there against
  // 2.0 ms on 96 CUs beside the projection's start, and since the grouped projection loop the FOM half is the one that ends
  // last: step 20.46 -> 20.26 ms).  FINROM_FOM_PREPASS_MASKED=1: the whole FOM half on the masked stream, as before.
  // Pivot records (DESIGN 4c') are for the sweep CONFINED to its masked stream: there every millisecond it lives shorter returns
  // CU-time to the projection.  A batch too small for the mask keeps the table-reading kernel on this path: its step is a chain of
  // launch latencies, which the benchmark's contract bounds from BELOW by the reference's flop count over the matrix peak
  // (tests/test_gpu_bench_contract.py: 0.662 ms at 4096 samples; on records the step is 0.62 ms, on tables 0.71).  Same bits either way.
  const bool records = fst != st;
  if (pre_unmasked) {
    if ((rc = fom_solve_stages(fom, x, S, qoi, w, info, pst, 1))) return fail(rc);
    if (hipEventRecord(rom->ev_join_fom, pst) != hipSuccess || hipStreamWaitEvent(fst, rom->ev_join_fom, 0) != hipSuccess) return fail(FINROM_ERR_HIP);
    if ((rc = fom_solve_stages(fom, x, S, qoi, w, info, fst, 2, records))) return fail(rc);
  } else if ((rc = fom_solve_stages(fom, x, S, qoi, w, info, fst, 3, records))) return fail(rc);
  join();
  // a roomy call returns a sample that either half flagged as NaN in qoi_r and err (launch_sub_flagged); every other call keeps
  // what its kernels wrote
  if ((rom->last_epilogue == FINROM_ROM_EPILOGUE_ROOMY || rom->last_epilogue == FINROM_ROM_EPILOGUE_ROOMY_SHORT_WAITS ||
       rom->last_epilogue == FINROM_ROM_EPILOGUE_ROOMY_BLOCK_ROW) && info != nullptr) {
    if ((rc = launch_sub_flagged(qoi, qoi_r, info, fom->d.n_obs, S * (int64_t)fom->d.n_obs, err, st))) return rc;
  } else if (err && (rc = launch_sub(qoi, qoi_r, S * (int64_t)fom->d.n_obs, err, st))) return rc;
  if (tracing) {
    if (fom->d.trace) trace_dump("fom", g_trace_buf[0], (size_t)((S + 63) / 64));
    if (rom->d.trace) trace_dump("proj", g_trace_buf[1], (size_t)S);
    fom->d.trace = nullptr; rom->d.trace = nullptr;
  }
  return 0;
}

}  // extern "C"
