// Host-only tables of the FOM's band plans: the validators of a band descriptor and of the half problem of a mirror-symmetric
// operator, and the functional form of the half plan's post.  No kernel and no HIP runtime call: everything here runs on a box
// without a GPU (tools/asan_validators.py).
#include "api_private.h"

#include <algorithm>

namespace finrom {

// Host-only check of a band descriptor against the sizes of the FOM it belongs to (every index the kernels dereference, the
// privacy of the slots the fins write to, the window / pipeline preconditions).  No device call: also exported as
// finrom_fom_band_validate so that a descriptor can be checked on a box without a GPU (tools/asan_validators.py).
int validate_band(const finrom_fom_band_desc* a, int n, int xdim, int n_obs, int64_t* gsize_out, int64_t* nL_out) {
  if (!a || n <= 0 || xdim <= 0 || n_obs < 0) { set_error("fom_set_band: null argument"); return FINROM_ERR_ARG; }
  struct { int n, xdim, n_obs; } d{n, xdim, n_obs};
  auto bad = [&](const char* what) { set_error(std::string("fom_set_band: invalid ") + what); return FINROM_ERR_ARG; };
  if (!band_supported(a->NSF, a->NSP, a->NX)) { set_error("fom_set_band: window sizes not built into the library"); return FINROM_ERR_UNSUPPORTED; }
  if (a->nfins < 0 || a->npf < 0 || a->nif != a->NSF - 1 || a->npost <= 0 || a->nAB <= 0 || a->nterms < 0 || a->nLx < 0) return bad("sizes");
  // the sweeps' prologue fills a whole window of NS nodes and their software pipelines request the entering node NS positions
  // ahead of the pivot: a segment with fewer pivots than window slots is not a shape the kernels were written for
  if (a->nfins > 0 && a->npf < a->NSF) return bad("npf (a fin needs at least NSF pivots)");
  if (a->npost < a->NSP) return bad("npost (the post needs at least NSP pivots)");
  const int G = a->nfins * (a->npf + a->nif) + a->npost;
  if ((int64_t)a->nfins * a->npf + a->npost != n) return bad("pivot count (must equal the number of dofs)");
  // every table is dereferenced below and by the kernels: a missing pointer is a descriptor error, not a host fault
  if (!a->abmap || !a->ab_c0 || !a->ab_ptr || !a->Fg || !a->act || !a->lx_ptr || !a->ent_extra || !a->ecp_ptr || !a->perm ||
      (a->nterms > 0 && (!a->ab_idx || !a->ab_w)) || (a->nfins > 0 && (!a->schur_off || !a->iface_elim)) ||
      (d.n_obs > 0 && !a->obs_ptr)) return bad("table pointer (null)");
  for (int e = 0; e < 3 * G; ++e) if (a->abmap[e] < 0 || a->abmap[e] >= a->nAB) return bad("abmap");
  const int64_t nL = (int64_t)a->nfins * a->npf * a->NSF + (int64_t)a->npost * a->NSP;
  const int64_t gsize = (int64_t)a->nAB + nL + a->nLx + n + band_xsize(a->NSP) + n;      // ... | y -> w | extras (LDS variant) | adjoint
  if (gsize * 512 >= (int64_t)1 << 31) { set_error("fom_set_band: workspace too long for 32-bit buffer offsets"); return FINROM_ERR_UNSUPPORTED; }
  if (a->ab_ptr[0] != 0 || a->ab_ptr[a->nAB] != a->nterms) return bad("ab_ptr");
  for (int e = 0; e < a->nAB; ++e) if (a->ab_ptr[e + 1] < a->ab_ptr[e]) return bad("ab_ptr");
  for (int t = 0; t < a->nterms; ++t) if (a->ab_idx[t] < 0 || a->ab_idx[t] >= d.xdim) return bad("ab_idx");
  if (a->lx_ptr[0] != 0 || a->lx_ptr[a->npost] != a->nLx || a->ecp_ptr[0] != 0) return bad("lx_ptr / ecp_ptr");
  for (int p = 0; p < a->npost; ++p) {
    if (a->act[p] < 0 || a->act[p] >= (1 << a->NX)) return bad("act");
    if (a->lx_ptr[p + 1] - a->lx_ptr[p] != __builtin_popcount((unsigned)a->act[p])) return bad("lx_ptr (must count the bits of act)");
    if (a->ent_extra[p] < 0 || a->ent_extra[p] > a->NX) return bad("ent_extra");
    if (a->ecp_ptr[p + 1] < a->ecp_ptr[p]) return bad("ecp_ptr");
  }
  const int necp_ = a->ecp_ptr[a->npost];
  if (necp_ > 0 && (!a->ecp_slot || !a->ecp_off)) return bad("table pointer (null)");
  for (int c = 0; c < necp_; ++c)
    if (a->ecp_slot[c] < 0 || a->ecp_slot[c] >= a->NX || a->ecp_off[c] < 0 || a->ecp_off[c] >= a->nAB) return bad("ecp_slot / ecp_off");
  const int nift = a->nif * (a->nif + 1) / 2;
  for (int t = 0; t < a->nfins * nift; ++t) if (a->schur_off[t] < 0 || a->schur_off[t] >= a->nAB) return bad("schur_off");
  // (interface nodes are POST nodes: the fins' backward sweeps read their w after the post's has written it)
  for (int t = 0; t < a->nfins * a->nif; ++t) if (a->iface_elim[t] < a->nfins * a->npf || a->iface_elim[t] >= n) return bad("iface_elim");
  {
    // The fins of a workgroup are swept by DIFFERENT waves (fom_band_ldsw_kernel), each adding its Schur complement to the post's
    // value slots with a plain load-add-store: a slot written by two fins would race.  Slots are private per fin, distinct
    // within a fin, and not shared with plain (read-only, de-duplicated) value slots of segment nodes other than the post's
    // own interface entries -- i.e. a Schur / extra-coupling slot appears in abmap at most once.
    std::vector<int> owner(a->nAB, -1);                 // fin that writes the slot
    for (int f = 0; f < a->nfins; ++f)
      for (int t = 0; t < nift; ++t) {
        const int off = a->schur_off[f * nift + t];
        if (owner[off] >= 0) return bad(owner[off] == f ? "schur_off (slot repeated within a fin)" : "schur_off (slot shared by two fins)");
        owner[off] = f;
      }
    std::vector<int> uses(a->nAB, 0);
    for (int e = 0; e < 3 * G; ++e) if (a->abmap[e] >= 0 && a->abmap[e] < a->nAB) ++uses[a->abmap[e]];
    for (int c = 0; c < necp_; ++c) ++uses[a->ecp_off[c]];
    for (int e = 0; e < a->nAB; ++e) if (owner[e] >= 0 && uses[e] > 1) return bad("schur_off (a slot the fins write to is read by more than one entry)");
  }
  {
    std::vector<char> seen(n, 0);
    for (int i = 0; i < n; ++i) { int v = a->perm[i]; if (v < 0 || v >= n || seen[v]) return bad("perm"); seen[v] = 1; }
  }
  if (d.n_obs > 0) {
    if (a->obs_ptr[0] != 0) return bad("obs_ptr");
    for (int o = 0; o < d.n_obs; ++o) if (a->obs_ptr[o + 1] < a->obs_ptr[o]) return bad("obs_ptr");
    if (a->obs_ptr[d.n_obs] > 0 && (!a->obs_idx || !a->obs_w)) return bad("table pointer (null)");
    for (int t = 0; t < a->obs_ptr[d.n_obs]; ++t) if (a->obs_idx[t] < 0 || a->obs_idx[t] >= n) return bad("obs_idx");
  }
  // the fins' sweeps do not carry a load on their own nodes over to the interface nodes' right-hand sides
  for (int f = 0; f < a->nfins; ++f)
    for (int t = 0; t < a->npf + a->nif; ++t)
      if (a->Fg[f * (a->npf + a->nif) + t] != 0.0) { set_error("fom_set_band: load on a fin's segment nodes is not supported by the sweep"); return FINROM_ERR_UNSUPPORTED; }
  // QoI-only tables: the same operator as obs_*, entry by entry
  const int nq = (a->qoi_FgQ != nullptr) + (a->qoi_row_fin != nullptr) + (a->qoi_obs_ptr != nullptr);
  if (nq != 0) {
    if (nq != 3 || d.n_obs <= 0) return bad("QoI-only tables (all or none)");
    const int post_e0 = a->nfins * a->npf, post_g0 = a->nfins * (a->npf + a->nif), ntot = a->npf + a->nif;
    if (a->qoi_obs_ptr[0] != 0) return bad("qoi_obs_ptr");
    for (int o = 0; o < d.n_obs; ++o) if (a->qoi_obs_ptr[o + 1] < a->qoi_obs_ptr[o]) return bad("qoi_obs_ptr");
    const int nqz = a->qoi_obs_ptr[d.n_obs];
    if (nqz > 0 && (!a->qoi_obs_idx || !a->qoi_obs_w)) return bad("table pointer (null)");
    for (int t = 0; t < nqz; ++t) if (a->qoi_obs_idx[t] < post_e0 || a->qoi_obs_idx[t] >= n) return bad("qoi_obs_idx (post nodes only)");
    std::vector<int> fin_row(std::max(a->nfins, 1), -1);
    for (int o = 0; o < d.n_obs; ++o) {
      const int f = a->qoi_row_fin[o];
      if (f < -1 || f >= a->nfins) return bad("qoi_row_fin");
      if (f >= 0) { if (fin_row[f] >= 0) return bad("qoi_row_fin (a fin belongs to at most one row)"); fin_row[f] = o; }
    }
    for (int g = 0; g < a->npost; ++g) if (a->qoi_FgQ[post_g0 + g] != a->Fg[post_g0 + g]) return bad("qoi_FgQ (must equal Fg on the post)");
    for (int f = 0; f < a->nfins; ++f)
      if (fin_row[f] < 0)
        for (int t = 0; t < ntot; ++t) if (a->qoi_FgQ[f * ntot + t] != 0.0) return bad("qoi_FgQ (weights on a fin no row owns)");
    std::vector<double> full(n), rec(n);
    for (int o = 0; o < d.n_obs; ++o) {
      std::fill(full.begin(), full.end(), 0.0); std::fill(rec.begin(), rec.end(), 0.0);
      for (int t = a->obs_ptr[o]; t < a->obs_ptr[o + 1]; ++t) full[a->obs_idx[t]] += a->obs_w[t];
      for (int t = a->qoi_obs_ptr[o]; t < a->qoi_obs_ptr[o + 1]; ++t) rec[a->qoi_obs_idx[t]] += a->qoi_obs_w[t];
      const int f = a->qoi_row_fin[o];
      if (f >= 0) {
        for (int t = 0; t < a->npf; ++t) rec[f * a->npf + t] += a->qoi_FgQ[f * ntot + t];
        for (int t = 0; t < a->nif; ++t) rec[a->iface_elim[f * a->nif + t]] += a->qoi_FgQ[f * ntot + a->npf + t];
      }
      for (int i = 0; i < n; ++i) if (full[i] != rec[i]) return bad("QoI-only tables (not the operator obs_* describes)");
    }
  }
  if (gsize_out) *gsize_out = gsize;
  if (nL_out) *nL_out = nL;
  return 0;
}

// Host-only check of the half problem of a mirror-symmetric operator: the half descriptor like any band descriptor (for n_half dofs
// and n_rows computed observation rows), register windows only, QoI-only tables present (the half plan serves calls without w),
// and the map from computed rows to output columns: in range, every one of the n_obs output columns written exactly once.
int validate_band_mirror(const finrom_fom_band_desc* a, int n_half, int xdim, int n_rows, int n_obs, const int32_t* out_ptr,
                         const int32_t* out_col, int64_t* gsize_out, int64_t* nL_out) {
  if (!a || !out_ptr || !out_col || n_rows <= 0 || n_obs <= 0) { set_error("fom_set_band_mirror: null argument"); return FINROM_ERR_ARG; }
  if (int rc = validate_band(a, n_half, xdim, n_rows, gsize_out, nL_out)) return rc;
  auto bad = [&](const char* what) { set_error(std::string("fom_set_band_mirror: invalid ") + what); return FINROM_ERR_ARG; };
  if (a->NSP > 14) { set_error("fom_set_band_mirror: only the register sweep takes a half plan"); return FINROM_ERR_UNSUPPORTED; }
  if (!a->qoi_FgQ) return bad("descriptor (the half plan needs the QoI-only tables)");
  if (out_ptr[0] != 0) return bad("out_ptr");
  for (int o = 0; o < n_rows; ++o) if (out_ptr[o + 1] < out_ptr[o]) return bad("out_ptr");
  if (out_ptr[n_rows] != n_obs) return bad("out_ptr (must end at the number of output columns)");
  std::vector<char> written(n_obs, 0);
  for (int c = 0; c < n_obs; ++c) {
    const int col = out_col[c];
    if (col < 0 || col >= n_obs) return bad("out_col (out of range)");
    if (written[col]) return bad("out_col (an output column is written twice, another one not at all)");
    written[col] = 1;
  }
  return 0;
}

// The post as functionals (fom_band.hip, DESIGN 4c'): the tables of a VALIDATED half descriptor, host only.
//   cw [npost][BAND_NF]   row o's post-only weights (qoi_obs_*), dense; rows beyond n_rows are zero
//   piv_row, piv_off [npost]   post pivot -> the row that owns the fin this pivot is an interface node of (-1: none) and the slot
//                              f * nif + t in which that fin's sweep leaves its g for the node
// -> 1: the form fits; 0: it does not -- more than BAND_NF rows, other window sizes than the half plans', a row with weights on two
// fins, a post node that is an interface node of two fins that rows own -- and the stored-factor form serves the plan;
// < 0: the derived tables do not describe the operator obs_* describes (an error, like any other validator finding).
int derive_post_functionals(const finrom_fom_band_desc* a, int n_half, int n_rows, std::vector<double>& cw, std::vector<int>& piv_row,
                            std::vector<int>& piv_off) {
  auto bad = [&](const char* what) { set_error(std::string("fom_set_band_mirror: invalid ") + what); return (int)FINROM_ERR_ARG; };
  const bool windows = a->NX <= 2 && ((a->NSF == 3 && a->NSP == 4) || (a->NSF == 4 && a->NSP == 6) || (a->NSF == 5 && a->NSP == 8));
  if (!windows || n_rows > BAND_NF || !a->qoi_FgQ) return 0;
  const int post_e0 = a->nfins * a->npf, ntot = a->npf + a->nif;
  for (int o = 0; o < n_rows; ++o)                        // a row's weights on fin nodes: one fin, the one row_fin names
    for (int t = a->obs_ptr[o]; t < a->obs_ptr[o + 1]; ++t)
      if (a->obs_idx[t] < post_e0 && a->obs_w[t] != 0.0 && a->obs_idx[t] / a->npf != a->qoi_row_fin[o]) return 0;
  cw.assign((size_t)a->npost * BAND_NF, 0.0);
  piv_row.assign(a->npost, -1); piv_off.assign(a->npost, 0);
  for (int o = 0; o < n_rows; ++o)
    for (int t = a->qoi_obs_ptr[o]; t < a->qoi_obs_ptr[o + 1]; ++t) {
      const int pv = a->qoi_obs_idx[t] - post_e0;
      if (pv < 0 || pv >= a->npost) return bad("qoi_obs_idx (a weight outside the post)");
      cw[(size_t)pv * BAND_NF + o] += a->qoi_obs_w[t];
    }
  for (int o = 0; o < n_rows; ++o) {
    const int f = a->qoi_row_fin[o];
    if (f < 0) continue;
    for (int t = 0; t < a->nif; ++t) {
      const int pv = a->iface_elim[f * a->nif + t] - post_e0;
      if (pv < 0 || pv >= a->npost) return bad("iface_elim (an interface node outside the post)");
      if (piv_row[pv] >= 0) return 0;
      piv_row[pv] = o; piv_off[pv] = f * a->nif + t;
    }
  }
  // every index the kernel dereferences, and the operator rebuilt from the tables against obs_*, entry by entry
  for (int pv = 0; pv < a->npost; ++pv)
    if (piv_row[pv] < -1 || piv_row[pv] >= n_rows || piv_off[pv] < 0 || piv_off[pv] >= a->nfins * a->nif) return bad("derived pivot map");
  std::vector<double> full(n_half), rec(n_half);
  for (int o = 0; o < n_rows; ++o) {
    std::fill(full.begin(), full.end(), 0.0); std::fill(rec.begin(), rec.end(), 0.0);
    for (int t = a->obs_ptr[o]; t < a->obs_ptr[o + 1]; ++t) full[a->obs_idx[t]] += a->obs_w[t];
    for (int pv = 0; pv < a->npost; ++pv) {
      rec[post_e0 + pv] += cw[(size_t)pv * BAND_NF + o];
      if (piv_row[pv] == o) {                             // the g slot holds, before the fin's elimination, the row's weight on the node
        const int f = piv_off[pv] / a->nif, t = piv_off[pv] % a->nif;
        rec[post_e0 + pv] += a->qoi_FgQ[f * ntot + a->npf + t];
      }
    }
    const int f = a->qoi_row_fin[o];
    if (f >= 0) for (int t = 0; t < a->npf; ++t) rec[f * a->npf + t] += a->qoi_FgQ[f * ntot + t];
    for (int i = 0; i < n_half; ++i) if (full[i] != rec[i]) return bad("derived functional tables (not the operator obs_* describes)");
  }
  return 1;
}

// The pivot records of the functional form (finrom.h; fom_band.hip, band_sweep_rec) from a VALIDATED half descriptor and the
// tables derive_post_functionals made of it.  Without the pad records (band_rec_pad) the kernel's arrays end in.
void derive_pivot_records(const finrom_fom_band_desc* a, const std::vector<double>& cw, const std::vector<int>& piv_row,
                          const std::vector<int>& piv_off, std::vector<BandFinRec>& fin_rec, std::vector<BandPostRec>& post_rec) {
  const int ntot = a->npf + a->nif, gfin = a->nfins * ntot;
  fin_rec.assign(gfin, BandFinRec{});
  for (int g = 0; g < gfin; ++g) {
    for (int e = 0; e < 3; ++e) fin_rec[g].off[e] = a->abmap[3 * g + e] << 9;
    fin_rec[g].fg = a->qoi_FgQ[g];
  }
  post_rec.assign(a->npost + a->NSP, BandPostRec{});
  for (int t = 0; t < a->npost + a->NSP; ++t) {
    BandPostRec& r = post_rec[t];
    if (t >= a->NSP) r.act = a->act[t - a->NSP];
    if (t >= a->npost) continue;
    for (int e = 0; e < 3; ++e) r.off[e] = a->abmap[3 * (gfin + t) + e] << 9;
    r.row = piv_row[t];
    r.gv = r.row >= 0 ? (a->nAB + piv_off[t]) << 9 : r.off[0];      // (no interface node: any slot will do, the sweep discards it)
    r.ex = a->ent_extra[t]; r.c0 = a->ecp_ptr[t]; r.c1 = a->ecp_ptr[t + 1];
    r.fg = a->qoi_FgQ[gfin + t];
    for (int o = 0; o < BAND_NF; ++o) r.cw[o] = cw[(size_t)t * BAND_NF + o];
  }
}

// The nine source tables rebuilt from the records, entry by entry; every offset the kernel loads from inside the workspace of
// the functional form (nAB value slots + nfins x nif slots of the fins' g).
int check_pivot_records(const finrom_fom_band_desc* a, const std::vector<double>& cw, const std::vector<int>& piv_row,
                        const std::vector<int>& piv_off, const BandFinRec* fin_rec, const BandPostRec* post_rec) {
  auto bad = [&](const char* what) { set_error(std::string("fom_set_band_mirror: invalid pivot record (") + what + ")"); return (int)FINROM_ERR_ARG; };
  const int ntot = a->npf + a->nif, gfin = a->nfins * ntot;
  const int64_t wbytes = ((int64_t)a->nAB + a->nfins * a->nif) << 9;
  for (int g = 0; g < gfin; ++g) {
    for (int e = 0; e < 3; ++e) if (fin_rec[g].off[e] != a->abmap[3 * g + e] << 9) return bad("abmap of a fin node");
    if (fin_rec[g].fg != a->qoi_FgQ[g]) return bad("FgQ of a fin node");
  }
  for (int t = 0; t < a->npost + a->NSP; ++t) {
    const BandPostRec& r = post_rec[t];
    if (r.act != (t >= a->NSP ? a->act[t - a->NSP] : 0)) return bad("act");
    if (t >= a->npost) {
      if (r.off[0] | r.off[1] | r.off[2] | r.gv | r.ex | r.c0 | r.c1 | r.row) return bad("tail record");
      continue;
    }
    for (int e = 0; e < 3; ++e) if (r.off[e] != a->abmap[3 * (gfin + t) + e] << 9) return bad("abmap");
    if (r.fg != a->qoi_FgQ[gfin + t]) return bad("FgQ");
    if (r.ex != a->ent_extra[t]) return bad("ent_extra");
    if (r.c0 != a->ecp_ptr[t] || r.c1 != a->ecp_ptr[t + 1]) return bad("ecp_ptr");
    if (r.row != piv_row[t]) return bad("piv_row");
    if (r.row >= 0 ? r.gv != (a->nAB + piv_off[t]) << 9 : (r.gv < 0 || (r.gv & 511) != 0 || r.gv >= wbytes)) return bad("piv_off");
    for (int o = 0; o < BAND_NF; ++o) if (r.cw[o] != cw[(size_t)t * BAND_NF + o]) return bad("cw");
  }
  return 0;
}

}  // namespace finrom

using namespace finrom;

extern "C" {

int finrom_fom_band_validate(const finrom_fom_band_desc* a, int32_t n, int32_t xdim, int32_t n_obs) {
  return validate_band(a, n, xdim, n_obs, nullptr, nullptr);
}

int finrom_fom_band_mirror_validate(const finrom_fom_band_desc* a, int32_t n_half, int32_t xdim, int32_t n_rows, int32_t n_obs,
                                    const int32_t* out_ptr, const int32_t* out_col) {
  if (int rc = validate_band_mirror(a, n_half, xdim, n_rows, n_obs, out_ptr, out_col, nullptr, nullptr)) return rc;
  std::vector<double> cw; std::vector<int> piv_row, piv_off;
  const int fits = derive_post_functionals(a, n_half, n_rows, cw, piv_row, piv_off);
  return fits < 0 ? fits : 0;
}

// Host only: the tables finrom_fom_set_band_mirror derives for the functional form of the post, for a test to walk.  *fits = 0: the
// descriptor keeps the stored-factor form and nothing is written; cw [npost * 5], piv_row and piv_off [npost] otherwise.
int finrom_fom_band_mirror_functionals(const finrom_fom_band_desc* a, int32_t n_half, int32_t xdim, int32_t n_rows, int32_t n_obs,
                                       const int32_t* out_ptr, const int32_t* out_col, int32_t* fits, double* cw, int32_t* piv_row,
                                       int32_t* piv_off) {
  if (!fits || !cw || !piv_row || !piv_off) { set_error("fom_band_mirror_functionals: null argument"); return FINROM_ERR_ARG; }
  if (int rc = validate_band_mirror(a, n_half, xdim, n_rows, n_obs, out_ptr, out_col, nullptr, nullptr)) return rc;
  std::vector<double> c; std::vector<int> pr, po;
  const int f = derive_post_functionals(a, n_half, n_rows, c, pr, po);
  if (f < 0) return f;
  *fits = f;
  if (f) { std::copy(c.begin(), c.end(), cw); std::copy(pr.begin(), pr.end(), piv_row); std::copy(po.begin(), po.end(), piv_off); }
  return 0;
}

// Host only: the pivot records finrom_fom_set_band_mirror installs with the functional form, for a test to walk.
int finrom_fom_band_mirror_records(const finrom_fom_band_desc* a, int32_t n_half, int32_t xdim, int32_t n_rows, int32_t n_obs,
                                   const int32_t* out_ptr, const int32_t* out_col, int32_t* fits, finrom_fom_band_fin_rec* fin_rec,
                                   finrom_fom_band_post_rec* post_rec) {
  if (!fits || !fin_rec || !post_rec) { set_error("fom_band_mirror_records: null argument"); return FINROM_ERR_ARG; }
  if (int rc = validate_band_mirror(a, n_half, xdim, n_rows, n_obs, out_ptr, out_col, nullptr, nullptr)) return rc;
  std::vector<double> c; std::vector<int> pr, po;
  const int f = derive_post_functionals(a, n_half, n_rows, c, pr, po);
  if (f < 0) return f;
  *fits = f;
  if (!f) return 0;
  std::vector<BandFinRec> fr; std::vector<BandPostRec> qr;
  derive_pivot_records(a, c, pr, po, fr, qr);
  if (int rc = check_pivot_records(a, c, pr, po, fr.data(), qr.data())) return rc;
  std::copy(fr.begin(), fr.end(), fin_rec); std::copy(qr.begin(), qr.end(), post_rec);
  return 0;
}

int finrom_fom_band_records_check(const finrom_fom_band_desc* a, int32_t n_half, int32_t xdim, int32_t n_rows, int32_t n_obs,
                                  const int32_t* out_ptr, const int32_t* out_col, const finrom_fom_band_fin_rec* fin_rec,
                                  const finrom_fom_band_post_rec* post_rec) {
  if (!fin_rec || !post_rec) { set_error("fom_band_records_check: null argument"); return FINROM_ERR_ARG; }
  if (int rc = validate_band_mirror(a, n_half, xdim, n_rows, n_obs, out_ptr, out_col, nullptr, nullptr)) return rc;
  std::vector<double> c; std::vector<int> pr, po;
  const int f = derive_post_functionals(a, n_half, n_rows, c, pr, po);
  if (f < 0) return f;
  if (!f) { set_error("fom_band_records_check: the descriptor does not fit the functional form"); return FINROM_ERR_ARG; }
  return check_pivot_records(a, c, pr, po, fin_rec, post_rec);
}

}  // extern "C"
