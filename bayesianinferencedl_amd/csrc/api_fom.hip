// The full-order model behind the C ABI: every finrom_fom_* entry point, the band-plan installer (build_band), and the
// FOM half as finrom_solve_pairs runs it in stages (env_no_band, fom_chunk_samples, fom_solve_stages: api_private.h).
#include "api_private.h"

#include <algorithm>
#include <cstdlib>

using namespace finrom;

extern "C" {

// ---------------------------------------------------------------------------------------
// FOM
// ---------------------------------------------------------------------------------------
int finrom_fom_create(const finrom_fom_desc* a, finrom_fom_t* out) {
  if (!a || !out) { set_error("fom_create: null argument"); return FINROM_ERR_ARG; }
  *out = nullptr;
  const int n = a->n, nnzL = a->nnzL;
  if (n <= 0 || nnzL < n || a->xdim <= 0 || a->n_obs < 0 || a->nasm < 0 || a->n_alist < 0 || a->cache_slots < 1 ||
      a->cache_slots > 126 || (a->fwd_chunk != 8 && a->fwd_chunk != 16) || a->nops_fwd < 2 * a->fwd_chunk ||
      a->nops_bwd < 2 * VM_CHUNK || a->nops_fwd % (2 * a->fwd_chunk) || a->nops_bwd % (2 * VM_CHUNK)) {
    set_error("fom_create: inconsistent sizes"); return FINROM_ERR_ARG;
  }
  // validate every index the kernels will dereference (a bad index would fault the GPU) and
  // the prefetch rule of the op streams
  auto bad = [&](const char* what) { set_error(std::string("fom_create: invalid ") + what); return FINROM_ERR_ARG; };
  const int gsize = nnzL + 2 * n;
  if ((int64_t)(nnzL + 3 * (int64_t)n) * 512 >= (int64_t)1 << 31) { set_error("fom_create: value vector too long for 32-bit buffer offsets"); return FINROM_ERR_UNSUPPORTED; }
  for (int t = 0; t < a->n_alist; ++t) if (a->a_list[t] < 0 || a->a_list[t] >= nnzL) return bad("a_list");
  if (a->asm_ptr[0] != 0 || a->asm_ptr[nnzL] != a->nasm) return bad("asm_ptr");
  for (int e = 0; e < nnzL; ++e) if (a->asm_ptr[e + 1] < a->asm_ptr[e]) return bad("asm_ptr");
  for (int t = 0; t < a->nasm; ++t) if (a->asm_idx[t] < 0 || a->asm_idx[t] >= a->xdim) return bad("asm_idx");
  int fused = 0;
  if (a->n_imm < 0 || (a->n_imm > 0 && !a->imm)) return bad("imm");
  {
    std::vector<int> stored(gsize, -10);
    std::vector<char> slot_set(std::max(a->cache_slots, 1), 0);      // row-cache slots that have been written (FINOFF)
    auto need = [&](int g, int c) { return g >= 0 && g < gsize && stored[g] + 2 <= c; };
    for (int t = 0; t < a->nops_fwd; ++t) {
      const int k = a->fwd_kind[t], A = a->fwd_a[t], B = a->fwd_b[t], D = a->fwd_d[t], c = t / a->fwd_chunk;
      if (A < -1 || A >= gsize) return bad("forward op operand index");     // fetched for every op, used or not
      switch (k) {
        case 0: if ((A >= 0 && !need(A, c)) || A < -1 || B < 0 || B >= a->cache_slots + 2) return bad("forward FMA op"); break;
        case 3: case 4: if (!need(A, c)) return bad("forward LDX/FMAX op"); break;
        case 5: if (!need(A, c) || D < 0 || D >= nnzL || B < -1 || B >= a->cache_slots) return bad("forward FINOFF op"); stored[D] = c;
                if (B >= 0) slot_set[B] = 1;
                break;
        case 11: if (B < 0 || B >= a->cache_slots || D < 0 || D >= a->cache_slots || !slot_set[B] || !slot_set[D]) return bad("forward FMALL op"); break;
        case 6: if (D < 0 || D >= nnzL || B < 0 || B >= n) return bad("forward FINDIAG op"); stored[D] = c; stored[nnzL + B] = c; break;
        case 7: if (D < 0 || D >= n) return bad("forward YSET op"); break;
        case 9: if (a->xdim > FOM_MAX_FUSED_X || B < 0 || B >= a->xdim || D < 0 || D >= a->n_imm) return bad("forward XFMA op"); fused = 1; break;
        case 10: if (a->xdim > FOM_MAX_FUSED_X || D < 0 || D >= a->n_imm) return bad("forward CADD op"); fused = 1; break;
        case 8: if (D < nnzL + n || D >= gsize) return bad("forward FINY op"); stored[D] = c; break;
        default: return bad("forward op kind");
      }
      if (t >= a->nops_fwd - 2 * a->fwd_chunk && (k != 0 || B != a->cache_slots + 1)) return bad("forward stream tail (must be padding)");
    }
    std::fill(stored.begin(), stored.end(), -10);
    auto need1 = [&](int g, int c) { return g >= 0 && g < gsize && stored[g] + 2 <= c; };   // backward: same look-ahead as forward
    for (int t = 0; t < a->nops_bwd; ++t) {
      const int k = a->bwd_kind[t], A = a->bwd_a[t], B = a->bwd_b[t], D = a->bwd_d[t], c = t / VM_CHUNK;
      if (A < -1 || A >= gsize || B < -1 || B >= gsize) return bad("backward op operand index");
      switch (k) {
        case 0: break;
        case 1: if (!need1(A, c) || !need1(B, c)) return bad("backward WFMA op"); break;
        case 3: if (!need1(A, c)) return bad("backward WSET op"); break;
        case 5: if (!need1(A, c) || D < nnzL + n || D >= gsize) return bad("backward WFIN op"); stored[D] = c; break;
        default: return bad("backward op kind");
      }
      if (t >= a->nops_bwd - 2 * VM_CHUNK && k != 0) return bad("backward stream tail (must be NOP padding)");
    }
  }
  if (a->n_obs > 0) {
    if (a->obs_ptr[0] != 0) return bad("obs_ptr");
    for (int o = 0; o < a->n_obs; ++o) if (a->obs_ptr[o + 1] < a->obs_ptr[o]) return bad("obs_ptr");
    for (int t = 0; t < a->obs_ptr[a->n_obs]; ++t) if (a->obs_idx[t] < 0 || a->obs_idx[t] >= n) return bad("obs_idx");
  }
  {
    std::vector<char> seen(n, 0);
    for (int i = 0; i < n; ++i) { int v = a->perm[i]; if (v < 0 || v >= n || seen[v]) return bad("perm"); seen[v] = 1; }
  }

  auto* h = new finrom_fom_s();
  FomDev& d = h->d;
  d.n = n; d.nnzL = nnzL; d.xdim = a->xdim; d.n_obs = a->n_obs; d.n_alist = a->n_alist; d.cache_slots = a->cache_slots;
  d.gsize = gsize;
  d.fwd_chunk = a->fwd_chunk;
  d.nchunks_fwd = a->nops_fwd / a->fwd_chunk - 2; d.nchunks_bwd = a->nops_bwd / VM_CHUNK - 2;
  d.trace = nullptr;
  d.has_grad = 0; d.nchunks_res = 0;
  std::vector<int> fkb(a->nops_fwd), bkb(a->nops_bwd);
  // device encoding of the forward stream: load offsets in bytes, the common multiply-adds (FMA, FMALL) carry the LDS
  // byte offsets of their row-cache slots in kb and d, every other op kind | (b+1) << 8, and one bit mask per chunk flags
  // the slots that are NOT plain multiply-adds (bits 0..15) and the multiply-adds whose second operand is in LDS (bits 16..31)
  std::vector<int> fa2(a->nops_fwd), fd2(a->nops_fwd), fmask(a->nops_fwd / a->fwd_chunk, 0);
  for (int t = 0; t < a->nops_fwd; ++t) {
    // ops without a global operand (padding, fused-assembly ops) fetch from beyond the buffer's range: the hardware
    // bounds check returns 0 without touching memory (a real element could be uninitialised: 0 * NaN)
    fa2[t] = a->fwd_a[t] < 0 ? 0x7FFFFFF0 : a->fwd_a[t] * 512;
    fd2[t] = a->fwd_d[t];
    // the common multiply-add is acc -= rc[b] * (G[a] + rc[d']): FMA reads the ZERO slot as d', FMALL an out-of-range G[a]
    // the common multiply-add is acc -= rc[b] * (G[a] + rc[d']): FMA reads the ZERO slot as d', FMALL an out-of-range G[a]
    if (a->fwd_kind[t] == 0) { fkb[t] = a->fwd_b[t] * 512; fd2[t] = (a->cache_slots + 1) * 512; }
    else if (a->fwd_kind[t] == 11) { fkb[t] = a->fwd_b[t] * 512; fd2[t] = a->fwd_d[t] * 512;
                                       fmask[t / a->fwd_chunk] |= 1 << (16 + t % a->fwd_chunk); }     // second operand in LDS
    else { fkb[t] = a->fwd_kind[t] | ((a->fwd_b[t] + 1) << 8); fmask[t / a->fwd_chunk] |= 1 << (t % a->fwd_chunk); }
  }
  // backward stream on the device: byte offsets of both operands (out of range = no operand: the fetch returns 0 without
  // touching memory) and kind | d << 8
  std::vector<int> ba2(a->nops_bwd), bb2(a->nops_bwd);
  for (int t = 0; t < a->nops_bwd; ++t) {
    const int k = a->bwd_kind[t];
    ba2[t] = (k == 0 || a->bwd_a[t] < 0) ? 0x7FFFFFF0 : a->bwd_a[t] * 512;
    bb2[t] = (k != 1 || a->bwd_b[t] < 0) ? 0x7FFFFFF0 : a->bwd_b[t] * 512;
    bkb[t] = k | ((k == 5 ? a->bwd_d[t] : 0) << 8);
  }
  int rc = 0;
  const int nobsnz = a->n_obs > 0 ? a->obs_ptr[a->n_obs] : 0;
  // assembly records: {entry, idx0..3, first/last of the remaining terms, 0} and {c0, w0..3}; unused slots
  // multiply parameter 0 by a zero weight
  std::vector<int> reci((size_t)a->n_alist * 8, 0);
  std::vector<double> recd((size_t)a->n_alist * 5, 0.0);
  for (int t = 0; t < a->n_alist; ++t) {
    const int e = a->a_list[t], t0 = a->asm_ptr[e], t1 = a->asm_ptr[e + 1];
    reci[t * 8 + 0] = e; recd[t * 5 + 0] = a->asm_c0[e];
    for (int k = 0; k < 4 && t0 + k < t1; ++k) { reci[t * 8 + 1 + k] = a->asm_idx[t0 + k]; recd[t * 5 + 1 + k] = a->asm_w[t0 + k]; }
    reci[t * 8 + 5] = std::min(t0 + 4, t1); reci[t * 8 + 6] = t1;
  }
  if (!rc) rc = up(h->owned, &d.asm_rec_i, reci.data(), reci.size());
  if (!rc) rc = up(h->owned, &d.asm_rec_d, recd.data(), recd.size());
  if (!rc) rc = up(h->owned, &d.asm_idx, a->asm_idx, a->nasm);
  if (!rc) rc = up(h->owned, &d.asm_w, a->asm_w, a->nasm);
  if (!rc) rc = up(h->owned, &d.rhs, a->rhs, n);
  if (!rc) rc = up(h->owned, &d.f_a, fa2.data(), fa2.size());
  if (!rc) rc = up(h->owned, &d.f_mask, fmask.data(), fmask.size());
  d.fused = fused;
  if (fused && a->n_alist != 0) { finrom_fom_destroy(h); set_error("fom_create: a fused stream must come with n_alist = 0"); return FINROM_ERR_ARG; }
  if (!rc) rc = up(h->owned, &d.f_imm, a->imm, (size_t)a->n_imm);
  if (!rc) rc = up(h->owned, &d.f_kb, fkb.data(), fkb.size());
  if (!rc) rc = up(h->owned, &d.f_d, fd2.data(), fd2.size());
  if (!rc) rc = up(h->owned, &d.b_a, ba2.data(), ba2.size());
  if (!rc) rc = up(h->owned, &d.b_b, bb2.data(), bb2.size());
  if (!rc) rc = up(h->owned, &d.b_kd, bkb.data(), bkb.size());
  if (!rc) rc = up(h->owned, &d.obs_ptr, a->obs_ptr, a->n_obs + 1);
  if (!rc) rc = up(h->owned, &d.obs_idx, a->obs_idx, nobsnz);
  if (!rc) rc = up(h->owned, &d.obs_w, a->obs_w, nobsnz);
  if (!rc) rc = up(h->owned, &d.perm, a->perm, n);
  if (rc) { finrom_fom_destroy(h); return rc; }
  *out = h;
  return 0;
}

void finrom_fom_destroy(finrom_fom_t h) {
  if (!h) return;
  for (void* p : h->owned) dev_free(p);                 // (queued while a stream capture is open: finrom_internal.h)
  h->xT.release(); h->Gw.release(); h->gradT.release(); h->qtmp.release(); h->hgrad.release();
  delete h;
}

}  // extern "C"
namespace finrom {
// FINROM_NO_BAND (A/B: the interpreter although the mesh has a band plan): read once per process, by whichever of
// fom_solve_stages, finrom_fom_gradient and finrom_solve_pairs is called first; all three see that value
bool env_no_band() { static const bool v = getenv("FINROM_NO_BAND") != nullptr; return v; }
// equal pieces when the batch exceeds the workspace bound `limit` (a short last piece would leave the GPU mostly idle)
static int64_t fom_equal_chunk(int64_t S, int64_t limit) {
  const int64_t npieces = (S + limit - 1) / limit;
  return npieces <= 1 ? limit : ((S + npieces - 1) / npieces + 63) / 64 * 64;
}
// stages: 1 = pack + assembly, 2 = interpreter (+ unpack of w), 3 = both.  finrom_solve_pairs runs stage 1, then
// launches the ROM half, then stage 2 (only possible when the batch fits one workspace chunk).
// the bound on a call's workspace, shared by every finrom_fom_* entry point that cuts a batch into pieces: 48 GiB, or
// FINROM_FOM_WORKSPACE_BYTES=<n>, read per call, so that a test can make a small batch run in pieces
static int64_t fom_workspace_bound() {
  const char* env_ws = getenv("FINROM_FOM_WORKSPACE_BYTES");
  return env_ws != nullptr && atoll(env_ws) > 0 ? (int64_t)atoll(env_ws) : (int64_t)((size_t)48 << 30);
}
// samples per piece for a workspace of `per_sample` bytes each: whole blocks of 64 lanes, one block at least
static int64_t fom_piece_samples(size_t per_sample) {
  return std::max<int64_t>(64, fom_workspace_bound() / (int64_t)per_sample / 64 * 64);
}
int64_t fom_chunk_samples(const FomDev& d, const BandDev* band) {
  // bound the per-call workspace (L values dominate: nnzL * 8 B per sample)
  return fom_piece_samples(((size_t)(band && band->on ? band->gsize : d.gsize) + d.xdim) * sizeof(double));
}
int fom_solve_stages(finrom_fom_t h, const double* x, int64_t S, double* qoi, double* w, int32_t* info, hipStream_t st, int stages,
                     bool records) {
  const FomDev& d = h->d;
  const bool no_band = env_no_band();
  // Small batches: where the mesh has a band plan the band sweep serves them too -- ONE wave walking its 1597 pivots takes 1.7 ms
  // (QoI only) / 2.3 ms (with w) at m = 12 and 4.2 / 4.4 ms at m = 20, the level-scheduled small-batch kernel 2.7 and 17.9 ms
  // (tools/fom_small_vs_band.py) -- so the latency-oriented schedule (one workgroup per sample) is the forward path only of
  // meshes without window sizes (m >= 32); finrom_fom_gradient keeps it for small batches (its adjoint stage beats a lone wave
  // of the band adjoint kernel: 3.1 against 10 ms).
  if (h->small.small_max > 0 && S <= h->small.small_max && !(h->band.on && !no_band)) {
    int rc;
    if (!h->small.in_lds && (rc = h->Gw.reserve((size_t)S * d.gsize * sizeof(double)))) return rc;
    if (!(stages & 2)) return 0;
    h->last_path = h->small.in_lds ? FINROM_FOM_PATH_SMALL_LDS : FINROM_FOM_PATH_SMALL_GLOBAL;
    return launch_fom_small(d, h->small, x, S, (double*)h->Gw.p, qoi, w, info, st);
  }
  if (h->band.on && !no_band) {
    const BandDev& b = h->band_for(w != nullptr);        // (the half plan of a mirror-symmetric operator when nobody wants w)
    const FomDev& basm = &b == &h->band_m ? h->band_m_asm : h->band_asm;
    h->last_path = band_path(b, w == nullptr);
    const int64_t chunk = fom_equal_chunk(S, fom_chunk_samples(d, &b));
    for (int64_t s0 = 0; s0 < S; s0 += chunk) {
      const int64_t Sc = std::min(chunk, S - s0), nblk = (Sc + 63) / 64;
      int rc;
      if (stages & (1 | 4)) {                            // (4: reserve the workspace only -- finrom_solve_pairs, before its fork)
        if ((rc = h->xT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
        if ((rc = h->Gw.reserve((size_t)nblk * b.gsize * 64 * sizeof(double)))) return rc;
      }
      if (stages & 1) {
        if ((rc = launch_pack(x + s0 * d.xdim, Sc, d.xdim, (double*)h->xT.p, st))) return rc;
        if ((rc = launch_fom_assemble(basm, (const double*)h->xT.p, nblk, (double*)h->Gw.p, st))) return rc;
      }
      if (stages & 2) {
        BandFnDev fnl = h->band_m_fn;
        if (!records) fnl.fin_rec = nullptr, fnl.post_rec = nullptr;      // (the sweep reads the tables themselves)
        const BandFnDev* fn = &b == &h->band_m && fnl.cw != nullptr ? &fnl : nullptr;
        if ((rc = launch_fom_band(b, (double*)h->Gw.p, nblk, Sc, qoi ? qoi + s0 * d.n_obs : nullptr, info ? info + s0 : nullptr, st, w == nullptr, fn))) return rc;
        if (w && (rc = launch_unpack((const double*)h->Gw.p, Sc, d.n, b.gsize, b.offY, b.perm, w + s0 * d.n, st))) return rc;
      }
    }
    return 0;
  }
  h->last_path = FINROM_FOM_PATH_INTERPRETER;
  const int64_t chunk = fom_equal_chunk(S, fom_chunk_samples(d));
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t Sc = std::min(chunk, S - s0);
    const int64_t nblk = (Sc + 63) / 64;
    int rc;
    if (stages & (1 | 4)) {
      if ((rc = h->xT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
      if ((rc = h->Gw.reserve((size_t)nblk * d.gsize * 64 * sizeof(double)))) return rc;
    }
    if (stages & 1) {
      if ((rc = launch_pack(x + s0 * d.xdim, Sc, d.xdim, (double*)h->xT.p, st))) return rc;
      if (!d.fused && (rc = launch_fom_assemble(d, (const double*)h->xT.p, nblk, (double*)h->Gw.p, st))) return rc;
    }
    if (stages & 2) {
      if ((rc = launch_fom(d, (const double*)h->xT.p, nblk, Sc, (double*)h->Gw.p, qoi ? qoi + s0 * d.n_obs : nullptr, info ? info + s0 : nullptr, st))) return rc;
      if (w && (rc = launch_unpack_w(d, (const double*)h->Gw.p, Sc, w + s0 * d.n, st))) return rc;
    }
  }
  return 0;
}
}  // namespace finrom
extern "C" {

int finrom_fom_solve(finrom_fom_t h, const double* x, int64_t S, double* qoi, double* w, int32_t* info, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!x || (!qoi && h->d.n_obs > 0)))) { set_error("fom_solve: bad argument"); return FINROM_ERR_ARG; }
  return fom_solve_stages(h, x, S, qoi, w, info, (hipStream_t)stream, 3);
}

int finrom_fom_last_path(finrom_fom_t h) {
  if (!h) { set_error("fom_last_path: null handle"); return FINROM_ERR_ARG; }
  return h->last_path;
}

int finrom_fom_set_small_max(finrom_fom_t h, int32_t small_max) {
  if (!h || small_max < 0) { set_error("fom_set_small_max: bad argument"); return FINROM_ERR_ARG; }
  if (small_max > 0 && h->small.rec == nullptr) { set_error("fom_set_small_max: finrom_fom_set_small has not been called"); return FINROM_ERR_ARG; }
  h->small.small_max = small_max;
  return 0;
}

int finrom_fom_set_small(finrom_fom_t h, const finrom_fom_small_desc* a) {
  if (!h || !a || a->small_max < 0 || a->npairs < 0 || a->nasm < 0 || a->nlev_f <= 0 || a->nlev_b <= 0) { set_error("fom_set_small: bad argument"); return FINROM_ERR_ARG; }
  const FomDev& d = h->d;
  const int n = d.n, nnzL = d.nnzL;
  auto bad = [&](const char* what) { set_error(std::string("fom_set_small: invalid ") + what); return FINROM_ERR_ARG; };
  // every index the kernel dereferences, and the level property (a row only reads rows of lower levels)
  if (a->row_ptr[0] != 0 || a->row_ptr[n] != nnzL) return bad("row_ptr");
  std::vector<int> ent_row(nnzL);
  for (int i = 0; i < n; ++i) {
    if (a->row_ptr[i + 1] <= a->row_ptr[i]) return bad("row_ptr");
    for (int e = a->row_ptr[i]; e < a->row_ptr[i + 1]; ++e) {
      ent_row[e] = i;
      const int j = a->ent_col[e];
      if (j < 0 || j > i || (e == a->row_ptr[i + 1] - 1) != (j == i)) return bad("ent_col (diagonal must close its row)");
    }
  }
  if (a->pair_ptr[0] != 0 || a->pair_ptr[nnzL] != a->npairs) return bad("pair_ptr");
  if (a->asm_ptr[0] != 0 || a->asm_ptr[nnzL] != a->nasm) return bad("asm_ptr");
  for (int e = 0; e < nnzL; ++e) {
    if (a->pair_ptr[e + 1] < a->pair_ptr[e] || a->asm_ptr[e + 1] < a->asm_ptr[e]) return bad("pair_ptr / asm_ptr");
    for (int k = a->pair_ptr[e]; k < a->pair_ptr[e + 1]; ++k) {
      const int pa = a->pair_a[k], pb = a->pair_b[k];
      if (pa < a->row_ptr[ent_row[e]] || pa >= e || pb < 0 || pb >= nnzL || ent_row[pb] != a->ent_col[e]) return bad("pair");
    }
  }
  for (int t = 0; t < a->nasm; ++t) if (a->asm_idx[t] < 0 || a->asm_idx[t] >= d.xdim) return bad("asm_idx");
  if (a->col_ptr[0] != 0 || a->col_ptr[n] != nnzL - n) return bad("col_ptr");
  for (int j = 0; j < n; ++j) {
    if (a->col_ptr[j + 1] < a->col_ptr[j]) return bad("col_ptr");
    for (int c = a->col_ptr[j]; c < a->col_ptr[j + 1]; ++c) {
      const int e = a->col_ent[c];
      if (e < 0 || e >= nnzL || a->ent_col[e] != j || ent_row[e] != a->col_row[c] || a->col_row[c] <= j) return bad("column view");
    }
  }
  auto levels_ok = [&](const int* ptr, const int* rows, int nlev, bool forward) {
    if (ptr[0] != 0 || ptr[nlev] != n) return false;
    std::vector<int> lev(n, -1);
    for (int l = 0; l < nlev; ++l) {
      if (ptr[l + 1] < ptr[l]) return false;
      for (int t = ptr[l]; t < ptr[l + 1]; ++t) { const int i = rows[t]; if (i < 0 || i >= n || lev[i] >= 0) return false; lev[i] = l; }
    }
    for (int i = 0; i < n; ++i) {
      if (lev[i] < 0) return false;
      if (forward) { for (int e = a->row_ptr[i]; e < a->row_ptr[i + 1] - 1; ++e) if (lev[a->ent_col[e]] >= lev[i]) return false; }
      else { for (int c = a->col_ptr[i]; c < a->col_ptr[i + 1]; ++c) if (lev[a->col_row[c]] >= lev[i]) return false; }
    }
    return true;
  };
  if (!levels_ok(a->lev_ptr_f, a->lev_rows_f, a->nlev_f, true)) return bad("forward levels");
  if (!levels_ok(a->lev_ptr_b, a->lev_rows_b, a->nlev_b, false)) return bad("backward levels");
  FomSmallDev q;
  int rc = 0;
  // device layout for latency: a stream of fixed-size records (see FomSmallRec), (entry, row) column items as 8-B items
  std::vector<FomSmallRec> rec;
  std::vector<int> rec_ptr(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    for (int e = a->row_ptr[i]; e < a->row_ptr[i + 1]; ++e) {
      const int k0 = a->pair_ptr[e], np = a->pair_ptr[e + 1] - k0, t0 = a->asm_ptr[e], nt = a->asm_ptr[e + 1] - t0;
      const int nrec = std::max(1, std::max((np + 15) / 16, (nt + 7) / 8));
      for (int c = 0; c < nrec; ++c) {
        FomSmallRec r{};
        r.e = e; r.col = a->ent_col[e];
        r.npair = std::max(0, std::min(16, np - 16 * c));
        for (int u = 0; u < r.npair; ++u) r.first[u] = int2{a->pair_a[k0 + 16 * c + u], a->pair_b[k0 + 16 * c + u]};
        const int ntc = std::max(0, std::min(8, nt - 8 * c));
        for (int u = 0; u < ntc; ++u) { r.aidx[u] = a->asm_idx[t0 + 8 * c + u]; r.aw[u] = a->asm_w[t0 + 8 * c + u]; }
        r.c0 = c == 0 ? a->asm_c0[e] : 0.0;
        r.flags = (c == nrec - 1 ? 1 : 0) | (r.col == i ? 2 : 0) | ((ntc > 0 || r.c0 != 0.0) ? 4 : 0);
        rec.push_back(r);
      }
    }
    rec_ptr[i + 1] = (int)rec.size();
  }
  rec.resize(rec.size() + 6, FomSmallRec{});
  std::vector<int2> colv((size_t)(nnzL - n) + 8, int2{0, 0});
  for (int c = 0; c < nnzL - n; ++c) colv[c] = int2{a->col_ent[c], a->col_row[c]};
  if (!rc) rc = up(h->owned, &q.row_ptr, a->row_ptr, n + 1);
  if (!rc) rc = up(h->owned, &q.ent_col, a->ent_col, nnzL);
  if (!rc) rc = up(h->owned, &q.rec_ptr, rec_ptr.data(), rec_ptr.size());
  if (!rc) rc = up(h->owned, &q.rec, rec.data(), rec.size());
  if (!rc) rc = up(h->owned, &q.col_ptr, a->col_ptr, n + 1);
  if (!rc) rc = up(h->owned, &q.colv, colv.data(), colv.size());
  if (!rc) rc = up(h->owned, &q.lev_ptr_f, a->lev_ptr_f, a->nlev_f + 1);
  if (!rc) rc = up(h->owned, &q.lev_rows_f, a->lev_rows_f, n);
  if (!rc) rc = up(h->owned, &q.lev_ptr_b, a->lev_ptr_b, a->nlev_b + 1);
  if (!rc) rc = up(h->owned, &q.lev_rows_b, a->lev_rows_b, n);
  if (rc) return rc;
  q.small_max = a->small_max; q.nlev_f = a->nlev_f; q.nlev_b = a->nlev_b;
  q.in_lds = (size_t)(nnzL + 3 * n + d.xdim) * sizeof(double) <= (size_t)156 * 1024;      // value vector (+ adjoint region) + x
  h->small = q;
  return 0;
}

}  // extern "C"
// Device tables of a validated band descriptor for a problem of n dofs and n_obs computed observation rows (the handle's own
// sizes for finrom_fom_set_band, the half problem's for finrom_fom_set_band_mirror): the sweep's BandDev and the parameters of
// its assembly pre-pass.  The handle owns the uploads.
static int build_band(finrom_fom_t h, const finrom_fom_band_desc* a, int n, int n_obs, int64_t gsize, int64_t nL, BandDev* b_out, FomDev* asm_out) {
  struct { int n, xdim, n_obs; } d{n, h->d.xdim, n_obs};
  const int G = a->nfins * (a->npf + a->nif) + a->npost, nift = a->nif * (a->nif + 1) / 2;
  BandDev b{};
  b.n = n; b.n_obs = d.n_obs; b.xdim = d.xdim; b.gsize = (int)gsize; b.nAB = a->nAB; b.nL = (int)nL; b.nLx = a->nLx;
  b.NSF = a->NSF; b.NSP = a->NSP; b.NX = a->NX; b.nfins = a->nfins; b.npf = a->npf; b.nif = a->nif; b.npost = a->npost;
  b.post_g0 = a->nfins * (a->npf + a->nif); b.post_e0 = a->nfins * a->npf; b.post_L0 = a->nfins * a->npf * a->NSF;
  b.offL = a->nAB; b.offLx = a->nAB + (int)nL; b.offY = a->nAB + (int)nL + a->nLx; b.offX = b.offY + n;
  b.offV = b.offX + band_xsize(a->NSP);
  // records of the assembly pre-pass (fom_assemble_kernel): every value slot, so that special slots start at zero
  std::vector<int> reci((size_t)a->nAB * 8, 0);
  std::vector<double> recd((size_t)a->nAB * 5, 0.0);
  for (int e = 0; e < a->nAB; ++e) {
    const int t0 = a->ab_ptr[e], t1 = a->ab_ptr[e + 1];
    reci[e * 8 + 0] = e; recd[e * 5 + 0] = a->ab_c0[e];
    for (int k = 0; k < 4 && t0 + k < t1; ++k) { reci[e * 8 + 1 + k] = a->ab_idx[t0 + k]; recd[e * 5 + 1 + k] = a->ab_w[t0 + k]; }
    reci[e * 8 + 5] = std::min(t0 + 4, t1); reci[e * 8 + 6] = t1;
  }
  FomDev& q = *asm_out;
  q = FomDev{};
  q.xdim = d.xdim; q.gsize = (int)gsize; q.n_alist = a->nAB;
  int rc = 0;
  const int necp = a->ecp_ptr[a->npost], nobsnz = d.n_obs > 0 ? a->obs_ptr[d.n_obs] : 0;
  if (!rc) rc = up(h->owned, &q.asm_rec_i, reci.data(), reci.size());
  if (!rc) rc = up(h->owned, &q.asm_rec_d, recd.data(), recd.size());
  if (!rc) rc = up(h->owned, &q.asm_idx, a->ab_idx, a->nterms);
  if (!rc) rc = up(h->owned, &q.asm_w, a->ab_w, a->nterms);
  if (!rc) rc = up(h->owned, &b.abmap, a->abmap, (size_t)3 * G);
  if (!rc) rc = up(h->owned, &b.Fg, a->Fg, G);
  if (!rc) rc = up(h->owned, &b.act, a->act, a->npost);
  if (!rc) rc = up(h->owned, &b.lx_ptr, a->lx_ptr, a->npost + 1);
  if (!rc) rc = up(h->owned, &b.ent_extra, a->ent_extra, a->npost);
  if (!rc) rc = up(h->owned, &b.ecp_ptr, a->ecp_ptr, a->npost + 1);
  if (!rc) rc = up(h->owned, &b.ecp_slot, a->ecp_slot, necp);
  if (!rc) rc = up(h->owned, &b.ecp_off, a->ecp_off, necp);
  if (!rc) rc = up(h->owned, &b.schur_off, a->schur_off, (size_t)a->nfins * nift);
  if (!rc) rc = up(h->owned, &b.iface_elim, a->iface_elim, (size_t)a->nfins * a->nif);
  if (!rc) rc = up(h->owned, &b.perm, a->perm, n);
  if (!rc) rc = up(h->owned, &b.obs_ptr, a->obs_ptr, d.n_obs + 1);
  if (!rc) rc = up(h->owned, &b.obs_idx, a->obs_idx, nobsnz);
  if (!rc) rc = up(h->owned, &b.obs_w, a->obs_w, nobsnz);
  if (a->qoi_FgQ != nullptr) {
    const int nqz = a->qoi_obs_ptr[d.n_obs];
    if (!rc) rc = up(h->owned, &b.FgQ, a->qoi_FgQ, G);
    if (!rc) rc = up(h->owned, &b.row_fin, a->qoi_row_fin, d.n_obs);
    if (!rc) rc = up(h->owned, &b.qobs_ptr, a->qoi_obs_ptr, d.n_obs + 1);
    if (!rc) rc = up(h->owned, &b.qobs_idx, a->qoi_obs_idx, nqz);
    if (!rc) rc = up(h->owned, &b.qobs_w, a->qoi_obs_w, nqz);
    b.qo = 1;
  }
  if (rc) return rc;
  b.on = getenv("FINROM_BAND_TIMING") != nullptr ? 2 : 1;      // 2: block 0 reports its phase clocks in sample 0's QoI (diagnostic)
  *b_out = b;
  return 0;
}
extern "C" {

int finrom_fom_set_band(finrom_fom_t h, const finrom_fom_band_desc* a) {
  if (!h || !a) { set_error("fom_set_band: null argument"); return FINROM_ERR_ARG; }
  const FomDev& d = h->d;
  int64_t gsize = 0, nL = 0;
  if (int rc = validate_band(a, d.n, d.xdim, d.n_obs, &gsize, &nL)) return rc;
  BandDev b{};
  if (int rc = build_band(h, a, d.n, d.n_obs, gsize, nL, &b, &h->band_asm)) return rc;
  h->band = b;
  h->band_m = BandDev{}; h->band_m_fn = BandFnDev{};      // (a half plan belongs to the plan it was installed beside)
  return 0;
}

int finrom_fom_set_band_mirror(finrom_fom_t h, const finrom_fom_band_desc* a, int32_t n_half, int32_t n_rows, const int32_t* out_ptr,
                               const int32_t* out_col) {
  if (!h || !a) { set_error("fom_set_band_mirror: null argument"); return FINROM_ERR_ARG; }
  if (!h->band.on) { set_error("fom_set_band_mirror: finrom_fom_set_band has not been called"); return FINROM_ERR_ARG; }
  const FomDev& d = h->d;
  if (n_half <= 0 || n_half > d.n) { set_error("fom_set_band_mirror: invalid n_half"); return FINROM_ERR_ARG; }
  int64_t gsize = 0, nL = 0;
  if (int rc = validate_band_mirror(a, n_half, d.xdim, n_rows, d.n_obs, out_ptr, out_col, &gsize, &nL)) return rc;
  BandDev b{};
  FomDev q{};
  if (int rc = build_band(h, a, n_half, n_rows, gsize, nL, &b, &q)) return rc;
  int rc = up(h->owned, &b.out_ptr, out_ptr, n_rows + 1);
  if (!rc) rc = up(h->owned, &b.out_col, out_col, d.n_obs);
  if (rc) return rc;
  b.n_out = d.n_obs;
  // The post as functionals, where the descriptor fits (FINROM_FOM_POST_STORED=1: the stored-factor form, the A/B switch).  The
  // workspace of that form is the value slots and the fins' g: the plan's sizes -- chunking, the pair path's reservation, the
  // assembly pre-pass's stride -- all follow gsize.
  BandFnDev fn{};
  if (getenv("FINROM_FOM_POST_STORED") == nullptr) {
    std::vector<double> cw; std::vector<int> piv_row, piv_off;
    const int fits = derive_post_functionals(a, n_half, n_rows, cw, piv_row, piv_off);
    if (fits < 0) return fits;
    if (fits) {
      rc = up(h->owned, &fn.cw, cw.data(), cw.size());
      if (!rc) rc = up(h->owned, &fn.piv_row, piv_row.data(), piv_row.size());
      if (!rc) rc = up(h->owned, &fn.piv_off, piv_off.data(), piv_off.size());
      if (!rc && getenv("FINROM_FOM_NO_PIVOT_RECORDS") == nullptr) {      // (the A/B switch: the sweep reads the tables themselves)
        std::vector<BandFinRec> fr; std::vector<BandPostRec> qr;
        derive_pivot_records(a, cw, piv_row, piv_off, fr, qr);
        if ((rc = check_pivot_records(a, cw, piv_row, piv_off, fr.data(), qr.data()))) return rc;
        fr.resize(fr.size() + band_rec_pad(a->NSF), BandFinRec{}); qr.resize(qr.size() + band_rec_pad(a->NSP), BandPostRec{});
        rc = up(h->owned, &fn.fin_rec, fr.data(), fr.size());
        if (!rc) rc = up(h->owned, &fn.post_rec, qr.data(), qr.size());
      }
      if (rc) return rc;
      b.offL = b.offLx = b.offX = b.offV = 0;             // (regions this form does not have)
      b.offY = a->nAB;
      b.gsize = q.gsize = a->nAB + a->nfins * a->nif;
    }
  }
  h->band_m = b; h->band_m_asm = q; h->band_m_fn = fn;
  return 0;
}

int finrom_fom_band_mirror_form(finrom_fom_t h) {
  if (!h || !h->band_m.on) return 0;
  return h->band_m_fn.cw != nullptr ? 2 : 1;
}

int finrom_fom_band_mirror_records_on(finrom_fom_t h) {
  return h && h->band_m.on && h->band_m_fn.post_rec != nullptr ? 1 : 0;
}

int finrom_fom_set_band_gradient(finrom_fom_t h, const finrom_fom_band_grad_desc* a) {
  if (!h || !a || !a->bt_ptr || !a->g_ptr) { set_error("fom_set_band_gradient: null argument"); return FINROM_ERR_ARG; }
  if (!h->band.on) { set_error("fom_set_band_gradient: finrom_fom_set_band has not been called"); return FINROM_ERR_ARG; }
  const FomDev& d = h->d;
  const int n = d.n;
  auto bad = [&](const char* what) { set_error(std::string("fom_set_band_gradient: invalid ") + what); return FINROM_ERR_ARG; };
  if (a->bt_ptr[0] != 0) return bad("bt_ptr");
  for (int i = 0; i < n; ++i) if (a->bt_ptr[i + 1] < a->bt_ptr[i]) return bad("bt_ptr");
  const int nbt = a->bt_ptr[n];
  if (nbt > 0 && (!a->bt_obs || !a->bt_w)) return bad("table pointer (null)");
  for (int t = 0; t < nbt; ++t) if (a->bt_obs[t] < 0 || a->bt_obs[t] >= d.n_obs) return bad("bt_obs");
  if (a->g_ptr[0] != 0) return bad("g_ptr");
  for (int j = 0; j < d.xdim; ++j) if (a->g_ptr[j + 1] < a->g_ptr[j]) return bad("g_ptr");
  const int ng = a->g_ptr[d.xdim];
  if (ng > 0 && (!a->g_a || !a->g_b || !a->g_w)) return bad("table pointer (null)");
  for (int t = 0; t < ng; ++t) if (a->g_a[t] < 0 || a->g_a[t] >= n || a->g_b[t] < 0 || a->g_b[t] >= n) return bad("g_a / g_b");
  BandGradDev g;
  int rc = 0;
  if (!rc) rc = up(h->owned, &g.bt_ptr, a->bt_ptr, n + 1);
  if (!rc) rc = up(h->owned, &g.bt_obs, a->bt_obs, nbt);
  if (!rc) rc = up(h->owned, &g.bt_w, a->bt_w, nbt);
  if (!rc) rc = up(h->owned, &g.g_ptr, a->g_ptr, d.xdim + 1);
  if (!rc) rc = up(h->owned, &g.g_a, a->g_a, ng);
  if (!rc) rc = up(h->owned, &g.g_b, a->g_b, ng);
  if (!rc) rc = up(h->owned, &g.g_w, a->g_w, ng);
  if (rc) return rc;
  g.on = 1;
  h->band_grad = g;
  return 0;
}

int finrom_fom_solve_rhs(finrom_fom_t h, const double* x, int64_t S, const double* rhs, int32_t nrhs, double* out, int32_t* info,
                         void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || nrhs < 0 || (S > 0 && nrhs > 0 && (!x || !rhs || !out))) { set_error("fom_solve_rhs: bad argument"); return FINROM_ERR_ARG; }
  if (!h->band.on) { set_error("fom_solve_rhs: needs the band sweep (finrom_fom_set_band)"); return FINROM_ERR_UNSUPPORTED; }
  if (S == 0 || nrhs == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const FomDev& d = h->d;
  const BandDev& b = h->band;
  h->last_path = band_path(b, false);
  const int64_t dr = (int64_t)nrhs * d.n;
  const size_t per_sample = ((size_t)b.gsize + d.xdim + 2 * (size_t)dr) * sizeof(double);
  const int64_t limit = fom_piece_samples(per_sample);
  for (int64_t s0 = 0; s0 < S; s0 += limit) {
    const int64_t Sc = std::min(limit, S - s0), nblk = (Sc + 63) / 64;
    int rc;
    if ((rc = h->xT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
    if ((rc = h->Gw.reserve((size_t)nblk * b.gsize * 64 * sizeof(double)))) return rc;
    if ((rc = h->gradT.reserve((size_t)nblk * 2 * dr * 64 * sizeof(double)))) return rc;      // rhsT | outT
    if ((rc = h->qtmp.reserve((size_t)Sc * std::max(d.n_obs, 1) * sizeof(double)))) return rc;
    double* rhsT = (double*)h->gradT.p;
    double* outT = rhsT + (size_t)nblk * dr * 64;
    if ((rc = launch_pack(x + s0 * d.xdim, Sc, d.xdim, (double*)h->xT.p, st))) return rc;
    if ((rc = launch_fom_assemble(h->band_asm, (const double*)h->xT.p, nblk, (double*)h->Gw.p, st))) return rc;
    if ((rc = launch_fom_band(b, (double*)h->Gw.p, nblk, Sc, (double*)h->qtmp.p, info ? info + s0 : nullptr, st, false))) return rc;
    if ((rc = launch_pack(rhs + s0 * dr, Sc, (int)dr, rhsT, st))) return rc;
    if ((rc = launch_fom_band_resolve(b, (double*)h->Gw.p, nblk, nrhs, rhsT, outT, st))) return rc;
    if ((rc = launch_unpack(outT, Sc, (int)dr, dr, 0, nullptr, out + s0 * dr, st))) return rc;
  }
  return 0;
}

int finrom_fom_set_gradient(finrom_fom_t h, const finrom_fom_grad_desc* a) {
  if (!h || !a || a->nops_res < VM_CHUNK || a->nops_res % VM_CHUNK) { set_error("fom_set_gradient: bad argument"); return FINROM_ERR_ARG; }
  FomDev& d = h->d;
  const int n = d.n, nnzL = d.nnzL, gsize = nnzL + 3 * n;
  auto bad = [&](const char* what) { set_error(std::string("fom_set_gradient: invalid ") + what); return FINROM_ERR_ARG; };
  {
    std::vector<int> stored(gsize, -10);
    auto need1 = [&](int g, int c) { return g >= 0 && g < gsize && stored[g] + 1 <= c; };
    for (int t = 0; t < a->nops_res; ++t) {
      const int k = a->res_kind[t], A = a->res_a[t], B = a->res_b[t], D = a->res_d[t], c = t / VM_CHUNK;
      if (A < -1 || A >= gsize || B < -1 || B >= gsize) return bad("resolve op operand index");
      switch (k) {
        case 0: break;
        case 1: if (!need1(A, c) || !need1(B, c)) return bad("WFMA op"); break;
        case 3: if (!need1(A, c)) return bad("WSET op"); break;
        case 5: if (!need1(A, c) || D < nnzL + 2 * n || D >= gsize) return bad("WFIN op"); stored[D] = c; break;
        default: return bad("op kind");
      }
    }
  }
  if (a->bt_ptr[0] != 0) return bad("bt_ptr");
  for (int i = 0; i < n; ++i) if (a->bt_ptr[i + 1] < a->bt_ptr[i]) return bad("bt_ptr");
  for (int t = 0; t < a->bt_ptr[n]; ++t) if (a->bt_obs[t] < 0 || a->bt_obs[t] >= d.n_obs) return bad("bt_obs");
  if (a->g_ptr[0] != 0) return bad("g_ptr");
  for (int j = 0; j < d.xdim; ++j) if (a->g_ptr[j + 1] < a->g_ptr[j]) return bad("g_ptr");
  for (int t = 0; t < a->g_ptr[d.xdim]; ++t) if (a->g_a[t] < 0 || a->g_a[t] >= n || a->g_b[t] < 0 || a->g_b[t] >= n) return bad("g_a/g_b");
  std::vector<int> rkb(a->nops_res);
  for (int t = 0; t < a->nops_res; ++t) rkb[t] = a->res_kind[t] | ((a->res_b[t] + 1) << 8);
  int rc = 0;
  if (!rc) rc = up(h->owned, &d.r_a, a->res_a, a->nops_res);
  if (!rc) rc = up(h->owned, &d.r_kb, rkb.data(), rkb.size());
  if (!rc) rc = up(h->owned, &d.r_d, a->res_d, a->nops_res);
  if (!rc) rc = up(h->owned, &d.bt_ptr, a->bt_ptr, n + 1);
  if (!rc) rc = up(h->owned, &d.bt_obs, a->bt_obs, a->bt_ptr[n]);
  if (!rc) rc = up(h->owned, &d.bt_w, a->bt_w, a->bt_ptr[n]);
  if (!rc) rc = up(h->owned, &d.g_ptr, a->g_ptr, d.xdim + 1);
  if (!rc) rc = up(h->owned, &d.g_a, a->g_a, a->g_ptr[d.xdim]);
  if (!rc) rc = up(h->owned, &d.g_b, a->g_b, a->g_ptr[d.xdim]);
  if (!rc) rc = up(h->owned, &d.g_w, a->g_w, a->g_ptr[d.xdim]);
  if (rc) return rc;
  d.nchunks_res = a->nops_res / VM_CHUNK;
  d.has_grad = 1;
  d.gsize = gsize;                       // value vector grows by the adjoint region
  return 0;
}

int finrom_fom_gradient(finrom_fom_t h, const double* x, const double* data, int32_t data_per_sample, int64_t S,
                        double* grad, double* J, double* qoi, int32_t* info, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!x || !data || !grad || !J))) { set_error("fom_gradient: bad argument"); return FINROM_ERR_ARG; }
  if (!h->d.has_grad && !h->band_grad.on) { set_error("fom_gradient: finrom_fom_set_gradient has not been called"); return FINROM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const FomDev& d = h->d;
  const bool no_band = env_no_band();
  const bool small = h->small.small_max > 0 && S <= h->small.small_max && d.n_obs <= 64 && d.has_grad;
  if (!small && h->band.on && h->band_grad.on && !no_band) {
    // the full band sweep (the factor and w stay in the workspace), then the adjoint solve and the contraction on the same layout
    const BandDev& b = h->band;
    h->last_path = band_path(b, false);
    const size_t per_sample = ((size_t)b.gsize + 2 * d.xdim) * sizeof(double);
    const int64_t chunk = fom_equal_chunk(S, fom_piece_samples(per_sample));
    for (int64_t s0 = 0; s0 < S; s0 += chunk) {
      const int64_t Sc = std::min(chunk, S - s0), nblk = (Sc + 63) / 64;
      int rc;
      if ((rc = h->xT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
      if ((rc = h->Gw.reserve((size_t)nblk * b.gsize * 64 * sizeof(double)))) return rc;
      if ((rc = h->gradT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
      double* q = qoi ? qoi + s0 * d.n_obs : nullptr;
      if (!q) { if ((rc = h->qtmp.reserve((size_t)Sc * d.n_obs * sizeof(double)))) return rc; q = (double*)h->qtmp.p; }
      if ((rc = launch_pack(x + s0 * d.xdim, Sc, d.xdim, (double*)h->xT.p, st))) return rc;
      if ((rc = launch_fom_assemble(h->band_asm, (const double*)h->xT.p, nblk, (double*)h->Gw.p, st))) return rc;
      if ((rc = launch_fom_band(b, (double*)h->Gw.p, nblk, Sc, q, info ? info + s0 : nullptr, st, false))) return rc;
      if ((rc = launch_fom_band_adjoint(b, h->band_grad, (double*)h->Gw.p, nblk, Sc, q, data + (data_per_sample ? s0 * d.n_obs : 0),
                                        data_per_sample ? d.n_obs : 0, (double*)h->gradT.p, J + s0, st))) return rc;
      if ((rc = launch_unpack((const double*)h->gradT.p, Sc, d.xdim, d.xdim, 0, nullptr, grad + s0 * d.xdim, st))) return rc;
    }
    return 0;
  }
  if (!d.has_grad) { set_error("fom_gradient: finrom_fom_set_gradient has not been called (the band tables serve large batches only)"); return FINROM_ERR_ARG; }
  if (h->small.small_max > 0 && S <= h->small.small_max && d.n_obs <= 64) {      // small batch: value and gradient in one workgroup per sample
    int rc;
    if (!h->small.in_lds && (rc = h->Gw.reserve((size_t)S * d.gsize * sizeof(double)))) return rc;
    double* q = qoi;
    if (!q) { if ((rc = h->qtmp.reserve((size_t)S * d.n_obs * sizeof(double)))) return rc; q = (double*)h->qtmp.p; }
    FomSmallGrad g;
    g.data = data; g.data_stride = data_per_sample ? d.n_obs : 0; g.grad = grad; g.J = J;
    h->last_path = h->small.in_lds ? FINROM_FOM_PATH_SMALL_LDS : FINROM_FOM_PATH_SMALL_GLOBAL;
    return launch_fom_small(d, h->small, x, S, (double*)h->Gw.p, q, nullptr, info, st, g);
  }
  h->last_path = FINROM_FOM_PATH_INTERPRETER;
  const size_t per_sample = ((size_t)d.gsize + 2 * d.xdim) * sizeof(double);
  const int64_t chunk = fom_piece_samples(per_sample);
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t Sc = std::min(chunk, S - s0);
    const int64_t nblk = (Sc + 63) / 64;
    int rc;
    if ((rc = h->xT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
    if ((rc = h->Gw.reserve((size_t)nblk * d.gsize * 64 * sizeof(double)))) return rc;
    if ((rc = h->gradT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
    double* q = qoi ? qoi + s0 * d.n_obs : nullptr;
    if (!q) { if ((rc = h->qtmp.reserve((size_t)Sc * d.n_obs * sizeof(double)))) return rc; q = (double*)h->qtmp.p; }
    if ((rc = launch_pack(x + s0 * d.xdim, Sc, d.xdim, (double*)h->xT.p, st))) return rc;
    if (!d.fused && (rc = launch_fom_assemble(d, (const double*)h->xT.p, nblk, (double*)h->Gw.p, st))) return rc;
    if ((rc = launch_fom(d, (const double*)h->xT.p, nblk, Sc, (double*)h->Gw.p, q, info ? info + s0 : nullptr, st))) return rc;
    if ((rc = launch_fom_adjoint(d, nblk, Sc, (double*)h->Gw.p, q, data + (data_per_sample ? s0 * d.n_obs : 0),
                                 data_per_sample ? d.n_obs : 0, (double*)h->gradT.p, J + s0, st))) return rc;
    if ((rc = launch_unpack((const double*)h->gradT.p, Sc, d.xdim, d.xdim, 0, nullptr, grad + s0 * d.xdim, st))) return rc;
  }
  return 0;
}

}  // extern "C"
