// Inference behind the C ABI: the Gaussian-field sampler (with field_prior_ws), finrom_mlp_*, finrom_mlp_misfit_grad,
// romml_grad_impl + finrom_romml_grad, finrom_lbfgs_*, finrom_sub.  The HMC entry points that build on these are api_hmc.hip's.
#include "api_private.h"

#include <algorithm>

using namespace finrom;

extern "C" {

int finrom_sampler_create(const double* U, int32_t n, finrom_sampler_t* out) {
  if (!U || n <= 0 || !out) { set_error("sampler_create: bad argument"); return FINROM_ERR_ARG; }
  // the kernel only visits the K-range of an UPPER factor (scipy.linalg.cholesky's default, gaussian_field.py:30): a lower
  // factor such as np.linalg.cholesky(C) would silently give wrong fields
  for (int i = 1; i < n; ++i)
    for (int j = 0; j < i; ++j)
      if (U[(size_t)i * n + j] != 0.0) { set_error("sampler_create: U must be upper triangular (pass the transpose of a lower factor)"); return FINROM_ERR_ARG; }
  auto* h = new finrom_sampler_s();
  h->n = n;
  int rc = upload(&h->U, U, (size_t)n * n);
  if (rc) { delete h; return rc; }
  *out = h;
  return 0;
}
void finrom_sampler_destroy(finrom_sampler_t h) { if (!h) return; dev_free(h->U); h->xi.release(); h->fpart.release(); h->ftick.release(); delete h; }
int finrom_sampler_draw(finrom_sampler_t h, const double* xi, int64_t S, double* k, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!xi || !k))) { set_error("sampler_draw: bad argument"); return FINROM_ERR_ARG; }
  return launch_sampler(h->U, h->n, xi, S, k, (hipStream_t)stream);
}

int finrom_sampler_draw_seeded(finrom_sampler_t h, uint64_t seed, int64_t first_global_sample, int64_t S, double* k, double* xi_out,
                               void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || first_global_sample < 0 || (S > 0 && !k)) { set_error("sampler_draw_seeded: bad argument"); return FINROM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  // pieces of <= 32k samples bound the xi scratch (1 GiB at n = 4101) when the caller does not want xi back
  const int64_t piece = xi_out ? S : std::min<int64_t>(S, 32768);
  for (int64_t s0 = 0; s0 < S; s0 += piece) {
    const int64_t Sc = std::min(piece, S - s0);
    double* xi = xi_out ? xi_out + s0 * h->n : nullptr;
    if (!xi) { int rc = h->xi.reserve((size_t)Sc * h->n * sizeof(double)); if (rc) return rc; xi = (double*)h->xi.p; }
    int rc = launch_philox_normal(seed, first_global_sample + s0, Sc, h->n, xi, st);
    if (!rc) rc = launch_sampler(h->U, h->n, xi, Sc, k + s0 * h->n, st);
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
namespace finrom {
// the two triangular products' workspace on the handle (field_prior.hip): grown outside a capture only (Scratch::reserve refuses
// it inside one, with a message); the arrival counters are zeroed once, the kernels leave them zero
int field_prior_ws(finrom_sampler_t h, int64_t S) {
  const bool fresh = h->ftick.p == nullptr;
  if (int rc = h->ftick.reserve(field_prior_tick_bytes(h->n))) return rc;
  if (fresh) FR_HIP(hipMemset(h->ftick.p, 0, field_prior_tick_bytes(h->n)));
  return h->fpart.reserve(field_prior_part_bytes(h->n, S));
}
}  // namespace finrom
extern "C" {
int finrom_sampler_field(finrom_sampler_t h, const double* mean, const double* v, int64_t S, double* k, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!v || !k))) { set_error("sampler_field: bad argument (null handle, v or k, or S < 0)"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  if (int rc = field_prior_ws(h, S)) return rc;
  return launch_field_prior(h->U, h->n, 0, v, nullptr, 0.0, mean, k, nullptr, nullptr, S, (double*)h->fpart.p, (int*)h->ftick.p,
                            (hipStream_t)stream);
}
int finrom_sampler_pullback(finrom_sampler_t h, const double* g, int64_t S, double* out, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!g || !out))) { set_error("sampler_pullback: bad argument (null handle, g or out, or S < 0)"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  if (int rc = field_prior_ws(h, S)) return rc;
  return launch_field_prior(h->U, h->n, 1, g, nullptr, 0.0, nullptr, out, nullptr, nullptr, S, (double*)h->fpart.p, (int*)h->ftick.p,
                            (hipStream_t)stream);
}

int finrom_mlp_create(const finrom_mlp_desc* a, finrom_mlp_t* out) {
  if (!a || !out) { set_error("mlp_create: null argument"); return FINROM_ERR_ARG; }
  *out = nullptr;
  if (a->n_in <= 0 || a->n_w <= 0 || a->n_w > 64 || a->n_layers < 0 || a->n_layers > 64 || a->n_out <= 0 || a->n_out > 64 ||
      !a->W0 || !a->b0 || !a->scale || !a->shift || !a->Wh || !a->bh || (a->n_layers > 0 && (!a->W || !a->b))) {
    set_error("mlp_create: inconsistent sizes (n_w, n_out <= 64)"); return FINROM_ERR_ARG;
  }
  auto* h = new finrom_mlp_s();
  MlpDev& d = h->d;
  d.n_in = a->n_in; d.n_w = a->n_w; d.n_layers = a->n_layers; d.n_out = a->n_out;
  int rc = 0;
  const size_t nw = a->n_w, L = a->n_layers;
  if (!rc) rc = up(h->owned, &d.W0, a->W0, (size_t)a->n_in * nw);
  if (!rc) rc = up(h->owned, &d.b0, a->b0, nw);
  if (!rc) rc = up(h->owned, &d.scale, a->scale, (L + 1) * nw);
  if (!rc) rc = up(h->owned, &d.shift, a->shift, (L + 1) * nw);
  if (!rc) rc = up(h->owned, &d.W, a->W, L * nw * nw);
  if (!rc) rc = up(h->owned, &d.b, a->b, L * nw);
  if (!rc) rc = up(h->owned, &d.Wh, a->Wh, nw * a->n_out);
  if (!rc) rc = up(h->owned, &d.bh, a->bh, (size_t)a->n_out);
  if (rc) { finrom_mlp_destroy(h); return rc; }
  *out = h;
  return 0;
}
void finrom_mlp_destroy(finrom_mlp_t h) {
  if (!h) return;
  for (void* p : h->owned) dev_free(p);
  h->tape.release(); h->theta.release(); h->gth.release(); h->shift.release(); h->qtmp.release(); h->etmp.release(); h->g0.release(); h->y0p.release(); h->thp.release();
  h->sur_w.release(); h->sur_zero.release(); h->sur_bad.release(); h->hml_grad.release(); h->nuts_ws.release();
  delete h;
}
int finrom_mlp_predict(finrom_mlp_t h, const double* k, int64_t S, double* e, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!k || !e))) { set_error("mlp_predict: bad argument"); return FINROM_ERR_ARG; }
  if (int fits = mlp_forward_fits(h->d)) return fits;      // (before any device call)
  int rc = h->tape.reserve((size_t)S * (h->d.n_layers + 1) * h->d.n_w * sizeof(float));
  if (rc) return rc;
  return launch_mlp_forward(h->d, k, S, nullptr, 0, (float*)h->tape.p, e, nullptr, (hipStream_t)stream);
}
int32_t finrom_mlp_stage_reach(int32_t n_layers, int32_t n_w, int32_t n_out, int32_t* staged, int32_t* stage_floats) {
  if (n_layers < 0 || n_layers > 64 || n_w <= 0 || n_w > 64 || n_out <= 0 || n_out > 64) { set_error("mlp_stage_reach: sizes outside finrom_mlp_create's"); return FINROM_ERR_ARG; }
  if (staged) *staged = mlp_tail_staged(n_layers, n_w, n_out) ? 1 : 0;
  if (stage_floats) *stage_floats = MLP_STAGE_FLOATS;
  return mlp_stage_reach(n_layers, n_w, n_out);
}
int32_t finrom_mlp_forward_max_in(void) { return MLP_FORWARD_MAX_IN; }
int finrom_mlp_set_tile_min(finrom_mlp_t h, int64_t tile_min) {
  if (!h || tile_min < 1) { set_error("mlp_set_tile_min: null handle or tile_min < 1"); return FINROM_ERR_ARG; }
  h->tile_min = tile_min;
  return 0;
}
int finrom_mlp_last_form(finrom_mlp_t h) { return h ? h->last_form : 0; }
int finrom_mlp_misfit_grad(finrom_mlp_t h, const double* k, const double* data, int32_t data_per_sample, int64_t S, double* grad,
                           double* loss, double* out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CallGuard cg(st);
  if (!h || S < 0 || (S > 0 && !k)) { set_error("mlp_misfit_grad: bad argument (null handle or k, or S < 0)"); return FINROM_ERR_ARG; }
  if ((data == nullptr) != (loss == nullptr)) { set_error("mlp_misfit_grad: data and loss are given or left out together"); return FINROM_ERR_ARG; }
  if (grad != nullptr && data == nullptr) { set_error("mlp_misfit_grad: the gradient needs data"); return FINROM_ERR_ARG; }
  if (!grad && !loss && !out) { set_error("mlp_misfit_grad: at least one of grad, loss, out is required"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  const MlpDev& m = h->d;
  const bool tile = S >= h->tile_min;
  if (!tile) { if (int fits = mlp_forward_fits(m)) return fits; }      // (before any device call)
  const int no = m.n_out;
  const int64_t stride = data_per_sample ? no : 0;
  int rc;
  if (tile && !h->sur_ready) {
    if (call_captures() || any_capture()) {
      set_error("mlp_misfit_grad: the tile form's padded weights cannot be made while a stream capture is open: run the same call once "
                "before the capture begins");
      return FINROM_ERR_UNSUPPORTED;
    }
    if ((rc = h->sur_w.reserve(sur_pad_floats(m) * sizeof(float)))) return rc;
    if ((rc = launch_sur_pad(m, (float*)h->sur_w.p, &h->sur_pad, st))) return rc;
    FR_HIP(hipStreamSynchronize(st));                  // (a later call may come on another stream)
    h->sur_ready = true;
  }
  // the per-sample forward writes its tape whatever is asked for; the tile form only for a gradient
  if (!tile || grad) { if ((rc = h->tape.reserve((size_t)S * (m.n_layers + 1) * m.n_w * sizeof(float)))) return rc; }
  if (!out) { if ((rc = h->etmp.reserve((size_t)S * no * sizeof(double)))) return rc; out = (double*)h->etmp.p; }
  if (tile) {
    if ((rc = h->sur_bad.reserve((size_t)S * sizeof(int)))) return rc;
    if ((rc = launch_sur_tile_forward(m, h->sur_pad, k, S, data, stride, grad ? (float*)h->tape.p : nullptr, out, loss, (int*)h->sur_bad.p, st))) return rc;
    if (grad && (rc = launch_sur_tile_backward(m, h->sur_pad, S, (const float*)h->tape.p, data, stride, out, (const int*)h->sur_bad.p, grad, st))) return rc;
    h->last_form = 2;
    return 0;
  }
  if (grad) {                                          // the walk back's qoi_r operand: zeros (0 + e is exact)
    const size_t cap0 = h->sur_zero.cap;
    if ((rc = h->sur_zero.reserve((size_t)S * no * sizeof(double)))) return rc;
    if (h->sur_zero.cap != cap0) {                     // (grown: outside any capture)
      FR_HIP(hipMemsetAsync(h->sur_zero.p, 0, h->sur_zero.cap, st));
      FR_HIP(hipStreamSynchronize(st));
    }
  }
  if ((rc = launch_sur_forward(m, k, S, data, stride, (float*)h->tape.p, out, loss, st))) return rc;
  if (grad && (rc = launch_sur_backward(m, S, (const float*)h->tape.p, data, stride, (const double*)h->sur_zero.p, out, grad, st))) return rc;
  h->last_form = 1;
  return 0;
}
}  // extern "C"
namespace finrom {
int romml_grad_impl(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, const double* k, const double* data,
                    int32_t data_per_sample, int64_t S, double* grad, double* loss, double* qoi_r, double* e_nn,
                    int32_t* info, void* stream, const HmcStep* hs) {
  if (!rom || !mlp || !Sop || S < 0 || (S > 0 && (!k || !data || (!grad && !hs) || !loss))) { set_error("romml_grad: bad argument"); return FINROM_ERR_ARG; }
  const MlpDev& m = mlp->d;
  if (m.n_out != rom->d.n_obs) { set_error("romml_grad: the error model's outputs are not the ROM's observables"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int P = rom->d.P, no = m.n_out;
  int rc;
  if ((rc = mlp->tape.reserve((size_t)S * (m.n_layers + 1) * m.n_w * sizeof(float)))) return rc;
  if ((rc = mlp->theta.reserve(((size_t)S * P + (size_t)S * 16 * 16) * sizeof(double)))) return rc;      // theta | the contraction workgroups' own copies (MlpFuse)
  if ((rc = mlp->gth.reserve((size_t)S * P * sizeof(double)))) return rc;
  if ((rc = mlp->shift.reserve((size_t)S * no * sizeof(double)))) return rc;
  if (!qoi_r) { if ((rc = mlp->qtmp.reserve((size_t)S * no * sizeof(double)))) return rc; qoi_r = (double*)mlp->qtmp.p; }
  if (!e_nn) { if ((rc = mlp->etmp.reserve((size_t)S * no * sizeof(double)))) return rc; e_nn = (double*)mlp->etmp.p; }
  const int64_t stride = data_per_sample ? no : 0;
  // (the sub-fin averages theta = S k are formed inside the network's forward kernel: it reads k anyway)
  // One-sample form (the ROM's contraction + solve kernels, S <= 64): the gradient contraction leaves its partial sums to the
  // error model's backward kernel instead of fencing and drawing tickets for a last workgroup (-7 us per call); the error
  // model's forward pass is one more workgroup per sample of the ROM's contraction kernel (MlpFuse), behind the sub-fin averages.
  // (Tried and removed: under stream capture, the error model's forward kernel on a side stream beside the ROM's contraction
  // kernel -- the solve kernel is the first to need its output.  One fork / join inside a replayed graph cost ~240 us per call
  // on this runtime: 113 -> 355 us, tools/graph_call_cost.py.)
  const bool one = rom->projection == FINROM_PROJECTION_DIRECT && rom_onesample_applies(rom->d, S) && rom->g_npairs > 0;
  if (hs != nullptr && !(one && P <= 16)) {
    set_error("hmc_leapfrog: needs the one-sample form of the reduced model (<= 64 chains, direct projection, r <= 96, <= 16 averages, finrom_rom_set_gradient)");
    return FINROM_ERR_UNSUPPORTED;
  }
  MlpFuse fm;
  if (hs != nullptr) { fm.mom = hs->mom; fm.eps = hs->eps; fm.k_out = hs->k_out; fm.theta_parts = hs->theta_parts_in; }
  if (one && P <= 16) {                                // the network's forward pass and theta = S k ride in the ROM's contraction kernel
    fm.on = 1; fm.m = m; fm.k = k; fm.data = data; fm.data_stride = stride; fm.tape = (float*)mlp->tape.p; fm.e_out = e_nn;
    fm.data_shift = (double*)mlp->shift.p;
    if ((rc = mlp->y0p.reserve((size_t)S * fm.nw0 * 64 * sizeof(float)))) return rc;
    fm.y0_part = (float*)mlp->y0p.p;
    fm.Sop = Sop; fm.P = P; fm.theta_out = (double*)mlp->theta.p; fm.theta_scr = (double*)mlp->theta.p + (size_t)S * P;
  } else if (P <= 16) {
    if ((rc = launch_mlp_forward(m, k, S, data, stride, (float*)mlp->tape.p, e_nn, (double*)mlp->shift.p, st, Sop, P, (double*)mlp->theta.p))) return rc;
  } else {
    if ((rc = launch_subfin_avg(Sop, P, m.n_in, k, S, (double*)mlp->theta.p, st))) return rc;
    if ((rc = launch_mlp_forward(m, k, S, data, stride, (float*)mlp->tape.p, e_nn, (double*)mlp->shift.p, st))) return rc;
  }
  MlpBackFuse bf;
  if (fm.on) {
    if ((rc = mlp->g0.reserve((size_t)S * 64 * sizeof(float)))) return rc;
    bf.on = 1; bf.m = m; bf.tape = (const float*)mlp->tape.p; bf.data = data; bf.data_stride = stride; bf.qoi_r = qoi_r; bf.e_nn = e_nn;
    bf.g0_out = (float*)mlp->g0.p;
  }
  // info is this call's alone: stored by the one-sample solve kernel, cleared here for the other forms (whose kernels or flags in)
  if (info != nullptr && !one && (rc = launch_clear_info(info, S, st))) return rc;
  rom->defer_gsum = one; rom->last_gpart = nullptr; rom->fuse = fm.on ? &fm : nullptr; rom->back = bf.on ? &bf : nullptr;
  rom->info_store = one;
  rc = finrom_rom_grad(rom, (const double*)mlp->theta.p, (const double*)mlp->shift.p, 1, S, loss, (double*)mlp->gth.p, nullptr,
                       qoi_r, info, st);
  const double* gparts = rom->last_gpart;
  rom->defer_gsum = false; rom->last_gpart = nullptr; rom->fuse = nullptr; rom->back = nullptr; rom->info_store = false;
  if (rc) return rc;
  if (fm.on && gparts == nullptr) {                    // (the predicate above and finrom_rom_grad's own must agree)
    set_error("romml_grad: internal: the one-sample form was announced but not taken");
    return FINROM_ERR_UNSUPPORTED;
  }
  return launch_mlp_backward(m, S, (const float*)mlp->tape.p, data, stride, qoi_r, e_nn, (const double*)mlp->gth.p, Sop, P, grad, st,
                             gparts, gparts ? ROM_GRAD_SMALL_NG : 0, bf.on && gparts ? (const float*)mlp->g0.p : nullptr,
                             hs != nullptr ? &hs->tail : nullptr);
}
}  // namespace finrom
extern "C" {

int finrom_romml_grad(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, const double* k, const double* data,
                      int32_t data_per_sample, int64_t S, double* grad, double* loss, double* qoi_r, double* e_nn,
                      int32_t* info, void* stream) {
  CallGuard cg((hipStream_t)stream);
  return romml_grad_impl(rom, mlp, Sop, k, data, data_per_sample, S, grad, loss, qoi_r, e_nn, info, stream, nullptr);
}

}  // extern "C"
// multi-start L-BFGS (lbfgs_kernels.hip): every check on the host, before the stream is looked at
static int lbfgs_dev(const finrom_lbfgs_state* a, LbfgsDev* L, const char* who) {
  auto bad = [&](const std::string& what) { set_error(std::string(who) + ": " + what); return FINROM_ERR_ARG; };
  if (!a) return bad("null state");
  if (a->S < 1) return bad("S = " + std::to_string(a->S) + " (need S >= 1)");
  if (a->S > 0x7fffffff) return bad("S = " + std::to_string(a->S) + " (one workgroup per start: need S < 2^31)");
  if (a->d < 1) return bad("d = " + std::to_string(a->d) + " (need d >= 1)");
  if (a->m < 1 || a->m > LBFGS_MAX_M) return bad("m = " + std::to_string(a->m) + " (need 1 <= m <= 16)");
  if (a->maxls < 1) return bad("maxls = " + std::to_string(a->maxls) + " (need maxls >= 1)");
  if (a->G != nullptr && (a->gdim < 1 || a->gdim > LBFGS_MAX_GDIM)) return bad("gdim = " + std::to_string(a->gdim) + " (need 1 <= gdim <= 16 with G)");
  if (a->G == nullptr && a->gdim != 0) return bad("gdim = " + std::to_string(a->gdim) + " without G (need 0)");
  if (a->k1_ptr != nullptr && (!a->k1_idx || !a->k1_val)) return bad("null k1_idx or k1_val with k1_ptr");
  if (a->fhist != nullptr && a->fhist_rows < 1) return bad("fhist_rows = " + std::to_string(a->fhist_rows) + " with fhist (need >= 1)");
  const char* null_name = !a->x ? "x" : !a->f ? "f" : !a->g ? "g" : !a->xt ? "xt" : !a->work ? "work" : !a->status ? "status" :
                          !a->nit ? "nit" : !a->nfev ? "nfev" : nullptr;
  if (null_name) return bad(std::string("null ") + null_name);
  if ((int64_t)a->d > (int64_t)LBFGS_MAX_E * 256) {
    set_error(std::string(who) + ": d = " + std::to_string(a->d) + " > 4352 (the kernels hold a start's vectors in registers)");
    return FINROM_ERR_UNSUPPORTED;
  }
  L->S = a->S; L->d = a->d; L->m = a->m; L->maxls = a->maxls; L->gdim = a->G ? a->gdim : 0;
  L->ftol = a->ftol; L->gtol = a->gtol; L->gamma = a->gamma; L->maxiter = a->maxiter; L->maxfun = a->maxfun;
  L->lo = a->lo; L->hi = a->hi; L->x = a->x; L->f = a->f; L->g = a->g; L->xt = a->xt; L->work = a->work;
  L->status = a->status; L->nit = (long long*)a->nit; L->nfev = (long long*)a->nfev;
  L->fhist = a->fhist; L->fhist_rows = a->fhist ? a->fhist_rows : 0; L->G = a->G;
  L->k1_ptr = a->k1_ptr; L->k1_idx = a->k1_idx; L->k1_val = a->k1_val;
  return 0;
}
extern "C" {
int finrom_lbfgs_begin(const finrom_lbfgs_state* a, void* stream) {
  LbfgsDev L;
  if (int rc = lbfgs_dev(a, &L, "lbfgs_begin")) return rc;
  CallGuard cg((hipStream_t)stream);
  return launch_lbfgs_begin(L, (hipStream_t)stream);
}
int finrom_lbfgs_propose(const finrom_lbfgs_state* a, void* stream) {
  LbfgsDev L;
  if (int rc = lbfgs_dev(a, &L, "lbfgs_propose")) return rc;
  CallGuard cg((hipStream_t)stream);
  return launch_lbfgs_propose(L, (hipStream_t)stream);
}
int finrom_lbfgs_accept(const finrom_lbfgs_state* a, const double* f_in, const double* g_in, const int32_t* info, void* stream) {
  LbfgsDev L;
  if (int rc = lbfgs_dev(a, &L, "lbfgs_accept")) return rc;
  if (!f_in || !g_in) { set_error(std::string("lbfgs_accept: null ") + (!f_in ? "f_in" : "g_in")); return FINROM_ERR_ARG; }
  CallGuard cg((hipStream_t)stream);
  return launch_lbfgs_accept(L, f_in, g_in, info, (hipStream_t)stream);
}

int finrom_sub(const double* a, const double* b, int64_t count, double* out, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (count < 0 || (count > 0 && (!a || !b || !out))) { set_error("sub: bad argument"); return FINROM_ERR_ARG; }
  return launch_sub(a, b, count, out, (hipStream_t)stream);
}

}  // extern "C"
