// The device-resident HMC chains behind the C ABI: every finrom_hmc_* entry point (begin / end / draw / both stages /
// stats / the leapfrog step in all model forms / the trajectory) and finrom_metric_*.  From api_infer.hip it calls field_prior_ws
// and romml_grad_impl (api_private.h).
#include "api_private.h"

#include <cmath>

using namespace finrom;

static int hmc_dev(const finrom_hmc_state* a, HmcDev* h, const char* who) {
  if (!a || a->C < 0 || a->n <= 0 || !a->mean || !a->K || !a->U || !a->dU || !a->Kq[0] || !a->Kq[1] || !a->P || !a->dUq || !a->H0 ||
      !a->P_block || !a->lu_block || !a->jt || !a->pt || !a->accept || !a->loss || !a->info) {
    set_error(std::string(who) + ": null field in finrom_hmc_state"); return FINROM_ERR_ARG;
  }
  h->C = a->C; h->n = a->n; h->eps = a->eps; h->c_lik = a->c_lik; h->c_pri = a->c_pri;
  h->mean = a->mean; h->K = a->K; h->U = a->U; h->dU = a->dU; h->Kq0 = a->Kq[0]; h->P = a->P; h->dUq = a->dUq; h->H0 = a->H0;
  h->P_block = a->P_block; h->lu_block = a->lu_block; h->jt = (long long*)a->jt; h->pt = (long long*)a->pt;
  h->accept = (long long*)a->accept; h->trace = a->trace; h->loss = a->loss; h->info = a->info;
  return 0;
}
extern "C" {
int finrom_hmc_begin(const finrom_hmc_state* a, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_begin")) return rc;
  return launch_hmc_begin(h, (hipStream_t)stream);
}
int finrom_hmc_end(const finrom_hmc_state* a, int32_t n_steps, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_end")) return rc;
  if (n_steps < 0) { set_error("hmc_end: n_steps < 0"); return FINROM_ERR_ARG; }
  return launch_hmc_end(h, a->Kq[n_steps & 1], (hipStream_t)stream);       // (the position ping-pongs once per step)
}
int finrom_hmc_draw(const uint64_t* seeds, int64_t C, int32_t n, int64_t first_proposal, int64_t B, double* P_block, double* lu_block,
                    void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (C < 0) { set_error("hmc_draw: C < 0"); return FINROM_ERR_ARG; }
  if (B < 0) { set_error("hmc_draw: B < 0"); return FINROM_ERR_ARG; }
  if (first_proposal < 0) { set_error("hmc_draw: first_proposal < 0"); return FINROM_ERR_ARG; }
  if (n < 1) { set_error("hmc_draw: n < 1"); return FINROM_ERR_ARG; }
  if (B == 0 || C == 0) return 0;
  if (!seeds || !P_block || !lu_block) { set_error("hmc_draw: null seeds, P_block or lu_block"); return FINROM_ERR_ARG; }
  if (B > INT64_MAX / C || B * C > INT64_MAX / 8 / n || first_proposal > INT64_MAX - B) {
    set_error("hmc_draw: B x C x n or first_proposal + B does not fit 64 bits"); return FINROM_ERR_ARG;
  }
  return launch_hmc_draw((const unsigned long long*)seeds, C, n, first_proposal, B, P_block, lu_block, (hipStream_t)stream);
}
int finrom_hmc_end_stage1(const finrom_hmc_state* a, int32_t n_steps, int32_t* ok1, double* Uq, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_end_stage1")) return rc;
  if (n_steps < 0) { set_error("hmc_end_stage1: n_steps < 0"); return FINROM_ERR_ARG; }
  if (h.C == 0) return 0;
  if (!ok1 || !Uq) { set_error("hmc_end_stage1: null ok1 or Uq"); return FINROM_ERR_ARG; }
  return launch_hmc_end_stage1(h, a->Kq[n_steps & 1], ok1, Uq, (hipStream_t)stream);
}
int finrom_hmc_end_stage2(const finrom_hmc_state* a, int32_t n_steps, const finrom_hmc_da* da, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_end_stage2")) return rc;
  if (n_steps < 0) { set_error("hmc_end_stage2: n_steps < 0"); return FINROM_ERR_ARG; }
  if (!da) { set_error("hmc_end_stage2: null descriptor"); return FINROM_ERR_ARG; }
  if (da->n_obs < 1) { set_error("hmc_end_stage2: n_obs < 1"); return FINROM_ERR_ARG; }
  if (h.C == 0) return 0;
  if (!da->ok1 || !da->Uq || !da->qoi_f || !da->info_f || !da->data || !da->lu2_block || !da->D || !da->loss_f || !da->accept1 ||
      !da->cand_loss_f) {
    set_error("hmc_end_stage2: null pointer in finrom_hmc_da (only correction may be NULL)"); return FINROM_ERR_ARG;
  }
  return launch_hmc_end_stage2(h, a->Kq[n_steps & 1], *da, (hipStream_t)stream);
}
int finrom_hmc_draw_stage2(const uint64_t* seeds, int64_t C, int64_t first_proposal, int64_t B, double* lu2_block, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (C < 0) { set_error("hmc_draw_stage2: C < 0"); return FINROM_ERR_ARG; }
  if (B < 0) { set_error("hmc_draw_stage2: B < 0"); return FINROM_ERR_ARG; }
  if (first_proposal < 0) { set_error("hmc_draw_stage2: first_proposal < 0"); return FINROM_ERR_ARG; }
  if (B == 0 || C == 0) return 0;
  if (!seeds || !lu2_block) { set_error("hmc_draw_stage2: null seeds or lu2_block"); return FINROM_ERR_ARG; }
  if (B > INT64_MAX / 8 / C || first_proposal > INT64_MAX - B) {
    set_error("hmc_draw_stage2: B x C or first_proposal + B does not fit 64 bits"); return FINROM_ERR_ARG;
  }
  return launch_hmc_draw_stage2((const unsigned long long*)seeds, C, first_proposal, B, lu2_block, (hipStream_t)stream);
}
int finrom_hmc_stats_update(const finrom_hmc_stats* s, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!s) { set_error("hmc_stats_update: null descriptor"); return FINROM_ERR_ARG; }
  if (s->C < 0) { set_error("hmc_stats_update: C < 0"); return FINROM_ERR_ARG; }
  if (s->n < 1) { set_error("hmc_stats_update: n < 1"); return FINROM_ERR_ARG; }
  if (s->batch < 1) { set_error("hmc_stats_update: batch < 1"); return FINROM_ERR_ARG; }
  if (s->burn < 0) { set_error("hmc_stats_update: burn < 0"); return FINROM_ERR_ARG; }
  if (s->proposal0 < 0) { set_error("hmc_stats_update: proposal0 < 0"); return FINROM_ERR_ARG; }
  if (s->C == 0) return 0;
  if (s->C > 65535) { set_error("hmc_stats_update: C > 65535 (one grid row per chain)"); return FINROM_ERR_ARG; }
  if (!s->pt || !s->accept || !s->cand || !s->cand_loss || !s->cur || !s->cur_loss || !s->acc_prev || !s->mean || !s->m2 ||
      !s->bsum || !s->bm_mean || !s->bm_m2) {
    set_error("hmc_stats_update: null pointer in finrom_hmc_stats (only misfit and accepted may be NULL)"); return FINROM_ERR_ARG;
  }
  return launch_hmc_stats(*s, (hipStream_t)stream);
}
int finrom_hmc_leapfrog(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, const finrom_hmc_state* a, int32_t step,
                        const double* data, int32_t data_per_sample, double* grad_out, double* qoi_r, double* e_nn, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog")) return rc;
  if (!rom || !mlp || a->n != mlp->d.n_in || step < 0) { set_error("hmc_leapfrog: bad argument"); return FINROM_ERR_ARG; }
  if (a->c_pri == 0.0) { set_error("hmc_leapfrog: c_pri = 0"); return FINROM_ERR_ARG; }
  HmcStep hs;
  hs.mom = a->P; hs.eps = a->eps; hs.k_out = a->Kq[(step + 1) & 1];
  // theta of THIS step's field from the previous step's momentum update, when this is that field's step (not the first step of a
  // trajectory: finrom_hmc_begin has no averaging operator at hand); and this step leaves the next one's
  if (int rc = mlp->thp.reserve((size_t)a->C * HMC_THETA_PARTS * 16 * sizeof(double))) return rc;
  const bool carried = step > 0 && mlp->carry_k == a->Kq[step & 1] && mlp->carry_mom == a->P && mlp->carry_eps == a->eps &&
                       mlp->carry_S == a->C;
  hs.theta_parts_in = carried ? (const double*)mlp->thp.p : nullptr;
  hs.tail.eps = a->eps; hs.tail.theta_parts = rom->d.P <= HMC_THETA_MAXP ? (double*)mlp->thp.p : nullptr;
  mlp->carry_k = nullptr;
  hs.tail.on = 1; hs.tail.kq = hs.k_out; hs.tail.mean = a->mean; hs.tail.mom = a->P; hs.tail.dU = a->dUq;
  hs.tail.coef = a->c_lik / a->c_pri; hs.tail.eps_cpri = a->eps * a->c_pri; hs.tail.info = a->info;
  const int rc = romml_grad_impl(rom, mlp, Sop, a->Kq[step & 1], data, data_per_sample, a->C, grad_out, a->loss, qoi_r, e_nn, a->info, stream, &hs);
  if (rc == 0 && hs.tail.theta_parts != nullptr) { mlp->carry_k = hs.k_out; mlp->carry_mom = a->P; mlp->carry_eps = a->eps; mlp->carry_S = a->C; }
  return rc;
}

}  // extern "C"
// the whitened steps' closing launch: the pullback of the field's gradient, with the momentum update behind it (FieldPriorTail)
static int hmc_field_tail(const finrom_hmc_state* a, finrom_sampler_t prior, double* vq, double* grad_field, hipStream_t st) {
  FieldPriorTail tl;
  tl.vq = vq; tl.c_lik = a->c_lik; tl.info = a->info; tl.mom = a->P; tl.dU = a->dUq; tl.eps = a->eps;
  return launch_field_prior(prior->U, prior->n, 1, grad_field, nullptr, 0.0, nullptr, nullptr, nullptr, &tl, a->C,
                            (double*)prior->fpart.p, (int*)prior->ftick.p, st);
}
// the leapfrog step in whitened coordinates: field kernel (position update in front), the plain romml value and gradient at the
// field, pullback kernel (momentum update behind); no theta carry (the field is not the position)
// (metric: the position moves along vel = M^-1 p, formed first -- finrom_hmc_leapfrog_field_metric; nullptr: along p itself)
static int hmc_leapfrog_field_impl(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, finrom_sampler_t prior, const double* field_mean,
                                   double* field, double* grad_field, const finrom_hmc_state* a, int32_t step, const double* data,
                                   int32_t data_per_sample, double* qoi_r, double* e_nn, const MetricDev* metric, double* vel,
                                   void* stream) {
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog_field")) return rc;
  if (a->c_pri != 1.0) { set_error("hmc_leapfrog_field: c_pri must be 1 (whitened coordinates: the prior of v is N(0, I))"); return FINROM_ERR_ARG; }
  if (step < 0) { set_error("hmc_leapfrog_field: step < 0"); return FINROM_ERR_ARG; }
  if (!rom || !mlp || !Sop || !prior) { set_error("hmc_leapfrog_field: null rom, mlp, Sop or prior handle"); return FINROM_ERR_ARG; }
  if (!field || !grad_field || !data) { set_error("hmc_leapfrog_field: null field, grad_field or data"); return FINROM_ERR_ARG; }
  if (a->n != prior->n || a->n != mlp->d.n_in) {
    set_error("hmc_leapfrog_field: n = " + std::to_string(a->n) + " is not the prior's (" + std::to_string(prior->n) +
              ") or the error model's input size (" + std::to_string(mlp->d.n_in) + ")");
    return FINROM_ERR_ARG;
  }
  mlp->carry_k = nullptr;                  // (a theta carry of finrom_hmc_leapfrog does not survive a step of this form)
  if (a->C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = field_prior_ws(prior, a->C)) return rc;
  double* vq = a->Kq[(step + 1) & 1];
  int rc = metric ? launch_hmc_velocity(*metric, a->P, a->C, vel, st) : 0;
  if (!rc) rc = launch_field_prior(prior->U, prior->n, 0, a->Kq[step & 1], metric ? vel : a->P, a->eps, field_mean, field, vq, nullptr,
                                   a->C, (double*)prior->fpart.p, (int*)prior->ftick.p, st);
  if (!rc) rc = romml_grad_impl(rom, mlp, Sop, field, data, data_per_sample, a->C, grad_field, a->loss, qoi_r, e_nn, a->info, stream, nullptr);
  if (rc) return rc;
  return hmc_field_tail(a, prior, vq, grad_field, st);
}
extern "C" {
int finrom_hmc_leapfrog_field(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, finrom_sampler_t prior, const double* field_mean,
                              double* field, double* grad_field, const finrom_hmc_state* a, int32_t step, const double* data,
                              int32_t data_per_sample, double* qoi_r, double* e_nn, void* stream) {
  CallGuard cg((hipStream_t)stream);
  return hmc_leapfrog_field_impl(rom, mlp, Sop, prior, field_mean, field, grad_field, a, step, data, data_per_sample, qoi_r, e_nn,
                                 nullptr, nullptr, stream);
}

}  // extern "C"
// ---- the chains under the full-order and the plain reduced model (hmc_model.hip; hmc.py model="fom" | "rom") ----------------------
static int hmc_model_map_check(const char* who, const double* A, int32_t P) {
  if (A != nullptr && (P < 1 || P > HMC_MODEL_MAXP)) {
    set_error(std::string(who) + ": P = " + std::to_string(P) + " is outside 1 .. " + std::to_string(HMC_MODEL_MAXP));
    return FINROM_ERR_ARG;
  }
  return 0;
}
static int hmc_drift_impl(const finrom_hmc_state* a, int32_t step, const double* A, const double* theta0, int32_t P, double* theta_out,
                          void* stream, const char* who) {
  HmcDev h;
  if (int rc = hmc_dev(a, &h, who)) return rc;
  if (step < 0) { set_error(std::string(who) + ": step < 0"); return FINROM_ERR_ARG; }
  if (int rc = hmc_model_map_check(who, A, P)) return rc;
  if (A != nullptr && !theta_out) { set_error(std::string(who) + ": A without theta_out"); return FINROM_ERR_ARG; }
  if (a->C > INT32_MAX) { set_error(std::string(who) + ": C > 2^31 - 1 (one workgroup per chain)"); return FINROM_ERR_ARG; }
  return launch_hmc_drift(h, a->Kq[step & 1], a->Kq[(step + 1) & 1], A, theta0, P, theta_out, (hipStream_t)stream);
}
static int hmc_kick_impl(const finrom_hmc_state* a, int32_t step, const double* grad, const double* g_theta, const double* A, int32_t P,
                         double* grad_out, void* stream, const char* who) {
  HmcDev h;
  if (int rc = hmc_dev(a, &h, who)) return rc;
  if (step < 0) { set_error(std::string(who) + ": step < 0"); return FINROM_ERR_ARG; }
  if ((grad != nullptr) == (g_theta != nullptr)) {
    set_error(std::string(who) + ": exactly one of grad and g_theta must be given"); return FINROM_ERR_ARG;
  }
  if (g_theta != nullptr && !A) { set_error(std::string(who) + ": g_theta without A"); return FINROM_ERR_ARG; }
  if (g_theta != nullptr) { if (int rc = hmc_model_map_check(who, A, P)) return rc; }
  if (a->c_pri == 0.0) { set_error(std::string(who) + ": c_pri = 0"); return FINROM_ERR_ARG; }
  if (a->C > 65535) { set_error(std::string(who) + ": C > 65535 (one grid row per chain)"); return FINROM_ERR_ARG; }
  return launch_hmc_kick(h, a->Kq[(step + 1) & 1], grad, g_theta, A, P, grad_out, (hipStream_t)stream);
}
extern "C" {
int finrom_hmc_drift(const finrom_hmc_state* a, int32_t step, const double* A, const double* theta0, int32_t P, double* theta_out,
                     void* stream) {
  CallGuard cg((hipStream_t)stream);
  return hmc_drift_impl(a, step, A, theta0, P, theta_out, stream, "hmc_drift");
}
int finrom_hmc_kick(const finrom_hmc_state* a, int32_t step, const double* grad, const double* g_theta, const double* A, int32_t P,
                    double* grad_out, void* stream) {
  CallGuard cg((hipStream_t)stream);
  return hmc_kick_impl(a, step, grad, g_theta, A, P, grad_out, stream, "hmc_kick");
}
}  // extern "C"
static int hmc_fom_check(finrom_fom_t fom, const finrom_hmc_state* a, const double* data, const char* who) {
  if (!fom || !data) { set_error(std::string(who) + ": null fom handle or data"); return FINROM_ERR_ARG; }
  if (fom->d.xdim != a->n) {
    set_error(std::string(who) + ": n = " + std::to_string(a->n) + " is not the full-order model's parameter count (" +
              std::to_string(fom->d.xdim) + "): the chains move nodal fields");
    return FINROM_ERR_UNSUPPORTED;
  }
  if (a->C > 65535) { set_error(std::string(who) + ": C > 65535 (one grid row per chain)"); return FINROM_ERR_UNSUPPORTED; }
  return 0;
}
extern "C" {
int finrom_hmc_leapfrog_fom(finrom_fom_t fom, const finrom_hmc_state* a, int32_t step, const double* data, int32_t data_per_sample,
                            double* grad_out, double* qoi, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog_fom")) return rc;
  if (step < 0) { set_error("hmc_leapfrog_fom: step < 0"); return FINROM_ERR_ARG; }
  if (a->c_pri == 0.0) { set_error("hmc_leapfrog_fom: c_pri = 0"); return FINROM_ERR_ARG; }
  if (int rc = hmc_fom_check(fom, a, data, "hmc_leapfrog_fom")) return rc;
  if (a->C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  double* g = grad_out;
  if (!g) { if (int rc = fom->hgrad.reserve((size_t)a->C * a->n * sizeof(double))) return rc; g = (double*)fom->hgrad.p; }
  double* kq = a->Kq[(step + 1) & 1];
  int rc = hmc_drift_impl(a, step, nullptr, nullptr, 0, nullptr, stream, "hmc_leapfrog_fom");
  if (!rc) rc = launch_clear_info(a->info, a->C, st);
  if (!rc) rc = finrom_fom_gradient(fom, kq, data, data_per_sample, a->C, g, a->loss, qoi, a->info, stream);
  if (!rc) rc = hmc_kick_impl(a, step, g, nullptr, nullptr, 0, nullptr, stream, "hmc_leapfrog_fom");
  return rc;
}
int finrom_hmc_leapfrog_field_fom(finrom_fom_t fom, finrom_sampler_t prior, const double* field_mean, double* field, double* grad_field,
                                  const finrom_hmc_state* a, int32_t step, const double* data, int32_t data_per_sample, double* qoi,
                                  void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog_field_fom")) return rc;
  if (a->c_pri != 1.0) { set_error("hmc_leapfrog_field_fom: c_pri must be 1 (whitened coordinates: the prior of v is N(0, I))"); return FINROM_ERR_ARG; }
  if (step < 0) { set_error("hmc_leapfrog_field_fom: step < 0"); return FINROM_ERR_ARG; }
  if (!prior || !field || !grad_field) { set_error("hmc_leapfrog_field_fom: null prior handle, field or grad_field"); return FINROM_ERR_ARG; }
  if (int rc = hmc_fom_check(fom, a, data, "hmc_leapfrog_field_fom")) return rc;
  if (a->n != prior->n) {
    set_error("hmc_leapfrog_field_fom: n = " + std::to_string(a->n) + " is not the prior's (" + std::to_string(prior->n) + ")");
    return FINROM_ERR_ARG;
  }
  if (a->C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = field_prior_ws(prior, a->C)) return rc;
  double* vq = a->Kq[(step + 1) & 1];
  int rc = launch_field_prior(prior->U, prior->n, 0, a->Kq[step & 1], a->P, a->eps, field_mean, field, vq, nullptr, a->C,
                              (double*)prior->fpart.p, (int*)prior->ftick.p, st);
  if (!rc) rc = launch_clear_info(a->info, a->C, st);
  if (!rc) rc = finrom_fom_gradient(fom, field, data, data_per_sample, a->C, grad_field, a->loss, qoi, a->info, stream);
  if (rc) return rc;
  return hmc_field_tail(a, prior, vq, grad_field, st);
}
int finrom_hmc_leapfrog_rom(finrom_rom_t rom, const double* A, const double* theta0, const finrom_hmc_state* a, int32_t step,
                            const double* data, int32_t data_per_sample, double* theta, double* g_theta, double* grad_out,
                            double* qoi_r, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog_rom")) return rc;
  if (step < 0) { set_error("hmc_leapfrog_rom: step < 0"); return FINROM_ERR_ARG; }
  if (a->c_pri == 0.0) { set_error("hmc_leapfrog_rom: c_pri = 0"); return FINROM_ERR_ARG; }
  if (!rom || !A || !data || !theta || !g_theta) { set_error("hmc_leapfrog_rom: null rom handle, A, data, theta or g_theta"); return FINROM_ERR_ARG; }
  if (rom->g_npairs == 0) { set_error("hmc_leapfrog_rom: finrom_rom_set_gradient has not been called"); return FINROM_ERR_ARG; }
  if (rom->d.P < 1 || rom->d.P > HMC_MODEL_MAXP) {
    set_error("hmc_leapfrog_rom: the reduced model has " + std::to_string(rom->d.P) + " averages; the step serves 1 .. " +
              std::to_string(HMC_MODEL_MAXP));
    return FINROM_ERR_UNSUPPORTED;
  }
  if (a->C > 65535) { set_error("hmc_leapfrog_rom: C > 65535 (one grid row per chain)"); return FINROM_ERR_UNSUPPORTED; }
  if (a->C == 0) return 0;
  const int P = rom->d.P;
  int rc = hmc_drift_impl(a, step, A, theta0, P, theta, stream, "hmc_leapfrog_rom");
  if (!rc) rc = launch_clear_info(a->info, a->C, (hipStream_t)stream);
  if (!rc) rc = finrom_rom_grad(rom, theta, data, data_per_sample, a->C, a->loss, g_theta, nullptr, qoi_r, a->info, stream);
  if (!rc) rc = hmc_kick_impl(a, step, nullptr, g_theta, A, P, grad_out, stream, "hmc_leapfrog_rom");
  return rc;
}

}  // extern "C"
// ---- the chains under the pure deep-learning surrogate (hmc_ml.hip; hmc.py model="ml", ml_form=) -----------------------------------
// everything both entry points refuse before any device call, then the workspaces on the handle: tape and out per chain, the walk
// back's zero operand (grown outside a capture only: Scratch::reserve refuses inside one, with a message)
static int hmc_ml_prepare(finrom_mlp_t mlp, const finrom_hmc_state* a, const double* data, double** out, const char* who) {
  if (!mlp || !data) { set_error(std::string(who) + ": null mlp handle or data"); return FINROM_ERR_ARG; }
  const MlpDev& m = mlp->d;
  if (a->n != m.n_in) {
    set_error(std::string(who) + ": n = " + std::to_string(a->n) + " is not the network's input size (" + std::to_string(m.n_in) + ")");
    return FINROM_ERR_ARG;
  }
  if (a->c_pri == 0.0) { set_error(std::string(who) + ": c_pri = 0"); return FINROM_ERR_ARG; }
  if (int fits = mlp_forward_fits(m)) return fits;
  if (a->C > 65535) { set_error(std::string(who) + ": C > 65535 (one grid row per chain)"); return FINROM_ERR_UNSUPPORTED; }
  if (a->C == 0) return 0;
  int rc;
  if ((rc = mlp->tape.reserve((size_t)a->C * (m.n_layers + 1) * m.n_w * sizeof(float)))) return rc;
  if (!*out) { if ((rc = mlp->etmp.reserve((size_t)a->C * m.n_out * sizeof(double)))) return rc; *out = (double*)mlp->etmp.p; }
  const size_t cap0 = mlp->sur_zero.cap;
  if ((rc = mlp->sur_zero.reserve((size_t)a->C * m.n_out * sizeof(double)))) return rc;
  if (mlp->sur_zero.cap != cap0) {                     // (grown: outside any capture)
    FR_HIP(hipMemset(mlp->sur_zero.p, 0, mlp->sur_zero.cap));
  }
  return 0;
}
extern "C" {
int finrom_hmc_leapfrog_ml(finrom_mlp_t mlp, const finrom_hmc_state* a, int32_t step, const double* data, int32_t data_per_sample,
                           double* grad_out, double* out, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog_ml")) return rc;
  if (step < 0) { set_error("hmc_leapfrog_ml: step < 0"); return FINROM_ERR_ARG; }
  if (int rc = hmc_ml_prepare(mlp, a, data, &out, "hmc_leapfrog_ml")) return rc;
  if (a->C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const MlpDev& m = mlp->d;
  double* g = grad_out;
  if (!g) { if (int rc = mlp->hml_grad.reserve((size_t)a->C * a->n * sizeof(double))) return rc; g = (double*)mlp->hml_grad.p; }
  const int64_t stride = data_per_sample ? m.n_out : 0;
  double* kq = a->Kq[(step + 1) & 1];
  int rc = launch_hmc_ml_forward(m, h, a->Kq[step & 1], kq, data, stride, (float*)mlp->tape.p, out, a->loss, a->info, st);
  if (!rc) rc = launch_sur_backward(m, a->C, (const float*)mlp->tape.p, data, stride, (const double*)mlp->sur_zero.p, out, g, st);
  if (!rc) rc = launch_hmc_kick(h, kq, g, nullptr, nullptr, 0, nullptr, st);
  return rc;
}
int finrom_hmc_trajectory_ml(finrom_mlp_t mlp, const finrom_hmc_state* a, int32_t n_steps, const double* data, int32_t data_per_sample,
                             void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_trajectory_ml")) return rc;
  if (n_steps < 0) { set_error("hmc_trajectory_ml: n_steps < 0"); return FINROM_ERR_ARG; }
  double* out = nullptr;
  if (int rc = hmc_ml_prepare(mlp, a, data, &out, "hmc_trajectory_ml")) return rc;
  if (a->C == 0) return 0;
  const MlpDev& m = mlp->d;
  return launch_hmc_ml_trajectory(m, h, n_steps, a->Kq[0], a->Kq[1], data, data_per_sample ? m.n_out : 0, (const double*)mlp->sur_zero.p,
                                  (float*)mlp->tape.p, out, a->loss, a->info, (hipStream_t)stream);
}
}  // extern "C"
// finrom_hmc_nuts_ml (eps_c NULL: the state's step) and finrom_hmc_nuts_ml_adapt (eps_c [C]: each chain's own)
static int hmc_nuts_ml_impl(finrom_mlp_t mlp, const finrom_hmc_state* a, const double* eps_c, const uint64_t* seeds, int64_t proposal0,
                            int32_t max_depth, const double* data, int32_t data_per_sample, int32_t* tree, double* accept_stat,
                            void* stream, const std::string& who) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, who.c_str())) return rc;
  if (max_depth < 1 || max_depth > NUTS_MAX_DEPTH) {
    set_error(who + ": max_depth = " + std::to_string(max_depth) + " is outside 1 .. " + std::to_string(NUTS_MAX_DEPTH)); return FINROM_ERR_ARG;
  }
  if (proposal0 < 0) { set_error(who + ": proposal0 < 0"); return FINROM_ERR_ARG; }
  if (!seeds) { set_error(who + ": null seeds"); return FINROM_ERR_ARG; }
  double* out = nullptr;
  if (int rc = hmc_ml_prepare(mlp, a, data, &out, who.c_str())) return rc;
  if (a->C == 0) return 0;
  const MlpDev& m = mlp->d;
  const int64_t wsd = hmc_nuts_ws_doubles(a->C, a->n);
  if (int rc = mlp->nuts_ws.reserve((size_t)(wsd + (2 + NUTS_SCALARS) * a->C) * sizeof(double))) return rc;      // (grown outside a capture only)
  NutsDev nd;
  nd.max_depth = max_depth; nd.proposal0 = proposal0; nd.seeds = (const unsigned long long*)seeds;
  nd.ws = (double*)mlp->nuts_ws.p; nd.wloss = nd.ws + wsd; nd.winfo = (int*)(nd.wloss + a->C); nd.scal = nd.wloss + 2 * a->C; nd.st_loss = a->loss;
  nd.tree = tree; nd.accept_stat = accept_stat; nd.eps_c = eps_c;
  return launch_hmc_nuts_ml(m, h, nd, data, data_per_sample ? m.n_out : 0, (const double*)mlp->sur_zero.p, (float*)mlp->tape.p, out,
                            (hipStream_t)stream);
}
extern "C" {
int finrom_hmc_nuts_ml(finrom_mlp_t mlp, const finrom_hmc_state* a, const uint64_t* seeds, int64_t proposal0, int32_t max_depth,
                       const double* data, int32_t data_per_sample, int32_t* tree, double* accept_stat, void* stream) {
  return hmc_nuts_ml_impl(mlp, a, nullptr, seeds, proposal0, max_depth, data, data_per_sample, tree, accept_stat, stream, "hmc_nuts_ml");
}
int finrom_hmc_nuts_ml_adapt(finrom_mlp_t mlp, const finrom_hmc_state* a, const double* eps, const uint64_t* seeds, int64_t proposal0,
                             int32_t max_depth, const double* data, int32_t data_per_sample, int32_t* tree, double* accept_stat,
                             void* stream) {
  if (!eps) { set_error("hmc_nuts_ml_adapt: null eps"); return FINROM_ERR_ARG; }
  return hmc_nuts_ml_impl(mlp, a, eps, seeds, proposal0, max_depth, data, data_per_sample, tree, accept_stat, stream, "hmc_nuts_ml_adapt");
}
}  // extern "C"
// ---- the No-U-turn transition under any model, one leaf per launch (hmc_nuts_model.hip; hmc.py model="fom" | "rom" | "romml", nuts=) ----
// everything the three entry points refuse before any device call; the workspace is the caller's, cut here into its three parts
static int hmc_nuts_tree_dev(const finrom_hmc_state* a, const finrom_hmc_nuts_tree* tr, HmcDev* h, NutsTreeDev* d, const char* who) {
  if (int rc = hmc_dev(a, h, who)) return rc;
  if (!tr || !tr->ws || !tr->seeds || !tr->state_loss || !tr->active) {
    set_error(std::string(who) + ": null descriptor or null field in finrom_hmc_nuts_tree (only tree and accept_stat may be NULL)");
    return FINROM_ERR_ARG;
  }
  if (a->c_pri == 0.0) { set_error(std::string(who) + ": c_pri = 0"); return FINROM_ERR_ARG; }
  if (tr->max_depth < 1 || tr->max_depth > NUTS_MAX_DEPTH) {
    set_error(std::string(who) + ": max_depth = " + std::to_string(tr->max_depth) + " is outside 1 .. " + std::to_string(NUTS_MAX_DEPTH));
    return FINROM_ERR_ARG;
  }
  if (tr->proposal0 < 0) { set_error(std::string(who) + ": proposal0 < 0"); return FINROM_ERR_ARG; }
  if (((uintptr_t)tr->ws & 7u) != 0) { set_error(std::string(who) + ": ws is not aligned to 8 bytes"); return FINROM_ERR_ARG; }
  if (a->C > 65535) { set_error(std::string(who) + ": C > 65535 (one grid row per chain)"); return FINROM_ERR_UNSUPPORTED; }
  d->max_depth = tr->max_depth; d->proposal0 = tr->proposal0; d->seeds = (const unsigned long long*)tr->seeds;
  d->ws = (double*)tr->ws;
  d->scal = d->ws + (int64_t)(NUTS_TREE_FIXED_ARRAYS + 2 * tr->max_depth) * a->C * a->n;
  d->ints = (int*)(d->scal + a->C * NUTS_TREE_SCALARS);
  d->st_loss = tr->state_loss; d->tree = tr->tree; d->accept_stat = tr->accept_stat; d->active = tr->active;
  return 0;
}
static int hmc_nuts_map(const char* who, const double* A, const double* theta0, int32_t P, double* theta_out, NutsMap* tm) {
  if (int rc = hmc_model_map_check(who, A, P)) return rc;
  if (A != nullptr && !theta_out) { set_error(std::string(who) + ": A without theta_out"); return FINROM_ERR_ARG; }
  tm->A = A; tm->theta0 = A != nullptr ? theta0 : nullptr; tm->P = A != nullptr ? P : 0; tm->theta_out = A != nullptr ? theta_out : nullptr;
  return 0;
}
extern "C" {
int64_t finrom_hmc_nuts_ws_bytes(int64_t C, int32_t n, int32_t max_depth) {
  if (C < 0 || n < 1 || max_depth < 1 || max_depth > NUTS_MAX_DEPTH) {
    set_error("hmc_nuts_ws_bytes: C < 0, n < 1 or max_depth outside 1 .. " + std::to_string(NUTS_MAX_DEPTH)); return FINROM_ERR_ARG;
  }
  return hmc_nuts_tree_ws_bytes(C, n, max_depth);
}
}  // extern "C"
// begin and leaf (eps_c NULL: the state's step) and their _adapt forms (eps_c [C]: each chain's own)
static int hmc_nuts_begin_impl(const finrom_hmc_state* a, const finrom_hmc_nuts_tree* tr, const double* eps_c, const double* A,
                               const double* theta0, int32_t P, double* theta_out, void* stream, const char* who) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h; NutsTreeDev d; NutsMap tm;
  if (int rc = hmc_nuts_tree_dev(a, tr, &h, &d, who)) return rc;
  if (int rc = hmc_nuts_map(who, A, theta0, P, theta_out, &tm)) return rc;
  d.eps_c = eps_c;
  return launch_hmc_nuts_begin(h, d, tm, (hipStream_t)stream);
}
static int hmc_nuts_leaf_impl(const finrom_hmc_state* a, const finrom_hmc_nuts_tree* tr, const double* eps_c, const double* grad,
                              const double* g_theta, const double* A, const double* theta0, int32_t P, double* theta_out, void* stream,
                              const std::string& who) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h; NutsTreeDev d; NutsMap tm;
  if (int rc = hmc_nuts_tree_dev(a, tr, &h, &d, who.c_str())) return rc;
  if ((grad != nullptr) == (g_theta != nullptr)) {
    set_error(who + ": exactly one of grad and g_theta must be given"); return FINROM_ERR_ARG;
  }
  if (g_theta != nullptr && !A) { set_error(who + ": g_theta without A"); return FINROM_ERR_ARG; }
  if (int rc = hmc_nuts_map(who.c_str(), A, theta0, P, theta_out, &tm)) return rc;
  d.eps_c = eps_c;
  return launch_hmc_nuts_leaf(h, d, grad, g_theta, tm, (hipStream_t)stream);
}
extern "C" {
int finrom_hmc_nuts_begin(const finrom_hmc_state* a, const finrom_hmc_nuts_tree* tr, const double* A, const double* theta0, int32_t P,
                          double* theta_out, void* stream) {
  return hmc_nuts_begin_impl(a, tr, nullptr, A, theta0, P, theta_out, stream, "hmc_nuts_begin");
}
int finrom_hmc_nuts_leaf(const finrom_hmc_state* a, const finrom_hmc_nuts_tree* tr, const double* grad, const double* g_theta,
                         const double* A, const double* theta0, int32_t P, double* theta_out, void* stream) {
  return hmc_nuts_leaf_impl(a, tr, nullptr, grad, g_theta, A, theta0, P, theta_out, stream, "hmc_nuts_leaf");
}
int finrom_hmc_nuts_begin_adapt(const finrom_hmc_state* a, const finrom_hmc_nuts_tree* tr, const double* eps, const double* A,
                                const double* theta0, int32_t P, double* theta_out, void* stream) {
  if (!eps) { set_error("hmc_nuts_begin_adapt: null eps"); return FINROM_ERR_ARG; }
  return hmc_nuts_begin_impl(a, tr, eps, A, theta0, P, theta_out, stream, "hmc_nuts_begin_adapt");
}
int finrom_hmc_nuts_leaf_adapt(const finrom_hmc_state* a, const finrom_hmc_nuts_tree* tr, const double* eps, const double* grad,
                               const double* g_theta, const double* A, const double* theta0, int32_t P, double* theta_out,
                               void* stream) {
  if (!eps) { set_error("hmc_nuts_leaf_adapt: null eps"); return FINROM_ERR_ARG; }
  return hmc_nuts_leaf_impl(a, tr, eps, grad, g_theta, A, theta0, P, theta_out, stream, "hmc_nuts_leaf_adapt");
}
// the dual-averaging update of every chain's step (hmc_nuts_model.hip): everything refused here, before any device call
int finrom_hmc_step_adapt_update(const finrom_hmc_step_adapt* ad, int64_t C, int64_t proposal0, const int64_t* pt,
                                 const double* accept_stat, double* step_size, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!ad || !ad->eps || !ad->hbar || !ad->xbar) {
    set_error("hmc_step_adapt_update: null descriptor or null eps, hbar or xbar in finrom_hmc_step_adapt"); return FINROM_ERR_ARG;
  }
  if (ad->tune < 0) { set_error("hmc_step_adapt_update: tune < 0"); return FINROM_ERR_ARG; }
  if (!(ad->target > 0.0 && ad->target < 1.0)) {
    set_error("hmc_step_adapt_update: target = " + std::to_string(ad->target) + " is outside (0, 1)"); return FINROM_ERR_ARG;
  }
  if (!(ad->gamma > 0.0) || !(ad->t0 > 0.0) || !std::isfinite(ad->mu)) {
    set_error("hmc_step_adapt_update: gamma or t0 is not > 0, or mu is not finite"); return FINROM_ERR_ARG;
  }
  if (C < 0) { set_error("hmc_step_adapt_update: C < 0"); return FINROM_ERR_ARG; }
  if (proposal0 < 0) { set_error("hmc_step_adapt_update: proposal0 < 0"); return FINROM_ERR_ARG; }
  if (C == 0) return 0;
  if (!pt) { set_error("hmc_step_adapt_update: null pt"); return FINROM_ERR_ARG; }
  if (!accept_stat) { set_error("hmc_step_adapt_update: null accept_stat"); return FINROM_ERR_ARG; }
  StepAdaptDev d;
  d.eps = ad->eps; d.hbar = ad->hbar; d.xbar = ad->xbar; d.mu = ad->mu; d.target = ad->target; d.gamma = ad->gamma; d.t0 = ad->t0;
  d.tune = ad->tune; d.C = C; d.proposal0 = proposal0; d.pt = (const long long*)pt; d.accept_stat = accept_stat; d.step_size = step_size;
  return launch_hmc_step_adapt(d, (hipStream_t)stream);
}
int finrom_hmc_nuts_end(const finrom_hmc_state* a, const finrom_hmc_nuts_tree* tr, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h; NutsTreeDev d;
  if (int rc = hmc_nuts_tree_dev(a, tr, &h, &d, "hmc_nuts_end")) return rc;
  return launch_hmc_nuts_end(h, d, (hipStream_t)stream);
}

// ---- low-rank metric (hmc_metric.hip) --------------------------------------------------------------------------------------------
int finrom_metric_create(const double* Vt, const double* lam, int32_t n, int32_t rho, finrom_metric_t* out) {
  if (!out) { set_error("metric_create: null out"); return FINROM_ERR_ARG; }
  *out = nullptr;
  if (!Vt || !lam || n <= 0) { set_error("metric_create: null Vt or lam, or n <= 0"); return FINROM_ERR_ARG; }
  if (rho < 1 || rho > METRIC_MAX_RHO) {
    set_error("metric_create: rho = " + std::to_string(rho) + " (need 1 <= rho <= 64)"); return FINROM_ERR_ARG;
  }
  for (int j = 0; j < rho; ++j)
    if (!std::isfinite(lam[j]) || !(lam[j] > 0.0)) {
      set_error("metric_create: lambda[" + std::to_string(j) + "] = " + std::to_string(lam[j]) + " (need finite and > 0)"); return FINROM_ERR_ARG;
    }
  double worst = 0.0;
  for (int i = 0; i < rho; ++i)
    for (int j = 0; j <= i; ++j) {
      long double s = 0.0L;
      for (int q = 0; q < n; ++q) s += (long double)Vt[(size_t)i * n + q] * Vt[(size_t)j * n + q];
      const double e = std::fabs((double)(s - (i == j ? 1.0L : 0.0L)));
      if (!(e <= worst)) worst = e;                      // (a NaN sticks)
    }
  if (!(worst <= 1e-10)) {
    set_error("metric_create: the rows of Vt are not orthonormal (|Vt Vt^T - I|_max = " + std::to_string(worst) + " > 1e-10)"); return FINROM_ERR_ARG;
  }
  std::vector<double> coef((size_t)METRIC_NUM_COEF * METRIC_MAX_RHO, 0.0);
  for (int j = 0; j < rho; ++j) {                        // (forms without cancellation at small lambda)
    const double l = lam[j], s = std::sqrt(1.0 + l);
    coef[(size_t)METRIC_OP_M * METRIC_MAX_RHO + j] = l;
    coef[(size_t)METRIC_OP_INV * METRIC_MAX_RHO + j] = -l / (1.0 + l);
    coef[(size_t)METRIC_OP_SQRT * METRIC_MAX_RHO + j] = l / (s + 1.0);
    coef[(size_t)METRIC_OP_INVSQRT * METRIC_MAX_RHO + j] = -l / ((1.0 + l) + s);
    coef[(size_t)METRIC_OP_D * METRIC_MAX_RHO + j] = l / (1.0 + l);
  }
  auto* h = new finrom_metric_s();
  h->d.n = n; h->d.rho = rho;
  double* dv = nullptr; double* dc = nullptr;
  int rc = upload(&dv, Vt, (size_t)rho * n);
  if (!rc) rc = upload(&dc, coef.data(), coef.size());
  h->d.Vt = dv; h->d.coef = dc;
  if (rc) { finrom_metric_destroy(h); return rc; }
  *out = h;
  return 0;
}
void finrom_metric_destroy(finrom_metric_t h) { if (!h) return; dev_free((void*)h->d.Vt); dev_free((void*)h->d.coef); delete h; }
int finrom_metric_apply(finrom_metric_t h, int32_t op, const double* x, int64_t S, double* y, double* quad, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!x || !y))) { set_error("metric_apply: bad argument (null handle, x or y, or S < 0)"); return FINROM_ERR_ARG; }
  if (op < FINROM_METRIC_M || op > FINROM_METRIC_INVSQRT) { set_error("metric_apply: op = " + std::to_string(op) + " (need 0 .. 3)"); return FINROM_ERR_ARG; }
  if (S > 0 && x == y) { set_error("metric_apply: y must not be x"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  return launch_metric_apply(h->d, op, x, S, y, quad, (hipStream_t)stream);
}
}  // extern "C"
static int hmc_metric_check(const finrom_hmc_state* a, finrom_metric_t m, const char* who) {
  if (!m) { set_error(std::string(who) + ": null metric handle"); return FINROM_ERR_ARG; }
  if (a->n != m->d.n) {
    set_error(std::string(who) + ": n = " + std::to_string(a->n) + " is not the metric's (" + std::to_string(m->d.n) + ")"); return FINROM_ERR_ARG;
  }
  return 0;
}
extern "C" {
int finrom_hmc_begin_metric(const finrom_hmc_state* a, finrom_metric_t metric, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_begin_metric")) return rc;
  if (int rc = hmc_metric_check(a, metric, "hmc_begin_metric")) return rc;
  return launch_hmc_begin_metric(h, metric->d, (hipStream_t)stream);
}
int finrom_hmc_end_metric(const finrom_hmc_state* a, finrom_metric_t metric, int32_t n_steps, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_end_metric")) return rc;
  if (int rc = hmc_metric_check(a, metric, "hmc_end_metric")) return rc;
  if (n_steps < 0) { set_error("hmc_end_metric: n_steps < 0"); return FINROM_ERR_ARG; }
  return launch_hmc_end_metric(h, metric->d, a->Kq[n_steps & 1], (hipStream_t)stream);
}
}  // extern "C"
// the No-U-turn transition under the metric (hmc_nuts.hip): finrom_hmc_nuts_ml's checks, the metric's, the larger workspace
// (eps_c NULL: the state's step; finrom_hmc_nuts_ml_metric_adapt: each chain's own)
static int hmc_nuts_ml_metric_impl(finrom_mlp_t mlp, const finrom_hmc_state* a, finrom_metric_t metric, const double* eps_c,
                                   const uint64_t* seeds, int64_t proposal0, int32_t max_depth, const double* data,
                                   int32_t data_per_sample, int32_t* tree, double* accept_stat, void* stream, const std::string& who) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, who.c_str())) return rc;
  if (max_depth < 1 || max_depth > NUTS_MAX_DEPTH) {
    set_error(who + ": max_depth = " + std::to_string(max_depth) + " is outside 1 .. " + std::to_string(NUTS_MAX_DEPTH));
    return FINROM_ERR_ARG;
  }
  if (proposal0 < 0) { set_error(who + ": proposal0 < 0"); return FINROM_ERR_ARG; }
  if (!seeds) { set_error(who + ": null seeds"); return FINROM_ERR_ARG; }
  if (int rc = hmc_metric_check(a, metric, who.c_str())) return rc;
  double* out = nullptr;
  if (int rc = hmc_ml_prepare(mlp, a, data, &out, who.c_str())) return rc;
  if (a->C == 0) return 0;
  const MlpDev& m = mlp->d;
  const int64_t wsd = hmc_nuts_metric_ws_doubles(a->C, a->n);
  if (int rc = mlp->nuts_ws.reserve((size_t)(wsd + (2 + NUTS_SCALARS) * a->C) * sizeof(double))) return rc;      // (grown outside a capture only)
  NutsDev nd;
  nd.max_depth = max_depth; nd.proposal0 = proposal0; nd.seeds = (const unsigned long long*)seeds;
  nd.ws = (double*)mlp->nuts_ws.p; nd.wloss = nd.ws + wsd; nd.winfo = (int*)(nd.wloss + a->C); nd.scal = nd.wloss + 2 * a->C; nd.st_loss = a->loss;
  nd.tree = tree; nd.accept_stat = accept_stat; nd.eps_c = eps_c;
  return launch_hmc_nuts_ml_metric(m, h, nd, metric->d, data, data_per_sample ? m.n_out : 0, (const double*)mlp->sur_zero.p,
                                   (float*)mlp->tape.p, out, (hipStream_t)stream);
}
extern "C" {
int finrom_hmc_nuts_ml_metric(finrom_mlp_t mlp, const finrom_hmc_state* a, finrom_metric_t metric, const uint64_t* seeds, int64_t proposal0,
                              int32_t max_depth, const double* data, int32_t data_per_sample, int32_t* tree, double* accept_stat,
                              void* stream) {
  return hmc_nuts_ml_metric_impl(mlp, a, metric, nullptr, seeds, proposal0, max_depth, data, data_per_sample, tree, accept_stat, stream,
                                 "hmc_nuts_ml_metric");
}
int finrom_hmc_nuts_ml_metric_adapt(finrom_mlp_t mlp, const finrom_hmc_state* a, finrom_metric_t metric, const double* eps,
                                    const uint64_t* seeds, int64_t proposal0, int32_t max_depth, const double* data,
                                    int32_t data_per_sample, int32_t* tree, double* accept_stat, void* stream) {
  if (!eps) { set_error("hmc_nuts_ml_metric_adapt: null eps"); return FINROM_ERR_ARG; }
  return hmc_nuts_ml_metric_impl(mlp, a, metric, eps, seeds, proposal0, max_depth, data, data_per_sample, tree, accept_stat, stream,
                                 "hmc_nuts_ml_metric_adapt");
}
int finrom_hmc_leapfrog_field_metric(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, finrom_sampler_t prior,
                                     const double* field_mean, double* field, double* grad_field, const finrom_hmc_state* a,
                                     int32_t step, const double* data, int32_t data_per_sample, double* qoi_r, double* e_nn,
                                     finrom_metric_t metric, double* vel, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!a || !metric || !vel) { set_error("hmc_leapfrog_field_metric: null state, metric handle or vel"); return FINROM_ERR_ARG; }
  if (a->n != metric->d.n) {
    set_error("hmc_leapfrog_field_metric: n = " + std::to_string(a->n) + " is not the metric's (" + std::to_string(metric->d.n) + ")");
    return FINROM_ERR_ARG;
  }
  return hmc_leapfrog_field_impl(rom, mlp, Sop, prior, field_mean, field, grad_field, a, step, data, data_per_sample, qoi_r, e_nn,
                                 &metric->d, vel, stream);
}

}  // extern "C"
