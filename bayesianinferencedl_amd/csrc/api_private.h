// Private to the host layer (api_runtime.hip, api_fom.hip, api_rom.hip, api_infer.hip, api_hmc.hip, fom_band_tables.hip,
// rom_tables.hip): the handle structs behind include/finrom.h's opaque pointers, and the few helpers one of those units defines
// and another calls.  No kernel source includes this header.  Who defines what is shared:
//   api_runtime.hip      overlap_enabled (and finrom_core.h's set_error, CallGuard, Scratch, dev_free, defer_or_run,
//                        ScopedKernelTimer)
//   api_fom.hip          env_no_band, fom_chunk_samples, fom_solve_stages       (called by api_rom.hip: finrom_solve_pairs)
//   api_infer.hip        field_prior_ws, romml_grad_impl (with struct HmcStep)  (called by api_hmc.hip)
//   fom_band_tables.hip  validate_band, validate_band_mirror, derive_post_functionals, derive_pivot_records, check_pivot_records
//   rom_tables.hip       what rom_tables.h declares
#pragma once
#include "finrom_internal.h"
#include "mlp_surrogate.h"
#include "rom_tables.h"

using namespace finrom;      // (the handle structs are the C ABI's: global names, made of finrom:: parts)

struct finrom_fom_s {
  FomDev d{};
  FomSmallDev small{};
  BandDev band{};                      // frontal band sweep (finrom_fom_set_band); band.on = 0: interpreter
  BandGradDev band_grad{};             // adjoint gradient on the band layout (finrom_fom_set_band_gradient)
  FomDev band_asm{};                   // parameters of the band sweep's assembly pre-pass (fom_assemble_kernel)
  // half-domain plan of a mirror-symmetric operator (finrom_fom_set_band_mirror): serves the calls that want no w
  BandDev band_m{};
  FomDev band_m_asm{};
  BandFnDev band_m_fn{};               // cw != nullptr: band_m is in the functional form of the post (no stored factor; DESIGN 4c')
  const BandDev& band_for(bool want_w) const { return !want_w && band_m.on ? band_m : band; }
  std::vector<void*> owned;
  Scratch xT, Gw, gradT, qtmp;
  Scratch hgrad;                       // finrom_hmc_leapfrog_fom without grad_out: the gradient between the FOM's launches and the kick
  int last_path = FINROM_FOM_PATH_NONE;   // finrom_fom_last_path
};
struct finrom_rom_s {
  RomDev d{};
  std::vector<void*> owned;
  Scratch Ar, Br, theta, qtmp, vw, grad_ticket, part, ext;
  int g_npairs = 0; const int* g_pair_p = nullptr; const int* g_pair_i = nullptr; const double* g_Gt = nullptr;
  RomGramDev gram;                     // offline/online form (finrom_rom_set_gram); gram.h is filled at create
  int projection = FINROM_PROJECTION_DIRECT;
  std::vector<double> tvg_host; std::vector<int> kmg_host, def_host;      // the grouped tables as uploaded (finrom_rom_set_mirror appends to them)
  int mirror_n = 0;                    // rows of the installed half descriptor
  int mirror_counts[3][3] = {};        // finrom_rom_mirror_info: {rows with terms, k-steps, k-steps with arithmetic} of the half / short / compact list
  // the COMPACT list (finrom_rom_set_mirror_compact, DESIGN 4b''): where its records start in RomDev::kmg, its padded k-step count (0:
  // none), its final factor.  Kept here, not in RomDev: a launch that offers it gets them in the short list's fields (rom_project).
  // Offered where finrom_solve_pairs masks the sweep by default (the batches of the block-row epilogue); read at creation:
  // FINROM_ROM_COMPACT=1 wherever the short list is offered (tests), FINROM_ROM_NO_COMPACT=1 never (A/B)
  int kmg_c = 0, nkg_c = 0, ext_final_c = 0;
  bool compact_always = getenv("FINROM_ROM_COMPACT") != nullptr, no_compact = getenv("FINROM_ROM_NO_COMPACT") != nullptr;
  bool compact(bool masked_by_default) const { return !no_compact && (compact_always || masked_by_default); }
  int last_form = FINROM_ROM_FORM_NONE;  // finrom_rom_last_form
  int last_epilogue = FINROM_ROM_EPILOGUE_NONE;      // finrom_rom_last_epilogue
  bool short_grouped = env_rom_short_grouped();      // (A/B, read at creation: the short half list keeps a group per leading parameter, as before group_pays)
  bool no_roomy = getenv("FINROM_PROJ_NO_ROOMY") != nullptr;      // (A/B, read at creation: the pair path keeps the 200-register one-wave kernel)
  // the roomy epilogue without fixed waits between dependent MFMAs: where finrom_solve_pairs runs the sweep on its masked
  // stream.  Read at creation: FINROM_PROJ_FIXED_WAITS=1 never (A/B), FINROM_PROJ_SHORT_WAITS=1 at every batch size (tests)
  bool fixed_waits = getenv("FINROM_PROJ_FIXED_WAITS") != nullptr, short_waits_always = getenv("FINROM_PROJ_SHORT_WAITS") != nullptr;
  bool short_waits(bool sweep_masked) const { return !fixed_waits && (short_waits_always || sweep_masked); }
  // the short-waits epilogue that eliminates each block row in place instead of forming U_kk^-T: where the
  // default takes the short waits, at the basis widths (d.NB) where it measured faster -- a handle under either switch above keeps
  // its form.  Read at creation: FINROM_PROJ_BLOCK_ROW=1 at every batch size and width (tests), FINROM_PROJ_NO_BLOCK_ROW=1 never (A/B)
  bool block_row_always = getenv("FINROM_PROJ_BLOCK_ROW") != nullptr, no_block_row = getenv("FINROM_PROJ_NO_BLOCK_ROW") != nullptr;
  bool block_row(bool masked_by_default) const {      // (the batches finrom_solve_pairs masks the sweep for unless told otherwise)
    if (no_block_row) return false;
    return block_row_always || (!fixed_waits && !short_waits_always && masked_by_default && ((ROM_BLOCK_ROW_NB_MASK >> d.NB) & 1));
  }
  hipStream_t side = nullptr;          // library-owned stream for the ROM half of finrom_solve_pairs / the error model of finrom_romml_grad
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // the FOM half of finrom_solve_pairs on a stream restricted to a SUBSET of the CUs (hipExtStreamCreateWithCUMask): the sweep's
  // waves then share SIMDs with the projection on those CUs only, and run faster for being fewer.  cus < 0: per_se = -cus
  // CUs in every shader engine (the mask's bit i is CU i / n_se of shader engine i % n_se -- measured: the first 32 c bits give the
  // sweep the same speed as any 32 c' <= bits < 32 (c + 1), and bit patterns that fill whole engines starve the dispatcher)
  hipStream_t fom_side = nullptr; hipEvent_t ev_join_fom = nullptr; int fom_side_cus = 0;
  int ensure_fom_side(int cus) {
    if (fom_side_cus == cus && (fom_side || cus != 0)) return 0;      // (made, or refused by the runtime once: do not ask again)
    if (call_captures() || any_capture()) { set_error("the FOM side stream cannot be created while a stream capture is open"); return FINROM_ERR_UNSUPPORTED; }
    if (fom_side) { (void)hipStreamDestroy(fom_side); fom_side = nullptr; }
    int dev = 0; hipDeviceProp_t pr;
    FR_HIP(hipGetDevice(&dev));
    FR_HIP(hipGetDeviceProperties(&pr, dev));
    const int ncu = pr.multiProcessorCount;
    const int want = cus;
    if (cus < 0) cus = -cus * (ncu / 8);                 // (eight CUs per shader engine on gfx950)
    if (cus < 1 || cus > ncu) { set_error("FINROM_FOM_CUS out of range"); return FINROM_ERR_ARG; }
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    for (int b = 0; b < cus; ++b) mask[b >> 5] |= 1u << (b & 31);      // the first `cus` bits
    // (a runtime that refuses the mask is not an error of the call: the FOM half then stays on the caller's stream, as before)
    if (hipExtStreamCreateWithCUMask(&fom_side, (uint32_t)mask.size(), mask.data()) != hipSuccess) { (void)hipGetLastError(); fom_side = nullptr; fom_side_cus = want; return 0; }
    if (!ev_join_fom) FR_HIP(hipEventCreateWithFlags(&ev_join_fom, hipEventDisableTiming));
    fom_side_cus = want;
    return 0;
  }
  int ensure_side() {
    if (side) return 0;
    if (call_captures() || any_capture()) { set_error("the library's side stream cannot be created while a stream capture is open: run the call once before the capture"); return FINROM_ERR_UNSUPPORTED; }
    int lo = 0, hi = 0;
    FR_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));          // numerically lower = higher priority
    FR_HIP(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, hi));
    FR_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    FR_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    return 0;
  }
  // finrom_romml_grad -> finrom_rom_grad (one-sample form only): leave the gradient's partial sums to the consumer; where they are
  bool defer_gsum = false; const double* last_gpart = nullptr;
  const MlpFuse* fuse = nullptr;       // (same path) the error model's forward pass as a workgroup of the contraction kernel
  const MlpBackFuse* back = nullptr;   // (same path) its walk back through the hidden layers as a workgroup of the gradient contraction
  bool info_store = false;             // (same path) the solve kernel stores info instead of or-ing into it
};
struct finrom_sampler_s {
  double* U = nullptr; int n = 0; Scratch xi;
  Scratch fpart, ftick;                // finrom_sampler_field / _pullback / finrom_hmc_leapfrog_field: partial sums, arrival counters
};
struct finrom_metric_s { MetricDev d{}; };
struct finrom_mlp_s {
  MlpDev d{}; std::vector<void*> owned; Scratch tape, theta, gth, shift, qtmp, etmp, g0, y0p, thp;
  // finrom_hmc_leapfrog: the partial sums of theta the last step left in thp, and the field they belong to (position buffer,
  // momentum buffer, step size, chains): the next step uses them only if it is that field's step
  const double* carry_k = nullptr; const double* carry_mom = nullptr; double carry_eps = 0.0; int64_t carry_S = 0;
  // finrom_mlp_misfit_grad (mlp_surrogate.hip): the tile form's padded weights (made by the first call that needs them, outside any
  // capture), the per-sample walk's zero operand, the tile form's row flags; which form the last call took
  Scratch sur_w, sur_zero, sur_bad;
  Scratch nuts_ws;                     // finrom_hmc_nuts_ml: the trees' per-chain arrays, a leaf's misfit and flag behind them
  Scratch hml_grad;                    // finrom_hmc_leapfrog_ml without grad_out: the gradient between the walk back and the kick
  SurPad sur_pad; bool sur_ready = false;
  int64_t tile_min = 4096;      // (the measured crossover of the two forms at n = 1597: DESIGN 7)
  int last_form = 0;
};

namespace finrom {
template <class T>
int up(std::vector<void*>& owned, const T** dst, const T* host, size_t count) {
  T* dp = nullptr;
  int rc = upload(&dp, host, count);
  if (rc) return rc;
  if (dp) owned.push_back(dp);
  *dst = dp;
  return 0;
}

// api_runtime.hip
bool overlap_enabled();                    // finrom_set_overlap's flag (finrom_solve_pairs reads it)

// fom_band_tables.hip (host only)
int validate_band(const finrom_fom_band_desc* a, int n, int xdim, int n_obs, int64_t* gsize_out, int64_t* nL_out);
int validate_band_mirror(const finrom_fom_band_desc* a, int n_half, int xdim, int n_rows, int n_obs, const int32_t* out_ptr,
                         const int32_t* out_col, int64_t* gsize_out, int64_t* nL_out);
int derive_post_functionals(const finrom_fom_band_desc* a, int n_half, int n_rows, std::vector<double>& cw, std::vector<int>& piv_row,
                            std::vector<int>& piv_off);
void derive_pivot_records(const finrom_fom_band_desc* a, const std::vector<double>& cw, const std::vector<int>& piv_row,
                          const std::vector<int>& piv_off, std::vector<BandFinRec>& fin_rec, std::vector<BandPostRec>& post_rec);
int check_pivot_records(const finrom_fom_band_desc* a, const std::vector<double>& cw, const std::vector<int>& piv_row,
                        const std::vector<int>& piv_off, const BandFinRec* fin_rec, const BandPostRec* post_rec);

// the FOM half as finrom_solve_pairs runs it, in stages (api_fom.hip)
bool env_no_band();                        // FINROM_NO_BAND, read once per process
int64_t fom_chunk_samples(const FomDev& d, const BandDev* band = nullptr);
// records = false: a half plan in the functional form sweeps on its tables although pivot records are installed
int fom_solve_stages(finrom_fom_t h, const double* x, int64_t S, double* qoi, double* w, int32_t* info, hipStream_t st, int stages,
                     bool records = true);

// api_infer.hip, for the HMC steps of api_hmc.hip
int field_prior_ws(finrom_sampler_t h, int64_t S);
// (hs: the call is a leapfrog step -- finrom_hmc_leapfrog: position update in front, momentum update behind; one-sample form only)
struct HmcStep { const double* mom; double eps; double* k_out; HmcTail tail; const double* theta_parts_in; };
int romml_grad_impl(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, const double* k, const double* data,
                    int32_t data_per_sample, int64_t S, double* grad, double* loss, double* qoi_r, double* e_nn,
                    int32_t* info, void* stream, const HmcStep* hs);
}  // namespace finrom
