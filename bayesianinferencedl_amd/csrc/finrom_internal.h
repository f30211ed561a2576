// Internal declarations of the reduced model and the learned error model (on top of finrom_core.h).
#pragma once
#include "finrom_core.h"

namespace finrom {

// ---- learned error model (mlp_kernels.hip, finrom_mlp_*) ----------------------------------
struct MlpDev {
  int n_in, n_w, n_layers, n_out;
  const float* W0; const float* b0;            // [n_in x n_w], [n_w]
  const float* scale; const float* shift;      // [(n_layers + 1) x n_w] inference-form batch normalisation (last row: the head)
  const float* W; const float* b;              // [n_layers x n_w x n_w], [n_layers x n_w]
  const float* Wh; const float* bh;            // [n_w x n_out], [n_out]
};
// the error model's forward pass riding as ONE MORE workgroup per sample in rom_small_proj_kernel (finrom_romml_grad's one-sample
// form: the ROM's contraction does not depend on it, the solve kernel behind both is the first to need its output)
struct MlpFuse {
  int on = 0;
  MlpDev m{};
  const double* k = nullptr; const double* data = nullptr; int64_t data_stride = 0;
  float* tape = nullptr; double* e_out = nullptr; double* data_shift = nullptr;
  // the sub-fin averages theta = S k too: every contraction workgroup forms its sample's theta itself (the same sums in the
  // same order, into its own 16 doubles of theta_scr [S x NC x 16], which its scalar loads then read), workgroup 0 also writes
  // theta_out [S x P] for the kernels behind
  const double* Sop = nullptr; int P = 0; double* theta_scr = nullptr; double* theta_out = nullptr;
  // finrom_hmc_leapfrog: the position update rides in front -- every reader of the field sees k + eps * mom, and the network's
  // workgroup (which reads all of it anyway) writes the moved field to k_out (NOT in place: the sample's other workgroups read k)
  const double* mom = nullptr; double eps = 0.0; double* k_out = nullptr;
  // round 4: the first layer over nw0 spare workgroups (partial sums y0_part [S x nw0 x 64] floats), the layers behind it as a
  // spare wave of the solve kernel (rom_onesample.hip)
  int nw0 = 4; float* y0_part = nullptr;
  // finrom_hmc_leapfrog, steps behind the first of a trajectory: theta = S (k + eps mom) arrives as HMC_THETA_PARTS partial sums
  // [S x HMC_THETA_PARTS x 16] left by the previous step's momentum update (which forms the new momentum anyway) -- the 4.6 us theta
  // phase at the head of every contraction workgroup becomes one load of 8 x P doubles
  const double* theta_parts = nullptr;
};
// The one-sample form's spare wave (mlp_forward_tail_wave<true>, mlp_device.h) reads the hidden layers' and the head's weights from
// MLP_STAGE_FLOATS floats of LDS -- the weights, zeros behind them -- and ALL 64 lanes run every layer's loop over 64 inputs
// unguarded: lane t reads [l n_w^2 + t + i n_w] for i < 64 in hidden layer l and [L n_w^2 + t + i n_out] in the head.
// mlp_stage_reach: one past the furthest of those indices.  The staged wave is taken only where that lies inside the zero-filled
// region (the weights' own count, L n_w^2 + n_w n_out, is never larger): e.g. 12 layers of 36 units are 15 876 floats of weights
// but lane 63 of layer 11 reads index 16 587 -- past the staged floats and past the kernel's LDS -- so they take the unstaged wave.
constexpr int MLP_STAGE_FLOATS = 16 * 256 * 4;      // what 256 threads stage with 16 four-float loads each: 64 KB (5 x 50 x 50 + 50 x 9 = 12 950 floats fit)
__host__ __device__ inline int mlp_stage_reach(int n_layers, int n_w, int n_out) {
  const int nh = n_layers * n_w * n_w;
  const int hid = n_layers > 0 ? nh - n_w * n_w + 63 * n_w + 63 : -1, head = nh + 63 * n_out + 63;
  return (hid > head ? hid : head) + 1;
}
__host__ __device__ inline bool mlp_tail_staged(int n_layers, int n_w, int n_out) {      // (& 3: the hidden weights are staged as four-float loads)
  return mlp_stage_reach(n_layers, n_w, n_out) <= MLP_STAGE_FLOATS && ((n_layers * n_w * n_w) & 3) == 0;
}
// mlp_forward_kernel keeps its input in dynamic LDS beside mlp_forward_body<1024>'s static arrays (part [16][64] + y, a [64] floats,
// tred [16] doubles = 4736 bytes) under the 64 KB a kernel may use without asking for more: inputs beyond this are refused by
// launch_mlp_forward (FINROM_ERR_UNSUPPORTED), not left to fail at launch.  The largest mesh with a band plan (m = 28) has 7 757 nodes.
constexpr int MLP_FORWARD_STATIC_LDS = (16 * 64 + 2 * 64) * 4 + 16 * 8;
constexpr int MLP_FORWARD_MAX_IN = (64 * 1024 - MLP_FORWARD_STATIC_LDS) / 4;      // 15 200
constexpr int HMC_THETA_PARTS = 8;      // = mlp_kernels.hip's MLP_SPLIT: one partial sum per workgroup of the backward kernel
constexpr int HMC_THETA_MAXP = 10;      // averages the carry handles (the fin has nine); beyond: every step forms theta itself
// finrom_hmc_leapfrog: the momentum update rides behind the gradient (mlp_backward_kernel's epilogue):
//   dU = (kq - mean) + coef * grad  (0 for a flagged sample);  mom -= eps_cpri * dU
struct HmcTail {
  int on = 0;
  const double* kq = nullptr; const double* mean = nullptr; double* mom = nullptr; double* dU = nullptr;
  double coef = 0.0, eps_cpri = 0.0; const int* info = nullptr;
  // the NEXT step's sub-fin averages while the new momentum is at hand: theta_parts[s][wg][p] = sum over this workgroup's rows of
  // Sop[p][i] (kq[i] + eps mom_new[i]); nullptr: not wanted
  double eps = 0.0; double* theta_parts = nullptr;
};
int launch_mlp_forward(const MlpDev& m, const double* k, int64_t S, const double* data, int64_t data_stride, float* tape,
                       double* e_out, double* data_shift, hipStream_t st, const double* Sop = nullptr, int P = 0,
                       double* theta_out = nullptr);
int mlp_forward_fits(const MlpDev& m);      // 0, or FINROM_ERR_UNSUPPORTED with the error text set (n_in > MLP_FORWARD_MAX_IN)
// (g_parts, n_parts: instead of g_theta, its n_parts partial sums [S x n_parts x 32] as rom_grad_contract_small_kernel leaves them)
int launch_mlp_backward(const MlpDev& m, int64_t S, const float* tape, const double* data, int64_t data_stride, const double* qoi_r,
                        const double* e_nn, const double* g_theta, const double* Sop, int P, double* grad, hipStream_t st,
                        const double* g_parts = nullptr, int n_parts = 0, const float* g0_in = nullptr, const HmcTail* tail = nullptr);
// (g0_in [S x 64]: the walk back through the head and the hidden layers has been done -- MlpBackFuse -- and left its result there)
struct MlpBackFuse {             // that walk as one more workgroup per sample of rom_grad_contract_small_kernel
  int on = 0;
  MlpDev m{};
  const float* tape = nullptr; const double* data = nullptr; int64_t data_stride = 0;
  const double* qoi_r = nullptr; const double* e_nn = nullptr; float* g0_out = nullptr;
};

// ---- HMC trajectory bookkeeping (hmc_kernels.hip, finrom_hmc_*) ------------------------------------
struct HmcDev {                  // finrom_hmc_state with the host-side fields resolved
  int64_t C; int n;
  double eps, c_lik, c_pri;
  const double* mean; double* K; double* U; double* dU;
  double* Kq0; double* P; double* dUq; double* H0;
  const double* P_block; const double* lu_block;
  long long* jt; long long* pt; long long* accept;
  double* trace; const double* loss; const int* info;
};
int launch_hmc_begin(const HmcDev& h, hipStream_t st);
int launch_hmc_end(const HmcDev& h, const double* Kq, hipStream_t st);
int launch_hmc_stats(const finrom_hmc_stats& s, hipStream_t st);      // hmc_stats.hip (the descriptor holds device pointers only)
// delayed acceptance: finrom_hmc_end cut into its decision (hmc_kernels.hip) and, behind a full-order solve, the second test and
// the commit (hmc_da.hip; the descriptor holds device pointers only)
int launch_hmc_end_stage1(const HmcDev& h, const double* Kq, int* ok1, double* Uq, hipStream_t st);
int launch_hmc_end_stage2(const HmcDev& h, const double* Kq, const finrom_hmc_da& da, hipStream_t st);
// hmc_model.hip (finrom_hmc_drift / _kick): the model-agnostic halves of a leapfrog step.  A [P x n] (optional, P <= HMC_MODEL_MAXP):
// drift: k_out = k + eps h.P and theta_out [C x P] = theta0 + A k_out;  kick: the gradient at kq is grad [C x n] or A^T g_theta,
// then h.dUq and h.P as HmcTail states them (flagged chains: dUq 0, momentum untouched); grad_out (optional): the gradient itself
constexpr int HMC_MODEL_MAXP = 16;
int launch_hmc_drift(const HmcDev& h, const double* k, double* k_out, const double* A, const double* theta0, int P, double* theta_out,
                     hipStream_t st);
int launch_hmc_kick(const HmcDev& h, const double* kq, const double* grad, const double* g_theta, const double* A, int P,
                    double* grad_out, hipStream_t st);

// hmc_nuts_model.hip (finrom_hmc_nuts_begin / _leaf / _end): the No-U-turn transition one leaf per launch, the tree's state in the
// caller's workspace.  ws: NUTS_TREE_FIXED_ARRAYS + 2 max_depth arrays [C x n]; behind them scal [C x NUTS_TREE_SCALARS] doubles and
// ints [C x NUTS_TREE_INTS] (hmc_nuts_tree_ws_bytes); st_loss [C]: the state's misfit; active [C]; tree, accept_stat: optional.
// NutsMap: the optional map of finrom_hmc_drift (A NULL: none; P <= HMC_MODEL_MAXP).
constexpr int NUTS_TREE_FIXED_ARRAYS = 13;
constexpr int NUTS_TREE_SCALARS = 8;
constexpr int NUTS_TREE_INTS = 8;
struct NutsTreeDev {
  int max_depth; long long proposal0;
  const unsigned long long* seeds;
  double* ws; double* scal; int* ints;
  double* st_loss; int* tree; double* accept_stat; int* active;
  const double* eps_c = nullptr;         // [C], optional: each chain's own step in the place of HmcDev::eps (begin and leaf)
};
// finrom_hmc_step_adapt_update: finrom_hmc_step_adapt with the call's own arguments beside it
struct StepAdaptDev {
  double* eps; double* hbar; double* xbar;
  double mu, target, gamma, t0; long long tune;
  int64_t C; long long proposal0; const long long* pt; const double* accept_stat; double* step_size;
};
int launch_hmc_step_adapt(const StepAdaptDev& ad, hipStream_t st);
struct NutsMap { const double* A; const double* theta0; int P; double* theta_out; };
int64_t hmc_nuts_tree_ws_bytes(int64_t C, int n, int max_depth);
int launch_hmc_nuts_begin(const HmcDev& h, const NutsTreeDev& a, const NutsMap& tm, hipStream_t st);
int launch_hmc_nuts_leaf(const HmcDev& h, const NutsTreeDev& a, const double* grad, const double* g_theta, const NutsMap& tm, hipStream_t st);
int launch_hmc_nuts_end(const HmcDev& h, const NutsTreeDev& a, hipStream_t st);

// ---- low-rank metric M = I + V diag(lambda) V^T (hmc_metric.hip, finrom_metric_*, finrom_hmc_*_metric) -----------------------
constexpr int METRIC_MAX_RHO = 64;
// rows of MetricDev::coef: the c_j of y = x + sum_j c_j V_j (V_j . x) for the four maps (finrom.h's FINROM_METRIC_* codes), then
// d_j = lambda_j / (1 + lambda_j) of the kinetic energy
enum { METRIC_OP_M = 0, METRIC_OP_INV = 1, METRIC_OP_SQRT = 2, METRIC_OP_INVSQRT = 3, METRIC_OP_D = 4, METRIC_NUM_COEF = 5 };
struct MetricDev {
  int n = 0, rho = 0;
  const double* Vt = nullptr;            // [rho x n] orthonormal rows
  const double* coef = nullptr;          // [METRIC_NUM_COEF x METRIC_MAX_RHO]
};
int launch_metric_apply(const MetricDev& m, int op, const double* x, int64_t S, double* y, double* quad, hipStream_t st);
int launch_hmc_velocity(const MetricDev& m, const double* P, int64_t C, double* Q, hipStream_t st);
int launch_hmc_begin_metric(const HmcDev& h, const MetricDev& m, hipStream_t st);
int launch_hmc_end_metric(const HmcDev& h, const MetricDev& m, const double* Kq, hipStream_t st);

// ---- batched multi-start L-BFGS bookkeeping (lbfgs_kernels.hip, finrom_lbfgs_*) ------------------------------------------
struct LbfgsDev {                // finrom_lbfgs_state, validated
  int64_t S; int d, m, maxls, gdim;
  double ftol, gtol, gamma; long long maxiter, maxfun;
  const double* lo; const double* hi;
  double* x; double* f; double* g; double* xt; double* work;
  int* status; long long* nit; long long* nfev; double* fhist; long long fhist_rows;
  const double* G;
  const int* k1_ptr; const int* k1_idx; const double* k1_val;
};
constexpr int LBFGS_MAX_M = 16;
constexpr int LBFGS_MAX_E = 17;          // elements per thread in registers: d <= 17 * 256 = 4352 (the m = 20 field mesh has 4101)
constexpr int LBFGS_MAX_GDIM = 16;
__host__ __device__ inline int64_t lbfgs_work_stride(int d, int m) { return (2 * (int64_t)m + 1) * d + 2 * (int64_t)m + 8; }
int launch_lbfgs_begin(const LbfgsDev& L, hipStream_t st);
int launch_lbfgs_propose(const LbfgsDev& L, hipStream_t st);
int launch_lbfgs_accept(const LbfgsDev& L, const double* f_in, const double* g_in, const int* info, hipStream_t st);

// ---- latent Gaussian-field prior (field_prior.hip, finrom_sampler_field / _pullback / finrom_hmc_leapfrog_field) --------------
// the pullback's epilogue in a whitened leapfrog step (c_pri = 1):  dU = vq + c_lik g_v (0 for a flagged sample);  mom -= eps dU
struct FieldPriorTail {
  const double* vq = nullptr; double c_lik = 0.0; const int* info = nullptr; double* mom = nullptr; double* dU = nullptr;
  double eps = 0.0;
};
size_t field_prior_part_bytes(int n, int64_t S);     // the partial-sum workspace of a call with S rows
size_t field_prior_tick_bytes(int n);                // its arrival counters (zero between calls)
// pull = 0: out = mean + U^T (x + eps p) (mean, p optional; v_out = x + eps p optional);  pull = 1: out = U x (out optional), tail
int launch_field_prior(const double* U, int n, int pull, const double* x, const double* p, double eps, const double* mean,
                       double* out, double* v_out, const FieldPriorTail* tail, int64_t S, double* part, int* tick, hipStream_t st);

// ---- ROM ------------------------------------------------------------------------------
struct RomDev {
  int n, r, rp, NB, P, n_obs;           // rp = 16*NB padded basis size
  int solve_in_lds;                     // packed factor fits in LDS (rp <= 176)
  long long* trace;                     // FINROM_TRACE (see FomDev::trace)
  // psi tables, rows grouped 4 per k-step so that the four rows of a k-step share ONE list of theta indices
  // (rows with the same term pattern together; leftovers merged under the union of their patterns, absent terms = zero
  // rows): theta then comes from SGPRs, and the k-step needs no theta-index loads, no LDS reads and no per-lane addresses
  const double* tvu;                    // [(nuslots + 4) * 4 * rp]
  int tvu_bytes;
  int nku;                              // number of pattern-uniform k-steps (even; sorted by term count, descending; every
                                        // term-count group holds an even number of k-steps, padded with a zero k-step)
  int uend[4];                          // uend[t] = number of k-steps with more than t terms (uend[0] = nku)
  const int* kmeta;                     // [(nku + 8) * 8] per k-step: first slot, term count, 2 x padding, theta indices of its 4 slots
  // the pattern-uniform k-steps grouped by their leading parameter and accumulated divided by it (proj_main_grouped; built in
  // finrom_rom_create, where the form is described): records {first slot, terms, flags (1: the first coefficient is 1, 2: rescale
  // the accumulators first), ext index of that factor, ext indices of the coefficients}
  const double* tvg; int tvg_bytes;
  const int* kmg;                       // [(nkg + 8) * 8]
  int nkg;                              // multiple of 3; 0: no grouped form (nothing to group, too many parameters, NB > 5)
  int n_ext, ext_final;                 // per-sample scalars (<= 64); ext index of the factor behind the last k-step
  const int* ext_def;                   // [n_ext * 3] ext[l] = (theta'[a] / theta'[b]) ^ (1 + (f & 1)) * (f & 2 ? 2 : 1), theta'[0] = 1
  double* ext;                          // [S x n_ext] workspace of the CALL (set by rom_project; nullptr: the ungrouped loop)
  // the HALF list of a mirror-symmetric ROM (finrom_rom_set_mirror, DESIGN 4b'): a second record list in the same format over the
  // left and centre-line rows of the symmetrised basis.  Its records sit behind the full list's in kmg (kmg_m ints in), its rows
  // behind the full table's in tvg, its factors behind the full list's in ext_def / the sample's row of ext; a sample whose
  // parameters equal their twins' (twin, 0-based) walks it instead of the full list.
  int nkg_m;                            // multiple of 3; 0: no half list (on this handle, or in this call)
  int kmg_m, ext_final_m;
  const int* twin;                      // [P]
  // the SHORT half list (finrom_rom_set_mirror_short, DESIGN 4b''): a third list, the half list without the rows that are zero up
  // to rounding, behind the half list in the same arrays; a mirror-symmetric sample walks it instead of the half list when every
  // parameter lies in [short_lo, short_hi], the range over which the caller's gate measured what leaving those rows out costs
  int nkg_s;                            // multiple of 3; 0: no short list (on this handle, or in this call)
  int kmg_s, ext_final_s;
  double short_lo, short_hi;
  // rows with a non-zero load F (root nodes): slot-major padded r-vectors (4 per slot) with the theta index of each
  // (0 = the constant 1), a runtime term count
  int rhs_nk, rhs_nt;
  const double* rhs_tv; const int* rhs_pidx; const double* rhs_f;
  const double* obs_phi;                // [n_obs x r]
};
struct RomGradArgs {                      // adjoint-gradient stage of rom_solve_kernel (finrom_rom_grad)
  const double* data = nullptr; int64_t data_stride = 0;    // observations [n_obs] (stride 0) or [S x n_obs]
  const double* theta = nullptr;                            // [S x P]
  double* J = nullptr; double* g = nullptr;                 // [S], [S x P]
  int npairs = 0; const int* pair_p = nullptr; const int* pair_i = nullptr; const double* Gt = nullptr;
  double* gpart = nullptr; int* ticket = nullptr;   // small batches (rom_grad_contract_small_kernel): [S x NG x 32] partial sums, [S] arrival counters (zero between calls)
  int defer_sum = 0;        // (small batches) leave the NG partial sums in gpart: the consumer adds them (mlp_backward_kernel in finrom_romml_grad)
  int info_store = 0;       // (one-sample solve kernel) info[s] is stored (0 or 2), not or-ed into: the caller did not have to clear it
  double* vw = nullptr;     // scratch [S x 2 rp]: when set, the substitution kernel leaves v_r and w_r there and the
                            // contraction g_i = sum_p theta_p v_r^T G_pi w_r runs in rom_grad_contract_kernel (fp64 MFMA, 16 samples per wave)
};
// offline/online form of the reduced operator (finrom_rom_set_gram, rom_gram.hip)
constexpr int ROM_GRAM_MAX_PAIRS = 64;
struct RomGramDev {
  int npairs = 0;
  const int* pair_p = nullptr; const int* pair_q = nullptr;   // [npairs], 0 = the constant term
  const double* Gt = nullptr;     // [npairs][NB(NB+1)/2][64][4]  tiles in the MFMA C/D register layout (r <= 96)
  const double* Gp = nullptr;     // [npairs][rp(rp+1)/2]         packed upper triangle, row by row (r > 96)
  const double* h = nullptr;      // [P+1][rp]                    h_p = Psi_p^T F
};
int launch_rom_gram(const RomDev& p, const RomGramDev& gm, const double* theta, int64_t S, double* Ar, double* Br, int factor,
                    int* info, hipStream_t st, double* w_r = nullptr, double* qoi_r = nullptr);
int launch_rom_grad(const RomDev& p, const double* Ar, const double* Br, int64_t S, double* w_r, double* qoi_r,
                    int* info, const RomGradArgs& ga, hipStream_t st);
int launch_rom_grad_contract(const RomDev& p, int64_t S, const RomGradArgs& ga, hipStream_t st);
int launch_rom_chol_blocked(const RomDev& p, double* Ar, int64_t S, int* info, hipStream_t st);
int launch_rom_proj(const RomDev& p, const double* theta, int64_t S, double* Ar, double* Br, int factor, int* info, hipStream_t st,
                    double* w_r = nullptr, double* qoi_r = nullptr, bool roomy = false, bool short_waits = false, bool block_row = false);
constexpr unsigned ROM_BLOCK_ROW_NB_MASK = 1u << 5;      // basis widths in 16-column blocks at which the block-row epilogue is the pair path's default
bool rom_roomy_applies(const RomDev& p, int factor, const double* w_r, const double* qoi_r);
constexpr int ROM_SPLITK_MAX_S = 64;      // batches up to this size take the split-K projection kernel (r = 49..96)
// (r mod 16 in 1..8, NB >= 7: the HalfCover form of the multi-wave kernels, rom_proj_half.hip)
int launch_rom_proj_half(const RomDev& p, const double* theta, int64_t S, double* Ar, double* Br, int factor, int* info,
                         hipStream_t st, double* w_r, double* qoi_r);
int launch_rom_proj_wide(const RomDev& p, const double* theta, int64_t S, double* Ar, double* Br, int factor, int* info,
                         hipStream_t st, double* w_r, double* qoi_r);
bool rom_splitk_applies(const RomDev& p, int64_t S);
// one-sample call patterns (rom_onesample.hip): contraction over several workgroups per sample + MFMA-form solve kernel
bool rom_onesample_applies(const RomDev& p, int64_t S);
size_t rom_onesample_scratch_bytes(const RomDev& p, int64_t S);
int launch_rom_onesample(const RomDev& p, const double* theta, int64_t S, double* part, int grad, const RomGradArgs& ga, double* w_r,
                         double* qoi_r, int* info, hipStream_t st, const MlpFuse* fuse = nullptr);
constexpr int ROM_GRAD_SMALL_NG = 36;      // blocks per sample in rom_grad_contract_small_kernel
int launch_rom_grad_contract_small(const RomDev& p, int64_t S, const RomGradArgs& ga, hipStream_t st, const MlpBackFuse* bf = nullptr);
int launch_rom_proj_splitk(const RomDev& p, const double* theta, int64_t S, double* Ar, double* Br, int factor, int* info,
                           hipStream_t st, double* w_r, double* qoi_r, const RomGradArgs& ga);
int launch_rom_proj_single(const RomDev& p, const double* theta, int64_t S, double* Ar, double* Br, int factor, int* info,
                           hipStream_t st, double* w_r, double* qoi_r, bool roomy = false, bool short_waits = false, bool block_row = false);
int launch_rom_solve(const RomDev& p, const double* Ar, const double* Br, int64_t S, double* w_r,
                     double* qoi_r, double* Ar_out, double* Br_out, int* info, int factored, hipStream_t st);

}  // namespace finrom
