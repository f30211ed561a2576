// The network as a model of its own (mlp_surrogate.hip, finrom_mlp_misfit_grad): value and gradient of 1/2 |data - NN(k)|^2.
// Included by mlp_surrogate.hip and the host layer only: a change here rebuilds neither the reduced model's nor the FOM's units.
#pragma once
#include "finrom_internal.h"

namespace finrom {

// the tile form's zero-padded copies of the weights (width 64, n_in to a multiple of SUR_KC): one allocation on the handle
constexpr int SUR_KC = 64;          // inputs per chunk of the streamed first layer (and of its transpose)
constexpr int SUR_ROWS = 64;        // samples per workgroup: four waves of 16 rows
struct SurPad {
  int n_inp = 0;                     // n_in rounded up to a multiple of SUR_KC
  const float* W0p = nullptr;        // [n_inp][64]
  const float* b0p = nullptr;        // [64]
  const float* scp = nullptr; const float* shp = nullptr;      // [(L + 1)][64]
  const float* Wp = nullptr;  const float* WpT = nullptr;      // [L][64][64]: W_l[i][j] and its transpose
  const float* bp = nullptr;         // [L][64]
  const float* Whp = nullptr; const float* WhpT = nullptr;     // [64][64]: Wh[i][o] and its transpose
  const float* bhp = nullptr;        // [64]
};
inline int sur_n_inp(int n_in) { return (n_in + SUR_KC - 1) / SUR_KC * SUR_KC; }
size_t sur_pad_floats(const MlpDev& m);
// fills buf (sur_pad_floats(m) floats) from the handle's weights and points *p into it
int launch_sur_pad(const MlpDev& m, float* buf, SurPad* p, hipStream_t st);

// per-sample form: one 1024-thread workgroup per sample (mlp_forward_body), then the walk back and the first layer's transpose.
// loss (with data) and tape are optional outputs of the forward launch; out [S x n_out] is required
int launch_sur_forward(const MlpDev& m, const double* k, int64_t S, const double* data, int64_t data_stride, float* tape, double* out,
                       double* loss, hipStream_t st);
int launch_sur_backward(const MlpDev& m, int64_t S, const float* tape, const double* data, int64_t data_stride, const double* zero,
                        const double* out, double* grad, hipStream_t st);
// tile form: SUR_ROWS samples per workgroup, the first layer and its transpose on the fp32 matrix cores.  bad [S]: 1 where the row
// has a non-finite input (written by the forward launch, read by the backward one)
int launch_sur_tile_forward(const MlpDev& m, const SurPad& p, const double* k, int64_t S, const double* data, int64_t data_stride,
                            float* tape, double* out, double* loss, int* bad, hipStream_t st);
int launch_sur_tile_backward(const MlpDev& m, const SurPad& p, int64_t S, const float* tape, const double* data, int64_t data_stride,
                             const double* out, const int* bad, double* grad, hipStream_t st);

// hmc_ml.hip (finrom_hmc_leapfrog_ml / finrom_hmc_trajectory_ml): the chains under this model, one 1024-thread workgroup per chain.
// forward: k_out = fma(h.eps, h.P, k), the network and the misfit at k_out (tape, out, loss), info = 1 where the loss is not finite
// else 0 -- the step form's first launch, launch_sur_backward and launch_hmc_kick behind it.  trajectory: n_steps such steps in one
// launch from kq0 (step s reads kq[s & 1] and writes kq[(s + 1) & 1]), the kick on h.P and h.dUq included; zero: [C x n_out] zeros
int launch_hmc_ml_forward(const MlpDev& m, const HmcDev& h, const double* k, double* k_out, const double* data, int64_t data_stride,
                          float* tape, double* out, double* loss, int* info, hipStream_t st);
int launch_hmc_ml_trajectory(const MlpDev& m, const HmcDev& h, int n_steps, double* kq0, double* kq1, const double* data,
                             int64_t data_stride, const double* zero, float* tape, double* out, double* loss, int* info, hipStream_t st);

// hmc_nuts.hip (finrom_hmc_nuts_ml): one No-U-turn transition of every chain in one launch, one 1024-thread workgroup per chain, then
// the counters' advance.  ws: NUTS_ARRAYS arrays [C x n] (hmc_nuts_ws_doubles), wloss [C] / winfo [C]: a leaf's misfit and flag; scal [C x NUTS_SCALARS];
// st_loss [C]: the state's misfit (written where a candidate is adopted); tree [rows x C x 4], accept_stat [rows x C]: optional;
// eps_c [C]: optional, each chain's own step in the place of HmcDev::eps (finrom_hmc_nuts_ml_adapt; NULL: the state's step)
constexpr int NUTS_MAX_DEPTH = 10;
constexpr int NUTS_ARRAYS = 15 + 2 * NUTS_MAX_DEPTH;
constexpr int NUTS_SCALARS = 8;      // per chain, thread 0's: H0, W, W_sub, the sum of min(1, w), the sub-tree candidate's U and misfit, u_top
struct NutsDev {
  int max_depth; long long proposal0;
  const unsigned long long* seeds;
  double* ws; double* wloss; int* winfo; double* scal; double* st_loss;
  int* tree; double* accept_stat;
  const double* eps_c = nullptr;
};
int64_t hmc_nuts_ws_doubles(int64_t C, int n);
int launch_hmc_nuts_ml(const MlpDev& m, const HmcDev& h, const NutsDev& a, const double* data, int64_t data_stride, const double* zero,
                       float* tape, double* out, hipStream_t st);
// finrom_hmc_nuts_ml_metric: the same transition under the metric M (P_block: standard normals).  ws: hmc_nuts_metric_ws_doubles -- the
// identity launch's arrays and behind them the velocities' (both edges, the walker's two, one per checkpoint)
int64_t hmc_nuts_metric_ws_doubles(int64_t C, int n);
int launch_hmc_nuts_ml_metric(const MlpDev& m, const HmcDev& h, const NutsDev& a, const MetricDev& mt, const double* data,
                              int64_t data_stride, const double* zero, float* tape, double* out, hipStream_t st);

}  // namespace finrom
