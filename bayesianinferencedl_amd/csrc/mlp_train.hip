// Training the learned error model on the device (finrom_mlp_train_*): what Keras does in the reference's run
// (deep_learning/dl_model.py:163-176 the model, :230-243 model.fit), restated for gfx950 in fp32.
//     y0 = x W0 + b0;   y_{l+1} = y_l + elu(bn_l(y_l)) W_l + b_l  (l < L);   out = elu(bn_L(y_L)) W_h + b_h
// bn in training form (batch mean, biased batch variance, eps 1e-3), loss = MSE + l1_l2(1e-4, 1e-4) on W0 and the units' W,
// Adam in Keras 1.x form.  The host statement is deep_learning/dl_model.py::ResBnFcModel.fit_host.
//
// Layout: every width (n_w, n_out) is padded to 64 on the device -- parameters, gradients, Adam's m and v live in ONE flat padded
// array each:  W0 [n_in][64] | b0 [64] | per layer l = 0 .. L (L: the head)  gamma [64] | beta [64] | W [64][64] | b [64].
// Padding is zero and stays zero: a padded column has y = 0, z = 0, elu(0) = 0, every gradient 0, and Adam moves a parameter with
// m = v = g = 0 by 0 / 1e-7 = 0.  The C ABI packs / unpacks the unpadded layout of ResBnFcModel.
//
// A step is a linear chain of launches on one stream (2 L + 10 of them), no allocation, no host synchronisation, no atomics:
//   reg_kernel            sum |w|, sum w^2 of the regularised matrices: 64 slices, each a fixed-order workgroup reduction
//   fwd0_kernel           X_b W0 on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: an exact k-ordered fma chain), the K dimension
//                         in TRAIN_KS fixed pieces -> partial sums; a wave = 16 batch rows x 64 columns x one K piece
//   y0_finish_kernel      y0 = b0 + the pieces in index order; per tile of 32 rows the column mean and M2
//   layer_fwd_kernel x (L + 1)   every workgroup combines the tiles' (mean, M2) in index order (Chan's update: one pass, no
//                         E[y^2] - mean^2 cancellation) -- the whole-batch statistic is finished "by the next launch", nobody
//                         waits for anybody --, normalises its 32 rows, elu, the 64 x 64 product from LDS, the next y and its
//                         tile statistics; the head: residual, d loss / d out, the tile's loss and MAPE sums
//   layer_bwd_kernel x (L + 1)   prologue: the gradient wrt y_{l+1} from the level above (its batch-norm backward needs two
//                         whole-batch sums, again finished by this launch from per-tile partials); then g W^T, elu', the tile's
//                         partial d gamma, d beta, d b, and a^T g (64 x 64 per tile)
//   gy0_kernel            the same prologue for y0, partial sums of d b0
//   dw0_kernel            X_b^T G0 on the matrix cores: a wave = 16 inputs x 16 columns over the whole batch in row order, plus
//                         the regulariser's gradient
//   grad_finish_kernel    the tiles' partial sums in index order -> d W, d b; the loss and MAPE of the step
//   adam_kernel, step_tail_kernel   Adam on the flat array; moving statistics, t += 1, the epoch's running sums
// Tile sums, statistics, the loss and the across-tile sums are carried in double (a few thousand additions per step): they add
// no rounding of their own to the fp32 products.  Buffers that one launch reads from ALL tiles while writing its own tile's
// entry for the next launch (tile statistics, d gamma / d beta partials) are double-buffered by layer parity.
#include "mlp_device.h"
#include "block_reduce.h"

#include <cmath>
#include <cstring>

namespace finrom {

constexpr int TW = 64;               // padded width
constexpr int TR = 32;               // batch rows per tile (workgroup) in the trunk
constexpr int TRAIN_KS = 8;          // K pieces of the first layer's forward product
constexpr int TRAIN_NREG = 64;       // slices of the regulariser's sums
constexpr int TRAIN_MAX_L = 8;
constexpr float BN_EPS_F = 1e-3f;
constexpr float REG_F = 1e-4f, REG2_F = 2e-4f;
constexpr int LAYER_STRIDE = 3 * TW + TW * TW;      // gamma | beta | W | b
enum { SC_LOSS = 0, SC_MAPE, SC_LR, SC_SUM_LOSS, SC_SUM_MAPE, SC_SUM_ROWS, SC_SUM_MSE, SC_B, SC_MSE, SC_EVAL_SQ, SC_EVAL_APE, SC_NUM };

struct TrainDev {
  int n_in, nw, L, n_out, max_batch, max_tiles;
  int64_t npad;
  float* P; float* M; float* V; float* G;
  float* mov;          // [(L + 1)][2][64] moving mean | variance
  double* bstat;       // [(L + 1)][2][64] batch mean | biased variance of the last step
  float* Y;            // [(L + 1)][max_batch][64] tape: y_l
  float* part0;        // [TRAIN_KS][max_batch][64]
  float* Gy; float* Gz;   // [max_batch][64]
  double* tstat;       // [2][max_tiles][2][64] tile mean | M2, by layer parity
  double* tsum;        // [2][max_tiles][2][64] tile sums of g_z | g_z xhat, by layer parity
  float* dWpart;       // [(L + 1)][max_tiles][64 x 64]
  double* dbpart;      // [(L + 2)][max_tiles][64]   (slot L + 1: b0)
  double* lpart;       // [max_tiles][2]
  double* regpart;     // [TRAIN_NREG][2]
  double* scal;        // [SC_NUM]
  long long* t;
  __host__ __device__ int64_t o_b0() const { return (int64_t)n_in * TW; }
  __host__ __device__ int64_t o_layer(int l) const { return (int64_t)n_in * TW + TW + (int64_t)l * LAYER_STRIDE; }
  __host__ __device__ int64_t o_gamma(int l) const { return o_layer(l); }
  __host__ __device__ int64_t o_beta(int l) const { return o_layer(l) + TW; }
  __host__ __device__ int64_t o_W(int l) const { return o_layer(l) + 2 * TW; }
  __host__ __device__ int64_t o_b(int l) const { return o_layer(l) + 2 * TW + TW * TW; }
};

typedef float f4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int64_t row_of(const int32_t* __restrict__ rows, int64_t base, int i) {
  return rows != nullptr ? (int64_t)rows[i] : base + i;
}

// ---- regulariser: sum |w| and sum w^2 over W0 and the units' W ---------------------------------------------------------------
__global__ __launch_bounds__(256) void reg_kernel(TrainDev d) {
  __shared__ double red[8];
  const int64_t n0 = (int64_t)d.n_in * TW, N = n0 + (int64_t)d.L * TW * TW;
  const int64_t i0 = N * blockIdx.x / TRAIN_NREG, i1 = N * (blockIdx.x + 1) / TRAIN_NREG;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    int64_t off = i;
    if (i >= n0) { const int64_t q = i - n0; off = d.o_W((int)(q / (TW * TW))) + q % (TW * TW); }
    const double w = (double)d.P[off];
    s1 += fabs(w); s2 += w * w;
  }
  block_sum2_256(s1, s2, red);
  if (threadIdx.x == 0) { d.regpart[blockIdx.x * 2] = s1; d.regpart[blockIdx.x * 2 + 1] = s2; }
}

// ---- first layer forward: part0[kp][r][:] = sum over K piece kp of X[row r][k] W0[k][:] ---------------------------------------
__global__ __launch_bounds__(256) void fwd0_kernel(TrainDev d, const float* __restrict__ X, const int32_t* __restrict__ rows,
                                                   int64_t base, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kp = blockIdx.y * 4 + wave;
  const int r0 = blockIdx.x * 16;
  const int li = lane & 15, g = lane >> 4;
  const int rr = r0 + li < B ? r0 + li : B - 1;                 // (rows beyond the batch: a valid row, not stored)
  const float* __restrict__ xrow = X + row_of(rows, base, rr) * d.n_in;
  const int nsteps = (d.n_in + 3) / 4;
  const int s0 = (int)((int64_t)nsteps * kp / TRAIN_KS), s1 = (int)((int64_t)nsteps * (kp + 1) / TRAIN_KS);
  f4_t acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f4_t{0.f, 0.f, 0.f, 0.f};
  constexpr int U = 4;
  for (int s = s0; s < s1; s += U) {
    float a[U], b[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = 4 * (s + u) + g;
      const bool ok = s + u < s1 && k < d.n_in;
      a[u] = ok ? xrow[k] : 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) b[u][c] = ok ? d.P[(int64_t)k * TW + c * 16 + li] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s + u < s1) {                                        // (uniform over the wave)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u][c], acc[c], 0, 0, 0);
      }
    }
  }
  float* __restrict__ out = d.part0 + (int64_t)kp * d.max_batch * TW;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + 4 * g + r;
    if (row < B) {
#pragma unroll
      for (int c = 0; c < 4; ++c) out[(int64_t)row * TW + c * 16 + li] = acc[c][r];
    }
  }
}

// the tile's column mean and M2 = sum (y - mean)^2 over its nv valid rows (threads 0 .. 63, rows in order)
__device__ __forceinline__ void tile_stats(const float (*T)[TW], int nv, double* __restrict__ out) {
  const int c = threadIdx.x;
  if (c < TW) {
    double s = 0.0;
    for (int r = 0; r < nv; ++r) s += (double)T[r][c];
    const double mean = s / nv;
    double m2 = 0.0;
    for (int r = 0; r < nv; ++r) { const double e = (double)T[r][c] - mean; m2 += e * e; }
    out[c] = mean; out[TW + c] = m2;
  }
}

__global__ __launch_bounds__(256) void y0_finish_kernel(TrainDev d, int B, int train) {
  __shared__ float T[TR][TW];
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6, tile = blockIdx.x;
  const float b0 = d.P[d.o_b0() + c];
#pragma unroll
  for (int r = 0; r < TR / 4; ++r) {
    const int rl = rg * (TR / 4) + r, row = tile * TR + rl;
    float y = 0.f;
    if (row < B) {
      float t = 0.f;
#pragma unroll
      for (int kp = 0; kp < TRAIN_KS; ++kp) t += d.part0[((int64_t)kp * d.max_batch + row) * TW + c];
      y = t + b0;
      d.Y[(int64_t)row * TW + c] = y;
    }
    T[rl][c] = y;
  }
  __syncthreads();
  if (train) tile_stats(T, min(TR, B - tile * TR), d.tstat + (int64_t)tile * 2 * TW);
}

// mean and 1 / sqrt(var + eps) of layer l as EVERY kernel forms them from the stored statistics (the same bits everywhere)
__device__ __forceinline__ void bn_coef(const TrainDev& d, int l, int c, float& mean, float& rstd) {
  mean = (float)d.bstat[(l * 2) * TW + c];
  rstd = 1.0f / sqrtf((float)d.bstat[(l * 2 + 1) * TW + c] + BN_EPS_F);
}

// ---- one layer forward over a tile of TR rows --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void layer_fwd_kernel(TrainDev d, int l, int B, int train, const float* __restrict__ Yt,
                                                        const int32_t* __restrict__ rows, int64_t base) {
  __shared__ __attribute__((aligned(16))) float Ws[TW][TW];
  __shared__ float As[TR][TW];
  __shared__ float smean[TW], srstd[TW];
  __shared__ double lred[2][TW];
  const int tid = threadIdx.x, c = tid & 63, rg = tid >> 6, tile = blockIdx.x;
  const int nt = (B + TR - 1) / TR;
  const bool head = l == d.L;
  for (int i = tid; i < TW * TW; i += 256) Ws[i / TW][i % TW] = d.P[d.o_W(l) + i];
  if (tid < TW) {
    float mean, var;
    if (train) {
      const double* ts = d.tstat + (int64_t)(l & 1) * d.max_tiles * 2 * TW;
      double n = 0.0, mu = 0.0, m2 = 0.0;
      for (int q = 0; q < nt; ++q) {                           // Chan's update, tiles in index order
        const double nb = (double)min(TR, B - q * TR), mb = ts[(int64_t)q * 2 * TW + tid], m2b = ts[(int64_t)q * 2 * TW + TW + tid];
        const double delta = mb - mu, ntot = n + nb;
        mu += delta * nb / ntot;
        m2 += m2b + delta * delta * n * nb / ntot;
        n = ntot;
      }
      const double vard = m2 / (double)B;
      if (tile == 0) { d.bstat[(l * 2) * TW + tid] = mu; d.bstat[(l * 2 + 1) * TW + tid] = vard; }
      mean = (float)mu; var = (float)vard;
    } else {
      mean = d.mov[(l * 2) * TW + tid]; var = d.mov[(l * 2 + 1) * TW + tid];
    }
    smean[tid] = mean; srstd[tid] = 1.0f / sqrtf(var + BN_EPS_F);
  }
  __syncthreads();
  const float gam = d.P[d.o_gamma(l) + c], bet = d.P[d.o_beta(l) + c], bias = d.P[d.o_b(l) + c];
  const float mean = smean[c], rstd = srstd[c];
  const float* __restrict__ Yl = d.Y + (int64_t)l * d.max_batch * TW;
  float y[TR / 4];
#pragma unroll
  for (int r = 0; r < TR / 4; ++r) {
    const int rl = rg * (TR / 4) + r, row = tile * TR + rl;
    float a = 0.f; y[r] = 0.f;
    if (row < B) {
      y[r] = Yl[(int64_t)row * TW + c];
      const float z = ((y[r] - mean) * rstd) * gam + bet;
      a = elu_f(z);
    }
    As[rl][c] = a;
  }
  __syncthreads();
  float acc[TR / 4];
#pragma unroll
  for (int r = 0; r < TR / 4; ++r) acc[r] = 0.f;
  for (int k = 0; k < TW; ++k) {
    const float w = Ws[k][c];
#pragma unroll
    for (int r = 0; r < TR / 4; ++r) acc[r] = fmaf(As[rg * (TR / 4) + r][k], w, acc[r]);
  }
  __syncthreads();                                             // As is reused below
  if (!head) {
    float* __restrict__ Yn = d.Y + (int64_t)(l + 1) * d.max_batch * TW;
#pragma unroll
    for (int r = 0; r < TR / 4; ++r) {
      const int rl = rg * (TR / 4) + r, row = tile * TR + rl;
      float yn = 0.f;
      if (row < B) { yn = y[r] + (acc[r] + bias); Yn[(int64_t)row * TW + c] = yn; }
      As[rl][c] = yn;
    }
    __syncthreads();
    if (train) tile_stats(As, min(TR, B - tile * TR), d.tstat + ((int64_t)((l + 1) & 1) * d.max_tiles + tile) * 2 * TW);
  } else {
    const float gs = 2.0f / (float)((int64_t)B * d.n_out);
    double sq = 0.0, ape = 0.0;
#pragma unroll
    for (int r = 0; r < TR / 4; ++r) {
      const int row = tile * TR + rg * (TR / 4) + r;
      if (row < B) {
        float gout = 0.f;
        if (c < d.n_out) {
          const float yt = Yt[row_of(rows, base, row) * d.n_out + c];
          const float diff = (acc[r] + bias) - yt;
          gout = diff * gs;
          sq += (double)diff * (double)diff;
          ape += (double)(fabsf(diff) / fmaxf(fabsf(yt), 1e-7f));
        }
        if (train) d.Gy[(int64_t)row * TW + c] = gout;
      }
    }
    double* wred = (double*)&Ws[0][0];                          // [4][2][64] doubles: the four row groups' sums
    wred[(rg * 2) * TW + c] = sq; wred[(rg * 2 + 1) * TW + c] = ape;
    __syncthreads();
    if (tid < TW) {
      lred[0][tid] = ((wred[tid] + wred[2 * TW + tid]) + wred[4 * TW + tid]) + wred[6 * TW + tid];
      lred[1][tid] = ((wred[TW + tid] + wred[3 * TW + tid]) + wred[5 * TW + tid]) + wred[7 * TW + tid];
    }
    __syncthreads();
    if (tid < 2) {
      double s = 0.0;
      for (int q = 0; q < d.n_out; ++q) s += lred[tid][q];
      d.lpart[tile * 2 + tid] = s;
    }
  }
}

// The gradient wrt y_lu for this tile's rows, from level lu's g_z (Gz) and the tiles' partial sums of g_z and g_z xhat:
//   g = [lu < L] g_{y_{lu+1}} + gamma rstd (g_z - mean(g_z) - xhat mean(g_z xhat));  written to Gy and to the LDS tile Gs.
// Workgroup 0 also writes d gamma_lu, d beta_lu.  (red: [2][64] doubles of LDS)
__device__ __forceinline__ void gy_update(const TrainDev& d, int lu, int B, int tile, float (*Gs)[TW], double (*red)[TW]) {
  const int tid = threadIdx.x, c = tid & 63, rg = tid >> 6;
  const int nt = (B + TR - 1) / TR;
  if (tid < TW) {
    const double* ts = d.tsum + (int64_t)(lu & 1) * d.max_tiles * 2 * TW;
    double sb = 0.0, sg = 0.0;
    for (int q = 0; q < nt; ++q) { sb += ts[(int64_t)q * 2 * TW + tid]; sg += ts[(int64_t)q * 2 * TW + TW + tid]; }
    red[0][tid] = sb; red[1][tid] = sg;
    if (tile == 0) { d.G[d.o_beta(lu) + tid] = (float)sb; d.G[d.o_gamma(lu) + tid] = (float)sg; }
  }
  __syncthreads();
  float mean, rstd;
  bn_coef(d, lu, c, mean, rstd);
  const float gam = d.P[d.o_gamma(lu) + c];
  const float mb = (float)(red[0][c] / (double)B), mg = (float)(red[1][c] / (double)B);
  const float* __restrict__ Yl = d.Y + (int64_t)lu * d.max_batch * TW;
#pragma unroll
  for (int r = 0; r < TR / 4; ++r) {
    const int rl = rg * (TR / 4) + r, row = tile * TR + rl;
    float v = 0.f;
    if (row < B) {
      const int64_t idx = (int64_t)row * TW + c;
      const float xh = (Yl[idx] - mean) * rstd;
      const float gy = (gam * rstd) * ((d.Gz[idx] - mb) - xh * mg);
      v = (lu < d.L ? d.Gy[idx] : 0.f) + gy;
      d.Gy[idx] = v;
    }
    Gs[rl][c] = v;
  }
  __syncthreads();
}

// ---- one layer backward over a tile --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void layer_bwd_kernel(TrainDev d, int l, int B) {
  __shared__ float Ws[TW][TW + 1];
  __shared__ float As[TR][TW], Gs[TR][TW];
  __shared__ double red[2][TW];
  __shared__ double pred[2][4][TW];
  const int tid = threadIdx.x, c = tid & 63, rg = tid >> 6, tile = blockIdx.x;
  const bool head = l == d.L;
  if (head) {
#pragma unroll
    for (int r = 0; r < TR / 4; ++r) {
      const int rl = rg * (TR / 4) + r, row = tile * TR + rl;
      Gs[rl][c] = row < B ? d.Gy[(int64_t)row * TW + c] : 0.f;
    }
  } else {
    gy_update(d, l + 1, B, tile, Gs, red);
  }
  for (int i = tid; i < TW * TW; i += 256) Ws[i / TW][i % TW] = d.P[d.o_W(l) + i];
  float mean, rstd;
  bn_coef(d, l, c, mean, rstd);
  const float gam = d.P[d.o_gamma(l) + c], bet = d.P[d.o_beta(l) + c];
  const float* __restrict__ Yl = d.Y + (int64_t)l * d.max_batch * TW;
  float xh[TR / 4], eg[TR / 4];
#pragma unroll
  for (int r = 0; r < TR / 4; ++r) {
    const int rl = rg * (TR / 4) + r, row = tile * TR + rl;
    float a = 0.f; xh[r] = 0.f; eg[r] = 0.f;
    if (row < B) {
      xh[r] = (Yl[(int64_t)row * TW + c] - mean) * rstd;
      const float z = xh[r] * gam + bet;
      a = elu_f(z); eg[r] = elu_grad_f(z);
    }
    As[rl][c] = a;
  }
  __syncthreads();
  {                                                            // g_a = g W^T, g_z = g_a elu'(z)
    float acc[TR / 4];
#pragma unroll
    for (int r = 0; r < TR / 4; ++r) acc[r] = 0.f;
    for (int j = 0; j < TW; ++j) {
      const float w = Ws[c][j];
#pragma unroll
      for (int r = 0; r < TR / 4; ++r) acc[r] = fmaf(Gs[rg * (TR / 4) + r][j], w, acc[r]);
    }
    double pb = 0.0, pg = 0.0;
#pragma unroll
    for (int r = 0; r < TR / 4; ++r) {
      const int row = tile * TR + rg * (TR / 4) + r;
      if (row < B) {
        const float gz = acc[r] * eg[r];
        d.Gz[(int64_t)row * TW + c] = gz;
        pb += (double)gz; pg += (double)(gz * xh[r]);
      }
    }
    pred[0][rg][c] = pb; pred[1][rg][c] = pg;
  }
  {                                                            // this tile's a^T g: column j = c, rows i = 16 rg .. 16 rg + 15
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int r = 0; r < TR; ++r) {
      const float gv = Gs[r][c];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = fmaf(As[r][rg * 16 + i], gv, acc[i]);
    }
    float* __restrict__ out = d.dWpart + ((int64_t)l * d.max_tiles + tile) * TW * TW;
#pragma unroll
    for (int i = 0; i < 16; ++i) out[(rg * 16 + i) * TW + c] = acc[i];
  }
  __syncthreads();
  if (tid < TW) {
    double* ts = d.tsum + ((int64_t)(l & 1) * d.max_tiles + tile) * 2 * TW;
    ts[tid] = ((pred[0][0][tid] + pred[0][1][tid]) + pred[0][2][tid]) + pred[0][3][tid];
    ts[TW + tid] = ((pred[1][0][tid] + pred[1][1][tid]) + pred[1][2][tid]) + pred[1][3][tid];
    double sb = 0.0;
    for (int r = 0; r < TR; ++r) sb += (double)Gs[r][tid];
    d.dbpart[((int64_t)l * d.max_tiles + tile) * TW + tid] = sb;
  }
}

__global__ __launch_bounds__(256) void gy0_kernel(TrainDev d, int B) {
  __shared__ float Gs[TR][TW];
  __shared__ double red[2][TW];
  gy_update(d, 0, B, blockIdx.x, Gs, red);
  if (threadIdx.x < TW) {
    double sb = 0.0;
    for (int r = 0; r < TR; ++r) sb += (double)Gs[r][threadIdx.x];
    d.dbpart[((int64_t)(d.L + 1) * d.max_tiles + blockIdx.x) * TW + threadIdx.x] = sb;
  }
}

// ---- d W0 = X_b^T G0 + the regulariser's gradient: a wave = inputs i0 .. i0 + 15 x columns 16 wave .. 16 wave + 15 -------------
__global__ __launch_bounds__(256) void dw0_kernel(TrainDev d, const float* __restrict__ X, const int32_t* __restrict__ rows, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * 16;
  const int ii = i0 + li < d.n_in ? i0 + li : d.n_in - 1;        // (inputs beyond n_in: a valid column, not stored)
  f4_t acc = f4_t{0.f, 0.f, 0.f, 0.f};
  constexpr int U = 8;
  for (int b = 0; b < B; b += 4 * U) {
    float a[U], gv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = b + 4 * u + g;
      const bool ok = r < B;
      a[u] = ok ? X[row_of(rows, 0, r) * d.n_in + ii] : 0.f;
      gv[u] = ok ? d.Gy[(int64_t)r * TW + wave * 16 + li] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (b + 4 * u < B) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], gv[u], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * g + r;
    if (i < d.n_in) {
      const int64_t idx = (int64_t)i * TW + wave * 16 + li;
      const float w = d.P[idx];
      const float sg = w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f);
      d.G[idx] = __fadd_rn(acc[r], __fadd_rn(__fmul_rn(REG_F, sg), __fmul_rn(REG2_F, w)));
    }
  }
}

// ---- the tiles' partial sums in index order: d W_l, d b_l, d b0; loss and MAPE of the step --------------------------------------
__global__ __launch_bounds__(256) void grad_finish_kernel(TrainDev d, int B) {
  const int l = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
  const int nt = (B + TR - 1) / TR;
  {
    const int e = part * 256 + tid;
    const float* __restrict__ src = d.dWpart + (int64_t)l * d.max_tiles * TW * TW + e;
    double s = 0.0;
    for (int q = 0; q < nt; ++q) s += (double)src[(int64_t)q * TW * TW];
    float gw = (float)s;
    if (l < d.L) {
      const float w = d.P[d.o_W(l) + e];
      const float sg = w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f);
      gw = __fadd_rn(gw, __fadd_rn(__fmul_rn(REG_F, sg), __fmul_rn(REG2_F, w)));
    }
    d.G[d.o_W(l) + e] = gw;
  }
  if (part == 0 && tid < TW) {
    double s = 0.0;
    for (int q = 0; q < nt; ++q) s += d.dbpart[((int64_t)l * d.max_tiles + q) * TW + tid];
    d.G[d.o_b(l) + tid] = (float)s;
    if (l == 0) {
      double s0 = 0.0;
      for (int q = 0; q < nt; ++q) s0 += d.dbpart[((int64_t)(d.L + 1) * d.max_tiles + q) * TW + tid];
      d.G[d.o_b0() + tid] = (float)s0;
    }
  }
  if (l == 0 && part == 0 && tid == 0) {
    double sq = 0.0, ape = 0.0, s1 = 0.0, s2 = 0.0;
    for (int q = 0; q < nt; ++q) { sq += d.lpart[q * 2]; ape += d.lpart[q * 2 + 1]; }
    for (int q = 0; q < TRAIN_NREG; ++q) { s1 += d.regpart[q * 2]; s2 += d.regpart[q * 2 + 1]; }
    const double cnt = (double)B * (double)d.n_out;
    d.scal[SC_MSE] = sq / cnt;
    d.scal[SC_LOSS] = sq / cnt + (double)REG_F * s1 + (double)REG_F * s2;
    d.scal[SC_MAPE] = 100.0 * ape / cnt;
    d.scal[SC_B] = (double)B;
  }
}

// ---- Adam (Keras 1.x form), elementwise on the flat padded array; every operation rounded on its own as NumPy does -------------
// (the square root is sqrtf, which hipcc refines to a correctly rounded result by default; __fsqrt_rn compiles to the bare
//  v_sqrt_f32 approximation here, one ulp off in 18 of 22 005 values when it was used)
__global__ __launch_bounds__(256) void adam_kernel(TrainDev d) {
  __shared__ float slr;
  if (threadIdx.x == 0) {
    const double t = (double)(*d.t + 1);
    slr = (float)(d.scal[SC_LR] * sqrt(1.0 - pow(0.999, t)) / (1.0 - pow(0.9, t)));
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= d.npad) return;
  constexpr float B1 = 0.9f, B2 = 0.999f, C1 = 1.0f - 0.9f, C2 = 1.0f - 0.999f;
  const float g = d.G[i];
  const float m = __fadd_rn(__fmul_rn(B1, d.M[i]), __fmul_rn(C1, g));
  const float v = __fadd_rn(__fmul_rn(B2, d.V[i]), __fmul_rn(C2, __fmul_rn(g, g)));
  d.M[i] = m; d.V[i] = v;
  d.P[i] = __fsub_rn(d.P[i], __fdiv_rn(__fmul_rn(slr, m), __fadd_rn(sqrtf(v), 1e-7f)));
}

__global__ __launch_bounds__(256) void step_tail_kernel(TrainDev d) {
  for (int i = threadIdx.x; i < (d.L + 1) * 2 * TW; i += 256)
    d.mov[i] = __fadd_rn(__fmul_rn(0.99f, d.mov[i]), __fmul_rn(0.01f, (float)d.bstat[i]));
  if (threadIdx.x == 0) {
    *d.t += 1;
    const double B = d.scal[SC_B];
    d.scal[SC_SUM_LOSS] += d.scal[SC_LOSS] * B;
    d.scal[SC_SUM_MAPE] += d.scal[SC_MAPE] * B;
    d.scal[SC_SUM_ROWS] += B;
    d.scal[SC_SUM_MSE] += d.scal[SC_MSE] * B;
  }
}

__global__ void eval_accum_kernel(TrainDev d, int B) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int nt = (B + TR - 1) / TR;
    double sq = 0.0, ape = 0.0;
    for (int q = 0; q < nt; ++q) { sq += d.lpart[q * 2]; ape += d.lpart[q * 2 + 1]; }
    d.scal[SC_EVAL_SQ] += sq; d.scal[SC_EVAL_APE] += ape;
  }
}

}  // namespace finrom

// ==== C ABI ======================================================================================================================
using namespace finrom;

struct finrom_mlp_train_s {
  TrainDev d{};
  std::vector<void*> owned;
  std::vector<float> hP, hMov;           // host staging (sized at create)
  std::vector<double> hStat;
  double h_lr = 0.0;
  int64_t n_flat = 0;
};

namespace {

template <class T>
int dalloc(finrom_mlp_train_s* h, T** p, size_t count) {
  *p = nullptr;
  hipError_t e = hipMalloc((void**)p, (count ? count : 1) * sizeof(T));
  if (e != hipSuccess) { set_error("mlp_train_create: hipMalloc failed (" + std::to_string(count * sizeof(T)) + " bytes)"); return FINROM_ERR_NOMEM; }
  h->owned.push_back(*p);
  FR_HIP(hipMemset(*p, 0, (count ? count : 1) * sizeof(T)));
  return 0;
}

// flat unpadded layout of the ABI <-> the padded device layout (mv: the layer's mean | var slots, [(L + 1)][2][64], or null)
template <class MV>
void pack(const TrainDev& d, const float* flat, float* pad, MV* mv) {
  const int nw = d.nw;
  std::memset(pad, 0, sizeof(float) * d.npad);
  const float* s = flat;
  for (int i = 0; i < d.n_in; ++i, s += nw) std::memcpy(pad + (int64_t)i * TW, s, sizeof(float) * nw);
  std::memcpy(pad + d.o_b0(), s, sizeof(float) * nw); s += nw;
  for (int l = 0; l <= d.L; ++l) {
    const int no = l == d.L ? d.n_out : nw;
    std::memcpy(pad + d.o_gamma(l), s, sizeof(float) * nw); s += nw;
    std::memcpy(pad + d.o_beta(l), s, sizeof(float) * nw); s += nw;
    for (int q = 0; q < 2; ++q, s += nw)
      if (mv != nullptr) for (int j = 0; j < nw; ++j) mv[(l * 2 + q) * TW + j] = (MV)s[j];
    for (int i = 0; i < nw; ++i, s += no) std::memcpy(pad + d.o_W(l) + (int64_t)i * TW, s, sizeof(float) * no);
    std::memcpy(pad + d.o_b(l), s, sizeof(float) * no); s += no;
  }
}
template <class MV>
void unpack(const TrainDev& d, const float* pad, const MV* mv, float* flat) {
  const int nw = d.nw;
  float* s = flat;
  for (int i = 0; i < d.n_in; ++i, s += nw) std::memcpy(s, pad + (int64_t)i * TW, sizeof(float) * nw);
  std::memcpy(s, pad + d.o_b0(), sizeof(float) * nw); s += nw;
  for (int l = 0; l <= d.L; ++l) {
    const int no = l == d.L ? d.n_out : nw;
    std::memcpy(s, pad + d.o_gamma(l), sizeof(float) * nw); s += nw;
    std::memcpy(s, pad + d.o_beta(l), sizeof(float) * nw); s += nw;
    for (int q = 0; q < 2; ++q, s += nw)
      for (int j = 0; j < nw; ++j) s[j] = mv != nullptr ? (float)mv[(l * 2 + q) * TW + j] : 0.f;
    for (int i = 0; i < nw; ++i, s += no) std::memcpy(s, pad + d.o_W(l) + (int64_t)i * TW, sizeof(float) * no);
    std::memcpy(s, pad + d.o_b(l), sizeof(float) * no); s += no;
  }
}

int sync_for_host(const char* what) {
  if (any_capture()) { set_error(std::string(what) + ": not while a stream capture is open"); return FINROM_ERR_UNSUPPORTED; }
  FR_HIP(hipDeviceSynchronize());
  return 0;
}

// forward pass of rows [0, B) of the batch (rows: indices into X / Yt, or null: base + i); train = 0: moving statistics
int launch_forward(const TrainDev& d, const float* X, const float* Yt, const int32_t* rows, int64_t base, int B, int train, hipStream_t st) {
  const int nt = (B + TR - 1) / TR;
  hipLaunchKernelGGL(fwd0_kernel, dim3((B + 15) / 16, TRAIN_KS / 4), dim3(256), 0, st, d, X, rows, base, B);
  hipLaunchKernelGGL(y0_finish_kernel, dim3(nt), dim3(256), 0, st, d, B, train);
  for (int l = 0; l <= d.L; ++l) hipLaunchKernelGGL(layer_fwd_kernel, dim3(nt), dim3(256), 0, st, d, l, B, train, Yt, rows, base);
  FR_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int finrom_mlp_train_create(const finrom_mlp_train_desc* a, finrom_mlp_train_t* out) {
  if (!a || !out) { set_error("mlp_train_create: null argument"); return FINROM_ERR_ARG; }
  *out = nullptr;
  if (a->n_in <= 0 || a->n_w <= 0 || a->n_out <= 0 || a->n_layers < 0) { set_error("mlp_train_create: n_in, n_w, n_out must be positive, n_layers >= 0"); return FINROM_ERR_ARG; }
  if (a->max_batch < 2) { set_error("mlp_train_create: max_batch must be at least 2 (batch statistics)"); return FINROM_ERR_ARG; }
  if (a->n_w > MLP_MAX_W) { set_error("mlp_train_create: n_w > 64 is not supported"); return FINROM_ERR_UNSUPPORTED; }
  if (a->n_out > MLP_MAX_W) { set_error("mlp_train_create: n_out > 64 is not supported"); return FINROM_ERR_UNSUPPORTED; }
  if (a->n_layers > TRAIN_MAX_L) { set_error("mlp_train_create: n_layers > 8 is not supported"); return FINROM_ERR_UNSUPPORTED; }
  if (a->max_batch > (1 << 20)) { set_error("mlp_train_create: max_batch > 1048576 is not supported"); return FINROM_ERR_UNSUPPORTED; }
  if (any_capture()) { set_error("mlp_train_create: not while a stream capture is open"); return FINROM_ERR_UNSUPPORTED; }
  auto* h = new finrom_mlp_train_s();
  TrainDev& d = h->d;
  d.n_in = a->n_in; d.nw = a->n_w; d.L = a->n_layers; d.n_out = a->n_out; d.max_batch = a->max_batch;
  d.max_tiles = (a->max_batch + TR - 1) / TR;
  d.npad = d.o_layer(d.L + 1);
  const size_t nl = d.L + 1, mb = d.max_batch, mt = d.max_tiles;
  h->n_flat = (int64_t)d.n_in * d.nw + d.nw + (int64_t)d.L * (5 * d.nw + (int64_t)d.nw * d.nw) + 4 * d.nw + (int64_t)d.nw * d.n_out + d.n_out;
  h->hP.resize(d.npad); h->hMov.resize(nl * 2 * TW); h->hStat.resize(nl * 2 * TW);
  int rc = 0;
  if (!rc) rc = dalloc(h, &d.P, d.npad);
  if (!rc) rc = dalloc(h, &d.M, d.npad);
  if (!rc) rc = dalloc(h, &d.V, d.npad);
  if (!rc) rc = dalloc(h, &d.G, d.npad);
  if (!rc) rc = dalloc(h, &d.mov, nl * 2 * TW);
  if (!rc) rc = dalloc(h, &d.bstat, nl * 2 * TW);
  if (!rc) rc = dalloc(h, &d.Y, nl * mb * TW);
  if (!rc) rc = dalloc(h, &d.part0, (size_t)TRAIN_KS * mb * TW);
  if (!rc) rc = dalloc(h, &d.Gy, mb * TW);
  if (!rc) rc = dalloc(h, &d.Gz, mb * TW);
  if (!rc) rc = dalloc(h, &d.tstat, 2 * mt * 2 * TW);
  if (!rc) rc = dalloc(h, &d.tsum, 2 * mt * 2 * TW);
  if (!rc) rc = dalloc(h, &d.dWpart, nl * mt * TW * TW);
  if (!rc) rc = dalloc(h, &d.dbpart, (nl + 1) * mt * TW);
  if (!rc) rc = dalloc(h, &d.lpart, mt * 2);
  if (!rc) rc = dalloc(h, &d.regpart, (size_t)TRAIN_NREG * 2);
  if (!rc) rc = dalloc(h, &d.scal, (size_t)SC_NUM);
  if (!rc) rc = dalloc(h, &d.t, (size_t)1);
  if (rc) { finrom_mlp_train_destroy(h); return rc; }
  *out = h;
  return 0;
}

void finrom_mlp_train_destroy(finrom_mlp_train_t h) {
  if (!h) return;
  for (void* p : h->owned) dev_free(p);
  delete h;
}

int64_t finrom_mlp_train_param_count(finrom_mlp_train_t h) { return h ? h->n_flat : 0; }

int finrom_mlp_train_set_params(finrom_mlp_train_t h, const float* params, const float* m, const float* v, int64_t t) {
  if (!h) { set_error("mlp_train_set_params: null handle"); return FINROM_ERR_ARG; }
  if (!params) { set_error("mlp_train_set_params: params is null"); return FINROM_ERR_ARG; }
  if (t < 0) { set_error("mlp_train_set_params: t must not be negative"); return FINROM_ERR_ARG; }
  int rc = sync_for_host("mlp_train_set_params");
  if (rc) return rc;
  const TrainDev& d = h->d;
  pack(d, params, h->hP.data(), h->hMov.data());
  FR_HIP(hipMemcpy(d.P, h->hP.data(), sizeof(float) * d.npad, hipMemcpyHostToDevice));
  FR_HIP(hipMemcpy(d.mov, h->hMov.data(), sizeof(float) * h->hMov.size(), hipMemcpyHostToDevice));
  const float* src[2] = {m, v}; float* dst[2] = {d.M, d.V};
  for (int q = 0; q < 2; ++q) {
    if (src[q]) { pack<float>(d, src[q], h->hP.data(), nullptr); FR_HIP(hipMemcpy(dst[q], h->hP.data(), sizeof(float) * d.npad, hipMemcpyHostToDevice)); }
    else FR_HIP(hipMemset(dst[q], 0, sizeof(float) * d.npad));
  }
  const long long tt = t;
  FR_HIP(hipMemcpy(d.t, &tt, sizeof(tt), hipMemcpyHostToDevice));
  return 0;
}

int finrom_mlp_train_get_params(finrom_mlp_train_t h, float* params, float* m, float* v, int64_t* t) {
  if (!h) { set_error("mlp_train_get_params: null handle"); return FINROM_ERR_ARG; }
  int rc = sync_for_host("mlp_train_get_params");
  if (rc) return rc;
  const TrainDev& d = h->d;
  if (params) {
    FR_HIP(hipMemcpy(h->hP.data(), d.P, sizeof(float) * d.npad, hipMemcpyDeviceToHost));
    FR_HIP(hipMemcpy(h->hMov.data(), d.mov, sizeof(float) * h->hMov.size(), hipMemcpyDeviceToHost));
    unpack(d, h->hP.data(), h->hMov.data(), params);
  }
  float* dst[2] = {m, v}; const float* src[2] = {d.M, d.V};
  for (int q = 0; q < 2; ++q)
    if (dst[q]) { FR_HIP(hipMemcpy(h->hP.data(), src[q], sizeof(float) * d.npad, hipMemcpyDeviceToHost)); unpack<float>(d, h->hP.data(), nullptr, dst[q]); }
  if (t) { long long tt = 0; FR_HIP(hipMemcpy(&tt, d.t, sizeof(tt), hipMemcpyDeviceToHost)); *t = tt; }
  return 0;
}

int finrom_mlp_train_set_grads(finrom_mlp_train_t h, const float* grads, const double* loss_mape, int32_t B) {
  if (!h) { set_error("mlp_train_set_grads: null handle"); return FINROM_ERR_ARG; }
  if (!grads || !loss_mape) { set_error("mlp_train_set_grads: grads / loss_mape is null"); return FINROM_ERR_ARG; }
  if (B < 2 || B > h->d.max_batch) { set_error("mlp_train_set_grads: B must be in [2, max_batch]"); return FINROM_ERR_ARG; }
  int rc = sync_for_host("mlp_train_set_grads");
  if (rc) return rc;
  const TrainDev& d = h->d;
  std::fill(h->hStat.begin(), h->hStat.end(), 0.0);
  pack(d, grads, h->hP.data(), h->hStat.data());
  FR_HIP(hipMemcpy(d.G, h->hP.data(), sizeof(float) * d.npad, hipMemcpyHostToDevice));
  FR_HIP(hipMemcpy(d.bstat, h->hStat.data(), sizeof(double) * h->hStat.size(), hipMemcpyHostToDevice));
  const double s[2] = {loss_mape[0], loss_mape[1]}, b = (double)B;
  FR_HIP(hipMemcpy(d.scal + SC_LOSS, s, sizeof(s), hipMemcpyHostToDevice));
  FR_HIP(hipMemcpy(d.scal + SC_B, &b, sizeof(b), hipMemcpyHostToDevice));
  FR_HIP(hipMemcpy(d.scal + SC_MSE, s, sizeof(double), hipMemcpyHostToDevice));      // (no regulariser is known here: the loss given)
  return 0;
}

int finrom_mlp_train_get_grads(finrom_mlp_train_t h, float* grads, double* loss_mape) {
  if (!h) { set_error("mlp_train_get_grads: null handle"); return FINROM_ERR_ARG; }
  int rc = sync_for_host("mlp_train_get_grads");
  if (rc) return rc;
  const TrainDev& d = h->d;
  if (grads) {
    FR_HIP(hipMemcpy(h->hP.data(), d.G, sizeof(float) * d.npad, hipMemcpyDeviceToHost));
    FR_HIP(hipMemcpy(h->hStat.data(), d.bstat, sizeof(double) * h->hStat.size(), hipMemcpyDeviceToHost));
    unpack(d, h->hP.data(), h->hStat.data(), grads);
  }
  if (loss_mape) FR_HIP(hipMemcpy(loss_mape, d.scal + SC_LOSS, 2 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int finrom_mlp_train_set_lr(finrom_mlp_train_t h, double lr, void* stream) {
  if (!h) { set_error("mlp_train_set_lr: null handle"); return FINROM_ERR_ARG; }
  if (!(lr >= 0.0) || !std::isfinite(lr)) { set_error("mlp_train_set_lr: lr must be finite and not negative"); return FINROM_ERR_ARG; }
  CallGuard cg((hipStream_t)stream);
  if (call_captures()) { set_error("mlp_train_set_lr: not under stream capture (lr lives in device memory: set it between replays)"); return FINROM_ERR_UNSUPPORTED; }
  h->h_lr = lr;
  FR_HIP(hipMemcpyAsync(h->d.scal + SC_LR, &h->h_lr, sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream));
  FR_HIP(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int finrom_mlp_train_grad(finrom_mlp_train_t h, const float* X, const float* Y, const int32_t* rows, int32_t B, void* stream) {
  if (!h) { set_error("mlp_train_grad: null handle"); return FINROM_ERR_ARG; }
  if (!X || !Y || !rows) { set_error("mlp_train_grad: X / Y / rows is null"); return FINROM_ERR_ARG; }
  if (B < 2) { set_error("mlp_train_grad: B must be at least 2 (batch statistics)"); return FINROM_ERR_ARG; }
  if (B > h->d.max_batch) { set_error("mlp_train_grad: B exceeds max_batch"); return FINROM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  CallGuard cg(st);
  const TrainDev& d = h->d;
  const int nt = (B + TR - 1) / TR;
  ScopedKernelTimer tm(K_MISC, st);
  hipLaunchKernelGGL(reg_kernel, dim3(TRAIN_NREG), dim3(256), 0, st, d);
  int rc = launch_forward(d, X, Y, rows, 0, B, 1, st);
  if (rc) return rc;
  for (int l = d.L; l >= 0; --l) hipLaunchKernelGGL(layer_bwd_kernel, dim3(nt), dim3(256), 0, st, d, l, B);
  hipLaunchKernelGGL(gy0_kernel, dim3(nt), dim3(256), 0, st, d, B);
  hipLaunchKernelGGL(dw0_kernel, dim3((d.n_in + 15) / 16), dim3(256), 0, st, d, X, rows, B);
  hipLaunchKernelGGL(grad_finish_kernel, dim3(d.L + 1, TW * TW / 256), dim3(256), 0, st, d, B);
  FR_HIP(hipGetLastError());
  return 0;
}

int finrom_mlp_train_apply(finrom_mlp_train_t h, void* stream) {
  if (!h) { set_error("mlp_train_apply: null handle"); return FINROM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  CallGuard cg(st);
  const TrainDev& d = h->d;
  ScopedKernelTimer tm(K_MISC, st);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((d.npad + 255) / 256)), dim3(256), 0, st, d);
  hipLaunchKernelGGL(step_tail_kernel, dim3(1), dim3(256), 0, st, d);
  FR_HIP(hipGetLastError());
  return 0;
}

int finrom_mlp_train_eval(finrom_mlp_train_t h, const float* X, const float* Y, int64_t S, double* out, void* stream) {
  if (!h) { set_error("mlp_train_eval: null handle"); return FINROM_ERR_ARG; }
  if (!X || !Y || !out) { set_error("mlp_train_eval: X / Y / out is null"); return FINROM_ERR_ARG; }
  if (S < 1) { set_error("mlp_train_eval: S must be positive"); return FINROM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  CallGuard cg(st);
  if (call_captures()) { set_error("mlp_train_eval: returns host values, not under stream capture"); return FINROM_ERR_UNSUPPORTED; }
  const TrainDev& d = h->d;
  FR_HIP(hipMemsetAsync(d.scal + SC_EVAL_SQ, 0, 2 * sizeof(double), st));
  hipLaunchKernelGGL(reg_kernel, dim3(TRAIN_NREG), dim3(256), 0, st, d);
  for (int64_t base = 0; base < S; base += d.max_batch) {
    const int B = (int)(S - base < d.max_batch ? S - base : d.max_batch);
    int rc = launch_forward(d, X, Y, nullptr, base, B, 0, st);
    if (rc) return rc;
    hipLaunchKernelGGL(eval_accum_kernel, dim3(1), dim3(64), 0, st, d, B);
  }
  FR_HIP(hipGetLastError());
  double acc[2], reg[TRAIN_NREG * 2];
  FR_HIP(hipMemcpyAsync(acc, d.scal + SC_EVAL_SQ, sizeof(acc), hipMemcpyDeviceToHost, st));
  FR_HIP(hipMemcpyAsync(reg, d.regpart, sizeof(reg), hipMemcpyDeviceToHost, st));
  FR_HIP(hipStreamSynchronize(st));
  double s1 = 0.0, s2 = 0.0;
  for (int q = 0; q < TRAIN_NREG; ++q) { s1 += reg[q * 2]; s2 += reg[q * 2 + 1]; }
  const double cnt = (double)S * (double)d.n_out;
  out[0] = acc[0] / cnt + (double)REG_F * s1 + (double)REG_F * s2;
  out[1] = 100.0 * acc[1] / cnt;
  return 0;
}

int finrom_mlp_train_epoch_stats(finrom_mlp_train_t h, double* out, int32_t reset, void* stream) {
  if (!h) { set_error("mlp_train_epoch_stats: null handle"); return FINROM_ERR_ARG; }
  if (!out) { set_error("mlp_train_epoch_stats: out is null"); return FINROM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  CallGuard cg(st);
  if (call_captures()) { set_error("mlp_train_epoch_stats: returns host values, not under stream capture"); return FINROM_ERR_UNSUPPORTED; }
  FR_HIP(hipMemcpyAsync(out, h->d.scal + SC_SUM_LOSS, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (reset) FR_HIP(hipMemsetAsync(h->d.scal + SC_SUM_LOSS, 0, 4 * sizeof(double), st));
  FR_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
