// The network as a model of its own: loss[s] = 1/2 |data - NN(k_s)|^2 and grad[s] = -vjp(data - NN(k_s)), the reference's pure
// deep-learning surrogate (deep_learning/dl_model.py `load_surrogate_model`, bayesian_inference/estimate_MAP.py `MLSolverWrapper`).
// Two forms behind finrom_mlp_misfit_grad:
//   per-sample  one 1024-thread workgroup per sample, the device functions of mlp_device.h unchanged (mlp_forward_body<1024>,
//               mlp_backward_hidden_wave) and the first layer's transpose as mlp_backward_kernel<NP> has it, without a ROM term:
//               S = 1 .. 64 dependent calls, latency;
//   tile        SUR_ROWS = 64 samples per 256-thread workgroup, for the batches a surrogate exists for.  k is read ONCE, in
//               chunks of SUR_KC inputs with coalesced loads, rounded to fp32 as the per-sample form rounds it and handed to
//               v_mfma_f32_16x16x4_f32 through LDS: wave w owns rows 16 w .. 16 w + 15, every (sample, unit) product is one
//               k-ordered fma chain over i = 0 .. n_in - 1 (the K dimension is never split), then + b0.  A row of the A operand
//               reaches only its own row of D, and the layers behind are computed per row: a sample's result depends neither on
//               S, nor on its row in the tile, nor on its neighbours.  The walk back is per row too; grad = -G0 W0^T is again
//               the matrix cores', K = 64 in one ordered chain over the units.
// f32 MFMA fragment maps (16x16x4): A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15],
// C/D[row = 4 (lane >> 4) + reg][col = lane & 15] -- NOT the f64 map of rom_proj_*.hip.
#include "mlp_device.h"
#include "mlp_surrogate.h"

namespace finrom {

typedef float f4_t __attribute__((ext_vector_type(4)));
constexpr int SUR_THREADS = 1024;
constexpr int SUR_SPLIT = 8;            // workgroups per sample of the per-sample backward launch, up to SUR_SPLIT_MAX_S samples
constexpr int SUR_SPLIT_MAX_S = 64;

// ---- per-sample form ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SUR_THREADS) void sur_forward_kernel(MlpDev m, const double* __restrict__ k, int64_t S,
                                                                  const double* __restrict__ data, int64_t data_stride,
                                                                  float* __restrict__ tape, double* out, double* __restrict__ loss) {
  extern __shared__ float xs[];                        // [n_in] input
  __shared__ double rr[MLP_MAX_W];
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x;
  mlp_forward_body<SUR_THREADS>(m, k, s, nullptr, 0, tape, out, nullptr, nullptr, 0, nullptr, xs, tid);
  if (loss == nullptr || tid >= 64) return;            // (wave 0 has written out: each lane reads back its own store)
  if (tid < m.n_out) {
    const double r = data[(data_stride ? s * data_stride : 0) + tid] - out[s * m.n_out + tid];
    rr[tid] = r * r;
  }
  wave_sync();
  if (tid == 0) {
    double t = 0.0;
    for (int o = 0; o < m.n_out; ++o) t += rr[o];
    loss[s] = 0.5 * t;
  }
}

// grad[s][i] = -sum_j g0[j] W0[i][j]: the walk back by wave 0 (upstream r = data - (zero + out)), then n_in / NP rows of the first
// layer's transpose per workgroup, four chains of 16 as in mlp_backward_kernel
template <int NP>
__global__ __launch_bounds__(SUR_THREADS) void sur_backward_kernel(MlpDev m, int64_t S, const float* __restrict__ tape,
                                                                   const double* __restrict__ data, int64_t data_stride,
                                                                   const double* __restrict__ zero, const double* __restrict__ out,
                                                                   double* __restrict__ grad) {
  __shared__ float g[MLP_MAX_W], up[MLP_MAX_W];
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x, nw = m.n_w;
  if (tid < 64) mlp_backward_hidden_wave(m, s, tape, data, data_stride, zero, out, g, up, tid);
  __syncthreads();
  const int wg = NP > 1 ? (int)blockIdx.y : 0;
  const int r0 = (int)((int64_t)m.n_in * wg / NP), r1 = (int)((int64_t)m.n_in * (wg + 1) / NP);
  for (int i = r0 + tid; i < r1; i += SUR_THREADS) {
    const float* __restrict__ wrow = m.W0 + (int64_t)i * nw;
    float a4[4] = {0.f, 0.f, 0.f, 0.f};
    int j = 0;
    for (; j + 16 <= nw; j += 16) {
      float wv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) wv[u] = wrow[j + u];
#pragma unroll
      for (int u = 0; u < 16; ++u) a4[u & 3] = fmaf(g[j + u], wv[u], a4[u & 3]);
    }
    for (; j < nw; ++j) a4[0] = fmaf(g[j], wrow[j], a4[0]);
    const float acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
    grad[s * m.n_in + i] = -(double)acc;               // d loss / d input = -vjp(r)
  }
}

// ---- tile form -----------------------------------------------------------------------------------------------------------------------
// LDS strides (floats): the A operand's rows 68 apart (lane (li, g) reads [li][4 s + g]: banks 4 li + g, two lanes per bank at
// worst), the staged weights' rows 80 apart (banks 16 g + li: none), the per-row phases' rows 65 apart (lane = row: none).
constexpr int SUR_XLD = 68, SUR_WLD = 80, SUR_ALD = 65;

__global__ __launch_bounds__(256) void sur_tile_forward_kernel(MlpDev m, SurPad p, const double* __restrict__ k, int64_t S,
                                                               const double* __restrict__ data, int64_t data_stride,
                                                               float* __restrict__ tape, double* __restrict__ out,
                                                               double* __restrict__ loss, int* __restrict__ bad) {
  __shared__ __attribute__((aligned(16))) float lds[SUR_ROWS * SUR_XLD + SUR_KC * SUR_WLD];
  __shared__ int badrow[SUR_ROWS];
  float* xs = lds;                                     // [64 rows][SUR_XLD]: the chunk of k in fp32
  float* ws = lds + SUR_ROWS * SUR_XLD;                // [64 inputs][SUR_WLD]: the chunk of W0
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  const int64_t s0 = (int64_t)blockIdx.x * SUR_ROWS;
  const int nw = m.n_w, n_in = m.n_in, no = m.n_out, L = m.n_layers;
  const int ncb = (nw + 15) >> 4;                      // 16-column blocks of units that hold any
  if (tid < SUR_ROWS) badrow[tid] = 0;
  __syncthreads();
  // this thread's share of a chunk: 16 doubles of k (element e = tid + 256 u: row e / 64, input e % 64 -- a wave reads 512
  // contiguous bytes of one row), four 16-byte pieces of W0p (contiguous: the chunk is 64 padded rows)
  double kv[16]; f4_t wv[4];
  const f4_t* __restrict__ W0v = (const f4_t*)p.W0p;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = tid + 256 * u, row = e >> 6, col = e & 63;
    const int64_t sr = s0 + row < S ? s0 + row : S - 1;      // (rows beyond the batch: a valid row, not stored)
    kv[u] = col < n_in ? k[sr * n_in + col] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) wv[u] = W0v[tid + 256 * u];
  f4_t acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f4_t{0.f, 0.f, 0.f, 0.f};
  for (int kc0 = 0; kc0 < p.n_inp; kc0 += SUR_KC) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = tid + 256 * u, row = e >> 6, col = e & 63;
      if (!__builtin_isfinite(kv[u])) badrow[row] = 1;
      xs[row * SUR_XLD + col] = (float)kv[u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = tid + 256 * u;
      *(f4_t*)&ws[(e >> 4) * SUR_WLD + 4 * (e & 15)] = wv[u];
    }
    __syncthreads();
    if (kc0 + SUR_KC < p.n_inp) {                      // the next chunk's loads fly under this chunk's MFMAs
      const int kn = kc0 + SUR_KC;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u, row = e >> 6, col = kn + (e & 63);
        const int64_t sr = s0 + row < S ? s0 + row : S - 1;
        kv[u] = col < n_in ? k[sr * n_in + col] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) wv[u] = W0v[(int64_t)kn * 16 + tid + 256 * u];
    }
#pragma unroll
    for (int s = 0; s < SUR_KC / 4; ++s) {
      const float a = xs[(16 * wave + li) * SUR_XLD + 4 * s + g];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < ncb) {                                 // (uniform over the workgroup)
          const float b = ws[(4 * s + g) * SUR_WLD + 16 * c + li];
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[c], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  // the layers behind, per row: thread (row = tid & 63, units 16 q .. 16 q + 15, q = its wave: the weights it reads are
  // wave-uniform LDS broadcasts).  A [64][SUR_ALD]: y0, then each layer's activations, at last the head's output; wl [64][64]
  float* A = lds;
  float* wl = lds + SUR_ROWS * SUR_XLD;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) A[(16 * wave + 4 * g + r) * SUR_ALD + 16 * c + li] = acc[c][r];
  __syncthreads();
  const int r = tid & 63, q = wave;
  const int64_t srow = s0 + r;
  const bool valid = srow < S;
  float y[16];
  {
    f4_t b0[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) b0[v] = ((const f4_t*)(p.b0p + 16 * q))[v];
#pragma unroll
    for (int u = 0; u < 16; ++u) y[u] = b0[u >> 2][u & 3] + A[r * SUR_ALD + 16 * q + u];
  }
  __syncthreads();
  float* __restrict__ tp = tape != nullptr && valid ? tape + srow * (int64_t)(L + 1) * nw : nullptr;
  for (int l = 0; l <= L; ++l) {                       // l == L: the head
    // the layer's scale, shift and bias for this thread's 16 units, requested together and before any store (loads behind a
    // store through a pointer the compiler cannot tell apart wait for one another: 48 trips to L2 in series per layer)
    f4_t sc[4], sh[4], bb[4];
    const float* __restrict__ bsrc = l < L ? p.bp + l * 64 : p.bhp;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      sc[v] = ((const f4_t*)(p.scp + l * 64 + 16 * q))[v];
      sh[v] = ((const f4_t*)(p.shp + l * 64 + 16 * q))[v];
      bb[v] = ((const f4_t*)(bsrc + 16 * q))[v];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int j = 16 * q + u;
      const float z = fmaf(y[u], sc[u >> 2][u & 3], sh[u >> 2][u & 3]);
      if (tp != nullptr && j < nw) tp[l * nw + j] = z;
      A[r * SUR_ALD + j] = elu_f(z);
    }
    const f4_t* __restrict__ Wsrc = (const f4_t*)(l < L ? p.Wp + (int64_t)l * 4096 : p.Whp);
#pragma unroll
    for (int u = 0; u < 4; ++u) ((f4_t*)wl)[tid + 256 * u] = Wsrc[tid + 256 * u];
    __syncthreads();
    float ac[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) ac[u] = bb[u >> 2][u & 3];
    for (int i = 0; i < nw; ++i) {
      const float ai = A[r * SUR_ALD + i];
      f4_t w[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) w[v] = ((const f4_t*)wl)[i * 16 + 4 * q + v];
#pragma unroll
      for (int u = 0; u < 16; ++u) ac[u] = fmaf(ai, w[u >> 2][u & 3], ac[u]);
    }
    __syncthreads();                                   // every thread of the row has read its activations
    if (l < L) {
#pragma unroll
      for (int u = 0; u < 16; ++u) y[u] += ac[u];
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u) A[r * SUR_ALD + 16 * q + u] = ac[u];
    }
  }
  __syncthreads();
  const int nvalid = S - s0 < SUR_ROWS ? (int)(S - s0) : SUR_ROWS;
  const double qnan = __builtin_nan("");
  for (int t = tid; t < nvalid * no; t += 256) {      // the tile's rows of out are contiguous
    const int row = t / no, j = t - row * no;
    out[s0 * no + t] = badrow[row] ? qnan : (double)A[row * SUR_ALD + j];
  }
  if (tid < nvalid) {
    bad[s0 + tid] = badrow[tid];
    if (loss != nullptr) {
      const double* __restrict__ d = data + (data_stride ? (s0 + tid) * data_stride : 0);
      double t = 0.0;
      for (int o = 0; o < no; ++o) { const double e = d[o] - (double)A[tid * SUR_ALD + o]; t += e * e; }
      loss[s0 + tid] = badrow[tid] ? qnan : 0.5 * t;
    }
  }
}

__global__ __launch_bounds__(256) void sur_tile_backward_kernel(MlpDev m, SurPad p, int64_t S, const float* __restrict__ tape,
                                                                const double* __restrict__ data, int64_t data_stride,
                                                                const double* __restrict__ out, const int* __restrict__ bad,
                                                                double* __restrict__ grad) {
  __shared__ __attribute__((aligned(16))) float lds[SUR_ROWS * SUR_ALD + SUR_KC * SUR_XLD];
  float* G = lds;                                      // [64 rows][SUR_ALD]: the upstream, then g of each layer, at last g0
  float* wl = lds + SUR_ROWS * SUR_ALD;                // [64][64] a layer's transposed weights; then [64 inputs][SUR_XLD] chunks of W0
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  const int64_t s0 = (int64_t)blockIdx.x * SUR_ROWS;
  const int nw = m.n_w, n_in = m.n_in, no = m.n_out, L = m.n_layers;
  // the walk back, per row: thread (row = tid & 63, units 16 q .. 16 q + 15)
  const int r = tid & 63, q = wave;
  const int64_t srow = s0 + r < S ? s0 + r : S - 1;    // (rows beyond the batch: a valid row, not stored)
  const float* __restrict__ tp = tape + srow * (int64_t)(L + 1) * nw;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int o = 16 * q + u;
    G[r * SUR_ALD + o] = o < no ? (float)(data[(data_stride ? srow * data_stride : 0) + o] - out[srow * no + o]) : 0.f;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) ((f4_t*)wl)[tid + 256 * u] = ((const f4_t*)p.WhpT)[tid + 256 * u];
  __syncthreads();
  float gi[16];
  {
    float ac[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) ac[u] = 0.f;
    for (int o = 0; o < no; ++o) {
      const float uo = G[r * SUR_ALD + o];
      f4_t w[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) w[v] = ((const f4_t*)wl)[o * 16 + 4 * q + v];
#pragma unroll
      for (int u = 0; u < 16; ++u) ac[u] = fmaf(uo, w[u >> 2][u & 3], ac[u]);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {                     // (the tape read at a clamped index: sixteen loads in flight, no branches)
      const int i = 16 * q + u;
      const float z = tp[L * nw + (i < nw ? i : nw - 1)];
      gi[u] = i < nw ? ac[u] * elu_grad_f(z) * p.scp[L * 64 + i] : 0.f;
    }
  }
  __syncthreads();                                     // every thread of the row has read the upstream
#pragma unroll
  for (int u = 0; u < 16; ++u) G[r * SUR_ALD + 16 * q + u] = gi[u];
  for (int l = L - 1; l >= 0; --l) {                   // g <- g + (W_l g) * elu'(z_l) * s_l   (skip + branch)
#pragma unroll
    for (int u = 0; u < 4; ++u) ((f4_t*)wl)[tid + 256 * u] = ((const f4_t*)(p.WpT + (int64_t)l * 4096))[tid + 256 * u];
    __syncthreads();
    float ac[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) ac[u] = 0.f;
    for (int j = 0; j < nw; ++j) {
      const float gj = G[r * SUR_ALD + j];
      f4_t w[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) w[v] = ((const f4_t*)wl)[j * 16 + 4 * q + v];
#pragma unroll
      for (int u = 0; u < 16; ++u) ac[u] = fmaf(gj, w[u >> 2][u & 3], ac[u]);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = 16 * q + u;
      const float z = tp[l * nw + (i < nw ? i : nw - 1)];
      gi[u] = i < nw ? gi[u] + ac[u] * elu_grad_f(z) * p.scp[l * 64 + i] : 0.f;
    }
    __syncthreads();                                   // everybody has read the old g (and the layer's weights)
#pragma unroll
    for (int u = 0; u < 16; ++u) G[r * SUR_ALD + 16 * q + u] = gi[u];
  }
  __syncthreads();
  // grad = -G0 W0^T: wave w keeps its 16 rows of G0 as the A operand of all 16 k-steps; W0p streams through LDS in chunks of 64
  // inputs (the B operand: B[k = unit][col = input]); four 16-input blocks = four independent accumulators per chunk
  float a[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) a[s] = G[(16 * wave + li) * SUR_ALD + 4 * s + g];
  int badv[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) { const int64_t sr = s0 + 16 * wave + 4 * g + rr; badv[rr] = sr < S ? bad[sr] : 0; }
  const int ncs = (nw + 3) >> 2;                       // k-steps that hold any unit
  const double qnan = __builtin_nan("");
  f4_t wv[4];
  const f4_t* __restrict__ W0v = (const f4_t*)p.W0p;
#pragma unroll
  for (int u = 0; u < 4; ++u) wv[u] = W0v[tid + 256 * u];
  for (int i0 = 0; i0 < p.n_inp; i0 += SUR_KC) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = tid + 256 * u;
      *(f4_t*)&wl[(e >> 4) * SUR_XLD + 4 * (e & 15)] = wv[u];
    }
    __syncthreads();
    if (i0 + SUR_KC < p.n_inp) {
#pragma unroll
      for (int u = 0; u < 4; ++u) wv[u] = W0v[(int64_t)(i0 + SUR_KC) * 16 + tid + 256 * u];
    }
    f4_t acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (s < ncs) {                                   // (uniform over the workgroup)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float bv = wl[(16 * b + li) * SUR_XLD + 4 * s + g];
          acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bv, acc[b], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + 16 * b + li;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int64_t sr = s0 + 16 * wave + 4 * g + rr;
        if (sr < S && i < n_in) grad[sr * n_in + i] = badv[rr] ? qnan : -(double)acc[b][rr];
      }
    }
    __syncthreads();
  }
}

// dst [batch][rows_pad][64] = src [batch][rows][cols] (element (r, c) at r sr + c sc), zeros beyond
__global__ __launch_bounds__(256) void sur_pad_kernel(const float* __restrict__ src, int rows, int cols, int64_t sr, int64_t sc,
                                                      int64_t sbatch, float* __restrict__ dst, int rows_pad) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)rows_pad * 64) return;
  const int rr = (int)(idx >> 6), c = (int)(idx & 63);
  const int64_t b = blockIdx.y;
  dst[b * rows_pad * 64 + idx] = rr < rows && c < cols ? src[b * sbatch + rr * sr + c * sc] : 0.f;
}

size_t sur_pad_floats(const MlpDev& m) {
  const size_t L = m.n_layers;
  return (size_t)sur_n_inp(m.n_in) * 64 + 64 + 2 * (L + 1) * 64 + 2 * L * 4096 + L * 64 + 2 * 4096 + 64;
}

int launch_sur_pad(const MlpDev& m, float* buf, SurPad* p, hipStream_t st) {
  const int L = m.n_layers, nw = m.n_w, no = m.n_out;
  p->n_inp = sur_n_inp(m.n_in);
  float* at = buf;
  auto pad = [&](const float* src, int batch, int rows, int cols, int64_t sr, int64_t sc, int64_t sbatch, int rows_pad) -> const float* {
    float* dst = at;
    at += (size_t)batch * rows_pad * 64;
    if (batch > 0)
      hipLaunchKernelGGL(sur_pad_kernel, dim3((unsigned)(((int64_t)rows_pad * 64 + 255) / 256), (unsigned)batch), dim3(256), 0, st, src, rows,
                         cols, sr, sc, sbatch, dst, rows_pad);
    return dst;
  };
  p->W0p = pad(m.W0, 1, m.n_in, nw, nw, 1, 0, p->n_inp);
  p->b0p = pad(m.b0, 1, 1, nw, 0, 1, 0, 1);
  p->scp = pad(m.scale, L + 1, 1, nw, 0, 1, nw, 1);
  p->shp = pad(m.shift, L + 1, 1, nw, 0, 1, nw, 1);
  p->Wp = pad(m.W, L, nw, nw, nw, 1, (int64_t)nw * nw, 64);
  p->WpT = pad(m.W, L, nw, nw, 1, nw, (int64_t)nw * nw, 64);
  p->bp = pad(m.b, L, 1, nw, 0, 1, nw, 1);
  p->Whp = pad(m.Wh, 1, nw, no, no, 1, 0, 64);
  p->WhpT = pad(m.Wh, 1, no, nw, 1, no, 0, 64);
  p->bhp = pad(m.bh, 1, 1, no, 0, 1, 0, 1);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_sur_forward(const MlpDev& m, const double* k, int64_t S, const double* data, int64_t data_stride, float* tape, double* out,
                       double* loss, hipStream_t st) {
  if (S == 0) return 0;
  if (int rc = mlp_forward_fits(m)) return rc;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(sur_forward_kernel, dim3((unsigned)S), dim3(SUR_THREADS), (size_t)m.n_in * sizeof(float), st, m, k, S, data, data_stride,
                     tape, out, loss);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_sur_backward(const MlpDev& m, int64_t S, const float* tape, const double* data, int64_t data_stride, const double* zero,
                        const double* out, double* grad, hipStream_t st) {
  if (S == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  if (S <= SUR_SPLIT_MAX_S)
    hipLaunchKernelGGL(sur_backward_kernel<SUR_SPLIT>, dim3((unsigned)S, SUR_SPLIT), dim3(SUR_THREADS), 0, st, m, S, tape, data, data_stride,
                       zero, out, grad);
  else
    hipLaunchKernelGGL(sur_backward_kernel<1>, dim3((unsigned)S), dim3(SUR_THREADS), 0, st, m, S, tape, data, data_stride, zero, out, grad);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_sur_tile_forward(const MlpDev& m, const SurPad& p, const double* k, int64_t S, const double* data, int64_t data_stride,
                            float* tape, double* out, double* loss, int* bad, hipStream_t st) {
  if (S == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(sur_tile_forward_kernel, dim3((unsigned)((S + SUR_ROWS - 1) / SUR_ROWS)), dim3(256), 0, st, m, p, k, S, data, data_stride,
                     tape, out, loss, bad);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_sur_tile_backward(const MlpDev& m, const SurPad& p, int64_t S, const float* tape, const double* data, int64_t data_stride,
                             const double* out, const int* bad, double* grad, hipStream_t st) {
  if (S == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(sur_tile_backward_kernel, dim3((unsigned)((S + SUR_ROWS - 1) / SUR_ROWS)), dim3(256), 0, st, m, p, S, tape, data,
                     data_stride, out, bad, grad);
  FR_HIP(hipGetLastError());
  return 0;
}

}  // namespace finrom
