// BatchNorm1d over node rows with its LeakyReLU, on a row-major [rows, cols]
// fp32 table.
//
// Replaces x.permute(0, 2, 1) -> nn.BatchNorm1d -> permute back ->
// F.leaky_relu of the reference's GCNBlock / EmbeddingBlock
// (gnn/models/networks/deep_rp_robust_gcn.py:39-45, 57-63): the statistics of
// channel c run over all B*N rows of column c, so no transposed copy exists.
//
// Geometry (a function of (rows, cols) only -- never of the device -- so the
// same input gives the same bits on every machine).  A block of 256 threads is
// RL row lanes x CL column lanes; CL is the power of two in [8, 64] whose
// 4 * CL columns first cover cols (64 from 129 columns on).  A block owns one
// tile of 4 * CL columns and one run of rows_per_block consecutive rows; row
// lane rl takes the run's rows rl, rl + RL, ... in that order, four columns of
// each.  In the float4 form column lane cl holds columns 4 cl .. 4 cl + 3 of
// the tile (one 16-B load: a wave-instruction reads 1 KiB of each of its
// rows), in the scalar form columns cl, cl + CL, cl + 2 CL, cl + 3 CL (four
// 4-B loads, 256 contiguous bytes per wave-instruction and row).  Either way
// column c of a block sums the same rows in the same order in every row lane,
// the row lanes' sums are added in row-lane order, and the blocks' partials in
// block order: the two forms give the same bits.
//
// Statistics accumulate in fp64: x widened is exact and so is the product of
// two widened fp32 values, so sum(x) and sum(x^2) carry only fp64 rounding;
// the partials, the finalize and var = E[x^2] - mean^2 stay fp64 and mean /
// invstd are rounded to fp32 once.  (One-pass fp32 E[x^2] - E[x]^2 and a
// sequential fp32 Welford both miss fp64 by ~1e-1 in the variance of a column
// with mean 4096 and variance 21: tests/test_bn_rows_design.py.)
//
// HBM bytes (B = rows * cols * 4): train forward 3 B (statistics read, apply
// read + write), eval 2 B, backward 7 B (dy, y, x read twice, dx written).
// No atomics, no allocation, no host sync.
#include "grl_internal.h"

namespace grl {
namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_BLOCKS = 1024;  // column tiles x row blocks of one pass (when a tile count allows)
constexpr int BN_ROWS_PER_LANE = 16;

struct BnGeo {
  int cl;        // column lanes
  int rl;        // row lanes = 256 / cl
  int64_t nct;   // column tiles of 4 * cl columns
  int64_t rpb;   // rows per block (a multiple of rl)
  int64_t nb;    // row blocks
};

BnGeo bn_geo(int64_t rows, int64_t cols) {
  BnGeo g;
  g.cl = 8;
  while (g.cl < 64 && 4 * g.cl < cols) g.cl *= 2;
  g.rl = BN_THREADS / g.cl;
  g.nct = std::max<int64_t>(ceil_div(cols, 4 * g.cl), 1);
  const int64_t max_nb = std::max<int64_t>(BN_MAX_BLOCKS / g.nct, 1);
  g.rpb = (int64_t)g.rl * BN_ROWS_PER_LANE;
  g.nb = std::max<int64_t>(ceil_div(rows, g.rpb), 1);
  if (g.nb > max_nb) {
    g.rpb = ceil_div(ceil_div(rows, max_nb), g.rl) * g.rl;
    g.nb = ceil_div(rows, g.rpb);
  }
  return g;
}

// workspace: [nb][2][cols] fp64 partials, then [2][cols] fp64 for the backward's per-column means
size_t bn_ws_bytes(const BnGeo& g, int64_t cols) { return (size_t)(g.nb * 2 + 2) * (size_t)cols * sizeof(double); }

// The four columns of this thread and which of them exist.
template <bool VEC>
struct BnCols {
  int64_t c[4];
  bool ok[4];
  __device__ BnCols(int cl_lanes, int cols) {
    const int cl = threadIdx.x % cl_lanes;
    const int64_t tile0 = (int64_t)blockIdx.x * 4 * cl_lanes;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c[i] = VEC ? tile0 + 4 * cl + i : tile0 + cl + (int64_t)cl_lanes * i;
      ok[i] = c[i] < cols;
    }
  }
  // this thread's slot of column i in a [4 * cl_lanes] tile image: the same column lands in the same slot in
  // both forms
  __device__ int slot(int cl_lanes, int i) const { return (int)(c[i] - (int64_t)blockIdx.x * 4 * cl_lanes); }
  __device__ void load(const float* __restrict__ p, float (&v)[4]) const {
    if (VEC) {
      if (ok[0]) {
        const float4 t = *reinterpret_cast<const float4*>(p + c[0]);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
      } else {
        v[0] = v[1] = v[2] = v[3] = 0.0f;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = ok[i] ? p[c[i]] : 0.0f;
    }
  }
  __device__ void store(float* p, const float (&v)[4]) const {
    if (VEC) {
      if (ok[0]) *reinterpret_cast<float4*>(p + c[0]) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (ok[i]) p[c[i]] = v[i];
    }
  }
  // a per-column vector (NULL: the constant `dflt`)
  __device__ void vec(const float* __restrict__ p, float dflt, float (&v)[4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (p && ok[i]) ? p[c[i]] : dflt;
  }
};

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.0f ? v : v * slope; }

// Row-lane sums of one block -> partials[blockIdx.y][k][column]: the row lanes are added in lane order by the
// thread that owns the column's slot.
template <bool VEC>
__device__ void bn_block_reduce(const BnCols<VEC>& cs, int cl_lanes, int cols, const double (&a)[4],
                                const double (&b)[4], double* __restrict__ partials) {
  __shared__ double lds[2 * 4 * BN_THREADS];  // [row lane][slot][2]
  const int rl = threadIdx.x / cl_lanes;
  const int tile = 4 * cl_lanes;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = cs.slot(cl_lanes, i);
    lds[(rl * tile + s) * 2 + 0] = a[i];
    lds[(rl * tile + s) * 2 + 1] = b[i];
  }
  __syncthreads();
  const int rls = BN_THREADS / cl_lanes;
  for (int s = threadIdx.x; s < tile; s += BN_THREADS) {
    const int64_t col = (int64_t)blockIdx.x * tile + s;
    if (col >= cols) continue;
    double sa = 0.0, sb = 0.0;
    for (int r = 0; r < rls; ++r) {
      sa += lds[(r * tile + s) * 2 + 0];
      sb += lds[(r * tile + s) * 2 + 1];
    }
    partials[((int64_t)blockIdx.y * 2 + 0) * cols + col] = sa;
    partials[((int64_t)blockIdx.y * 2 + 1) * cols + col] = sb;
  }
}

// (a) per row block and column: sum x, sum x^2
template <bool VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows,
                                                              int cols, int cl_lanes, int64_t rpb,
                                                              double* __restrict__ partials) {
  const BnCols<VEC> cs(cl_lanes, cols);
  const int rls = BN_THREADS / cl_lanes;
  const int64_t r0 = (int64_t)blockIdx.y * rpb;
  const int64_t r1 = r0 + rpb < rows ? r0 + rpb : rows;
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  int64_t r = r0 + threadIdx.x / cl_lanes;
  // four rows' loads in flight, added in row order
  for (; r + 3 * (int64_t)rls < r1; r += 4 * (int64_t)rls) {
    float v[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cs.load(x + (r + (int64_t)k * rls) * ldx, v[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double d = (double)v[k][i];
        s1[i] += d;
        s2[i] = fma(d, d, s2[i]);
      }
  }
  for (; r < r1; r += rls) {
    float v[4];
    cs.load(x + r * ldx, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double d = (double)v[i];
      s1[i] += d;
      s2[i] = fma(d, d, s2[i]);
    }
  }
  bn_block_reduce<VEC>(cs, cl_lanes, cols, s1, s2, partials);
}

// (b) one thread per column: the partials in block order; mean, invstd, the running statistics
__global__ __launch_bounds__(BN_THREADS) void bn_stats_finalize_kernel(const double* __restrict__ partials, int64_t nb,
                                                                       int64_t rows, int cols, float eps,
                                                                       float momentum, float* running_mean,
                                                                       float* running_var,
                                                                       float* __restrict__ save_mean,
                                                                       float* __restrict__ save_invstd) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t b = 0; b < nb; ++b) {
    s1 += partials[(b * 2 + 0) * cols + c];
    s2 += partials[(b * 2 + 1) * cols + c];
  }
  const double n = (double)rows;
  const double mean = s1 / n;
  double var = s2 / n - mean * mean;
  var = var > 0.0 ? var : 0.0;
  save_mean[c] = (float)mean;
  save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  const double m = (double)momentum;
  if (running_mean) running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
  if (running_var) running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * var * (n / (n - 1.0)));
}

// (c) / eval: y = leaky(gamma * (x - mean) * invstd + beta).  EVAL: mean / invstd are the running mean and
// 1 / sqrt(running_var + eps), formed here.  Every thread reads its elements before it writes them and no two
// threads share one, so y may alias x.
template <bool VEC, bool EVAL>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const float* x, int64_t ldx, int64_t rows, int cols,
                                                              int cl_lanes, int64_t rpb,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ stat, float eps, float slope,
                                                              float* y, int64_t ldy) {
  const BnCols<VEC> cs(cl_lanes, cols);
  const int rls = BN_THREADS / cl_lanes;
  const int64_t r0 = (int64_t)blockIdx.y * rpb;
  const int64_t r1 = r0 + rpb < rows ? r0 + rpb : rows;
  float mu[4], sc[4], sh[4], ga[4];
  cs.vec(mean, 0.0f, mu);
  cs.vec(stat, 1.0f, sc);
  cs.vec(gamma, 1.0f, ga);
  cs.vec(beta, 0.0f, sh);
#pragma unroll
  for (int i = 0; i < 4; ++i) sc[i] = ga[i] * (EVAL ? 1.0f / sqrtf(sc[i] + eps) : sc[i]);
  for (int64_t r = r0 + threadIdx.x / cl_lanes; r < r1; r += rls) {
    float v[4];
    cs.load(x + r * ldx, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = leaky(fmaf(v[i] - mu[i], sc[i], sh[i]), slope);
    cs.store(y + r * ldy, v);
  }
}

// backward pass 1: per row block and column sum g, sum g * xhat; g = dy * (y > 0 ? 1 : slope)
template <bool VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_stats_kernel(const float* __restrict__ dy, int64_t lddy,
                                                                  const float* __restrict__ y, int64_t ldy,
                                                                  const float* __restrict__ x, int64_t ldx,
                                                                  int64_t rows, int cols, int cl_lanes, int64_t rpb,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, float slope,
                                                                  double* __restrict__ partials) {
  const BnCols<VEC> cs(cl_lanes, cols);
  const int rls = BN_THREADS / cl_lanes;
  const int64_t r0 = (int64_t)blockIdx.y * rpb;
  const int64_t r1 = r0 + rpb < rows ? r0 + rpb : rows;
  float mu[4], is[4];
  cs.vec(mean, 0.0f, mu);
  cs.vec(invstd, 1.0f, is);
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = r0 + threadIdx.x / cl_lanes; r < r1; r += rls) {
    float g[4], o[4], v[4];
    cs.load(dy + r * lddy, g);
    cs.load(y + r * ldy, o);
    cs.load(x + r * ldx, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double gd = (double)(o[i] > 0.0f ? g[i] : g[i] * slope);
      const double xh = ((double)v[i] - (double)mu[i]) * (double)is[i];
      s1[i] += gd;
      s2[i] = fma(gd, xh, s2[i]);
    }
  }
  bn_block_reduce<VEC>(cs, cl_lanes, cols, s1, s2, partials);
}

// backward finalize: dbeta = sum g, dgamma = sum g * xhat (written where asked for); their means over the rows go
// to `means` [2][cols] for pass 2
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_finalize_kernel(const double* __restrict__ partials, int64_t nb,
                                                                     int64_t rows, int cols,
                                                                     float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta,
                                                                     double* __restrict__ means) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t b = 0; b < nb; ++b) {
    s1 += partials[(b * 2 + 0) * cols + c];
    s2 += partials[(b * 2 + 1) * cols + c];
  }
  if (dbeta) dbeta[c] = (float)s1;
  if (dgamma) dgamma[c] = (float)s2;
  means[c] = s1 / (double)rows;
  means[cols + c] = s2 / (double)rows;
}

// backward pass 2: dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)); dx may alias dy (each element
// is read before it is written, by the one thread that owns it)
template <bool VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(const float* dy, int64_t lddy,
                                                                  const float* __restrict__ y, int64_t ldy,
                                                                  const float* __restrict__ x, int64_t ldx,
                                                                  int64_t rows, int cols, int cl_lanes, int64_t rpb,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, float slope,
                                                                  const double* __restrict__ means, float* dx,
                                                                  int64_t lddx) {
  const BnCols<VEC> cs(cl_lanes, cols);
  const int rls = BN_THREADS / cl_lanes;
  const int64_t r0 = (int64_t)blockIdx.y * rpb;
  const int64_t r1 = r0 + rpb < rows ? r0 + rpb : rows;
  float mu[4], is[4], ga[4], mg[4], mgx[4];
  cs.vec(mean, 0.0f, mu);
  cs.vec(invstd, 1.0f, is);
  cs.vec(gamma, 1.0f, ga);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    mg[i] = cs.ok[i] ? (float)means[cs.c[i]] : 0.0f;
    mgx[i] = cs.ok[i] ? (float)means[cols + cs.c[i]] : 0.0f;
    ga[i] *= is[i];
  }
  for (int64_t r = r0 + threadIdx.x / cl_lanes; r < r1; r += rls) {
    float g[4], o[4], v[4];
    cs.load(dy + r * lddy, g);
    cs.load(y + r * ldy, o);
    cs.load(x + r * ldx, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float ge = o[i] > 0.0f ? g[i] : g[i] * slope;
      const float xh = (v[i] - mu[i]) * is[i];
      g[i] = ga[i] * ((ge - mg[i]) - xh * mgx[i]);
    }
    cs.store(dx + r * lddx, g);
  }
}

bool bn_vec_ok(int64_t cols, std::initializer_list<int64_t> lds, std::initializer_list<const void*> ptrs) {
  if (cols % 4) return false;
  for (int64_t ld : lds)
    if (ld % 4) return false;
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % 16) return false;
  return true;
}

}  // namespace
}  // namespace grl

using namespace grl;

#define BN_LAUNCH(kernel, vec, ...)                                                                   \
  do {                                                                                                \
    if (vec)                                                                                          \
      hipLaunchKernelGGL((kernel<true>), grid, dim3(BN_THREADS), 0, st, __VA_ARGS__);                 \
    else                                                                                              \
      hipLaunchKernelGGL((kernel<false>), grid, dim3(BN_THREADS), 0, st, __VA_ARGS__);                \
  } while (0)

extern "C" size_t grl_bn_rows_workspace_size(int64_t rows, int32_t cols) {
  if (rows <= 0 || cols <= 0) return 0;
  return bn_ws_bytes(bn_geo(rows, cols), cols);
}

extern "C" int grl_bn_rows_fwd_train(const float* x, int64_t ldx, int64_t rows, int32_t cols, const float* gamma,
                                     const float* beta, float eps, float slope, float momentum, float* running_mean,
                                     float* running_var, float* y, int64_t ldy, float* save_mean, float* save_invstd,
                                     void* workspace, size_t ws_bytes, grl_stream_t stream) {
  TraceRange trace_("grl_bn_rows_fwd_train");
  GRL_CHECK_ARG(rows >= 0 && cols >= 0, "grl_bn_rows_fwd_train: negative size");
  GRL_CHECK_ARG(ldx >= cols && ldy >= cols, "grl_bn_rows_fwd_train: row strides below cols");
  if (rows == 0 || cols == 0) return GRL_OK;
  GRL_CHECK_ARG(rows >= 2, "grl_bn_rows_fwd_train: batch statistics need at least 2 rows (got %lld)",
                (long long)rows);
  GRL_CHECK_ARG(x && y && save_mean && save_invstd, "grl_bn_rows_fwd_train: NULL pointer");
  const BnGeo g = bn_geo(rows, cols);
  GRL_CHECK_ARG(workspace && ws_bytes >= bn_ws_bytes(g, cols) && reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
                "grl_bn_rows_fwd_train: workspace too small (%zu bytes, grl_bn_rows_workspace_size gives %zu) or "
                "not 8-B aligned",
                ws_bytes, bn_ws_bytes(g, cols));
  hipStream_t st = as_stream(stream);
  double* partials = static_cast<double*>(workspace);
  const dim3 grid((unsigned)g.nct, (unsigned)g.nb);
  BN_LAUNCH(bn_stats_kernel, bn_vec_ok(cols, {ldx}, {x}), x, ldx, rows, (int)cols, g.cl, g.rpb, partials);
  GRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((unsigned)ceil_div(cols, BN_THREADS)), dim3(BN_THREADS), 0, st,
                     partials, g.nb, rows, (int)cols, eps, momentum, running_mean, running_var, save_mean,
                     save_invstd);
  GRL_LAUNCH_CHECK();
  const bool vec = bn_vec_ok(cols, {ldx, ldy}, {x, y});
  if (vec)
    hipLaunchKernelGGL((bn_apply_kernel<true, false>), grid, dim3(BN_THREADS), 0, st, x, ldx, rows, (int)cols, g.cl,
                       g.rpb, gamma, beta, save_mean, save_invstd, eps, slope, y, ldy);
  else
    hipLaunchKernelGGL((bn_apply_kernel<false, false>), grid, dim3(BN_THREADS), 0, st, x, ldx, rows, (int)cols, g.cl,
                       g.rpb, gamma, beta, save_mean, save_invstd, eps, slope, y, ldy);
  GRL_LAUNCH_CHECK();
  return GRL_OK;
}

extern "C" int grl_bn_rows_fwd_eval(const float* x, int64_t ldx, int64_t rows, int32_t cols, const float* gamma,
                                    const float* beta, const float* running_mean, const float* running_var, float eps,
                                    float slope, float* y, int64_t ldy, grl_stream_t stream) {
  TraceRange trace_("grl_bn_rows_fwd_eval");
  GRL_CHECK_ARG(rows >= 0 && cols >= 0, "grl_bn_rows_fwd_eval: negative size");
  GRL_CHECK_ARG(ldx >= cols && ldy >= cols, "grl_bn_rows_fwd_eval: row strides below cols");
  if (rows == 0 || cols == 0) return GRL_OK;
  GRL_CHECK_ARG(x && y && running_mean && running_var, "grl_bn_rows_fwd_eval: NULL pointer");
  const BnGeo g = bn_geo(rows, cols);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)g.nct, (unsigned)g.nb);
  if (bn_vec_ok(cols, {ldx, ldy}, {x, y}))
    hipLaunchKernelGGL((bn_apply_kernel<true, true>), grid, dim3(BN_THREADS), 0, st, x, ldx, rows, (int)cols, g.cl,
                       g.rpb, gamma, beta, running_mean, running_var, eps, slope, y, ldy);
  else
    hipLaunchKernelGGL((bn_apply_kernel<false, true>), grid, dim3(BN_THREADS), 0, st, x, ldx, rows, (int)cols, g.cl,
                       g.rpb, gamma, beta, running_mean, running_var, eps, slope, y, ldy);
  GRL_LAUNCH_CHECK();
  return GRL_OK;
}

extern "C" int grl_bn_rows_bwd(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* x, int64_t ldx,
                               int64_t rows, int32_t cols, const float* gamma, const float* save_mean,
                               const float* save_invstd, float slope, float* dx, int64_t lddx, float* dgamma,
                               float* dbeta, void* workspace, size_t ws_bytes, grl_stream_t stream) {
  TraceRange trace_("grl_bn_rows_bwd");
  GRL_CHECK_ARG(rows >= 0 && cols >= 0, "grl_bn_rows_bwd: negative size");
  GRL_CHECK_ARG(lddy >= cols && ldy >= cols && ldx >= cols && lddx >= cols,
                "grl_bn_rows_bwd: row strides below cols");
  if (rows == 0 || cols == 0) return GRL_OK;
  GRL_CHECK_ARG(dy && y && x && dx && save_mean && save_invstd, "grl_bn_rows_bwd: NULL pointer");
  const BnGeo g = bn_geo(rows, cols);
  GRL_CHECK_ARG(workspace && ws_bytes >= bn_ws_bytes(g, cols) && reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
                "grl_bn_rows_bwd: workspace too small (%zu bytes, grl_bn_rows_workspace_size gives %zu) or not 8-B "
                "aligned",
                ws_bytes, bn_ws_bytes(g, cols));
  hipStream_t st = as_stream(stream);
  double* partials = static_cast<double*>(workspace);
  double* means = partials + g.nb * 2 * (int64_t)cols;
  const dim3 grid((unsigned)g.nct, (unsigned)g.nb);
  BN_LAUNCH(bn_bwd_stats_kernel, bn_vec_ok(cols, {lddy, ldy, ldx}, {dy, y, x}), dy, lddy, y, ldy, x, ldx, rows,
            (int)cols, g.cl, g.rpb, save_mean, save_invstd, slope, partials);
  GRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)ceil_div(cols, BN_THREADS)), dim3(BN_THREADS), 0, st,
                     partials, g.nb, rows, (int)cols, dgamma, dbeta, means);
  GRL_LAUNCH_CHECK();
  BN_LAUNCH(bn_bwd_apply_kernel, bn_vec_ok(cols, {lddy, ldy, ldx, lddx}, {dy, y, x, dx}), dy, lddy, y, ldy, x, ldx,
            rows, (int)cols, g.cl, g.rpb, gamma, save_mean, save_invstd, slope, means, dx, lddx);
  GRL_LAUNCH_CHECK();
  return GRL_OK;
}
