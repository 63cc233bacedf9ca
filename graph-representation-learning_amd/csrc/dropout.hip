// Feature dropout keyed on (seed, call, global row, column).
//
// Replaces nn.Dropout(0.5) on node-feature rows (gnn/models/networks/
// drop_robust_gcn.py:64,77,81,86,100).  The reference draws the mask from
// torch's generator over the tensor it is given, so a node-range shard of
// the graph could not reproduce the one-GPU mask of its rows, and ranks
// seeded alike would draw the same pattern over different rows.  Here the
// mask of element (r, c) is a counter hash of the global element id
// (row0 + r) * cols + c under the DropEdge key (seed, call): the same bits
// for a row wherever it is computed, and any row block's mask is computable
// on its own.  The backward is the same map applied to the gradient.
//
// HBM-bound elementwise pass: rows * cols * 8 bytes (one read, one write);
// the bf16 form (grl_feature_dropout_bf16) half of that.
#include <type_traits>

#include "grl_internal.h"

namespace grl {
namespace {

// out[r][c] = keep(row0 + r, c) ? x[r][c] * scale : 0; cols % 4 == 0 with
// 16-B aligned rows take the float4 form (one hash per element either way)
template <bool VEC>
__global__ __launch_bounds__(256) void feature_dropout_kernel(const float* __restrict__ x, int64_t ldx,
                                                              float* __restrict__ out, int64_t ldo, int64_t rows,
                                                              int cols, int64_t row0, DropDev d) {
  d = resolve_key(d);
  const int64_t per_row = VEC ? cols / 4 : cols;
  const int64_t n = rows * per_row;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / per_row;
    const int64_t j = i - r * per_row;
    const uint64_t id = (uint64_t)(row0 + r) * (uint64_t)cols;
    if (VEC) {
      float4 v = *reinterpret_cast<const float4*>(x + r * ldx + 4 * j);
      const uint64_t e = id + 4 * (uint64_t)j;
      v.x = dropedge_weight(d, v.x, e);
      v.y = dropedge_weight(d, v.y, e + 1);
      v.z = dropedge_weight(d, v.z, e + 2);
      v.w = dropedge_weight(d, v.w, e + 3);
      *reinterpret_cast<float4*>(out + r * ldo + 4 * j) = v;
    } else {
      out[r * ldo + j] = dropedge_weight(d, x[r * ldx + j], id + (uint64_t)j);
    }
  }
}

// feature_dropout_kernel over bf16 bits (grl_feature_dropout_bf16): the same
// element ids, hash and keep rule, each value widened (exact), weighted in fp32
// as there and rounded once to nearest even -- bitwise that kernel on the
// widened x, rounded.  An inactive record copies the bits.  V = columns per
// lane: 8 (one 16-B load), 4 (8 B) or 1; the host picks by alignment, every
// form gives the same bits.  Every lane reads its columns before it writes
// them and no two lanes share one, so out may alias x.
template <int V>
__global__ __launch_bounds__(256) void feature_dropout_bf16_kernel(const uint16_t* x, int64_t ldx, uint16_t* out,
                                                                   int64_t ldo, int64_t rows, int cols, int64_t row0,
                                                                   DropDev d) {
  d = resolve_key(d);
  const int64_t per_row = cols / V;
  const int64_t n = rows * per_row;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / per_row;
    const int64_t j = i - r * per_row;
    const uint64_t e = (uint64_t)(row0 + r) * (uint64_t)cols + (uint64_t)V * (uint64_t)j;
    if constexpr (V == 1) {
      const uint16_t h = x[r * ldx + j];
      out[r * ldo + j] =
          d.active ? (uint16_t)cvt_pk_bf16(dropedge_weight(d, __uint_as_float((uint32_t)h << 16), e), 0.0f) : h;
    } else {
      using vec_t = typename std::conditional<V == 8, uint4, uint2>::type;
      union {
        vec_t v;
        uint32_t w[V / 2];
      } u;
      u.v = *reinterpret_cast<const vec_t*>(x + r * ldx + V * j);
      if (d.active) {
#pragma unroll
        for (int k = 0; k < V / 2; ++k) {
          const float lo = dropedge_weight(d, __uint_as_float(u.w[k] << 16), e + 2 * k);
          const float hi = dropedge_weight(d, __uint_as_float(u.w[k] & 0xFFFF0000u), e + 2 * k + 1);
          u.w[k] = cvt_pk_bf16(lo, hi);
        }
      }
      *reinterpret_cast<vec_t*>(out + r * ldo + V * j) = u.v;
    }
  }
}

template <int V>
void launch_feature_dropout_bf16(const uint16_t* x, int64_t ldx, uint16_t* out, int64_t ldo, int64_t rows, int cols,
                                 int64_t row0, const DropDev& d, hipStream_t st) {
  const int64_t n = rows * (cols / V);
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, 256), 8 * 1024);
  hipLaunchKernelGGL(feature_dropout_bf16_kernel<V>, dim3(grid), dim3(256), 0, st, x, ldx, out, ldo, rows, cols, row0,
                     d);
}

}  // namespace
}  // namespace grl

using namespace grl;

extern "C" int grl_feature_dropout_bf16(const uint16_t* x, int64_t ldx, uint16_t* out, int64_t ldo, int64_t rows,
                                        int32_t cols, int64_t row0, const GrlDropEdge* de, grl_stream_t stream) {
  TraceRange trace_("grl_feature_dropout_bf16");
  GRL_CHECK_ARG(rows >= 0 && cols >= 0 && row0 >= 0, "grl_feature_dropout_bf16: negative size");
  GRL_CHECK_ARG(ldx >= cols && ldo >= cols, "grl_feature_dropout_bf16: row strides below cols");
  if (rows == 0 || cols == 0) return GRL_OK;
  GRL_CHECK_ARG(x && out, "grl_feature_dropout_bf16: NULL pointer");
  const uintptr_t at = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out);
  GRL_CHECK_ARG(at % 2 == 0, "grl_feature_dropout_bf16: x and out must be 2-B aligned");
  const DropDev d = to_dev(de);
  // 16 B a lane (8 columns) where pointers and strides keep every lane's load on that grid, else 8 B (4), else 2 B
  const int64_t sizes = (int64_t)cols | ldx | ldo;
  hipStream_t st = as_stream(stream);
  if (at % 16 == 0 && sizes % 8 == 0)
    launch_feature_dropout_bf16<8>(x, ldx, out, ldo, rows, (int)cols, row0, d, st);
  else if (at % 8 == 0 && sizes % 4 == 0)
    launch_feature_dropout_bf16<4>(x, ldx, out, ldo, rows, (int)cols, row0, d, st);
  else
    launch_feature_dropout_bf16<1>(x, ldx, out, ldo, rows, (int)cols, row0, d, st);
  GRL_LAUNCH_CHECK();
  return GRL_OK;
}

extern "C" int grl_feature_dropout(const float* x, int64_t ldx, float* out, int64_t ldo, int64_t rows, int32_t cols,
                                   int64_t row0, const GrlDropEdge* de, grl_stream_t stream) {
  TraceRange trace_("grl_feature_dropout");
  GRL_CHECK_ARG(rows >= 0 && cols >= 0 && row0 >= 0, "grl_feature_dropout: negative size");
  GRL_CHECK_ARG(ldx >= cols && ldo >= cols, "grl_feature_dropout: row strides below cols");
  if (rows == 0 || cols == 0) return GRL_OK;
  GRL_CHECK_ARG(x && out, "grl_feature_dropout: NULL pointer");
  const DropDev d = to_dev(de);
  const bool vec = cols % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(out) % 16 == 0;
  const int64_t n = rows * (vec ? cols / 4 : cols);
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, 256), 8 * 1024);
  hipStream_t st = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(feature_dropout_kernel<true>, dim3(grid), dim3(256), 0, st, x, ldx, out, ldo, rows, (int)cols,
                       row0, d);
  else
    hipLaunchKernelGGL(feature_dropout_kernel<false>, dim3(grid), dim3(256), 0, st, x, ldx, out, ldo, rows, (int)cols,
                       row0, d);
  GRL_LAUNCH_CHECK();
  return GRL_OK;
}
