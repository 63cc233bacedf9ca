// Typed-CSR SpMM forward over a bf16 feature table (grl_typed_spmm_fwd_bf16).
//
// The contract of spmm_kernel<..., BWD=false> (spmm.hip) with one difference:
// the gathered table and the self-term rows are bf16 bits.  A gathered
// operand is x = uint_as_float(bits << 16) -- widening bf16 is exact -- and
// every output element runs the fp32 kernel's fmaf chain in CSR order into
// fp32 accumulators, so Z is bitwise the fp32 kernel's on the widened table
// while the gather moves half the bytes.
//
// Load shape: a lane owns 8 contiguous columns, one 16 B load.
//  * F > 256: one instruction fetches one row of up to 512 columns (1 KiB per
//    wave-instruction); wider rows are cut in 512-column blocks along grid.y;
//  * F <= 256: a row needs at most 32 lanes, so every gather instruction
//    fetches two edges' rows (lanes 0-31 edge j, lanes 32-63 edge j+1) and
//    v_permlane32_swap hands the second to lanes 0-31, which accumulate both
//    in CSR order -- the form of spmm_pair_kernel, for the reason stated there;
//  * X not 16 B-aligned, ldx % 8, F % 8, or Z not float4-storable: one bf16 per
//    lane per 64-column block (the fp32 kernel's VEC = 1 shape).
// Everything else -- one wavefront per work item on the persistent grid, 64
// edge indices per wave-load, ballot over the DropEdge weights, typed segments
// flushed on wave-uniform boundaries, non-temporal fp32 stores, hub rows as
// chunk partials summed in chunk order by a fixup -- is the fp32 kernel's.
#include <climits>

#include "grl_internal.h"

namespace grl {
namespace {

// Device view of a split plan (all null / zero when the graph is not split).
struct SplitDev {
  int threshold;  // INT_MAX: nothing is heavy
  int64_t num_chunks;
  const int32_t* chunk_begin;
  const int32_t* chunk_end;
  float* partials;
};

// CPL bf16 columns of one lane as loaded, and their exact fp32 widening.
template <int CPL>
struct BitsT;
template <>
struct BitsT<8> {
  using type = uint4;
};
template <>
struct BitsT<1> {
  using type = uint16_t;
};

__device__ __forceinline__ float bf_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf_hi(uint32_t p) { return __uint_as_float(p & 0xFFFF0000u); }

__device__ __forceinline__ void widen(const uint4& b, float (&x)[8]) {
  x[0] = bf_lo(b.x), x[1] = bf_hi(b.x), x[2] = bf_lo(b.y), x[3] = bf_hi(b.y);
  x[4] = bf_lo(b.z), x[5] = bf_hi(b.z), x[6] = bf_lo(b.w), x[7] = bf_hi(b.w);
}
__device__ __forceinline__ void widen(const uint16_t& b, float (&x)[1]) { x[0] = bf_lo(b); }

// Non-temporal stores, as spmm.hip's: Z is written once and should not evict
// gathered rows from L2 / the MALL.
using f4v = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ void vstore(float* p, const float (&v)[8]) {
  const f4v a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
  __builtin_nontemporal_store(a, reinterpret_cast<f4v*>(p));
  __builtin_nontemporal_store(b, reinterpret_cast<f4v*>(p) + 1);
}
__device__ __forceinline__ void vstore(float* p, const float (&v)[1]) { __builtin_nontemporal_store(v[0], p); }

template <int CPL>
__device__ __forceinline__ void vzero(float (&a)[CPL]) {
#pragma unroll
  for (int i = 0; i < CPL; ++i) a[i] = 0.f;
}
template <int CPL>
__device__ __forceinline__ void vfma(float (&acc)[CPL], float w, const float (&x)[CPL]) {
#pragma unroll
  for (int i = 0; i < CPL; ++i) acc[i] = __builtin_fmaf(w, x[i], acc[i]);
}
// the self term: w * x, or zeros where DropEdge took it
template <int CPL>
__device__ __forceinline__ void vself(float (&x)[CPL], float w) {
#pragma unroll
  for (int i = 0; i < CPL; ++i) x[i] = w != 0.0f ? w * x[i] : 0.f;
}

// One row per gather instruction: CPL = 8 for rows of 257..512 columns per
// grid.y block, CPL = 1 (NV 64-column blocks per wave) for the scalar form.
template <int CPL, int NV, int U, bool VALS>
__global__ __launch_bounds__(256) void spmm_bf16_kernel(
    int64_t num_rows, int S, int hs, const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
    const float* __restrict__ vals, uint64_t edge_base, uint64_t self_base, int64_t self_row0,
    const uint16_t* __restrict__ src, int64_t lds, int F, float* __restrict__ out, int64_t ldo, int zseg, DropDev de,
    SplitDev sp) {
  using bits_t = typename BitsT<CPL>::type;
  de = resolve_key(de);
  const int lane = threadIdx.x & 63;
  const int cbase = blockIdx.y * (64 * CPL * NV);
  int coff[NV];
  bool cval[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    coff[k] = cbase + (k * 64 + lane) * CPL;
    cval[k] = coff[k] < F;
  }
  const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + uniform_i(threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t num_items = sp.num_chunks + num_rows;

  for (int64_t item = wave0; item < num_items; item += nwaves) {
    float acc[NV][CPL];
#pragma unroll
    for (int k = 0; k < NV; ++k) vzero(acc[k]);
    int pv, nseg;
    float* obase;
    if (item < sp.num_chunks) {
      // ---- chunk of a heavy segment -> partial row ----------------------------
      const int64_t c = item;
      pv = lane == 0 ? sp.chunk_begin[c] : (lane == 1 ? sp.chunk_end[c] : 0);
      nseg = 1;
      obase = sp.partials + c * F;
    } else {
      const int64_t n = item - sp.num_chunks;
      float* orow = out + n * ldo;
      pv = lane <= S ? ptr[n * S + lane] : 0;
      nseg = S;
      const bool heavy = readlane_i(pv, nseg) - readlane_i(pv, 0) > sp.threshold;
      // ---- self term (identity block of A_pre) --------------------------------
      if (hs) {
        float w = 1.0f;
        if (de.active && de.drop_self) w = dropedge_weight(de, 1.0f, self_base + (uint64_t)n);
        const uint16_t* srow = src + (n + self_row0) * lds;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          if (cval[k]) {
            float x[CPL];
            widen(*reinterpret_cast<const bits_t*>(srow + coff[k]), x);
            vself(x, w);
            vstore(orow + coff[k], x);
          }
        }
      }
      if (heavy) continue;  // typed segments come from the chunk partials (fixup)
      obase = orow + hs * zseg;
    }

    // ---- gather-accumulate over the item's edges --------------------------
    const int e_begin = readlane_i(pv, 0);
    const int e_end = readlane_i(pv, nseg);
    int t = 0;
    int seg_end = readlane_i(pv, 1);
    for (int c0 = e_begin; c0 < e_end; c0 += 64) {
      const int cnt = min(64, e_end - c0);
      int sidx = 0;
      float w = 0.0f;
      if (lane < cnt) {
        sidx = idx[c0 + lane];
        const float v = VALS ? vals[c0 + lane] : 1.0f;
        w = v;
        if (de.active) w = dropedge_weight(de, v, edge_base + (uint64_t)(c0 + lane));
      }
      uint64_t kept = __ballot(w != 0.0f);
      while (kept) {
        int jj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (kept) {
            jj[u] = __builtin_ctzll(kept);
            kept &= kept - 1;
          } else {
            jj[u] = -1;
          }
        }
        bits_t xv[U][NV];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (jj[u] >= 0) {
            const int r = readlane_i(sidx, jj[u]);
            const uint16_t* srow = src + (int64_t)r * lds;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
              if (cval[k])
                xv[u][k] = *reinterpret_cast<const bits_t*>(srow + coff[k]);
              else
                xv[u][k] = bits_t{};
            }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (jj[u] >= 0) {
            const int e = c0 + jj[u];
            while (e >= seg_end) {  // flush finished segments (wave-uniform)
#pragma unroll
              for (int k = 0; k < NV; ++k) {
                if (cval[k]) vstore(obase + t * zseg + coff[k], acc[k]);
                vzero(acc[k]);
              }
              ++t;
              seg_end = readlane_i(pv, t + 1);
            }
            const float wj = readlane_f(w, jj[u]);
#pragma unroll
            for (int k = 0; k < NV; ++k) {
              float x[CPL];
              widen(xv[u][k], x);
              vfma(acc[k], wj, x);
            }
          }
        }
      }
    }
    // ---- flush the remaining (possibly empty) segments -------------------
    for (; t < nseg; ++t) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        if (cval[k]) vstore(obase + t * zseg + coff[k], acc[k]);
        vzero(acc[k]);
      }
    }
  }
}

// Rows of at most 256 columns: two edges per gather instruction.  Lanes 32-63
// only fetch; stores and the self term are lanes 0-31's.  The rows change
// halves as loaded (4 dwords of bf16 bits, not 8 widened floats).
__device__ __forceinline__ uint32_t swap_halves(uint32_t x) {
  return __builtin_amdgcn_permlane32_swap(x, x, false, false)[1];
}

// Bounded to 8 waves per SIMD: unbounded it takes 66 VGPRs (7 waves) and ran
// C3 in 4.10 ms against 3.58 ms (p = 0.3: 3.43 / 3.08 ms).  The same bound on
// spmm_bf16_kernel, which already fits 8 waves, cost 5 % at F = 512.
template <int U, bool VALS>
__global__ __launch_bounds__(256, 8) void spmm_bf16_pair_kernel(
    int64_t num_rows, int S, int hs, const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
    const float* __restrict__ vals, uint64_t edge_base, uint64_t self_base, int64_t self_row0,
    const uint16_t* __restrict__ src, int64_t lds, int F, float* __restrict__ out, int64_t ldo, int zseg, DropDev de,
    SplitDev sp) {
  de = resolve_key(de);
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5;
  const int coff = (lane & 31) * 8;
  const bool ld_ok = coff < F;
  const bool own = half == 0 && ld_ok;
  const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + uniform_i(threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t num_items = sp.num_chunks + num_rows;

  for (int64_t item = wave0; item < num_items; item += nwaves) {
    float acc[8];
    vzero(acc);
    int pv, nseg;
    float* obase;
    if (item < sp.num_chunks) {
      const int64_t c = item;
      pv = lane == 0 ? sp.chunk_begin[c] : (lane == 1 ? sp.chunk_end[c] : 0);
      nseg = 1;
      obase = sp.partials + c * F;
    } else {
      const int64_t n = item - sp.num_chunks;
      float* orow = out + n * ldo;
      pv = lane <= S ? ptr[n * S + lane] : 0;
      nseg = S;
      const bool heavy = readlane_i(pv, nseg) - readlane_i(pv, 0) > sp.threshold;
      if (hs) {
        float w = 1.0f;
        if (de.active && de.drop_self) w = dropedge_weight(de, 1.0f, self_base + (uint64_t)n);
        if (own) {
          float x[8];
          widen(*reinterpret_cast<const uint4*>(src + (n + self_row0) * lds + coff), x);
          vself(x, w);
          vstore(orow + coff, x);
        }
      }
      if (heavy) continue;
      obase = orow + hs * zseg;
    }

    const int e_begin = readlane_i(pv, 0);
    const int e_end = readlane_i(pv, nseg);
    int t = 0;
    int seg_end = readlane_i(pv, 1);
    for (int c0 = e_begin; c0 < e_end; c0 += 64) {
      const int cnt = min(64, e_end - c0);
      int sidx = 0;
      float w = 0.0f;
      if (lane < cnt) {
        sidx = idx[c0 + lane];
        const float v = VALS ? vals[c0 + lane] : 1.0f;
        w = v;
        if (de.active) w = dropedge_weight(de, v, edge_base + (uint64_t)(c0 + lane));
      }
      uint64_t kept = __ballot(w != 0.0f);
      while (kept) {
        int jj[2 * U];
#pragma unroll
        for (int u = 0; u < 2 * U; ++u) {
          if (kept) {
            jj[u] = __builtin_ctzll(kept);
            kept &= kept - 1;
          } else {
            jj[u] = -1;
          }
        }
        uint4 xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int ja = jj[2 * u], jb = jj[2 * u + 1];
          if (ja >= 0) {
            const int ra = readlane_i(sidx, ja);
            const int rb = jb >= 0 ? readlane_i(sidx, jb) : ra;
            const int r = half ? rb : ra;
            if (ld_ok && (half == 0 || jb >= 0))
              xv[u] = *reinterpret_cast<const uint4*>(src + (int64_t)r * lds + coff);
            else
              xv[u] = uint4{};
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int j = jj[2 * u + h];
            if (j < 0) continue;
            const int e = c0 + j;
            while (e >= seg_end) {  // flush finished segments (wave-uniform)
              if (own) vstore(obase + t * zseg + coff, acc);
              vzero(acc);
              ++t;
              seg_end = readlane_i(pv, t + 1);
            }
            const float wj = readlane_f(w, j);
            uint4 b = xv[u];
            if (h == 1) b = make_uint4(swap_halves(b.x), swap_halves(b.y), swap_halves(b.z), swap_halves(b.w));
            float x[8];
            widen(b, x);
            vfma(acc, wj, x);
          }
        }
      }
    }
    for (; t < nseg; ++t) {
      if (own) vstore(obase + t * zseg + coff, acc);
      vzero(acc);
    }
  }
}

// Heavy segment h: out = sum of its chunk partials in chunk order, one
// wavefront per heavy segment (the forward case of spmm_fixup_kernel).
template <int VEC>
__global__ __launch_bounds__(256) void spmm_bf16_fixup_kernel(
    int64_t num_heavy, const int32_t* __restrict__ heavy_seg, const int32_t* __restrict__ heavy_cptr,
    const float* __restrict__ partials, int S, int hs, int F, float* __restrict__ out, int64_t ldo, int zseg) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + uniform_i(threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t h = wave0; h < num_heavy; h += nwaves) {
    const int64_t s = heavy_seg[h];
    const int64_t n = s / S, t = s % S;
    const int c_begin = heavy_cptr[h], c_end = heavy_cptr[h + 1];
    float* orow = out + n * ldo + (hs + t) * zseg;
    for (int col = lane * VEC; col < F; col += 64 * VEC) {
      if constexpr (VEC == 4) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = c_begin; c < c_end; ++c) {
          const float4 v = *reinterpret_cast<const float4*>(partials + (int64_t)c * F + col);
          acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
        }
        *reinterpret_cast<float4*>(orow + col) = acc;
      } else {
        float acc = 0.f;
        for (int c = c_begin; c < c_end; ++c) acc += partials[(int64_t)c * F + col];
        orow[col] = acc;
      }
    }
  }
}

int to_split_dev(const GrlSplitPlan* plan, int F, SplitDev& sp) {
  sp = SplitDev{INT_MAX, 0, nullptr, nullptr, nullptr};
  if (!plan) return GRL_OK;
  GRL_CHECK_ARG(plan->threshold >= 0 && plan->chunk_edges > 0 && plan->num_heavy >= 0 && plan->num_chunks >= 0,
                "split plan: bad threshold/chunk_edges/counts");
  if (plan->num_chunks > 0) {
    GRL_CHECK_ARG(plan->chunk_begin && plan->chunk_end && plan->partials, "split plan: NULL chunk arrays");
    if (plan->partials_capacity < plan->num_chunks * (int64_t)F)
      GRL_FAIL(GRL_E_WORKSPACE, "split plan: partials hold %lld floats, need %lld", (long long)plan->partials_capacity,
               (long long)(plan->num_chunks * (int64_t)F));
  }
  GRL_CHECK_ARG(plan->num_heavy == 0 || (plan->heavy_seg && plan->heavy_cptr), "split plan: NULL heavy arrays");
  sp.threshold = plan->threshold;
  sp.num_chunks = plan->num_chunks;
  sp.chunk_begin = plan->chunk_begin;
  sp.chunk_end = plan->chunk_end;
  sp.partials = plan->partials;
  return GRL_OK;
}

int launch_spmm_bf16(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int F, int64_t self_row0, float* Z,
                     int64_t ldz, int zseg, const DropDev& de, hipStream_t stream) {
  SplitDev sp;
  const int rc = to_split_dev(g->split, F, sp);
  if (rc) return rc;
  const int S = g->num_types, hs = g->has_self ? 1 : 0;
  // 16 B loads of X and float4 stores of Z (the partials are F floats apart: F % 8 covers them)
  const bool vec = al16(X) && al16(Z) && ldx % 8 == 0 && F % 8 == 0 && ldz % 4 == 0 && zseg % 4 == 0;
  const int nv = F <= 64 ? 1 : (F <= 128 ? 2 : 4);
  const int ycols = vec ? 512 : 64 * nv;
  const int64_t items = g->num_rows + sp.num_chunks;
  const int64_t cap = (int64_t)device_cu_count() * opt(OPT_SPMM_BLOCKS_PER_CU);  // 4-wave blocks per CU in flight
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(items, 4), cap), (unsigned)ceil_div(F, ycols));
  const dim3 block(256);
#define GRL_BF16_LAUNCH(...)                                                                                     \
  hipLaunchKernelGGL((__VA_ARGS__), grid, block, 0, stream, g->num_rows, S, hs, g->rowptr, g->colidx, g->vals,   \
                     g->edge_id_base, g->self_id_base, self_row0, X, ldx, F, Z, ldz, zseg, de, sp)
  if (vec && F <= 256) {
    if (g->vals) GRL_BF16_LAUNCH(spmm_bf16_pair_kernel<8, true>); else GRL_BF16_LAUNCH(spmm_bf16_pair_kernel<8, false>);
  } else if (vec) {
    if (g->vals) GRL_BF16_LAUNCH(spmm_bf16_kernel<8, 1, 8, true>); else GRL_BF16_LAUNCH(spmm_bf16_kernel<8, 1, 8, false>);
  } else if (nv == 1) {
    if (g->vals) GRL_BF16_LAUNCH(spmm_bf16_kernel<1, 1, 8, true>); else GRL_BF16_LAUNCH(spmm_bf16_kernel<1, 1, 8, false>);
  } else if (nv == 2) {
    if (g->vals) GRL_BF16_LAUNCH(spmm_bf16_kernel<1, 2, 8, true>); else GRL_BF16_LAUNCH(spmm_bf16_kernel<1, 2, 8, false>);
  } else {
    if (g->vals) GRL_BF16_LAUNCH(spmm_bf16_kernel<1, 4, 8, true>); else GRL_BF16_LAUNCH(spmm_bf16_kernel<1, 4, 8, false>);
  }
#undef GRL_BF16_LAUNCH
  GRL_LAUNCH_CHECK();
  const GrlSplitPlan* plan = g->split;
  if (plan && plan->num_heavy > 0) {
    const dim3 fgrid((unsigned)std::min<int64_t>(ceil_div(plan->num_heavy, 4), cap));
    if (vec)
      hipLaunchKernelGGL(spmm_bf16_fixup_kernel<4>, fgrid, block, 0, stream, plan->num_heavy, plan->heavy_seg,
                         plan->heavy_cptr, plan->partials, S, hs, F, Z, ldz, zseg);
    else
      hipLaunchKernelGGL(spmm_bf16_fixup_kernel<1>, fgrid, block, 0, stream, plan->num_heavy, plan->heavy_seg,
                         plan->heavy_cptr, plan->partials, S, hs, F, Z, ldz, zseg);
    GRL_LAUNCH_CHECK();
  }
  return GRL_OK;
}

}  // namespace
}  // namespace grl

using namespace grl;

extern "C" int grl_typed_spmm_fwd_bf16(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F,
                                       int64_t self_col0, float* Z, int64_t ldz, int32_t zseg,
                                       const GrlDropEdge* de, grl_stream_t stream) {
  TraceRange trace_("grl_typed_spmm_fwd_bf16");
  const int rc = csr_fwd_check("grl_typed_spmm_fwd_bf16", g, F, ldx, X && Z);
  if (rc) return rc;
  GRL_CHECK_ARG(zseg >= F && self_col0 >= 0, "grl_typed_spmm_fwd_bf16: need zseg >= F, self_col0 >= 0 (zseg=%d "
                "self_col0=%lld)", zseg, (long long)self_col0);
  GRL_CHECK_ARG(ldz >= (int64_t)(segments(g) - 1) * zseg + F,
                "grl_typed_spmm_fwd_bf16: ldz %lld too small for %d segments of stride %d", (long long)ldz,
                segments(g), zseg);
  if (g->num_rows == 0) return GRL_OK;
  return launch_spmm_bf16(g, X, ldx, F, self_col0 + g->self_row0, Z, ldz, zseg, to_dev(de), as_stream(stream));
}
