// Internal helpers shared by the gfx950 translation units of libgrl.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>

#include "grl.h"

#include <rocprofiler-sdk-roctx/roctx.h>

namespace grl {

// ---- thread-local error string (grl_last_error) --------------------------
void set_error(const char* fmt, ...);

#define GRL_FAIL(code, ...)          \
  do {                               \
    ::grl::set_error(__VA_ARGS__);   \
    return (code);                   \
  } while (0)

#define GRL_CHECK_ARG(cond, ...)                         \
  do {                                                   \
    if (!(cond)) GRL_FAIL(GRL_E_INVALID, __VA_ARGS__);   \
  } while (0)

#define GRL_HIP(call)                                                        \
  do {                                                                       \
    hipError_t _e = (call);                                                  \
    if (_e != hipSuccess)                                                    \
      GRL_FAIL(GRL_E_HIP, "%s failed: %s (%s:%d)", #call,                    \
               hipGetErrorString(_e), __FILE__, __LINE__);                   \
  } while (0)

// Launch-error check after <<<>>> (no device sync: stream-ordered API).
#define GRL_LAUNCH_CHECK() GRL_HIP(hipGetLastError())

inline hipStream_t as_stream(grl_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// ---- DropEdge counter hash -------------------------------------------------
// splitmix64 finalizer (Steele, Lea, Flood 2014).  The same function is
// restated independently in oracle/grl_oracle.c and oracle/hash.py.
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__host__ __device__ __forceinline__ uint64_t dropedge_key(uint64_t seed, uint64_t call) {
  return mix64(mix64(seed ^ 0x6A09E667F3BCC909ull) + call * 0x9E3779B97F4A7C15ull);
}

__host__ __device__ __forceinline__ uint32_t dropedge_bits(uint64_t key, uint64_t id) {
  return static_cast<uint32_t>(mix64(key ^ (id * 0xD1B54A32D192ED03ull)) >> 32);
}

// Synthetic-graph candidate hash: 64 random bits for (seed, candidate, lane).
__host__ __device__ __forceinline__ uint64_t synth_bits(uint64_t seed, uint64_t k, uint32_t lane) {
  return mix64(mix64(seed + 0x243F6A8885A308D3ull * (uint64_t)(lane + 1)) ^ (k * 0x9E3779B97F4A7C15ull));
}

// Segments of a Z row: the identity block (has_self) and one per edge type.
inline int segments(int num_types, int has_self) { return num_types + (has_self ? 1 : 0); }
inline int segments(const GrlTypedCsr* g) { return segments(g->num_types, g->has_self); }

inline bool al16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// ---- what the GraphConv layer (graphconv.hip: the grl_graphconv_* entry
// points and their dispatch) takes from the primitives ----------------------
// spmm.hip.  The argument check the forward entry points over a typed CSR
// share (grl_typed_spmm_fwd, _fwd_slice, grl_graphconv_fwd, _fwd_train): the
// graph, its type count, F and ldx, and -- for a graph with rows -- the
// pointers (`ptrs`: the entry point's own are non-NULL), nnz and self_row0.
int csr_fwd_check(const char* who, const GrlTypedCsr* g, int F, int64_t ldx, bool ptrs);
// Row-range typed-SpMM forward: grl_graphconv_fwd's row chunks.
int spmm_fwd_rows(const GrlTypedCsr* g, int64_t r0, int64_t rows, const float* X, int64_t ldx, int F, float* Z,
                  const GrlDropEdge* de, hipStream_t st);

// linear.hip.  Whether an [M, K] x [K, N] product chosen for max(M,
// path_rows) rows takes the x6 GEMM, and the bytes of W's planes if so (else
// 0); W [K, N] row-major split into those planes; the x6 GEMM of `rows` rows
// of A [rows, K] on planes already split (out [rows, N] contiguous), whose
// bits do not depend on `rows`; LB_M, its row tile.
constexpr int LB_M = 256;
bool x6_path_ok(int64_t M, int64_t path_rows, int64_t N, int64_t K);
size_t x6_ws_bytes_p(int64_t M, int64_t path_rows, int64_t N, int64_t K);
int x6_split_w(const float* W, int64_t K, int64_t N, uint16_t* planes, hipStream_t st);
int x6_gemm_rows(const float* A, int64_t rows, int64_t K, const uint16_t* planes, int64_t N, const float* bias,
                 int relu, float* out, hipStream_t st);

// Plain-data copy of GrlDropEdge passed by value to kernels.
struct DropDev {
  uint64_t key;
  uint32_t threshold;
  float scale;
  int32_t active;
  int32_t drop_self;
  const uint64_t* seed_dev;  // non-null: key = dropedge_key(*seed_dev, call) (resolve_key)
  uint64_t call;
};

inline DropDev to_dev(const GrlDropEdge* de) {
  DropDev d{0, 0, 1.0f, 0, 0, nullptr, 0};
  if (de && de->active) {
    d.key = de->key;
    d.threshold = de->threshold;
    d.scale = de->scale;
    d.active = 1;
    d.drop_self = de->drop_self;
    d.seed_dev = de->seed_dev;
    d.call = de->call_id;
  }
  return d;
}

// Device-resident seed: every kernel taking a DropDev resolves its key once
// at entry (one uniform 8-byte load; a graph replay sees the seed written
// before it on the same stream).
__device__ __forceinline__ DropDev resolve_key(DropDev d) {
  if (d.active && d.seed_dev) d.key = dropedge_key(*d.seed_dev, d.call);
  return d;
}

// weight of an entry with value v and global id `id` under DropEdge d
__device__ __forceinline__ float dropedge_weight(const DropDev& d, float v, uint64_t id) {
  if (!d.active) return v;
  return dropedge_bits(d.key, id) >= d.threshold ? v * d.scale : 0.0f;
}

__device__ __forceinline__ int readlane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }

// two fp32 -> one dword of two bf16 (lo in bits 15:0), each rounded to nearest even: the library's one
// fp32 -> bf16 rounding (the bf16-output GraphConv epilogue, the bf16 feature dropout, the scaled ReLU mask pass)
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// lane l ^ 1's value (a DPP move within the quad, no LDS): the bf16-output epilogues' lane pairs trade one
// value of each register pair with it and store dwords of two adjacent columns (graphconv_ws_body.inc,
// gemm_x6_kernel's EPI_BF16)
__device__ __forceinline__ float swap_lane_pair(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));  // quad_perm [1, 0, 3, 2]
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// roctx range around a C-ABI entry point: `rocprofv3 --marker-trace` shows
// where host time goes between kernels (a no-op call without a profiler).
struct TraceRange {
  explicit TraceRange(const char* name) { roctxRangePushA(name); }
  ~TraceRange() { roctxRangePop(); }
  TraceRange(const TraceRange&) = delete;
  TraceRange& operator=(const TraceRange&) = delete;
};

// Number of CUs of the current device (cached per process).
int device_cu_count();

// Path options (grl_set_option / grl_get_option, include/grl.h): the test and
// A/B hooks that select among kernel forms of one entry point.  Defaults are
// the production choices; nothing in the library reads the environment.
// One entry per option: X(enumerator, name, default, lo, hi).
#define GRL_OPTIONS(X)                                                                    \
  /* 1: split-bf16 (x6) GEMMs where sized for them; 0: fp32-MFMA kernels */               \
  X(OPT_GEMM_X6, "gemm_x6", 1, 0, 1)                                                      \
  /* 1: one-kernel GraphConv forward where eligible; 0: SpMM + GEMM */                    \
  X(OPT_GRAPHCONV_FUSED, "graphconv_fused", 1, 0, 1)                                      \
  /* 1: one-kernel GraphConv data gradient (read by the host layer) */                    \
  X(OPT_GRAPHCONV_FUSED_BWD, "graphconv_fused_bwd", 1, 0, 1)                              \
  /* 1: grl_graphconv_bwd_data_bf16 eligible (bf16 gradient table, bf16 dX); 0: never */  \
  X(OPT_GRAPHCONV_BWD_BF16, "graphconv_bwd_bf16", 1, 0, 1)                                \
  /* 1: grl_linear_bwd_weight_bf16g eligible (dW from a bf16 gradient); 0: never */       \
  X(OPT_DW_BF16G, "dw_bf16g", 1, 0, 1)                                                    \
  /* 1: grl_linear_bwd_weight_bf16zg eligible (dW from a bf16 Z and gradient); 0: never */ \
  X(OPT_DW_BF16Z, "dw_bf16z", 1, 0, 1)                                                    \
  /* 1: grl_linear_fwd_bf16x eligible (forward GEMM over a bf16 X); 0: never */            \
  X(OPT_LINEAR_BF16X, "linear_bf16x", 1, 0, 1)                                            \
  /* 1: grl_linear_bwd_weight_bf16z eligible (dW from a bf16 Z and an fp32 gradient); 0: never */ \
  X(OPT_DW_BF16Z_F32G, "dw_bf16z_f32g", 1, 0, 1)                                          \
  /* 1: grl_linear_fwd_to_bf16 eligible (the x6 forward GEMM storing bf16 rows); 0: never */ \
  X(OPT_LINEAR_OUT_BF16, "linear_out_bf16", 1, 0, 1)                                      \
  /* 1: persistent warp-specialized one-kernel form; 0: phase-alternating */              \
  X(OPT_FG_WS, "fg_ws", 1, 0, 1)                                                          \
  /* -1: whole-row waves for tables > 12 GB; 1 / 0: always / never */                     \
  X(OPT_SPMM_WIDE, "spmm_wide", -1, -1, 1)                                                \
  /* SpMM workgroups per CU (24) */                                                       \
  X(OPT_SPMM_BLOCKS_PER_CU, "spmm_blocks_per_cu", 24, 1, 64)                              \
  /* 1: x6 attention kernels; 0: fp32-MFMA kernels */                                     \
  X(OPT_ATTN_X6, "attn_x6", 1, 0, 1)                                                      \
  /* 1: 8-wave pipelined forward; 0: 4-wave */                                            \
  X(OPT_ATTN_FWD8, "attn_fwd8", 1, 0, 1)                                                  \
  /* 1: 8-wave dH pass; 0: 4-wave */                                                      \
  X(OPT_ATTN_DH8, "attn_dh8", 1, 0, 1)                                                    \
  /* 1: dQ folded into the dK pass; 0: separate dQ kernel */                              \
  X(OPT_ATTN_FUSED_DQ, "attn_fused_dq", 1, 0, 1)                                          \
  /* 1: software-pipelined x6 forward; 0: unpipelined */                                  \
  X(OPT_ATTN_PIPE, "attn_pipe", 1, 0, 1)                                                  \
  /* 1: dH pass on 16x16x32 MFMAs (dk <= 16; default); 0: the 32x32x16 kernel */          \
  X(OPT_ATTN_DH16, "attn_dh16", 1, 0, 1)                                                  \
  /* 1: fused dK/dQ pass on 16x16x32 MFMAs (dk <= 16; default); 0: the 32x32x16 kernel */ \
  X(OPT_ATTN_KQ16, "attn_kq16", 1, 0, 1)                                                  \
  /* fused dK/dQ slab budget in bytes (0: 24 GiB) */                                      \
  X(OPT_ATTN_QSLAB_MAX, "attn_qslab_max", 0, 0, INT64_MAX)                                \
  /* persistent kernels' bounded-wait limit (0: 2^24 sleeps) */                           \
  X(OPT_WS_SPIN, "ws_spin", 0, 0, (int64_t)1 << 30)                                       \
  /* 1: an eager one-kernel call checks its own status (debug) */                         \
  X(OPT_WS_STATUS_SYNC, "ws_status_sync", 0, 0, 1)
enum GrlOpt {
#define GRL_OPT_ENUM(id, name, def, lo, hi) id,
  GRL_OPTIONS(GRL_OPT_ENUM)
#undef GRL_OPT_ENUM
  OPT_COUNT
};
int64_t opt(GrlOpt o);

}  // namespace grl
