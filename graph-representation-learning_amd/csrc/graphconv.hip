// One GraphConv layer forward in ONE kernel for gfx950 (inference):
//
//   out = relu?( (A_drop X) W + bias )
//       gnn/models/networks/robust_gcn.py:45-51 (new_V = matmul(A_pre, V);
//       matmul(new_V, h_weights) + bias) and the F.relu of drop_robust_gcn.py:76.
//
// The two-kernel path (grl_typed_spmm_fwd, then the x6 GEMM) writes Z =
// A_drop X to HBM and reads it back: 7.2 GB each way at C3 (N = 1M, L = 6,
// F = 256).  Here Z never leaves the CU.  Two kernels share the pieces:
//  * graphconv_ws_kernel (default): persistent, one workgroup per CU, gather
//    waves and MFMA waves specialised and coupled by an LDS ring of Z tiles
//    (64 rows x 128 columns); see its comment below;
//  * graphconv_fused_kernel (fg_ws = 0): 32-row tiles, every wave
//    alternates gather and multiply phases, three workgroups per CU;
//  * graphconv_ws_bf16_kernel: graphconv_ws_kernel over a table of bf16 bits
//    (grl_graphconv_fwd_bf16, _fwd_train_bf16): the same body text
//    (graphconv_ws_body.inc) with 8 B-per-lane gather loads widened at the
//    fmaf, bitwise the fp32 kernel on the widened table;
//  * graphconv_ws_bf16o_kernel: graphconv_ws_bf16_kernel writing bf16 rows
//    with a caller-given stride (grl_graphconv_fwd_bf16_to_bf16,
//    _fwd_train_bf16_to_bf16): the epilogue rounds the finished tile to
//    nearest even in registers and stores two columns per dword;
//  * graphconv_ws_bf16g_kernel: the data-gradient form of that kernel
//    (grl_graphconv_bwd_data_bf16): it gathers a bf16 gradient table over the
//    typed transpose and writes bf16 dX rows.
// Shared pieces: the gather sums a wave's rows' segment-t neighbour rows
// (one float4 per lane, one 1 KB row per wave-instruction, the rows' edge
// lists streamed as one list with flushes at row boundaries); the multiply
// runs v_mfma_f32_32x32x16_bf16 six plane products per K16 step into fp32
// accumulators with W pre-split (fused_w_planes_kernel) in MFMA fragment
// order, fetched from L2 straight into registers (one coalesced 1 KB load
// per fragment); bias + ReLU in the epilogue; only out (N x C) is written.
// Arithmetic: each Z element is the same fmaf chain as spmm_kernel (CSR
// order, the same DropEdge weights), split and multiplied in the same K16
// order and product order as gemm_x6_kernel, so the result is bitwise that
// of the two-kernel path (tests/test_gpu_graphconv.py).
//
// The grl_graphconv_* entry points and the rules that choose between these
// kernels and the SpMM + GEMM chain are at the end of this file; from
// spmm.hip and linear.hip they take what grl_internal.h declares.
#include <cstring>

#include "grl_internal.h"
#include "x6.h"

#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <vector>

// Diagnostic switches (GRL_WS_STAMP, GRL_WS_ONLY_ROLE, GRL_WS_DIAG_*,
// GRL_WS_WHATIF below) are honoured only in diagnostic builds, which
// tools/build_diag.sh and tools/ws_regs.sh make with -DGRL_DIAG; a product
// build ignores them.
#ifndef GRL_DIAG
#undef GRL_WS_STAMP
#undef GRL_WS_ONLY_ROLE
#undef GRL_WS_DIAG_LB
#undef GRL_WS_DIAG_ONE
#undef GRL_WS_WHATIF
#endif

namespace grl {
namespace {

constexpr int FG_R = 32;                  // destination rows per tile
constexpr int FG_WAVES = 4;               // waves per workgroup
constexpr int FG_RW = FG_R / FG_WAVES;    // rows per wave in the gather
constexpr int FG_LD = 256 + 8;            // bf16 per Z-tile plane row (F <= 256) + one 16-B pad chunk
constexpr int FG_PLANE = FG_R * FG_LD;    // bf16 per plane
#ifndef GRL_FG_U
#define GRL_FG_U 8
#endif
// GRL_FG_PIPE_IDX=1: segment t+1's edge list and first 64 source rows /
// weights are loaded before segment t is gathered (their latency hidden)
#ifndef GRL_FG_PIPE_IDX
#define GRL_FG_PIPE_IDX 1
#endif
// GRL_FG_BDEPTH: register stages of W fragments in the multiply (2 or 3)
#ifndef GRL_FG_BDEPTH
#define GRL_FG_BDEPTH 2
#endif
#ifndef GRL_FG_WPE
#define GRL_FG_WPE 3
#endif
constexpr int FG_U = GRL_FG_U;            // neighbour rows in flight per wave
constexpr int FG_CB = 8;                  // 32-column blocks of out (C <= 256, zero padded)
constexpr int FG_FRAG = 64 * 8;           // bf16 per MFMA fragment (64 lanes x 8)

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void fma4(float4& acc, float w, const float4& x) {
  acc.x = __builtin_fmaf(w, x.x, acc.x);
  acc.y = __builtin_fmaf(w, x.y, acc.y);
  acc.z = __builtin_fmaf(w, x.z, acc.z);
  acc.w = __builtin_fmaf(w, x.w, acc.w);
}

// W [K][C] row-major -> three bf16 planes in MFMA B-fragment order:
// Wf[ks][cb][q][lane][e] = plane q of W(k = 16 ks + 8 (lane >> 5) + e,
// n = 32 cb + (lane & 31)) for cb < cbn (8: C <= 256, 16: C <= 512), zero for
// n >= C.
// t_cin > 0 (the data-gradient form, grl_graphconv_bwd_data): W(k, n) is the
// block-transposed forward weight, W(s t_cin + c, n) = Wfwd[s C + n][c] for
// the forward's [(L+1) C][t_cin] h_weights (block s of the result = W_s^T).
__global__ void fused_w_planes_kernel(const float* __restrict__ W, int64_t K, int C, uint16_t* __restrict__ Wf,
                                      int64_t t_cin, int cbn) {
  const int64_t total = K * cbn * 32;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
    const int64_t rest = i >> 9;
    const int cb = (int)(rest % cbn);
    const int64_t ks = rest / cbn;
    const int64_t k = ks * 16 + 8 * (lane >> 5) + e;
    const int n = cb * 32 + (lane & 31);
    const float v = n >= C ? 0.0f : (t_cin > 0 ? W[((k / t_cin) * C + n) * t_cin + k % t_cin] : W[k * C + n]);
    uint16_t h0, h1, h2;
    split1(v, h0, h1, h2);
    const int64_t o = (rest * 3) * FG_FRAG + lane * 8 + e;
    Wf[o] = h0;
    Wf[o + FG_FRAG] = h1;
    Wf[o + 2 * FG_FRAG] = h2;
  }
}

// Z-tile plane rows are 528 B apart (33 chunks of 16 B): row r's chunk c
// sits in bank slot (r + c) mod 16, so the fragment reads (ds_read_b128: lane
// groups of 16 rows at one chunk) and the row stores (ds_write_b64, 16 lanes
// on 128 contiguous bytes) are conflict-free, and a fragment's address is a
// per-lane base plus a compile-time offset per K16 step.
__device__ __forceinline__ int zoff(int r, int chunk) { return r * FG_LD + (chunk << 3); }

template <int KS, bool VALS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GRL_FG_WPE, GRL_FG_WPE))) void graphconv_fused_kernel(
    int64_t M, int L, int hs, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const float* __restrict__ vals, uint64_t edge_base, uint64_t self_base, const float* __restrict__ X,
    int64_t ldx, const uint16_t* __restrict__ Wf, const float* __restrict__ bias, int relu,
    float* __restrict__ out, int C, DropDev de) {
  constexpr int F = KS * 16;
  __shared__ __attribute__((aligned(16))) uint16_t zs[3 * FG_PLANE];
  de = resolve_key(de);
  const int lane = threadIdx.x & 63;
  const int wave = uniform_i(threadIdx.x >> 6);
  const int l32 = lane & 31, h = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * FG_R;
  const int64_t rw0 = m0 + wave * FG_RW;
  const int col = lane * 4;
  const bool col_ok = col < F;

  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

  // one finished Z row (this wave's row `slot`, this lane's 4 columns) -> planes
  auto flush = [&](int slot, const float4& v) {
    if (col_ok) {
      uint2 q0, q1, q2;
      split3(v, q0, q1, q2);
      const int rr = wave * FG_RW + slot;
      const int off = zoff(rr, lane >> 1) + (lane & 1) * 4;
      *reinterpret_cast<uint2*>(zs + off) = q0;
      *reinterpret_cast<uint2*>(zs + FG_PLANE + off) = q1;
      *reinterpret_cast<uint2*>(zs + 2 * FG_PLANE + off) = q2;
    }
  };

  // ---------------- multiply: acc += Zs(32 x F) W_s(F x 64 cols of this wave) ----------------
  auto multiply = [&](int s) {
    const uint16_t* wk = Wf + ((int64_t)s * KS * FG_CB + wave * 2) * 3 * FG_FRAG + lane * 8;
    constexpr int WSTEP = FG_CB * 3 * FG_FRAG;  // bf16 between K16 steps
    auto load_b = [&](bf16x8_t (&bb)[2][3], int ks) {
      const uint16_t* w = wk + ks * WSTEP;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q) bb[j][q] = *reinterpret_cast<const bf16x8_t*>(w + (j * 3 + q) * FG_FRAG);
    };
    auto step = [&](const bf16x8_t (&bb)[2][3], int ks) {
      bf16x8_t a[3];
      const int ao = zoff(l32, 2 * ks + h);
#pragma unroll
      for (int q = 0; q < 3; ++q) a[q] = *reinterpret_cast<const bf16x8_t*>(zs + q * FG_PLANE + ao);
#pragma unroll
      for (int j = 0; j < 2; ++j) x6_mfma(acc[j], a, bb[j]);
    };
#if GRL_FG_BDEPTH == 2
    // ping-pong: the next step's W fragments are in flight during this step's MFMAs
    bf16x8_t b0[2][3], b1[2][3];
    load_b(b0, 0);
#pragma unroll 1
    for (int ks = 0; ks < KS; ks += 2) {
      load_b(b1, ks + 1);  // KS is even
      step(b0, ks);
      if (ks + 2 < KS) load_b(b0, ks + 2);
      step(b1, ks + 1);
    }
#else
    // three register stages: step ks's fragments were issued two steps
    // earlier (an L2 hit under load takes longer than one step's 12 MFMAs)
    bf16x8_t bb[3][2][3];
    load_b(bb[0], 0);
    load_b(bb[1], 1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + 2 < KS) load_b(bb[(ks + 2) % 3], ks + 2);
      // keep the scheduler from sinking the loads into the MFMA stream (its
      // vmcnt waits would then stop on fragments issued a few MFMAs earlier)
      __builtin_amdgcn_sched_barrier(0);
      step(bb[ks % 3], ks);
      __builtin_amdgcn_sched_barrier(0);
    }
#endif
  };

  // ---------------- edge lists, one typed segment ahead ----------------
  // rowptr window of this wave's rows (lane l: rowptr[rw0 L + l], l <= FG_RW L;
  // rows past M read as empty), loaded once per tile
  const int nvalid = (int)max<int64_t>(0, min<int64_t>(FG_RW, M - rw0));
  const int rp = lane <= FG_RW * L ? rowptr[min<int64_t>(rw0 * L + min(lane, nvalid * L), M * L)] : 0;
  struct SegList {
    int b, exc, incl, total;
  };
  // the wave's rows' segment-t edge ranges as one list (lanes < FG_RW: row lane)
  auto seg_list = [&](int t) {
    const int r = min(lane, FG_RW - 1);
    SegList sg;
    sg.b = __shfl(rp, r * L + t);
    const int e1 = __shfl(rp, r * L + t + 1);  // all lanes: ds_bpermute reads only active lanes
    const int cnt = lane < FG_RW ? e1 - sg.b : 0;
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < FG_RW; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    sg.incl = incl;
    sg.exc = incl - cnt;
    sg.total = readlane_i(incl, FG_RW - 1);
    return sg;
  };
  // list entries [c0, c0 + 64): source row and DropEdge weight (0 = dropped / past the end)
  auto fetch = [&](const SegList& sg, int c0, int& sidx, float& w) {
    const int p = c0 + lane;
    int sl = 0;
#pragma unroll
    for (int i = 0; i < FG_RW - 1; ++i) sl += p >= readlane_i(sg.incl, i) ? 1 : 0;
    const int e = __shfl(sg.b, sl) + (p - __shfl(sg.exc, sl));  // CSR position of entry p
    sidx = 0;
    w = 0.0f;
    if (p < sg.total) {
      sidx = colidx[e];
      const float v = VALS ? vals[e] : 1.0f;
      w = de.active ? dropedge_weight(de, v, edge_base + (uint64_t)e) : v;
    }
  };
  SegList cur = seg_list(0);
  int sidx_c;
  float w_c;
  fetch(cur, 0, sidx_c, w_c);  // in flight during segment 0

  // ---------------- segment 0: the identity block of A_pre (robust_gcn.py:58-65) ----------------
  if (hs) {
    float4 xv[FG_RW];
#pragma unroll
    for (int i = 0; i < FG_RW; ++i)
      xv[i] = (rw0 + i < M && col_ok) ? *reinterpret_cast<const float4*>(X + (rw0 + i) * ldx + col) : zero4();
#pragma unroll
    for (int i = 0; i < FG_RW; ++i) {
      float w = 1.0f;
      if (de.active && de.drop_self) w = dropedge_weight(de, 1.0f, self_base + (uint64_t)(rw0 + i));
      const float4 x = w != 0.0f ? make_float4(w * xv[i].x, w * xv[i].y, w * xv[i].z, w * xv[i].w) : zero4();
      flush(i, x);
    }
    __syncthreads();
    multiply(0);
    __syncthreads();
  }

  // ---------------- typed segments: gather Z segment t of this wave's rows, then multiply ----------------
  for (int t = 0; t < L; ++t) {
    // the next segment's list and first 64 entries load while this one gathers and multiplies
    SegList nxt = cur;
    int sidx_n = 0;
    float w_n = 0.0f;
#if GRL_FG_PIPE_IDX
    if (t + 1 < L) {
      nxt = seg_list(t + 1);
      fetch(nxt, 0, sidx_n, w_n);
    }
#else
    if (t > 0) {
      cur = seg_list(t);
      fetch(cur, 0, sidx_c, w_c);
    }
#endif
    const int total = cur.total;
    int slot = 0;
    int bound = readlane_i(cur.incl, 0);  // end position of row `slot` in the combined list
    float4 a4 = zero4();
    for (int c0 = 0; c0 < total; c0 += 64) {
      int sidx = sidx_c;
      float w = w_c;
      if (c0 > 0) fetch(cur, c0, sidx, w);  // rows with more than 64 segment edges together
      uint64_t kept = __ballot(w != 0.0f);
      while (kept) {
        int jj[FG_U];
#pragma unroll
        for (int u = 0; u < FG_U; ++u) {
          if (kept) {
            jj[u] = __builtin_ctzll(kept);
            kept &= kept - 1;
          } else {
            jj[u] = -1;
          }
        }
        float4 xv[FG_U];
#pragma unroll
        for (int u = 0; u < FG_U; ++u) {
          if (jj[u] >= 0) {
            const int r = readlane_i(sidx, jj[u]);
            xv[u] = col_ok ? *reinterpret_cast<const float4*>(X + (int64_t)r * ldx + col) : zero4();
          }
        }
#pragma unroll
        for (int u = 0; u < FG_U; ++u) {
          if (jj[u] >= 0) {
            const int pos = c0 + jj[u];
            while (pos >= bound) {  // rows finished before this entry (wave-uniform)
              flush(slot, a4);
              a4 = zero4();
              ++slot;
              bound = readlane_i(cur.incl, slot);
            }
            fma4(a4, readlane_f(w, jj[u]), xv[u]);
          }
        }
      }
    }
    for (; slot < FG_RW; ++slot) {
      flush(slot, a4);
      a4 = zero4();
    }
    __syncthreads();
    multiply(hs + t);
    __syncthreads();
    cur = nxt;
    sidx_c = sidx_n;
    w_c = w_n;
  }

  // ---------------- epilogue: bias + ReLU, as gemm_x6_kernel ----------------
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = (wave * 2 + j) * 32 + l32;
    if (n >= C) continue;
    const bool epi = bias != nullptr || relu;
    const float bv = bias ? bias[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t m = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (m < M) {
        float v = acc[j][r];
        if (epi) {
          v = v + bv;
          if (relu) v = v > 0.0f ? v : 0.0f;
        }
        out[m * C + n] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Warp-specialized persistent form (the default).  One workgroup per CU, 12
// waves: PROD gather waves produce Z tiles into a 4-slot LDS ring, 12 - PROD
// MFMA waves consume them, so the HBM-bound gather and the matrix cores run
// at the same time instead of in alternating phases.
//  * a tile is 64 destination rows; a ring unit is a 128-column part of one
//    VIRTUAL segment of it, kept fp32 (64 x 128 floats + a pad chunk per row,
//    33 KB): every W fragment fetched from L2 feeds 64 rows (at 32 rows W's
//    re-read stream alone exceeded what L2 delivers to a CU), and the MFMA
//    waves split their A fragments into the x6 planes as they read them;
//  * virtual segments: a segment of F <= 256 columns is one; F = 256 FV
//    (gcn3's 2C-wide input, C5's d = 512 and its gcn3 at 1024) is FV
//    consecutive 256-column parts, each gathered as its own pass over the
//    segment's edge list (the list and its first 64 sources are reused, the
//    rows' 1 KB halves are what is read).  A finished row then fills only the
//    2 units of its part, so the 4-slot ring keeps a free slot ahead of the
//    MFMA waves at any F.  K order, and so every product, is unchanged;
//  * the unit stream: tile it of this workgroup (tile = blockIdx.x + it *
//    gridDim.x), virtual segment v, part hh -> unit u = (it * S FV + v) NH +
//    hh, ring slot u % 4, generation u / 4;
//  * gather wave p owns rows RW p..RW p + RW - 1 of each tile (RW = 64 /
//    PROD): it streams its rows' segment edges as one list (flushes at row
//    boundaries), gathering one float4 per lane per source row (1 KB per
//    wave-instruction, up to U rows in flight), and a finished row goes to
//    the virtual segment's NH units at once; the next segment's list and
//    first 64 sources load while this one gathers.  Before its first store
//    to a virtual segment's units it waits until the MFMA waves released
//    their slots' previous generation (consumed[slot] >= CONS g); after its
//    last it adds 1 to produced[slot] (release); gather waves never wait for
//    each other;
//  * MFMA wave c owns output columns 64c..64c+63 for all 64 rows (2 x 2
//    MFMA blocks): it waits for produced[slot] >= PROD (g + 1) (acquire), runs
//    the unit's K16 steps (24 MFMAs each) with the next step's W fragments
//    in flight (the W stream crosses unit and tile boundaries: it is
//    periodic in the segment order), then adds 1 to consumed[slot]; after a
//    tile's last unit it stores the tile.
//  * PROD = 8 (C <= 256: 4 MFMA waves) or 4 (C <= 512: 8 MFMA waves, each
//    gather wave 16 rows with two rowptr-window registers and more rows in
//    flight, so the bytes in flight per CU stay the same).
// Every wave walks the same unit sequence and units complete in order, so
// the waits cannot form a cycle; each spin is bounded anyway (a kernel that
// could hang the GPU is not an option): a wave whose bound runs out sets the
// call's status word (vector atomic OR into the caller's workspace) and
// stops; graphconv_status then poisons the call's outputs (stream-ordered).
// Arithmetic per element is the same as graphconv_fused_kernel's (same
// chains, split, K order, product order): bitwise the two-kernel result.
constexpr int WS_R = 64;                   // rows per tile
constexpr int WS_KC = 128;                 // Z columns per ring unit
constexpr int WS_FV = 256;                 // columns per virtual segment (at most)
constexpr int WS_LDF = WS_KC + 4;          // floats per ring row (+ one 16-B pad chunk: conflict-free)
constexpr int WS_SLOT = WS_R * WS_LDF;     // floats per ring slot
constexpr int WS_WAVES = 12;               // gather + MFMA waves per workgroup
constexpr int WS_CB = 2;                   // 32-column blocks per MFMA wave
constexpr int WS_NB = (140 * 1024) / (WS_SLOT * 4);  // ring slots that ~140 KB hold: 4
#ifndef GRL_WS_U
#define GRL_WS_U 12
#endif
#ifndef GRL_WS_U16
#define GRL_WS_U16 12
#endif
// the bf16-table kernel's rows in flight (2 dwords a row, not 4): its own knobs
#ifndef GRL_WS_BF16_U
#define GRL_WS_BF16_U 12
#endif
#ifndef GRL_WS_BF16_U16
#define GRL_WS_BF16_U16 12
#endif
constexpr int WS_SPIN = 1 << 24;           // bounded waits (~0.5 s of s_sleep 1); the ws_spin path option overrides
constexpr int WS_STATUS_TIMEOUT = 1;       // status bit: a bounded wait ran out (results invalid)

// GRL_WS_STAMP=1 (diagnostic builds only): every wave adds up the cycles it
// spent waiting on the ring and its total, read back with grl_debug_ws_stats
#ifndef GRL_WS_STAMP
#define GRL_WS_STAMP 0
#endif
// GRL_WS_ONLY_ROLE (register-use diagnostics only, never a working build):
// 1 = compile the gather role alone, 2 = the MFMA role alone
#ifndef GRL_WS_ONLY_ROLE
#define GRL_WS_ONLY_ROLE 0
#endif
// GRL_WS_WHATIF (timing-only diagnostic builds, wrong results): 1 = the MFMA
// waves re-read two steps of W (L2-hot) instead of the stream, 2 = no A split,
// 4 = the gather alone (MFMA waves only release slots), 8 = the MFMA side
// alone (gather waves store zeros for the typed segments)
#ifndef GRL_WS_WHATIF
#define GRL_WS_WHATIF 0
#endif
#if GRL_WS_STAMP
__device__ unsigned long long g_ws_dbg[1024 * 12 * 2];
#endif

__device__ __forceinline__ int lds_load_acq(int* p) {
  return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_add_rel(int* p, int v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// wait until *p >= target (wave-uniform); false if the bound ran out, after
// recording it in *status (one lane, vector atomic to global memory)
__device__ __forceinline__ bool wait_ge(int* p, int target, unsigned long long* waited, int spin_limit,
                                        int* status) {
#if GRL_WS_STAMP
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
  for (int spin = 0; spin < spin_limit; ++spin) {
    if (lds_load_acq(p) >= target) {
#if GRL_WS_STAMP
      *waited += __builtin_amdgcn_s_memtime() - t0;
#endif
      return true;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_or(status, WS_STATUS_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return false;
}

// KS: K16 steps of one virtual segment (its width / 16); FV: virtual segments
// per segment (F = 16 KS FV); PROD: gather waves (8: C <= 256, 4: C <= 512).
// EID (the data-gradient form over the typed transpose): entry e's DropEdge
// id is edge_base + eid[e] (its forward CSR position) instead of edge_base + e.
// Rows >= self_rows have no self term (a shard's transpose: its halo rows);
// the forward passes M.
#ifndef GRL_WS_DIAG_LB
#define GRL_WS_DIAG_LB (64 * WS_WAVES)  // register-use diagnostics: a smaller bound shows the unconstrained demand
#endif
// The kernel's body is graphconv_ws_body.inc, shared as text by the fp32
// kernel and the bf16-table kernel below it (why, and what differs: there).

// a lane's 4 bf16 columns as loaded -> fp32, exactly
__device__ __forceinline__ float4 widen4(const uint2& b) {
  return make_float4(lo_f(b.x), hi_f(b.x), lo_f(b.y), hi_f(b.y));
}

template <int KS, bool VALS, bool EID = false, int FV = 1, int PROD = 8>
__global__ __launch_bounds__(GRL_WS_DIAG_LB) void graphconv_ws_kernel(
    int64_t M, int L, int hs, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const float* __restrict__ vals, uint64_t edge_base, uint64_t self_base, const float* __restrict__ X,
    int64_t ldx, const uint16_t* __restrict__ Wf, const float* __restrict__ bias, int relu,
    float* __restrict__ out, int C, DropDev de, int64_t num_tiles, float* __restrict__ Zout, int64_t ldz,
    const int32_t* __restrict__ eid, int64_t self_rows, int spin_limit, int* __restrict__ status,
    int64_t self_row0) {
#define GRL_WS_BF16 0
#define GRL_WS_OUT16 0
#include "graphconv_ws_body.inc"
#undef GRL_WS_OUT16
#undef GRL_WS_BF16
}

// The forward over a bf16 table (grl_graphconv_fwd_bf16, _fwd_train_bf16): X
// holds bf16 bits, ldx counts them.  No data-gradient form (its gathered
// operand is the fp32 gradient).
template <int KS, bool VALS, int FV = 1, int PROD = 8>
__global__ __launch_bounds__(GRL_WS_DIAG_LB) void graphconv_ws_bf16_kernel(
    int64_t M, int L, int hs, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const float* __restrict__ vals, uint64_t edge_base, uint64_t self_base, const uint16_t* __restrict__ X,
    int64_t ldx, const uint16_t* __restrict__ Wf, const float* __restrict__ bias, int relu,
    float* __restrict__ out, int C, DropDev de, int64_t num_tiles, float* __restrict__ Zout, int64_t ldz,
    int spin_limit, int* __restrict__ status, int64_t self_row0) {
  constexpr bool EID = false;
  const int32_t* const eid = nullptr;
  const int64_t self_rows = M;
#define GRL_WS_BF16 1
#define GRL_WS_OUT16 0
#include "graphconv_ws_body.inc"
#undef GRL_WS_OUT16
#undef GRL_WS_BF16
}

// GRL_WS_OUT16_PACK: the bf16-output kernel's store form, 1 = lane pairs trade
// a value and store dwords, 0 = one 2 B store per element (the same bits; the
// A/B is in DESIGN.md §4.17)
#ifndef GRL_WS_OUT16_PACK
#define GRL_WS_OUT16_PACK 1
#endif

// (cvt_pk_bf16, the rounding of the epilogue's stores, and swap_lane_pair, the lane pairs' trade: grl_internal.h)

// The bf16-table forward writing bf16 rows (grl_graphconv_fwd_bf16_to_bf16,
// _fwd_train_bf16_to_bf16): graphconv_ws_bf16_kernel but for the epilogue's
// stores -- out holds bf16 bits, ldo (>= C, counted in bf16 elements) apart a
// row, each the fp32 epilogue value rounded to nearest even.  Zout stays fp32.
template <int KS, bool VALS, int FV = 1, int PROD = 8>
__global__ __launch_bounds__(GRL_WS_DIAG_LB) void graphconv_ws_bf16o_kernel(
    int64_t M, int L, int hs, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const float* __restrict__ vals, uint64_t edge_base, uint64_t self_base, const uint16_t* __restrict__ X,
    int64_t ldx, const uint16_t* __restrict__ Wf, const float* __restrict__ bias, int relu,
    uint16_t* __restrict__ out, int C, DropDev de, int64_t num_tiles, float* __restrict__ Zout, int64_t ldz,
    int spin_limit, int* __restrict__ status, int64_t self_row0, int64_t ldo) {
  constexpr bool EID = false;
  const int32_t* const eid = nullptr;
  const int64_t self_rows = M;
#define GRL_WS_BF16 1
#define GRL_WS_OUT16 1
#include "graphconv_ws_body.inc"
#undef GRL_WS_OUT16
#undef GRL_WS_BF16
}

// graphconv_ws_bf16o_kernel whose Zout holds bf16 bits too
// (grl_graphconv_fwd_train_bf16_z16): the gather waves round the copy of a
// finished row that goes to HBM (8 B a lane, ldz counted in bf16 elements);
// the ring, and so out, is that kernel's.  The forward form only.
template <int KS, bool VALS, int FV = 1, int PROD = 8>
__global__ __launch_bounds__(GRL_WS_DIAG_LB) void graphconv_ws_bf16oz_kernel(
    int64_t M, int L, int hs, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const float* __restrict__ vals, uint64_t edge_base, uint64_t self_base, const uint16_t* __restrict__ X,
    int64_t ldx, const uint16_t* __restrict__ Wf, const float* __restrict__ bias, int relu,
    uint16_t* __restrict__ out, int C, DropDev de, int64_t num_tiles, uint16_t* __restrict__ Zout, int64_t ldz,
    int spin_limit, int* __restrict__ status, int64_t self_row0, int64_t ldo) {
  constexpr bool EID = false;
  const int32_t* const eid = nullptr;
  const int64_t self_rows = M;
#define GRL_WS_BF16 1
#define GRL_WS_OUT16 1
#define GRL_WS_Z16 1
#include "graphconv_ws_body.inc"
#undef GRL_WS_Z16
#undef GRL_WS_OUT16
#undef GRL_WS_BF16
}

// The data-gradient form over a bf16 gradient table, writing bf16 rows
// (grl_graphconv_bwd_data_bf16): graphconv_ws_kernel's EID form -- entry e's
// DropEdge id through eid, the self term for rows < self_rows -- with
// graphconv_ws_bf16o_kernel's gather loads (X = G, bf16 bits, ldx apart a
// row) and epilogue (out = dX, bf16 bits, ldo apart a row).  Zout (G_agg)
// stays fp32.  The same body text: no line of it is this kernel's alone.
template <int KS, bool VALS, int FV = 1, int PROD = 8>
__global__ __launch_bounds__(GRL_WS_DIAG_LB) void graphconv_ws_bf16g_kernel(
    int64_t M, int L, int hs, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const float* __restrict__ vals, uint64_t edge_base, uint64_t self_base, const uint16_t* __restrict__ X,
    int64_t ldx, const uint16_t* __restrict__ Wf, const float* __restrict__ bias, int relu,
    uint16_t* __restrict__ out, int C, DropDev de, int64_t num_tiles, float* __restrict__ Zout, int64_t ldz,
    const int32_t* __restrict__ eid, int64_t self_rows, int spin_limit, int* __restrict__ status,
    int64_t self_row0, int64_t ldo) {
  constexpr bool EID = true;
#define GRL_WS_BF16 1
#define GRL_WS_OUT16 1
#include "graphconv_ws_body.inc"
#undef GRL_WS_OUT16
#undef GRL_WS_BF16
}

}  // namespace

#if GRL_WS_STAMP
extern "C" int grl_debug_ws_stats(unsigned long long* host, int64_t n) {
  GRL_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_ws_dbg), (size_t)n * 8));
  return GRL_OK;
}
#endif

// The graphconv_fused path option 0 keeps grl_graphconv_fwd on the
// two-kernel path (A/B aid and tests).
static bool graphconv_fused_enabled() { return opt(OPT_GRAPHCONV_FUSED) != 0; }

// The gathered width F: one virtual segment (64, 128, 256) or 2 / 4 of 256
// columns; the output width C <= 512 (C > 256: 4 gather + 8 MFMA waves); L
// <= 7 (a gather wave's rowptr window holds RW L + 1 entries in 1 or 2
// registers).  The phase-alternating kernel (fg_ws = 0) takes F <= 256, C
// <= 256 only; other shapes always run the persistent one.
static bool graphconv_fused_shape_ok(int F, int C, int L) {
  return (F == 64 || F == 128 || F == 256 || F == 512 || F == 1024) && C >= 1 && C <= 512 && L >= 1 && L <= 7;
}

// 32-column blocks of W's planes: 8 for C <= 256, 16 for C <= 512
static int planes_cb(int C) { return C <= 256 ? FG_CB : 2 * FG_CB; }

// W's planes, then 256 B whose first word is the call's status
static size_t graphconv_fused_ws_bytes(int64_t K, int C) { return (size_t)K * planes_cb(C) * 32 * 3 * 2 + 256; }

static int* ws_status(void* ws, int64_t K, int C) {
  return reinterpret_cast<int*>(static_cast<char*>(ws) + (size_t)K * planes_cb(C) * 32 * 3 * 2);
}

static int ws_spin_limit() {
  const int64_t v = opt(OPT_WS_SPIN);  // test / diagnostic aid: a tiny bound forces the timeout path
  return v > 0 ? (int)v : WS_SPIN;
}

// A persistent kernel whose bounded wait ran out left its outputs partly
// unwritten.  Stream-ordered handling (no host sync on the call): a
// follow-up kernel fills the call's outputs with NaN when the call's status
// word is set, and ORs the entry point's bit into the per-device sticky
// word, which grl_check() reads and clears at the caller's next sync point.
// ws_status_sync = 1 (debug aid) makes an eager call wait for its kernel and
// return GRL_E_TIMEOUT itself, as round 3's entry points did.
__device__ int g_grl_sticky;  // bit i: a call of WS_WHO_NAMES[i] had its outputs poisoned

// The entries that run the persistent kernel, by their bit's position in the
// sticky word (grl_check's callers read the bits: positions never change).
constexpr const char* WS_WHO_NAMES[] = {
    "grl_graphconv_fwd",              "grl_graphconv_fwd_train",              "grl_graphconv_bwd_data",
    "grl_graphconv_fwd_bf16",         "grl_graphconv_fwd_train_bf16",         "grl_graphconv_fwd_bf16_to_bf16",
    "grl_graphconv_fwd_train_bf16_to_bf16", "grl_graphconv_bwd_data_bf16",    "grl_graphconv_fwd_train_bf16_z16"};
constexpr int WS_WHO_COUNT = sizeof(WS_WHO_NAMES) / sizeof(WS_WHO_NAMES[0]);
constexpr int WS_WHO_BWD_DATA = 1 << 2, WS_WHO_BWD_DATA_BF16 = 1 << 7;
// a forward entry's bit: by its table (bf16), its out (out16), its Z (z16) and whether it writes Z at all
constexpr int ws_who_fwd(bool bf16, bool out16, bool z16, bool train) {
  return 1 << (z16 ? 8 : out16 ? 5 + train : bf16 ? 3 + train : train);
}
static const char* who_name(int who) { return WS_WHO_NAMES[__builtin_ctz(who)]; }

__global__ void ws_poison_kernel(const int* __restrict__ status, float* __restrict__ a, int64_t na,
                                 float* __restrict__ b, int64_t nb, int who) {
  if (*status == 0) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_fetch_or(&g_grl_sticky, who, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float nan = __builtin_nanf("");
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < na + nb; i += (int64_t)gridDim.x * blockDim.x)
    (i < na ? a[i] : b[i - na]) = nan;
}

// ws_poison_kernel for a strided bf16 out [M, C] (ldo apart a row): a bf16 NaN
// into C of every ldo elements, never the columns beside them; b (Z) as there.
__global__ void ws_poison_bf16_kernel(const int* __restrict__ status, uint16_t* __restrict__ a, int64_t M, int C,
                                      int64_t ldo, float* __restrict__ b, int64_t nb, int who) {
  if (*status == 0) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_fetch_or(&g_grl_sticky, who, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float nan = __builtin_nanf("");
  const int64_t na = M * C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < na + nb; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < na)
      a[(i / C) * ldo + i % C] = 0x7fc0;
    else
      b[i - na] = nan;
  }
}

// a: the call's out, float [M, C] contiguous or uint16_t (bf16 bits) [M, C] with row stride ldo; b: its Z / G_agg
// of nb elements, float or (grl_graphconv_fwd_train_bf16_z16) bf16 bits, poisoned as one more bf16 array of a row
template <typename OT, typename ZT = float>
static int graphconv_status(const int* status, OT* a, int64_t M, int C, int64_t ldo, ZT* b, int64_t nb,
                            hipStream_t st, int who) {
  const bool sync = opt(OPT_WS_STATUS_SYNC) != 0;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (sync) GRL_HIP(hipStreamIsCapturing(st, &cs));
  if (!sync || cs != hipStreamCaptureStatusNone) {
    if constexpr (std::is_same<ZT, uint16_t>::value) {
      static_assert(std::is_same<OT, uint16_t>::value, "a bf16 Z: with a bf16 out only");
      hipLaunchKernelGGL(ws_poison_bf16_kernel, dim3(1024), dim3(256), 0, st, status, a, M, C, ldo,
                         static_cast<float*>(nullptr), (int64_t)0, who);
      if (b && M > 0)  // Z [M, nb / M] contiguous
        hipLaunchKernelGGL(ws_poison_bf16_kernel, dim3(1024), dim3(256), 0, st, status, b, M, (int)(nb / M), nb / M,
                           static_cast<float*>(nullptr), (int64_t)0, who);
    } else if constexpr (std::is_same<OT, uint16_t>::value)
      hipLaunchKernelGGL(ws_poison_bf16_kernel, dim3(1024), dim3(256), 0, st, status, a, M, C, ldo, b, b ? nb : 0, who);
    else
      hipLaunchKernelGGL(ws_poison_kernel, dim3(1024), dim3(256), 0, st, status, a, M * C, b, b ? nb : 0, who);
    GRL_LAUNCH_CHECK();
    return GRL_OK;
  }
  int h = 0;
  GRL_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, st));
  GRL_HIP(hipStreamSynchronize(st));
  if (h & WS_STATUS_TIMEOUT)
    GRL_FAIL(GRL_E_TIMEOUT, "%s: a wave of the persistent GraphConv kernel gave up waiting on its LDS ring "
             "(bound %d sleeps); the outputs are invalid", who_name(who), ws_spin_limit());
  return GRL_OK;
}

// One launch of the persistent kernel for gathered width F and output width
// C over a table of XT (float, or uint16_t: bf16 bits): the template instance
// for (F, C > 256) with or without edge values / eid (the data-gradient form:
// fp32 table and out, or bf16 table and out -- graphconv_ws_bf16g_kernel);
// grid = one workgroup per CU (at most the tiles).  The bf16 forward kernels
// have no eid / self_rows arguments.  OT = uint16_t (a bf16 table only): out
// holds bf16 bits with row stride ldo (graphconv_ws_bf16o_kernel, _bf16g_);
// OT = float: out is [M, C] contiguous and ldo is not looked at.  ZT =
// uint16_t (a bf16 out, the forward only): Z holds bf16 bits, ldz counts them
// (graphconv_ws_bf16oz_kernel).
template <typename XT, bool EID, typename OT = float, typename ZT = float>
static void launch_ws(int F, int C, bool v, dim3 grid, hipStream_t st, int64_t M, int L, int hs,
                      const GrlTypedCsr* g, const XT* X, int64_t ldx, const uint16_t* Wf, const float* bias,
                      int relu, OT* out, int64_t ldo, DropDev d, int64_t tiles, ZT* Z, int64_t ldz,
                      const int32_t* eid, int64_t self_rows, int spin, int* status) {
  constexpr bool BF16 = std::is_same<XT, uint16_t>::value;
  constexpr bool OUT16 = std::is_same<OT, uint16_t>::value;
  constexpr bool Z16 = std::is_same<ZT, uint16_t>::value;
  static_assert(!(BF16 && EID) || OUT16, "the data-gradient form over a bf16 table writes a bf16 dX only");
  static_assert(!OUT16 || BF16, "bf16 output: over a bf16 table only");
  static_assert(!Z16 || (OUT16 && !EID), "bf16 Z: the forward with a bf16 out only");
#define GRL_WS_HEAD                                                                                                \
  grid, dim3(64 * WS_WAVES), 0, st, M, L, hs, g->rowptr, g->colidx, g->vals, g->edge_id_base, g->self_id_base, X, \
      ldx, Wf, bias, relu, out, C, d, tiles, Z, ldz
#define GRL_WS_INST(KS_, VALS_, FV_, PROD_)                                                                       \
  do {                                                                                                            \
    if constexpr (Z16)                                                                                            \
      hipLaunchKernelGGL((graphconv_ws_bf16oz_kernel<KS_, VALS_, FV_, PROD_>), GRL_WS_HEAD, spin, status,         \
                         g->self_row0, ldo);                                                                      \
    else if constexpr (OUT16 && EID)                                                                              \
      hipLaunchKernelGGL((graphconv_ws_bf16g_kernel<KS_, VALS_, FV_, PROD_>), GRL_WS_HEAD, eid, self_rows, spin,  \
                         status, g->self_row0, ldo);                                                              \
    else if constexpr (OUT16)                                                                                     \
      hipLaunchKernelGGL((graphconv_ws_bf16o_kernel<KS_, VALS_, FV_, PROD_>), GRL_WS_HEAD, spin, status,          \
                         g->self_row0, ldo);                                                                      \
    else if constexpr (BF16)                                                                                      \
      hipLaunchKernelGGL((graphconv_ws_bf16_kernel<KS_, VALS_, FV_, PROD_>), GRL_WS_HEAD, spin, status,           \
                         g->self_row0);                                                                           \
    else                                                                                                          \
      hipLaunchKernelGGL((graphconv_ws_kernel<KS_, VALS_, EID, FV_, PROD_>), GRL_WS_HEAD, eid, self_rows, spin,   \
                         status, g->self_row0);                                                                   \
  } while (0)
#define GRL_WS_ONE(KS_, FV_, PROD_)        \
  do {                                     \
    if (v)                                 \
      GRL_WS_INST(KS_, true, FV_, PROD_);  \
    else                                   \
      GRL_WS_INST(KS_, false, FV_, PROD_); \
  } while (0)
#define GRL_WS_PRODS(KS_, FV_)       \
  do {                               \
    if (C <= 256)                    \
      GRL_WS_ONE(KS_, FV_, 8);       \
    else                             \
      GRL_WS_ONE(KS_, FV_, 4);       \
  } while (0)
#ifdef GRL_WS_DIAG_ONE  // register-use diagnostics only: one instance (F = 256 FV, PROD)
  GRL_WS_ONE(16, GRL_WS_DIAG_FV, GRL_WS_DIAG_PROD);
#else
  switch (F) {
    case 64: GRL_WS_PRODS(4, 1); break;
    case 128: GRL_WS_PRODS(8, 1); break;
    case 256: GRL_WS_PRODS(16, 1); break;
    case 512: GRL_WS_PRODS(16, 2); break;
    default: GRL_WS_PRODS(16, 4); break;  // 1024
  }
#endif
#undef GRL_WS_PRODS
#undef GRL_WS_ONE
#undef GRL_WS_INST
#undef GRL_WS_HEAD
}

// XT = float: X is the fp32 table; XT = uint16_t: bf16 bits, always on the
// persistent kernel (there is no bf16 phase-alternating kernel).  OT =
// uint16_t (a bf16 table only): out holds bf16 bits, ldo apart a row.  ZT =
// uint16_t (a bf16 out only): Z holds bf16 bits (grl_graphconv_fwd_train_bf16_z16).
// who: the calling entry's sticky bit (ws_who_fwd).
template <typename XT, typename OT, typename ZT>
static int graphconv_fused_fwd(int who, const GrlTypedCsr* g, const XT* X, int64_t ldx, int F, const float* W,
                               const float* bias, int C, int relu, OT* out, int64_t ldo, const GrlDropEdge* de,
                               void* ws, hipStream_t st, ZT* Z) {
  constexpr bool BF16 = std::is_same<XT, uint16_t>::value;
  constexpr bool OUT16 = std::is_same<OT, uint16_t>::value;
  static_assert(!OUT16 || BF16, "bf16 output: a bf16 table only");
  const int hs = g->has_self ? 1 : 0;
  const int64_t K = (int64_t)segments(g) * F;
  uint16_t* Wf = static_cast<uint16_t*>(ws);
  const int cbn = planes_cb(C);
  const int64_t n_el = K * cbn * 32;
  hipLaunchKernelGGL(fused_w_planes_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(n_el, 256), 4096)), dim3(256), 0,
                     st, W, K, C, Wf, (int64_t)0, cbn);
  GRL_LAUNCH_CHECK();
  const int64_t M = g->num_rows;
  const int64_t tiles = ceil_div(M, FG_R);
  GRL_CHECK_ARG(tiles < 2147483647LL, "%s: too many row tiles", who_name(who));
  const DropDev d = to_dev(de);
  const bool v = g->vals != nullptr;
  // the persistent kernel (Z out, wide shapes and row-range views: only it)
  if (BF16 || opt(OPT_FG_WS) != 0 || Z || F > 256 || C > 256 || g->self_row0 != 0) {
    const int64_t ldz = K;
    const int64_t ws_tiles = ceil_div(M, WS_R);
    const int64_t grid = std::min<int64_t>(ws_tiles, (int64_t)device_cu_count());
    int* status = ws_status(ws, K, C);
    const int spin = ws_spin_limit();
    GRL_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    launch_ws<XT, false, OT, ZT>(F, C, v, dim3((unsigned)grid), st, M, g->num_types, hs, g, X, ldx, Wf, bias, relu,
                                 out, ldo, d, ws_tiles, Z, ldz, nullptr, M, spin, status);
    GRL_LAUNCH_CHECK();
    return graphconv_status(status, out, M, C, ldo, Z, M * ldz, st, who);
  }
  if constexpr (!BF16) {
#define GRL_FUSED_LAUNCH(KS_)                                                                                      \
  do {                                                                                                               \
    if (v)                                                                                                           \
      hipLaunchKernelGGL((graphconv_fused_kernel<KS_, true>), dim3((unsigned)tiles), dim3(256), 0, st, M,            \
                         g->num_types, hs, g->rowptr, g->colidx, g->vals, g->edge_id_base, g->self_id_base, X, ldx,  \
                         Wf, bias, relu, out, C, d);                                                                 \
    else                                                                                                             \
      hipLaunchKernelGGL((graphconv_fused_kernel<KS_, false>), dim3((unsigned)tiles), dim3(256), 0, st, M,           \
                         g->num_types, hs, g->rowptr, g->colidx, g->vals, g->edge_id_base, g->self_id_base, X, ldx,  \
                         Wf, bias, relu, out, C, d);                                                                 \
  } while (0)
  if (F == 256)
    GRL_FUSED_LAUNCH(16);
  else if (F == 128)
    GRL_FUSED_LAUNCH(8);
  else
    GRL_FUSED_LAUNCH(4);
#undef GRL_FUSED_LAUNCH
  }
  GRL_LAUNCH_CHECK();
  return GRL_OK;
}

// dX = sum_s G_s W_s^T over the typed transpose gt (grl_graphconv_bwd_data):
// graphconv_ws_kernel with the rows' CSC segments, DropEdge ids through eid,
// and W's planes taken block-transposed.  Cin = G's width (the forward's C),
// Cout = dX's width (the forward's F).  GT = OT = float: G fp32, dX [M, Cout]
// contiguous (lddx = Cout); GT = OT = uint16_t: both hold bf16 bits, dX's rows
// lddx apart (grl_graphconv_bwd_data_bf16, graphconv_ws_bf16g_kernel).
template <typename GT, typename OT>
static int graphconv_fused_bwd_data(const GrlTypedCsr* gt, const int32_t* eid, const GT* G, int64_t ldg,
                                    int64_t self_rows, int Cin, const float* W, int Cout, OT* dX, int64_t lddx,
                                    float* Gagg, const GrlDropEdge* de, void* ws, hipStream_t st) {
  const int hs = gt->has_self ? 1 : 0;
  const int64_t K = (int64_t)segments(gt) * Cin;
  uint16_t* Wf = static_cast<uint16_t*>(ws);
  const int cbn = planes_cb(Cout);
  const int64_t n_el = K * cbn * 32;
  hipLaunchKernelGGL(fused_w_planes_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(n_el, 256), 4096)), dim3(256), 0,
                     st, W, K, Cout, Wf, (int64_t)Cin, cbn);
  GRL_LAUNCH_CHECK();
  const int64_t M = gt->num_rows;
  const int64_t ws_tiles = ceil_div(M, WS_R);
  GRL_CHECK_ARG(ws_tiles < 2147483647LL, "%s: too many row tiles",
                who_name(std::is_same<OT, uint16_t>::value ? WS_WHO_BWD_DATA_BF16 : WS_WHO_BWD_DATA));
  const int64_t grid = std::min<int64_t>(ws_tiles, (int64_t)device_cu_count());
  const DropDev d = to_dev(de);
  const bool v = gt->vals != nullptr;
  int* status = ws_status(ws, K, Cout);
  const int spin = ws_spin_limit();
  GRL_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
  launch_ws<GT, true, OT>(Cin, Cout, v, dim3((unsigned)grid), st, M, gt->num_types, hs, gt, G, ldg, Wf, nullptr, 0, dX,
                          lddx, d, ws_tiles, Gagg, K, eid, self_rows, spin, status);
  GRL_LAUNCH_CHECK();
  return graphconv_status(status, dX, M, Cout, lddx, Gagg, M * K, st,
                          std::is_same<OT, uint16_t>::value ? WS_WHO_BWD_DATA_BF16 : WS_WHO_BWD_DATA);
}

// ---- the layer's dispatch: which kernels a grl_graphconv_* call runs -------
static size_t ws_align(size_t b) { return (b + 255) & ~(size_t)255; }

// The workspace of the two-kernel chain (the SpMM into an fp32 Z, then the
// linear, whose GEMM path is chosen for path_rows rows), as byte offsets of
// 256-B aligned regions: an fp32 Z [M, K] at 0 (z_in_ws: inference, and a
// bf16 Z, which is rounded from it; else the caller's fp32 Z is the SpMM's
// target), the linear's fp32 out [M, C] at lin_out (a bf16 out, rounded from
// it), the linear's own workspace at lin_ws.  The queries answer `total`; the
// entries take their pointers from the same struct.
struct FwdChainLayout {
  size_t lin_out, lin_ws, total;
};
static FwdChainLayout fwd_chain_layout(const GrlTypedCsr* g, int64_t K, int C, bool out16, bool z_in_ws) {
  FwdChainLayout l;
  l.lin_out = z_in_ws ? ws_align((size_t)g->num_rows * (size_t)K * 4) : 0;
  l.lin_ws = l.lin_out + (out16 ? ws_align((size_t)g->num_rows * (size_t)C * 4) : 0);
  l.total = l.lin_ws + grl_linear_fwd_ex_workspace_size(g->num_rows, (int32_t)K, C, g->path_rows);
  return l;
}

// grl_graphconv_fwd takes the fused kernel when its arithmetic equals the
// two-kernel path's (the linear on the x6 GEMM: large graphs, 16-B aligned W,
// C % 4 == 0), the shapes fit it (graphconv_fused_shape_ok), every row of X
// (XT = float, or uint16_t: bf16 bits) is aligned to the one load of a lane's
// 4 columns (16 B / 8 B) and its bytes fit 32 bits (the gather's row offset),
// and no heavy row is split (the split path sums chunk partials, a different
// order).
template <typename XT>
static bool fused_path(const GrlTypedCsr* g, const XT* X, int64_t ldx, int F, const float* W, int C) {
  return graphconv_fused_enabled() && graphconv_fused_shape_ok(F, C, g->num_types) &&
         x6_path_ok(g->num_rows, g->path_rows, C, (int64_t)segments(g) * F) && al16(W) && C % 4 == 0 &&
         reinterpret_cast<uintptr_t>(X) % (4 * sizeof(XT)) == 0 && ldx % 4 == 0 &&
         ldx < (int64_t)((1ULL << 32) / sizeof(XT)) && (!g->split || g->split->num_heavy == 0);
}

// The one-kernel rule of a forward entry: fused_path, and the rows the kernel
// writes take its stores.  A bf16 out (OT = uint16_t, ldo apart a row) the
// epilogue's dword stores of two columns: out 4 B-aligned, ldo even (an fp32
// out is [num_rows, C] contiguous, ldo not looked at).  A Z written (train)
// the gather waves' one store of a lane's 4 columns: 16 B-aligned for fp32, 8 B
// for bf16 bits (K % 4 == 0 there).
template <typename XT, typename OT, typename ZT>
static bool fwd_one_kernel(const GrlTypedCsr* g, const XT* X, int64_t ldx, int F, const float* W, int C, const OT* out,
                           int64_t ldo, const ZT* Z, bool train) {
  if (std::is_same<OT, uint16_t>::value && (reinterpret_cast<uintptr_t>(out) % 4 != 0 || ldo % 2 != 0)) return false;
  if (train && reinterpret_cast<uintptr_t>(Z) % (4 * sizeof(ZT)) != 0) return false;
  return fused_path(g, X, ldx, F, W, C);
}

// Elsewhere a bf16 out or Z is the chain's fp32 array passed through this:
// dst[m, c] (ldo apart a row) = src[m, c] rounded to nearest even, the kernel's
// own conversion, so the bits are the one-kernel form's.
__global__ void round_rows_bf16_kernel(const float* __restrict__ src, int64_t M, int C, uint16_t* __restrict__ dst,
                                       int64_t ldo) {
  const int64_t n = M * C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[(i / C) * ldo + i % C] = (uint16_t)cvt_pk_bf16(src[i], 0.0f);
}

static int round_rows_bf16(const float* src, int64_t M, int C, uint16_t* dst, int64_t ldo, hipStream_t st) {
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(M * C, 256), 8192);
  hipLaunchKernelGGL(round_rows_bf16_kernel, dim3(blocks), dim3(256), 0, st, src, M, C, dst, ldo);
  GRL_LAUNCH_CHECK();
  return GRL_OK;
}

// What the bf16-output entries check beyond graphconv_fwd_check (host-side,
// before any row is looked at).
static int out16_check(const char* who, const void* X, const void* out, int64_t ldo, int C) {
  GRL_CHECK_ARG(ldo >= C, "%s: need ldo >= C (ldo=%lld C=%d)", who, (long long)ldo, C);
  GRL_CHECK_ARG(reinterpret_cast<uintptr_t>(X) % 2 == 0 && reinterpret_cast<uintptr_t>(out) % 2 == 0,
                "%s: X and out hold 2-byte elements and must be 2-B aligned", who);
  return GRL_OK;
}

// The data gradient of one GraphConv layer by reassociation (see grl.h):
// dX = sum_s (A_drop,s^T G) W_s^T on the one-kernel GraphConv over the typed
// transpose.  Eligible when the shape is (grl_graphconv_bwd_data_shape_ok) and
// the call's pointers and plan are: a whole-range transpose, W 16 B-aligned,
// every row of G (GT = float, or uint16_t: bf16 bits) aligned to the gather's
// one load of a lane's 4 columns (16 B / 8 B) with its bytes fitting 32 bits,
// no heavy-row split plan, int32 entries.  grl_graphconv_bwd_data_bf16 (dX
// holds bf16 bits too, lddx apart a row) besides: the graphconv_bwd_bf16 path
// option on, and a dX row takes the epilogue's dword stores of two columns
// (an fp32 dX is [num_rows, F] contiguous, dX and lddx not looked at).
template <typename GT>
static bool bwd_data_path(const GrlTypedCsr* gt, const GT* G, int64_t ldg, int C, const float* W, int F, const GT* dX,
                          int64_t lddx) {
  if (std::is_same<GT, uint16_t>::value &&
      (opt(OPT_GRAPHCONV_BWD_BF16) == 0 || reinterpret_cast<uintptr_t>(dX) % 4 != 0 || lddx % 2 != 0))
    return false;
  return grl_graphconv_bwd_data_shape_ok(gt->num_rows, gt->num_types, gt->has_self, C, F) && gt->self_row0 == 0 &&
         al16(W) && reinterpret_cast<uintptr_t>(G) % (4 * sizeof(GT)) == 0 && ldg % 4 == 0 &&
         ldg < (int64_t)((1ULL << 32) / sizeof(GT)) && (!gt->split || gt->split->num_heavy == 0) &&
         gt->nnz < 2147483647LL;
}

// What grl_graphconv_fwd and _fwd_train check alike (`outs`: their outputs are
// non-NULL); *K = the linear's depth, set for a graph with rows.
static int graphconv_fwd_check(const char* who, const GrlTypedCsr* g, const void* X, int64_t ldx, int F,
                               const float* W, int C, bool outs, const void* ws, int32_t* K) {
  const int rc = csr_fwd_check(who, g, F, ldx, X && W && outs);
  if (rc) return rc;
  GRL_CHECK_ARG(C > 0, "%s: need C > 0 (got %d)", who, C);
  if (g->num_rows == 0) return GRL_OK;
  const int64_t K64 = (int64_t)segments(g) * F;
  GRL_CHECK_ARG(K64 <= 2147483647LL, "%s: (has_self + num_types) * F exceeds int32", who);
  GRL_CHECK_ARG(ws == nullptr || al16(ws), "%s: workspace must be 16-B aligned", who);
  *K = (int32_t)K64;
  return GRL_OK;
}

}  // namespace grl

using namespace grl;

// ---- the forward, written once for an fp32 table (XT = float) and a table of
// bf16 bits (XT = uint16_t; W, bias, out and Z are fp32 either way) ----------
// Z [num_rows, segments * F] = A_drop X: the first kernel of the two-kernel chain
static int spmm_fwd(const GrlTypedCsr* g, const float* X, int64_t ldx, int32_t F, float* Z, const GrlDropEdge* de,
                    grl_stream_t stream) {
  return grl_typed_spmm_fwd(g, X, ldx, F, Z, de, stream);
}
static int spmm_fwd(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F, float* Z, const GrlDropEdge* de,
                    grl_stream_t stream) {
  return grl_typed_spmm_fwd_bf16(g, X, ldx, F, 0, Z, (int64_t)segments(g) * F, F, de, stream);
}

// What a forward entry's workspace query answers: W's planes where the call
// takes one kernel, else the chain's total.  TRAIN: the entry writes Z.
template <bool TRAIN, typename XT, typename OT, typename ZT>
static size_t graphconv_fwd_query(const GrlTypedCsr* g, const XT* X, int64_t ldx, int32_t F, const float* W, int32_t C,
                                  const OT* out, int64_t ldo, const ZT* Z) {
  constexpr bool OUT16 = std::is_same<OT, uint16_t>::value;
  if (!g || g->num_rows <= 0 || g->num_types < 1 || F <= 0 || C <= 0 || (OUT16 && ldo < C)) return 0;
  const int64_t K = (int64_t)segments(g) * F;
  if (K > 2147483647LL) return 0;
  if (fwd_one_kernel(g, X, ldx, F, W, C, out, ldo, Z, TRAIN)) return graphconv_fused_ws_bytes(K, C);
  return fwd_chain_layout(g, K, C, OUT16, !TRAIN || std::is_same<ZT, uint16_t>::value).total;
}

// Every grl_graphconv_fwd* entry.  XT, OT, ZT: float, or uint16_t for bf16 bits
// (a bf16 out over a bf16 table only, a bf16 Z with a bf16 out only; W and bias
// are fp32).  TRAIN: Z [num_rows, segments * F] is written too; else Z is NULL.
// One kernel where the rule holds and the workspace takes W's planes; else the
// two-kernel chain over fwd_chain_layout; else, for inference over an fp32
// table, Z in row chunks.
template <bool TRAIN, typename XT, typename OT, typename ZT>
static int graphconv_fwd_run(const GrlTypedCsr* g, const XT* X, int64_t ldx, int32_t F, const float* W,
                             const float* bias, int32_t C, int32_t relu, OT* out, int64_t ldo, ZT* Z,
                             const GrlDropEdge* de, void* workspace, size_t workspace_bytes, grl_stream_t stream) {
  constexpr bool BF16 = std::is_same<XT, uint16_t>::value;
  constexpr bool OUT16 = std::is_same<OT, uint16_t>::value;
  constexpr bool Z16 = std::is_same<ZT, uint16_t>::value;
  static_assert(TRAIN || !Z16, "inference passes a NULL float* Z");
  constexpr int who_bit = ws_who_fwd(BF16, OUT16, Z16, TRAIN);
  const char* const who = who_name(who_bit);
  TraceRange trace_(who);
  int32_t K = 0;
  int rc = graphconv_fwd_check(who, g, X, ldx, F, W, C, out && (Z || !TRAIN), workspace, &K);
  if (rc) return rc;
  if constexpr (OUT16) {
    rc = out16_check(who, X, out, ldo, C);
    if (rc) return rc;
  }
  if constexpr (Z16)
    GRL_CHECK_ARG(reinterpret_cast<uintptr_t>(Z) % 2 == 0, "%s: Z holds 2-byte elements and must be 2-B aligned", who);
  if (g->num_rows == 0) return GRL_OK;
  const int64_t M = g->num_rows;
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  if (fwd_one_kernel(g, X, ldx, F, W, C, out, ldo, Z, TRAIN) && ws && workspace_bytes >= graphconv_fused_ws_bytes(K, C))
    return graphconv_fused_fwd(who_bit, g, X, ldx, F, W, bias, C, relu, out, ldo, de, ws, st, Z);  // Z stays on the CU
  const FwdChainLayout l = fwd_chain_layout(g, K, C, OUT16, !TRAIN || Z16);
  // (the fp32-out training entries put nothing of their own in the workspace: the linear takes all of it and
  // picks its arithmetic from the bytes it is given, so they refuse nothing here)
  if ((TRAIN && !OUT16) || (ws && workspace_bytes >= l.total)) {
    float* Z32 = reinterpret_cast<float*>(ws);  // the SpMM's target: the workspace's head, or the caller's fp32 Z
    if constexpr (TRAIN && !Z16) Z32 = Z;
    float* lin_out = reinterpret_cast<float*>(ws + l.lin_out);
    if constexpr (!OUT16) lin_out = out;
    rc = spmm_fwd(g, X, ldx, F, Z32, de, stream);
    if (!rc)
      rc = grl_linear_fwd_ex(Z32, K, W, 0, bias, lin_out, M, K, C, relu, g->path_rows, ws + l.lin_ws,
                             workspace_bytes - l.lin_ws, stream);
    if constexpr (OUT16) {
      if (!rc) rc = round_rows_bf16(lin_out, M, C, out, ldo, st);
    }
    if constexpr (Z16) {
      if (!rc) rc = round_rows_bf16(Z32, M, K, Z, (int64_t)K, st);
    }
    return rc;
  }
  if constexpr (TRAIN || BF16) {
    GRL_FAIL(GRL_E_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, l.total);  // no row-chunked form
  } else {
    // Row chunks: Z for R rows at a time (bounded memory), on the x6 GEMM only,
    // whose per-element arithmetic does not depend on M -- so the result is
    // bitwise that of the whole-graph call.
    const bool x6 = x6_path_ok(M, g->path_rows, C, K) && al16(W) && C % 4 == 0;
    if (!x6 || (g->split && g->split->num_heavy > 0) || !ws)
      GRL_FAIL(GRL_E_WORKSPACE, "%s: workspace %zu < %zu (row chunking needs the x6 GEMM shape and no heavy-row split "
               "plan)", who, workspace_bytes, grl_graphconv_fwd_workspace_size(M, g->num_types, g->has_self, F, C));
    const size_t planes_bytes = ws_align(x6_ws_bytes_p(M, g->path_rows, C, K));
    const int64_t per_row = (int64_t)K * 4;
    int64_t R = workspace_bytes > planes_bytes ? (int64_t)((workspace_bytes - planes_bytes) / per_row) : 0;
    R = R / LB_M * LB_M;
    if (R < LB_M)
      GRL_FAIL(GRL_E_WORKSPACE, "%s: workspace %zu holds fewer than %d rows of Z", who, workspace_bytes, LB_M);
    uint16_t* planes = reinterpret_cast<uint16_t*>(ws);
    float* Zr = reinterpret_cast<float*>(ws + planes_bytes);
    rc = x6_split_w(W, K, C, planes, st);
    for (int64_t r0 = 0; r0 < M && !rc; r0 += R) {
      const int64_t rows = std::min<int64_t>(R, M - r0);
      rc = spmm_fwd_rows(g, r0, rows, X, ldx, F, Zr, de, st);
      if (!rc) rc = x6_gemm_rows(Zr, rows, K, planes, C, bias, relu, out + r0 * C, st);
    }
    return rc;
  }
}

static float* const NO_Z = nullptr;  // inference: no Z is written

extern "C" size_t grl_graphconv_fwd_workspace_query(const GrlTypedCsr* g, const float* X, int64_t ldx, int32_t F,
                                                   const float* W, int32_t C) {
  return graphconv_fwd_query<false>(g, X, ldx, F, W, C, (const float*)nullptr, (int64_t)C, NO_Z);
}

extern "C" size_t grl_graphconv_fwd_bf16_workspace_query(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx,
                                                        int32_t F, const float* W, int32_t C) {
  return graphconv_fwd_query<false>(g, X, ldx, F, W, C, (const float*)nullptr, (int64_t)C, NO_Z);
}

extern "C" size_t grl_graphconv_fwd_bf16_to_bf16_workspace_query(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx,
                                                                int32_t F, const float* W, int32_t C,
                                                                const uint16_t* out, int64_t ldo) {
  return graphconv_fwd_query<false>(g, X, ldx, F, W, C, out, ldo, NO_Z);
}

extern "C" size_t grl_graphconv_fwd_train_bf16_z16_workspace_query(const GrlTypedCsr* g, const uint16_t* X,
                                                                  int64_t ldx, int32_t F, const float* W, int32_t C,
                                                                  const uint16_t* out, int64_t ldo,
                                                                  const uint16_t* Z) {
  return graphconv_fwd_query<true>(g, X, ldx, F, W, C, out, ldo, Z);
}

extern "C" size_t grl_graphconv_fwd_workspace_size(int64_t num_rows, int32_t num_types, int32_t has_self, int32_t F,
                                                   int32_t C) {
  if (num_rows <= 0 || num_types < 1 || F <= 0 || C <= 0) return 0;
  const int64_t K = (int64_t)segments(num_types, has_self) * F;
  if (K > 2147483647LL) return 0;
  return ws_align((size_t)num_rows * (size_t)K * 4) + grl_linear_fwd_workspace_size(num_rows, (int32_t)K, C);
}

extern "C" int grl_graphconv_fwd(const GrlTypedCsr* g, const float* X, int64_t ldx, int32_t F, const float* W,
                                 const float* bias, int32_t C, int32_t relu, float* out, const GrlDropEdge* de,
                                 void* workspace, size_t workspace_bytes, grl_stream_t stream) {
  return graphconv_fwd_run<false>(g, X, ldx, F, W, bias, C, relu, out, (int64_t)C, NO_Z, de, workspace,
                                  workspace_bytes, stream);
}

extern "C" int grl_graphconv_fwd_bf16(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F, const float* W,
                                      const float* bias, int32_t C, int32_t relu, float* out, const GrlDropEdge* de,
                                      void* workspace, size_t workspace_bytes, grl_stream_t stream) {
  return graphconv_fwd_run<false>(g, X, ldx, F, W, bias, C, relu, out, (int64_t)C, NO_Z, de, workspace,
                                  workspace_bytes, stream);
}

extern "C" int grl_graphconv_fwd_bf16_to_bf16(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F,
                                              const float* W, const float* bias, int32_t C, int32_t relu,
                                              uint16_t* out, int64_t ldo, const GrlDropEdge* de, void* workspace,
                                              size_t workspace_bytes, grl_stream_t stream) {
  return graphconv_fwd_run<false>(g, X, ldx, F, W, bias, C, relu, out, ldo, NO_Z, de, workspace, workspace_bytes,
                                  stream);
}

extern "C" int grl_graphconv_fwd_train(const GrlTypedCsr* g, const float* X, int64_t ldx, int32_t F, const float* W,
                                       const float* bias, int32_t C, int32_t relu, float* out, float* Z,
                                       const GrlDropEdge* de, void* workspace, size_t workspace_bytes,
                                       grl_stream_t stream) {
  return graphconv_fwd_run<true>(g, X, ldx, F, W, bias, C, relu, out, (int64_t)C, Z, de, workspace, workspace_bytes,
                                 stream);
}

extern "C" int grl_graphconv_fwd_train_bf16(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F,
                                            const float* W, const float* bias, int32_t C, int32_t relu, float* out,
                                            float* Z, const GrlDropEdge* de, void* workspace, size_t workspace_bytes,
                                            grl_stream_t stream) {
  return graphconv_fwd_run<true>(g, X, ldx, F, W, bias, C, relu, out, (int64_t)C, Z, de, workspace, workspace_bytes,
                                 stream);
}

extern "C" int grl_graphconv_fwd_train_bf16_to_bf16(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F,
                                                    const float* W, const float* bias, int32_t C, int32_t relu,
                                                    uint16_t* out, int64_t ldo, float* Z, const GrlDropEdge* de,
                                                    void* workspace, size_t workspace_bytes, grl_stream_t stream) {
  return graphconv_fwd_run<true>(g, X, ldx, F, W, bias, C, relu, out, ldo, Z, de, workspace, workspace_bytes, stream);
}

extern "C" int grl_graphconv_fwd_train_bf16_z16(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F,
                                                const float* W, const float* bias, int32_t C, int32_t relu,
                                                uint16_t* out, int64_t ldo, uint16_t* Z, const GrlDropEdge* de,
                                                void* workspace, size_t workspace_bytes, grl_stream_t stream) {
  return graphconv_fwd_run<true>(g, X, ldx, F, W, bias, C, relu, out, ldo, Z, de, workspace, workspace_bytes, stream);
}

extern "C" int32_t grl_graphconv_bwd_data_shape_ok(int64_t rows, int32_t num_types, int32_t has_self, int32_t C,
                                                   int32_t F) {
  const int64_t K = (int64_t)segments(num_types, has_self) * C;
  return graphconv_fused_enabled() && graphconv_fused_shape_ok(C, F, num_types) && x6_path_ok(rows, 0, F, K) &&
         F % 4 == 0 && K <= 2147483647LL;
}

// Both data-gradient entries.  GT = float: G fp32, dX [num_rows, F] contiguous
// (lddx = F); GT = uint16_t: both hold bf16 bits, dX's rows lddx apart, which
// has checks of its own (2-byte elements, strided dword stores into dX, the
// gather waves' 16 B stores into G_agg).
template <typename GT>
static int graphconv_bwd_data_run(const GrlTypedCsr* gt, const int32_t* eid, const GT* G, int64_t ldg, int64_t g_rows,
                                  int32_t C, const float* W, int32_t F, GT* dX, int64_t lddx, float* G_agg,
                                  const GrlDropEdge* de, void* workspace, size_t workspace_bytes,
                                  grl_stream_t stream) {
  constexpr bool BF16 = std::is_same<GT, uint16_t>::value;
  const char* const who = who_name(BF16 ? WS_WHO_BWD_DATA_BF16 : WS_WHO_BWD_DATA);
  TraceRange trace_(who);
  GRL_CHECK_ARG(gt != nullptr, "%s: graph is NULL", who);
  GRL_CHECK_ARG(gt->num_rows >= 0 && gt->num_types >= 1 && gt->num_types <= 63,
                "%s: num_types must be in [1, 63] (got %d)", who, gt->num_types);
  GRL_CHECK_ARG(C > 0 && ldg >= C && F > 0 && g_rows >= 0 && g_rows <= gt->num_rows,
                "%s: need C > 0, ldg >= C, F > 0, 0 <= g_rows <= num_rows", who);
  if constexpr (BF16) {
    GRL_CHECK_ARG(lddx >= F, "%s: need lddx >= F (lddx=%lld F=%d)", who, (long long)lddx, F);
    GRL_CHECK_ARG(reinterpret_cast<uintptr_t>(G) % 2 == 0 && reinterpret_cast<uintptr_t>(dX) % 2 == 0,
                  "%s: G and dX hold 2-byte elements and must be 2-B aligned", who);
  }
  if (gt->num_rows == 0) return GRL_OK;
  // (an empty node-range shard: no G rows and no entries, so its empty G is never read)
  GRL_CHECK_ARG((G || (g_rows == 0 && gt->nnz == 0)) && W && dX && gt->rowptr && (gt->nnz == 0 || (gt->colidx && eid)),
                "%s: NULL pointer", who);
  if constexpr (BF16)
    GRL_CHECK_ARG(al16(G_agg), "%s: G_agg must be 16-B aligned (the gather waves' 16 B row stores)", who);
  if (!bwd_data_path<GT>(gt, G, ldg, C, W, F, dX, lddx))
    GRL_FAIL(GRL_E_UNSUPPORTED, "%s: outside the one-kernel path (C %d, F %d, L %d, rows %lld, the operands' "
             "alignment%s; see %s_workspace_query)", who, C, F, gt->num_types, (long long)gt->num_rows,
             BF16 ? " or the graphconv_bwd_bf16 option" : "", who);
  const size_t need = graphconv_fused_ws_bytes((int64_t)segments(gt) * C, F);
  if (!workspace || !al16(workspace) || workspace_bytes < need)
    GRL_FAIL(GRL_E_WORKSPACE, "%s: workspace %zu < %zu (16-B aligned)", who, workspace_bytes, need);
  return graphconv_fused_bwd_data(gt, eid, G, ldg, g_rows, C, W, F, dX, lddx, G_agg, de, workspace, as_stream(stream));
}

extern "C" size_t grl_graphconv_bwd_data_workspace_query(const GrlTypedCsr* gt, const float* G, int64_t ldg, int32_t C,
                                                        const float* W, int32_t F) {
  if (!gt || gt->num_rows <= 0 || gt->num_types < 1 || C <= 0 || F <= 0) return 0;
  return bwd_data_path<float>(gt, G, ldg, C, W, F, nullptr, F) ? graphconv_fused_ws_bytes((int64_t)segments(gt) * C, F)
                                                              : 0;
}

extern "C" int grl_graphconv_bwd_data(const GrlTypedCsr* gt, const int32_t* eid, const float* G, int64_t ldg,
                                      int64_t g_rows, int32_t C, const float* W, int32_t F, float* dX, float* G_agg,
                                      const GrlDropEdge* de, void* workspace, size_t workspace_bytes,
                                      grl_stream_t stream) {
  return graphconv_bwd_data_run(gt, eid, G, ldg, g_rows, C, W, F, dX, (int64_t)F, G_agg, de, workspace,
                                workspace_bytes, stream);
}

extern "C" size_t grl_graphconv_bwd_data_bf16_workspace_query(const GrlTypedCsr* gt, const uint16_t* G, int64_t ldg,
                                                             int32_t C, const float* W, int32_t F, const uint16_t* dX,
                                                             int64_t lddx) {
  if (!gt || gt->num_rows <= 0 || gt->num_types < 1 || C <= 0 || F <= 0 || !dX || lddx < F || ldg < C) return 0;
  return bwd_data_path(gt, G, ldg, C, W, F, dX, lddx) ? graphconv_fused_ws_bytes((int64_t)segments(gt) * C, F) : 0;
}

extern "C" int grl_graphconv_bwd_data_bf16(const GrlTypedCsr* gt, const int32_t* eid, const uint16_t* G, int64_t ldg,
                                           int64_t g_rows, int32_t C, const float* W, int32_t F, uint16_t* dX,
                                           int64_t lddx, float* G_agg, const GrlDropEdge* de, void* workspace,
                                           size_t workspace_bytes, grl_stream_t stream) {
  return graphconv_bwd_data_run(gt, eid, G, ldg, g_rows, C, W, F, dX, lddx, G_agg, de, workspace, workspace_bytes,
                                stream);
}

namespace grl {
namespace {
// grl_check's read-and-clear in ONE atomic exchange, its old value written
// to a pinned host word: a poison kernel on another stream that lands
// between a read and a separate clear would lose its report.
__global__ void sticky_take_kernel(int* __restrict__ host_word) {
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_exchange(&g_grl_sticky, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(host_word, old, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
}  // namespace
}  // namespace grl

namespace grl {
namespace {
// grl_check's pinned host words: one per host thread at a time (virtual ranks
// check concurrently).  A thread takes a word from a process-wide free list
// (allocating only when the list is empty) and gives it back when it exits,
// so a session that starts fresh threads per run reuses the same few words
// instead of leaking one per thread.  Portable + coherent: usable whichever
// device a later check targets.
std::mutex g_word_mu;
std::vector<int*> g_free_words;
struct CheckWord {
  int* p = nullptr;
  ~CheckWord() {
    if (p) {
      std::lock_guard<std::mutex> lk(g_word_mu);
      g_free_words.push_back(p);
    }
  }
};
}  // namespace
}  // namespace grl

extern "C" int grl_check(grl_stream_t stream) {
  using namespace grl;
  hipStream_t st = as_stream(stream);
  thread_local CheckWord held;
  if (!held.p) {
    {
      std::lock_guard<std::mutex> lk(g_word_mu);
      if (!g_free_words.empty()) {
        held.p = g_free_words.back();
        g_free_words.pop_back();
      }
    }
    if (!held.p) {
      void* p = nullptr;
      GRL_HIP(hipHostMalloc(&p, sizeof(int), hipHostMallocCoherent | hipHostMallocPortable));
      held.p = static_cast<int*>(p);
    }
  }
  int* const word = held.p;
  *reinterpret_cast<volatile int*>(word) = 0;
  hipLaunchKernelGGL(sticky_take_kernel, dim3(1), dim3(64), 0, st, word);
  GRL_LAUNCH_CHECK();
  GRL_HIP(hipStreamSynchronize(st));
  const int h = *reinterpret_cast<volatile int*>(word);
  if (h == 0) return GRL_OK;
  char names[320];
  size_t n = 0;
  names[0] = 0;
  for (int i = 0; i < WS_WHO_COUNT; ++i)
    if (h & (1 << i)) n += snprintf(names + n, sizeof(names) - n, "%s%s", n ? ", " : "", who_name(1 << i));
  GRL_FAIL(GRL_E_TIMEOUT, "%s: a wave of the persistent GraphConv kernel gave up waiting on its LDS ring "
           "(bound %d sleeps); those calls' outputs were set to NaN", names, ws_spin_limit());
}
