// The body of the warp-specialised persistent GraphConv kernel, included by
// graphconv.hip once per kernel, inside the kernel's braces, with
// GRL_WS_BF16 defined: 0 = graphconv_ws_kernel (X fp32), 1 =
// graphconv_ws_bf16_kernel (X bf16 bits), and GRL_WS_OUT16: 1 (with
// GRL_WS_BF16 1) = graphconv_ws_bf16o_kernel, whose epilogue alone differs
// (out holds bf16 bits, ldo apart a row), or -- with EID true and eid /
// self_rows real arguments -- graphconv_ws_bf16g_kernel, the data-gradient
// form of that kernel.  GRL_WS_Z16: 1 (with both others 1, the forward form)
// = graphconv_ws_bf16oz_kernel, whose gather waves' copy of a finished row to
// Zout alone differs (bf16 bits; not defined = 0).  Textual sharing, not a function
// template: the fp32 kernels' machine code is pinned
// (tests/test_codegen_pin.py); an inlined function template around the body,
// and a traits class around the loads alone, each moved every one of them,
// so the fp32 text stands here as it was and the bf16 text beside it.  The
// body uses the kernel's parameters and template parameters by name (KS,
// VALS, EID, FV, PROD; eid and self_rows, which the bf16 kernel defines as
// constants).
//
// The table's element type touches the gather role's loads only.  bf16: a
// lane's 4 columns of a source row are 8 B of bf16 bits, kept as loaded -- 2
// dwords per row in flight instead of 4 -- and widened at the fmaf, exactly,
// so the fmaf chains, and with them the ring, Zout and out, are bitwise those
// of the fp32 kernel on the widened table.
  constexpr int FVW = KS * 16;                // columns per virtual segment
  constexpr int F = FVW * FV;                 // columns per segment
  constexpr int KC = FVW < WS_KC ? FVW : WS_KC;  // Z columns per unit
  constexpr int NH = FVW / KC;                // units per virtual segment
  constexpr int KSU = KC / 16;                // K16 steps per unit
  constexpr int CONS = WS_WAVES - PROD;       // MFMA waves
  constexpr int CB = CONS * WS_CB;            // 32-column blocks of W's planes (C <= 32 CB)
  constexpr int RW = WS_R / PROD;             // rows per gather wave
#if GRL_WS_BF16
  constexpr int U = RW > 8 ? GRL_WS_BF16_U16 : GRL_WS_BF16_U;  // neighbour rows in flight per gather wave
#else
  constexpr int U = RW > 8 ? GRL_WS_U16 : GRL_WS_U;  // neighbour rows in flight per gather wave
#endif
  static_assert(FV == 1 || FVW == WS_FV, "wide segments are cut into 256-column virtual segments");
  static_assert(NH < WS_NB, "a virtual segment's units are distinct ring slots, and one more is free");
  static_assert(PROD == 8 || PROD == 4, "8 gather + 4 MFMA waves, or 4 + 8 (two 8-row groups per gather wave)");
  __shared__ __attribute__((aligned(16))) float ring[WS_NB * WS_SLOT];
  __shared__ int produced[WS_NB], consumed[WS_NB];
  if (threadIdx.x < WS_NB) {
    produced[threadIdx.x] = 0;
    consumed[threadIdx.x] = 0;
  }
  __syncthreads();
  de = resolve_key(de);
  const int lane = threadIdx.x & 63;
  const int wave = uniform_i(threadIdx.x >> 6);
  const int S = L + hs;
  unsigned long long waited = 0;
#if GRL_WS_STAMP
  const unsigned long long t_start = __builtin_amdgcn_s_memtime();
  auto stamp_out = [&]() {
    if (lane == 0 && blockIdx.x < 1024) {
      g_ws_dbg[(blockIdx.x * 12 + wave) * 2] = waited;
      g_ws_dbg[(blockIdx.x * 12 + wave) * 2 + 1] = __builtin_amdgcn_s_memtime() - t_start;
    }
  };
#else
  auto stamp_out = [&]() {};
#endif

#if GRL_WS_ONLY_ROLE == 2
  if (false) {
#else
  if (wave < PROD) {
#endif
    // =========================== gather waves ===========================
    // A gather wave's RW rows are NG groups of GR = 8; each group's edges of a
    // segment stream as one list (the rowptr window of 8 rows fits one
    // register), the groups one after the other.
    constexpr int GR = 8;
    constexpr int NG = RW / GR;
#ifndef GRL_WS_SC
#define GRL_WS_SC 4
#endif
    constexpr int SC = GRL_WS_SC;        // self rows loaded per step
    const int col = lane * 4;            // this lane's 4 columns of the virtual segment
    const bool col_ok = col < FVW;
    const int part = col / KC;           // the unit (part of the virtual segment) they belong to
    const int ucol = col - part * KC;    // column within that unit
    int u = 0;                           // first unit of the current virtual segment
    // segment lists: lanes < GR hold row lane's range start b and the
    // inclusive count incl; the first 64 entries' source rows / weights are
    // fetched one list ahead
    struct List {
      int b, incl, exc, total, sidx;
      float w;
    };
    auto make_list = [&](int rp, int t) {
      List ls;
      const int r = min(lane, GR - 1);
      ls.b = __shfl(rp, r * L + t);
      const int e1 = __shfl(rp, r * L + t + 1);  // all lanes: ds_bpermute reads active lanes only
      const int cnt = lane < GR ? e1 - ls.b : 0;
      int incl = cnt;
#pragma unroll
      for (int d = 1; d < GR; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
      }
      ls.incl = incl;
      ls.exc = incl - cnt;
      ls.total = readlane_i(incl, GR - 1);
      return ls;
    };
    // list entries [c0, c0 + 64): source row and DropEdge weight (0 = dropped / past the end)
    auto fetch = [&](const List& ls, int c0, int& sidx, float& w) {
      const int pp = c0 + lane;
      int sl = 0;
#pragma unroll
      for (int i = 0; i < GR - 1; ++i) sl += pp >= readlane_i(ls.incl, i) ? 1 : 0;
      const int e = __shfl(ls.b, sl) + (pp - __shfl(ls.exc, sl));  // CSR position of entry pp
      sidx = 0;
      w = 0.0f;
      if (pp < ls.total) {
        sidx = colidx[e];
        const float v = VALS ? vals[e] : 1.0f;
        if (EID)
          w = de.active ? dropedge_weight(de, v, edge_base + (uint64_t)(uint32_t)eid[e]) : v;
        else
          w = de.active ? dropedge_weight(de, v, edge_base + (uint64_t)e) : v;
      }
    };
    for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
      const int64_t rw0 = tile * WS_R + wave * RW;
      const int nvalid = (int)max<int64_t>(0, min<int64_t>(RW, M - rw0));
      // rowptr window of each group's rows (lane l: rowptr[(rw0 + 8 g) L + l], l <= 8 L; rows past M read as empty)
      int rp[NG];
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        const int nv = max(0, min(GR, nvalid - gi * GR));
        rp[gi] = lane <= GR * L ? rowptr[min<int64_t>((rw0 + gi * GR) * L + min(lane, nv * L), M * L)] : 0;
      }
      List cur = make_list(rp[0], 0);
      fetch(cur, 0, cur.sidx, cur.w);
      for (int s = 0; s < S; ++s) {
#pragma unroll 1
        for (int hv = 0; hv < FV; ++hv, u += NH) {
          // claim the virtual segment's NH slots (this wave's rows only), once, before the first store
          bool have = false;
          auto claim = [&]() -> bool {
            if (have) return true;
#pragma unroll
            for (int q = 0; q < NH; ++q)
              if (!wait_ge(&consumed[(u + q) % WS_NB], CONS * ((u + q) / WS_NB), &waited, spin_limit, status))
                return false;
            have = true;
            return true;
          };
          float* const dst = ring + ((u + part) % WS_NB) * WS_SLOT + ucol + wave * RW * WS_LDF;
#if GRL_WS_BF16
          const uint16_t* const xs = X + hv * FVW + col;  // this lane's columns of the virtual segment
#else
          const float* const xs = X + hv * FVW + col;  // this lane's columns of the virtual segment
#endif
          // training forward (Zout): the row also goes to HBM for the weight
          // gradient, with non-temporal stores as spmm_kernel's
#if GRL_WS_Z16
          // GRL_WS_Z16: Zout holds bf16 bits (ldz counts them).  The ring keeps the unrounded fp32 row, so out
          // does not move; the HBM copy alone is rounded to nearest even, 8 B a lane instead of 16.
          uint16_t* const zrow = Zout ? Zout + rw0 * ldz + (int64_t)s * F + hv * FVW + col : nullptr;
          auto flush = [&](int r, const float4& v) {  // r: the wave's row
            if (col_ok) {
              *reinterpret_cast<float4*>(dst + r * WS_LDF) = v;
              if (zrow && r < nvalid) {
                typedef uint32_t z_u32x2_t __attribute__((ext_vector_type(2)));
                z_u32x2_t t = {cvt_pk_bf16(v.x, v.y), cvt_pk_bf16(v.z, v.w)};
                __builtin_nontemporal_store(t, reinterpret_cast<z_u32x2_t*>(zrow + (int64_t)r * ldz));
              }
            }
          };
#else
          float* const zrow = Zout ? Zout + rw0 * ldz + (int64_t)s * F + hv * FVW + col : nullptr;
          auto flush = [&](int r, const float4& v) {  // r: the wave's row
            if (col_ok) {
              *reinterpret_cast<float4*>(dst + r * WS_LDF) = v;
              if (zrow && r < nvalid) {
                f32x4_t t = {v.x, v.y, v.z, v.w};
                __builtin_nontemporal_store(t, reinterpret_cast<f32x4_t*>(zrow + (int64_t)r * ldz));
              }
            }
          };
#endif
          if (s < hs) {
            // identity block of A_pre (robust_gcn.py:58-65): the rows' own features, SC rows at a time
            // (a rolled loop: unrolled, the rows' loads and uniform DropEdge hashes crowd the registers)
#pragma unroll 1
            for (int i0 = 0; i0 < RW; i0 += SC) {
#if GRL_WS_BF16
              uint2 xb[SC];
#pragma unroll
              for (int i = 0; i < SC; ++i)
                xb[i] = (i0 + i < nvalid && rw0 + i0 + i < self_rows && col_ok)
                            ? *reinterpret_cast<const uint2*>(xs + (self_row0 + rw0 + i0 + i) * ldx) : make_uint2(0u, 0u);
#else
              float4 xv[SC];
#pragma unroll
              for (int i = 0; i < SC; ++i)
                xv[i] = (i0 + i < nvalid && rw0 + i0 + i < self_rows && col_ok)
                            ? *reinterpret_cast<const float4*>(xs + (self_row0 + rw0 + i0 + i) * ldx) : zero4();
#endif
              if (!claim()) return;
#if GRL_WS_BF16
              float4 xv[SC];
#pragma unroll
              for (int i = 0; i < SC; ++i) xv[i] = widen4(xb[i]);
#endif
#pragma unroll
              for (int i = 0; i < SC; ++i) {
                float w = 1.0f;
                if (de.active && de.drop_self) w = dropedge_weight(de, 1.0f, self_base + (uint64_t)(rw0 + i0 + i));
                flush(i0 + i, w != 0.0f ? make_float4(w * xv[i].x, w * xv[i].y, w * xv[i].z, w * xv[i].w) : zero4());
              }
            }
          } else {
#if GRL_WS_WHATIF & 8
            // what-if: the MFMA side alone (typed segments are never gathered)
            if (!claim()) return;
            for (int r = 0; r < RW; ++r) flush(r, zero4());
            if (false)
#endif
#pragma unroll 1
            for (int gi = 0; gi < NG; ++gi) {
              // the next list (next group; else the next segment's first, unless the next virtual part
              // of this segment re-walks this list) and its first 64 entries load while this one gathers
              List nxt = cur;
              if (gi + 1 < NG) {
                nxt = make_list(rp[NG - 1], s - hs);  // NG <= 2: the next group is the last
                fetch(nxt, 0, nxt.sidx, nxt.w);
              } else if (hv + 1 < FV) {
                if (NG > 1) {
                  nxt = make_list(rp[0], s - hs);
                  fetch(nxt, 0, nxt.sidx, nxt.w);
                }
              } else if (s + 1 < S) {
                nxt = make_list(rp[0], s + 1 - hs);
                fetch(nxt, 0, nxt.sidx, nxt.w);
              }
              int row = gi * GR;  // the wave's row being summed
              int bound = readlane_i(cur.incl, 0);
              float4 a4 = zero4();
              for (int c0 = 0; c0 < cur.total; c0 += 64) {
                int sidx = cur.sidx;
                float w = cur.w;
                if (c0 > 0) fetch(cur, c0, sidx, w);  // rows with more than 64 segment edges together
                uint64_t kept = __ballot(w != 0.0f);
                while (kept) {
                  int jj[U];
#pragma unroll
                  for (int q = 0; q < U; ++q) {
                    if (kept) {
                      jj[q] = __builtin_ctzll(kept);
                      kept &= kept - 1;
                    } else {
                      jj[q] = -1;
                    }
                  }
#if GRL_WS_BF16
                  uint2 xv[U];  // bf16 bits as loaded
#pragma unroll
                  for (int q = 0; q < U; ++q) {
                    if (jj[q] >= 0) {
                      const int src = readlane_i(sidx, jj[q]);
                      // the fp32 form's addressing (below) with row bytes ldx * 2 (ldx < 2^31)
                      const uint64_t ra = reinterpret_cast<uint64_t>(X + hv * FVW) +
                                          (uint64_t)(uint32_t)src * (uint32_t)(ldx * 2);
                      typedef __attribute__((address_space(1))) const uint16_t gbf16;
                      typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
                      typedef __attribute__((address_space(1))) const u32x2_t gvec2;
                      gbf16* const rowp = (gbf16*)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(ra >> 32)) << 32) |
                                                   (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)ra));
                      xv[q] = make_uint2(0u, 0u);
                      if (col_ok) {
                        const u32x2_t t = PROD == 4 ? __builtin_nontemporal_load((gvec2*)(rowp + col))
                                                    : *(gvec2*)(rowp + col);
                        xv[q] = make_uint2(t[0], t[1]);
                      }
                    }
                  }
#else
                  float4 xv[U];
#pragma unroll
                  for (int q = 0; q < U; ++q) {
                    if (jj[q] >= 0) {
                      const int src = readlane_i(sidx, jj[q]);
                      // the source row's address is wave-uniform: a scalar base + the lane's column
                      // offset (global_load's saddr form, no 64-bit VALU add per gathered row)
                      // (src, ldx >= 0 and ldx < 2^30: an unsigned 32 x 32 -> 64-bit product of bytes)
                      const uint64_t ra = reinterpret_cast<uint64_t>(X + hv * FVW) +
                                          (uint64_t)(uint32_t)src * (uint32_t)(ldx * 4);
                      typedef __attribute__((address_space(1))) const float gfloat;
                      typedef __attribute__((address_space(1))) const f32x4_t gvec4;
                      gfloat* const rowp = (gfloat*)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(ra >> 32)) << 32) |
                                                     (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)ra));
                      xv[q] = zero4();
                      if (col_ok) {
                        // C > 256: streaming loads, so the gathered rows (no reuse to speak of in L2) evict
                        // less of W's 11 MB of planes (1.3 % at F = C = 512, profiles/r05_ab_wide_ntx.txt)
                        const f32x4_t t = PROD == 4 ? __builtin_nontemporal_load((gvec4*)(rowp + col))
                                                    : *(gvec4*)(rowp + col);
                        xv[q] = make_float4(t[0], t[1], t[2], t[3]);
                      }
                    }
                  }
#endif
#pragma unroll
                  for (int q = 0; q < U; ++q) {
                    if (jj[q] >= 0) {
                      const int pos = c0 + jj[q];
                      while (pos >= bound) {  // rows finished before this entry (wave-uniform)
                        if (!claim()) return;
                        flush(row, a4);
                        a4 = zero4();
                        ++row;
                        bound = readlane_i(cur.incl, row - gi * GR);
                      }
#if GRL_WS_BF16
                      fma4(a4, readlane_f(w, jj[q]), widen4(xv[q]));
#else
                      fma4(a4, readlane_f(w, jj[q]), xv[q]);
#endif
                    }
                  }
                }
              }
              if (!claim()) return;
              for (; row < (gi + 1) * GR; ++row) {
                flush(row, a4);
                a4 = zero4();
              }
              cur = nxt;
            }
          }
          if (lane == 0)
#pragma unroll
            for (int q = 0; q < NH; ++q) lds_add_rel(&produced[(u + q) % WS_NB], 1);
        }
      }
    }
    stamp_out();
  } else {
#if GRL_WS_ONLY_ROLE == 1
    return;
#endif
    // =========================== MFMA waves ===========================
    const int c = wave - PROD;
    const int l32 = lane & 31, h = lane >> 5;
    constexpr int WSTEP = CB * 3 * FG_FRAG;     // bf16 between K16 steps of W
    const int nsteps = S * KS * FV;             // one tile's K16 steps (the W stream's period)
    // uniform base (SGPRs) + the lane's 16 B: saddr loads
    const uint16_t* wbase = Wf + (int64_t)(c * WS_CB) * 3 * FG_FRAG;
    const int loff = lane * 8;
    auto load_b = [&](bf16x8_t (&bb)[WS_CB][3], int gstep) {
#if GRL_WS_WHATIF & 1
      gstep = gstep & 1;  // what-if (timing only): a 2-step W stream that stays in L2
#endif
      const uint16_t* w = wbase + (int64_t)gstep * WSTEP;
#pragma unroll
      for (int j = 0; j < WS_CB; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q) bb[j][q] = *reinterpret_cast<const bf16x8_t*>(w + (j * 3 + q) * FG_FRAG + loff);
    };
    f32x16 acc[2][WS_CB];  // [row block][column block]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < WS_CB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    // 12 MFMAs of row block i against both column blocks
    auto mma = [&](int i, const bf16x8_t (&b)[WS_CB][3], const bf16x8_t (&a)[3]) {
#pragma unroll
      for (int j = 0; j < WS_CB; ++j) x6_mfma(acc[i][j], a, b[j]);
    };
    // this lane's 8 k (step ks) of row i*32 + l32 of a fp32 ring unit
    auto read_a = [&](const float* zs, int ks, int i, float4& v0, float4& v1) {
      const float* ar = zs + (i * 32 + l32) * WS_LDF + ks * 16 + h * 8;
      v0 = *reinterpret_cast<const float4*>(ar);
      v1 = *reinterpret_cast<const float4*>(ar + 4);
    };
    auto split_a = [&](const float4& v0, const float4& v1, bf16x8_t (&a)[3]) {
#if GRL_WS_WHATIF & 2
      a[0] = __builtin_bit_cast(bf16x8_t, make_uint4(__float_as_uint(v0.x), __float_as_uint(v0.y), __float_as_uint(v1.x), __float_as_uint(v1.y)));
      a[1] = __builtin_bit_cast(bf16x8_t, make_uint4(__float_as_uint(v0.z), __float_as_uint(v0.w), __float_as_uint(v1.z), __float_as_uint(v1.w)));
      a[2] = a[0];  // what-if (timing only): no split VALU
      return;
#endif
      uint2 p0, p1, p2, r0, r1, r2;
      split3(v0, p0, p1, p2);
      split3(v1, r0, r1, r2);
      a[0] = __builtin_bit_cast(bf16x8_t, make_uint4(p0.x, p0.y, r0.x, r0.y));
      a[1] = __builtin_bit_cast(bf16x8_t, make_uint4(p1.x, p1.y, r1.x, r1.y));
      a[2] = __builtin_bit_cast(bf16x8_t, make_uint4(p2.x, p2.y, r2.x, r2.y));
    };
    // scheduling hint for the region just written: 2 MFMAs, then 3 VALU / 1 MFMA
    auto interleave = [&]() {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
#pragma unroll
      for (int q = 0; q < 10; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
    };
    bf16x8_t bb[2][WS_CB][3];
    int nxt = 0;  // K16 step (within the tile) of the next W fragments to load
    load_b(bb[0], nxt);
    nxt = nxt + 1 == nsteps ? 0 : nxt + 1;
    int u = 0;
    for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
      for (int su = 0; su < S * FV * NH; ++su, ++u) {
        const int slot = u % WS_NB, g = u / WS_NB;
        const float* zs = ring + slot * WS_SLOT;
        if (!wait_ge(&produced[slot], PROD * (g + 1), &waited, spin_limit, status)) return;
#if GRL_WS_WHATIF & 4
        if (lane == 0) lds_add_rel(&consumed[slot], 1);  // what-if: the gather alone
        continue;
#endif
        // Software-pipelined by row block: the split of the next row block's
        // A fragments (VALU) is interleaved with the current row block's 12
        // MFMAs (an MFMA holds the SIMD's issue for 8 of its 32 cycles; the
        // VALU fits in the rest), instead of running between them.
        bf16x8_t pa[2][3];
        {
          float4 v0, v1;
          read_a(zs, 0, 0, v0, v1);
          split_a(v0, v1, pa[0]);
        }
#pragma unroll
        for (int ks = 0; ks < KSU; ++ks) {  // KSU is even: the stage of step ks is ks & 1
          load_b(bb[(ks + 1) & 1], nxt);
          nxt = nxt + 1 == nsteps ? 0 : nxt + 1;
          const int st = ks & 1;
          float4 v0, v1;
          read_a(zs, ks, 1, v0, v1);
          __builtin_amdgcn_sched_barrier(0);
          mma(0, bb[st], pa[0]);
          split_a(v0, v1, pa[1]);
          interleave();
          __builtin_amdgcn_sched_barrier(0);
          if (ks + 1 < KSU) read_a(zs, ks + 1, 0, v0, v1);
          __builtin_amdgcn_sched_barrier(0);
          mma(1, bb[st], pa[1]);
          if (ks + 1 < KSU) split_a(v0, v1, pa[0]);
          interleave();
          __builtin_amdgcn_sched_barrier(0);
        }
        // the slot's A fragments are in registers once their reads returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) lds_add_rel(&consumed[slot], 1);
      }
      // tile done: bias + ReLU, as gemm_x6_kernel
      const int64_t m0 = tile * WS_R;
      const bool epi = bias != nullptr || relu;
#if GRL_WS_OUT16
      // bf16 rows (the fp32 value rounded to nearest even) with the caller's
      // stride ldo; the two blocks of the fp32 form below -- whole tile, ragged
      // tile with per-element row bounds -- as one text over WHOLE.
      // GRL_WS_OUT16_PACK: lanes l and l ^ 1 (columns n, n + 1; C % 4 == 0, so
      // both or neither are < C) trade one value of each register pair (2p,
      // 2p + 1: rows m, m + 1); the even lane then stores row m's columns
      // (n, n + 1) as one dword, the odd lane row m + 1's (n - 1, n): out is
      // 4 B-aligned and ldo even.  Else one 2 B store per element.
      auto store_tile = [&](auto whole_c) {
        constexpr bool WHOLE = decltype(whole_c)::value;
#pragma unroll
        for (int j = 0; j < WS_CB; ++j) {
          const int n = (c * WS_CB + j) * 32 + l32;
          const float bv = (bias && n < C) ? bias[n] : 0.0f;
          auto fin = [&](float v) {
            if (epi) {
              v = v + bv;
              if (relu) v = v > 0.0f ? v : 0.0f;
            }
            return v;
          };
#if GRL_WS_OUT16_PACK
          const int odd = lane & 1;
          const int64_t mr = m0 + 4 * h + odd;  // this lane's row of register pair 0
          uint16_t* const o = out + mr * ldo + (n - odd);
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int p = 0; p < 8; ++p) {
              const float v0 = fin(acc[i][j][2 * p]), v1 = fin(acc[i][j][2 * p + 1]);
              const float got = swap_lane_pair(odd ? v0 : v1);  // the neighbour column's value of this lane's row
              const uint32_t pk = odd ? cvt_pk_bf16(got, v1) : cvt_pk_bf16(v0, got);
              const int row = i * 32 + ((2 * p) & 3) + 8 * (p >> 1);
              if (n < C && (WHOLE || mr + row < M)) *reinterpret_cast<uint32_t*>(o + (int64_t)row * ldo) = pk;
              acc[i][j][2 * p] = 0.0f;
              acc[i][j][2 * p + 1] = 0.0f;
            }
#else
          const int64_t mr = m0 + 4 * h;
          uint16_t* const o = out + mr * ldo + n;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = i * 32 + (r & 3) + 8 * (r >> 2);
              if (n < C && (WHOLE || mr + row < M))
                o[(int64_t)row * ldo] = (uint16_t)cvt_pk_bf16(fin(acc[i][j][r]), 0.0f);
              acc[i][j][r] = 0.0f;
            }
#endif
        }
      };
      if (m0 + WS_R <= M)  // wave-uniform
        store_tile(std::true_type{});
      else
        store_tile(std::false_type{});
#else
      if (m0 + WS_R <= M) {  // whole tile (wave-uniform): row offsets are uniform multiples of C
#pragma unroll
        for (int j = 0; j < WS_CB; ++j) {
          const int n = (c * WS_CB + j) * 32 + l32;
          const float bv = (bias && n < C) ? bias[n] : 0.0f;
          float* const o = out + (m0 + 4 * h) * C + n;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              float v = acc[i][j][r];
              if (epi) {
                v = v + bv;
                if (relu) v = v > 0.0f ? v : 0.0f;
              }
              if (n < C) o[(int64_t)(i * 32 + (r & 3) + 8 * (r >> 2)) * C] = v;
              acc[i][j][r] = 0.0f;
            }
        }
        continue;
      }
#pragma unroll
      for (int j = 0; j < WS_CB; ++j) {
        const int n = (c * WS_CB + j) * 32 + l32;
        const float bv = (bias && n < C) ? bias[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m < M && n < C) {
              float v = acc[i][j][r];
              if (epi) {
                v = v + bv;
                if (relu) v = v > 0.0f ? v : 0.0f;
              }
              out[m * C + n] = v;
            }
            acc[i][j][r] = 0.0f;
          }
      }
#endif
    }
    stamp_out();
  }
