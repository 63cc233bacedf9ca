/*
 * grl.h — C ABI of the MI355X (gfx950) message-passing engine behind
 * gnn.models.GraphCNNDropEdge / gnn.models.networks.robust_gcn.GraphConv.
 *
 * The reference (hoangthanh283/graph-representation-learning) is pure
 * Python/PyTorch and has no FFI; every entry point below replaces one aten
 * call (or one block of Python) on its GraphConv/DropEdge hot path.  The
 * citation on each function names the reference code it stands in for
 * (paths relative to the reference repository root).  A maintainer binds
 * these with ctypes; nothing here mentions torch.
 *
 * Conventions
 *  - Every pointer marked "device" is HBM memory owned by the caller (torch
 *    caching allocator).  The library never allocates or frees persistent
 *    memory; scratch comes from a caller workspace sized by *_workspace_size.
 *  - Every call is stream-ordered on `stream` (a hipStream_t passed as void*,
 *    NULL = default stream) and never synchronises the device, so calls can
 *    be captured into a hipGraph.  Failures found on the device are
 *    stream-ordered too: where grl_graphconv_fwd, grl_graphconv_fwd_train
 *    and grl_graphconv_bwd_data run their persistent one-kernel form, a
 *    follow-up kernel fills that call's outputs with NaN if a bounded wait
 *    ran out and records the entry point in a sticky per-device status word;
 *    grl_check() (the caller's existing sync point: a loss.item(), an event
 *    wait) reads and clears that word and returns GRL_E_TIMEOUT.
 *  - Return value 0 = success, negative GRL_E_* = failure; grl_last_error()
 *    returns a thread-local message for the last failure on this thread.
 *  - Empty operands: an operand with no rows (an empty torch tensor, whose
 *    data pointer is NULL) may be NULL whenever the call reads none of it --
 *    e.g. a node-range shard with no own rows: its typed-SpMM backward,
 *    ReLU/bias gradient (db = 0), weight gradient (dW = 0, db = 0) and
 *    one-kernel data gradient succeed and write zeros where they write.
 *  - fp32 features, int32 indices.  Sums over a row's edges run in CSR order
 *    with one fmaf per edge, so results are bitwise reproducible run to run
 *    (no float atomics anywhere).
 */
#ifndef GRL_H_
#define GRL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* grl_stream_t; /* hipStream_t */

enum {
  GRL_OK = 0,
  GRL_E_INVALID = -1,     /* bad shape / null pointer / inconsistent sizes   */
  GRL_E_UNSUPPORTED = -2, /* well-formed request this build does not handle  */
  GRL_E_HIP = -3,         /* a HIP runtime call failed                       */
  GRL_E_WORKSPACE = -4,   /* workspace smaller than *_workspace_size()       */
  GRL_E_OVERFLOW = -5,    /* a count does not fit the int32 index type       */
  GRL_E_TIMEOUT = -6      /* a persistent kernel's bounded wait ran out; its  */
                          /* outputs are invalid (see grl_graphconv_fwd)      */
};

/*
 * Heavy-row split plan (load balance for power-law graphs, e.g. R-MAT hubs).
 * A row whose edge count exceeds `threshold` is not gathered by one
 * wavefront: each of its segments is cut into chunks of at most
 * `chunk_edges` edges, every chunk is summed by its own wavefront into
 * `partials` (num_chunks x F floats), and a fixup pass adds a segment's
 * chunk partials in chunk order (deterministic, no atomics).  Built once per
 * graph by grl_split_plan_count / grl_split_plan_build; attach it to the
 * GrlTypedCsr / GrlTypedCsc `split` field (NULL = no splitting).
 */
typedef struct GrlSplitPlan {
  int32_t threshold;          /* rows with more edges than this are split   */
  int32_t chunk_edges;        /* max edges per chunk                         */
  int64_t num_heavy;          /* heavy segments (all segments of heavy rows) */
  int64_t num_chunks;
  const int32_t* heavy_seg;   /* device [num_heavy]: segment id row*nseg+t   */
  const int32_t* heavy_cptr;  /* device [num_heavy+1]: chunk range per seg   */
  const int32_t* chunk_begin; /* device [num_chunks]: first edge position    */
  const int32_t* chunk_end;   /* device [num_chunks]: one past last edge     */
  float* partials;            /* device scratch, >= num_chunks * F floats    */
  int64_t partials_capacity;  /* floats available in `partials`              */
} GrlSplitPlan;

/*
 * Typed CSR: the sparse form of the reference's preprocessed adjacency
 * A_pre[b, n*(L+1)+l, m] (gnn/models/networks/robust_gcn.py:53-72).
 * Row segment (n, t) for t in [0, num_types) lists the source rows m whose
 * features node n aggregates through edge type t, i.e. the nonzeros of
 * A_in[b, n, t, m] in the collate layout (B, N, L, N).  With has_self = 1 the
 * identity block l = 0 of A_pre is implicit (robust_gcn.py:58-65) and output
 * segment 0 of row n is the node's own feature row.
 *
 * Z row n has (has_self + num_types) segments of F floats:
 *   Z[n, has_self + t, :] = sum_{e in seg(n,t)} w_e * X[colidx[e], :]
 *   Z[n, 0, :]            = w_self(n) * X[n, :]             (if has_self)
 * which is exactly new_V of robust_gcn.py:45-47 for one graph of the batch.
 */
typedef struct GrlTypedCsr {
  int64_t num_rows;      /* destination nodes (rows of Z)                     */
  int32_t num_types;     /* typed segments per node (L, num_edges)            */
  int32_t has_self;      /* 1: implicit identity segment 0                    */
  const int32_t* rowptr; /* device [num_rows*num_types + 1], rowptr[0] == 0   */
  const int32_t* colidx; /* device [nnz]: source row of X                     */
  const float* vals;     /* device [nnz] edge values, or NULL for all-ones    */
  int64_t nnz;
  uint64_t edge_id_base; /* global DropEdge id of colidx[0] (node-range shard)*/
  uint64_t self_id_base; /* global DropEdge id of row 0's self loop           */
  const GrlSplitPlan* split; /* heavy-row plan over rowptr, or NULL           */
  int64_t self_row0;     /* X row of row 0's self term (0; a row-range view of
                            a graph -- rowptr a slice, the identity rows from
                            this row on -- sets its first row).  Forward entry
                            points only: grl_csr_to_csc and
                            grl_graphconv_bwd_data require 0.               */
  int64_t path_rows;     /* rows the GEMM path (split-bf16 x6 or fp32) is
                            chosen for; 0 = num_rows.  A node-range shard (or
                            a row-range view) passes the whole graph's row
                            count, so its rows take the one-GPU layer's path:
                            with it, every output row is bitwise the whole
                            graph's (both paths' per-row arithmetic is
                            independent of the row count).                   */
} GrlTypedCsr;

/*
 * Transposed typed CSR (CSC over source rows), used by the backward pass
 * dX = A_drop^T dZ (the BmmBackward0 of robust_gcn.py:45).
 *   dX[m, :] = w_self(m) * dZ[m, 0, :]  (m < self_rows, if has_self)
 *            + sum_{i in col(m)} w_{eid[i]} * dZ_rows[zrow[i], :]
 * where dZ_rows is dZ viewed as contiguous rows of F floats, so
 * zrow = n*(has_self+num_types) + has_self + t for edge (n, t, m).
 */
typedef struct GrlTypedCsc {
  int64_t num_rows;      /* rows of dX (local + halo rows in a shard)         */
  int64_t self_rows;     /* rows that own a self loop (local rows)            */
  int32_t num_types;
  int32_t has_self;
  const int32_t* colptr; /* device [num_rows + 1]                              */
  const int32_t* zrow;   /* device [nnz]                                       */
  const int32_t* eid;    /* device [nnz]: CSR position of the edge (local)     */
  const float* vals;     /* device [nnz] values in CSC order, or NULL          */
  int64_t nnz;
  uint64_t edge_id_base; /* as in the matching GrlTypedCsr                     */
  uint64_t self_id_base;
  const GrlSplitPlan* split; /* heavy-column plan over colptr, or NULL        */
} GrlTypedCsc;

/*
 * DropEdge: the reference's nn.Dropout(p) applied to A_pre
 * (gnn/models/networks/drop_robust_gcn.py:38,76,80,85) as a fused,
 * regenerable mask.  An entry with global id `id` is kept iff
 *   grl_dropedge_bits(key, id) >= threshold,   weight = value * scale,
 * with scale = float(1/(1-p)) as torch's native dropout computes it.
 * Edge ids are CSR positions (+ edge_id_base); the self loop of global node g
 * has id E_total + g.  No mask tensor ever exists.
 */
typedef struct GrlDropEdge {
  uint64_t key;       /* grl_dropedge_key(seed, call_id)                       */
  uint32_t threshold; /* floor(p * 2^32); 0 keeps everything                   */
  float scale;        /* 1/(1-p) (0 when p >= 1); 1 when p == 0                */
  int32_t active;     /* 0: identity (eval mode / p == 0)                      */
  int32_t drop_self;  /* 1: the identity block is masked too (efficient_mode)  */
  /* Device-resident stream (HIP-graph replays): when seed_dev != NULL every
   * kernel derives key = grl_dropedge_key(*seed_dev, call_id) at launch
   * instead of using `key`, so a captured training step draws a fresh mask
   * on each replay from a seed written on the device (e.g. by the RNG kernel
   * captured with it).  NULL for grl_dropedge_init.                        */
  const uint64_t* seed_dev;
  uint64_t call_id;
} GrlDropEdge;

/* Library identity / errors. */
const char* grl_version(void);
const char* grl_last_error(void);

/* Sticky device status of the current device: waits for `stream`, reads the
 * word the persistent kernels' follow-up kernels set (see Conventions) and
 * clears it.  GRL_OK, or GRL_E_TIMEOUT naming every entry point whose
 * outputs were invalidated (NaN) since the last check.  The one call that
 * synchronises; meant for points where the caller syncs anyway (the
 * reference's loss.item(), kv_procedure.py:140; an event wait).  Not
 * capturable.                                                              */
int grl_check(grl_stream_t stream);

/* Path options: the test / A-B hooks that pick among the kernel forms of one
 * entry point (e.g. "gemm_x6" 0 = the fp32-MFMA GEMMs, "graphconv_fused" 0 =
 * SpMM + GEMM instead of the one-kernel layer, "attn_x6" 0 = the fp32-MFMA
 * attention kernels, "ws_spin" = the persistent kernels' wait bound).  The
 * defaults are the production paths; every form computes the same result
 * within its documented tolerance.  Process-wide, read at each call (a
 * workspace query and the call it sizes must see the same settings).  The
 * names and ranges are listed in csrc/common.hip; an unknown name or an
 * out-of-range value is GRL_E_INVALID.  Nothing in the library reads the
 * environment.                                                             */
int grl_set_option(const char* name, int64_t value);
int grl_get_option(const char* name, int64_t* value);

/* roctx ranges (rocprofv3 --marker-trace): the hot entry points push their
 * own; these let a host layer bracket its steps, e.g. the halo exchange of a
 * node-range shard (grl/dist.py).  Pop closes the innermost open range.   */
void grl_trace_push(const char* name);
void grl_trace_pop(void);

/* Fills *de for drop probability p, RNG stream (seed, call_id).
 * drop_self = 1 reproduces efficient_mode=True (drop_robust_gcn.py:69,76):
 * the mask covers the identity block; 0 reproduces efficient_mode=False,
 * where dropout hits raw A before preprocess_adj adds the identity.
 * Host-only, no device work.  Replaces nn.Dropout.__init__/bernoulli_ setup. */
int grl_dropedge_init(GrlDropEdge* de, float p, uint64_t seed, uint64_t call_id,
                      int32_t drop_self);

/* As grl_dropedge_init, with the seed read on the device at each launch
 * from *seed_dev (device memory, 8 bytes; must stay valid while `de` is used,
 * including by graph replays).  Host-only, no device work.                 */
int grl_dropedge_init_device(GrlDropEdge* de, float p, const uint64_t* seed_dev,
                             uint64_t call_id, int32_t drop_self);

/* Feature dropout on node rows (nn.Dropout(p) at drop_robust_gcn.py:64,77,81,
 * 86,100): out[r][c] = x[r][c] * scale if element id (row0 + r) * cols + c
 * survives `de` (the DropEdge hash and keep rule above; the caller gives the
 * feature draws their own call ids), else 0.  row0 = the global row of x's
 * first row (a node-range shard's row_begin), so every row's mask is the
 * one-GPU model's wherever the row is computed.  The backward is the same
 * call on the gradient.  x / out [rows][ld*] fp32 (out may alias x).      */
int grl_feature_dropout(const float* x, int64_t ldx, float* out, int64_t ldo,
                        int64_t rows, int32_t cols, int64_t row0,
                        const GrlDropEdge* de, grl_stream_t stream);

/* grl_feature_dropout over bf16 bits: the same element ids, hash and keep
 * rule, so a column slice of a table with cols = C draws exactly the fp32
 * model's mask for that layer.  out is bitwise grl_feature_dropout on the
 * widened x, rounded once to nearest even: a kept element is
 * RNE_bf16(float(x) * scale), a dropped one bf16 +0, and an inactive record
 * copies the bits.  x / out: rows ldx / ldo >= cols ELEMENTS apart (a column
 * slice of a wider table is a valid operand), 2-B aligned; out may alias x
 * (the pass runs in place).  16 B per lane where both pointers are 16-B
 * aligned and cols, ldx, ldo are multiples of 8, 8 B on the matching 8-B /
 * multiple-of-4 conditions, else one element per lane -- the same bits.
 * Errors as grl_feature_dropout; an odd address is GRL_E_INVALID.  No host
 * sync.                                                                    */
int grl_feature_dropout_bf16(const uint16_t* x, int64_t ldx, uint16_t* out,
                             int64_t ldo, int64_t rows, int32_t cols,
                             int64_t row0, const GrlDropEdge* de,
                             grl_stream_t stream);

/*
 * BatchNorm1d over node rows with its LeakyReLU: the reference's
 * x.permute(0, 2, 1) -> nn.BatchNorm1d -> permute back -> F.leaky_relu of
 * GCNBlock / EmbeddingBlock (gnn/models/networks/deep_rp_robust_gcn.py:39-45,
 * 57-63) on the row-major table as it lies, without a transposed copy.
 * Every table is fp32 [rows][ld*] with ld* >= cols (a column slice of a wider
 * table is a valid operand); gamma, beta, the statistics and the parameter
 * gradients are contiguous fp32 [cols].  Channel c's statistics run over all
 * `rows` values of column c.  Sums accumulate in fp64 (a widened fp32 value
 * and the product of two are exact there) per row block, the blocks' partials
 * are added in block order by one thread per column, and mean / invstd are
 * rounded to fp32 once.  The row blocks are a function of (rows, cols) only,
 * never of the device, and nothing is atomic: the same input gives the same
 * bits run to run and machine to machine.  Rows take 16 B per lane where
 * cols and every row stride are multiples of 4 and every table pointer is
 * 16-B aligned, else 4 B per lane -- the same bits either way.  Any
 * cols >= 1.  rows == 0 or cols == 0: GRL_OK, nothing is launched.  Errors
 * (GRL_E_INVALID): a negative size, a row stride below cols, a NULL table, a
 * workspace below grl_bn_rows_workspace_size or not 8-B aligned.  No
 * allocation, no host sync.
 */

/* Bytes of the partials workspace of grl_bn_rows_fwd_train and
 * grl_bn_rows_bwd for a [rows][cols] table (0 for an empty one).          */
size_t grl_bn_rows_workspace_size(int64_t rows, int32_t cols);

/* Training forward: save_mean[c] = mean of column c, save_invstd[c] =
 * 1 / sqrt(biased variance + eps), then
 *   y = leaky(gamma * (x - mean) * invstd + beta, slope),
 * leaky(v, s) = v > 0 ? v : v * s.  gamma / beta NULL = 1 / 0.  Where non-NULL
 * the running statistics are updated in place as torch does:
 *   running_mean = (1 - momentum) * running_mean + momentum * mean
 *   running_var  = (1 - momentum) * running_var
 *                  + momentum * variance * rows / (rows - 1).
 * rows == 1 is GRL_E_INVALID (torch refuses one value per channel in
 * training).  Three kernels: statistics, finalize, apply; x is read twice and
 * y written once.                                                          */
int grl_bn_rows_fwd_train(const float* x, int64_t ldx, int64_t rows, int32_t cols,
                          const float* gamma, const float* beta, float eps,
                          float slope, float momentum, float* running_mean,
                          float* running_var, float* y, int64_t ldy,
                          float* save_mean, float* save_invstd, void* workspace,
                          size_t ws_bytes, grl_stream_t stream);

/* Inference forward, one pass:
 *   y = leaky(gamma * (x - running_mean) / sqrt(running_var + eps) + beta, slope)
 * with the per-column scale formed in the kernel.  gamma / beta NULL = 1 / 0.
 * y may alias x.                                                           */
int grl_bn_rows_fwd_eval(const float* x, int64_t ldx, int64_t rows, int32_t cols,
                         const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var,
                         float eps, float slope, float* y, int64_t ldy,
                         grl_stream_t stream);

/* Backward of grl_bn_rows_fwd_train from its x, y, save_mean, save_invstd.
 *   g = dy * (y > 0 ? 1 : slope)   (the sign of y is the pre-activation's for
 *       every slope >= 0; y == 0 takes slope, as torch's leaky_relu backward)
 *   xhat = (x - mean) * invstd
 *   dbeta = sum_r g, dgamma = sum_r g * xhat        (written where non-NULL)
 *   dx = gamma * invstd * (g - dbeta / rows - xhat * dgamma / rows)
 * gamma NULL = 1.  dx may alias dy.  Three kernels: partial sums, finalize,
 * apply.  slope must be the forward's.                                     */
int grl_bn_rows_bwd(const float* dy, int64_t lddy, const float* y, int64_t ldy,
                    const float* x, int64_t ldx, int64_t rows, int32_t cols,
                    const float* gamma, const float* save_mean,
                    const float* save_invstd, float slope, float* dx,
                    int64_t lddx, float* dgamma, float* dbeta, void* workspace,
                    size_t ws_bytes, grl_stream_t stream);

/* keep[i] = 1 if id_base + i survives DropEdge `de`, else 0 (i < count).
 * Exposes the fused mask for parity checks against the dense reference
 * (the mask nn.Dropout would draw over A_pre, drop_robust_gcn.py:76).    */
int grl_dropedge_mask(const GrlDropEdge* de, uint64_t id_base, int64_t count,
                      uint8_t* keep /* device */, grl_stream_t stream);

/* ---------------------------------------------------------------------- */
/* Hot path                                                                */
/* ---------------------------------------------------------------------- */

/* Z = A_drop X in typed-CSR form.  Replaces
 *   new_V = torch.matmul(A, V.view(-1, N, F)).view(-1, N, (L+1)*F)
 * (gnn/models/networks/robust_gcn.py:45-47) together with the edge_dropout
 * applied to A right before it (drop_robust_gcn.py:76,80,85).
 * X: device, row stride ldx floats (>= F).  Z: device, contiguous
 * [num_rows, (has_self+num_types)*F].  de may be NULL (eval).            */
int grl_typed_spmm_fwd(const GrlTypedCsr* g, const float* X, int64_t ldx,
                       int32_t F, float* Z, const GrlDropEdge* de,
                       grl_stream_t stream);

/* Column slice of Z = A_drop X, for the pipelined halo exchange of a
 * node-range shard (grl/dist.py): the aggregation of
 * robust_gcn.py:45-47 restricted to F feature columns, so columns whose halo
 * rows have arrived are aggregated while the next slice is still in flight.
 *   Z[n*ldz + s*zseg + j] = segment s of row n, column j < F
 *   (s < has_self+num_types; Z points at the slice's first column),
 * the self term of row n reads X row self_col0 + n (the shard's own rows
 * inside a gathered table).  X: the slice's table, row stride ldx >= F.
 * Per element the same edges in the same order as grl_typed_spmm_fwd, so a
 * sliced aggregation is bitwise equal to the whole one.                     */
int grl_typed_spmm_fwd_slice(const GrlTypedCsr* g, const float* X, int64_t ldx,
                             int32_t F, int64_t self_col0, float* Z,
                             int64_t ldz, int32_t zseg, const GrlDropEdge* de,
                             grl_stream_t stream);

/* Z = A_drop X with X stored as bf16 bits (the upper 16 bits of the fp32
 * value, as torch.bfloat16 keeps them); ldx counted in bf16 elements.  The
 * arguments and the layout of Z are grl_typed_spmm_fwd_slice's; whole graph:
 * self_col0 = 0, ldz = segments*F, zseg = F.  Z stays fp32: every gathered
 * element is widened exactly (bits << 16) and accumulated by the same fmaf
 * chain in CSR order, so Z is bitwise what grl_typed_spmm_fwd[_slice] gives
 * on the widened table, at half the gather bytes and half the table memory.
 * 16 B loads (8 columns a lane) when X is 16 B-aligned, ldx % 8 == 0 and
 * F % 8 == 0 and Z takes float4 stores; one element a lane otherwise.
 * Mixed-precision training keeps node features in bf16; the gradient of
 * this call is grl_typed_spmm_bwd on the fp32 dZ, rounded by the caller.   */
int grl_typed_spmm_fwd_bf16(const GrlTypedCsr* g, const uint16_t* X, int64_t ldx,
                            int32_t F, int64_t self_col0, float* Z,
                            int64_t ldz, int32_t zseg, const GrlDropEdge* de,
                            grl_stream_t stream);

/* grl_typed_spmm_fwd_bf16 writing Z as bf16 bits: ldz and zseg counted in
 * bf16 elements, everything else that entry's (arguments, layout, checks).
 *   Z is BITWISE the round-to-nearest-even bf16 of the fp32 Z that
 *   grl_typed_spmm_fwd_bf16 writes on the same arguments -- the self segment,
 *   every typed segment, and heavy rows after the fixup.
 * The accumulators and a split plan's chunk partials (num_chunks * F floats,
 * as for the fp32 entries) stay fp32; the one rounding is at the store, for a
 * heavy segment in the fixup.  16 B loads and 16 B stores (8 columns a lane)
 * when X and Z are 16 B-aligned and ldx, F, ldz and zseg are multiples of 8;
 * one element a lane otherwise.  A pointer that is not 2 B-aligned is
 * GRL_E_INVALID.  The output of one aggregation is the table of the next
 * (multi-hop propagation) with no cast pass and no fp32 Z in between.       */
int grl_typed_spmm_fwd_bf16_to_bf16(const GrlTypedCsr* g, const uint16_t* X,
                                    int64_t ldx, int32_t F, int64_t self_col0,
                                    uint16_t* Z, int64_t ldz, int32_t zseg,
                                    const GrlDropEdge* de,
                                    grl_stream_t stream);

/* dX = A_drop^T dZ.  Replaces autograd's BmmBackward0 for robust_gcn.py:45
 * (grad of V through the aggregation), with the same DropEdge mask as the
 * forward call that used `de`.  dZ: contiguous [*, (has_self+num_types)*F];
 * dX: device, row stride lddx, num_rows rows, fully overwritten.          */
int grl_typed_spmm_bwd(const GrlTypedCsc* g, const float* dZ, int32_t F,
                       float* dX, int64_t lddx, const GrlDropEdge* de,
                       grl_stream_t stream);

/* dX += A_drop^T dZ over this CSC's edges, continuing every column's sum
 * from the value dX already holds (no self term).  Graphs with >= 2^31 typed
 * edges run as row blocks of < 2^31 edges (int32 positions inside a block,
 * 64-bit global edge ids via edge_id_base): the first block's CSC goes
 * through grl_typed_spmm_bwd, the later ones through this call, in block
 * order -- their CSC positions all follow the earlier blocks', so each
 * column's fmaf chain is the one a single CSC over all edges would run.   */
int grl_typed_spmm_bwd_accum(const GrlTypedCsc* g, const float* dZ, int32_t F,
                             float* dX, int64_t lddx, const GrlDropEdge* de,
                             grl_stream_t stream);

/* Columns [col0, col0 + F) of dX = A_drop^T dZ into dX (row stride lddx,
 * num_rows rows of F floats, fully overwritten), dZ contiguous
 * [*, (has_self+num_types)*F_total].  Per element bitwise equal to
 * grl_typed_spmm_bwd (same edges, same order): the multi-GPU backward
 * (grl.dist.HaloPipeline.backward) gathers one column slice of the halo-row
 * gradients while the previous slice travels back to its owners -- the
 * reverse of the forward halo exchange that replaces the dense
 * BmmBackward0 of robust_gcn.py:45 on a node-range shard.               */
int grl_typed_spmm_bwd_slice(const GrlTypedCsc* g, const float* dZ,
                             int32_t F_total, int32_t col0, int32_t F,
                             float* dX, int64_t lddx, const GrlDropEdge* de,
                             grl_stream_t stream);

/* grl_typed_spmm_bwd_slice over a gradient stored as bf16 bits, writing dX
 * as bf16 bits: F_total and lddx counted in bf16 elements, arguments and
 * checks otherwise that entry's (F_total = F, col0 = 0: the whole gradient).
 *   dX is BITWISE the round-to-nearest-even bf16 of what
 *   grl_typed_spmm_bwd[_slice] writes on the exactly widened dZ with the same
 *   graph, DropEdge record and split plan: the self term first, then the
 *   column's entries in CSC order, one fmaf each, in fp32; rounded once at the
 *   store (a heavy column: in the fixup, after its fp32 chunk partials).
 * The gather moves half the bytes and neither a widened dZ nor an fp32 dX
 * exists.  16 B loads and stores when dZ + col0 and dX are 16 B-aligned and
 * F_total, F and lddx are multiples of 8; one element a lane otherwise.  A
 * pointer that is not 2 B-aligned is GRL_E_INVALID.  There is no accumulating
 * form: a bf16 dX cannot continue a sum without a second rounding.          */
int grl_typed_spmm_bwd_bf16(const GrlTypedCsc* g, const uint16_t* dZ,
                            int32_t F_total, int32_t col0, int32_t F,
                            uint16_t* dX, int64_t lddx, const GrlDropEdge* de,
                            grl_stream_t stream);

/* out = Z W + bias (optionally ReLU), fp32-accurate on the matrix cores.
 * Replaces torch.matmul(new_V, self.h_weights) + self.bias
 * (robust_gcn.py:50) and, with relu = 1, the F.relu around the layer
 * (drop_robust_gcn.py:76).  Z [M, K] row-major (ldz), W [K, C] row-major,
 * bias [C] or NULL, out [M, C] contiguous.
 * Large M (>= 16 GFLOP, K % 16 == 0, 16-B aligned): fp32 values split
 * exactly into three bf16 parts, six partial products on
 * v_mfma_f32_32x32x16_bf16 (error at the fp32-rounding level, DESIGN.md
 * §4.2); W's bf16 planes go to `workspace`.  The path option gemm_x6 = 0
 * (grl_set_option) selects v_mfma_f32_32x32x2_f32 instead.
 * Otherwise, calls of >= 256 output tiles walk all of K in one pass; calls
 * that cannot fill the chip (small graphs: a 74-node page is one 128-row
 * tile) split K into chunks over workgroups -- sized from K and the call's
 * tile count, at most 64 -- as fp32 slabs in `workspace`, added in chunk
 * order (deterministic) with bias/ReLU applied once (slabs over 256 MB in
 * row blocks).  Each form is M-invariant, and grl_linear_fwd_ex's path_rows
 * makes every choice for the whole call's rows.
 * grl_linear_fwd_workspace_size() is 0 when no workspace is needed (it may
 * then be NULL), else the bytes the call requires.                        */
size_t grl_linear_fwd_workspace_size(int64_t M, int32_t K, int32_t C);
int grl_linear_fwd(const float* Z, int64_t ldz, const float* W,
                   const float* bias, float* out, int64_t M, int32_t K,
                   int32_t C, int32_t relu, void* workspace,
                   size_t workspace_bytes, grl_stream_t stream);

/* grl_linear_fwd with the weight's layout and the path's row count explicit:
 * w_layout 0: W [K, C] row-major (GraphConv.h_weights); 1: W [C, K]
 * row-major (nn.Linear.weight: out = Z W^T + bias, the row-local linears of
 * GraphCNNDropEdge -- emb2, NodeSelfAtten's f / g / h, the RanPAC projection,
 * the classifier -- drop_robust_gcn.py:36-58, robust_gcn.py:81-83).
 * path_rows: the row count every arithmetic choice is made for (x6 vs fp32,
 * one pass vs chunk slabs and the chunk size; 0 = M); a node-range shard
 * passes the whole graph's, so its rows are bitwise the one-GPU call's.
 * Workspace: grl_linear_fwd_ex_workspace_size().                           */
size_t grl_linear_fwd_ex_workspace_size(int64_t M, int32_t K, int32_t C,
                                        int64_t path_rows);
int grl_linear_fwd_ex(const float* Z, int64_t ldz, const float* W,
                      int32_t w_layout, const float* bias, float* out,
                      int64_t M, int32_t K, int32_t C, int32_t relu,
                      int64_t path_rows, void* workspace,
                      size_t workspace_bytes, grl_stream_t stream);

/* The GEMM path of grl_linear_fwd_ex(M, K, C, path_rows) under the current
 * path options: 1 = the x6 GEMM, 0 = an fp32-MFMA form.  1 exactly when
 * M >= 1, K % 16 == 0, C >= 4, gemm_x6 is on and, for R = max(M, path_rows)
 * rows, R >= 4 and 2 R C K >= 1.6e10 flops -- the calls for which
 * grl_linear_fwd_ex_workspace_size() is the size of W's planes,
 * 3 * roundup(C, 256) * K * 2 + 256 bytes.  A host layer that cuts a layer
 * into row blocks (grl/dist.py) asks this, with the whole layer's rows as
 * path_rows, to keep every block on the whole call's path.  Host-only, no
 * device work.                                                             */
int32_t grl_linear_fwd_path(int64_t M, int32_t K, int32_t C,
                            int64_t path_rows);

/* grl_linear_fwd_ex over an X stored as bf16: X holds bf16
 * bits [M, K], rows ldx elements apart (a column slice of a wider table is
 * valid); W, w_layout, bias, out and path_rows as in grl_linear_fwd_ex.  A
 * bf16 value is plane 0 of its own three-way split, so X is DMA'd as stored
 * into one LDS plane and each block takes three plane products for six: no
 * widened copy, half the A bytes, half the MFMAs.
 * Contract: out is bitwise grl_linear_fwd_ex on the exactly widened X with
 * the same path_rows and options, for finite inputs (-0 included; NaN and Inf
 * are outside the contract).
 * Eligible -- the query answers grl_linear_fwd_ex_workspace_size(M, K, C,
 * path_rows), the size of W's planes, else 0 -- where grl_linear_fwd_ex would
 * take its x6 GEMM (grl_linear_fwd_path(M, K, C, path_rows) == 1, C % 4 == 0,
 * W 16 B-aligned), X is 16 B-aligned with ldx % 8 == 0, and the path option
 * linear_bf16x is 1.  Anything else: GRL_E_UNSUPPORTED -- there is no second
 * path inside the library; the caller widens X and runs grl_linear_fwd_ex.
 * GRL_E_INVALID, decided on the host: a negative size, ldx < K, a w_layout
 * other than 0 or 1, an odd X address, a NULL X, W or out with M > 0 and
 * C > 0.  GRL_E_WORKSPACE: a NULL, misaligned or short workspace.  M == 0 or
 * C == 0: GRL_OK, nothing is written.  Stream-ordered, no host sync.        */
size_t grl_linear_fwd_bf16x_workspace_query(const uint16_t* X, int64_t ldx,
                                            const float* W, int64_t M,
                                            int32_t K, int32_t C,
                                            int64_t path_rows);
int grl_linear_fwd_bf16x(const uint16_t* X, int64_t ldx, const float* W,
                         int32_t w_layout, const float* bias, float* out,
                         int64_t M, int32_t K, int32_t C, int32_t relu,
                         int64_t path_rows, void* workspace,
                         size_t workspace_bytes, grl_stream_t stream);

/* grl_linear_fwd_ex writing bf16 rows: Z, W, w_layout, bias,
 * relu and path_rows as in grl_linear_fwd_ex; out holds bf16 bits [M, C], rows
 * ldo >= C bf16 elements apart (a column slice of a wider bf16 table is a
 * valid out).  The x6 GEMM's epilogue rounds each fp32 value once to nearest
 * even and stores it: no fp32 [M, C] table and no cast pass (the data
 * gradient of grl_linear_fwd_bf16x's node: g [M, C'] x W [C', K'] -> bf16 dX).
 * Contract: out is bitwise grl_linear_fwd_ex's fp32 output with the same
 * path_rows and options rounded to nearest even, for finite values.
 * Eligible -- the query answers grl_linear_fwd_ex_workspace_size(M, K, C,
 * path_rows), the size of W's planes, else 0 -- where grl_linear_fwd_ex takes
 * its x6 GEMM (grl_linear_fwd_path(M, K, C, path_rows) == 1, C % 4 == 0, Z and
 * W 16 B-aligned, ldz % 4 == 0), out is 4 B-aligned with ldo even, and the path
 * option linear_out_bf16 is 1.  Anything else: GRL_E_UNSUPPORTED -- there is
 * no second path inside the library; the caller runs grl_linear_fwd_ex and
 * casts.  GRL_E_INVALID, decided on the host: a negative size, ldz < K,
 * ldo < C, a w_layout other than 0 or 1, an odd out address, a NULL Z, W or
 * out with M > 0 and C > 0.  GRL_E_WORKSPACE: a NULL, misaligned or short
 * workspace.  M == 0 or C == 0: GRL_OK, nothing is written.  Stream-ordered,
 * no host sync.                                                             */
size_t grl_linear_fwd_to_bf16_workspace_query(const float* Z, int64_t ldz,
                                              const float* W, const uint16_t* out,
                                              int64_t ldo, int64_t M, int32_t K,
                                              int32_t C, int64_t path_rows);
int grl_linear_fwd_to_bf16(const float* Z, int64_t ldz, const float* W,
                           int32_t w_layout, const float* bias, uint16_t* out,
                           int64_t ldo, int64_t M, int32_t K, int32_t C,
                           int32_t relu, int64_t path_rows, void* workspace,
                           size_t workspace_bytes, grl_stream_t stream);

/* One GraphConv layer forward in one call (inference):
 *   out = relu?( (A_drop X) W + bias )       robust_gcn.py:45-51 (+ the F.relu
 * of drop_robust_gcn.py:76), i.e. grl_typed_spmm_fwd then grl_linear_fwd with
 * Z = A_drop X held in `workspace` (W [(has_self+num_types)*F, C] row-major,
 * bias [C] or NULL, out [num_rows, C] contiguous).  With the workspace of
 * grl_graphconv_fwd_workspace_size() Z exists whole (7.2 GB at C3); a smaller
 * workspace makes the call aggregate and multiply rows in chunks that fit
 * (>= 256 rows of Z plus W's bf16 planes), bitwise equal to the whole-graph
 * result -- allowed when the linear takes the x6 path (large graphs) and the
 * graph has no heavy-row split plan, else GRL_E_WORKSPACE.  Replaces the
 * GraphConv.forward pair `torch.matmul(A, V)` / `matmul(new_V, h_weights)`
 * for eval; training keeps Z for dW (grl_linear_bwd_weight).              */
size_t grl_graphconv_fwd_workspace_size(int64_t num_rows, int32_t num_types,
                                        int32_t has_self, int32_t F, int32_t C);
int grl_graphconv_fwd(const GrlTypedCsr* g, const float* X, int64_t ldx,
                      int32_t F, const float* W, const float* bias, int32_t C,
                      int32_t relu, float* out, const GrlDropEdge* de,
                      void* workspace, size_t workspace_bytes,
                      grl_stream_t stream);

/* Workspace grl_graphconv_fwd uses for THIS graph, X and W (0 on bad
 * arguments).  Large graphs without a heavy-row split plan, F in {64, 128,
 * 256}, C <= 256, float4-aligned X rows and W run as ONE kernel
 * (graphconv.hip): Z = A_drop X stays on chip (32-row tiles in LDS as x6
 * bf16 planes, MFMA against W's planes) and the workspace holds only W's
 * planes (2.75 MB at K = 1792, C = 256) -- bitwise the two-kernel result.
 * Otherwise this is grl_graphconv_fwd_workspace_size().
 * graphconv_fused = 0 forces the two-kernel path.                      */
size_t grl_graphconv_fwd_workspace_query(const GrlTypedCsr* g, const float* X,
                                         int64_t ldx, int32_t F,
                                         const float* W, int32_t C);

/* Training forward of one GraphConv layer: out as grl_graphconv_fwd AND
 * Z = A_drop X ([num_rows, (has_self+num_types)*F] contiguous, 16-B aligned),
 * which the backward needs for dW (grl_linear_bwd_weight).  Where the
 * one-kernel path applies, Z is written by the gather waves as they finish
 * rows (its 7.2 GB write at C3 overlaps the MFMAs; the 7.2 GB read-back of
 * the two-kernel path disappears); elsewhere grl_typed_spmm_fwd then
 * grl_linear_fwd.  Bitwise the same out and Z either way.  Workspace:
 * grl_linear_fwd_workspace_size(num_rows, K, C).                         */
int grl_graphconv_fwd_train(const GrlTypedCsr* g, const float* X, int64_t ldx,
                            int32_t F, const float* W, const float* bias,
                            int32_t C, int32_t relu, float* out, float* Z,
                            const GrlDropEdge* de, void* workspace,
                            size_t workspace_bytes, grl_stream_t stream);

/* grl_graphconv_fwd / _fwd_train / _fwd_workspace_query over a feature table
 * stored as bf16 bits (as grl_typed_spmm_fwd_bf16 takes it; ldx counted in
 * bf16 elements).  W, bias, out and Z are fp32; the checks and error codes
 * are the fp32 entries'.  Widening bf16 is exact and every Z element runs the
 * fp32 kernels' fmaf chain, so out and Z are bitwise what the fp32 entries
 * give on the widened table, at half the gather bytes.
 * One kernel (the persistent warp-specialised form only: its gather waves
 * load a lane's 4 columns as 8 B and widen them at the fmaf; ring, MFMA
 * waves and epilogue are the fp32 kernel's) where grl_graphconv_fwd's rule
 * holds with the table's alignment restated: X 8 B-aligned, ldx % 4 == 0,
 * ldx < 2^31.  The workspace query then returns the size of W's planes.
 * Elsewhere grl_typed_spmm_fwd_bf16 into Z, then grl_linear_fwd_ex with
 * g->path_rows: the training entry writes the caller's Z (workspace as
 * grl_graphconv_fwd_train); the inference entry keeps Z whole in the
 * workspace (the query's size; smaller: GRL_E_WORKSPACE -- there is no
 * row-chunked form).  graphconv_fused = 0 and ws_spin apply as to the fp32
 * entries; a bounded wait that runs out poisons out (and Z) and is reported
 * by grl_check() under these entries' own names.  The data gradient is the
 * fp32 layer's (grl_graphconv_bwd_data on the fp32 output gradient), or,
 * for a bf16 output gradient and a bf16 dX, grl_graphconv_bwd_data_bf16.    */
size_t grl_graphconv_fwd_bf16_workspace_query(const GrlTypedCsr* g,
                                              const uint16_t* X, int64_t ldx,
                                              int32_t F, const float* W,
                                              int32_t C);
int grl_graphconv_fwd_bf16(const GrlTypedCsr* g, const uint16_t* X,
                           int64_t ldx, int32_t F, const float* W,
                           const float* bias, int32_t C, int32_t relu,
                           float* out, const GrlDropEdge* de, void* workspace,
                           size_t workspace_bytes, grl_stream_t stream);
int grl_graphconv_fwd_train_bf16(const GrlTypedCsr* g, const uint16_t* X,
                                 int64_t ldx, int32_t F, const float* W,
                                 const float* bias, int32_t C, int32_t relu,
                                 float* out, float* Z, const GrlDropEdge* de,
                                 void* workspace, size_t workspace_bytes,
                                 grl_stream_t stream);

/* The bf16-table entries above writing a bf16 table: out holds bf16 bits,
 * row n at out + n * ldo (ldo >= C, counted in bf16 elements), so a layer
 * can fill a column range of a wider table and the next layer gather from
 * it, with no cast pass and no concatenation in between.
 *   out is BITWISE the round-to-nearest-even bf16 of what the matching _bf16
 *   entry writes (bias, then ReLU, in fp32; rounded once); Z (training
 *   entry) stays fp32 with row stride K and is bitwise that entry's.
 * X and out may be disjoint column ranges of one allocation (gcn2 reads
 * table[:, 0:C] and writes table[:, C:2C]); ranges that overlap are
 * undefined.  Columns of a row outside [0, C) are never written.
 * One kernel (the persistent form; its MFMA waves round the finished tile in
 * registers and store two columns per dword) where the _bf16 entries' rule
 * holds AND out is 4 B-aligned with ldo even; the workspace query then
 * answers the size of W's planes.  Elsewhere grl_typed_spmm_fwd_bf16 into Z,
 * grl_linear_fwd_ex with g->path_rows into an fp32 [num_rows, C] scratch in
 * the workspace, and a rounding pass into out -- the same bits.  The
 * inference entry then needs the query's size (Z whole, the scratch, the
 * linear's workspace); the training entry, whose Z is the caller's, needs
 * roundup(num_rows * C * 4, 256) + grl_linear_fwd_ex_workspace_size(num_rows,
 * K, C, g->path_rows).  A smaller workspace: GRL_E_WORKSPACE.
 * GRL_E_INVALID, decided on the host: the _bf16 entries' checks, NULL out,
 * ldo < C, X or out not 2 B-aligned (the query answers 0 for ldo < C).
 * There is no fp32-table form with a bf16 output: a model's first table is
 * cast once by the caller.  (The data-gradient form with a bf16 output is
 * grl_graphconv_bwd_data_bf16, over a bf16 gradient table.)  A bounded wait that runs
 * out fills out's C columns of every row (and Z) with NaN and is reported by
 * grl_check() under these entries' names.                                  */
size_t grl_graphconv_fwd_bf16_to_bf16_workspace_query(
    const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F,
    const float* W, int32_t C, const uint16_t* out, int64_t ldo);
int grl_graphconv_fwd_bf16_to_bf16(const GrlTypedCsr* g, const uint16_t* X,
                                   int64_t ldx, int32_t F, const float* W,
                                   const float* bias, int32_t C, int32_t relu,
                                   uint16_t* out, int64_t ldo,
                                   const GrlDropEdge* de, void* workspace,
                                   size_t workspace_bytes,
                                   grl_stream_t stream);
int grl_graphconv_fwd_train_bf16_to_bf16(
    const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F,
    const float* W, const float* bias, int32_t C, int32_t relu, uint16_t* out,
    int64_t ldo, float* Z, const GrlDropEdge* de, void* workspace,
    size_t workspace_bytes, grl_stream_t stream);

/* grl_graphconv_fwd_train_bf16_to_bf16 whose Z holds bf16 bits as well: Z
 * [num_rows, K] contiguous, K = (has_self + num_types) * F, half the bytes
 * kept for the weight gradient (grl_linear_bwd_weight_bf16zg reads it as
 * stored).
 *   out is BITWISE grl_graphconv_fwd_train_bf16_to_bf16's;
 *   Z is BITWISE the round-to-nearest-even bf16 of the fp32 Z that entry
 *   writes (the multiply consumes the unrounded rows; only the copy that
 *   goes to memory is rounded, once).
 * One kernel where that entry takes its one kernel AND Z is 8 B-aligned (its
 * gather waves store 8 B of a row at a time; K % 4 == 0 holds whenever the
 * one-kernel shape rule does); the query then answers the size of W's planes.
 * Elsewhere grl_typed_spmm_fwd_bf16 into an fp32 Z scratch at the head of the
 * workspace, grl_linear_fwd_ex with g->path_rows into an fp32 [num_rows, C]
 * scratch behind it, and the rounding pass over each -- the same bits; the
 * query answers that total (roundup(num_rows * K * 4, 256) + roundup(num_rows
 * * C * 4, 256) + grl_linear_fwd_ex_workspace_size(num_rows, K, C,
 * g->path_rows)).  A smaller workspace: GRL_E_WORKSPACE.  graphconv_fused = 0
 * forces that form.
 * GRL_E_INVALID, decided on the host: the sibling entry's checks, plus a NULL
 * or odd Z (the query answers 0 for ldo < C).  num_rows == 0: GRL_OK.  A
 * bounded wait that runs out fills out's C columns of every row AND Z with
 * bf16 NaN and is reported by grl_check() under this entry's name.          */
size_t grl_graphconv_fwd_train_bf16_z16_workspace_query(
    const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F,
    const float* W, int32_t C, const uint16_t* out, int64_t ldo,
    const uint16_t* Z);
int grl_graphconv_fwd_train_bf16_z16(
    const GrlTypedCsr* g, const uint16_t* X, int64_t ldx, int32_t F,
    const float* W, const float* bias, int32_t C, int32_t relu, uint16_t* out,
    int64_t ldo, uint16_t* Z, const GrlDropEdge* de, void* workspace,
    size_t workspace_bytes, grl_stream_t stream);

/* Data gradient of one GraphConv layer in ONE kernel.  Replaces the
 * autograd chain MmBackward0 (dZ = G W^T, robust_gcn.py:50) then
 * BmmBackward0 (dX = A_drop^T dZ, robust_gcn.py:45) by its reassociation
 *   dX = sum_s (A_drop,s^T G) W_s^T     (W_s = rows [s F, (s+1) F) of W),
 * i.e. the one-kernel GraphConv forward run over the typed transpose gt
 * (rows = source nodes, segments (m, t) in forward-CSR order, colidx = the
 * forward row n, vals = the CSC values; entry e's DropEdge id is
 * gt->edge_id_base + eid[e], its forward CSR position, and row m's self id
 * gt->self_id_base + m, so the mask is the forward's).  dZ (7.2 GB at C3)
 * never exists.  G = the output gradient through the ReLU, [num_rows, C]
 * (ldg); W the forward h_weights [(has_self+num_types)*F, C]; dX
 * [num_rows, F] contiguous, overwritten.  Floating point: the same products
 * summed in another order than the two-kernel chain (fp32-level difference,
 * tests/test_gpu_graphconv.py).  G has g_rows rows (the forward rows); gt
 * rows m < g_rows carry the self term w_self(m) G[m] W_0^T, rows beyond
 * (a node-range shard's halo columns) none -- dX of those rows is the
 * partial gradient the halo exchange sends home.  G_agg (NULL, or
 * [gt->num_rows, (has_self+num_types)*C] contiguous) also receives the
 * gathered sums A_drop,s^T G per segment -- with them the weight gradient
 * is dW_s = X^T (A_drop,s^T G), so a layer that kept X instead of Z needs
 * no re-aggregation (grl.ops.graph_conv, recompute mode).  Eligible shapes: a nonzero
 * grl_graphconv_bwd_data_workspace_query(), which is also the workspace
 * size; otherwise GRL_E_UNSUPPORTED and the caller runs the chain.       */
size_t grl_graphconv_bwd_data_workspace_query(const GrlTypedCsr* gt,
                                              const float* G, int64_t ldg,
                                              int32_t C, const float* W,
                                              int32_t F);
int grl_graphconv_bwd_data(const GrlTypedCsr* gt, const int32_t* eid,
                           const float* G, int64_t ldg, int64_t g_rows,
                           int32_t C, const float* W, int32_t F, float* dX,
                           float* G_agg, const GrlDropEdge* de,
                           void* workspace, size_t workspace_bytes,
                           grl_stream_t stream);

/* The shape half of grl_graphconv_bwd_data's eligibility, for a host layer
 * that decides before it builds the typed transpose: 1 when graphconv_fused
 * is on, C is 64, 128, 256, 512 or 1024, 1 <= F <= 512 with F % 4 == 0,
 * 1 <= num_types <= 7, and the [rows, S C] x [S C, F] product (S = has_self +
 * num_types, rows = the transpose's rows) takes the x6 GEMM
 * (grl_linear_fwd_path(rows, S C, F, 0)); else 0.  The workspace query is
 * nonzero exactly when this holds for gt's rows and the call's pointers and
 * plan qualify too: gt->self_row0 == 0, G and W 16-B aligned, ldg % 4 == 0,
 * ldg < 2^30, no heavy-row split plan, nnz < 2^31.  Host-only, no device
 * work.                                                                     */
int32_t grl_graphconv_bwd_data_shape_ok(int64_t rows, int32_t num_types,
                                        int32_t has_self, int32_t C,
                                        int32_t F);

/* grl_graphconv_bwd_data over a gradient table of bf16 bits, writing a bf16
 * dX: the backward of a layer whose output (and so output gradient) is bf16.
 * G holds bf16 bits, row n at G + n * ldg (ldg >= C, counted in bf16
 * elements); dX holds bf16 bits, row m at dX + m * lddx (lddx >= F).  W and
 * G_agg are fp32 as in the fp32 entry; gt, eid, g_rows and de mean what they
 * mean there.
 *   dX is BITWISE the round-to-nearest-even bf16 of what
 *   grl_graphconv_bwd_data writes for the widened G (widening is exact, the
 *   fmaf chains and MFMA products are the same, one rounding in the
 *   epilogue); G_agg is bitwise that entry's.
 * Columns of a dX row outside [0, F) are never written; G and dX may be
 * disjoint column ranges of one allocation (overlapping ranges: undefined).
 * One kernel (the persistent form's data-gradient instance with the bf16
 * table's 8 B gather loads and the bf16 output's packed dword stores), and
 * only that: eligible is a nonzero workspace query, which holds when
 * grl_graphconv_bwd_data_shape_ok does, gt->self_row0 == 0, W is 16 B-aligned,
 * G is 8 B-aligned with ldg % 4 == 0 and ldg < 2^31, dX is 4 B-aligned with
 * lddx % 2 == 0, there is no heavy-row split plan, nnz < 2^31 and the path
 * option graphconv_bwd_bf16 is 1 (0: the query answers 0).  The answer is the
 * size of W's planes plus the status word, the fp32 query's bytes.  Other
 * shapes: GRL_E_UNSUPPORTED -- there is no second path inside the library;
 * the caller widens G and runs grl_graphconv_bwd_data.
 * GRL_E_INVALID, decided on the host: the fp32 entry's checks, a NULL dX,
 * lddx < F, ldg < C, an odd G or dX address, a G_agg that is not 16 B-aligned
 * (the query answers 0 for a NULL dX, lddx < F and ldg < C).  gt->num_rows
 * == 0 and a shard's empty operands are accepted as there.  A missing,
 * unaligned or short workspace: GRL_E_WORKSPACE.  A bounded wait that runs
 * out fills dX's F columns of every row (and G_agg) with NaN and is reported
 * by grl_check() under this entry's name.                                   */
size_t grl_graphconv_bwd_data_bf16_workspace_query(
    const GrlTypedCsr* gt, const uint16_t* G, int64_t ldg, int32_t C,
    const float* W, int32_t F, const uint16_t* dX, int64_t lddx);
int grl_graphconv_bwd_data_bf16(const GrlTypedCsr* gt, const int32_t* eid,
                                const uint16_t* G, int64_t ldg, int64_t g_rows,
                                int32_t C, const float* W, int32_t F,
                                uint16_t* dX, int64_t lddx, float* G_agg,
                                const GrlDropEdge* de, void* workspace,
                                size_t workspace_bytes, grl_stream_t stream);

/* Backward of grl_linear_fwd (autograd MmBackward0 of robust_gcn.py:50, with
 * the ReLU of drop_robust_gcn.py:76 folded in when relu_out != NULL):
 *   dZ = (g * [relu_out > 0]) W^T           grl_linear_bwd_data,  dZ [M, K] (ld lddz)
 *   dW = Z^T (g * [relu_out > 0])           grl_linear_bwd_weight, dW [K, C]
 *   db = sum over rows of (g * [relu_out > 0])                     db [C] (or NULL)
 * g, relu_out: [M, C] contiguous (relu_out = the forward's ReLU output).
 * dW's reduction over M is split over workgroups into fp32 slabs (workspace)
 * added in split order: deterministic, no atomics.  dZ splits its short
 * reduction (C) the same way when M is small (workspace rule as
 * grl_linear_fwd).                                                          */
size_t grl_linear_bwd_data_workspace_size(int64_t M, int32_t K, int32_t C);
int grl_linear_bwd_data(const float* g, const float* relu_out, const float* W,
                        float* dZ, int64_t lddz, int64_t M, int32_t K, int32_t C,
                        void* workspace, size_t workspace_bytes,
                        grl_stream_t stream);
size_t grl_linear_bwd_weight_workspace_size(int64_t M, int32_t K, int32_t C);
int grl_linear_bwd_weight(const float* Z, int64_t ldz, const float* g,
                          const float* relu_out, float* dW, float* db, int64_t M,
                          int32_t K, int32_t C, void* workspace,
                          size_t workspace_bytes, grl_stream_t stream);

/* grl_linear_bwd_weight for a g stored as bf16 (bf16 bits, [M, C], rows
 * ldg >= C elements apart: a column slice of a wider table is a valid g), read
 * as stored -- no widened copy:
 *   dW = Z^T g   [K, C] contiguous        db = sum over rows of g   [C] or NULL
 * Z fp32 [M, K], rows ldz apart.  There is no relu_out: the caller masks first
 * (grl_relu_grad_bf16's g_eff16).  A bf16 value is ONE plane of the split-bf16
 * scheme, so the kernel (gemm_x3t_kernel) issues three plane products per
 * block where grl_linear_bwd_weight's issues six, three of them on planes
 * that are all zeros; the other three run in the same order over the same K16
 * steps, splits and slab order, and db is summed in the same row blocks and
 * order.  dW and db are bitwise grl_linear_bwd_weight(Z, widened g, NULL) for
 * finite g (-0 included; NaN and Inf are outside the contract).
 * Eligible -- the query answers grl_linear_bwd_weight_workspace_size(M, K, C),
 * else 0 -- where grl_linear_bwd_weight would take its split-bf16 kernel
 * (gemm_x6 on, M >= 16, K % 4 == 0, C % 4 == 0, 2 M K C >= 1.6e10), Z is 16 B-
 * aligned with ldz % 4 == 0, g is 8 B-aligned with ldg % 4 == 0, and the path
 * option dw_bf16g is 1.  Anything else: GRL_E_UNSUPPORTED -- there is no
 * second path inside the library; the caller widens g and runs
 * grl_linear_bwd_weight.  GRL_E_INVALID, decided on the host: a negative
 * size, ldz < K, ldg < C, an odd g address, a NULL Z, g or dW with M > 0.  A
 * missing or short workspace: GRL_E_WORKSPACE.  M == 0 writes dW = 0 and
 * db = 0; K == 0 or C == 0 returns GRL_OK.  Stream-ordered, no host sync.  */
size_t grl_linear_bwd_weight_bf16g_workspace_query(const float* Z, int64_t ldz,
                                                   const uint16_t* g, int64_t ldg,
                                                   int64_t M, int32_t K, int32_t C);
int grl_linear_bwd_weight_bf16g(const float* Z, int64_t ldz, const uint16_t* g,
                                int64_t ldg, float* dW, float* db, int64_t M,
                                int32_t K, int32_t C, void* workspace,
                                size_t workspace_bytes, grl_stream_t stream);

/* grl_linear_bwd_weight_bf16g for a Z stored as bf16 too (bf16 bits, [M, K],
 * rows ldz >= K elements apart; grl_graphconv_fwd_train_bf16_z16 writes one):
 *   dW = Z^T g   [K, C] contiguous        db = sum over rows of g   [C] or NULL
 * Both operands are ONE plane of the split-bf16 scheme, so the kernel
 * (gemm_x1t_kernel) issues one plane product per block where the bf16g entry
 * issues three, two of them on planes that are all zeros; it runs over the
 * same K16 steps, splits and slab order, and db is that entry's.  dW and db are
 * bitwise grl_linear_bwd_weight_bf16g(widened Z, g), and so bitwise
 * grl_linear_bwd_weight(widened Z, widened g, NULL), for finite operands (-0
 * included; NaN and Inf are outside the contract).
 * Eligible -- the query answers grl_linear_bwd_weight_workspace_size(M, K, C),
 * else 0 -- where grl_linear_bwd_weight would take its split-bf16 kernel
 * (gemm_x6 on, M >= 16, K % 4 == 0, C % 4 == 0, 2 M K C >= 1.6e10), Z and g
 * are 8 B-aligned with ldz % 4 == 0 and ldg % 4 == 0, and the path option
 * dw_bf16z is 1.  Anything else: GRL_E_UNSUPPORTED -- there is no second path
 * inside the library; the caller widens Z.  GRL_E_INVALID, decided on the
 * host: a negative size, ldz < K, ldg < C, an odd Z or g address, a NULL Z, g
 * or dW with M > 0.  A missing or short workspace: GRL_E_WORKSPACE.  M == 0
 * writes dW = 0 and db = 0; K == 0 or C == 0 returns GRL_OK.  Stream-ordered,
 * no host sync.                                                             */
size_t grl_linear_bwd_weight_bf16zg_workspace_query(const uint16_t* Z, int64_t ldz,
                                                    const uint16_t* g, int64_t ldg,
                                                    int64_t M, int32_t K, int32_t C);
int grl_linear_bwd_weight_bf16zg(const uint16_t* Z, int64_t ldz, const uint16_t* g,
                                 int64_t ldg, float* dW, float* db, int64_t M,
                                 int32_t K, int32_t C, void* workspace,
                                 size_t workspace_bytes, grl_stream_t stream);

/* grl_linear_bwd_weight for a Z stored as bf16 and an fp32 g (DESIGN.md
 * §4.25; the backward of grl_linear_fwd_bf16x's node): Z holds bf16 bits
 * [M, K], rows ldz >= K elements apart (a column slice of a wider table is a
 * valid Z), read as stored -- no widened copy; g fp32 [M, C] contiguous:
 *   dW = Z^T g   [K, C] contiguous        db = sum over rows of g   [C] or NULL
 * A bf16 value is ONE plane of the split-bf16 scheme, so the kernel
 * (gemm_x3ta_kernel) stages Z as one plane and issues three plane products per
 * block where grl_linear_bwd_weight's issues six, three of them on planes that
 * are all zeros; the other three run in the same order over the same K16
 * steps, splits and slab order, and db is that entry's.  dW and db are bitwise
 * grl_linear_bwd_weight(widened Z, g, NULL) for finite operands (-0 included;
 * NaN and Inf are outside the contract).
 * Eligible -- the query answers grl_linear_bwd_weight_workspace_size(M, K, C),
 * else 0 -- where grl_linear_bwd_weight would take its split-bf16 kernel
 * (gemm_x6 on, M >= 16, K % 4 == 0, C % 4 == 0, 2 M K C >= 1.6e10), Z is 8 B-
 * aligned with ldz % 4 == 0, g is 16 B-aligned, and the path option
 * dw_bf16z_f32g is 1.  Anything else: GRL_E_UNSUPPORTED -- there is no second
 * path inside the library; the caller widens Z and runs grl_linear_bwd_weight.
 * GRL_E_INVALID, decided on the host: a negative size, ldz < K, an odd Z
 * address, a NULL Z, g or dW with M > 0.  A missing or short workspace:
 * GRL_E_WORKSPACE.  M == 0 writes dW = 0 and db = 0; K == 0 or C == 0 returns
 * GRL_OK.  Stream-ordered, no host sync.                                    */
size_t grl_linear_bwd_weight_bf16z_workspace_query(const uint16_t* Z, int64_t ldz,
                                                   const float* g, int64_t M,
                                                   int32_t K, int32_t C);
int grl_linear_bwd_weight_bf16z(const uint16_t* Z, int64_t ldz, const float* g,
                                float* dW, float* db, int64_t M, int32_t K,
                                int32_t C, void* workspace,
                                size_t workspace_bytes, grl_stream_t stream);

/* ReLU's derivative applied once (autograd ThresholdBackward of the ReLU at
 * drop_robust_gcn.py:76, the bias gradient of robust_gcn.py:51 with it):
 *   g_eff = g * [relu_out > 0]  (masked entries +0.0; g_eff may alias g)
 *   db    = sum over rows of g_eff                     (db may be NULL)
 * in one pass.  db is summed in the row blocks and order grl_linear_bwd_weight
 * uses for its db, so the two are bitwise equal on the same g_eff.  Used
 * before the large-M backward GEMMs, whose LDS-DMA operand path cannot mask
 * on the way.  g, relu_out, g_eff: [M, C] contiguous.                       */
size_t grl_relu_grad_workspace_size(int64_t M, int32_t C);
int grl_relu_grad(const float* g, const float* relu_out, float* g_eff, float* db,
                  int64_t M, int32_t C, void* workspace, size_t workspace_bytes,
                  grl_stream_t stream);

/* grl_relu_grad for a bf16 output gradient and a bf16 ReLU output (bf16 bits;
 * rows ldg / ldo >= C elements apart), both read once.  Each output may be
 * NULL:
 *   g_eff16 = relu_out > 0 ? g : +0   bf16 bits, rows lde >= C apart; may
 *                                     alias g (grl_graphconv_bwd_data_bf16's G)
 *   g_eff32 = the same, widened       fp32 [M, C] contiguous (the dW GEMM's)
 *   db      = sum over rows of it
 * A selection: nothing is rounded.  db is summed in grl_relu_grad's row blocks
 * and order, so db and g_eff32 are bitwise grl_relu_grad's db and g_eff on the
 * widened operands.  Workspace (db only): grl_relu_grad_workspace_size(M, C).
 * M == 0 writes db = 0, C == 0 returns GRL_OK, as there.                    */
int grl_relu_grad_bf16(const uint16_t* g, int64_t ldg, const uint16_t* relu_out,
                       int64_t ldo, uint16_t* g_eff16, int64_t lde,
                       float* g_eff32, float* db, int64_t M, int32_t C,
                       void* workspace, size_t workspace_bytes,
                       grl_stream_t stream);

/* grl_relu_grad_bf16 with a scale -- the backward of ReLU followed by feature
 * dropout in one pass, when relu_out is the DROPPED output
 * (grl_feature_dropout_bf16 applied in place to the layer's bf16 output):
 *   x = relu_out > 0 ? RNE_bf16(float(g) * scale) : +0
 * with scale the record's 1 / (1 - p).  The dropped output is > 0 exactly
 * where the element was kept and the ReLU was open (a positive bf16 times
 * scale >= 1 never rounds to 0; at p = 1 everything is +0), so the one
 * selection is both masks and no hash is drawn.  g_eff16 = x, g_eff32 = x
 * widened, db = its column sums in grl_relu_grad's row blocks and order; the
 * operands, NULL-able outputs, workspace and empty cases are
 * grl_relu_grad_bf16's.  One rounding, the bf16-output epilogue's.           */
int grl_relu_grad_bf16_scaled(const uint16_t* g, int64_t ldg,
                              const uint16_t* relu_out, int64_t ldo,
                              uint16_t* g_eff16, int64_t lde, float* g_eff32,
                              float* db, int64_t M, int32_t C, float scale,
                              void* workspace, size_t workspace_bytes,
                              grl_stream_t stream);

/* emb1: Linear(K -> C) (+ReLU) over sparse bag-of-characters rows
 * (drop_robust_gcn.py:36,64; rows from TextlineEncoding,
 * textline_encoding.py:23-42):
 *   out[m, :] = relu?(bias + sum_{k: V[m,k] != 0, ascending} V[m,k] Wt[k, :])
 * V [M, K] row stride ldv (dense storage, mostly zeros), Wt [K, C]
 * contiguous (= nn.Linear.weight^T), bias [C] or NULL, out [M, C].  Only the
 * nonzeros cost gathers; C in [1, 512].  Backward: grl_bag_linear_bwd_weight
 * (dWt, db) and grl_linear_bwd_data (dV).                                 */
int grl_bag_linear_fwd(const float* V, int64_t ldv, int64_t M, int32_t K,
                       const float* Wt, int32_t C, const float* bias,
                       int32_t relu, float* out, grl_stream_t stream);

/* emb1's weight gradient (autograd MmBackward0 / AddmmBackward0 of
 * drop_robust_gcn.py:64 through nn.Linear) on the same sparse rows:
 *   dWt[k, :] = sum_{m: V[m,k] != 0, ascending m} V[m,k] g'[m, :],
 *   db = sum_m g'[m, :],   g' = g * [relu_out > 0] (relu_out NULL: g' = g).
 * V [M, K] stride ldv, g / relu_out [M, C] contiguous, dWt [K, C], db [C] or
 * NULL; C in [1, 512].  Only V's nonzeros read a row of g'.  Row ranges are
 * summed in range order (deterministic).  Workspace from the query.       */
size_t grl_bag_linear_bwd_weight_workspace_size(int64_t M, int32_t K, int32_t C);
int grl_bag_linear_bwd_weight(const float* V, int64_t ldv, const float* g,
                              const float* relu_out, float* dWt, float* db,
                              int64_t M, int32_t K, int32_t C, void* workspace,
                              size_t workspace_bytes, grl_stream_t stream);

/* ---------------------------------------------------------------------- */
/* Node self-attention                                                     */
/* ---------------------------------------------------------------------- */
/* NodeSelfAtten (robust_gcn.py:78-99) fused, flash-style (no B x N x N
 * score matrix):  out = gamma * softmax_rows(Q K^T) H + V   per batch,
 * Q = f(V), K = g(V) [B, N, dk], H = h(V), V [B, N, dv], gamma [dv], all
 * contiguous fp32; no 1/sqrt(dk) scale and no mask (every node of the padded
 * batch attends to every node, as the reference does).  dk in [0, 32]
 * (input_dim // 8; 0 = uniform attention, Q/K may then be NULL), dv in
 * [1, 256].  For training pass o_norm [B, N, dv]
 * (= softmax(QK^T) H) and row_max/row_sum [B, N] (the softmax statistics);
 * NULL otherwise.
 * fp32-accurate on the bf16 matrix cores (each fp32 value split exactly into
 * three bf16 parts, six partial products; attn_x6 = 0 selects the
 * fp32-MFMA kernels).  `workspace` (grl_node_attention_workspace_size bytes,
 * or NULL) holds the once-per-call bf16 splits of K and H (backward: also Q
 * and dO); NULL or too small makes every workgroup split its own blocks.   */
size_t grl_node_attention_workspace_size(int64_t B, int64_t N, int32_t dk,
                                         int32_t dv);
int grl_node_attention_fwd(const float* Q, const float* K, const float* H,
                           const float* V, const float* gamma, float* out,
                           float* o_norm, float* row_max, float* row_sum,
                           int64_t B, int64_t N, int32_t dk, int32_t dv,
                           void* workspace, size_t workspace_bytes,
                           grl_stream_t stream);

/* Backward of the attention core.  dO = gamma * d_out [B, N, dv] and
 * D = rowsum(dO * o_norm) [B, N] come from the caller (elementwise); the
 * kernels recompute P from row_max/row_sum and write dQ, dK [B, N, dk] and
 * dH [B, N, dv] (fully overwritten).  Deterministic, no atomics: dK / dH are
 * key-stationary; dQ is query-stationary, or -- with a workspace of
 * grl_node_attention_bwd_workspace_size bytes, dk <= 16 -- folded into the
 * dK kernel as one partial slab per 256-key workgroup (B ceil(N/256) N 64
 * bytes; beyond 24 GiB the fused pass runs in key chunks, each chunk's slabs
 * added onto dQ in order: the same additions) added in workgroup order.  d gamma = sum(d_out * o_norm) and the residual's d_out are the
 * caller's.                                                                  */
size_t grl_node_attention_bwd_workspace_size(int64_t B, int64_t N, int32_t dk,
                                             int32_t dv);
int grl_node_attention_bwd(const float* Q, const float* K, const float* H,
                           const float* dO, const float* row_max,
                           const float* row_sum, const float* D, float* dQ,
                           float* dK, float* dH, int64_t B, int64_t N,
                           int32_t dk, int32_t dv, void* workspace,
                           size_t workspace_bytes, grl_stream_t stream);

/* The same two calls over the query rows [q_begin, q_end) only -- a node-
 * range shard's own queries against EVERY key (NodeSelfAtten on a sharded
 * graph, robust_gcn.py:90-96; grl/dist.py sharded_node_attention).  All
 * arrays keep their [B, N, ...] shapes; rows outside the range of Q / V /
 * dO are read as padding only, and those of out / o_norm / row_max /
 * row_sum / dQ are not written.  fwd: out, o_norm and the stats of the
 * range.  bwd: dQ of the range (complete), and dK, dH of EVERY key as the
 * range's queries' contribution (partials: a shard adds the other shards'
 * in rank order); row_max / row_sum / D must hold the range's rows (the
 * whole softmax's statistics).  The whole range (0, N) is exactly
 * grl_node_attention_fwd / _bwd.  No key split, no folded dQ when ranged. */
int grl_node_attention_fwd_rows(const float* Q, const float* K, const float* H,
                                const float* V, const float* gamma, float* out,
                                float* o_norm, float* row_max, float* row_sum,
                                int64_t B, int64_t N, int32_t dk, int32_t dv,
                                int64_t q_begin, int64_t q_end, void* workspace,
                                size_t workspace_bytes, grl_stream_t stream);
int grl_node_attention_bwd_rows(const float* Q, const float* K, const float* H,
                                const float* dO, const float* row_max,
                                const float* row_sum, const float* D, float* dQ,
                                float* dK, float* dH, int64_t B, int64_t N,
                                int32_t dk, int32_t dv, int64_t q_begin,
                                int64_t q_end, void* workspace,
                                size_t workspace_bytes, grl_stream_t stream);

/* The forward over key / value tables STORED as bf16: K16 [B, N, dk] and
 * H16 [B, N, dv], contiguous bf16 bits.  Q, V, gamma and every output are
 * fp32 and mean what they mean in grl_node_attention_fwd_rows; the whole
 * range (0, N) is the unranged call.  A bf16 value is plane 0 of its three-
 * way split with planes 1 and 2 equal to +0, so the kernel stages the
 * caller's tables as they lie (no split pass, no plane workspace) and runs
 * three plane products per MFMA tile where the fp32 entry runs six.
 *   _path (host only): 1 exactly when the tables can be staged as they lie:
 * dk in {16, 32}, dv in {32, 64, 128, 256} and the path option attn_x6 is
 * 1; else 0.
 *   The call: GRL_E_UNSUPPORTED where _path is 0 or K16 / H16 is not 16 B-
 * aligned -- there is no second path inside the library; the caller widens
 * the tables and calls grl_node_attention_fwd_rows.  Empty cases (B == 0,
 * N == 0, q_begin == q_end: GRL_OK) and argument checks (NULLs, row_max /
 * row_sum both or none, the range inside [0, N]: GRL_E_INVALID, decided on
 * the host) are those of the fp32 entry.  No host sync.
 *   `workspace` (_workspace_size bytes, or NULL) holds only the key split's
 * partials: the split is the fp32 entry's (a function of B and N alone);
 * NULL or too small runs unsplit.  The pipelined kernel runs at every N.
 * attn_fwd8 = 0 selects 4-wave workgroups, as for fp32; attn_pipe is
 * ignored (no unpipelined bf16 form exists).
 *   Contract, for finite inputs: row_max and row_sum are BITWISE those of
 * grl_node_attention_fwd_rows on the widened K16 and H16 under the default
 * options (attn_x6 = 1).  out and o_norm are EQUAL AS VALUES: bitwise,
 * except that a zero may differ in sign -- an output accumulator rescaled
 * between key blocks can underflow to -0, which the fp32 kernel's zero-plane
 * products turn into +0 and which stays -0 when they are skipped.  Not
 * bitwise against the fp32-MFMA kernels (attn_x6 = 0).                    */
int32_t grl_node_attention_fwd_bf16kv_path(int64_t B, int64_t N, int32_t dk,
                                           int32_t dv);
size_t grl_node_attention_fwd_bf16kv_workspace_size(int64_t B, int64_t N,
                                                    int32_t dk, int32_t dv);
int grl_node_attention_fwd_bf16kv_rows(const float* Q, const uint16_t* K16,
                                       const uint16_t* H16, const float* V,
                                       const float* gamma, float* out,
                                       float* o_norm, float* row_max,
                                       float* row_sum, int64_t B, int64_t N,
                                       int32_t dk, int32_t dv, int64_t q_begin,
                                       int64_t q_end, void* workspace,
                                       size_t workspace_bytes,
                                       grl_stream_t stream);

/* ---------------------------------------------------------------------- */
/* Graph formats                                                           */
/* ---------------------------------------------------------------------- */

/* Dense adjacency -> typed CSR, block-diagonal over the batch.
 * Replaces GraphConv.preprocess_adj (robust_gcn.py:53-72): instead of the
 * dense (B, (L+1)N, N) A_pre, emit the nonzeros of A[b, n, t, m] addressed by
 * element strides {sb, sn, st, sm} (the collate layout (B,N,L,N) has
 * sm = 1; the permuted view GraphConv.forward receives, (B,N,N,L), is the
 * same storage).  Global node id = b*N + n; global row = (b*N + n)*L + t.
 * Two phases because nnz is data-dependent:
 *   1) grl_dense_to_csr_rowptr writes rowptr[B*N*L + 1] (the caller reads
 *      rowptr[B*N*L] to size colidx/vals);
 *   2) grl_dense_to_csr_fill writes colidx (global source node b*N + m) and
 *      vals (the A value; NULL to skip) in ascending m within each row.   */
size_t grl_dense_to_csr_workspace_size(int64_t num_segments);
int grl_dense_to_csr_rowptr(const float* A, int64_t B, int64_t N, int32_t L,
                            const int64_t strides[4], int32_t* rowptr,
                            void* workspace, size_t workspace_bytes,
                            grl_stream_t stream);
int grl_dense_to_csr_fill(const float* A, int64_t B, int64_t N, int32_t L,
                          const int64_t strides[4], const int32_t* rowptr,
                          int32_t* colidx, float* vals, grl_stream_t stream);

/* Heavy-row plan over a segment pointer array ptr[rows*nseg + 1] (rowptr
 * with nseg = L for the forward CSR, colptr with nseg = 1 for the CSC).
 *   grl_split_plan_count -> counts[0] = heavy segments, counts[1] = chunks
 *                           (device int64[2]; the caller reads them to size
 *                           the plan arrays)
 *   grl_split_plan_build -> fills plan->heavy_seg/heavy_cptr/chunk_begin/
 *                           chunk_end (caller-allocated, sizes from count)
 * Deterministic: segments and chunks are emitted in row, segment, edge order. */
size_t grl_split_plan_workspace_size(int64_t rows);
int grl_split_plan_count(const int32_t* ptr, int64_t rows, int32_t nseg, int32_t threshold,
                         int32_t chunk_edges, int64_t* counts, void* workspace,
                         size_t workspace_bytes, grl_stream_t stream);
int grl_split_plan_build(const int32_t* ptr, int64_t rows, int32_t nseg, GrlSplitPlan* plan,
                         void* workspace, size_t workspace_bytes, grl_stream_t stream);

/* Typed CSR -> CSC over source rows [0, num_cols) for the backward pass.
 * Stable: within a column, entries keep CSR (edge id) order, so dX sums are
 * deterministic.  colptr [num_cols+1], zrow/eid [nnz], vals_out [nnz] (only
 * written when g->vals != NULL).                                          */
size_t grl_csr_to_csc_workspace_size(int64_t nnz, int64_t num_cols);
int grl_csr_to_csc(const GrlTypedCsr* g, int64_t num_cols, int32_t* colptr,
                   int32_t* zrow, int32_t* eid, float* vals_out,
                   void* workspace, size_t workspace_bytes,
                   grl_stream_t stream);

/* Heuristic spatial graph of one document (host-only, no device work).
 * Replaces Graph(...) and Graph._get_adj_matrix
 * (gnn/data_generator/data_process/utils/graph_utils.py:425-834) as called by
 * HeuristicGraphBuilder.process (heuristic_graph_builder.py:56-83).
 * Items are the sample's text lines in label-index order with their axis-
 * aligned boxes (min/max of the polygon); kind 0 = text line, 1 = "cell",
 * 2 = "table" (dropped, as in the reference).  Edge types are
 * lr, rl, tb, bt, child, parent (graph_utils.py:434).
 *   grl_layout_graph_size  -> *out_n = min(#items, #graph nodes), the side of
 *                             the adjacency the reference keeps
 *   grl_layout_graph_dense -> (out_n, 6, out_n) adjacency as IEEE fp16 bits
 *                             (the reference's float16 array); edge_type
 *                             0 = normal_binary, 1 = fc_similarity, 2 = fc_binary
 *   grl_layout_graph_edges -> the normal_binary edges as sorted unique
 *                             (src, type, dst) int32 triples: typed CSR input
 *                             without the dense O(N^2) matrix.  *count is the
 *                             number of edges; nothing is written if it
 *                             exceeds `capacity` (call again with room).   */
typedef struct GrlLayoutItem {
  double x1, y1, x2, y2; /* box: min/max of the polygon's x and y            */
  int32_t kind;          /* 0 text line, 1 cell, 2 table                      */
  int32_t has_text;      /* str(text) != ""                                  */
} GrlLayoutItem;
int grl_layout_graph_size(const GrlLayoutItem* items, int32_t n, int32_t* out_n);
int grl_layout_graph_dense(const GrlLayoutItem* items, int32_t n, int32_t edge_type,
                           int32_t out_n, uint16_t* adj_half);
int grl_layout_graph_edges(const GrlLayoutItem* items, int32_t n, int32_t out_n,
                           int32_t* edges, int64_t capacity, int64_t* count);

/* Synthetic graphs for the benchmark configs.
 * Candidate edge k in [0, num_candidates) is (src, type, dst) drawn from a
 * counter-based hash of (seed, k): Erdos-Renyi (kind 0: src, dst uniform in
 * [0, N)) or R-MAT (kind 1: a,b,c,d = 0.57,0.19,0.19,0.05, N = 2^scale);
 * type uniform in [0, L).  Node-range shard [row_begin, row_end) keeps the
 * candidates whose src falls in it, dedupes (src, type, dst) and emits typed
 * CSR rows for those nodes (global colidx).  Three phases:
 *   grl_synth_count   -> *count (device int64) = candidates in the shard
 *   grl_synth_build   -> rowptr [(row_end-row_begin)*L + 1], colidx, and
 *                        *nnz (device int64) after dedupe
 * Workspace from grl_synth_workspace_size(count).                         */
typedef struct GrlSynthSpec {
  int32_t kind;           /* 0 = Erdos-Renyi, 1 = R-MAT                     */
  int32_t num_types;      /* L                                              */
  int64_t num_nodes;      /* N                                              */
  int64_t num_candidates; /* N * avg_deg before dedupe                      */
  uint64_t seed;
  int64_t row_begin, row_end;
} GrlSynthSpec;
int grl_synth_count(const GrlSynthSpec* spec, int64_t* count /* device */,
                    grl_stream_t stream);
size_t grl_synth_workspace_size(const GrlSynthSpec* spec, int64_t count);
/* deg[v - row_begin] += candidates with src v, for v in [row_begin, row_end)
 * (before dedupe; deg must be zeroed by the caller).  Used to choose
 * edge-balanced node-range shard boundaries for power-law graphs. */
int grl_synth_degrees(const GrlSynthSpec* spec, int32_t* deg, grl_stream_t stream);
int grl_synth_build(const GrlSynthSpec* spec, int64_t count, int32_t* rowptr,
                    int32_t* colidx, int64_t* nnz /* device */,
                    void* workspace, size_t workspace_bytes,
                    grl_stream_t stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GRL_H_ */
