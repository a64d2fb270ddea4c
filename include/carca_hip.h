/* carca_hip.h -- C ABI of libcarca_hip.so: the MI355X (gfx950) CARCA hot path.
 *
 * The reference (r-papso/carca-replication) is pure PyTorch and has no FFI of its own; its
 * plug-in boundary is the nn.Module ABCs of src/abstract.py:8-50.  This library sits UNDER
 * those modules: each entry point replaces the ATen op sequence of one reference method, named
 * below with file:line.  The Python host layer (carca_replication_amd/modules.py) keeps the
 * reference's class names, constructors, state_dict keys and forward() semantics and binds
 * these symbols with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 (ids: int32) unless it says "host";
 *  - tensors are row-major; `ld*` is a row stride in elements; activation strides must be
 *    multiples of 4 elements and bases 16-byte aligned (torch allocations are);
 *  - `stream` is a hipStream_t passed as void*; launches are asynchronous on it and the host never
 *    waits for the device; callers own every tensor, nothing of theirs is retained after the call
 *    returns (graph-capturable).  What a launch needs beyond its arguments (partial tiles of a split
 *    product, row tables) is the library's own: one lazily grown scratch buffer per stream, reused
 *    in stream order, or memory owned by the capture (carca_capture_scope below);
 *  - return 0 on success, a negative CARCA_ERR_* for a rejected call (message from
 *    carca_last_error()), a positive hipError_t for a failed launch.  Never aborts.
 */
#ifndef CARCA_HIP_H
#define CARCA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CARCA_ABI_VERSION 3
#define CARCA_OK 0
#define CARCA_ERR_UNSUPPORTED (-1) /* shape outside what the kernels were built for */
#define CARCA_ERR_BADARG (-2)      /* null pointer, misaligned stride, ... */

#define CARCA_MAX_SEGS 4   /* profile + up to 3 target groups per embed call */
#define CARCA_MAX_GROUPS 3 /* target groups per scoring call (train: pos, neg) */
#define CARCA_MAX_L 64     /* profile slots one workgroup keeps in LDS */
#define CARCA_MAX_PROFILE_L 1024 /* profile slots of carca_recommend / carca_rank_items (staged CARCA_MAX_L at a time) */
#define CARCA_EMBED_GATHER 1
#define CARCA_EMBED_FEAT 2
#define CARCA_EMBED_JOINT 4
#define CARCA_EMBED_ALL 7
/* with CARCA_EMBED_FEAT, evaluation only: the feature product over one representative per group of equal attribute rows
 * (rows of equal id whose attribute bytes are equal; tuning key 20) */
#define CARCA_EMBED_DEDUP 8

int carca_abi_version(void);
/* Kernel-variant knobs for tuning runs and A/B tests (tools/, tests/); 0 = the shipped choice everywhere.
 *   key 0  row / weight-gradient GEMM and the item-row gather, ONE switch at a time (csrc/carca_common.h names them CARCA_GV_*);
 *          any non-zero value also moves the narrow row products off their default kernel:
 *            1 rows: force 128x96 tiles
 *            2 rows: force the one-block-per-CU kernels; AND weight gradient: force the persistent kernel
 *            3 = 2 + in-kernel stamps (both)
 *            4 rows and tiled weight gradient: no buffer loads; weight gradient: never the persistent kernel
 *            5 tiled weight gradient only          6 never group weight gradients / row GEMMs
 *            7 rows: force the one-block-per-CU kernel with 384 x 128 tiles where the tiled kernel would run
 *            8 never let the item-row gather ride in the feature GEMM's launch
 *            9 / 10 narrow rows: 64 x 96 tiles with prefetch depth 4 / 2
 *            11 / 12 narrow rows: the 80 x 96 kernel wherever it applies / never
 *            13 persistent weight gradient: equal item counts     14 ... atomic flush instead of partial-tile slots
 *            15 the one-tile-per-workgroup feature GEMM (no hand-over of partial tiles)
 *            16 persistent weight gradient: consecutive workgroups instead of per-XCD groups
 *            18 the gather's own launch: one row per wave
 *            19 the gather keeps its own launch beside the stream-K kernels; AND tiled weight gradient: row splits
 *            combine by atomics instead of partial tiles
 *            21 split-precision kernel without LDS-DMA        22 persistent weight gradient over every row
 *            23 feature GEMM over every row (gemm_rows_sk_kernel instead of gemm_rows_skc_kernel, which leaves rows
 *            with id 0 out)
 *            24 / 25 short-K streaming kernel (gemm_rows_cus_kernel): never / wherever it is correct
 *            26 / 27 persistent narrow-output kernel (gemm_rows_n96s_kernel): never / wherever it is correct
 *            158 = 15 + 8 (the key holds one value)
 *   key 1  attention kernels: 1 one workgroup per user, 2 always two, 3 one 8-wave workgroup per user (the variant
 *          for batches of more users than CUs, two workgroups resident per CU)
 *   key 2  weight gradient: row-split slot target      key 4  weight gradient: minimum 32-row chunks per split
 *   key 3  weight gradient: plain stores instead of atomics (timing diagnostic, wrong results)
 *   key 5  grouped weight gradient: row-split slot target per product; AND gemm_rows_n96s_kernel's timing experiments
 *          (bit mask; WRONG results)
 *   key 6  1: the round-1 paths (materialised V in the scoring kernel, per-op SelfAttentionBlock backward)
 *   key 7  scoring kernel layout (1 one workgroup per user, 2 fold kernel, 3 persistent stream kernel)
 *   key 8  DETERMINISTIC MODE (1 = on): no fp32 atomics anywhere in the backward pass -- every accumulation into the
 *          pass's gradient buffer (weight gradients, LayerNorm gamma / beta, bias sums, the embedding scatter-add) goes
 *          into a 64-bit fixed-point shadow buffer (carca_det_begin / carca_det_flush below), whose integer sums do not
 *          depend on the order in which workgroups arrive; HR / NDCG sums are added in a fixed order by one block.
 *          Same inputs => same bits, run to run.  Reference: none (torch's CUDA backward has the same nondeterminism:
 *          index_add / atomicAdd in embedding_dense_backward); it exists so that trajectory tests can be tight.
 *   key 9  in-kernel phase stamps of the row-chain kernels (1 FFN side, 2 input side; carca_set_debug_buffer)
 *   key 10 CU budget of the one-workgroup-per-CU weight-gradient kernel (0 = every CU): a caller that runs two halves
 *          of a backward pass on two streams gives each launch half the chip (autograd.py: the target rows' embedding
 *          backward beside the profile rows' encoder backward)
 *   key 11 feature GEMM with the stream-K hand-over: K steps the cheap workgroup takes over per tile (0 = cost model)
 *   key 12 ... log2 of the bound on a taker's wait for its partial tile, in ~0.4 us sleeps (0 = 23, about 5 s); on expiry
 *          the launch's output is wrong, the library's error word is set and carca_poll_errors / the next such launch fail
 *   key 13 ... TEST ONLY: 1 + index of the one partial tile whose giver withholds its flag (exercises key 12's expiry)
 *   key 14 persistent scoring kernel: 1 = ticket dealing of a step's first jobs (A/B)
 *   key 15 timing diagnostics of the 80 x 96 row GEMM, the scoring kernels, the split-precision kernels and the prologue of
 *          gemm_rows_skc_kernel (bit masks; WRONG results)
 *   key 16 PRECISION OF THE FEATURE GEMM (AllEmbedding.feats_embed, carca.py:86), opt-in: 0 = exact-fp32 MFMA (default,
 *          the path every parity figure is quoted on); 1 = operands split into three bf16 parts, six bf16-MFMA products,
 *          fp32 accumulation (fp32-class accuracy on the 16x faster pipe); 2 = two fp16 parts (the second scaled by
 *          2^11), three products, two fp32 accumulators -- |operands| < 65504 required.  Only where the one-workgroup-per-CU
 *          kernel would run; anything else keeps the fp32 kernels.  + 16: wherever the kernel's own conditions hold
 *          (K0 % 4 == 0, K1 <= 8, plain epilogue), whatever the grid -- for parity tests at fixture sizes.
 *   key 17 / 18  gemm_rows_skc_kernel: 1 + the K steps that owning a row block costs a team / a lone workgroup (0 = built in)
 *   key 19 gemm_rows_skc_kernel: K steps of k-source 0 below which the product stays off it (0 = 64)
 *   key 20 feature product of an evaluation forward (carca_forward without a backward's saves): 0 = over one representative
 *          row per group of equal attribute rows (CARCA_EMBED_DEDUP), 1 = over every kept row (A/B, tests)
 *   key 21 1 = the per-item cache of that product (carca_feat_cache_arm) is never used (A/B, tests)
 *   key 22 1 = under that cache every row compares its bytes with its entry itself; 0 = one row of up to four of an item
 *          compares for all of them with one read of the entry (the same results; A/B, tests).  Does not switch the cache off
 *   key 23 eval SelfAttentionBlock with two workgroups per user and pads_uniform: 0 = the idle second workgroups of one-tile
 *          users take query tiles of four-tile users, 1 = never (the same bits; A/B, tests)
 *   key 24 deep top-k (carca_retrieve / carca_retrieve_among / carca_knn_retrieve): parts S a user's logit row is split
 *          into for the selection.  0 = the shipped choice; v > 0 forces S = v, clamped to [1, 64] and
 *          to the row length, and lowered like the shipped choice where the key scratch would pass 1 GiB (the same bits for
 *          every S; A/B, tests).  carca_recommend_sampled / carca_knn_recommend_sampled run that selection, and a forced
 *          value also forces the parts of their perturb pass (clamped to [1, 1024] and to a chunk per wave): the same bits */
int carca_set_tuning(int key, int value);
/* Deterministic mode, per backward pass: register the pass's flat fp32 gradient buffer `flat` (n floats) and its shadow
 * (n uint64, ZERO on entry); kernels launched on `stream` afterwards accumulate gradients that land inside `flat` into
 * the shadow.  carca_det_flush(lo, hi) adds shadow[lo:hi] / 2^36 into flat[lo:hi] and clears it -- before anything
 * READS an accumulated range and at the end of the pass.  carca_det_begin(NULL, 0, NULL) ends the pass. */
int carca_det_begin(float* flat, long long n, unsigned long long* shadow, void* stream);
int carca_det_flush(float* flat, unsigned long long* shadow, long long lo, long long hi, void* stream);
/* Diagnostic runs only: device buffer (>= 16 x #workgroups uint64) that the attention kernels fill with
 * s_memtime stamps at their phase boundaries; NULL (default) disables stamping. */
int carca_set_debug_buffer(void* device_ptr);
const char* carca_last_error(void); /* host string, thread-local, valid until the next call */
/* Failures of a kernel that no launch status can carry (today: key 12's expiry).  CARCA_OK, or a negative code with the
 * message set; the condition is cleared by the call that reports it.  Costs one read of host memory: call it wherever the
 * host has synchronised anyway (end of an evaluation epoch, after a graph replay's loss was read). */
int carca_poll_errors(void);
/* Memory the library allocates for kernels that are CAPTURED into a hipGraph (partial-tile buffers, row tables, descriptor
 * copies -- what an eager launch takes from a per-stream scratch buffer) belongs to the capture in progress:
 * carca_capture_scope returns that capture's id while `stream` is capturing (0 otherwise), carca_capture_bytes what has
 * been allocated under it, and carca_capture_release frees it -- call it once the graph built from the capture is gone. */
int carca_capture_scope(void* stream, unsigned long long* id_out);
long long carca_capture_bytes(unsigned long long id);
int carca_capture_release(unsigned long long id);
/* Outside a capture the same memory is one buffer per (device, stream, purpose), kept for the life of the process and keyed
 * by the raw stream handle: a caller that DESTROYS a stream it launched on hands the stream's buffers back with this call
 * (after synchronising the stream, on the device the launches ran on; refused while the stream is being captured). */
int carca_release_stream_scratch(void* stream);

/* ------------------------------------------------------------------------------------------
 * Padded geometry shared by every entry point.  For model width d and H heads (dh = d/H):
 *   DPI = 64 / 96 / 128 (smallest >= d) padded input-feature count (k of the projections)
 *   DHP = round_up(dh, 16)           padded per-head width
 *   DPO = H * DHP                    head-padded output-feature count
 * Activations travel between kernels as [rows, DPI] with zeroed pad columns.
 * ---------------------------------------------------------------------------------------- */
int carca_padded_dims(int d, int H, int* dpi, int* dhp, int* dpo);
/* 1 if the fused per-user attention kernels (self-attention block, cross-attention scoring and their backward) are built
 * for the (DPI, DHP, H) that (d, H) pads to, else 0; never an error (0 for d > 128 or d % H != 0).  Models whose
 * geometry is not built run the composed row-level path instead (long_profile.py). */
int carca_attn_geometry_built(int d, int H);

/* ---- weight packing -----------------------------------------------------------------------
 * Copies parameter matrices (state_dict layout) into the zero-padded, 16-byte-aligned,
 * optionally head-permuted layout the attention kernels read MFMA fragments from.
 * dst[rp][cp] = src[r][c] where rp (cp) is r (c) itself, or its head-padded position when
 * row_dh (col_dh) > 0; every dst element is written (pads = 0).  descs is a HOST array. */
typedef struct CarcaPackDesc {
  const float* src; /* [rows, cols], row stride src_ld */
  float* dst;       /* [dst_rows, dst_cols] dense */
  int32_t rows, cols, src_ld;
  int32_t dst_rows, dst_cols;
  int32_t row_dh, row_dhp; /* 0,0 = plain rows */
  int32_t col_dh, col_dhp; /* 0,0 = plain cols */
  int32_t transposed;      /* 1: logical element (r, c) lives at src[c * src_ld + r] (rows/cols are logical) */
  int32_t frag16;          /* 1: dst is written in MFMA-fragment order instead of row-major (dst_rows, dst_cols multiples
                            * of 16): packed element (rp, cp) lives at
                            *   (((rp/16) * (dst_cols/16) + cp/16) * 64 + ((cp%16)/4) * 16 + rp%16) * 4 + cp%4,
                            * i.e. the 64 lanes x 4 floats one wave loads for one 16x16 tile are 1 KB contiguous */
  /* fold_vec != NULL: the logical source is not src itself but the per-head contraction of its ROWS with a vector,
   *   S'[h][c] = sum_{i < rows/fold_H} fold_vec[h*(rows/fold_H) + i] * src[h*(rows/fold_H) + i][c],  h < fold_H,
   * a [fold_H, cols] matrix that is then placed like any other (row_dh must be 0).  This is how decoder.ffn is folded
   * into the cross-attention's value projection once per weight version (CarcaCaWeights.wu / cu). */
  const float* fold_vec;
  int32_t fold_H;
} CarcaPackDesc;
int carca_pack_weights(const CarcaPackDesc* descs, int n, void* stream);

/* ---- building block: row GEMM  C[m][n] = sum_k A[m][k] * Bt[n][k]  (+ epilogue) ------------------
 * The tiled fp32-MFMA kernel behind AllEmbedding's two Linear layers (carca.py:86,89) and every
 * dense input-gradient product of the backward pass.  Rows come from up to CARCA_MAX_SEGS segments
 * (one launch for profile + target groups); k runs over up to two column sources (a0 | a1), each
 * with its own Bt, so torch.cat((a, c), -1) @ W^T never materialises the concatenation.
 * Epilogue, in this order, each part optional:
 *   v = alpha * acc + bias[n] + pos[(row % T)][n] + add[row][n] + add_table[ids[row]][n] + rowscale[row] * colvec[n]
 *   v *= gate_scale * (gate[row][n] > 0 ? 1 : gate_slope) (LeakyReLU' (x dropout1'), from the saved activation)
 *   v  = ids[row] != 0 ? v : 0                          (when mask_rows)
 *   C[row][n] = v for n < N;  C[row][n] = 0 for N <= n < ncols_out                              */
typedef struct CarcaGemmSeg {
  const float* a0;       /* [rows, lda0] */
  const float* a1;       /* [rows, lda1] or NULL when K1 == 0 */
  float* c;              /* [rows, ldc] */
  const int32_t* ids;    /* [rows] or NULL (needed by mask_rows / add_pos) */
  const float* add;      /* [rows, ld_add] or NULL */
  const float* gate;     /* [rows, ld_gate] or NULL */
  const float* rowscale; /* [rows] or NULL */
  int32_t rows, T, add_pos;
  /* Rows of a0 / a1 may belong to a [B, T, K] VIEW whose users are a0_bstride / a1_bstride elements apart
   * (e.g. o_a[:, :L] of train.py:86-88): row r then starts at (r / T) * bstride + (r % T) * lda.  0 = dense. */
  int64_t a0_bstride, a1_bstride;
  /* >= 1: a0 is a TABLE [n_items, lda0] and row r reads a0[ids[r]] (attribute rows gathered by item id inside the
   * GEMM's operand load -- no dense [B, T, n_attrs] tensor exists; data.py:119-132 always sets p_a = attrs[p_x]).
   * A value > 1 also states the table's row count, which lets the launcher pick the 32-bit-offset load path. */
  int32_t a0_gather;
} CarcaGemmSeg;
typedef struct CarcaGemmDesc {
  CarcaGemmSeg seg[CARCA_MAX_SEGS];
  int32_t nseg;
  int32_t lda0, lda1, K0, K1;
  const float* bt0; /* [N, ldb0] */
  const float* bt1; /* [N, ldb1] or NULL */
  int32_t ldb0, ldb1;
  int32_t N, ldc, ncols_out;
  const float* bias;   /* [N] or NULL */
  const float* pos;    /* [T, N] or NULL */
  const float* colvec; /* [N] or NULL */
  int32_t ld_add, ld_gate;
  float gate_slope;
  int32_t mask_rows;
  float alpha;             /* v = alpha * acc + bias + ...; 0 means 1 */
  float gate_scale;        /* extra factor on the gate (1/(1-p) when the saved activation went through dropout); 0 = 1 */
  int32_t gate_zero_drops; /* 1: an exactly-zero saved activation was DROPPED -> gradient 0 (else LeakyReLU'(0) = slope) */
  /* An addend GATHERED by id: v += add_table[ids[row]][n] (every segment needs ids).  How the joint embedding takes the
   * item rows without a gather launch and without their K columns: e = q W_jq^T + (sqrt(d) E W_jz^T)[id] + b_j
   * (carca.py:87-89), the bracket prepared once per weight version (CarcaForwardDesc.z_table). */
  const float* add_table;  /* [n_rows_of_the_table, ld_add_table] or NULL */
  int32_t ld_add_table;
} CarcaGemmDesc;
int carca_gemm_rows(const CarcaGemmDesc* desc /*host*/, void* stream);
/* Kernels behind it and what they assume of the GPU (the launcher picks by shape; carca_gemm_rows_log names the choice):
 *  - gemm_rows_sk_kernel / gemm_rows_skc_kernel (K0 >= 2048 with a grid of about one 384 x 96 tile per CU: the feature
 *    product at C2 / C3 / C4) are PERSISTENT grids of one workgroup per CU in which a workgroup may WAIT for a partial tile
 *    that another workgroup of the same launch writes (stream-K hand-over).  Every workgroup of the launch must become
 *    resident: give such a launch the whole device -- ONE stream of this library per device at a time, no CU mask smaller
 *    than the grid, no long-running kernel of another stream holding CUs.  The wait is bounded (tuning key 12, ~5 s): a
 *    taker that gives up writes the library's error word, and carca_poll_errors / the next such launch fail loudly instead
 *    of the GPU hanging; the results of that launch are wrong.  The captured train step's second stream runs its kernels
 *    under a CU budget (tuning key 10) and never one of these two beside another.
 *  - gemm_rows_cus_kernel (short K, >= 1.75 tiles per CU: the feature product at C5) and gemm_rows_n96s_kernel (narrow
 *    output over >= 2.5 blocks of 160 rows per CU: the joint embedding at C5) are persistent too, but no workgroup ever
 *    waits for another: they are correct under any scheduling, beside any other stream.
 *  - every other kernel is an ordinary grid of independent tiles. */
/* Opt-in split-precision path of the product above (tuning key 16; csrc/gemm_split.hip): the weight matrix as packed
 * 16-bit planes, prepared once per weight version.  It takes products with K0 % 4 == 0 (k-source 0 in 32-wide K steps;
 * k-source 1, at most 8 columns, is added as exact fp32 multiply-adds) and the plain epilogue, on 384 x 96 tiles.
 * carca_split_bytes gives the size of the packed copy of the [N, K0] block of k-source 0 (mode 1 = bf16 x 3, 2 = fp16 x 2),
 * carca_split_pack writes it (w = bt0, row stride ldw), and carca_split_bind tells this THREAD's following launches that
 * `planes` is the packed copy of the matrix at `w`: a launch whose bt0, mode and shape match uses it, any other launch
 * under key 16 splits its weights itself, into scratch, every time (correct, ~8 us at C2).  carca_split_bind(NULL, NULL,
 * 0, 0, 0) unbinds.  The caller keeps `planes` alive and re-packs when the weights change. */
long long carca_split_bytes(int N, int K0, int mode);
int carca_split_pack(const float* w, int ldw, int K0, int N, int mode, void* out, void* stream);
int carca_split_bind(const float* w, const void* planes, int mode, int N, int K0);
long long carca_split_launch_count(void); /* launches of the split-precision kernel by this process so far */
/* n INDEPENDENT products (host array): the narrow ones (d-wide input gradients of the backward pass) share launches,
 * so that two ~150-block products cost one launch instead of two back to back; same results as n single calls. */
int carca_gemm_rows_group(const CarcaGemmDesc* descs /*host*/, int n, void* stream);

/* ---- building block: weight-gradient GEMM  dW[n][k] += sum_r dY[r][n] * X[r][k] -------------------
 * The contraction runs over ROWS (users x slots), split across workgroups; partial tiles are
 * combined with fp32 atomic adds into dW (caller zeroes dW / db first; summation order, hence the
 * last bits, varies run to run).  db[n] += sum_r dY[r][n] when db != NULL.  Rows whose ids == 0
 * are skipped when mask_rows (the e * mask of carca.py:94 seen from the backward side). */
typedef struct CarcaWgradSeg {
  const float* dy;    /* [rows, ld_dy] */
  const float* x;     /* [rows, ld_x]  -> dW[:, 0:K] */
  const float* x1;    /* [rows, ld_x1] -> dW[:, K:K+K1], or NULL when K1 == 0 */
  const int32_t* ids; /* [rows] or NULL */
  int32_t rows;
  int32_t T;                     /* rows per user, used with the strides below */
  int64_t x_bstride, x1_bstride; /* users of a [B, T, K] view are this many elements apart; 0 = dense */
  int32_t x_gather;              /* >= 1: x is a table [n_items, ld_x], row r reads x[ids[r]]; > 1 also states n_items */
} CarcaWgradSeg;
typedef struct CarcaWgradDesc {
  CarcaWgradSeg seg[CARCA_MAX_SEGS];
  int32_t nseg;
  int32_t ld_dy, ld_x, ld_x1;
  int32_t N, K, K1; /* dW is [N, K + K1] */
  float* dw;
  int32_t ldw;
  float* db; /* [N] or NULL */
  int32_t mask_rows;
} CarcaWgradDesc;
int carca_gemm_wgrad(const CarcaWgradDesc* desc /*host*/, void* stream);
/* n independent products in ONE launch (the d x d weight gradients of a backward pass are ~20 us latency-bound
 * launches; side by side they fill the chip).  Same semantics as n calls of carca_gemm_wgrad in any order; products
 * with more than 96 x 1024 outputs are passed on to carca_gemm_wgrad one by one. */
int carca_gemm_wgrad_group(const CarcaWgradDesc* descs /*host, [n]*/, int n, void* stream);

/* ---- a1 + a2 + a9: AllEmbedding.forward over several row segments ---------------------------
 * Replaces get_mask (utils.py:6-7) + AllEmbedding.forward (carca.py:85-95) + the additive
 * encodings (carca.py:25-31, 54-60) for the profile and every target group in ONE call:
 *   q = [attrs ; ctx] W_f^T + b_f ; z = E[ids] * sqrt(d) ; e = [z ; q] W_j^T + b_j (+ pos[t]) ;
 *   e *= (ids != 0).
 * zq is workspace AND the tensor the backward needs: [sum(rows), d + g], rows of segment s
 * start at sum(rows of earlier segments).  The q columns of rows with id 0 are written as ZEROS, not computed: their e is
 * masked (carca.py:92-94) and their gradient is zero, so the feature product leaves those rows out where that pays
 * (gemm_rows_skc_kernel: 16 % of an evaluation batch's rows at BASELINE's profile lengths, 47 % of a training batch's).
 * e_out rows have stride ld_e >= d, columns d..ld_e-1
 * are written as zeros.  `stages` selects which of the three launches to issue (bit 0 gather,
 * bit 1 feature GEMM, bit 2 joint GEMM; 7 = all) so a profiler can bracket one of them with events. */
typedef struct CarcaRowSeg {
  const int32_t* ids; /* [rows] item ids, 0 = pad */
  const float* attrs; /* [rows, n_attrs] */
  const float* ctx;   /* [rows, n_ctx] */
  float* e_out;       /* [rows, ld_e] */
  int32_t rows;       /* B * T */
  int32_t T;          /* slots per user (position index = row % T) */
  int32_t add_pos;    /* 1: add pos[row % T] (profile side, carca.py:91-92) */
  int64_t attrs_bstride, ctx_bstride; /* elements between users when attrs/ctx are [B, T, .] views; 0 = dense */
  const float* attrs_table; /* optional [n_items, n_attrs]: when set, `attrs` is ignored and row r uses attrs_table[ids[r]] */
  int32_t attrs_table_rows; /* n_items of attrs_table when known, else 0 (only a speed hint: see CarcaGemmSeg.a0_gather) */
} CarcaRowSeg;
int carca_embed_fwd(const CarcaRowSeg* segs /*host*/, int nseg, int n_attrs, int n_ctx, int d, int g,
                    const float* items_w /*[n_items,d]*/, const float* feats_w /*[g,n_attrs+n_ctx]*/,
                    const float* feats_b /*[g]*/, const float* joint_w /*[d,d+g]*/, const float* joint_b /*[d]*/,
                    const float* pos /*[T,d] or NULL*/, float* zq, int ld_e, int stages, void* stream);

/* ---- a3 + a4: SelfAttentionBlock.forward -----------------------------------------------------
 * Replaces SelfAttentionBlock.forward (carca.py:297-318) incl. MultiHeadAttention.forward
 * (carca.py:228-265) with causal=0, in eval mode / dropout p = 0.  One workgroup per user.
 * Pointers in CarcaSaWeights are PACKED (carca_pack_weights): projections [DPO, DPI] with
 * head-padded rows, biases [DPO] head-padded, ffn matrices [DPI, DPI], LayerNorm vectors [DPI].
 * The five matrices are in FRAGMENT ORDER (CarcaPackDesc.frag16 = 1): a wave's operand load for one 16x16 tile is
 * then eight full cache lines instead of sixteen half-used ones (row-major cost 15 k of the 21 k cycles of the
 * K/V projection phase at C2). */
typedef struct CarcaSaWeights {
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b; /* [DPI] */
  const float *wq, *wk, *wv;                  /* [DPO, DPI], fragment order */
  const float *bq, *bk, *bv;                  /* [DPO] */
  const float *w1, *w2;                       /* [DPI, DPI], fragment order */
  const float *b1, *b2;                       /* [DPI] */
} CarcaSaWeights;
/* Training-mode dropout (nn.Dropout sites carca.py:258,309,312,416): element e of a site is kept iff
 * hash(seed, site, e) >= p * 2^24 (counter-based: no state, any launch order), kept values are scaled by
 * 1/(1-p).  torch's Philox stream cannot be reproduced inside a kernel, so parity is defined at p = 0 and
 * through the masks: every site also writes its keep-mask (uint8, 1 = kept) so that tests can replay the
 * reference arithmetic with the SAME masks.  p = 0 (or a NULL pointer) disables everything. */
typedef struct CarcaDropout {
  float p;
  uint64_t seed;
  uint32_t site; /* first site id of this call; a kernel with several sites uses site, site+1, ... */
  const uint64_t* seed_offset; /* device, or NULL: *seed_offset is added to `seed` when the kernel starts -- a step
                                  captured into a hipGraph repeats its launch arguments, the graph bumps this counter */
} CarcaDropout;

/* Tensors the backward pass needs (all optional; pass save = NULL in eval): */
typedef struct CarcaSaSave {
  float* qn;             /* [B*L, DPI] LayerNorm1(x) */
  float *qh, *kh, *vh;   /* [B*L, DPO] projections, head-padded columns */
  float* r;              /* [B*L, DPI] LayerNorm2's input (attention + residual) */
  float* s2;             /* [B*L, DPI] LayerNorm2's output */
  float* h1;             /* [B*L, DPI] dropout1(LeakyReLU(ffn_1(s2))) */
  uint8_t* m_attn;       /* [B, H, L, L] keep-mask of the attention-weight dropout (site+0), or NULL */
  uint8_t* m_ffn1;       /* [B*L, DPI] keep-mask of dropout1 (site+1), or NULL */
  uint8_t* m_ffn2;       /* [B*L, DPI] keep-mask of dropout2 (site+2), or NULL */
} CarcaSaSave;
int carca_sa_block_fwd(const float* x /*[B*L, ldx]*/, int ldx, const int32_t* ids /*[B*L]*/, float* y /*[B*L, ldy]*/,
                       int ldy, int B, int L, int d, int H, const CarcaSaWeights* w /*host struct*/, int residual,
                       const CarcaSaSave* save /*host struct or NULL*/, const CarcaDropout* drop /*or NULL*/,
                       void* stream);

/* The same block in eval mode (nothing saved, no dropout) with one more promise from the caller:
 *   pads_uniform != 0: within a user, all LEADING pad rows (ids == 0 before the first real slot) of x are equal.  True for
 *   the masked embedding (rows of zeros, carca.py:94) and, since a pad row's output depends on its own input only,
 *   for every block output downstream of it; carca_forward passes 1.  The kernel then computes one of those rows and
 *   writes it to every leading pad slot, and projects / attends / feeds forward only ceil((real slots + 1) / 16) row
 *   tiles.  0 = no assumption (what carca_sa_block_fwd passes for save == NULL, drop == NULL). */
int carca_sa_block_eval(const float* x, int ldx, const int32_t* ids, float* y, int ldy, int B, int L, int d, int H,
                        const CarcaSaWeights* w /*host struct*/, int residual, int pads_uniform, void* stream);
/* Workgroups that the calling thread's last eager eval-mode launch of the block lent to another user: with two workgroups
 * per user and pads_uniform, the second workgroup of a one-tile user (it has no tile of its own) takes tiles 0 / 1 of a
 * four-tile user, up to two donors per recipient, both in user order (tuning key 23 = 1: never).  Read back once the
 * launch's stream has drained; 0 where nothing was lent, -1 before the first such launch. */
long long carca_sa_eval_lent(void);

/* ---- a5 + a6: final LayerNorm + CrossAttentionBlock.forward, grouped --------------------------
 * Replaces CARCA.forward's final norm (carca.py:421) and, for every target group,
 * CrossAttentionBlock.forward (carca.py:338-349): K/V projections of the normed profile are
 * computed once per user, then each group's targets are scored:
 *   y = sigmoid(ffn(MHA(o, p, p) + o)), tril(-1) masking iff training (carca.py:339).
 * One workgroup per user.  y_out[g] is [B, N_g] dense. */
typedef struct CarcaCaWeights {
  const float *ln_w, *ln_b; /* final norm [DPI]; both NULL = p_raw is already normed (standalone decoder) */
  const float *wq, *wk, *wv; /* [DPO, DPI], fragment order (CarcaPackDesc.frag16) */
  const float *bq, *bk, *bv; /* [DPO] */
  const float* ffn_w_pad;    /* decoder.ffn.weight in head-padded order [DPO] */
  const float* ffn_w;        /* decoder.ffn.weight plain, zero-padded [DPI] */
  const float* ffn_b;        /* [1] */
  /* decoder.ffn folded into the value projection (the block's output is the scalar w . (PV + o), carca.py:340-345, so
   * w_h . (P_h V_h) = P_h u_h with u_h[key] = p[key] . wu[h] + cu[h]): wu[h][c] = sum_i w[h*dh+i] W_V[h*dh+i][c]
   * ([16, DPI], rows >= H zero, fragment order), cu[h] = sum_i w[h*dh+i] b_V[h*dh+i] ([16]).  Built by
   * carca_pack_weights (CarcaPackDesc.fold_vec).  Used by the inference kernel (save == NULL); may be NULL, which
   * selects the kernel that materialises V. */
  const float *wu, *cu;
} CarcaCaWeights;
typedef struct CarcaTargetGroup {
  const float* o;     /* embedded targets [B*N, ldo] */
  const int32_t* ids; /* [B*N] */
  float* y;           /* [B, N], row stride ldy */
  int32_t N;
  int32_t ldy;        /* elements between users in y; 0 = N (dense).  > N: the groups' scores are column blocks of ONE
                       * [B, sum N] tensor (what CARCA.forward's torch.cat would build, carca.py:431) */
} CarcaTargetGroup;
typedef struct CarcaCaSave {
  float *kh, *vh;              /* [B*L, DPO] */
  float* qh[CARCA_MAX_GROUPS]; /* [B*N_g, DPO] per group */
  uint8_t* m_attn[CARCA_MAX_GROUPS]; /* [B, H, N_g, L] keep-masks of the attention-weight dropout (site+g), or NULL */
} CarcaCaSave;
int carca_cross_score_fwd(const float* p_raw /*[B*L, ldp] encoder output BEFORE the final norm*/, int ldp,
                          const int32_t* p_ids /*[B*L]*/, float* p_normed /*[B*L, ldp] or NULL*/,
                          const CarcaTargetGroup* groups /*host*/, int ngroups, int ldo, int B, int L, int d, int H,
                          const CarcaCaWeights* w /*host struct*/, int residual, int training,
                          const CarcaCaSave* save /*host struct or NULL*/, const CarcaDropout* drop /*or NULL*/,
                          void* stream);

/* ---- backward kernels (the autograd of the lines cited at each forward entry point) -------------------
 * LayerNorm backward over `rows` rows of width d: dx = dLN(dy; x, gamma) (+ addend); dgamma/dbeta are
 * accumulated with atomics (caller zeroes).  Columns d..ncols_out-1 of dx are written as zeros. */
int carca_layernorm_bwd(const float* dy, int ld_dy, const float* x, int ld_x, const float* gamma, int rows, int d,
                        const float* addend /*or NULL*/, int ld_add, float* dx, int ld_dx, int ncols_out,
                        float* dgamma /*or NULL*/, float* dbeta /*or NULL*/, void* stream);
/* d_items[ids[r]][:] += scale * dz[r][:] for ids[r] != 0 (nn.Embedding(padding_idx=0), carca.py:73,87-88) */
int carca_embed_scatter(const float* dz, int ld_dz, const int32_t* ids, int rows, int d, float scale,
                        float* d_items /*[n_items, d]*/, void* stream);
/* out[(row % T)][c] += sum_rows rowscale[row] * (ids[row] != 0) * x[row][c]; T = 1: plain column sum.
 * rowscale / ids may be NULL.  cols <= 256.  Caller zeroes out. */
int carca_colsum(const float* x, int ld_x, int rows, int cols, const float* rowscale, const int32_t* ids, int T,
                 float* out /*[T, cols]*/, void* stream);
/* Attention core of SelfAttentionBlock (carca.py:246-260, causal = 0): given d(attention output)
 * [B*L, ld_da] in plain feature order and the saved projections, recompute P and return dQ, dK, dV
 * (head-padded, [B*L, DPO]). */
int carca_sa_attn_bwd(const float* qh, const float* kh, const float* vh, const float* d_attn, int ld_da,
                      const int32_t* ids, float* dqh, float* dkh, float* dvh, int B, int L, int d, int H,
                      const uint8_t* m_attn /*[B,H,L,L] or NULL*/, float drop_scale /*1/(1-p)*/, void* stream);
/* Attention core + sigmoid(ffn(.)) head of CrossAttentionBlock (carca.py:340-347) for every group:
 * dlogit = dy * y * (1 - y); d(attention output) = dlogit (x) ffn_w_pad; returns dQ per group, dK, dV
 * (summed over groups) and accumulates d ffn_w_pad[f] += sum dlogit * O[.][f] (caller zeroes it). */
typedef struct CarcaCrossBwdGroup {
  const float* qh;    /* [B*N, DPO] saved by the forward */
  const float* y;     /* [B*N] forward output */
  const float* dy;    /* [B*N] incoming gradient */
  const int32_t* ids; /* [B*N] */
  float* dqh;         /* [B*N, DPO] out */
  float* dlogit;      /* [B*N] out, or NULL */
  const uint8_t* m_attn; /* [B, H, N, L] keep-mask saved by the forward, or NULL */
  int32_t N;
  int32_t ld_y;          /* elements between users in y AND dy; 0 = N (see CarcaTargetGroup.ldy) */
} CarcaCrossBwdGroup;
int carca_cross_attn_bwd(const float* kh, const float* vh, const int32_t* p_ids, const CarcaCrossBwdGroup* groups,
                         int ngroups, const float* ffn_w_pad, float* dkh, float* dvh, float* d_ffn_w_pad, int B, int L,
                         int d, int H, int training, float drop_scale, void* stream);
/* In-place dropout of x [rows, cols] (row stride ld): x = keep ? x / (1-p) : 0; mask [rows, cols] uint8.
 * Used for CARCA.dropout on the profile embedding (carca.py:416). */
int carca_dropout_fwd(float* x, int rows, int cols, int ld, const CarcaDropout* drop, uint8_t* mask, void* stream);
/* out[r][c] = x[r][c] * mask[r][c] * scale for c < cols, 0 for cols <= c < ncols_out (dropout backward) */
int carca_mask_mul(const float* x, int ld_x, const uint8_t* mask, int ld_m, float scale, float* out, int ld_out,
                   int rows, int cols, int ncols_out, void* stream);
/* ---- f4: the reference's ablation decoders and the stand-alone final LayerNorm ---------------------------
 * Row kernels on the padded activation layout (d <= 128; pad columns of every output are written as zeros).
 * carca_layernorm_fwd replaces CARCA.norm.forward (carca.py:421) where no cross-attention kernel fuses it. */
int carca_layernorm_fwd(const float* x, int ldx, float* y, int ldy, int rows, int d, const float* w, const float* b,
                        void* stream);
/* DotProduct.forward (carca.py:361-367) / the scoring step of WeightedDotProduct.forward (carca.py:390-397):
 * y[b][t] = link(p_row . o[b][t]) with p_row = p[b][t] (slotwise = 1: train mode, needs T == L) or p[b][L-1]
 * (slotwise = 0: eval mode); link 0 = sigmoid, 1 = (s + 1) / 2.  p is [B*L, ldp], o is [B*T, ldo], y is [B*T]. */
int carca_dot_score_fwd(const float* p, int ldp, const float* o, int ldo, float* y, int B, int L, int T, int d,
                        int slotwise, int link, void* stream);
/* its backward: d_o[row] = dl * p_row (written), dp[p_row] += dl * o[row] (ACCUMULATED: caller zeroes dp before the
 * first group), dl = dy * dlink/ds */
int carca_dot_score_bwd(const float* p, int ldp, const float* o, int ldo, const float* y, const float* dy, float* dp,
                        int ld_dp, float* d_o, int ld_do, int B, int L, int T, int d, int slotwise, int link,
                        void* stream);
/* WeightedDotProduct's history weighting (carca.py:376-378,385-386): out[b][t][:] = c_t x[b][t][:] with
 * c_t = sum_{j<=t} gamma^j (the reference repeats the history along a new axis, so slots are scaled, not mixed).
 * The map is diagonal, hence its own backward. */
int carca_slot_decay_scale(const float* x, int ldx, float* out, int ldo, int B, int L, int d, float gamma, void* stream);
/* torch.nn.functional.normalize(x, dim=-1) (carca.py:388-389) and its backward */
int carca_l2norm_fwd(const float* x, int ldx, float* y, int ldy, int rows, int d, void* stream);
int carca_l2norm_bwd(const float* x, int ldx, const float* dy, int ld_dy, float* dx, int ld_dx, int rows, int d,
                     void* stream);
/* KNN.forward (knn.py:13-19), the reference's attribute-similarity baseline model: y[b][t] = p_last(b) . o(b, t) over
 * the F attribute features, p_last = the LAST profile slot's attribute row (knn.py:14); raw dot product, no link.
 *   table_rows == 0: p_a is the dense [B, L, F] profile attributes, o_a the dense [B, T, F] target attributes, rows
 *                    contiguous, user b at p_a + b*p_bstride / o_a + b*o_bstride floats (so the two train groups may
 *                    be the halves of one [B, 2L, F] tensor, train.py:86-88); p_x / o_x unused, may be NULL;
 *   table_rows  > 0: p_a is the attribute table [table_rows, F] (o_a unused); rows are p_x[b][L-1] and o_x[b][t]
 *                    (p_x [B, L], o_x [B*T], both contiguous; strides unused); ids outside the table score 0.
 * HBM-bound: B*T*F*4 bytes streamed once. */
int carca_knn_score(const float* p_a, int64_t p_bstride, const float* o_a, int64_t o_bstride, const int32_t* p_x,
                    const int32_t* o_x, int table_rows, float* y, int B, int L, int T, int F, void* stream);
/* ---- stand-alone pieces of the reference's module surface (abstract.py:31, carca.py:25-31, 54-60, 228-265) ----------
 * The hot path never runs these (encodings ride in the embedding GEMM's epilogue, attention is fused into K2 / K4);
 * they exist so that a caller who uses the modules the way the ABCs allow gets the reference's numbers instead of an
 * exception.
 * carca_add_positions: Encoding.forward(x): out[b][t][:] = x[b][t][:] + pos[t][:] for x [B*T, ldx], pos [T, d]. */
int carca_add_positions(const float* x, int ldx, const float* pos, float* out, int ldo, int B, int T, int d, void* stream);
/* carca_mha_core: the attention core of MultiHeadAttention.forward (carca.py:242-260) on PROJECTED inputs (plain feature
 * order, head h = columns [h d/H, (h+1) d/H)): q [B*Tq, ldq], k, v [B*Tk, ldk]; mask = (q_ids != 0) x (k_ids != 0),
 * lower-triangular with diagonal `causal` when has_causal; W = softmax((mask ? 0 : -2^32+1) + q k^T) / sqrt(d/H)) * mask;
 * out [B*Tq, ldo] = W v with heads merged back; w_out (optional) [H*B, Tq, Tk], head-major like the reference's
 * return_w (head h of user b at index h*B + b).  One wave per (user, head, query); any Tq, Tk. */
int carca_mha_core(const float* q, int ldq, const float* k, const float* v, int ldk, const int32_t* q_ids,
                   const int32_t* k_ids, int B, int Tq, int Tk, int d, int H, int has_causal, int causal, float* out,
                   int ldo, float* w_out /*or NULL*/, void* stream);
/* Which kernel each row product took.  carca_gemm_rows_log(NULL, 1) clears the calling thread's log and switches it on
 * ((NULL, 0): off); from then on every row-GEMM launch of that thread appends "kernel rows=.. N=.. K=.. grid=..;".
 * carca_gemm_rows_log(buf, cap) copies the log (NUL-terminated) and returns its length.  tools/bench_configs.py names each
 * configuration's dominant kernel with it. */
int carca_gemm_rows_log(char* out /*or NULL*/, int cap);
/* Rows of the calling thread's last eager "+dedup" launch that represent a distinct attribute row of their batch (one per
 * group of equal attribute rows), whether the product multiplied them or a per-item cache (below) supplied them; read back
 * once the launch's stream has drained; -1 when there was none or the last one was captured.  A hash table that a
 * launch did not hand back clean shows here -- rows stop merging -- and never in the results.  (Under a cache, rows
 * that hit and do not own their id's table slot count as merged: where an id's lowest row carries other bytes than the
 * cache while later rows carry the cache's, those later rows are not counted.) */
long long carca_feat_dedup_rows_multiplied(void);
/* ... and the rows of that launch the product really multiplied: those of the count above that no cache entry served. */
long long carca_feat_dedup_rows_computed(void);
/* ... and the rows of that launch whose compare with their cache entry another row's wave (or their own, as the first of
 * a group) issued together with its neighbours'; 0 where the launch grouped nothing: no cache, the attribute-table path,
 * key 22 = 1, a captured launch, no launch yet. */
long long carca_feat_dedup_rows_grouped(void);
/* A per-item cache of the evaluation feature product's attribute part, P[i] = attrs[i] W_a^T (feat_dedup.hip; DESIGN.md
 * 4f), indexed by item id.  The "+dedup" launches fill it lazily -- a slot's owner row publishes its P row (and, for dense
 * batches, the attribute row it was computed from) into an EMPTY entry -- and later launches take a filled entry's row
 * instead of multiplying, after comparing the batch row's bytes with a_c (dense batches) or without a compare where the
 * rows are gathered from `table` by id.  A filled entry is never overwritten; the owner of the memory empties the cache
 * (zeroes `state`) whenever W_a or the table may have changed.  All device memory, valid until the launches have run.
 *   p_c [n_rows, ld_p] (ld_p >= g), a_c [n_rows, ld_a] (ld_a >= n_attrs) or NULL (table batches only),
 *   state [n_rows] int32: 0 empty, 1 filled, table: the attribute table a_c == NULL stands for, or NULL. */
typedef struct {
  float* p_c;
  float* a_c;
  int32_t* state;
  const float* table;
  int32_t n_rows, ld_p, ld_a;
} CarcaFeatCache;
/* Arms `cache` (copied) for the calling thread's NEXT carca_forward, which hands it to its "+dedup" launches if it has any
 * and disarms it in every case; NULL disarms.  Ignored (the parent launches, nothing read or written) under stream
 * capture, with tuning key 21 = 1, and while a knob of the product's kernel (keys 0, 9 - 13, 15, 17 - 19) is off its
 * default: such a run is about that kernel. */
int carca_feat_cache_arm(const CarcaFeatCache* cache /*or NULL*/);
/* The value carca_set_tuning last gave `key` (0 = the shipped choice); -1 for a key outside the table. */
int carca_get_tuning(int key);
/* carca_mha_core with nn.Dropout on the weights (carca.py:258): W * keep / (1 - p) multiplies v, w_out stays pre-dropout
 * (carca.py:262-263); element (b, h, t, j) of site drop->site, keep-mask written to keep_out [B, H, Tq, Tk] (uint8,
 * or NULL).  drop NULL or p = 0: carca_mha_core.  The attention of profiles longer than the fused kernels' 64 slots
 * (carca_replication_amd/long_profile.py). */
int carca_mha_core_drop(const float* q, int ldq, const float* k, const float* v, int ldk, const int32_t* q_ids,
                        const int32_t* k_ids, int B, int Tq, int Tk, int d, int H, int has_causal, int causal, float* out,
                        int ldo, float* w_out /*or NULL*/, const CarcaDropout* drop /*or NULL*/, uint8_t* keep_out /*or NULL*/,
                        void* stream);
/* Backward of carca_mha_core (torch.autograd over carca.py:242-260): d_out [B*Tq, ldo] (or NULL) and d_w [H*B, Tq, Tk]
 * (or NULL: the gradient of the returned weights) -> dq [B*Tq, ldq] (written), dk, dv [B*Tk, ldk] (ACCUMULATED: zero
 * them first).  The weights are recomputed from q, k and the masks. */
int carca_mha_core_bwd(const float* q, int ldq, const float* k, const float* v, int ldk, const int32_t* q_ids,
                       const int32_t* k_ids, int B, int Tq, int Tk, int d, int H, int has_causal, int causal,
                       const float* d_out /*or NULL*/, int ldo, const float* d_w /*or NULL*/, float* dq, float* dk, float* dv,
                       void* stream);
/* carca_mha_core_bwd behind carca_mha_core_drop: keep = the forward's keep-mask [B, H, Tq, Tk] (NULL = no dropout),
 * keep_scale = 1 / (1 - p). */
int carca_mha_core_bwd_drop(const float* q, int ldq, const float* k, const float* v, int ldk, const int32_t* q_ids,
                            const int32_t* k_ids, int B, int Tq, int Tk, int d, int H, int has_causal, int causal,
                            const float* d_out /*or NULL*/, int ldo, const float* d_w /*or NULL*/, float* dq, float* dk,
                            float* dv, const uint8_t* keep /*or NULL*/, float keep_scale, void* stream);
/* Inverse of carca_pack_weights for gradients: real[r][c] (+)= packed[rp][cp] (same descriptor fields:
 * src = real tensor, dst = packed buffer).  accumulate = 0 overwrites, 1 adds. */
int carca_unpack_grads(const CarcaPackDesc* descs, int n, int accumulate, void* stream);

/* ---- backward of whole modules as ONE host call each (csrc/block_bwd.hip) --------------------------------------
 * The launch sequence of a module's backward is issued from C, like carca_forward issues the inference forward: the
 * training step is otherwise bound by interpreter time per launch.  Each entry launches its input-gradient chain on
 * `stream` and APPENDS its weight-gradient products to the caller's host array `wgrads` (*n_wgrads is advanced); the
 * caller launches them together with carca_gemm_wgrad_group once the whole pass is issued -- until then the
 * workspace and every saved tensor must stay alive.
 * carca_sa_block_bwd: autograd of SelfAttentionBlock.forward (carca.py:297-318): given dL/d(output) it produces
 * dL/d(input) and five products (ffn_2, ffn_1, W_Q, W_K, W_V with their biases); LayerNorm gammas / betas are
 * accumulated directly.  All gradient buffers are ACCUMULATED into (caller zeroes). */
typedef struct CarcaSaBwdDesc {
  int32_t B, L, d, H, residual;
  float drop_p;           /* the block's dropout probability in the forward (0 = none: masks unused) */
  const int32_t* ids;     /* [B*L] */
  const float* dy;        /* [B*L, DPI] gradient of the block's output */
  const float *x_in, *qn, *qh, *kh, *vh, *r, *s2, *h1; /* the block's input + CarcaSaSave of the forward */
  const uint8_t *m_attn, *m_ffn2;                      /* keep-masks of the forward (drop_p > 0) */
  const float *wq_t, *wk_t, *wv_t; /* [DPI, DPO]: Bt[n = input feature][k = head-padded output feature] = W[k][n] */
  const float *w1_t, *w2_t;        /* [DPI, DPI] transposed ffn weights */
  const float *ln1_w, *ln2_w;      /* LayerNorm gammas [d] */
  float *g_w1, *g_b1, *g_w2, *g_b2;             /* d ffn_1 / ffn_2: [d, d] (row stride d), [d] */
  float *g_wq, *g_wk, *g_wv, *g_bq, *g_bk, *g_bv; /* head-padded staging: [DPO, d] (row stride d), [DPO] */
  float *g_ln1_w, *g_ln1_b, *g_ln2_w, *g_ln2_b; /* [d] */
  float* workspace;       /* carca_sa_block_bwd_workspace(B, L, d, H) floats, alive until the products have run */
  float* dx;              /* out [B*L, DPI] gradient of the block's input */
} CarcaSaBwdDesc;
size_t carca_sa_block_bwd_workspace(int B, int L, int d, int H);
int carca_sa_block_bwd(const CarcaSaBwdDesc* desc /*host*/, CarcaWgradDesc* wgrads /*host, room for 5 more*/,
                       int* n_wgrads, void* stream);

/* carca_cross_score_bwd: autograd of the final LayerNorm (carca.py:421) + CrossAttentionBlock.forward (carca.py:338-349)
 * over every target group: given dL/dy per group it produces dL/d(embedded targets) per group (masked like e * mask),
 * dL/d(encoder output) and up to four products (ffn head, W_Q over all groups, W_K, W_V). */
typedef struct CarcaCrossBwdIn {
  const float* qh;       /* [B*N, DPO] saved by carca_cross_score_fwd */
  const float* y;        /* [B*N] forward scores */
  const float* dy;       /* [B*N] incoming gradient */
  const int32_t* ids;    /* [B*N] */
  const float* o;        /* [B*N, DPI] embedded targets (the forward's input) */
  const uint8_t* m_attn; /* keep-mask of the forward (drop_p > 0) or NULL */
  float* de;             /* out [B*N, DPI]: gradient of the embedded targets */
  int32_t N;
  int32_t ld_y;          /* elements between users in y AND dy; 0 = N */
} CarcaCrossBwdIn;
typedef struct CarcaCrossBwdDesc {
  int32_t B, L, d, H, ngroups, residual, training;
  float drop_p;
  CarcaCrossBwdIn group[CARCA_MAX_GROUPS];
  const int32_t* p_ids;                /* [B*L] */
  const float *kh, *vh;                /* [B*L, DPO] saved */
  const float* p_normed;               /* [B*L, DPI] final-norm output saved by the forward */
  const float* enc_out;                /* [B*L, DPI] encoder output (the final norm's input) */
  const float *wq_t, *wk_t, *wv_t;     /* [DPI, DPO] transposed head-padded copies */
  const float* ffn_w_pad;              /* [DPO] decoder.ffn.weight, head-padded (CarcaCaWeights.ffn_w_pad) */
  const float* ffn_w;                  /* [d] decoder.ffn.weight as is */
  const float* norm_w;                 /* [d] final LayerNorm gamma; NULL = the stand-alone CrossAttentionBlock on an already
                                          normed profile: no LayerNorm stage (enc_out, g_norm_* unused, dx = d p_normed)
                                          and de is the gradient of the block's INPUT o, not masked by ids */
  float *g_ffn_w, *g_ffn_b;            /* [d], [1] */
  float* g_ffn_w_pad;                  /* [DPO] head-padded staging of the attention part of d ffn.weight */
  float *g_wq, *g_wk, *g_wv, *g_bq, *g_bk, *g_bv; /* head-padded staging: [DPO, d], [DPO] */
  float *g_norm_w, *g_norm_b;          /* [d] */
  float* workspace;                    /* carca_cross_score_bwd_workspace(...) floats, alive until the products ran */
  float* dx;                           /* out [B*L, DPI]: gradient of the encoder output */
} CarcaCrossBwdDesc;
size_t carca_cross_score_bwd_workspace(int B, int L, int d, int H, const int32_t* Ns /*host [ngroups]*/, int ngroups);
int carca_cross_score_bwd(const CarcaCrossBwdDesc* desc /*host*/, CarcaWgradDesc* wgrads /*host, room for 4 more*/,
                          int* n_wgrads, void* stream);

/* carca_embed_bwd: autograd of AllEmbedding.forward (carca.py:85-95) over all row segments, given dL/de per segment
 * (NOT yet masked: the e * mask of carca.py:94 is applied here): position-encoding gradient, d joint_embed, d [z ; q],
 * item-row scatter-add, d feats_embed.  Everything is launched here (these products feed each other). */
typedef struct CarcaEmbedBwdSeg {
  const float* de;           /* [rows, ld_de] */
  const int32_t* ids;        /* [rows] */
  const float* attrs;        /* [rows, n_attrs] (or a [B, T, n_attrs] view, see attrs_bstride) */
  const float* ctx;          /* [rows, n_ctx] */
  const float* attrs_table;  /* optional [n_items, n_attrs]: rows gathered by id instead of `attrs` */
  int64_t attrs_bstride, ctx_bstride;
  int32_t rows, T, attrs_table_rows;
  int32_t joint_only;        /* 1: this segment only enters d joint_embed here -- its d [z ; q], scatter-add and d feats_embed
                              * are another call's (the same pass's second stream, see skip_joint) */
} CarcaEmbedBwdSeg;
typedef struct CarcaEmbedBwdDesc {
  CarcaEmbedBwdSeg seg[CARCA_MAX_SEGS]; /* seg[0] = the profile (the only one with a position encoding) */
  int32_t nseg, d, g, n_attrs, n_ctx, ld_de, L;
  const float* zq;        /* [sum rows, d + g] saved by carca_embed_fwd */
  const float* joint_wt;  /* [d + g, ld_joint_wt]: joint_embed.weight transposed (Bt of the input-gradient product) */
  int32_t ld_joint_wt;
  float *g_items, *g_feats_w, *g_feats_b, *g_joint_w, *g_joint_b; /* accumulated into (caller zeroes) */
  float* g_pos;           /* [L, d] gradient of LearnableEncoding.encoding.weight, or NULL */
  float* workspace;       /* carca_embed_bwd_workspace(...) floats */
  void* ev_early;         /* optional hipEvent_t recorded on `stream` right BEFORE the last launch (d feats_embed, as long as
                           * the whole forward GEMM): behind it every other gradient of the model is final, so a gradient
                           * all-reduce of everything but feats_embed.{weight,bias} can start under that kernel */
  int32_t skip_joint;     /* 1: no d joint_embed in this call (a later call of the pass lists these segments joint_only):
                           * a backward pass may hand the target rows' share to a second stream as soon as their d e is
                           * final and keep the small d joint_embed product in ONE launch over all rows */
} CarcaEmbedBwdDesc;
size_t carca_embed_bwd_workspace(const int32_t* rows /*host [nseg]*/, int nseg, int d, int g);
int carca_embed_bwd(const CarcaEmbedBwdDesc* desc /*host*/, void* stream);
/* 1 when this thread's last carca_embed_bwd call with an ev_early recorded it.  On a stream that is being captured the
 * record is an EXTERNAL event-record node (every replay records the event in front of its last kernel); a HIP runtime that
 * offers no way to add one leaves the event alone and this returns 0: reduce the early range behind the replay then. */
int carca_early_event_recorded(void);

/* ---- f3: the optimizer step of the train driver (training.py:174, train.py:96) -------------------------------
 * torch.optim.Adam's update (no amsgrad; weight_decay added to the gradient) for every tensor of the table in one
 * launch: g += wd*p; m += (1-b1)(g-m); v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).
 * `tensors` is a HOST array of n entries (device pointers, n elements each, fp32); step = t >= 1.  The scalar
 * hyper-parameters arrive as doubles and are combined in double before one rounding to fp32, as torch does. */
typedef struct {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  /* Optional row mask of an embedding table [n / row_len, row_len]: rows whose byte is 0 are SKIPPED.  Exact as long as
   * the caller marks every row that ever received a non-zero gradient and weight_decay is 0: a row with g = m = v = 0
   * has an update of exactly 0 (m, v stay 0, p -= lr * 0 / (0 + eps)), so skipping it gives the bits of the dense
   * sweep without reading or writing its four arrays (1 M items x 128: 2.5 GB per step).  NULL = every row. */
  const uint8_t* row_mask;
  int64_t row_len;
} CarcaAdamTensor;
int carca_adam_step(const CarcaAdamTensor* tensors, int n, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int step, void* stream);
/* The same launch with two options.  carca_adam_step forwards here with decoupled = 0, grad_scale = NULL.
 *   grad_scale (device, one float, may be NULL): g = g * *grad_scale before anything else, the product rounded on its
 *     own -- the bits of scaling the gradient in a separate pass (clipping by global norm: out[1] of carca_grad_norm).
 *   decoupled != 0: torch.optim.AdamW's decay, p = p * (1 - lr*weight_decay) (the factor combined in double, rounded
 *     once), then Adam's update on the undecayed g, instead of g += wd*p.
 * A row mask needs weight_decay == 0 with either style: decoupled decay moves untouched rows too. */
int carca_adam_step_ex(const CarcaAdamTensor* tensors, int n, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int step, int decoupled, const float* grad_scale, void* stream);
/* The 2-norm of every gradient of the table taken as one vector, and the factor that clips it to max_norm (> 0):
 *   out[0] = norm = (float)sqrt(sum g^2),  out[1] = scale = min(1, max_norm / (norm + 1e-6f))  (fp32)
 * -- torch.nn.utils.clip_grad_norm_'s arithmetic with error_if_nonfinite=False: a non-finite gradient gives a
 * non-finite scale.  Only g, n, row_mask and row_len of an entry are read; rows whose mask byte is 0 are not read at all
 * (their gradient is exactly 0 by the contract above, so the result has the bits of the unmasked sum); a row mask needs
 * row_len >= 1 dividing n.  One fp32 partial per 1024-element chunk goes to `partials` (device, n_partials >= the sum
 * over entries of ceil(n_i / 1024) floats), one block then adds them in double in index order: no atomics, the same
 * bits for the same gradients on every call.  The library allocates nothing; `partials` and `out` (device, 2 floats)
 * are the caller's.  Launches only: reading `out` is the caller's synchronisation. */
int carca_grad_norm(const CarcaAdamTensor* tensors /*host [n]*/, int n, double max_norm, float* partials, int64_t n_partials,
                    float* out /*[2]: norm, scale*/, void* stream);
/* mask[ids[i]] = 1 for i < n (ids outside [0, n_rows) are ignored): the rows a batch touches, for CarcaAdamTensor.row_mask */
int carca_mark_rows(const int32_t* ids, int64_t n, uint8_t* mask, int64_t n_rows, void* stream);
/* table[ids[i]][0 .. row_len) = 0 for every id of up to CARCA_MAX_SEGS id lists (ids outside [0, n_rows) ignored): clears
 * the rows the previous step's scatter-add touched instead of the whole gradient table.  carca_concat_ids copies the
 * lists back to back into `out` (sum of counts entries): the caller's private record of a step's "dirty" rows. */
int carca_zero_rows(float* table, int64_t n_rows, int row_len, const int32_t* const* ids /*host [nlists]*/,
                    const int64_t* counts /*host [nlists]*/, int nlists, void* stream);
int carca_concat_ids(const int32_t* const* ids /*host [nlists]*/, const int64_t* counts /*host*/, int nlists,
                     int32_t* out, void* stream);

/* ---- f1: batch construction on the device (data.py:53-192) ---------------------------------------------------
 * The interaction log lives in HBM as CSR: user u owns hist[offs[u] .. offs[u+1]) (item ids in interaction order) and
 * the context rows hctx[offs[u] ..] of those interactions (hctx[pos] = ctx[(user, hist[pos])], data.py:17-25).
 * `users` selects the batch; held_out / floor_ are pad_profile's split constants (data.py:53-74):
 *   train: held_out = 2 if a test split exists else 1, floor_ = 1;  val: 1 or 0, floor_ = 2;  test: 0, floor_ = 3.
 * Negatives are distinct ids in [1, n_items-1] outside the user's whole history (data.py:77-87), drawn by rejection
 * from a counter-based hash of (seed, user, attempt): reproducible per seed, not python's `random` stream.
 * carca_build_eval_batch = get_test_sequences (data.py:140-192): p_x [B,L] left-padded history, p_c [B,L,n_ctx],
 *   o_x [B,1+N] = held-out item then N negatives, o_c [B,1+N,n_ctx] = the held-out interaction's context for every
 *   candidate, y_true [B,1+N] = one-hot at column 0.  N <= 2048.
 * carca_build_train_batch = get_train_sequences (data.py:90-137): o_x [B,2L] = successors | negatives aligned with the
 *   history slots, o_c [B,2L,n_ctx] = the successor's context for both, y_true [B,2L] = (p_x > 0) | 0.
 * Attribute rows are NOT materialised: AllEmbedding.register_attr_table gathers them inside the feature GEMM.
 * offs has n_users + 1 entries; a user index outside [0, n_users) yields an all-pad row (no history, no candidates). */
int carca_build_eval_batch(const int32_t* hist, const int64_t* offs, const float* hctx, const int32_t* users, int n_users,
                           int B, int L, int N, int n_ctx, int n_items, int held_out, int floor_, uint64_t seed, int32_t* p_x,
                           float* p_c, int32_t* o_x, float* o_c, int32_t* y_true, void* stream);
int carca_build_train_batch(const int32_t* hist, const int64_t* offs, const float* hctx, const int32_t* users, int n_users,
                            int B, int L, int n_ctx, int n_items, int held_out, int floor_, uint64_t seed, int32_t* p_x,
                            float* p_c, int32_t* o_x, float* o_c, int32_t* y_true, void* stream);

/* ---- a7: CARCA.forward (carca.py:411-431), inference path, as ONE host call -----------------------------
 * Issues the whole launch sequence -- gather, feature GEMM, joint GEMM, every SelfAttentionBlock, final norm +
 * grouped cross-attention scoring -- on `stream` without returning to the caller in between, so that a slow
 * host thread cannot starve the GPU (the Python layer needs ~25 interpreter-level calls per forward otherwise).
 * No tensors are saved for a backward pass and no dropout is applied: eval mode, or train mode without grad
 * at p = 0.  All buffers are caller-allocated:
 *   segs[0] = profile, segs[1..ngroups] = target groups (their e_out feed the scoring kernel),
 *   x_work[2] = two [B*L, ld_e] ping-pong buffers for the blocks' outputs.
 * ev (optional, host array of 4 hipEvent_t, entries may be NULL): so that a benchmark can time exactly these kernels
 * inside its timed region.  ev[0], ev[1] (both or neither) are BOUND to the feature GEMM's dispatch on `stream`
 * (hipExtLaunchKernel: start / end of that kernel, hipEventElapsedTime(ev[0], ev[1]) = its duration; nothing extra is
 * queued).  ev[2], ev[3] (both or neither) are bound the same way to the scoring kernel's dispatch (a hipEventRecord
 * would be a barrier packet of its own: ~6 us of GPU time between two kernels). */
#define CARCA_MAX_BLOCKS 8
typedef struct CarcaForwardDesc {
  CarcaRowSeg segs[CARCA_MAX_SEGS];
  int32_t ngroups;
  int32_t B, L, d, g, H, n_attrs, n_ctx, n_blocks, ld_e;
  const float *items_w, *feats_w, *feats_b, *joint_w, *joint_b, *pos;
  float* zq;
  float* x_work[2];
  CarcaSaWeights sa[CARCA_MAX_BLOCKS];
  int32_t sa_residual[CARCA_MAX_BLOCKS];
  CarcaCaWeights ca;
  int32_t ca_residual, training;
  float* y[CARCA_MAX_GROUPS];   /* [B, N_g] outputs, row stride ldy */
  int32_t N[CARCA_MAX_GROUPS];
  int32_t ldy;                  /* 0 = every group dense [B, N_g]; else the groups are column blocks of one [B, ldy] tensor */
  float* p_normed;              /* optional [B*L, ld_e] */
  /* Optional FOLDED embedding (inference with frozen weights).  AllEmbedding has no nonlinearity (carca.py:86-89),
   * so e = z W_jz^T + [a;c] (W_jq W_f)^T + (W_jq b_f + b_j): with fold_wc = W_jq W_f [d, F] (row stride
   * fold_ldwc) and fold_bias [d] prepared once per weight version, the F->g->d pair of GEMMs becomes one F->d
   * GEMM (5x fewer executed flops at g = 5d) and zq is not touched.  Same algebra, different fp32 summation
   * order (~1e-6 relative); NULL = the two-GEMM path that mirrors the reference operation by operation. */
  const float* fold_wc;
  const float* fold_bias;
  int32_t fold_ldwc;
  /* TRAINING extras (all zero / NULL = the inference forward): the same launch sequence with the tensors the backward
   * entries (carca_sa_block_bwd, carca_cross_score_bwd, carca_embed_bwd) need, and the reference's dropout sites.
   *   x_out[i]     block i writes its output here instead of the ping-pong buffers (block i+1's input is saved)
   *   sa_save[i]   CarcaSaSave of block i (save_blocks = 1);  ca_save: CarcaCaSave of the scoring kernel (save_cross = 1);
   *                p_normed (above) receives the final norm's output
   *   p_embed / p_block / p_cross  dropout probabilities of CARCA.dropout (carca.py:416), of every block's three sites
   *                and of the decoder's attention weights; one `seed` per forward; sites 1000, 4 i .. 4 i + 2, 2000 + g;
   *                m_embed [B*L, d] receives the embedding dropout's keep-mask */
  float* x_out[CARCA_MAX_BLOCKS];
  CarcaSaSave sa_save[CARCA_MAX_BLOCKS];
  CarcaCaSave ca_save;
  int32_t save_blocks, save_cross;
  float p_embed, p_block, p_cross;
  uint64_t seed;
  uint8_t* m_embed;
  const uint64_t* seed_offset; /* device or NULL, see CarcaDropout */
  int32_t n_events;            /* entries of carca_forward's `ev` array: 0 or 4 = the four described there, 8 = four more:
                                * ev[4], ev[5] bound to the FIRST SelfAttentionBlock's dispatch, ev[6], ev[7] to the joint
                                * GEMM's (AllEmbedding.joint_embed, carca.py:89) */
  /* Optional PROJECTED item table (inference, nothing saved for a backward): z_table[i] = sqrt(d) items_w[i] W_jz^T,
   * [n_items, ld_z_table], prepared once per weight version.  joint_embed is linear (carca.py:89), so
   *   e = [z ; q] W_j^T + b_j = q W_jq^T + z_table[id] + b_j:
   * the item rows are never gathered into zq (no gather launch, carca.py:87-88), the joint product runs over the g
   * columns of q only, and the item term is added per row in its epilogue.  Same algebra, another fp32 summation order
   * (~1e-7 relative).  NULL = the reference's operation order (gather, then one product over d + g columns). */
  const float* z_table;
  int32_t ld_z_table;
} CarcaForwardDesc;
int carca_forward(const CarcaForwardDesc* desc /*host*/, void* const* ev /*4 hipEvent_t or NULL*/, void* stream);
/* Event helpers so that a host language without a HIP binding can time kernels on the launch stream. */
int carca_event_create(void** ev_out);
int carca_event_destroy(void* ev);
int carca_event_elapsed_ms(void* start, void* stop, float* ms_out); /* both must have completed */
int carca_stream_wait_event(void* stream, void* event);            /* hipStreamWaitEvent */

/* ---- a8: BinaryCrossEntropy.forward (carca.py:441-444) -----------------------------------------
 * loss = sum(l * m) / sum(m), l = -(t log(y+eps) + (1-t) log(1-y+eps)), m = (ids != 0).
 * scratch: 2 floats, written by the call as [sum(l*m), sum(m)]; loss_out: 1 float.  dy (optional)
 * receives dloss/dy.  denom (optional, device float[1]) replaces sum(m) as the normaliser: with users
 * sharded over ranks it holds the all-reduced mask count, so that summing the ranks' gradients gives
 * exactly the single-process batch gradient. */
int carca_bce_fwd(const float* y, const int32_t* y_true, const int32_t* ids, int n, float eps, float* scratch,
                  float* loss_out, float* dy /*or NULL*/, const float* denom /*or NULL*/, void* stream);

/* ---- M: compute_HR / compute_NDCG (train.py:15-32) without the sort ----------------------------
 * With p = pos[u] (the positive's column; NULL = column 0 as in data.py:165,190):
 * rank[u] = #{j != p : y[u][j] > y[u][p]}; sums[0] += [rank < k], sums[1] += [rank<k]/log2(rank+2),
 * sums[2] += #{j != p : y[u][j] == y[u][p]} (ties: the reference's unstable sort is undefined there).
 * NaN: `>` and `==` above are taken in the order of the reference's torch.sort(descending=True) -- a NaN score ranks
 * above every number and ties with NaN.  A finite positive ranks below every NaN candidate; a NaN positive has rank 0 and
 * the other NaNs of its row are counted in sums[2].
 * sums is accumulated into (caller zeroes it once per evaluation).  pos holds B entries, each in [0, N). */
/* One evaluation batch of train.py:41-51 in one launch: sums[0..2] as carca_rank_metrics with the positive in column 0
 * (data.py:165,190; the same NaN order), sums[3] += BinaryCrossEntropy(y, y_true, ids != 0) (carca.py:441-444),
 * sums[4] += B; fixed summation order (reproducible).  B x N <= 16384, else CARCA_ERR_UNSUPPORTED (use the two calls). */
int carca_eval_metrics(const float* y /*[B,N]*/, const int32_t* y_true, const int32_t* ids, int B, int N, int k, float eps,
                       float* sums /*[5]*/, void* stream);
int carca_rank_metrics(const float* y /*[B,N]*/, int B, int N, int k, const int32_t* pos /*[B] or NULL*/,
                       int32_t* rank /*[B] or NULL*/, float* sums /*[3]*/, void* stream);

/* ---- full-catalogue top-k (replaces scoring every item as a target group: carca.py:338-349, 352-399 over the candidate
 * lists of data.py:180-185, ranked as train.py:15-32 does) ------------------------------------------------------------
 * Eval mode only.  Each embedding is affine in the context, e(i, c) = T[i] + M c for i != 0, so the item side is a table
 * built once per weight version and the user side a few rows per user.  For user u, item i >= 1:
 *   decoder 0 (CrossAttentionBlock): logit = sum_h softmax_l((item_q[i]_h . K_ulh + user_q[u]_h . K_ulh) / sqrt(dh)) u_ulh
 *            + item_w[i] + user_off[u] + ffn_b[0]  over the profile slots l with p_ids != 0 (no slot: attention term 0);
 *            item_q = QT [n_items, d] (T W_Q^T + b_Q), user_k = K [B*L, d], user_u = folded values [B*L, H]
 *            (p_l . wu_h + cu_h), user_q = (M c_u) W_Q^T [B, d] or NULL, item_w = w_ffn . T[i] or NULL (no residual),
 *            user_off [B] or NULL, ffn_b device float[1] or NULL;
 *   decoder 1 (DotProduct / WeightedDotProduct): logit = user_q[u] . (item_q[i] + user_m[u]), item_q = T, user_q = the
 *            scored profile row, user_m = M c_u [B, d] or NULL;
 *   decoder 2 (WeightedDotProduct(normalize=True)): decoder 1's logit / max(||item_q[i] + user_m[u]||, 1e-12).
 * Writes the k best items per user, best first: ids_out [B, k] int64 and scores = sigmoid(logit) ((logit + 1) / 2 for
 * decoder 2) -- what the model's forward returns for that item.  Ties go to the smaller id; id 0 and the nonzero entries of
 * exclude [B, n_exclude] (int32, 0 = no entry, duplicates allowed) are never selected; fewer than k eligible items pad
 * with id 0 and score 0.  Bit-identical run to run (no float atomics).  Logits of the B x n_items pairs live in stream
 * scratch.  L may be up to CARCA_MAX_PROFILE_L: the dot decoders read only the scored row; decoder 0 keeps a user's valid
 * slots in LDS whole up to CARCA_MAX_L, and beyond walks them CARCA_MAX_L at a time with the same per-slot arithmetic in the
 * same order, so a (user, item) logit depends on the user's valid slots and not on L or on where the pad slots lie
 * (DESIGN.md section 19).  exclude may then be as wide as the profile.  CARCA_ERR_UNSUPPORTED: L > CARCA_MAX_PROFILE_L,
 * k > 128, d > 128 or d % H != 0, a cross-attention (d, H) with no kernel built.  CARCA_ERR_BADARG: null pointers, strides shorter than a row, ld_item_q / ld_user_k / ld_user_q /
 * ld_user_m not multiples of 4. */
typedef struct CarcaRecommendDesc {
  int B, L, n_items, d, H, k;
  int decoder;          /* 0 cross-attention, 1 dot, 2 normalised dot */
  const int32_t* p_ids; /* [B, ld_p_ids] profile ids */
  int ld_p_ids;
  const float* item_q; /* [n_items, ld_item_q] */
  int ld_item_q;
  const float* item_w; /* [n_items] with stride ld_item_w, or NULL */
  int ld_item_w;
  const float* user_k; /* [B*L, ld_user_k] */
  int ld_user_k;
  const float* user_u; /* [B*L, ld_user_u] */
  int ld_user_u;
  const float* user_q; /* [B, ld_user_q] (decoder 0: may be NULL) */
  int ld_user_q;
  const float* user_m; /* [B, ld_user_m] or NULL */
  int ld_user_m;
  const float* user_off; /* [B] with stride ld_user_off, or NULL */
  int ld_user_off;
  const float* ffn_b; /* float[1] or NULL */
  const int32_t* exclude; /* [B, ld_exclude], first n_exclude columns read */
  int n_exclude, ld_exclude;
  float* scores; /* [B, ld_scores] */
  int ld_scores;
  int64_t* ids_out; /* [B, ld_ids_out] */
  int ld_ids_out;
} CarcaRecommendDesc;
int carca_recommend(const CarcaRecommendDesc* desc, void* stream);

/* ---- exact full-catalogue ranks of listed items (the full-ranking protocol's question, "where does the held-out item
 * land among all items", without a top-k list) ---------------------------------------------------------------------
 * The model-side fields (B .. ffn_b) and the exclusion list mean exactly what they mean in CarcaRecommendDesc, and the
 * logit of a (user, item) pair is bit-identical to carca_recommend's, so the two calls order items identically: logit
 * descending, ties to the smaller id.  For user u and list entry j, with id = items[u][j]:
 *   ranks[u][j]  = number of ELIGIBLE items (id != 0, not excluded) that order strictly before id -- the position
 *                  carca_recommend would give it; an excluded or repeated id still gets the position it would take;
 *   scores[u][j] = sigmoid(logit) ((logit + 1) / 2 for decoder 2), as carca_recommend's scores;
 *   id 0 or an id outside [0, n_items): rank -1 and score 0 (never read out of bounds).
 * Three launches, no host wait, nothing retained: the listed and excluded items are scored; a sweep over the catalogue
 * counts per (user, target) the items ordering before the target with integer atomics into a zeroed counter (no
 * [B, n_items] buffer); a correction subtracts the distinct excluded ids that order before it.  Bit-identical run to
 * run.  Scratch: stream scratch, or the capture's memory.  L up to CARCA_MAX_PROFILE_L as carca_recommend (the list is then
 * scored in rounds of 256 entries, the profile staged again in each).  CARCA_ERR_UNSUPPORTED as carca_recommend, and n_list outside
 * 1..128.  CARCA_ERR_BADARG as carca_recommend, and null items / scores / ranks or strides shorter than n_list. */
typedef struct CarcaRankDesc {
  int B, L, n_items, d, H;
  int decoder;          /* 0 cross-attention, 1 dot, 2 normalised dot */
  const int32_t* p_ids; /* [B, ld_p_ids] profile ids */
  int ld_p_ids;
  const float* item_q; /* [n_items, ld_item_q] */
  int ld_item_q;
  const float* item_w; /* [n_items] with stride ld_item_w, or NULL */
  int ld_item_w;
  const float* user_k; /* [B*L, ld_user_k] */
  int ld_user_k;
  const float* user_u; /* [B*L, ld_user_u] */
  int ld_user_u;
  const float* user_q; /* [B, ld_user_q] (decoder 0: may be NULL) */
  int ld_user_q;
  const float* user_m; /* [B, ld_user_m] or NULL */
  int ld_user_m;
  const float* user_off; /* [B] with stride ld_user_off, or NULL */
  int ld_user_off;
  const float* ffn_b; /* float[1] or NULL */
  const int32_t* exclude; /* [B, ld_exclude], first n_exclude columns read */
  int n_exclude, ld_exclude;
  const int32_t* items; /* [B, ld_items], first n_list columns: the items to rank */
  int n_list, ld_items;
  float* scores; /* [B, ld_scores] */
  int ld_scores;
  int64_t* ranks; /* [B, ld_ranks] */
  int ld_ranks;
} CarcaRankDesc;
int carca_rank_items(const CarcaRankDesc* desc, void* stream);

/* ---- top-k and exact ranks among a candidate set ("among THESE items": in stock, one category, cold items; full-ranking
 * metrics over a target item set) ------------------------------------------------------------
 * CarcaCandidates is one set S of item ids shared by the batch: ids [n] int32 on the device, ASCENDING and DISTINCT (the
 * caller's contract: positions then order as ids do, so ties still go to the smaller id), every id in [1, n_items).  An id
 * outside [1, n_items) in the list is treated as not live and is never read out of bounds.  n = 0 is legal (no sweep is
 * launched).  The descriptors are carca_recommend's and carca_rank_items' own, and carca_recommend / carca_rank_items are
 * the same implementation over the whole catalogue: the logit of a (user, item) pair does not depend on the position that
 * holds the item, so scores and the item order are bit-identical to the unrestricted calls'.
 *
 * carca_recommend_among: the k best items of S minus the excluded ids per user, in carca_recommend's order, padded with
 * id 0 and score 0.  The logit scratch is [B, n], indexed by position; exclusion finds an excluded id's position by binary
 * search; selection keys on the position and writes ids[position].
 *
 * carca_rank_items_among: ranks[u][j] = number of eligible items OF S (in S, not excluded) that order strictly before
 * items[u][j]; a target outside S, an excluded or a repeated one still gets the position it would take; id 0 or an id
 * outside [0, n_items): rank -1 and score 0.  scores as carca_rank_items.  The counting sweep runs over S; the correction
 * subtracts only the distinct excluded ids that S holds.
 *
 * Cost falls with n: the sweep's grid, the scratch and the selection cover n positions, not n_items.  Limits (L up to
 * CARCA_MAX_PROFILE_L) and errors as the unrestricted calls, and CARCA_ERR_BADARG for a null list, n < 0, or null ids with n > 0. */
typedef struct CarcaCandidates {
  const int32_t* ids; /* [n] ascending, distinct, in [1, n_items) */
  int n;
} CarcaCandidates;
int carca_recommend_among(const CarcaRecommendDesc* desc, const CarcaCandidates* candidates, void* stream);
int carca_rank_items_among(const CarcaRankDesc* desc, const CarcaCandidates* candidates, void* stream);

/* ---- deep top-k: the first stage in front of a re-ranker, a business-rule filter or carca_recommend_lists (DESIGN.md
 * section 26) ----------------------------------------------------------------------------------------------------------
 * carca_recommend / carca_recommend_among in depth: the descriptor and the candidate list are theirs, every field means
 * what it means there, and 1 <= k <= 4096.  The contract is carca_recommend's:
 *   order      best first by RAW LOGIT descending, ties to the smaller id; the link (sigmoid, or (logit + 1) / 2 for
 *              decoder 2) is applied to the k selected logits only;
 *   exclusion  id 0 and the nonzero entries of exclude [B, n_exclude] are never returned;
 *   padding    fewer than k eligible items pad with id 0 and score 0; an empty candidate list gives all zeros;
 *   prefix     the first j columns of a call with k are the call with j, bit for bit in both outputs, for every j <= k;
 *              for k <= 128 both outputs are carca_recommend's (carca_recommend_among's) bit for bit;
 *   scores     a returned pair's score has carca_recommend's / carca_score_lists' bits: scoring and exclusion ARE
 *              carca_recommend's launches into its [B, n_items] ([B, n] under a list) stream scratch;
 *   keys       selection orders by the 64-bit key (order-preserving logit bits, then the complemented column); under a
 *              candidate list the column is the position in the ascending list and ids_out holds ids[position];
 *   ids_out    int64, usable unchanged as the lists of carca_recommend_lists / carca_score_lists (id 0 scores 0 there).
 * Selection splits a user's row into S contiguous parts: a launch on grid (B, S) writes each part's min(k, part length)
 * best keys to [B, S, kp] uint64 of stream scratch (or the capture's memory), a launch on grid (B) takes the k largest of
 * them, links and writes; S = 1 skips the first launch and selects from the row.  S is chosen from B, the row length and
 * the CU count (tuning key 24 forces it) and lowered, down to 1, while that scratch would pass 1 GiB -- never an error.
 * Keys are distinct, so the result is bit-identical run to run and for every S.  Integer LDS atomics only.
 * Limits and errors as carca_recommend / carca_recommend_among with "retrieve" in the message, and CARCA_ERR_UNSUPPORTED
 * for k > 4096; CARCA_ERR_BADARG for k < 1 or ld_scores / ld_ids_out < k. */
int carca_retrieve(const CarcaRecommendDesc* desc, void* stream);
int carca_retrieve_among(const CarcaRecommendDesc* desc, const CarcaCandidates* candidates, void* stream);

/* ---- Gumbel top-k sampling with logged propensities: exploration, and the pi(a | x) of an off-policy estimator
 *  -----------------------------------------------------------------------------------------------
 * carca_recommend_sampled draws, per user, k items WITHOUT replacement from softmax(logit / temperature) over the user's
 * eligible items -- a Plackett-Luce list -- and returns each drawn item's log-probability under that softmax.  The
 * descriptor and the (nullable) candidate list are carca_retrieve's, 1 <= k <= 4096; eligibility is carca_recommend's
 * (id != 0, not in exclude, inside the candidate list when one is given).  With z = logit / temperature (one fp32
 * division) and g the noise below:
 *   ids_out    the k eligible items with the largest z + g, largest first, ties in z + g to the smaller id (the keys of
 *              carca_retrieve's selection over the perturbed values); fewer than k eligible items pad with id 0;
 *   scores     link(raw logit) of the pair, bit for bit carca_recommend's / carca_score_lists': scoring and exclusion ARE
 *              carca_recommend's launches, and the perturb pass only reads their buffer; padding scores 0;
 *   log_probs  z - logsumexp(z over the user's eligible items): the item's first-draw log-probability; padding is -inf.
 *              The conditional log-probabilities of the ordered list follow on the host: lp_j - log1p(-sum_{m<j} exp(lp_m)).
 * NOISE CONTRACT.  g is a function of (seed, user key, item id) alone -- never of the column (under a candidate list the
 * id is ids[position]), the batch row, the batch size or any launch shape.  User u's key is user_keys[u], or u when
 * user_keys is NULL.  Every variable below is a 32-bit unsigned, arithmetic mod 2^32; seed and key are 64 bits (the key
 * an int64 reinterpreted), _lo = bits 0..31, _hi = bits 32..63:
 *   mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *   hu = mix32( seed_lo ^ (key_lo * 0x9E3779B1) )
 *   hu = mix32( hu ^ seed_hi ^ (key_hi * 0x85EBCA77) )
 *   h  = mix32( hu ^ (item * 0xC2B2AE3D) )
 *   U  = ((h >> 9) + 0.5) * 2^-23          exact in fp32; 23 hash bits reach U
 *   g  = -log(-log(U))                      fp32
 * U lies in [2^-24, 1 - 2^-24], strictly inside (0, 1) for every h, so g is finite for every element: g ranges over
 * [g_min, g_max] = [-log(24 log 2), -log(-log(1 - 2^-24))] = [-2.8116, 16.6355].  The resolution bounds what can be drawn:
 * an item whose z lies more than g_max - g_min = 19.447 below the user's best z (softmax odds against the best item
 * below exp(-19.447) = 3.6e-9) is never drawn ahead of it.  A perturbed value is clamped to the finite fp32 range, so it
 * never carries the exclusion sentinel's bits.
 * Consequences: the same arguments and seed give the same bits; the first j columns of a call with k are the call with
 * j; a user's row depends on (seed, its key, its model-side rows and exclusion) only, not on the batch it sits in; under
 * a candidate list S the result is the unrestricted perturbed order with the items outside S struck out; no split of
 * the selection or of the perturb pass changes a bit (logsumexp is summed per fixed 1024-column chunk in 64-bit fixed
 * point and merged in a fixed shape).  No atomics.
 * Launches behind carca_recommend's scoring and exclusion: the perturb pass on grid (B, S), carca_retrieve's selection,
 * a finishing launch on grid (B).  Stream scratch (or the capture's memory): a SECOND [B, n_items] ([B, n] under a list)
 * fp32 buffer beside carca_recommend's, plus 8 bytes per user and 1024 columns -- 512 MB more at 1 M items x 128 users.
 * Errors as carca_retrieve with "recommend_sampled" in the message; CARCA_ERR_BADARG also for a null sampling block, a
 * temperature that is not a finite, positive, normal fp32 number (below FLT_MIN = 1.18e-38 the division would overflow),
 * null log_probs or ld_log_probs < k. */
typedef struct CarcaSampling {
  float temperature;         /* finite, >= FLT_MIN */
  uint64_t seed;
  const int64_t* user_keys;  /* [B] on the device, or NULL: user u's key is u */
  float* log_probs;          /* [B, ld_log_probs], first k columns written */
  int ld_log_probs;
} CarcaSampling;
int carca_recommend_sampled(const CarcaRecommendDesc* desc, const CarcaCandidates* candidates /* nullable */,
                            const CarcaSampling* sampling, void* stream);
/* The perturb pass of carca_recommend_sampled alone, over buffers the caller holds (a measurement hook: tools/
 * bench_sampled.py times it against its bytes): perturbed[u][i] = logits[u][i] / temperature + g(seed, key of u, item i), the
 * exclusion sentinel (bits 0xFFFFFFFF) copied through, and per user and 1024-column chunk (max z, sum exp(z - max)) over the
 * other columns into partials.  logits, perturbed: [B, n_slots] fp32 with row stride n_slots, 16-byte aligned; partials:
 * [B, ceil(n_slots / 1024), 2] fp32.  Of the sampling block temperature, seed and user_keys are read.  CARCA_ERR_BADARG for
 * null pointers, B or n_slots < 1, a bad temperature or a misaligned buffer. */
int carca_sampled_perturb(const float* logits, float* perturbed, float* partials, int B, int n_slots,
                          const CarcaSampling* sampling, void* stream);

/* ---- a sampling policy's log-probabilities for listed items: the numerator of an off-policy estimator (DESIGN.md
 * section 28) --------------------------------------------------------------------------------------------------------
 * carca_log_prob_items returns, for a list of n_list item ids per user, each item's log-probability under
 * softmax(logit / temperature) over the user's eligible items -- the distribution carca_recommend_sampled draws from --
 * and that softmax's logsumexp and entropy per user.  The descriptor and the (nullable) candidate list are
 * carca_recommend_sampled's; its k, scores and ids_out are NOT read.  Eligibility is carca_recommend's (id != 0, not in
 * exclude, inside the candidate list when one is given).  With z = logit / temperature (one fp32 division):
 *   lse[u]          logsumexp of z over user u's eligible items; -inf when there is none;
 *   log_probs[u][j] z - lse[u] when items[u][j] is eligible for u; exactly -inf otherwise: id 0, an excluded id, an id
 *                   outside the candidate list, a negative id, an id >= n_items.  The id is compared as an int64, so
 *                   2^40 does not wrap into range.  The list may be in any order and repeat ids; n_list = 0 is allowed
 *                   (lse and entropy are still written);
 *   entropy[u]      -sum_i p_i log p_i over the eligible items, in nats; 0 when there is none.  exp(entropy) is the
 *                   effective number of items the policy chooses among.
 * BITS.  For the ids carca_recommend_sampled returned under the same descriptor, candidate list and temperature,
 * log_probs equals that call's log_probs bit for bit (padding, id 0, is -inf on both sides): scoring and exclusion are
 * the same launches, the chunk partials come from the SAME device code as the perturb pass's (csrc/sampled_select.h:
 * sp_z, sp_chunk_sums), and they merge in the same shape.  A user's row, lse and entropy depend on that user's
 * model-side rows, exclusion and list entry only: not on the batch, on the order of the list, or on the row split S
 * (tuning key 24).  Per fixed 1024-column chunk: an exact maximum, sum exp(z - max) and the entropy partial
 * sum exp(z - max) (max - z) in 64-bit fixed point, units of 2^-32 (each entropy term is at most 2^32 / e); thread t of
 * the finishing launch folds chunks t, t + 256, ..., then a fixed tree over 256 threads; with (m, s, w) the running
 * maximum, sum and entropy partial, w' = (w + s (M - m)) e^(m - M) + (pw + ps (M - pm)) e^(pm - M) and
 * entropy = max(log s + w / s, 0).  No atomics.
 * Launches behind carca_recommend's scoring and exclusion: the reduce pass on grid (B, S), S as the perturb pass's, and a
 * finishing launch on grid (B).  Stream scratch (or the capture's memory): carca_recommend's [B, n_items] ([B, n] under a
 * list) fp32 buffer plus 12 bytes per user and 1024 columns -- no second buffer, half of carca_recommend_sampled's.
 * Errors as carca_recommend_sampled with "log_prob_items" in the message; CARCA_ERR_BADARG for a null policy block, a
 * temperature that is not a finite, positive, normal fp32 number, n_list < 0, null items or log_probs with n_list > 0,
 * ld_items or ld_log_probs < n_list.  z must stay finite: |logit| / temperature below FLT_MAX. */
typedef struct CarcaPolicyItems {
  float temperature;     /* finite, >= FLT_MIN */
  const int64_t* items;  /* [B, ld_items] on the device, the first n_list columns read */
  int n_list;
  int ld_items;
  float* log_probs;      /* [B, ld_log_probs], the first n_list columns written */
  int ld_log_probs;
  float* lse;            /* [B], or NULL: not written */
  float* entropy;        /* [B], or NULL: not written */
} CarcaPolicyItems;
int carca_log_prob_items(const CarcaRecommendDesc* desc, const CarcaCandidates* candidates /* nullable */,
                         const CarcaPolicyItems* policy, void* stream);
/* The reduce pass of carca_log_prob_items alone, over a buffer the caller holds (a measurement hook: tools/bench_policy.py
 * times it against its bytes, beside carca_sampled_perturb on the same buffer): per user and 1024-column chunk (max z,
 * sum exp(z - max), sum exp(z - max) (max - z)) over the columns that do not hold the exclusion sentinel (bits
 * 0xFFFFFFFF), z = logits / temperature.  logits: [B, n_slots] fp32 with row stride n_slots, 16-byte aligned, only read;
 * partials: [B, ceil(n_slots / 1024), 3] fp32.  The first two of a chunk's three values are carca_sampled_perturb's pair,
 * bit for bit.  CARCA_ERR_BADARG for null pointers, B or n_slots < 1, a bad temperature or a misaligned buffer. */
int carca_policy_reduce(const float* logits, float* partials, int B, int n_slots, float temperature, void* stream);

/* ---- item groups: the k best of EVERY group in one call, and the k best overall with at most m per group (a page of
 * carousels; "at most two per brand") ----------------------------------------------------------
 * CarcaItemGroups labels items with one of n_groups groups (category, brand, shelf); an item may carry no label and is
 * then never returned.  All arrays int32 on the device, the caller's contract:
 *   order   [n]            the grouped ids, sorted by (group, id): every id in [1, n_items), distinct;
 *   offsets [n_groups + 1] group g owns positions [offsets[g], offsets[g + 1]) of order; nondecreasing, offsets[0] = 0,
 *                          offsets[n_groups] = n; an empty group is legal;
 *   pos_of  [n_items]      the position of an id in order, -1 where it has none (n_items is the descriptor's).
 * A bound of offsets outside [0, n], or an entry of pos_of outside [-1, n), is clamped or ignored and never used as an
 * index.  The descriptor is carca_recommend's own.  The catalogue is swept ONCE, in the grouped order, by
 * carca_recommend_among's scoring launch (the logit of a (user, item) pair does not depend on the position that holds
 * the item: the same bits), into stream scratch [B, n]; the exclusion launch finds an id's position in pos_of.
 *
 * carca_recommend_groups: per (user, group) the k best items of the group minus the excluded ids, in carca_recommend's
 * order (logit descending, ties to the smaller id), padded with id 0 and score 0 -- list (u, g) is bit for bit row u of
 * carca_recommend_among over group g's slice of order.  scores / ids_out: row u holds the n_groups lists side by side,
 * scores[u][g * k + j] (ld_scores, ld_ids_out >= n_groups * k).  One selection launch, grid (B, n_groups).
 *
 * carca_recommend_capped: per user carca_recommend's order over the grouped, non-excluded items walked from the best,
 * skipping an item once max_per_group items of its group are in the list, until k are taken; ties go to the smaller id
 * across groups too; padding as carca_recommend; max_per_group >= k: no cap.  scores / ids_out [B, k].  Two launches behind
 * the exclusion: every group's best m = min(k, max_per_group) as 64-bit keys on the item id, [B, n_groups, m] uint64 of
 * stream scratch, then per user the k largest of them.
 *
 * Bit-identical run to run.  Limits and errors as carca_recommend, and CARCA_ERR_UNSUPPORTED for n_groups > 65535 or a key
 * scratch B * n_groups * m * 8 beyond 1 GiB; CARCA_ERR_BADARG for null groups or arrays, n_groups < 1, n outside
 * [0, n_items) or max_per_group < 1. */
typedef struct CarcaItemGroups {
  const int32_t* order;   /* [n] */
  const int32_t* offsets; /* [n_groups + 1] */
  const int32_t* pos_of;  /* [n_items] */
  int n;                  /* grouped items */
  int n_groups;
} CarcaItemGroups;
int carca_recommend_groups(const CarcaRecommendDesc* desc, const CarcaItemGroups* groups, void* stream);
int carca_recommend_capped(const CarcaRecommendDesc* desc, const CarcaItemGroups* groups, int max_per_group, void* stream);

/* ---- the k best USERS per listed item ("which k users should hear about each of these Q items": a campaign, new
 * arrivals, overstock) ---------------------------------------------------------------------------
 * The descriptor is carca_recommend's own (scores / ld_scores / ids_out / ld_ids_out are not read and may be null; k is
 * the audience size), `items` a CarcaCandidates of Q ascending, distinct ids.  CarcaAudience is the running result, one row
 * of k 64-bit keys per listed item, best first:
 *   key = (order-preserving bits of the raw logit) << 32 | (0xFFFFFFFF - user id); 0 = no entry.
 * A larger key is a larger logit, and between equal logits the smaller user id; keys of a row are distinct as long as no
 * user id is fed twice (a repeated id is the caller's error: both entries count).  Row u of the batch is user
 * user_ids[u], or user_base + u where user_ids is null; a negative user id drops the row.  User u is not eligible for
 * item i where the exclusion list of row u holds i (the descriptor's exclude, as carca_recommend's).
 *
 * carca_recommend_users: scores the B users against the Q items with carca_recommend_among's scoring and exclusion
 * launches (stream scratch [B, Q]; the logit of a pair is bit-identical to carca_recommend's) and merges them into the
 * state: afterwards row q holds the k largest keys of its old keys and the batch's eligible users, descending, zeros
 * last.  The caller zeroes the state before the first call and must have the rows sorted as this call leaves them.
 * Because the keys are distinct and totally ordered, the state after a sequence of calls depends only on the set of
 * (user, logit) pairs fed -- not on how the users were split into calls, nor on the order of the calls.  One merge launch
 * behind the two shared ones (a workgroup per 16 adjacent items walks the users; integer LDS atomics only), no host wait.
 * Q = 0 is legal and launches nothing.
 *
 * carca_audience_read: keys [n_rows, ld_keys] -> scores [n_rows, k] = sigmoid(logit) ((logit + 1) / 2 for decoder 2) --
 * carca_recommend's score of that (user, item), bit for bit -- and users [n_rows, k]; an empty entry gives score 0 and
 * user -1.  Both outputs are dense.
 *
 * Limits and errors as carca_recommend (L up to CARCA_MAX_PROFILE_L, 1 <= k <= 128), and CARCA_ERR_UNSUPPORTED for
 * B * Q (n_rows * k) of 2^31 or more; CARCA_ERR_BADARG for a null list / state / keys, ld_keys < k, or a user_base that
 * lets a row id reach 2^31. */
typedef struct CarcaAudience {
  unsigned long long* keys; /* [Q, ld_keys], the first k of a row used */
  int ld_keys;
  const int32_t* user_ids;  /* [B], or NULL: row u is user user_base + u */
  int user_base;
} CarcaAudience;
int carca_recommend_users(const CarcaRecommendDesc* desc, const CarcaCandidates* items, const CarcaAudience* state,
                          void* stream);
int carca_audience_read(const unsigned long long* keys, int ld_keys, int n_rows, int k, int decoder, float* scores,
                        int64_t* users, void* stream);

/* ---- a candidate list of its own per user (the second stage behind a retriever; the evaluation protocol's 1 + 100
 * candidates, data.py:180-185) ---------------------------------------------------------------
 * The model-side fields (B .. ffn_b), k and the exclusion list mean exactly what they mean in CarcaRecommendDesc, and the
 * logit of a (user, item) pair is bit-identical to carca_recommend's.  items [B, ld_items] int32, the first n_list
 * columns read, n_list >= 1: user u's own list, in any order, duplicates allowed; an id of 0 or outside [1, n_items) is
 * no item and is never read out of bounds.  The user is staged once per workgroup and the list streams past it.
 *
 * carca_score_lists: scores[u][j] = sigmoid(logit) ((logit + 1) / 2 for decoder 2) of (u, items[u][j]), 0 where the id
 * is no item; caller order, duplicates each scored, no exclusion (k, exclude, ids_out and sorted_rows are not read).
 * One launch, no scratch, any n_list.
 *
 * carca_recommend_lists: per user the k best among the DISTINCT items of its row minus the excluded ids, in
 * carca_recommend's order (logit descending, ties to the smaller id), padded with id 0 and score 0 -- row u is what
 * carca_recommend_among gives user u alone with the distinct items of items[u] as the candidate list, bit for bit.
 *   sorted_rows == 0: n_list <= 1024, rows in any order; one launch, one workgroup per user, no scratch (the keys of a
 *                     row are sorted in LDS, and a repeated id's equal keys are dropped there);
 *   sorted_rows != 0: the caller's contract is that every row is NONDECREASING (repeats side by side; ids that are no
 *                     items at the two ends); any n_list.  Raw logits [B, n_list] go to stream scratch (or the capture's
 *                     memory) by position, then carca_recommend's exclusion and selection launches run per row.
 * Bit-identical run to run, and between the two forms.  Limits (L up to CARCA_MAX_PROFILE_L, k <= 128) and errors as
 * carca_recommend, and CARCA_ERR_UNSUPPORTED for n_list > 1024 without sorted_rows, CARCA_ERR_BADARG for a null list,
 * n_list < 1 or strides shorter than a row. */
typedef struct CarcaListsDesc {
  int B, L, n_items, d, H, k;
  int decoder;          /* 0 cross-attention, 1 dot, 2 normalised dot */
  const int32_t* p_ids; /* [B, ld_p_ids] profile ids */
  int ld_p_ids;
  const float* item_q; /* [n_items, ld_item_q] */
  int ld_item_q;
  const float* item_w; /* [n_items] with stride ld_item_w, or NULL */
  int ld_item_w;
  const float* user_k; /* [B*L, ld_user_k] */
  int ld_user_k;
  const float* user_u; /* [B*L, ld_user_u] */
  int ld_user_u;
  const float* user_q; /* [B, ld_user_q] (decoder 0: may be NULL) */
  int ld_user_q;
  const float* user_m; /* [B, ld_user_m] or NULL */
  int ld_user_m;
  const float* user_off; /* [B] with stride ld_user_off, or NULL */
  int ld_user_off;
  const float* ffn_b; /* float[1] or NULL */
  const int32_t* exclude; /* [B, ld_exclude], first n_exclude columns read */
  int n_exclude, ld_exclude;
  const int32_t* items; /* [B, ld_items], first n_list columns: each user's own list */
  int n_list, ld_items;
  int sorted_rows; /* carca_recommend_lists: every row is nondecreasing */
  float* scores; /* [B, ld_scores]: n_list columns (carca_score_lists) or k (carca_recommend_lists) */
  int ld_scores;
  int64_t* ids_out; /* [B, ld_ids_out] (carca_recommend_lists) */
  int ld_ids_out;
} CarcaListsDesc;
int carca_score_lists(const CarcaListsDesc* desc, void* stream);
int carca_recommend_lists(const CarcaListsDesc* desc, void* stream);

/* ---- several request contexts per user ("tonight, tomorrow morning, at the weekend"; "at which of these send times
 * does item i score best for user u") -----------------------------------------------------------
 * The candidate's context (data.py:180-185: every candidate of a user carries the request's context) enters a logit only
 * through the rows M c: for decoder 0 through user_q = (M c) W_Q^T (the score bias beta_hl = user_q_h . K_hl) and
 * user_off = w_ffn . M c (carca.py:338-347 over e = T[i] + M c), for decoders 1 and 2 through user_m = M c
 * (carca.py:361-367, 385-399).  K, u, the scored profile row and the head dot products item_q[i]_h . K_hl do not depend
 * on it.  CarcaContexts carries those rows for n_contexts = C >= 1 contexts per user: row u * C + c belongs to (user u,
 * context c).  The entry points below take an existing descriptor plus this struct; the descriptor's own user_q (decoder
 * 0), user_off and user_m are then NOT read (decoder 1 / 2: the descriptor's user_q is the scored profile row, as
 * always).  A null row pointer means "no context term", as in the descriptor.  The profile is staged once per
 * workgroup, the head dot product of a (head, slot, item) is computed once, and the contexts are served eight at a time
 * (fewer where a geometry's registers ask for it); C is not capped.  The logit of (user u under context c, item i) is
 * bit-identical to the one carca_recommend / carca_score_lists compute from a descriptor that holds row u * C + c as
 * user u's row.  Decoder 0 needs L <= CARCA_MAX_L here (the chunked protocol of longer profiles is not served under
 * several contexts).  No float atomics: bit-identical run to run.
 *
 * carca_score_lists_at: carca_score_lists under each context.  best_context == NULL: scores[u][c * n_list + j] is
 * carca_score_lists' scores[u][j] under context c (ld_scores >= C * n_list).  best_context != NULL ([B, ld_best_context]
 * int64): no [B, C, n_list] result is formed; scores[u][j] (ld_scores >= n_list) is the link of the largest LOGIT of
 * entry j over the C contexts and best_context[u][j] its context, a tie going to the smaller context index; an id that is
 * no item gives score 0 and context -1.  One launch, no scratch.
 *
 * carca_recommend_at / carca_recommend_among_at: carca_recommend / carca_recommend_among under each context:
 * scores[u][c * k + r] and ids_out[u][c * k + r], r < k, are row u of the single-context call under context c.  The two
 * outputs are dense: ld_scores == ld_ids_out == C * k.  desc->exclude has B * C rows, row u * C + c for (user u, context
 * c): the caller repeats a user's row for each of its contexts.  The sweep writes raw logits [B * C, n] (n = n_items or
 * the candidate count) to stream scratch, or the capture's memory; then carca_recommend's exclusion and selection
 * launches run over the B * C rows.  Three launches, no host wait.
 *
 * CARCA_ERR_UNSUPPORTED as the single-context calls, and decoder 0 with L > CARCA_MAX_L, or B * C (C * n_list, C * k) of
 * 2^31 or more.  CARCA_ERR_BADARG as the single-context calls, and a null CarcaContexts, n_contexts < 1, a context row
 * stride shorter than its row or (user_q, user_m) not a multiple of 4, ld_scores / ld_best_context shorter than their
 * rows, or (recommend) output strides other than C * k. */
typedef struct CarcaContexts {
  int n_contexts;        /* C >= 1 */
  const float* user_q;   /* [B * C, ld_user_q] (M c) W_Q^T, read by decoder 0, or NULL */
  int ld_user_q;
  const float* user_off; /* [B * C] with stride ld_user_off: w_ffn . M c, read by decoder 0, or NULL */
  int ld_user_off;
  const float* user_m;   /* [B * C, ld_user_m] M c, read by decoders 1 and 2, or NULL */
  int ld_user_m;
} CarcaContexts;
int carca_score_lists_at(const CarcaListsDesc* desc, const CarcaContexts* contexts, int64_t* best_context,
                         int ld_best_context, void* stream);
int carca_recommend_at(const CarcaRecommendDesc* desc, const CarcaContexts* contexts, void* stream);
int carca_recommend_among_at(const CarcaRecommendDesc* desc, const CarcaContexts* contexts,
                             const CarcaCandidates* candidates, void* stream);

/* ---- which profile slots drive a cross-attention score (the decoder's attention, MultiHeadAttention.forward's
 * return_w, carca.py:253-263, under CrossAttentionBlock.forward's eval path, carca.py:338-347) ---
 * The model-side fields (B .. ffn_b) and the list (items / n_list / ld_items) mean exactly what they mean in
 * CarcaListsDesc; k and the exclusion list are carried so that one model side fills both and are not read.  decoder must
 * be 0: a dot decoder's eval score reads the last profile slot only (carca.py:362).  For user u and list entry j, with
 * id = items[u][j], over the user's valid slots t (p_ids[u][t] != 0):
 *   w_h(t)   = softmax over the valid slots of (q_h(id) + dq_h(u)) . K_h[u][t] / sqrt(d / H): head h's attention weight;
 *   c(t)     = sum_h w_h(t) * user_u[u * L + t][h], heads in ascending order;
 *   base     = item_w[id] + user_off[u] + ffn_b[0] (the terms that are given);
 *   logit    = base + sum_t c(t), and scores[u][j] = sigmoid(logit) with carca_score_lists' bits.
 * An id of 0 or outside [1, n_items) is no item: score 0, base 0, every weight and contribution 0, never read out of
 * bounds.  A padding slot (interior ones included) and every slot of an empty profile has weight and contribution 0
 * (carca.py:256).  Which outputs are given selects the form:
 *   weights != NULL (dense): contrib [B, n_list, ld_contrib] and weights [B, H, n_list, ld_weights], the first L columns
 *                     of every row written, padding positions as 0 (no memset needed); slots and slot_items NULL;
 *   slots != NULL (top_m):  per (u, j) the top_m valid slots with the largest c, descending, ties to the LATER slot:
 *                     slots [B, n_list, ld_slots] their positions in [0, L), slot_items [B, n_list, ld_slot_items] the
 *                     profile ids there, contrib [B, n_list, ld_contrib] their c -- bit for bit the dense form's
 *                     entries; fewer than top_m valid slots, and an id that is no item, pad with slot -1, item 0 and
 *                     contribution 0.  1 <= top_m <= 8.  No [B, n_list, L] buffer exists; weights NULL.
 * One launch, the user staged once per workgroup, two passes over the staged slots per entry; no atomics, no scratch,
 * bit-identical run to run.  L up to CARCA_MAX_PROFILE_L as carca_score_lists.  CARCA_ERR_UNSUPPORTED as
 * carca_score_lists, and a decoder other than 0 or top_m outside 1..8.  CARCA_ERR_BADARG as carca_score_lists, and null
 * outputs, both forms or neither, or strides shorter than a row. */
typedef struct CarcaExplainDesc {
  int B, L, n_items, d, H, k;
  int decoder;          /* 0 cross-attention (the only one served) */
  const int32_t* p_ids; /* [B, ld_p_ids] profile ids */
  int ld_p_ids;
  const float* item_q; /* [n_items, ld_item_q] */
  int ld_item_q;
  const float* item_w; /* [n_items] with stride ld_item_w, or NULL */
  int ld_item_w;
  const float* user_k; /* [B*L, ld_user_k] */
  int ld_user_k;
  const float* user_u; /* [B*L, ld_user_u] */
  int ld_user_u;
  const float* user_q; /* [B, ld_user_q] (may be NULL) */
  int ld_user_q;
  const float* user_m; /* not read */
  int ld_user_m;
  const float* user_off; /* [B] with stride ld_user_off, or NULL */
  int ld_user_off;
  const float* ffn_b; /* float[1] or NULL */
  const int32_t* exclude; /* not read */
  int n_exclude, ld_exclude;
  const int32_t* items; /* [B, ld_items], first n_list columns: each user's own list */
  int n_list, ld_items;
  float* scores; /* [B, ld_scores] */
  int ld_scores;
  float* base; /* [B, ld_base] */
  int ld_base;
  float* contrib; /* dense: [B, n_list, ld_contrib], L columns; top_m: [B, n_list, ld_contrib], top_m columns */
  int ld_contrib;
  float* weights; /* dense: [B, H, n_list, ld_weights], L columns; else NULL */
  int ld_weights;
  int64_t* slots; /* top_m: [B, n_list, ld_slots]; else NULL */
  int ld_slots;
  int64_t* slot_items; /* top_m: [B, n_list, ld_slot_items]; else NULL */
  int ld_slot_items;
  int top_m;
} CarcaExplainDesc;
int carca_explain_lists(const CarcaExplainDesc* desc, void* stream);

/* ---- KNN baseline: full-catalogue top-k and exact ranks (replace KNN.forward over the catalogue as target groups:
 * knn.py:13-19 over the candidate lists of data.py:180-185, ranked as train.py:15-32 does) ------
 * The catalogue is the rows of the attribute table [n_items, ld_table] (fp32, F features).  For user u and item i >= 1:
 *   logit = q_u . table[i] over the F features, no link (KNN.forward's raw score);
 *   q_u   = user_a[u] (dense mode: the last profile slot's attribute row, [B, ld_user_a]) when user_a is given, else
 *           table[p_ids[u][L-1]] (table mode), a zero row when that id is outside [0, n_items).
 * Scoring is one users x items GEMM in fp32 MFMA (exact fp32 products, fp32 sums).  With table_i8 (table mode only) it
 * runs in i8 MFMA with i32 sums over that int8 copy of the table, [n_items, ld_table_i8], ld_table_i8 a multiple of 64.
 * The caller passes it only for a table whose entries are all integers with max|x| <= 127 and max|x|^2 * F < 2^24:
 * every partial sum is then an exact integer, so both variants give the same bits.  Logits of the B x n_items pairs live
 * in stream scratch (or the capture's memory); no host wait, nothing retained; bit-identical run to run.
 * CARCA_ERR_UNSUPPORTED: B > 65535, F > 2^22, k or n_list outside 1..128.  CARCA_ERR_BADARG: null pointers, strides
 * shorter than a row, ld_table > 2^24, table_i8 with user_a or with a bad ld_table_i8.
 *
 * carca_knn_recommend: the k best items per user, best first, in carca_recommend's order (logit descending, ties to the
 * smaller id): ids_out [B, k] int64 and scores = the logits.  Id 0 and the nonzero entries of exclude [B, n_exclude]
 * (int32, 0 = no entry, duplicates allowed) are never selected; fewer than k eligible items pad with id 0 and score 0.
 * Shares carca_recommend's exclusion and selection launches. */
typedef struct CarcaKnnRecommendDesc {
  int B, L, n_items, F, k;
  const int32_t* p_ids; /* [B, ld_p_ids] profile ids (table mode) */
  int ld_p_ids;
  const float* user_a; /* [B, ld_user_a] query rows, or NULL (table mode) */
  int64_t ld_user_a;
  const float* table; /* [n_items, ld_table] */
  int ld_table;
  const int8_t* table_i8; /* [n_items, ld_table_i8] or NULL */
  int ld_table_i8;
  const int32_t* exclude; /* [B, ld_exclude], first n_exclude columns read */
  int n_exclude, ld_exclude;
  float* scores; /* [B, ld_scores] */
  int ld_scores;
  int64_t* ids_out; /* [B, ld_ids_out] */
  int ld_ids_out;
} CarcaKnnRecommendDesc;
int carca_knn_recommend(const CarcaKnnRecommendDesc* desc, void* stream);
/* carca_knn_retrieve: carca_knn_recommend in depth, 1 <= k <= 4096, with carca_retrieve's contract (above): the order is
 * logit descending with ties to the smaller id, id 0 and the excluded ids are never returned, fewer than k eligible items
 * pad with id 0 and score 0; the first j columns of a call with k are the call with j bit for bit, and for k <= 128 both
 * outputs are carca_knn_recommend's; scores = the logits, with carca_knn_recommend's / carca_knn_rank_items' bits (the
 * query, scoring and exclusion launches are carca_knn_recommend's); keys are (order bits, complemented id); ids_out is
 * int64.  Selection is carca_retrieve's two launches (one where S = 1), bit-identical for every S and run to run.
 * Errors as carca_knn_recommend, with CARCA_ERR_UNSUPPORTED for k outside 1..4096. */
int carca_knn_retrieve(const CarcaKnnRecommendDesc* desc, void* stream);
/* carca_knn_recommend_sampled: carca_recommend_sampled (above) over the KNN descriptor, 1 <= k <= 4096: the query, scoring
 * and exclusion launches are carca_knn_recommend's, scores = the raw logits with its bits (no link), and the noise
 * contract, log_probs, padding and consequences are carca_recommend_sampled's.  The logit buffer's columns are item ids;
 * a (nullable) candidate list strikes the items outside it out in the perturb pass, so time and scratch follow n_items. */
int carca_knn_recommend_sampled(const CarcaKnnRecommendDesc* desc, const CarcaCandidates* candidates /* nullable */,
                                const CarcaSampling* sampling, void* stream);
/* carca_knn_log_prob_items: carca_log_prob_items (above) over the KNN descriptor, whose k, scores and ids_out are not
 * read: the query, scoring and exclusion launches are carca_knn_recommend_sampled's, so for the ids that call returned
 * log_probs equals its log_probs bit for bit.  The logit buffer's columns are item ids; a (nullable) candidate list
 * strikes the items outside it out in the reduce pass and in the lookup, so time and scratch follow n_items. */
int carca_knn_log_prob_items(const CarcaKnnRecommendDesc* desc, const CarcaCandidates* candidates /* nullable */,
                             const CarcaPolicyItems* policy, void* stream);

/* carca_knn_rank_items: for user u and list entry j, with id = items[u][j]:
 *   ranks[u][j]  = number of ELIGIBLE items (id != 0, not excluded) that order strictly before id in
 *                  carca_knn_recommend's order; an excluded or repeated id still gets the position it would take;
 *   scores[u][j] = the logit, bit-identical to carca_knn_recommend's;
 *   id 0 or an id outside [0, n_items): rank -1 and score 0 (never read out of bounds).
 * The model-side fields and the exclusion list are carca_knn_recommend's, and so is the scoring launch; the listed
 * items' keys are read from its logits, then a sweep counts per (user, target) the items ordering before the target
 * with integer atomics. */
typedef struct CarcaKnnRankDesc {
  int B, L, n_items, F;
  const int32_t* p_ids;
  int ld_p_ids;
  const float* user_a;
  int64_t ld_user_a;
  const float* table;
  int ld_table;
  const int8_t* table_i8;
  int ld_table_i8;
  const int32_t* exclude;
  int n_exclude, ld_exclude;
  const int32_t* items; /* [B, ld_items], first n_list columns: the items to rank */
  int n_list, ld_items;
  float* scores; /* [B, ld_scores] */
  int ld_scores;
  int64_t* ranks; /* [B, ld_ranks] */
  int ld_ranks;
} CarcaKnnRankDesc;
int carca_knn_rank_items(const CarcaKnnRankDesc* desc, void* stream);

/* ---- full-catalogue softmax cross-entropy for the dot decoders ------------------------------
 * P [R, ld_p] profile rows, T [n_items, ld_t] catalogue rows (d features; ld_p, ld_t multiples of 4, bases 16-byte
 * aligned), pos [R] int32.  Row r is VALID iff pos[r] lies in [1, n_items); id 0 is never a class.
 *   carca_catalogue_xent_fwd: lse[r] = log sum_{i=1..n_items-1} exp(P[r] . T[i]), row_loss[r] = lse[r] - P[r] . T[pos[r]]
 *     (both 0 for a row that is not valid), loss[0] = sum of row_loss / n_valid (0 when no row is valid);
 *   carca_catalogue_xent_bwd: with lse from the forward and the upstream scale grad[0], G = softmax - onehot(pos):
 *     dP = grad / n_valid * G T  (0 for rows that are not valid and for the columns past d),
 *     dT = grad / n_valid * G^T P (row 0 and the columns past d: 0).
 * Products in exact-fp32 MFMA; the logit tiles are recomputed, never stored.  n_valid and the list of valid rows are
 * found on the device (no host wait).  The item range is split over splits_items workgroup columns of items_per_split
 * items (a multiple of 64); the backward's dT splits the valid rows over splits_rows.  Scratch (scratch_floats 4-byte
 * words, caller-allocated; ops.catalogue_xent_plan gives the size): 2 ceil64(R) + 64 words of row lists, then the
 * forward's 2 ceil64(splits_items R) (max, sum-exp) partials, or the backward's ceil64(splits_items R ld) dP partials and,
 * with splits_rows > 1, ceil64(splits_rows n_items ld) dT partials, ld = round_up(d, 4).  No float atomics: the same call
 * gives the same bits.  CARCA_ERR_UNSUPPORTED: d > 256.  CARCA_ERR_BADARG: null pointers, strides, split counts outside
 * 1..256, items_per_split * splits_items < n_items, scratch too small. */
typedef struct CarcaCatalogueXentDesc {
  int R, n_items, d;
  const float* P;
  int ld_p;
  const float* T;
  int ld_t;
  const int32_t* pos;
  int splits_items, items_per_split, splits_rows;
  float* scratch;
  int64_t scratch_floats;
  float* lse;      /* [R]: forward output, backward input */
  float* row_loss; /* [R] forward */
  float* loss;     /* [1] forward */
  const float* grad; /* [1] backward: upstream scale of loss */
  float* dP;       /* [R, ld_p] backward */
  float* dT;       /* [n_items, ld_t] backward */
} CarcaCatalogueXentDesc;
int carca_catalogue_xent_fwd(const CarcaCatalogueXentDesc* desc, void* stream);
int carca_catalogue_xent_bwd(const CarcaCatalogueXentDesc* desc, void* stream);

/* ---- row log-softmax with a temperature and per-row exclusion, forward and backward ---------
 * The differentiable log-probability of a served policy.  P, T, the strides, the splits and the scratch's first part as
 * for carca_catalogue_xent (ops.policy_xent_plan gives the sizes).  items [R] int32; excl [R, n_excl] int32, each row
 * ASCENDING (any values: entries outside [1, n_items) exclude nothing; duplicates allowed), null with n_excl = 0.
 * With z[r, i] = P[r] . T[i] / temperature: class i of row r is eligible iff 1 <= i < n_items and i is not in excl[r];
 * row r is VALID iff items[r] is an eligible class of r.
 *   carca_policy_xent_fwd: lse[r] = logsumexp of z[r, .] over the eligible classes, log_prob[r] = z[r, items[r]] - lse[r],
 *     entropy[r] = -sum p log p over the eligible classes (only when the pointer is given), valid[r] = 1 / 0; lse,
 *     log_prob and entropy are exactly 0 on rows that are not valid.  The forward's scratch holds one more
 *     ceil64(splits_items R) words when entropy is given.
 *   carca_policy_xent_bwd: with lse (and entropy, when h is given) from the forward, c[r] = dL/dlog_prob[r] and
 *     h[r] = dL/dentropy[r] (null: none):
 *     dz[r, i] = (c[r] (1[i = items[r]] - p[r, i]) - h[r] p[r, i] (log p[r, i] + entropy[r])) / temperature on the eligible
 *     (r, i) of valid rows, 0 elsewhere;  dP = dz T (rows that are not valid and columns past d: 0), dT = dz^T P (row 0 and
 *     columns past d: 0).  No division by n_valid and no scalar scale: c and h carry all of it.  With n_excl > 0 the
 *     backward also takes the lists transposed: t_off [n_items + 1] offsets into t_rows, which holds for each item the
 *     ascending VALID-ROW indices (the rank of a row among the valid rows, in row order) of the valid rows whose list names
 *     it; only items in [1, n_items) are read.
 * Products in exact-fp32 MFMA; the logit tiles are recomputed, never stored; no float atomics: the same call gives the
 * same bits.  CARCA_ERR_UNSUPPORTED: d > 256, R n_excl >= 2^31.  CARCA_ERR_BADARG: as carca_catalogue_xent, a temperature
 * that is not a finite number > 0, h without entropy, n_excl > 0 without the lists. */
typedef struct CarcaPolicyXentDesc {
  int R, n_items, d;
  const float* P;
  int ld_p;
  const float* T;
  int ld_t;
  const int32_t* items;
  float temperature;
  const int32_t* excl; /* [R, n_excl] ascending rows, or null */
  int n_excl;
  const int32_t* t_off;  /* backward with n_excl > 0: [n_items + 1] */
  const int32_t* t_rows; /* backward with n_excl > 0 */
  int splits_items, items_per_split, splits_rows;
  float* scratch;
  int64_t scratch_floats;
  float* lse;      /* [R]: forward output, backward input */
  float* log_prob; /* [R] forward */
  float* entropy;  /* [R] or null: forward output, backward input with h */
  uint8_t* valid;  /* [R] forward */
  const float* c;  /* [R] backward */
  const float* h;  /* [R] or null, backward */
  float* dP;       /* [R, ld_p] backward */
  float* dT;       /* [n_items, ld_t] backward */
} CarcaPolicyXentDesc;
int carca_policy_xent_fwd(const CarcaPolicyXentDesc* desc, void* stream);
int carca_policy_xent_bwd(const CarcaPolicyXentDesc* desc, void* stream);

/* ---- sampled softmax cross-entropy with the logQ correction for the dot decoders ------------
 * P [R, ld_p] profile rows, Tp [R, ld_tp] the rows of their positives, S [K, ld_s] the rows of K samples shared by every
 * row (d features; ld_p, ld_tp, ld_s multiples of 4; P and S 16-byte aligned), pos [R] and s_ids [K] int32, bp [R] and
 * bs [K] the logQ corrections -log(K Q(id)).  Row r is VALID iff pos[r] lies in [1, n_items).  Sample k is a negative of
 * row r iff s_ids[k] lies in [1, n_items) and differs from pos[r] (accidental hits removed; duplicates each count).
 *   carca_sampled_xent_fwd: with z'(r, +) = P[r] . Tp[r] + bp[r] and z'(r, k) = P[r] . S[k] + bs[k],
 *     lse[r] = log( exp z'(r, +) + sum over the negatives k of r of exp z'(r, k) ), row_loss[r] = lse[r] - z'(r, +)
 *     (both 0 for a row that is not valid), loss[0] = sum of row_loss / n_valid (0 when no row is valid);
 *   carca_sampled_xent_bwd: with lse and row_loss from the forward and the upstream scale grad[0],
 *     G[r, k] = exp(z'(r, k) - lse[r]) on the negatives (else 0), p_pos = exp(-row_loss[r]):
 *     dP  = grad / n_valid (G S + (p_pos - 1) Tp), dTp = grad / n_valid (p_pos - 1) P  (0 for rows that are not valid),
 *     dS  = grad / n_valid G^T P (0 for samples that are no class); every output 0 past d.
 * Products in exact-fp32 MFMA; the logit tiles are recomputed, never stored.  The samples are split over
 * splits_samples workgroup columns of samples_per_split (a multiple of 64); the backward's dS splits the valid rows over
 * splits_rows.  Scratch (scratch_floats 4-byte words, caller-allocated; ops.sampled_xent_plan gives the size):
 * 2 ceil64(R) + 64 words of row lists, then the forward's 2 ceil64(splits_samples R) (max, sum-exp) partials, or the
 * backward's ceil64((splits_samples + 1) R ld) dP partials and, with splits_rows > 1, ceil64(splits_rows K ld) dS
 * partials, ld = round_up(d, 4).  No float atomics: the same call gives the same bits.  CARCA_ERR_UNSUPPORTED: d > 256.
 * CARCA_ERR_BADARG: null pointers, strides, split counts outside 1..256, samples_per_split * splits_samples < K,
 * scratch too small. */
typedef struct CarcaSampledXentDesc {
  int R, K, n_items, d;
  const float* P;
  int ld_p;
  const float* Tp;
  int ld_tp;
  const float* bp;       /* [R] */
  const int32_t* pos;    /* [R] */
  const float* S;
  int ld_s;
  const int32_t* s_ids;  /* [K] */
  const float* bs;       /* [K] */
  int splits_samples, samples_per_split, splits_rows;
  float* scratch;
  int64_t scratch_floats;
  float* lse;        /* [R]: forward output, backward input */
  float* row_loss;   /* [R]: forward output, backward input */
  float* loss;       /* [1] forward */
  const float* grad; /* [1] backward: upstream scale of loss */
  float* dP;         /* [R, ld_p] backward */
  float* dTp;        /* [R, ld_tp] backward */
  float* dS;         /* [K, ld_s] backward */
} CarcaSampledXentDesc;
int carca_sampled_xent_fwd(const CarcaSampledXentDesc* desc, void* stream);
int carca_sampled_xent_bwd(const CarcaSampledXentDesc* desc, void* stream);

/* ---- softmax cross-entropy over per-list negatives for the dot decoders ----------------------
 * P [R, ld_p] profile rows, Tp [R, ld_tp] the rows of their positives, S [U, ld_s] the embedded rows of the U distinct
 * items of the lists (d features; ld_p, ld_tp, ld_s multiples of 4; P, S and dS 16-byte aligned), pos [R] int32, lists
 * [G, N] int32 item ids, index [G, N] int32 the row of S of each entry (< 0: the entry is no class; any other value is
 * clamped into [0, U) before it is used as an address), bias [G, N] and pos_bias [R] additive corrections or NULL.
 * R = G rows_per_list, rows_per_list in 1..1024: row r reads list g = r / rows_per_list.  Row r is VALID iff pos[r] lies
 * in [1, n_items).  Entry (g, j) is a negative of row r iff index[g][j] >= 0, lists[g][j] lies in [1, n_items) and
 * differs from pos[r] (duplicates each count).
 *   carca_listed_xent_fwd: with z(r, +) = P[r] . Tp[r] + pos_bias[r] and z(r, j) = P[r] . S[index[g][j]] + bias[g][j],
 *     lse[r] = log( exp z(r, +) + sum over the negatives j of r of exp z(r, j) ), row_loss[r] = lse[r] - z(r, +)
 *     (both 0 for a row that is not valid; row_loss 0 for a valid row without a negative), loss[0] = sum of row_loss /
 *     n_valid (0 when no row is valid);
 *   carca_listed_xent_bwd: with lse and row_loss from the forward and the upstream scale grad[0],
 *     G[r, j] = exp(z(r, j) - lse[r]) on the negatives (else 0), p_pos = exp(-row_loss[r]):
 *     dP  = grad / n_valid (sum_j G[r, j] S[index[g][j]] + (p_pos - 1) Tp), dTp = grad / n_valid (p_pos - 1) P  (0 for
 *     rows that are not valid), dS[u] = grad / n_valid sum over the entries (g, j) of item u of E[g][j], E[g][j] = sum
 *     over the rows r of group g of G[r, j] P[r], summed in the order of the by-item CSR: csr_off [U + 1] int32 and
 *     csr_ent int32, csr_ent[csr_off[u] .. csr_off[u + 1]) the flat positions g N + j of the live entries with index
 *     u, ascending; a row of S without an entry gets 0; every output 0 past d.
 * Products in exact-fp32 MFMA; the logit tiles are recomputed, never stored.  A list is split over `splits` workgroup
 * columns of entries_per_split (a multiple of 64).  Scratch (scratch_floats 4-byte words, 16-byte aligned,
 * caller-allocated; ops.listed_xent_plan gives the size): 2 ceil64(R) + 64 + ceil64(G + 1) words of row lists and group
 * offsets, then the forward's 2 ceil64(splits R) (max, sum-exp) partials, or the backward's ceil64((splits + 1) R ld) dP
 * partials and the ceil64(G N ld) entry partials E, ld = round_up(d, 4).  No float atomics: the same call gives the same
 * bits.  U = 0 is legal (S, dS, csr_* unused): every valid row's loss is 0.
 * CARCA_ERR_UNSUPPORTED: d > 256, G N >= 2^31, R >= 2^25 - 64.  CARCA_ERR_BADARG: null pointers, strides, alignment,
 * rows_per_list outside 1..1024 or R != G rows_per_list, splits outside 1..256, entries_per_split * splits < N,
 * scratch too small. */
typedef struct CarcaListedXentDesc {
  int R, G, rows_per_list, N, U, n_items, d;
  const float* P;
  int ld_p;
  const float* Tp;
  int ld_tp;
  const float* pos_bias;   /* [R] or NULL */
  const int32_t* pos;      /* [R] */
  const float* S;          /* [U, ld_s] */
  int ld_s;
  const int32_t* lists;    /* [G, N] */
  const int32_t* index;    /* [G, N] */
  const float* bias;       /* [G, N] or NULL */
  const int32_t* csr_off;  /* [U + 1] backward */
  const int32_t* csr_ent;  /* [>= csr_off[U]] backward */
  int splits, entries_per_split;
  float* scratch;
  int64_t scratch_floats;
  float* lse;        /* [R]: forward output, backward input */
  float* row_loss;   /* [R]: forward output, backward input */
  float* loss;       /* [1] forward */
  const float* grad; /* [1] backward: upstream scale of loss */
  float* dP;         /* [R, ld_p] backward */
  float* dTp;        /* [R, ld_tp] backward */
  float* dS;         /* [U, ld_s] backward */
} CarcaListedXentDesc;
int carca_listed_xent_fwd(const CarcaListedXentDesc* desc, void* stream);
int carca_listed_xent_bwd(const CarcaListedXentDesc* desc, void* stream);

/* ---- binary cross-entropy against K shared negatives (gBCE) for the dot decoders -------------
 * P [R, ld_p] profile rows, Tp [R, ld_tp] the rows of their positives (context included), S [K, ld_s] the rows of K
 * samples shared by every row (zero context), C [R, ld_c] the rows' context share M c_r, or NULL (d features; ld_p, ld_tp,
 * ld_s multiples of 4, ld_c >= d; P and S 16-byte aligned), pos [R] and s_ids [K] int32.  Row r is VALID iff pos[r] lies
 * in [1, n_items).  Sample k is a negative of row r iff s_ids[k] lies in [1, n_items) and differs from pos[r] (accidental
 * hits removed; duplicates each count).  With sp = softplus, z(r, +) = P[r] . Tp[r] and z(r, k) = P[r] . S[k] + br[r]:
 *   carca_sampled_bce_fwd: zpos[r] = z(r, +), br[r] = P[r] . C[r] (0 without C), gsum[r] = G_r = sum over the negatives k
 *     of r of sigmoid(z(r, k)), row_loss[r] = beta sp(-zpos[r]) + sum over the negatives of sp(z(r, k)) (all 0 for a row
 *     that is not valid), loss[0] = sum of row_loss / n_valid (0 when no row is valid);
 *   carca_sampled_bce_bwd: with zpos, br and gsum from the forward and the upstream scale grad[0],
 *     G[r, k] = sigmoid(z(r, k)) on the negatives (else 0), gp = -beta sigmoid(-zpos[r]):
 *     dP  = grad / n_valid (G S + gp Tp + G_r C), dTp = grad / n_valid gp P, dC = grad / n_valid G_r P (0 for rows that
 *     are not valid), dS = grad / n_valid G^T P (0 for samples that are no class); every output 0 past d.
 * The softplus is max(x, 0) + log(1 + exp(-|x|)): no overflow.  Products in exact-fp32 MFMA; the logit tiles are
 * recomputed, never stored.  Splits and scratch as carca_sampled_xent_* (ops.sampled_bce_plan gives the sizes): 2
 * ceil64(R) + 64 words of row lists, then the forward's 2 ceil64(splits_samples R) (sum sp, sum sigmoid) partials, or the
 * backward's ceil64((splits_samples + 1) R ld) dP partials or, where larger (splits_rows > 1), ceil64(splits_rows K ld)
 * dS partials in the same words (dP is complete before dS starts), ld = round_up(d, 4).  No float atomics: the same
 * call gives the same bits.  CARCA_ERR_UNSUPPORTED: d > 256.
 * CARCA_ERR_BADARG: null pointers, strides, beta outside [0, 1], split counts outside 1..256, samples_per_split *
 * splits_samples < K, scratch too small, C without dC in the backward. */
typedef struct CarcaSampledBceDesc {
  int R, K, n_items, d;
  const float* P;
  int ld_p;
  const float* Tp;
  int ld_tp;
  const float* C;        /* [R, ld_c] or NULL */
  int ld_c;
  const int32_t* pos;    /* [R] */
  const float* S;
  int ld_s;
  const int32_t* s_ids;  /* [K] */
  float beta;            /* weight of the positive's term */
  int splits_samples, samples_per_split, splits_rows;
  float* scratch;
  int64_t scratch_floats;
  float* zpos;       /* [R]: forward output, backward input */
  float* br;         /* [R]: forward output, backward input */
  float* gsum;       /* [R]: forward output, backward input */
  float* row_loss;   /* [R] forward */
  float* loss;       /* [1] forward */
  const float* grad; /* [1] backward: upstream scale of loss */
  float* dP;         /* [R, ld_p] backward */
  float* dTp;        /* [R, ld_tp] backward */
  float* dC;         /* [R, ld_c] backward (with C) */
  float* dS;         /* [K, ld_s] backward */
} CarcaSampledBceDesc;
int carca_sampled_bce_fwd(const CarcaSampledBceDesc* desc, void* stream);
int carca_sampled_bce_bwd(const CarcaSampledBceDesc* desc, void* stream);

/* ---- item-to-item top-k over a row table: "which items are closest to this item"  -------------
 * carca_row_rnorm: out[i] = 1 / max(sqrt(sum_c table[i][c]^2), 1e-12) over the first n_cols columns of each of the n_rows
 * rows of table [n_rows, ld], in fp32, one wave per row.
 *
 * carca_similar_items: for each of the Q query ids items[q] (int32) the k columns of the table X [n_items, ld_table] (fp32,
 * n_cols live columns; ld_table a multiple of 4, base 16-byte aligned; no column past n_cols reaches a product) that score
 * highest against row items[q]:
 *   metric CARCA_SIMILAR_DOT:    score = X[q] . X[i];
 *   metric CARCA_SIMILAR_COSINE: score = ((X[q] . X[i]) * rnorm[q]) * rnorm[i], rnorm [n_items] from carca_row_rnorm (the
 *     caller owns it: it is not recomputed per call).  An all-zero row is eligible and scores 0.
 * Eligible: ids 1 .. n_items - 1, minus the query's own id when exclude_self, intersected with the candidate list when
 * one is given (candidates NULL: the whole table; n >= 1 otherwise -- the caller pads for an empty list).  Order and
 * padding are carca_recommend's: score descending, ties to the smaller id, fewer than k eligible items pad with id 0 and
 * score 0; scores are the raw metric (no link).  A query id outside [1, n_items) gives a fully padded row; duplicates are
 * allowed.  With a list, its rows and their rnorm are first copied into the caller's cand_table [n, ld_cand_table] (a
 * multiple of 4, >= n_cols, 16-byte aligned) and cand_rnorm [n] when gather_candidates is set -- a caller that splits its
 * queries over several calls sets it on the first only -- and the same scoring kernel runs over that compact table.
 * Exact-fp32 MFMA products; the Q x C scores (C = n_items or n) live in stream scratch (or the capture's memory), with
 * the gathered query rows when n_cols > 128; the selection launch is carca_recommend's.  A pair's score bits do not
 * depend on Q, on the query's position or on the list; the same call gives the same bits.  No host wait.
 * CARCA_ERR_UNSUPPORTED: k outside 1..128, n_cols > 2^22.  CARCA_ERR_BADARG: null pointers, strides, alignment, an
 * unknown metric, cosine without rnorm, a list without cand_table (or, for cosine, cand_rnorm), n outside 1..n_items-1. */
enum { CARCA_SIMILAR_DOT = 0, CARCA_SIMILAR_COSINE = 1 };
typedef struct CarcaSimilarDesc {
  int Q, n_items, n_cols, k;
  int metric, exclude_self;
  const float* table; /* [n_items, ld_table] */
  int ld_table;
  const float* rnorm;   /* [n_items], or NULL for CARCA_SIMILAR_DOT */
  const int32_t* items; /* [Q] query ids */
  float* cand_table;    /* [n, ld_cand_table] with a candidate list, else unused */
  int ld_cand_table;
  float* cand_rnorm;    /* [n] with a candidate list and CARCA_SIMILAR_COSINE */
  int gather_candidates; /* fill cand_table / cand_rnorm in this call (else a previous call on the stream has) */
  float* scores; /* [Q, ld_scores] */
  int ld_scores;
  int64_t* ids_out; /* [Q, ld_ids_out] */
  int ld_ids_out;
} CarcaSimilarDesc;
int carca_row_rnorm(const float* table, int ld, int n_rows, int n_cols, float* out, void* stream);
int carca_similar_items(const CarcaSimilarDesc* desc, const CarcaCandidates* candidates, void* stream);

/* ---- diversity re-ranking of a top-k pool: maximal marginal relevance + intra-list diversity ---
 * carca_mmr_rerank: per user u of B a pool of P entries (pool_scores[u][j], pool_ids[u][j]), j = 0 .. P - 1 in pool order
 * (carca_recommend's outputs, or any caller's), re-ranked greedily over the rows of table X [n_items, ld_table] (fp32,
 * n_cols live columns; ld_table a multiple of 4, base 16-byte aligned; no column past n_cols reaches a product):
 *   valid entries: 1 <= id < n_items; every other entry is skipped (no host check, no read); a repeated id is an entry
 *     of its own;
 *   sim(a, b) = X[a] . X[b] (CARCA_SIMILAR_DOT) or ((X[a] . X[b]) * rnorm[a]) * rnorm[b] (CARCA_SIMILAR_COSINE; rnorm
 *     [n_items] from carca_row_rnorm, the caller's; an all-zero row has similarity 0 to everything);
 *   rel_j = (s_j - s_min) / (s_max - s_min) over the user's valid entries, 0 where s_max == s_min (normalize != 0), or
 *     s_j (normalize == 0);
 *   step t = 0 .. k - 1, while an untaken valid entry remains: obj_j = lam * rel_j - (1 - lam) * M_j with M_j = 0 at
 *     t = 0 and max over the selected s of sim(id_j, id_s) after; the largest obj wins, ties to the smaller pool position.
 * Outputs: scores [B, k] the selected entries' pool scores (their bits), ids_out [B, k] in selection order, both padded
 * with 0 where fewer than k entries are valid; ild [B] the mean over pairs a < b of the selected entries of 1 - sim (the
 * values the selection used, summed in selection order), 0 with fewer than two.  lam = 1 gives the first k valid entries.
 * One workgroup per user; only the rows of the pool's Gram matrix that the selection asks for are computed (n_cols <= 128:
 * the pool's rows staged in LDS; wider: streamed from the table at each step).  Plain fp32 fmaf sums whose order depends
 * on n_cols alone: bitwise-equal rows give bitwise-equal similarities; no atomics, no scratch, no host wait; a user's
 * result does not depend on B or on its position.
 * CARCA_ERR_UNSUPPORTED: P outside 1..128, k outside 1..P, B > 65535, n_cols > 2^22.  CARCA_ERR_BADARG: null pointers,
 * strides, alignment, an unknown metric, cosine without rnorm, lam outside [0, 1]. */
typedef struct CarcaMmrDesc {
  int B, P, k, n_items, n_cols;
  int metric, normalize; /* CARCA_SIMILAR_DOT / CARCA_SIMILAR_COSINE; rel normalised per user */
  float lam;
  const float* pool_scores; /* [B, ld_pool_scores] */
  int ld_pool_scores;
  const int64_t* pool_ids; /* [B, ld_pool_ids] */
  int ld_pool_ids;
  const float* table; /* [n_items, ld_table] */
  int ld_table;
  const float* rnorm; /* [n_items], or NULL for CARCA_SIMILAR_DOT */
  float* scores;      /* [B, ld_scores] */
  int ld_scores;
  int64_t* ids_out; /* [B, ld_ids_out] */
  int ld_ids_out;
  float* ild; /* [B] */
} CarcaMmrDesc;
int carca_mmr_rerank(const CarcaMmrDesc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CARCA_HIP_H */
