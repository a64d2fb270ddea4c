// Item-to-item top-k over a row table (include/carca_hip.h: carca_similar_items, carca_row_rnorm).
//
// X [n_items, ld] is a table of fp32 rows, n_cols of them live: CARCA's item table T[i] = e(i, 0), KNN's attribute table,
// or any caller's.  For a chunk of Q query ids the call scores every (query, column) pair into a [Q, C] stream-scratch
// buffer and selects the k best columns per query with catalogue_select.h's selection launch, unchanged:
//   score = X[q] . X[i]                       ("dot")
//   score = ((X[q] . X[i]) * r_q) * r_i       ("cosine"), r = 1 / max(||row||, 1e-12) from carca_row_rnorm
// Columns are item ids (rc::AllItems, C = n_items) or positions in an ascending candidate list (rc::ListedItems, C = n):
// the listed rows and their r are first copied into a compact [C, ld_cand] table (rs::gather_kernel) and the same scoring
// kernels run over it, so a pair's score bits do not depend on the list, on the query's position or on the chunk.
// Launches per chunk: (gather, first chunk of a call with a list), scoring, selection.  The scoring epilogue writes the
// selection's sentinel into the id-0 column (no list), into the query's own column (exclude_self) and into every column of
// a query whose id is outside [1, n_items): there is no exclusion launch and no second pass over the buffer.
// Two scoring kernels, both exact-fp32 products on v_mfma_f32_16x16x4_f32 over a workgroup of 64 queries:
//   n_cols <= 128: query-stationary.  Each wave loads the A operands of the 64 query rows once (KP / 4 registers per
//     16-query block, KP = 64 / 96 / 128 the padded width) and streams 16-item tiles through them: only item rows and
//     the r vectors are read in the loop.  The tiles go round-robin over the waves of the workgroups of a query block.
//   n_cols > 128: rs::score_kernel (row_stream.h), the streaming loop KNN's catalogue calls run too (operands re-read
//     from a gathered, zero-padded query buffer at every 64-byte step, MFMA chains folded every 256 k), with this
//     file's prologue and epilogue.
// Item rows come through buffer loads whose wave-uniform base carries the 64-bit row offset: lane offsets stay below 16
// rows, loads past the last row return 0, and no column past n_cols reaches a product (masked after the load).
#include "catalogue_select.h"
#include "row_stream.h"

namespace {

constexpr int SI_STAT_MAX = 128;      // widest row of the query-stationary kernel
constexpr int SI_SELF_NONE = -1;      // no column to blank for this query
constexpr int SI_SELF_INVALID = -2;   // the query id is outside [1, n_items): every column blanked

// ---- reciprocal row norms: one wave per row -----------------------------------------------------------------------
__global__ __launch_bounds__(rs::THREADS) void si_rnorm_kernel(const float* __restrict__ table, int64_t ld, int n_rows,
                                                              int n_cols, float* __restrict__ out) {
  const int row = blockIdx.x * rs::WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const float* x = table + (size_t)row * ld;
  float s = 0.f;
  for (int c = lane; c < n_cols; c += 64) s = fmaf(x[c], x[c], s);
  s = wave_sum(s);
  if (lane == 0) out[row] = 1.f / fmaxf(sqrtf(s), 1e-12f);
}

// ---- the row source of rs::gather_kernel: src[ids[u]], a zero row for an id outside [1, n_src) and past the n ids;
// thread 0 also copies the row's r where the caller asks for it
struct SiRow {
  const float* src;
  int64_t ld_src;
  int n_src;
  const float* rn_src;  // or NULL
  const int32_t* ids;
  int n;
  float* rn_dst;  // [n] or NULL
  __device__ const float* operator()(int u) const {
    if (u >= n) return nullptr;
    const int id = ids[u];
    const float* row = id >= 1 && id < n_src ? src + (size_t)id * ld_src : nullptr;
    if (rn_dst && threadIdx.x == 0) rn_dst[u] = (row && rn_src) ? rn_src[id] : 0.f;
    return row;
  }
};

// ---- scoring -------------------------------------------------------------------------------------------------------
struct SiScore {
  const float* table;  // [n_items, ld]: the query rows (stationary kernel)
  int ld;
  const float* rn;  // [n_items] or NULL (dot)
  const float* ctable;  // [C, cld]: the columns' rows (the table itself without a list)
  int cld;
  const float* crn;  // [C] or NULL
  const float* qbuf;  // streaming kernel: [nqb * 64, ldq] gathered query rows, zero past n_cols
  int ldq, nchunks;
  const int32_t* items;  // [Q] query ids
  int Q, n_items, n_cols, C;
  int cosine, exclude_self;
  int nqb;  // query blocks
  int tiles, nsplit;  // stationary kernel: 16-item tiles, and the workgroups that share one query block's tiles
  float* out;  // [Q, C]
};

struct SiQueries {  // per query of the workgroup's block
  alignas(16) float rq[rs::QB];
  int self[rs::QB];
};

// Workgroup prologue: r_q and the column to blank of each of the block's 64 queries.  Ends with a barrier.
template <class Map>
__device__ __forceinline__ void si_stage_queries(const SiScore& P, int q0, const Map& map, SiQueries& S) {
  const int t = threadIdx.x;
  if (t < rs::QB) {
    const int q = q0 + t;
    const int id = q < P.Q ? P.items[q] : 0;
    const bool valid = id >= 1 && id < P.n_items;
    S.rq[t] = (valid && P.rn) ? P.rn[id] : 0.f;
    S.self[t] = !valid ? SI_SELF_INVALID : (P.exclude_self ? map.find(id) : SI_SELF_NONE);
  }
  __syncthreads();
}

// One 16-item x 64-query tile out of the accumulators: D holds column (item) r, rows (queries) 4g .. 4g + 3 of each block.
template <class Map>
__device__ __forceinline__ void si_epilogue(const SiScore& P, const f32x4 (&acc)[rs::MQ], int q0, int col, int g,
                                            const SiQueries& S) {
  if (col >= P.C) return;
  const float ri = P.cosine ? P.crn[col] : 0.f;
  const float sent = __uint_as_float(rc::RC_SENTINEL);
  const bool pad_col = !Map::listed && col == 0;  // id 0 is the padding item; no list holds it
#pragma unroll
  for (int m = 0; m < rs::MQ; ++m) {
    const f32x4 rq = *reinterpret_cast<const f32x4*>(&S.rq[16 * m + 4 * g]);
    const int* self = &S.self[16 * m + 4 * g];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = q0 + 16 * m + 4 * g + j;
      float v = acc[m][j];
      if (P.cosine) v = (v * rq[j]) * ri;
      const int sc = self[j];
      if (pad_col || sc == SI_SELF_INVALID || sc == col) v = sent;
      if (q < P.Q) P.out[(size_t)q * P.C + col] = v;
    }
  }
}

// rs::score_kernel's epilogue for the streaming case (n_cols > 128)
template <class Map>
struct SiStream {
  SiScore P;
  Map map;
  typedef SiQueries Shared;
  __device__ void stage(int q0, Shared& S) const { si_stage_queries(P, q0, map, S); }
  __device__ void store(const f32x4 (&tile)[rs::MQ], int q0, int col, int g, const Shared& S) const {
    si_epilogue<Map>(P, tile, q0, col, g, S);
  }
};

template <int KP, class Map>
__global__ __launch_bounds__(rs::THREADS) void si_score_stationary_kernel(SiScore P, Map map) {
  constexpr int NCH = KP / 16;
  __shared__ SiQueries S;
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qb = blockIdx.x % P.nqb, split = blockIdx.x / P.nqb;
  const int q0 = qb * rs::QB;
  si_stage_queries(P, q0, map, S);
  const int lim = P.n_cols - 4 * g;
  // A operands: chunk c of query row 16m + r, bytes 64c + 16g .. +15, zero for an invalid query
  f32x4 a[NCH][rs::MQ];
#pragma unroll
  for (int m = 0; m < rs::MQ; ++m) {
    const int q = q0 + 16 * m + r;
    const int id = q < P.Q ? P.items[q] : 0;
    const bool valid = id >= 1 && id < P.n_items;
    const float* row = P.table + (size_t)(valid ? id : 0) * P.ld;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      a[c][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (valid && 16 * c < lim) {  // (ld is a multiple of 4: the 16 bytes stay inside the row's stride)
        const u32x4 v = *reinterpret_cast<const u32x4*>(row + 16 * c + 4 * g);
        a[c][m] = rs::mask4(v, c, lim);
      }
    }
  }
  const int t_end = P.tiles, t_step = P.nsplit * rs::WAVES;
  const int t_off = (r * P.cld + 4 * g) * 4;
  auto load_tile = [&](int t, f32x4 (&b)[NCH]) {
    const int i0 = t * 16, rows = min(16, P.C - i0);
    const auto tr = rs::rsrc(P.ctable + (size_t)i0 * P.cld, (unsigned)rows * P.cld * 4);
#pragma unroll
    for (int c = 0; c < NCH; ++c) b[c] = rs::mask4(__builtin_amdgcn_raw_buffer_load_b128(tr, t_off, c * 64, 0), c, lim);
  };
  auto score_tile = [&](int t, const f32x4 (&b)[NCH]) {
    f32x4 acc[rs::MQ];
#pragma unroll
    for (int m = 0; m < rs::MQ; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int m = 0; m < rs::MQ; ++m) acc[m] = mfma16_group(a[c][m], b[c], acc[m]);
    si_epilogue<Map>(P, acc, q0, t * 16 + r, g, S);
  };
  // Tiles go round-robin over the waves of the nsplit workgroups of a query block: at any time they write one window of
  // nsplit x 64 neighbouring columns per query row.  The next tile's rows are in flight under this tile's products.
  int t = split * rs::WAVES + wave;
  f32x4 b0[NCH], b1[NCH];
  if (t < t_end) load_tile(t, b0);
  while (t < t_end) {
    if (t + t_step < t_end) load_tile(t + t_step, b1);
    score_tile(t, b0);
    t += t_step;
    if (t >= t_end) break;
    if (t + t_step < t_end) load_tile(t + t_step, b0);
    score_tile(t, b1);
    t += t_step;
  }
}

template <class Map>
int si_launch_score(const SiScore& P0, const Map& map, hipStream_t stream) {
  SiScore P = P0;
  if (P.n_cols > SI_STAT_MAX) {
    const rs::Operands R = {P.ctable, P.cld, P.qbuf, P.ldq, P.C, P.n_cols, P.nchunks, P.nqb};
    return rs::launch_score<rs::F32Aligned>(R, SiStream<Map>{P, map}, "similar_items", stream);
  }
  // enough workgroups to fill the device, each wave keeping at least 2 tiles under its A operands where the range allows
  const int want = (1024 + P.nqb - 1) / P.nqb;
  const int most = (P.tiles + 2 * rs::WAVES - 1) / (2 * rs::WAVES);
  P.nsplit = max(1, min(want, most));
  const long long blocks = (long long)P.nqb * P.nsplit;
  CARCA_CHECK_SUPPORTED(blocks < (1ll << 31), "similar_items: %lld scoring workgroups", blocks);
  const dim3 grid((unsigned)blocks), block(rs::THREADS);
  if (P.n_cols <= 64)
    hipLaunchKernelGGL((si_score_stationary_kernel<64, Map>), grid, block, 0, stream, P, map);
  else if (P.n_cols <= 96)
    hipLaunchKernelGGL((si_score_stationary_kernel<96, Map>), grid, block, 0, stream, P, map);
  else
    hipLaunchKernelGGL((si_score_stationary_kernel<128, Map>), grid, block, 0, stream, P, map);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

size_t si_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

}  // namespace

extern "C" int carca_row_rnorm(const float* table, int ld, int n_rows, int n_cols, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(table && out && n_rows >= 1 && n_cols >= 1 && ld >= n_cols, "row_rnorm: null pointer, empty table or ld < n_cols");
  hipLaunchKernelGGL(si_rnorm_kernel, dim3((n_rows + rs::WAVES - 1) / rs::WAVES), dim3(rs::THREADS), 0, stream, table,
                     (int64_t)ld, n_rows, n_cols, out);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

extern "C" int carca_similar_items(const CarcaSimilarDesc* desc, const CarcaCandidates* cand, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "similar_items: null descriptor");
  const CarcaSimilarDesc& D = *desc;
  CARCA_CHECK_ARG(D.Q >= 1 && D.n_items >= 1 && D.n_cols >= 1, "similar_items: Q, n_items and n_cols must be positive");
  CARCA_CHECK_SUPPORTED(D.k >= 1 && D.k <= rc::RC_KMAX, "similar_items: k = %d outside 1..128", D.k);
  // (32-bit lane offsets: 64 query rows and 16 table rows stay below 2^30 bytes)
  CARCA_CHECK_SUPPORTED(D.n_cols <= (1 << 22), "similar_items: n_cols = %d exceeds 2^22", D.n_cols);
  CARCA_CHECK_ARG(D.metric == CARCA_SIMILAR_DOT || D.metric == CARCA_SIMILAR_COSINE, "similar_items: metric must be 0 (dot) or 1 (cosine)");
  CARCA_CHECK_ARG(D.table && D.ld_table >= D.n_cols && D.ld_table <= (1 << 24) && D.ld_table % 4 == 0 &&
                      ((uintptr_t)D.table & 15) == 0,
                  "similar_items: null or unaligned table, or ld_table outside n_cols..2^24 or no multiple of 4");
  CARCA_CHECK_ARG(D.metric == CARCA_SIMILAR_DOT || D.rnorm, "similar_items: the cosine metric needs rnorm");
  CARCA_CHECK_ARG(D.items, "similar_items: null items");
  CARCA_CHECK_ARG(D.scores && D.ids_out && D.ld_scores >= D.k && D.ld_ids_out >= D.k,
                  "similar_items: null output or row stride shorter than k");
  int C = D.n_items;
  if (cand) {
    CARCA_CHECK_ARG(cand->n >= 1 && cand->n < D.n_items && cand->ids, "similar_items: bad candidate list (n = 0 launches nothing: "
                    "the caller pads)");
    C = cand->n;
    CARCA_CHECK_ARG(D.cand_table && D.ld_cand_table >= D.n_cols && D.ld_cand_table <= (1 << 24) && D.ld_cand_table % 4 == 0 &&
                        ((uintptr_t)D.cand_table & 15) == 0 && (D.metric == CARCA_SIMILAR_DOT || D.cand_rnorm),
                    "similar_items: a candidate list needs cand_table (aligned, ld_cand_table a multiple of 4 in n_cols..2^24) "
                    "and, for cosine, cand_rnorm");
  }
  const bool streaming = D.n_cols > SI_STAT_MAX;
  const int nqb = (D.Q + rs::QB - 1) / rs::QB;
  const int ldq = round_up(D.n_cols, 16);  // a whole number of 64-byte chunks
  const size_t out_bytes = si_align((size_t)D.Q * (size_t)C * sizeof(float));
  const size_t q_bytes = streaming ? si_align((size_t)nqb * rs::QB * ldq * sizeof(float)) : 0;
  const size_t bytes = out_bytes + q_bytes;
  char* base = (char*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                      : carca_stream_scratch(stream, CARCA_SCRATCH_SIMILAR, bytes));
  CARCA_CHECK_ARG(base, "similar_items: scratch allocation of %zu bytes failed", bytes);
  if (cand && D.gather_candidates) {
    const SiRow src = {D.table, D.ld_table, D.n_items, D.rnorm, cand->ids, C, D.cand_rnorm};
    hipLaunchKernelGGL((rs::gather_kernel<float, SiRow>), dim3(C), dim3(rs::THREADS), 0, stream, src, D.n_cols, D.cand_table,
                       D.ld_cand_table);
    CARCA_LAUNCH_CHECK();
  }
  SiScore P = {};
  P.table = D.table, P.ld = D.ld_table, P.rn = D.rnorm;
  P.ctable = cand ? D.cand_table : D.table, P.cld = cand ? D.ld_cand_table : D.ld_table;
  P.crn = cand ? D.cand_rnorm : D.rnorm;
  P.items = D.items, P.Q = D.Q, P.n_items = D.n_items, P.n_cols = D.n_cols, P.C = C;
  P.cosine = D.metric == CARCA_SIMILAR_COSINE, P.exclude_self = D.exclude_self != 0;
  P.nqb = nqb, P.tiles = (C + 15) / 16, P.out = (float*)base;
  if (streaming) {
    float* qbuf = (float*)(base + out_bytes);
    const SiRow src = {D.table, D.ld_table, D.n_items, nullptr, D.items, D.Q, nullptr};
    hipLaunchKernelGGL((rs::gather_kernel<float, SiRow>), dim3(nqb * rs::QB), dim3(rs::THREADS), 0, stream, src, D.n_cols,
                       qbuf, ldq);
    CARCA_LAUNCH_CHECK();
    P.qbuf = qbuf, P.ldq = ldq, P.nchunks = ldq / 16;
  }
  rc::SelectView S = {};
  S.n_items = D.n_items, S.k = D.k, S.scores = D.scores, S.ld_scores = D.ld_scores, S.ids_out = D.ids_out;
  S.ld_ids_out = D.ld_ids_out;
  if (cand) {
    const rc::ListedItems map = {cand->ids, C};
    const int rc_ = si_launch_score(P, map, stream);
    if (rc_ != CARCA_OK) return rc_;
    hipLaunchKernelGGL((rc::rc_select_kernel<rc::SelectView, rc::ListedItems>), dim3(D.Q), dim3(rc::RC_SEL_THREADS), 0, stream, S,
                       (const float*)P.out, C, map);
  } else {
    const rc::AllItems map = {};
    const int rc_ = si_launch_score(P, map, stream);
    if (rc_ != CARCA_OK) return rc_;
    hipLaunchKernelGGL((rc::rc_select_kernel<rc::SelectView, rc::AllItems>), dim3(D.Q), dim3(rc::RC_SEL_THREADS), 0, stream, S,
                       (const float*)P.out, C, map);
  }
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
