// Diversity re-ranking of a top-k pool: greedy maximal marginal relevance and the intra-list diversity of the result
// (include/carca_hip.h: carca_mmr_rerank).
//
// One workgroup per user.  Pool entry j (position j of the user's P <= 128 entries) is valid iff 1 <= id_j < n_items.
// The selection lives in wave 0: lane l owns entries l and l + 64 (score, rel, M, the running sum D of 1 - sim against the
// selected entries, the live flag) in registers.  A step is
//   wave 0:  obj = lam * rel - (1 - lam) * M per live entry; arg max over the (obj, position) key, ties to the smaller
//            position; the winner's outputs are written and its D joins the ILD sum (selection order);
//   all:     sim(j, winner) for every live entry j -> LDS;        (not after the last step)
//   wave 0:  M = sim at the first step, max(M, sim) after; D += 1 - sim.
// Only those k - 1 rows of the pool's [P, P] Gram matrix are ever computed ("lazy rows": 2 (k - 1) P n_cols flops against
// 2 P^2 n_cols for the whole block).  Two instantiations of the similarity pass:
//   n_cols <= 128 (NARROW): the pool's rows are staged once in LDS (P x (round4(n_cols) + 4) floats, the + 4 spreading
//     neighbouring rows over the banks); thread j sums row j against the winner's row, four fmaf chains by column mod 4.
//   n_cols > 128: rows stream from the table.  Wave w owns entries w, w + 8, ..., eight of them per sweep over the columns;
//     per stage of 1024 columns a lane loads the winner's 4 x 16 bytes and the same bytes of the eight rows (36 loads in
//     flight), one fmaf chain per row and lane, folded by wave_sum at the end of the sweep.
// In both, the order of a sum depends on n_cols alone, never on which rows meet: bitwise-equal rows give bitwise-equal
// similarities, so equal scores on equal rows tie exactly and go to the smaller position.  No atomics, no scratch.
// Loads: a dead entry reads the winner's row instead (always a valid row; the sum is discarded), a column past the row's
// last 16-byte group is clamped to that group and masked to 0 after the load: no address leaves [row, row + round4(n_cols)).
#include <limits.h>

#include "carca_common.h"

namespace {

constexpr int MMR_PMAX = 128;          // pool entries per user
constexpr int MMR_NARROW = 128;        // widest row of the LDS-resident instantiation
constexpr int MMR_THREADS_NARROW = 256;
constexpr int MMR_THREADS_STREAM = 512;
constexpr int MMR_STAGE = 1024;        // streaming: columns per stage, 4 x 16 bytes per lane
constexpr int MMR_GROUP = 8;           // streaming: rows per sweep, their loads in flight together

struct MmrArgs {
  int P, k, n_items, n_cols, cosine, normalize;
  float lam;
  const float* pool_scores;
  int ld_pool_scores;
  const int64_t* pool_ids;
  int ld_pool_ids;
  const float* table;
  int ld_table;
  const float* rnorm;
  float* scores;
  int ld_scores;
  int64_t* ids_out;
  int ld_ids_out;
  float* ild;
};

struct MmrShared {
  int id[MMR_PMAX];     // the entry's item id, 0 for an invalid entry
  float rn[MMR_PMAX];   // its reciprocal row norm (cosine)
  float sim[MMR_PMAX];  // this step's similarity to the winner
  int live[MMR_PMAX];   // valid and not yet selected
  int sel;              // this step's winner (pool position), -1: none left
};

__device__ __forceinline__ float mmr_wave_min(float v) { return -wave_max(-v); }

// NARROW similarity pass: thread j, row j against row sel, both in LDS
__device__ __forceinline__ void mmr_sims_lds(const MmrArgs& A, const float* rows, int ldr, int nc4, int sel, MmrShared& S) {
  const int j = threadIdx.x;
  if (j >= A.P || !S.live[j]) return;
  const float* rj = rows + j * ldr;
  const float* rs = rows + sel * ldr;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nc4; c += 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(rj + c), b = *reinterpret_cast<const f32x4*>(rs + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = fmaf(a[i], b[i], acc[i]);
  }
  const float dot = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  S.sim[j] = A.cosine ? (dot * S.rn[j]) * S.rn[sel] : dot;
}

// the lane's 16 bytes at column col of a row (col a multiple of 4): clamped into the row, zero from n_cols on
template <bool FULL>
__device__ __forceinline__ f32x4 mmr_load4(const float* row, int col, int n_cols, int last4) {
  if (FULL) return *reinterpret_cast<const f32x4*>(row + col);
  f32x4 v = *reinterpret_cast<const f32x4*>(row + min(col, last4));
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = col + i < n_cols ? v[i] : 0.f;
  return v;
}

// one stage of MMR_STAGE columns: the winner's 16-byte groups against the same groups of the group's rows
template <bool FULL>
__device__ __forceinline__ void mmr_stream_stage(const MmrArgs& A, const float* const (&rowp)[MMR_GROUP], const float* srow,
                                                 int c0, int last4, float (&acc)[MMR_GROUP]) {
  constexpr int NV = MMR_STAGE / 256;
  const int lane = threadIdx.x & 63;
  f32x4 sv[NV], v[MMR_GROUP][NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) sv[i] = mmr_load4<FULL>(srow, c0 + 256 * i + 4 * lane, A.n_cols, last4);
#pragma unroll
  for (int rr = 0; rr < MMR_GROUP; ++rr)
#pragma unroll
    for (int i = 0; i < NV; ++i) v[rr][i] = mmr_load4<FULL>(rowp[rr], c0 + 256 * i + 4 * lane, A.n_cols, last4);
#pragma unroll
  for (int rr = 0; rr < MMR_GROUP; ++rr)
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[rr] = fmaf(v[rr][i][e], sv[i][e], acc[rr]);
}

// streaming similarity pass: wave w, entries w + nwaves r, MMR_GROUP of them per sweep over the columns
template <int THREADS>
__device__ __forceinline__ void mmr_sims_stream(const MmrArgs& A, int sel, MmrShared& S) {
  constexpr int NW = THREADS / 64;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int last4 = (A.n_cols - 1) / 4 * 4;
  const int sid = __builtin_amdgcn_readfirstlane(S.id[sel]);  // (row pointers stay wave-uniform)
  const float* srow = A.table + (size_t)sid * A.ld_table;
  const float rs = S.rn[sel];
  for (int j0 = wave; j0 < A.P; j0 += NW * MMR_GROUP) {
    const float* rowp[MMR_GROUP];
    float acc[MMR_GROUP];
#pragma unroll
    for (int rr = 0; rr < MMR_GROUP; ++rr) {
      const int j = j0 + NW * rr;
      const int id = __builtin_amdgcn_readfirstlane((j < A.P && S.live[j]) ? S.id[j] : 0);
      rowp[rr] = id ? A.table + (size_t)id * A.ld_table : srow;
      acc[rr] = 0.f;
    }
    int c0 = 0;
    for (; c0 + MMR_STAGE <= A.n_cols; c0 += MMR_STAGE) mmr_stream_stage<true>(A, rowp, srow, c0, last4, acc);
    if (c0 < A.n_cols) mmr_stream_stage<false>(A, rowp, srow, c0, last4, acc);
#pragma unroll
    for (int rr = 0; rr < MMR_GROUP; ++rr) {
      const int j = j0 + NW * rr;
      const float dot = wave_sum(acc[rr]);
      if (lane == 0 && j < A.P && S.live[j]) S.sim[j] = A.cosine ? (dot * S.rn[j]) * rs : dot;
    }
  }
}

template <bool NARROW, int THREADS>
__global__ __launch_bounds__(THREADS) void mmr_kernel(MmrArgs A) {
  extern __shared__ __attribute__((aligned(16))) float mmr_rows[];  // NARROW: [P][ldr]
  __shared__ MmrShared S;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  if (t < MMR_PMAX) {
    const long long id = t < A.P ? (long long)A.pool_ids[(size_t)b * A.ld_pool_ids + t] : 0;
    const bool valid = id >= 1 && id < A.n_items;
    S.id[t] = valid ? (int)id : 0;
    S.rn[t] = (valid && A.cosine) ? A.rnorm[id] : 0.f;
    S.live[t] = valid;
    S.sim[t] = 0.f;
  }
  __syncthreads();
  const int nc4 = round_up(A.n_cols, 4), ldr = nc4 + 4;
  if constexpr (NARROW) {  // the pool's rows, zero past n_cols and for an invalid entry
    const int q4 = nc4 / 4, total = A.P * q4;
#pragma unroll 4
    for (int x = t; x < total; x += THREADS) {
      const int j = x / q4, c = (x - j * q4) * 4;
      const int id = S.id[j];
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (id) {
        v = *reinterpret_cast<const f32x4*>(A.table + (size_t)id * A.ld_table + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = c + i < A.n_cols ? v[i] : 0.f;
      }
      *reinterpret_cast<f32x4*>(mmr_rows + j * ldr + c) = v;
    }
    __syncthreads();
  }
  // ---- wave 0: the entries' state ----
  float s[2] = {0.f, 0.f}, rel[2] = {0.f, 0.f}, M[2] = {0.f, 0.f}, D[2] = {0.f, 0.f};
  bool live[2] = {false, false};
  float total = 0.f;
  int count = 0;
  const float oml = 1.f - A.lam;
  if (wave == 0) {
    float smin = INFINITY, smax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int pos = lane + 64 * e;
      live[e] = S.live[pos] != 0;
      if (pos < A.P) s[e] = A.pool_scores[(size_t)b * A.ld_pool_scores + pos];
      if (live[e]) smin = fminf(smin, s[e]), smax = fmaxf(smax, s[e]);
    }
    smin = mmr_wave_min(smin), smax = wave_max(smax);
    const float range = smax - smin;
#pragma unroll
    for (int e = 0; e < 2; ++e) rel[e] = !A.normalize ? s[e] : (range > 0.f ? (s[e] - smin) / range : 0.f);
  }
  for (int step = 0; step < A.k; ++step) {
    if (wave == 0) {
      float bo = 0.f;
      int bp = INT_MAX;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float obj = __fsub_rn(__fmul_rn(A.lam, rel[e]), __fmul_rn(oml, M[e]));
        if (live[e] && (bp == INT_MAX || obj > bo)) bo = obj, bp = lane + 64 * e;
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float o2 = __shfl_xor(bo, off);
        const int p2 = __shfl_xor(bp, off);
        if (p2 != INT_MAX && (bp == INT_MAX || o2 > bo || (o2 == bo && p2 < bp))) bo = o2, bp = p2;
      }
      bp = __builtin_amdgcn_readfirstlane(bp);
      if (bp != INT_MAX) {
        const int e = bp >> 6, owner = bp & 63;
        total += __shfl(e ? D[1] : D[0], owner);
        ++count;
        if (lane == owner) {
          A.scores[(size_t)b * A.ld_scores + step] = e ? s[1] : s[0];
          A.ids_out[(size_t)b * A.ld_ids_out + step] = S.id[bp];
          if (e) live[1] = false; else live[0] = false;
          S.live[bp] = 0;
        }
      }
      if (lane == 0) S.sel = bp == INT_MAX ? -1 : bp;
    }
    __syncthreads();
    const int sel = S.sel;
    if (sel < 0 || step == A.k - 1) break;  // (uniform over the workgroup)
    if constexpr (NARROW)
      mmr_sims_lds(A, mmr_rows, ldr, nc4, sel, S);
    else
      mmr_sims_stream<THREADS>(A, sel, S);
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int e = 0; e < 2; ++e)
        if (live[e]) {
          const float sim = S.sim[lane + 64 * e];
          M[e] = step == 0 ? sim : fmaxf(M[e], sim);
          D[e] += 1.f - sim;
        }
    }
  }
  if (wave == 0) {
    for (int x = count + lane; x < A.k; x += 64) {
      A.scores[(size_t)b * A.ld_scores + x] = 0.f;
      A.ids_out[(size_t)b * A.ld_ids_out + x] = 0;
    }
    if (lane == 0) A.ild[b] = count >= 2 ? total / (0.5f * (float)count * (float)(count - 1)) : 0.f;
  }
}

}  // namespace

extern "C" int carca_mmr_rerank(const CarcaMmrDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "mmr_rerank: null descriptor");
  const CarcaMmrDesc& D = *desc;
  CARCA_CHECK_ARG(D.B >= 1 && D.n_items >= 1 && D.n_cols >= 1, "mmr_rerank: B, n_items and n_cols must be positive");
  CARCA_CHECK_SUPPORTED(D.P >= 1 && D.P <= MMR_PMAX, "mmr_rerank: pool size P = %d outside 1..128", D.P);
  CARCA_CHECK_SUPPORTED(D.k >= 1 && D.k <= D.P, "mmr_rerank: k = %d outside 1..P = %d", D.k, D.P);
  CARCA_CHECK_SUPPORTED(D.B <= 65535, "mmr_rerank: B = %d exceeds 65535", D.B);
  CARCA_CHECK_SUPPORTED(D.n_cols <= (1 << 22), "mmr_rerank: n_cols = %d exceeds 2^22", D.n_cols);
  CARCA_CHECK_ARG(D.metric == CARCA_SIMILAR_DOT || D.metric == CARCA_SIMILAR_COSINE, "mmr_rerank: metric must be 0 (dot) or 1 (cosine)");
  CARCA_CHECK_ARG(D.lam >= 0.f && D.lam <= 1.f, "mmr_rerank: lam = %g outside [0, 1]", (double)D.lam);
  CARCA_CHECK_ARG(D.table && D.ld_table >= D.n_cols && D.ld_table <= (1 << 24) && D.ld_table % 4 == 0 &&
                      ((uintptr_t)D.table & 15) == 0,
                  "mmr_rerank: null or unaligned table, or ld_table outside n_cols..2^24 or no multiple of 4");
  CARCA_CHECK_ARG(D.metric == CARCA_SIMILAR_DOT || D.rnorm, "mmr_rerank: the cosine metric needs rnorm");
  CARCA_CHECK_ARG(D.pool_scores && D.pool_ids && D.ld_pool_scores >= D.P && D.ld_pool_ids >= D.P,
                  "mmr_rerank: null pool or row stride shorter than P");
  CARCA_CHECK_ARG(D.scores && D.ids_out && D.ild && D.ld_scores >= D.k && D.ld_ids_out >= D.k,
                  "mmr_rerank: null output or row stride shorter than k");
  MmrArgs A = {};
  A.P = D.P, A.k = D.k, A.n_items = D.n_items, A.n_cols = D.n_cols;
  A.cosine = D.metric == CARCA_SIMILAR_COSINE, A.normalize = D.normalize != 0, A.lam = D.lam;
  A.pool_scores = D.pool_scores, A.ld_pool_scores = D.ld_pool_scores, A.pool_ids = D.pool_ids, A.ld_pool_ids = D.ld_pool_ids;
  A.table = D.table, A.ld_table = D.ld_table, A.rnorm = D.rnorm;
  A.scores = D.scores, A.ld_scores = D.ld_scores, A.ids_out = D.ids_out, A.ld_ids_out = D.ld_ids_out, A.ild = D.ild;
  if (D.n_cols <= MMR_NARROW) {
    auto kern = mmr_kernel<true, MMR_THREADS_NARROW>;
    constexpr size_t LDS_MAX = sizeof(float) * MMR_PMAX * (MMR_NARROW + 4);
    static bool attr_set = false;
    if (!attr_set) {
      hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
      if (e != hipSuccess) {
        carca_set_error("mmr_rerank: cannot reserve %zu B of LDS: %s", LDS_MAX, hipGetErrorString(e));
        return (int)e;
      }
      attr_set = true;
    }
    const size_t lds_bytes = sizeof(float) * D.P * (round_up(D.n_cols, 4) + 4);
    hipLaunchKernelGGL(kern, dim3(D.B), dim3(MMR_THREADS_NARROW), lds_bytes, stream, A);
  } else {
    hipLaunchKernelGGL((mmr_kernel<false, MMR_THREADS_STREAM>), dim3(D.B), dim3(MMR_THREADS_STREAM), 0, stream, A);
  }
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
