// The feature product of an evaluation batch over its DISTINCT attribute rows (carca_gemm_rows_feat_dedup, gemm.hip).
//
// Attribute rows are per item (data.py: p_a = attrs[p_x], o_a = attrs[o_x]), and an evaluation batch repeats items: at
// C2 the 16.2 k kept rows (id != 0) hold 8.9 k distinct ids, at C3 65 k hold 12 k.  q = [a ; c] W_f^T + b_f splits into
//     q_r = P[u(r)] + c_r W_c^T + b_f,   P = A_unique W_a^T,
// so the 4096-deep product runs over one representative row per group and the six context columns per row.  Four launches:
//   1. dedup_insert_kernel   every kept row into an open-addressing table keyed by id (2x the rows, CAS on the key):
//                            the group's representative is its LOWEST row (atomicMax of ~row), whatever the timing;
//                            its grid also writes [W_c^T ; b_f] as one compact [K1 + 1][N] block for launch 4 (per
//                            launch: the weights change between evaluations);
//   2. dedup_resolve_kernel  a row whose representative is another row compares the two attribute rows as 32-bit
//                            integers (dense batches; rows gathered from one table by the same id are the same row) and
//                            stays its own representative on any difference (-0.0 / +0.0, NaN payloads: never merged);
//                            writes the row's representative and the kept-row flags the product plans from;
//   3. gemm_rows_skc_kernel  over the flagged rows, K1 = 0, no bias: P at the representatives' rows (gemm.hip);
//   4. dedup_expand_kernel   q_r = P[u(r)] + c_r W_c^T + b_f for every kept row (multiply-adds in k order, then the bias),
//                            zeros for id 0; it also hands the table back clean (the owner row of each slot clears it),
//                            so nothing is cleared per batch: the table is zeroed once, when its buffer is allocated.
//                            Memory-bound (R g floats written, the distinct P rows read): a workgroup takes the compact
//                            weight block and its rows' rep / slot / context values in ONE round trip, then every wave
//                            has all the P loads of its four rows in flight together, 8 bytes per lane where the rows
//                            are 8-byte aligned (g = 450: rows are never 16-byte aligned).
// Results are the same bits run to run and in a graph replay (nothing depends on timing), and the same between a dense
// batch and the attribute table (the same groups: equal ids carry equal bytes).
//
// With a per-item cache (CarcaFeatCache) P[i] outlives the batch: an evaluation epoch is hundreds of batches
// over one catalogue and W_a is frozen for all of it.  The same four launches:
//   2. a row whose item's entry is FILLED compares its bytes with the entry's copy of the attribute row it was computed
//      from (dense batches; rows gathered from the cache's table need no compare): equal = a HIT, rep = -2 - id, nothing to
//      multiply; different = the row goes on as if there were no cache (the entry is never overwritten).  g merges into
//      its slot's owner r0 only on equal bytes and r0 hits only on the entry's bytes, so a member of a hit owner hits and
//      a member that missed never merges into a hit owner.  The owner of a slot whose entry is EMPTY is marked for
//      publishing.  need = flag && !hit is what launch 3 plans from, and their number goes to a device word;
//   3. returns at its top where that word reads 0;
//   4. takes P from the batch scratch or from the cache according to rep, and a wave copies each of its rows that is marked
//      into the cache: the P row as loaded, the attribute row (dense), then state = 1.  Publishing writes only entries
//      that were empty when launch 2 ran and hits read only entries that were filled then: nothing is read and written
//      in one launch.
// A row's P bits are then those of the batch that first computed it (another cut of the K sums; the same for equal call
// sequences).
//
// Where the cache keeps attribute rows (dense batches), launch 2's time is the bytes it requests, and the rows of one item
// all ask for the same entry.  So launch 1 also ranks the rows of each table slot (a third table array counts them; rank
// [R] and the rows of the first DD_LIST ranks go to the per-launch scratch), and in launch 2 the row of every DD_GROUP-th
// rank of a FILLED entry compares its own bytes and those of the next ranks' rows with one read of the entry, and writes
// for each of them what that row's wave would have written; the other listed rows leave at once.  Every wave decides
// which of the three it is from what launch 1 wrote and from `state`: nobody waits for anybody, and which row took which
// rank changes no result.  A row's `slot` is the one word launch 2 reads and writes, so only the row's own wave writes
// it.  Rows past the list, rows of an empty entry, the table path and a launch without a cache run the code above
// (launches without ranks in an instantiation of launch 2 that holds nothing else).
#include <hip/hip_ext.h>

#include <vector>

#include "carca_common.h"
#include "../../include/carca_hip.h"

namespace {

constexpr int EXP_ROWS = 16;      // rows per expand workgroup (4 per wave, all in flight together)
constexpr int EXP_MAX_N = 1024;   // output columns the expand kernel keeps W_c / b_f of in LDS
constexpr int EXP_MAX_K1 = 8;
constexpr int EXP_WB4 = ((EXP_MAX_K1 + 1) * EXP_MAX_N / 4 + 255) / 256;  // 16-byte pieces of the weight block per thread
// floats of the compact weight block [K1 + 1][N] (rows 0 .. K1-1: W_c^T, row K1: b_f), padded to whole 16-byte pieces
__host__ __device__ inline int exp_wb_floats(int K1, int N) { return ((K1 + 1) * N + 3) / 4 * 4; }
// the hit compare of a batch against a filled cache (round 20): the rows of a table slot are ranked by the insert launch, the
// first DD_LIST ranks are listed, and the row of every DD_GROUP-th rank compares its group with one read of the entry
constexpr int DD_LIST = 16;
constexpr int DD_GROUP = 4;
static_assert(DD_LIST % DD_GROUP == 0 && DD_GROUP <= 8, "a leader's ranks stay inside the list");

__device__ __forceinline__ int dd_seg(const CarcaDedupRun& a, int g) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < CARCA_MAX_SEGS; ++i)
    if (i < a.nseg && g >= a.row0[i]) s = i;
  return s;
}
__device__ __forceinline__ const float* dd_a0_row(const CarcaDedupRun& a, int s, int r) {
  const CarcaGemmSeg& sg = a.d.seg[s];
  if (sg.a0_gather) return sg.a0 + (size_t)sg.ids[r] * a.d.lda0;
  if (sg.a0_bstride) return sg.a0 + (size_t)(r / sg.T) * sg.a0_bstride + (size_t)(r % sg.T) * a.d.lda0;
  return sg.a0 + (size_t)r * a.d.lda0;
}

__global__ __launch_bounds__(256) void dedup_insert_kernel(const CarcaDedupRun a) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  {  // the expand launch's weight block: one strided element per thread here instead of all of them per workgroup there
    const int N = a.d.N, K1 = a.d.K1, nw = exp_wb_floats(K1, N);
    for (int i = g; i < nw; i += gridDim.x * 256) {
      const int k = i / N, n = i - k * N;
      a.wcb[i] = k < K1 ? a.d.bt1[(size_t)n * a.d.ldb1 + k] : (k == K1 && a.d.bias ? a.d.bias[n] : 0.f);
    }
  }
  if (g == 0 && a.cnt) a.cnt[0] = 0;  // (the resolve launch counts the rows the product has to multiply into it)
  if (g >= a.R) return;
  const int s = dd_seg(a, g);
  const int id = a.d.seg[s].ids[g - a.row0[s]];
  int h = -1;
  if (id != 0) {
    unsigned hh = ((unsigned)id * 0x9E3779B1u) >> (32 - a.hbits);
    for (;;) {  // (the table holds 2x the rows: a free slot is always found)
      const int k = atomicCAS(&a.key[hh], 0, id);
      if (k == 0 || k == id) break;
      hh = (hh + 1) & a.hmask;
    }
    atomicMax(&a.val[hh], 0xFFFFFFFFu - (unsigned)g);  // (max of ~row = the lowest row)
    h = (int)hh;
    if (a.cnt_slot) {  // the row's rank among its slot's rows: which row takes which depends on timing, no result does
      const int k = atomicAdd(&a.cnt_slot[hh], 1);
      a.rank[g] = k;
      if (k < DD_LIST) a.mem[(size_t)hh * DD_LIST + k] = g;
    }
  }
  a.slot[g] = h;
}

// whether two rows of K 32-bit words differ, by one wave (integer compare: -0.0 / +0.0 and NaN payloads differ)
// VEC: both rows 16-byte aligned and K % 4 == 0
template <bool VEC>
__device__ __forceinline__ bool dd_rows_differ(const unsigned* p, const unsigned* q, const int K, const int lane) {
  bool diff = false;
  if constexpr (VEC) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    // 4 KB of each row per round (4 loads per lane and row in flight), a vote after each
    for (int k0 = 0; k0 < K && !diff; k0 += 1024) {
      u4 x[4], y[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + (u * 64 + lane) * 4;
        x[u] = k < K ? *reinterpret_cast<const u4*>(p + k) : u4{0, 0, 0, 0};
        y[u] = k < K ? *reinterpret_cast<const u4*>(q + k) : u4{0, 0, 0, 0};
      }
      bool d = false;
#pragma unroll
      for (int u = 0; u < 4; ++u) d = d || x[u][0] != y[u][0] || x[u][1] != y[u][1] || x[u][2] != y[u][2] || x[u][3] != y[u][3];
      diff = __ballot(d) != 0;
    }
  } else {
    for (int k0 = 0; k0 < K && !diff; k0 += 256) {
      bool d = false;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 64 + lane;
        if (k < K) d = d || p[k] != q[k];
      }
      diff = __ballot(d) != 0;
    }
  }
  return diff;
}

// which of the rows p[0 .. n-1] differ from row q (bit j: row j), by one wave: q's words are loaded ONCE per round and every
// row's round is in flight with them; a row that differed is not read further.  2 KB per row and round (VEC), so that
// DD_GROUP rows and the entry stay inside the registers of eight waves per SIMD.
template <bool VEC>
__device__ __forceinline__ unsigned dd_group_differ(const unsigned* const (&p)[DD_GROUP], const int n, const unsigned* q,
                                                    const int K, const int lane) {
  unsigned diff = 0;
  const unsigned all = (1u << n) - 1u;
  if constexpr (VEC) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    constexpr int RU = 2;
    for (int k0 = 0; k0 < K && diff != all; k0 += RU * 256) {
      u4 y[RU], x[DD_GROUP][RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int k = k0 + (u * 64 + lane) * 4;
        y[u] = k < K ? *reinterpret_cast<const u4*>(q + k) : u4{0, 0, 0, 0};
      }
#pragma unroll
      for (int j = 0; j < DD_GROUP; ++j) {
        const bool on = j < n && !((diff >> j) & 1u);
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          const int k = k0 + (u * 64 + lane) * 4;
          x[j][u] = on && k < K ? __builtin_nontemporal_load(reinterpret_cast<const u4*>(p[j] + k)) : u4{0, 0, 0, 0};
        }
      }
#pragma unroll
      for (int j = 0; j < DD_GROUP; ++j) {
        const bool on = j < n && !((diff >> j) & 1u);
        bool d = false;
#pragma unroll
        for (int u = 0; u < RU; ++u)
          d = d || x[j][u][0] != y[u][0] || x[j][u][1] != y[u][1] || x[j][u][2] != y[u][2] || x[j][u][3] != y[u][3];
        if (on && __ballot(d) != 0) diff |= 1u << j;
      }
    }
  } else {
    for (int k0 = 0; k0 < K && diff != all; k0 += 256) {
      bool d[DD_GROUP];
#pragma unroll
      for (int j = 0; j < DD_GROUP; ++j) d[j] = false;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 64 + lane;
        if (k < K) {
          const unsigned y = q[k];
#pragma unroll
          for (int j = 0; j < DD_GROUP; ++j)
            if (j < n && !((diff >> j) & 1u)) d[j] = d[j] || p[j][k] != y;
        }
      }
#pragma unroll
      for (int j = 0; j < DD_GROUP; ++j)
        if (j < n && __ballot(d[j]) != 0) diff |= 1u << j;
    }
  }
  return diff;
}

// whether row g merges into its slot's owner r0 (another row): rows of one table under one id are one row, else by bytes
template <bool VEC>
__device__ __forceinline__ bool dd_merges(const CarcaDedupRun& a, const int g, const int r0, const int lane) {
  const int s = dd_seg(a, g), t = dd_seg(a, r0);
  const CarcaGemmSeg &sg = a.d.seg[s], &tg = a.d.seg[t];
  if (sg.a0_gather && tg.a0_gather && sg.a0 == tg.a0) return true;  // (one table, one id: one row)
  const unsigned* p = reinterpret_cast<const unsigned*>(dd_a0_row(a, s, g - a.row0[s]));
  const unsigned* q = reinterpret_cast<const unsigned*>(dd_a0_row(a, t, r0 - a.row0[t]));
  return !dd_rows_differ<VEC>(p, q, a.d.K0, lane);
}

// what the resolve launch leaves of kept row g (one lane): its representative and the flags the product plans from
__device__ __forceinline__ void dd_write_row(const CarcaDedupRun& a, const int g, const int r0, const int ci, const bool filled,
                                             const bool hit, const bool merge) {
  // (a hit that does not own the slot counts as merged: its owner hit too unless the owner carries other bytes)
  a.rep[g] = hit ? -2 - ci : (merge ? r0 : g);
  a.flag[g] = hit ? (r0 == g ? 1 : 0) : (merge ? 0 : 1);
  if (a.cache.state) {
    const int need = !hit && !merge;
    a.need[g] = need;
    a.pub[g] = r0 == g && ci > 0 && !filled ? ci : 0;  // (the owner is its own representative: P[g] is computed)
    if (need) atomicAdd(a.cnt, 1);
  }
}

// one wave per row; VEC: every attribute row (the cache's copies included) 16-byte aligned and K0 % 4 == 0; GROUPS: the
// insert launch ranked the rows and key 22 is off -- every other launch (no cache, the table path, a cold call's empty
// entries aside) runs an instantiation without the group code: on the table path this pass is a few us of launch and
// round trips, and the group code in its way cost it 1.6 us
template <bool VEC, bool GROUPS>
__global__ __launch_bounds__(256) void dedup_resolve_kernel(const CarcaDedupRun a) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (g >= a.R) return;
  const int h = a.slot[g];
  const bool cache = a.cache.state != nullptr;
  if (h < 0) {
    if (lane == 0) {
      a.rep[g] = -1;
      a.flag[g] = 0;
      if (cache) {
        a.need[g] = 0;
        a.pub[g] = 0;
      }
      if (a.grp) a.grp[g] = 0;
    }
    return;
  }
  // (ranks exist only under a cache that keeps attribute rows, and only for rows with an id)
  int rk = DD_LIST;
  if constexpr (GROUPS) rk = a.rank[g];
  const int r0 = (int)(0xFFFFFFFFu - a.val[h]);
  const int s = dd_seg(a, g);
  const CarcaGemmSeg& sg = a.d.seg[s];
  // the cache entry of this row's item: ci > 0 where it has one, filled or empty
  int ci = 0;
  bool filled = false, hit = false, from_table = false;
  if (cache) {
    const int id = __builtin_amdgcn_readfirstlane(a.key[h]);
    from_table = sg.a0_gather && sg.a0 == a.cache.table;
    if (id > 0 && id < a.cache.n_rows && (a.cache.a_c || from_table)) {
      ci = id;
      filled = a.cache.state[id] == 1;
    }
    // A GROUPED row: filled entry, ranked, rank inside the list.  Every row of the slot decides this from what the insert
    // launch left (slot, key, rank) and from state, which nobody writes during this launch, and all rows of a slot carry one
    // id: they agree.  The row of every DD_GROUP-th rank compares for the ranks up to the next one; the others leave.
    if (GROUPS && filled && rk < DD_LIST) {
      if (rk % DD_GROUP == 0) {
        const int n = min(min(a.cnt_slot[h], DD_LIST) - rk, DD_GROUP);  // (>= 1: this row)
        int m[DD_GROUP];
        const unsigned* p[DD_GROUP];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < DD_GROUP; ++j) {
          m[j] = j > 0 && j < n ? __builtin_amdgcn_readfirstlane(a.mem[(size_t)h * DD_LIST + rk + j]) : g;
          if ((unsigned)m[j] >= (unsigned)a.R) {  // no row of this batch: the list is corrupt.  Nothing is read or written
            bad = true;                           // out of bounds (the entry counts as this row again) and the host is
            m[j] = g;                             // told: the rows the list should have named keep no outputs
          }
          const int t = dd_seg(a, m[j]);
          p[j] = reinterpret_cast<const unsigned*>(dd_a0_row(a, t, m[j] - a.row0[t]));
        }
        if (bad && lane == 0 && a.err) *a.err = 4;  // (reported by carca_poll_errors and the next stream-K launch)
        const unsigned* q = reinterpret_cast<const unsigned*>(a.cache.a_c + (size_t)ci * a.cache.ld_a);
        const unsigned diff = dd_group_differ<VEC>(p, n, q, a.d.K0, lane);
#pragma unroll 1
        for (int j = 0; j < n; ++j) {
          int mj = g;
#pragma unroll
          for (int i = 1; i < DD_GROUP; ++i)
            if (j == i) mj = m[i];
          const bool hj = !((diff >> j) & 1u);
          bool merge = false;
          if (!hj && r0 != mj) merge = dd_merges<VEC>(a, mj, r0, lane);  // (a changed row under a cached id: rare)
          if (lane == 0) {
            dd_write_row(a, mj, r0, ci, true, hj, merge);
            a.grp[mj] = 1;
          }
        }
      }
      // (its own wave alone writes a row's slot: that wave reads it at its top)
      if (lane == 0 && r0 != g) a.slot[g] = -1;
      return;
    }
    if (filled) {
      if (a.cache.a_c) {
        const unsigned* p = reinterpret_cast<const unsigned*>(dd_a0_row(a, s, g - a.row0[s]));
        const unsigned* q = reinterpret_cast<const unsigned*>(a.cache.a_c + (size_t)ci * a.cache.ld_a);
        hit = !dd_rows_differ<VEC>(p, q, a.d.K0, lane);
      } else {
        hit = true;  // (the table the entry was computed from, the same id: the same row)
      }
    }
  }
  bool merge = false;
  if (!hit && r0 != g) merge = dd_merges<VEC>(a, g, r0, lane);
  if (lane == 0) {
    dd_write_row(a, g, r0, ci, filled, hit, merge);
    if (a.grp) a.grp[g] = 0;
    if (r0 != g) a.slot[g] = -1;  // (the slot stays with its owner, the lowest row: the expand kernel clears it)
  }
}

// what the expand kernel needs of a row's segment, picked with constant indices (a per-lane index into the kernel
// arguments would be a memory round trip of its own)
struct DdRowSeg {
  const float* a1;
  float* c;
  long a1_bstride;
  int T, r;
};
__device__ __forceinline__ DdRowSeg dd_row_seg(const CarcaDedupRun& a, int g) {
  DdRowSeg o{a.d.seg[0].a1, a.d.seg[0].c, a.d.seg[0].a1_bstride, a.d.seg[0].T, g};
#pragma unroll
  for (int i = 1; i < CARCA_MAX_SEGS; ++i)
    if (i < a.nseg && g >= a.row0[i]) o = DdRowSeg{a.d.seg[i].a1, a.d.seg[i].c, a.d.seg[i].a1_bstride, a.d.seg[i].T, g - a.row0[i]};
  return o;
}

// VW: floats per access (2: N, ldc, ldp even and every output segment 8-byte aligned)
template <int VW>
__global__ __launch_bounds__(256) void dedup_expand_kernel(const CarcaDedupRun a) {
  typedef float vec __attribute__((ext_vector_type(VW)));
  typedef float f4 __attribute__((ext_vector_type(4)));
  // the weight block [K1 + 1][N] | context values [EXP_ROWS][8] | representatives [EXP_ROWS] | ids to publish under [EXP_ROWS]
  extern __shared__ f4 exp_lds[];
  carca_warm_kernargs<sizeof(CarcaDedupRun)>();
  const int N = a.d.N, K1 = a.d.K1, nw4 = exp_wb_floats(K1, N) / 4;
  float* Ws = reinterpret_cast<float*>(exp_lds);
  float* cxs = Ws + nw4 * 4;
  int* reps = reinterpret_cast<int*>(cxs + EXP_ROWS * EXP_MAX_K1);
  int* pubs = reps + EXP_ROWS;
  const bool cache = a.cache.state != nullptr;
  const int tid = threadIdx.x, g0 = blockIdx.x * EXP_ROWS;
  // one round trip: the weight block, the rows' context values (thread = row, k), rep and slot (thread = row)
  f4 w[EXP_WB4];
  const f4* wcb4 = reinterpret_cast<const f4*>(a.wcb);
#pragma unroll
  for (int j = 0; j < EXP_WB4; ++j) {
    const int i = tid + j * 256;
    if (i < nw4) w[j] = wcb4[i];
  }
  if (tid < EXP_ROWS * EXP_MAX_K1) {
    const int row = tid / EXP_MAX_K1, k = tid % EXP_MAX_K1, g = g0 + row;
    float cv = 0.f;
    if (g < a.R && k < K1) {
      const DdRowSeg sg = dd_row_seg(a, g);
      const float* cr = sg.a1_bstride ? sg.a1 + (size_t)(sg.r / sg.T) * sg.a1_bstride + (size_t)(sg.r % sg.T) * a.d.lda1
                                      : sg.a1 + (size_t)sg.r * a.d.lda1;
      cv = cr[k];
    }
    cxs[tid] = cv;
  } else if (tid < EXP_ROWS * EXP_MAX_K1 + EXP_ROWS) {
    const int row = tid - EXP_ROWS * EXP_MAX_K1, g = g0 + row;
    // (-2: past the last row, -1: id 0 -- the resolve kernel wrote rep = -1 there and P has no such row; below -2: row
    // -2 - u of the cache)
    int u = -2, pb = 0;
    if (g < a.R) {
      u = a.rep[g];
      if (cache) pb = a.pub[g];
      const int h = a.slot[g];
      if (h >= 0) {  // (nobody reads the table after the resolve kernel)
        a.key[h] = 0;
        a.val[h] = 0u;
        if (a.cnt_slot) a.cnt_slot[h] = 0;
      }
    }
    reps[row] = u;
    pubs[row] = pb;
  }
#pragma unroll
  for (int j = 0; j < EXP_WB4; ++j) {
    const int i = tid + j * 256;
    if (i < nw4) exp_lds[i] = w[j];
  }
  __syncthreads();
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int RW = EXP_ROWS / 4, CH = 4;  // rows per wave; 64-lane column chunks in flight per row
  const int nv = N / VW;                    // (VW = 2: N is even)
  int u[RW], pb[RW];
  vec* crow[RW];
  const vec* prow[RW];
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    const int row = wave * RW + i;
    u[i] = __builtin_amdgcn_readfirstlane(reps[row]);
    pb[i] = __builtin_amdgcn_readfirstlane(pubs[row]);
    const DdRowSeg sg = dd_row_seg(a, min(g0 + row, a.R - 1));
    crow[i] = reinterpret_cast<vec*>(sg.c + (size_t)sg.r * a.d.ldc);
    prow[i] = reinterpret_cast<const vec*>(u[i] < -2 ? a.cache.p_c + (size_t)(-2 - u[i]) * a.cache.ld_p
                                                    : a.P + (size_t)max(u[i], 0) * a.ldp);
  }
  const vec* Wv = reinterpret_cast<const vec*>(Ws);
  for (int c0 = 0; c0 < nv; c0 += CH * 64) {
    vec v[RW][CH];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int p = c0 + c * 64 + lane;
        v[i][c] = u[i] != -1 && u[i] != -2 && p < nv ? prow[i][p] : vec(0.f);
      }
      if (pb[i] > 0) {  // (a slot's owner whose item has an empty entry: its P row as loaded)
        vec* pc = reinterpret_cast<vec*>(a.cache.p_c + (size_t)pb[i] * a.cache.ld_p);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int p = c0 + c * 64 + lane;
          if (p < nv) pc[p] = v[i][c];
        }
      }
    }
    // (k outermost: one read of W_c's row k and of the rows' context values serves all RW x CH accesses; per element
    // the multiply-adds still run in k order from P's value, then the bias)
#pragma unroll 1
    for (int k = 0; k < K1; ++k) {
      vec wk[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) wk[c] = Wv[k * nv + min(c0 + c * 64 + lane, nv - 1)];
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const float cx = cxs[(wave * RW + i) * EXP_MAX_K1 + k];
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int e = 0; e < VW; ++e) v[i][c][e] = fmaf(cx, wk[c][e], v[i][c][e]);
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int p = c0 + c * 64 + lane;
      const vec b = Wv[K1 * nv + min(p, nv - 1)];
#pragma unroll
      for (int i = 0; i < RW; ++i)
        if (u[i] != -2 && p < nv) crow[i][p] = u[i] != -1 ? v[i][c] + b : vec(0.f);
    }
  }
  // publishing: the attribute row each marked row's P was computed from (dense batches), then the entry counts as filled
  if (cache) {
#pragma unroll 1
    for (int i = 0; i < RW; ++i) {
      if (pb[i] <= 0) continue;
      if (a.cache.a_c) {
        const int g = g0 + wave * RW + i, s = dd_seg(a, g);
        const float* src = dd_a0_row(a, s, g - a.row0[s]);
        float* dst = a.cache.a_c + (size_t)pb[i] * a.cache.ld_a;
        if (a.vec) {
          const f4* s4 = reinterpret_cast<const f4*>(src);
          f4* d4 = reinterpret_cast<f4*>(dst);
          for (int k = lane; k < a.d.K0 / 4; k += 64) d4[k] = s4[k];
        } else {
          for (int k = lane; k < a.d.K0; k += 64) dst[k] = src[k];
        }
      }
      if (lane == 0) a.cache.state[pb[i]] = 1;
    }
  }
}

// the last eager launch of this thread, for carca_feat_dedup_rows_multiplied: where its flags lie in the stream's scratch
struct DdLast {
  hipStream_t stream;
  size_t bytes, flag_off, need_off;  // (need_off = flag_off without a cache: every flagged row is multiplied)
  int R;
  size_t grp_off;  // (0: the launch ranked no rows)
};
thread_local DdLast g_dd_last{nullptr, 0, 0, 0, 0, 0};

}  // namespace

int carca_feat_dedup_prepare(const CarcaGemmDesc* desc, hipStream_t stream, CarcaDedupRun* run) {
  const CarcaGemmDesc& D = *desc;
  if (D.K1 > EXP_MAX_K1 || D.N > EXP_MAX_N || D.ncols_out != D.N || (D.alpha != 0.f && D.alpha != 1.f) || !D.mask_rows ||
      (D.K1 > 0 && !D.bt1))
    return 1;
  CarcaDedupRun& a = *run;
  a = CarcaDedupRun{};
  a.d = D;
  a.nseg = D.nseg;
  long R = 0;
  bool vec = D.K0 % 4 == 0 && D.lda0 % 4 == 0;
  for (int s = 0; s < D.nseg; ++s) {
    const CarcaGemmSeg& sg = D.seg[s];
    if (!sg.ids || sg.add || sg.gate || sg.rowscale || sg.add_pos) return 1;
    if (a.d.seg[s].T < 1) a.d.seg[s].T = 1;
    vec = vec && ((uintptr_t)sg.a0 & 15) == 0 && sg.a0_bstride % 4 == 0;
    a.row0[s] = (int)R;
    R += sg.rows;
  }
  for (int s = D.nseg; s <= CARCA_MAX_SEGS; ++s) a.row0[s] = (int)R;
  if (R < 1 || R > (1l << 28)) return 1;
  a.R = (int)R;
  a.vec = vec ? 1 : 0;
  int hb = 12;
  while ((1l << hb) < 2 * R) ++hb;
  a.hbits = hb;
  a.hmask = (1u << hb) - 1;
  a.ldp = D.N;
  // 8-byte accesses in the expand launch: every q row and P row 8-byte aligned (g = 450: never 16)
  bool vec2 = D.N % 2 == 0 && D.ldc % 2 == 0;
  for (int s = 0; s < D.nseg; ++s) vec2 = vec2 && ((uintptr_t)D.seg[s].c & 7) == 0;
  a.vec2 = vec2 ? 1 : 0;
  const bool cap = carca_stream_capturing(stream);
  // the per-item cache armed for this forward: never under capture (a replay would publish into memory the graph does not
  // own) and never with tuning key 21 = 1
  // ... and never while a knob of the product's kernel is off its default: a tuning or diagnostic run is about that
  // kernel (stamps, hand-over bounds, a withheld flag), and a launch with nothing to multiply would tell it nothing
  bool knobs = false;
  for (int k : {CARCA_TUNE_GEMM_VARIANT, CARCA_TUNE_STAMPS, CARCA_TUNE_CU_CAP, CARCA_TUNE_SK_DON, CARCA_TUNE_SK_SPIN_LOG2,
                CARCA_TUNE_SK_WITHHOLD, CARCA_TUNE_DIAG, CARCA_TUNE_SKC_OV_TEAM, CARCA_TUNE_SKC_OV_LONE,
                CARCA_TUNE_SKC_MIN_STEPS})
    knobs = knobs || carca_tuning(k) != 0;
  CarcaFeatCache fc;
  const bool cached = carca_take_feat_cache(&fc) && !cap && !knobs && carca_tuning(CARCA_TUNE_FEAT_CACHE) != 1 &&
                      fc.ld_p >= D.N && (!fc.a_c || fc.ld_a >= D.K0);
  if (cached) {
    a.cache = fc;
    if (fc.a_c && (((uintptr_t)fc.a_c & 15) != 0 || fc.ld_a % 4 != 0)) a.vec = 0;
    if (((uintptr_t)fc.p_c & 7) != 0 || fc.ld_p % 2 != 0) a.vec2 = 0;
  }
  // the table (zeroed when allocated, kept clean by the expand kernel) and the per-launch arrays + weight block + P.
  // The table always has room for its third array, the per-slot row counts: every launch on a stream shares one buffer
  // whatever its hbits, so all of it has to be clean between launches -- which is why the slots' row lists, which nobody
  // clears, lie with the per-launch arrays (behind them: flag_off / need_off stay where they were).
  const bool ranked = cached && fc.a_c != nullptr;
  a.solo = carca_tuning(CARCA_TUNE_DEDUP_SOLO) == 1 ? 1 : 0;
  const size_t hbytes = (size_t)3 * sizeof(int) << hb;
  const size_t nints = (size_t)(cached ? 5 * R + 1 : 3 * R) + (ranked ? (size_t)2 * R + ((size_t)DD_LIST << hb) : 0);
  const size_t ibytes = (nints * sizeof(int) + 255) / 256 * 256;
  const size_t wbytes = ((size_t)exp_wb_floats(D.K1, D.N) * sizeof(float) + 255) / 256 * 256;
  const size_t bytes = ibytes + wbytes + (size_t)R * a.ldp * sizeof(float);
  char* ht = (char*)(cap ? carca_capture_alloc(stream, hbytes, false, nullptr, hbytes)
                         : carca_stream_scratch(stream, CARCA_SCRATCH_DEDUP_HASH, hbytes, hbytes));
  char* buf = (char*)(cap ? carca_capture_alloc(stream, bytes, false, nullptr)
                          : carca_stream_scratch(stream, CARCA_SCRATCH_DEDUP, bytes));
  if (!ht || !buf) return (int)hipErrorOutOfMemory;
  a.key = (int*)ht;
  a.val = (unsigned*)(ht + ((size_t)sizeof(int) << hb));
  a.slot = (int*)buf;
  a.rep = a.slot + R;
  a.flag = a.rep + R;
  if (cached) {
    a.need = a.flag + R;
    a.pub = a.need + R;
    a.cnt = a.pub + R;
  }
  if (ranked) {
    a.err = carca_kernel_error_word();
    a.cnt_slot = (int*)(ht + ((size_t)2 * sizeof(int) << hb));
    a.rank = a.cnt + 1;
    a.grp = a.rank + R;
    a.mem = a.grp + R;
  }
  a.wcb = (float*)(buf + ibytes);
  a.P = (float*)(buf + ibytes + wbytes);
  g_dd_last = cap ? DdLast{nullptr, 0, 0, 0, 0}
                  : DdLast{stream, bytes, (size_t)2 * R * sizeof(int), (size_t)(cached ? 3 : 2) * R * sizeof(int), a.R,
                           ranked ? (size_t)(6 * R + 1) * sizeof(int) : 0};
  return CARCA_OK;
}

// launches 1 and 2; `start` (or null) bound to the first one's dispatch
int carca_feat_dedup_plan(const CarcaDedupRun* run, hipStream_t stream, hipEvent_t start) {
  const CarcaDedupRun& a = *run;
  const dim3 gi((a.R + 255) / 256), gr((a.R + 3) / 4);
  if (start)
    hipExtLaunchKernelGGL(dedup_insert_kernel, gi, dim3(256), 0, stream, start, nullptr, 0, a);
  else
    hipLaunchKernelGGL(dedup_insert_kernel, gi, dim3(256), 0, stream, a);
  CARCA_LAUNCH_CHECK();
  const bool groups = a.rank != nullptr && !a.solo;
  auto kern = a.vec ? (groups ? dedup_resolve_kernel<true, true> : dedup_resolve_kernel<true, false>)
                    : (groups ? dedup_resolve_kernel<false, true> : dedup_resolve_kernel<false, false>);
  hipLaunchKernelGGL(kern, gr, dim3(256), 0, stream, a);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// launch 4; `stop` (or null) bound to its dispatch
int carca_feat_dedup_expand(const CarcaDedupRun* run, hipStream_t stream, hipEvent_t stop) {
  const CarcaDedupRun& a = *run;
  const dim3 ge((a.R + EXP_ROWS - 1) / EXP_ROWS);
  const size_t lds = ((size_t)exp_wb_floats(a.d.K1, a.d.N) + EXP_ROWS * EXP_MAX_K1 + 2 * EXP_ROWS) * sizeof(float);
  auto kern = a.vec2 ? dedup_expand_kernel<2> : dedup_expand_kernel<1>;
  if (stop)
    hipExtLaunchKernelGGL(kern, ge, dim3(256), lds, stream, nullptr, stop, 0, a);
  else
    hipLaunchKernelGGL(kern, ge, dim3(256), lds, stream, a);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// Rows of this thread's last eager dedup launch with a set entry in the int array at `off` of its scratch, read back after
// the launch's stream has drained; -1: no such launch (none yet, or the last one was captured).
static long long dd_count_last(size_t DdLast::*off) {
  const DdLast l = g_dd_last;
  if (!l.R) return -1;
  // (the same request as the launch's: the stream's buffer as it stands, not a pointer kept past a release)
  const char* buf = (const char*)carca_stream_scratch(l.stream, CARCA_SCRATCH_DEDUP, l.bytes);
  if (!buf) return -1;
  std::vector<int> flag(l.R);
  if (hipMemcpyAsync(flag.data(), buf + l.*off, (size_t)l.R * sizeof(int), hipMemcpyDeviceToHost, l.stream) != hipSuccess ||
      hipStreamSynchronize(l.stream) != hipSuccess)
    return -1;
  long long n = 0;
  for (int f : flag) n += f != 0;
  return n;
}

// The launch's flagged rows: one per group of equal attribute rows of the batch, whether the product multiplied it or the
// cache supplied it (a hit that does not own its id's slot counts as merged).  For tests: a table that is not handed
// back clean shows here (rows that no longer merge), never in q.
extern "C" long long carca_feat_dedup_rows_multiplied(void) { return dd_count_last(&DdLast::flag_off); }
// ... and the rows the product multiplied: the flagged rows that no cache entry served.
extern "C" long long carca_feat_dedup_rows_computed(void) { return dd_count_last(&DdLast::need_off); }
// ... and the rows whose compare with their cache entry the row of a group's first rank issued, that row included; 0 where
// the launch ranked no rows (no cache, the attribute-table path, a captured launch, none yet).
extern "C" long long carca_feat_dedup_rows_grouped(void) {
  return g_dd_last.grp_off ? dd_count_last(&DdLast::grp_off) : 0;
}
