// The feature product of an evaluation batch over its DISTINCT attribute rows (carca_gemm_rows_feat_dedup, gemm.hip).
//
// Attribute rows are per item (data.py: p_a = attrs[p_x], o_a = attrs[o_x]), and an evaluation batch repeats items: at
// C2 the 16.2 k kept rows (id != 0) hold 8.9 k distinct ids, at C3 65 k hold 12 k.  q = [a ; c] W_f^T + b_f splits into
//     q_r = P[u(r)] + c_r W_c^T + b_f,   P = A_unique W_a^T,
// so the 4096-deep product runs over one representative row per group and the six context columns per row.  Four launches:
//   1. dedup_insert_kernel   every kept row into an open-addressing table keyed by id (2x the rows, CAS on the key):
//                            the group's representative is its LOWEST row (atomicMax of ~row), whatever the timing;
//   2. dedup_resolve_kernel  a row whose representative is another row compares the two attribute rows as 32-bit
//                            integers (dense batches; rows gathered from one table by the same id are the same row) and
//                            stays its own representative on any difference (-0.0 / +0.0, NaN payloads: never merged);
//                            writes the row's representative and the kept-row flags the product plans from;
//   3. gemm_rows_skc_kernel  over the flagged rows, K1 = 0, no bias: P at the representatives' rows (gemm.hip);
//   4. dedup_expand_kernel   q_r = P[u(r)] + c_r W_c^T + b_f for every kept row (multiply-adds in k order, then the bias),
//                            zeros for id 0; it also hands the table back clean (the owner row of each slot clears it),
//                            so nothing is cleared per batch: the table is zeroed once, when its buffer is allocated.
// Results are the same bits run to run and in a graph replay (nothing depends on timing), and the same between a dense
// batch and the attribute table (the same groups: equal ids carry equal bytes).
#include <hip/hip_ext.h>

#include "carca_common.h"
#include "../../include/carca_hip.h"

namespace {

constexpr int EXP_ROWS = 32;      // rows per expand workgroup (8 per wave)
constexpr int EXP_MAX_N = 1024;   // output columns the expand kernel keeps W_c / b_f of in LDS
constexpr int EXP_MAX_K1 = 8;

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
__device__ __forceinline__ const float* dd_a1_row(const CarcaDedupRun& a, int s, int r) {
  const CarcaGemmSeg& sg = a.d.seg[s];
  if (sg.a1_bstride) return sg.a1 + (size_t)(r / sg.T) * sg.a1_bstride + (size_t)(r % sg.T) * a.d.lda1;
  return sg.a1 + (size_t)r * a.d.lda1;
}

__global__ __launch_bounds__(256) void dedup_insert_kernel(const CarcaDedupRun a) {
  const int g = blockIdx.x * 256 + threadIdx.x;
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
  }
  a.slot[g] = h;
}

// one wave per row; VEC: every attribute row 16-byte aligned and K0 % 4 == 0
template <bool VEC>
__global__ __launch_bounds__(256) void dedup_resolve_kernel(const CarcaDedupRun a) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (g >= a.R) return;
  const int h = a.slot[g];
  if (h < 0) {
    if (lane == 0) {
      a.rep[g] = -1;
      a.flag[g] = 0;
    }
    return;
  }
  const int r0 = (int)(0xFFFFFFFFu - a.val[h]);
  bool merge = false;
  if (r0 != g) {
    const int s = dd_seg(a, g), t = dd_seg(a, r0);
    const CarcaGemmSeg &sg = a.d.seg[s], &tg = a.d.seg[t];
    merge = sg.a0_gather && tg.a0_gather && sg.a0 == tg.a0;  // (one table, one id: one row)
    if (!merge) {
      const unsigned* p = reinterpret_cast<const unsigned*>(dd_a0_row(a, s, g - a.row0[s]));
      const unsigned* q = reinterpret_cast<const unsigned*>(dd_a0_row(a, t, r0 - a.row0[t]));
      const int K = a.d.K0;
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
      merge = !diff;
    }
  }
  if (lane == 0) {
    a.rep[g] = merge ? r0 : g;
    a.flag[g] = merge ? 0 : 1;
    if (r0 != g) a.slot[g] = -1;  // (the slot stays with its owner, the lowest row: the expand kernel clears it)
  }
}

__global__ __launch_bounds__(256) void dedup_expand_kernel(const CarcaDedupRun a) {
  __shared__ float Ws[EXP_MAX_K1 * EXP_MAX_N];  // W_c transposed: [k][n]
  __shared__ float Bb[EXP_MAX_N];
  const CarcaGemmDesc& D = a.d;
  const int N = D.N, K1 = D.K1;
  for (int i = threadIdx.x; i < K1 * N; i += 256) {
    const int k = i / N, n = i - k * N;
    Ws[i] = D.bt1[(size_t)n * D.ldb1 + k];
  }
  for (int n = threadIdx.x; n < N; n += 256) Bb[n] = D.bias ? D.bias[n] : 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#pragma unroll 1
  for (int i = 0; i < EXP_ROWS / 4; ++i) {
    const int g = blockIdx.x * EXP_ROWS + i * 4 + wave;
    if (g >= a.R) break;
    const int s = dd_seg(a, g), r = g - a.row0[s];
    const CarcaGemmSeg& sg = D.seg[s];
    float* crow = sg.c + (size_t)r * D.ldc;
    if (sg.ids[r] == 0) {
      for (int n = lane; n < D.ncols_out; n += 64) crow[n] = 0.f;
      continue;
    }
    const int u = a.rep[g], h = a.slot[g];
    if (h >= 0 && lane == 0) {  // (nobody reads the table after the resolve kernel)
      a.key[h] = 0;
      a.val[h] = 0u;
    }
    float cx[EXP_MAX_K1];
    if (K1 > 0) {
      const float* cr = dd_a1_row(a, s, r);
#pragma unroll
      for (int k = 0; k < EXP_MAX_K1; ++k) cx[k] = k < K1 ? cr[k] : 0.f;
    }
    const float* prow = a.P + (size_t)u * a.ldp;
    for (int n = lane; n < N; n += 64) {
      float v = prow[n];
#pragma unroll
      for (int k = 0; k < EXP_MAX_K1; ++k)
        if (k < K1) v = fmaf(cx[k], Ws[k * N + n], v);
      crow[n] = v + Bb[n];
    }
  }
}

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
  // the table (zeroed when allocated, kept clean by the expand kernel) and the per-launch arrays + P
  const size_t hbytes = (size_t)2 * sizeof(int) << hb;
  const size_t ibytes = ((size_t)3 * R * sizeof(int) + 255) / 256 * 256;
  const size_t bytes = ibytes + (size_t)R * a.ldp * sizeof(float);
  const bool cap = carca_stream_capturing(stream);
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
  a.P = (float*)(buf + ibytes);
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
  if (a.vec)
    hipLaunchKernelGGL(dedup_resolve_kernel<true>, gr, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(dedup_resolve_kernel<false>, gr, dim3(256), 0, stream, a);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// launch 4; `stop` (or null) bound to its dispatch
int carca_feat_dedup_expand(const CarcaDedupRun* run, hipStream_t stream, hipEvent_t stop) {
  const CarcaDedupRun& a = *run;
  const dim3 ge((a.R + EXP_ROWS - 1) / EXP_ROWS);
  if (stop)
    hipExtLaunchKernelGGL(dedup_expand_kernel, ge, dim3(256), 0, stream, nullptr, stop, 0, a);
  else
    hipLaunchKernelGGL(dedup_expand_kernel, ge, dim3(256), 0, stream, a);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
