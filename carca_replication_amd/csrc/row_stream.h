// The streaming row-product kernel: S = Q X^T for a zero-padded buffer Q of query rows and a row table X, shared by the
// KNN baseline's full-catalogue calls (knn_catalogue.hip) and similar_items for rows wider than 128
// (similar_items.hip; section 17), with the padded row gather that fills Q.  Each 64-lane wave owns 16 table rows x 64
// query rows; both operands are re-read from global memory at every 64-byte step through sized buffer resources (16
// bytes per lane, the wave-uniform base carrying the 64-bit row offset, loads past the last row returning 0).  An
// element policy says how a chunk is loaded and multiplied; an epilogue policy, passed by value, what becomes of a tile:
//   struct Epilogue { struct Shared;                       // declared in LDS by the kernel
//     void stage(int q0, Shared&) const;                   // before the loop, by every thread of the workgroup
//     void store(const f32x4 (&tile)[MQ], int q0, int column, int g, const Shared&) const; };
// `tile` holds column (table row) `column`, rows (queries) q0 + 16m + 4g .. + 3 of each 16-query block m.
#pragma once
#include "carca_common.h"

namespace rs {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MQ = 4;             // 16-query blocks per wave
constexpr int QB = 16 * MQ;       // query rows per workgroup (and the row padding of the query buffer)
constexpr int TB = 16 * WAVES;    // table rows per workgroup: 16 per wave
constexpr int UNROLL = 4;         // 64-byte row chunks in flight per operand
constexpr int FOLD = 16;          // fp32: chunks per MFMA chain (a multiple of UNROLL)

typedef int i32x4 __attribute__((ext_vector_type(4)));

// carca_rsrc over `bytes` bytes only: loads past the end return 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// the lane's four k of chunk c, zero where k >= cols (lim = cols - 4g)
__device__ __forceinline__ f32x4 mask4(u32x4 v, int c, int lim) {
  f32x4 f;
#pragma unroll
  for (int j = 0; j < 4; ++j) f[j] = (16 * c + j < lim) ? __uint_as_float(v[j]) : 0.f;
  return f;
}

struct Operands {
  const void* table;  // [rows, ld] elements
  int ld;
  const void* q;  // [nqb * QB, ldq] query rows, zero past `cols` and in the rows past the last query
  int ldq;
  int rows, cols;  // live table rows; live columns
  int nchunks;     // 64-byte chunks of a query row
  int nqb;         // query blocks
};

// ---- element policies: load_t is chunk c of the lane's table row (t_off = its byte offset at chunk 0) -----------
struct F32Aligned {  // rows 16-byte aligned: one b128 load
  typedef f32x4 V;
  static constexpr int ES = 4;
  static constexpr bool FOLDS = true;
  static __device__ __forceinline__ V as(u32x4 v) {
    return (V){__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
  }
  static __device__ __forceinline__ V load_t(__amdgpu_buffer_rsrc_t tr, int t_off, int c, int lim) {
    return mask4(__builtin_amdgcn_raw_buffer_load_b128(tr, t_off, c * 64, 0), c, lim);
  }
  // k = 16c + 4g + s at step s, the same permutation for both operands
  static __device__ __forceinline__ V mma(V a, V b, V c) { return mfma16_group(a, b, c); }
};
struct F32Unaligned : F32Aligned {  // any stride: four b32 loads
  static __device__ __forceinline__ V load_t(__amdgpu_buffer_rsrc_t tr, int t_off, int c, int lim) {
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __builtin_amdgcn_raw_buffer_load_b32(tr, t_off + (16 * c + j) * 4, 0, 0);
    return mask4(v, c, lim);
  }
};
struct I8 {  // i32 accumulation, converted once: no fold, and the padding bytes of both operands are zero
  typedef i32x4 V;
  static constexpr int ES = 1;
  static constexpr bool FOLDS = false;
  static __device__ __forceinline__ V as(u32x4 v) { return (V){(int)v[0], (int)v[1], (int)v[2], (int)v[3]}; }
  static __device__ __forceinline__ V load_t(__amdgpu_buffer_rsrc_t tr, int t_off, int c, int) {
    return as(__builtin_amdgcn_raw_buffer_load_b128(tr, t_off, c * 64, 0));
  }
  static __device__ __forceinline__ V mma(V a, V b, V c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
};

// Operand chunk c of a row is its bytes 64c .. 64c + 63: lane (r = l & 15, g = l >> 4) holds bytes 64c + 16g .. +15 of
// query row r (A operand) and table row r (B operand).
template <class E, class Epilogue>
__global__ __launch_bounds__(THREADS) void score_kernel(Operands P, Epilogue epi) {
  typedef typename E::V V;
  __shared__ typename Epilogue::Shared S;
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qb = blockIdx.x % P.nqb, it = blockIdx.x / P.nqb;
  const int q0 = qb * QB, i0 = it * TB + wave * 16;
  epi.stage(q0, S);  // (may end in a barrier: before anything that depends on the wave)
  const int lim = P.cols - 4 * g;
  const int rows = max(0, min(16, P.rows - i0));  // live table rows of this wave
  // wave-uniform bases carry the 64-bit row offsets; lane offsets stay below 16 table rows and 64 query rows
  const auto tr = rsrc((const char*)P.table + (size_t)i0 * P.ld * E::ES, (unsigned)rows * P.ld * E::ES);
  const auto qr = rsrc((const char*)P.q + (size_t)q0 * P.ldq * E::ES, (unsigned)QB * P.ldq * E::ES);
  const int t_off = r * P.ld * E::ES + g * 16;
  int q_off[MQ];
#pragma unroll
  for (int m = 0; m < MQ; ++m) q_off[m] = (16 * m + r) * P.ldq * E::ES + g * 16;
  auto load_t = [&](int c) -> V { return E::load_t(tr, t_off, c, lim); };
  auto load_q = [&](int m, int c) -> V { return E::as(__builtin_amdgcn_raw_buffer_load_b128(qr, q_off[m], c * 64, 0)); };
  // fp32: the MFMA chain restarts every FOLD chunks (256 k) and is added into `tot`, so an output's rounding error
  // grows with two short sums rather than one long fmaf chain (a 4,096-long chain of positive terms: ~2e-6 relative)
  V acc[MQ];
  f32x4 tot[MQ];
#pragma unroll
  for (int m = 0; m < MQ; ++m) acc[m] = (V){0, 0, 0, 0}, tot[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto fold = [&]() {
#pragma unroll
    for (int m = 0; m < MQ; ++m) {
      if constexpr (E::FOLDS) tot[m] += acc[m], acc[m] = (V){0, 0, 0, 0};
    }
  };
  int c = 0;
  for (; c + UNROLL <= P.nchunks; c += UNROLL) {
    V t[UNROLL], q[UNROLL][MQ];
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) {
      t[j] = load_t(c + j);
#pragma unroll
      for (int m = 0; m < MQ; ++m) q[j][m] = load_q(m, c + j);
    }
#pragma unroll
    for (int j = 0; j < UNROLL; ++j)
#pragma unroll
      for (int m = 0; m < MQ; ++m) acc[m] = E::mma(q[j][m], t[j], acc[m]);
    if ((c + UNROLL) % FOLD == 0) fold();
  }
  for (; c < P.nchunks; ++c) {
    const V t = load_t(c);
#pragma unroll
    for (int m = 0; m < MQ; ++m) acc[m] = E::mma(load_q(m, c), t, acc[m]);
  }
  fold();
  if constexpr (!E::FOLDS) {
#pragma unroll
    for (int m = 0; m < MQ; ++m) tot[m] = __builtin_convertvector(acc[m], f32x4);
  }
  epi.store(tot, q0, i0 + r, g, S);
}

// sizes the grid (query blocks fastest) and launches one instantiation
template <class E, class Epilogue>
int launch_score(const Operands& P, const Epilogue& epi, const char* what, hipStream_t stream) {
  const long long blocks = (long long)P.nqb * ((P.rows + TB - 1) / TB);
  CARCA_CHECK_SUPPORTED(blocks < (1ll << 31), "%s: %lld scoring workgroups", what, blocks);
  hipLaunchKernelGGL((score_kernel<E, Epilogue>), dim3((unsigned)blocks), dim3(THREADS), 0, stream, P, epi);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// ---- padded row gather: dst[u] = the row src(u) over the live columns, zero past them; a zero row where src(u) is NULL
template <class T, class Src>
__global__ __launch_bounds__(THREADS) void gather_kernel(Src src, int cols, T* dst, int ld_dst) {
  const int u = blockIdx.x;
  const T* row = src(u);
  T* out = dst + (size_t)u * ld_dst;
  for (int k = threadIdx.x; k < ld_dst; k += THREADS) out[k] = (row && k < cols) ? row[k] : T(0);
}

}  // namespace rs
