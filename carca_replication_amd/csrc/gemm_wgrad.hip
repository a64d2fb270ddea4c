// The tiled weight-gradient GEMM on v_mfma_f32_32x32x2_f32 (exact fp32):
//
//   carca_gemm_wgrad  dW[n][k] += sum_r dY[r][n] * X[r][k]                  contraction over rows
//
// gemm_wgrad produces every weight gradient except the feats_embed one where the persistent kernel takes it (wgrad_cu.hip).
//   gemm_wgrad_kernel        block tile 96 (n) x 128 (k), 32 rows per step; both operands are read from their
//                            row-major LDS tiles TRANSPOSED (lane = n resp. k), so neither dY nor X is ever transposed
//                            in memory; row splits combine through partial tiles + a reduce launch (or fp32 atomics).
//   gemm_wgrad_group_kernel  several such products in one launch.
#include "carca_common.h"
#include <vector>
#include "../../include/carca_hip.h"

namespace {


struct WgradDev {
  CarcaWgradDesc d;
  int chunk_start[CARCA_MAX_SEGS + 1];  // 32-row chunks per segment, prefix sums
  int nnb, nkb, nkb0, nsplit, chunks_per_split;
  int diag_plain_store;  // diagnostic (tuning key 3): overwrite instead of atomicAdd, to time the kernel without atomics
  // Row splits WITHOUT atomics: block (split, nb, kb) stores its 96 x 128 tile plainly, in register order, at
  // part[((split * nnb + nb) * nkb + kb) * 12288 ..] and wgrad_part_reduce adds a tile's splits in order into dw.  (A/B at
  // C2 with plain stores in place of the atomics, wrong results: train step -43 us -- an fp32 atomic costs ~5 ns and the
  // thirteen d x d products + the joint-embedding dW issue 11 M of them per step.)  NULL = atomics (grad_add).
  float* part;
};

template <int BNO, int BKO, int BR, bool BUF>
__device__ __forceinline__ void wgrad_body(const WgradDev& args, int b) {
  static_assert(BNO == 96 && BKO == 128 && BR == 32, "tile shape baked into the lane maps below");
  constexpr int NT = 256;
  __shared__ __attribute__((aligned(16))) float Ys[BR * BNO];  // dY tile [row][n]
  __shared__ __attribute__((aligned(16))) float Xs[BR * BKO];  // X  tile [row][k]

  const CarcaWgradDesc& D = args.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kb = b % args.nkb;
  b /= args.nkb;
  const int nb = b % args.nnb;
  const int split = b / args.nnb;
  const bool src1 = kb >= args.nkb0;  // this block's dW columns come from the second X source
  const int n0 = nb * BNO, k0 = (src1 ? kb - args.nkb0 : kb) * BKO;
  const int klen = src1 ? D.K1 : D.K;
  const int ldx = src1 ? D.ld_x1 : D.ld_x;
  const int c_begin = split * args.chunks_per_split;
  const int c_end = min(c_begin + args.chunks_per_split, args.chunk_start[D.nseg]);
  const bool n_full = n0 + BNO <= D.N, k_full = k0 + BKO <= klen;

  constexpr int Y4 = BNO / 4, X4 = BKO / 4;                            // float4 per tile row
  constexpr int Y_PER = BR * Y4 / NT, X_PER = BR * X4 / NT;            // 3, 4
  f32x4 ry[Y_PER], rx[X_PER];

  auto load_chunk = [&](int c) {
    int s = 0;
#pragma unroll
    for (int i = 1; i < CARCA_MAX_SEGS; ++i)
      if (i < D.nseg && c >= args.chunk_start[i]) s = i;
    const CarcaWgradSeg sg = D.seg[s];
    const int r0 = (c - args.chunk_start[s]) * BR;
#pragma unroll
    for (int i = 0; i < Y_PER; ++i) {
      const int slot = tid + i * NT;
      const int r = slot / Y4, c4 = slot - r * Y4;
      const int row = r0 + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      bool ok = row < sg.rows;
      if (ok && D.mask_rows) ok = sg.ids[row] != 0;
      if (ok) {
        const float* p = sg.dy + (size_t)row * D.ld_dy + n0 + c4 * 4;
        if (n_full) {
          if constexpr (BUF)
            v = gload4(sg.dy, row * D.ld_dy + n0 + c4 * 4);
          else
            v = *reinterpret_cast<const f32x4_u*>(p);
        } else {
          const int nn = n0 + c4 * 4;
          v[0] = nn + 0 < D.N ? p[0] : 0.f;
          v[1] = nn + 1 < D.N ? p[1] : 0.f;
          v[2] = nn + 2 < D.N ? p[2] : 0.f;
          v[3] = nn + 3 < D.N ? p[3] : 0.f;
        }
      }
      ry[i] = v;
    }
#pragma unroll
    for (int i = 0; i < X_PER; ++i) {
      const int slot = tid + i * NT;
      const int r = slot / X4, c4 = slot - r * X4;
      const int row = r0 + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < sg.rows) {
        const int64_t bs = src1 ? sg.x1_bstride : sg.x_bstride;
        const size_t roff = (!src1 && sg.x_gather) ? (size_t)sg.ids[row] * ldx
                            : bs                    ? (size_t)(row / sg.T) * bs + (size_t)(row % sg.T) * ldx
                                                    : (size_t)row * ldx;
        const float* p = (src1 ? sg.x1 : sg.x) + roff + k0 + c4 * 4;
        if (k_full) {
          if constexpr (BUF)
            v = gload4(src1 ? sg.x1 : sg.x, (int)roff + k0 + c4 * 4);
          else
            v = *reinterpret_cast<const f32x4_u*>(p);
        } else {
          const int kk = k0 + c4 * 4;
          v[0] = kk + 0 < klen ? p[0] : 0.f;
          v[1] = kk + 1 < klen ? p[1] : 0.f;
          v[2] = kk + 2 < klen ? p[2] : 0.f;
          v[3] = kk + 3 < klen ? p[3] : 0.f;
        }
      }
      rx[i] = v;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int i = 0; i < Y_PER; ++i) {
      const int slot = tid + i * NT;
      *reinterpret_cast<f32x4*>(&Ys[slot * 4]) = ry[i];
    }
#pragma unroll
    for (int i = 0; i < X_PER; ++i) {
      const int slot = tid + i * NT;
      *reinterpret_cast<f32x4*>(&Xs[slot * 4]) = rx[i];
    }
  };

  // wave w owns k columns 32w..32w+31 of the block's 128 and all three 32-wide n tiles
  f32x16 acc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;  // thread t < 96 of a kb == 0 block sums column n0 + t of dY

  const int lr = lane & 31, lh = lane >> 5;
  if (c_begin < c_end) {
    load_chunk(c_begin);
    store_chunk();
  }
  __syncthreads();
  for (int c = c_begin; c < c_end; ++c) {
    if (c + 1 < c_end) load_chunk(c + 1);
    // D[m = n index][n = k index] = sum_r Ys[r][m] * Xs[r][n]:  A lane (i, kk) = Ys[2s + kk][i]
#pragma unroll 4
    for (int st = 0; st < BR / 2; ++st) {
      const int r = 2 * st + lh;
      const float xb = Xs[r * BKO + wave * 32 + lr];
      const float y0 = Ys[r * BNO + lr], y1 = Ys[r * BNO + 32 + lr], y2 = Ys[r * BNO + 64 + lr];
      acc[0] = mfma32(y0, xb, acc[0]);
      acc[1] = mfma32(y1, xb, acc[1]);
      acc[2] = mfma32(y2, xb, acc[2]);
    }
    if (D.db && kb == 0 && tid < BNO) {
#pragma unroll 8
      for (int r = 0; r < BR; ++r) bsum += Ys[r * BNO + tid];
    }
    __syncthreads();
    if (c + 1 < c_end) {
      store_chunk();
      __syncthreads();
    }
  }

  // D row (= n) = (reg&3) + 8*(reg>>2) + 4*(lane>>5), col (= k) = lane&31
  const int k = k0 + wave * 32 + lr;
  if (args.part) {
    float* dst = args.part + ((size_t)(split * args.nnb + nb) * args.nkb + kb) * (BNO * BKO);
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(t * 16 + r) * NT + tid] = acc[t][r];
  } else if (k < klen) {
    const int kcol = (src1 ? D.K : 0) + k;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (n < D.N) {
          if (args.diag_plain_store)
            D.dw[(size_t)n * D.ldw + kcol] = acc[t][r];
          else
            grad_add(&D.dw[(size_t)n * D.ldw + kcol], acc[t][r]);
        }
      }
  }
  if (D.db && kb == 0 && tid < BNO && n0 + tid < D.N) grad_add(&D.db[n0 + tid], bsum);
}

template <int BNO, int BKO, int BR, bool BUF = false>
__global__ __launch_bounds__(256) void gemm_wgrad_kernel(const WgradDev args) {
  wgrad_body<BNO, BKO, BR, BUF>(args, blockIdx.x);
}

// Several independent products in ONE launch: the d x d weight gradients of a backward pass are ~20 us latency-bound
// launches of ~100 blocks each; side by side they fill the chip and cost one launch.  Block -> (problem, local block).
constexpr int WGRAD_GROUP_MAX = 32;
struct WgradGroupIndex {
  int n;
  int block_start[WGRAD_GROUP_MAX + 1];
};
template <int BNO, int BKO, int BR>
__global__ __launch_bounds__(256) void gemm_wgrad_group_kernel(const WgradDev* __restrict__ devs,
                                                               const WgradGroupIndex idx) {
  int p = 0;
  for (int i = 1; i < idx.n; ++i)
    if ((int)blockIdx.x >= idx.block_start[i]) p = i;
  wgrad_body<BNO, BKO, BR, true>(devs[p], (int)blockIdx.x - idx.block_start[p]);
}

// dw tile (nb, kb) += its splits' partial tiles, in split order (fixed: bit-reproducible).  12 blocks of 256 threads per
// tile; a thread takes four consecutive floats of the register-order tile: the same n, four consecutive k.
__device__ __forceinline__ void wgrad_part_reduce_body(const WgradDev& g, int lb) {
  const CarcaWgradDesc& D = g.d;
  const int tile = lb / 12, sl = lb - tile * 12;
  const int nb = tile / g.nkb, kb = tile - nb * g.nkb;
  const int q = (sl * 256 + (int)threadIdx.x) * 4;  // 0 .. 12284
  const int e = q >> 8, t = q & 255;
  const int wave = t >> 6, lane = t & 63, lr = lane & 31, lh = lane >> 5;
  const size_t tile_fl = 96 * 128;
  // eight splits' loads in flight at a time (a plain loop waits for every load before it issues the next: 22 us for
  // 40 MB); the additions stay in split order
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  const float* base = g.part + ((size_t)nb * g.nkb + kb) * tile_fl + q;
  const size_t step = (size_t)g.nnb * g.nkb * tile_fl;
  int s = 0;
  for (; s + 8 <= g.nsplit; s += 8) {
    f32x4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f32x4*>(base + (size_t)(s + i) * step);
#pragma unroll
    for (int i = 0; i < 8; ++i) sum += v[i];
  }
  for (; s < g.nsplit; ++s) sum += *reinterpret_cast<const f32x4*>(base + (size_t)s * step);
  const int tt = e >> 4, r = e & 15;
  const int n = nb * 96 + tt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
  if (n >= D.N) return;
  const bool src1 = kb >= g.nkb0;
  const int k0 = (src1 ? kb - g.nkb0 : kb) * 128, klen = src1 ? D.K1 : D.K;
  float* row = D.dw + (size_t)n * D.ldw + (src1 ? D.K : 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = k0 + wave * 32 + lr + i;
    if (k < klen) row[k] += sum[i];
  }
}
__global__ __launch_bounds__(256) void wgrad_part_reduce_kernel(const WgradDev g) { wgrad_part_reduce_body(g, blockIdx.x); }
__global__ __launch_bounds__(256) void wgrad_part_reduce_group_kernel(const WgradDev* __restrict__ devs,
                                                                      const WgradGroupIndex idx) {
  int p = 0;
  for (int i = 1; i < idx.n; ++i)
    if ((int)blockIdx.x >= idx.block_start[i]) p = i;
  wgrad_part_reduce_body(devs[p], (int)blockIdx.x - idx.block_start[p]);
}

}  // namespace

int carca_wgrad_cu_try(const CarcaWgradDesc* desc, hipStream_t stream);  // wgrad_cu.hip

static int wgrad_check(const CarcaWgradDesc* desc) {
  CARCA_CHECK_ARG(desc && desc->nseg >= 1 && desc->nseg <= CARCA_MAX_SEGS, "gemm_wgrad: bad segment count");
  CARCA_CHECK_ARG(desc->dw && desc->N >= 1 && desc->K >= 1 && desc->K1 >= 0 && desc->ldw >= desc->K + desc->K1 &&
                      desc->ld_dy >= desc->N && desc->ld_x >= desc->K && (desc->K1 == 0 || desc->ld_x1 >= desc->K1),
                  "gemm_wgrad: bad geometry");
  for (int s = 0; s < desc->nseg; ++s) {
    const CarcaWgradSeg& sg = desc->seg[s];
    CARCA_CHECK_ARG(sg.rows >= 1 && sg.dy && sg.x && !(desc->mask_rows && !sg.ids) && (desc->K1 == 0 || sg.x1),
                    "gemm_wgrad: segment %d malformed", s);
    CARCA_CHECK_ARG(sg.T >= 1 || (!sg.x_bstride && !sg.x1_bstride), "gemm_wgrad: segment %d needs T >= 1", s);
    CARCA_CHECK_ARG(!(sg.x_gather && !sg.ids), "gemm_wgrad: segment %d gathers without ids", s);
  }
  return CARCA_OK;
}

// tiling / row splits of the tiled kernel for one product; returns the grid size; *fits: buffer loads are safe
static int wgrad_prepare(const CarcaWgradDesc* desc, WgradDev& g, bool* fits_out, int slot_budget = 0) {
  constexpr int BNO = 96, BKO = 128, BR = 32;
  g = WgradDev{};
  g.d = *desc;
  int chunks = 0;
  for (int s = 0; s < desc->nseg; ++s) {
    const CarcaWgradSeg& sg = desc->seg[s];
    if (g.d.seg[s].T < 1) g.d.seg[s].T = 1;
    g.chunk_start[s] = chunks;
    chunks += (sg.rows + BR - 1) / BR;
  }
  g.chunk_start[desc->nseg] = chunks;
  g.nnb = (desc->N + BNO - 1) / BNO;
  g.nkb0 = (desc->K + BKO - 1) / BKO;
  g.nkb = g.nkb0 + (desc->K1 + BKO - 1) / BKO;
  // row splits: fill the chip's 4 x 256 resident slots in ONE round (119 registers -> 4 blocks per CU;
  // measured at C2: 512 slots 1017 us, 768 972, 1024 809, 1536 865), but keep >= 2 chunks (64 rows) per split
  const int tiles = g.nnb * g.nkb;
  // Products of a few tiles (joint embedding: 5) pay for every split with a full tile of atomics: 384 slots there
  // (N = 90, K = 540, 19328 rows: 1024 slots 74.5 us, 768 65.8, 640 61.6, 512 59.6, 384 57.5, 256 67.6)
  const int slots = slot_budget > 0 ? slot_budget
                    : carca_tuning(CARCA_TUNE_WGRAD_SLOTS) > 0 ? carca_tuning(CARCA_TUNE_WGRAD_SLOTS)
                    : tiles >= 64 ? 1024 : 640;  // (640 since the splits end in plain stores: 384 / 512 / 640 / 768 / 1024 -> train
                                                 // step 1.749 / 1.743 / 1.737 / 1.740 / 1.736 ms, tools/ab_train.py "2=...")
  int nsplit = tiles >= slots ? 1 : slots / tiles;
  const int min_chunks = carca_tuning(CARCA_TUNE_WGRAD_MIN_CHUNKS) > 0 ? carca_tuning(CARCA_TUNE_WGRAD_MIN_CHUNKS) : 2;  // (measured on the d x d products: 4 -> 21 us, 2 -> 18 us, 1 -> 23 us)
  nsplit = max(1, min(nsplit, (chunks + min_chunks - 1) / min_chunks));
  g.diag_plain_store = carca_tuning(CARCA_TUNE_WGRAD_PLAIN_STORE);
  g.chunks_per_split = (chunks + nsplit - 1) / nsplit;
  g.nsplit = (chunks + g.chunks_per_split - 1) / g.chunks_per_split;
  // buffer loads when every operand offset provably fits 32 bits of bytes (a gather table's size must be stated)
  const uint64_t lim = 1ull << 30;
  bool fits = carca_tuning(CARCA_TUNE_GEMM_VARIANT) != CARCA_GV_NO_BUFFER_LOADS;
  for (int s = 0; s < desc->nseg && fits; ++s) {
    const CarcaWgradSeg& sg = desc->seg[s];
    const int T = sg.T >= 1 ? sg.T : 1;
    const uint64_t ub = (uint64_t)((sg.rows - 1) / T), ut = (uint64_t)(T - 1);
    const uint64_t lx = sg.x_gather ? (sg.x_gather > 1 ? (uint64_t)(sg.x_gather - 1) * desc->ld_x : lim)
                        : sg.x_bstride ? ub * sg.x_bstride + ut * desc->ld_x
                                       : (uint64_t)(sg.rows - 1) * desc->ld_x;
    const uint64_t lx1 = desc->K1 == 0 ? 0
                         : sg.x1_bstride ? ub * sg.x1_bstride + ut * desc->ld_x1
                                         : (uint64_t)(sg.rows - 1) * desc->ld_x1;
    fits = lx + desc->K < lim && lx1 + desc->K1 < lim && (uint64_t)sg.rows * desc->ld_dy < lim;
  }
  *fits_out = fits;
  return tiles * g.nsplit;
}

// Partial tiles of the row splits (WgradDev.part): stream scratch (carca_common.h) -- the product's kernel writes them, its
// reduce launch reads them, the next product on the stream is ordered behind both; inside a hipGraph capture the capture
// gets storage of its own.  CARCA_GV_WPART_ATOMICS = atomics (A/B).
namespace {
float* wpart_take(size_t floats, hipStream_t stream) {
  if (carca_tuning(CARCA_TUNE_GEMM_VARIANT) == CARCA_GV_WPART_ATOMICS || carca_tuning(CARCA_TUNE_WGRAD_PLAIN_STORE) != 0) return nullptr;
  if (carca_stream_capturing(stream)) return (float*)carca_capture_alloc(stream, floats * sizeof(float), false, nullptr);
  return (float*)carca_stream_scratch(stream, CARCA_SCRATCH_WPART, floats * sizeof(float));
}
}  // namespace

extern "C" int carca_gemm_wgrad(const CarcaWgradDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = wgrad_check(desc)) return rc;
  // the big product (dW of feats_embed) goes to the persistent one-block-per-CU kernel; tuning variant 4 / 5 = never
  const int variant = carca_tuning(CARCA_TUNE_GEMM_VARIANT);
  if (variant != CARCA_GV_NO_BUFFER_LOADS && variant != CARCA_GV_WGRAD_TILED) {
    const int r = carca_wgrad_cu_try(desc, stream);
    if (r != 1) return r;
  }
  constexpr int BNO = 96, BKO = 128, BR = 32;
  WgradDev g;
  bool fits = false;
  const int grid = wgrad_prepare(desc, g, &fits);
  const int tiles = g.nnb * g.nkb;
  if (g.nsplit > 1) g.part = wpart_take((size_t)g.nsplit * tiles * BNO * BKO, stream);  // (one split: nothing to combine)
  if (fits)
    hipLaunchKernelGGL((gemm_wgrad_kernel<BNO, BKO, BR, true>), dim3(grid), dim3(256), 0, stream, g);
  else
    hipLaunchKernelGGL((gemm_wgrad_kernel<BNO, BKO, BR>), dim3(grid), dim3(256), 0, stream, g);
  if (g.part) hipLaunchKernelGGL(wgrad_part_reduce_kernel, dim3(tiles * 12), dim3(256), 0, stream, g);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// Grouped launch: the kernel reads its descriptors from pinned, device-mapped host memory that THIS thread writes, so a
// slot may only be rewritten once the launch that reads it has finished: every slot carries an event recorded behind its
// launch, and a launch takes the first slot whose event has completed (hipEventQuery -- the host never waits; while none
// has, the pool grows: its size follows the number of launches in flight).  Products that are big enough for the
// persistent kernel, or whose offsets do not fit the buffer-load path, are issued one by one instead.
namespace {
struct GroupSlot {
  WgradDev* host;  // [WGRAD_GROUP_MAX] pinned, mapped into the device's address space (no copy command: a small async H2D
  WgradDev* dev;   // copy turned out to stall the issuing thread until the stream had drained)
  hipEvent_t ev;
  bool used;
};
std::vector<GroupSlot> g_group_slots;
int group_slot_take() {
  int found = -1;
  for (size_t i = 0; i < g_group_slots.size() && found < 0; ++i)
    if (!g_group_slots[i].used || hipEventQuery(g_group_slots[i].ev) == hipSuccess) found = (int)i;
  (void)hipGetLastError();  // (a query of a pending event leaves hipErrorNotReady behind: not the next launch's error)
  if (found >= 0) return found;
  GroupSlot sl{};
  if (hipHostMalloc((void**)&sl.host, sizeof(WgradDev) * WGRAD_GROUP_MAX, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&sl.dev, sl.host, 0) != hipSuccess ||
      hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) != hipSuccess)
    return -1;
  g_group_slots.push_back(sl);
  return (int)g_group_slots.size() - 1;
}
}  // namespace

extern "C" int carca_gemm_wgrad_group(const CarcaWgradDesc* descs, int n, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(descs && n >= 1, "gemm_wgrad_group: no products");
  for (int i = 0; i < n; ++i)
    if (int rc = wgrad_check(&descs[i])) return rc;
  constexpr int BNO = 96, BKO = 128, BR = 32;
  const int variant = carca_tuning(CARCA_TUNE_GEMM_VARIANT);
  int done = 0;
  const bool capturing = carca_stream_capturing(stream);  // (hipGraph capture: storage of its own, see carca_common.h)
  while (done < n) {
    int slot = -1;
    WgradDev *host, *dev;
    if (capturing) {
      host = (WgradDev*)carca_capture_alloc(stream, sizeof(WgradDev) * WGRAD_GROUP_MAX, true, (void**)&dev);
      if (!host) return CARCA_ERR_BADARG;
    } else {
      slot = group_slot_take();
      if (slot < 0) {
        carca_set_error("gemm_wgrad_group: cannot allocate a descriptor slot");
        return CARCA_ERR_BADARG;
      }
      host = g_group_slots[slot].host;
      dev = g_group_slots[slot].dev;
    }
    WgradGroupIndex idx{}, ridx{};
    int blocks = 0, rblocks = 0;
    size_t part_floats = 0;
    while (done < n && idx.n < WGRAD_GROUP_MAX) {
      bool fits = false;
      WgradDev g;
      // row-split budget per product (tuning key 5; 0 = the single-product default).  A/B at C2, interleaved in one
      // process (tools/ab_train.py): ungrouped 2.341 ms/step, grouped 2.229, grouped with 64 / 85 / 128 slots per
      // product 2.223 / 2.263 / 2.220 -- the budget does not matter, the single launch does
      // Second look with the kernel trace (tools/train_trace.sh, 13 products of a C2 backward pass in one launch):
      // 1024 slots per product (100 two-chunk splits each) 105 us, 64 -> 72 us, 48 -> 73, 40 -> 76, 32 -> 76, 24 -> 92,
      // 16 -> 108: every split ends with a 96 x 128 tile of atomics, so fewer, longer splits win until the chip runs dry
      // (with partial tiles instead of atomics: 32 -> 1.766 ms per train step, 64 -> 1.744, 96 -> 1.742, 128 -> 1.752)
      const int budget = carca_tuning(CARCA_TUNE_WGRAD_GROUP_SLOTS) > 0 ? carca_tuning(CARCA_TUNE_WGRAD_GROUP_SLOTS) : 96;
      const int grid = wgrad_prepare(&descs[done], g, &fits, budget);
      const bool big = (long)descs[done].N * (descs[done].K + descs[done].K1) > 96 * 1024;  // single-product path decides
      if (!fits || big || variant == CARCA_GV_NO_GROUP) {  // (A/B switch)
        if (int rc = carca_gemm_wgrad(&descs[done], stream_)) return rc;
        ++done;
        continue;
      }
      host[idx.n] = g;
      idx.block_start[idx.n] = blocks;
      ridx.block_start[idx.n] = rblocks;
      blocks += grid;
      rblocks += g.nnb * g.nkb * 12;
      part_floats += (size_t)g.nsplit * g.nnb * g.nkb * BNO * BKO;
      ++idx.n;
      ++done;
    }
    if (idx.n == 0) continue;
    idx.block_start[idx.n] = blocks;
    ridx.n = idx.n;
    ridx.block_start[idx.n] = rblocks;
    float* part = wpart_take(part_floats, stream);
    if (part) {  // every product its own stretch of the slot
      size_t at = 0;
      for (int i = 0; i < idx.n; ++i) {
        host[i].part = part + at;
        at += (size_t)host[i].nsplit * host[i].nnb * host[i].nkb * BNO * BKO;
      }
    }
    hipLaunchKernelGGL((gemm_wgrad_group_kernel<BNO, BKO, BR>), dim3(blocks), dim3(256), 0, stream, dev, idx);
    if (part) hipLaunchKernelGGL(wgrad_part_reduce_group_kernel, dim3(rblocks), dim3(256), 0, stream, dev, ridx);
    if (slot >= 0) {
      (void)hipEventRecord(g_group_slots[slot].ev, stream);
      g_group_slots[slot].used = true;
    }
    CARCA_LAUNCH_CHECK();
  }
  return CARCA_OK;
}
