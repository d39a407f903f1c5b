// Grouped GEMMs for the dropless mixture-of-experts FFN (models/mistral.py, moe_dropless): one launch covers every
// expert, and the per-expert row ranges are read on the device, so a captured step replays with any routing.
//
// The rows [0, R) of the packed slot layout (moe.hip, moe_assign_dropless) are cut into E segments by
// offsets [E + 1] (int32, device memory): segment e = rows [offsets[e], offsets[e + 1]), every bound a multiple of
// 128, offsets[E] <= R; the rows past offsets[E] belong to nobody.
//
//   NT  c[r, :] = a[r, :] B_e^T  for r in segment e   a [R][K], B_e [N][K], c [R][N]     forward, data gradients
//       a 128-row tile lies in one segment; a tile in no segment (the tail) stores zeros
//   TN  dW_e (+)= dy[seg e]^T x[seg e]                dy [R][M], x [R][N], dW_e [M][N]   weight gradients
//       the reduction runs over the segment's rows in ascending order inside one workgroup (no split-K, no
//       atomics: one fixed summation order per element); an empty segment writes zeros, or nothing when accumulating
//
// The operand tables (up to 64 pointers, the accumulate flags as a bit mask) are kernel arguments.  offsets is
// uniform per workgroup: read by scalar loads, before the first barrier; every bound derived from it is clamped to
// [0, R], so a wrong table cannot move an access out of the operands.
// The tile loop is gemm.hip's: 128 x 128 x 64 tiles, 4 waves (2 x 2), a 4-deep LDS ring filled by LDS-DMA with a
// counted vmcnt across the barrier, v_mfma_f32_32x32x16 with swapped roles (lane <-> m, 8-byte stores), fp32
// accumulation, one rounding.  The NT tiles are walked row-block-major (all N / 128 column tiles of one 128-row block,
// then the next block; segment-major, as segments are contiguous) and XCD-grouped, so each XCD works on a contiguous
// run of tiles.  The tiles of one row block share its A rows; an expert's weight is re-read once per row block, and
// stays in the XCD's 4 MB L2 between row blocks only while N K is small (the test shapes).  At the M7B gate|up shape a
// row block streams the whole 235 MB weight.  A walk that groups several row blocks of a segment over a few column
// tiles, so that a weight slab is reused from L2, is the first open item of the kernel's tuning.
#include "common.h"
#include "gemm_common.h"
#include "launchers.h"
#include "mfma_tiles.h"

namespace {

constexpr int kMaxGroups = 64;
constexpr int BT = 128;                        // tile edge (rows and columns)
constexpr int NSTAGE = 4;                      // LDS ring depth
constexpr int STAGE_BYTES = 2 * BT * kBK * 2;  // A and B image of one k-step
constexpr int SMEM_BYTES = NSTAGE * STAGE_BYTES;

struct GroupedNtArgs {
  const bf16_t* a;
  bf16_t* c;
  const int* offsets;
  long lda, ldb, ldc;
  int R, N, K, E;
  const bf16_t* b[kMaxGroups];
};

struct GroupedTnArgs {
  const bf16_t* dy;
  const bf16_t* x;
  const int* offsets;
  long lddy, ldx;
  int R, M, N, E;
  unsigned long long accumulate;               // bit e: dW_e += instead of =
  bf16_t* dw[kMaxGroups];
};

constexpr int FT = BT / 64;                    // 32 x 32 MFMA tiles per wave and direction

// acc += A B over nk k-steps starting at k-element kbeg.  NT: a [m][k], b [n][k]; TN: a [k][m], b [k][n].
// nk >= 1 (the callers take the empty reduction before their first barrier).
template <bool TN>
DLTB_DEV void tile_loop(const bf16_t* a, long lda, const bf16_t* b, long ldb, int m0, int n0, int kbeg, int nk,
                        char* smem, f32x16 (&acc)[FT][FT]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r = lane & 31;
  const int wm = w & 1, wn = w >> 1;
  const int wv = __builtin_amdgcn_readfirstlane(w);
  constexpr int WT = BT / 2;
  constexpr int A_BYTES = BT * kBK * 2;

  auto load_stage = [&](int kt, int st) {
    char* sa = smem + st * STAGE_BYTES;
    char* sb = sa + A_BYTES;
    const int k0 = kbeg + kt * kBK;
    if constexpr (!TN) {
      GldsTile<64, BT, true>::load(a + k0, lda, m0, sa, wv, lane);
      GldsTile<64, BT, true>::load(b + k0, ldb, n0, sb, wv, lane);
    } else {
      GldsTile<BT, kBK, true>::load(a + m0, lda, k0, sa, wv, lane);
      GldsTile<BT, kBK, true>::load(b + n0, ldb, k0, sb, wv, lane);
    }
  };
  // LDS-DMA wave-instructions per stage and wave: the unit of the counted vmcnt below
  constexpr int GLDS = TN ? 2 * GldsTile<BT, kBK>::NI : 2 * GldsTile<64, BT>::NI;
  static_assert(2 * GLDS < 64, "vmcnt range");

  // prologue: the first min(nk, NSTAGE - 1) stages.  `ahead` below counts only stages that were issued, so
  // nk = 1 .. NSTAGE - 1 (a ring that never fills) and nk > NSTAGE (a ring that wraps) take the same waits.
#pragma unroll
  for (int st = 0; st < NSTAGE - 1; ++st)
    if (st < nk) load_stage(st, st);
  for (int kt = 0; kt < nk; ++kt) {
    const int ahead = min(nk - 1 - kt, NSTAGE - 2);     // stages issued after kt that may stay in flight
    if (ahead >= 2) wait_vm<2 * GLDS>();
    else if (ahead == 1) wait_vm<GLDS>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();                       // every wave's part of stage kt has landed
    if (kt + NSTAGE - 1 < nk) load_stage(kt + NSTAGE - 1, (kt + NSTAGE - 1) % NSTAGE);
    const char* sa = smem + (kt % NSTAGE) * STAGE_BYTES;
    const char* sb = sa + A_BYTES;
#pragma unroll
    for (int s = 0; s < kBK / 16; ++s) {
      bfx8 fa[FT], fb[FT];
#pragma unroll
      for (int i = 0; i < FT; ++i) {
        if constexpr (!TN) fa[i] = row_frag<64>(sa, wm * WT + 32 * i + r, 2 * s + h);
        else fa[i] = tr_frag<BT>(sa, 16 * s, wm * WT + 32 * i, lane);
      }
#pragma unroll
      for (int j = 0; j < FT; ++j) {
        if constexpr (!TN) fb[j] = row_frag<64>(sb, wn * WT + 32 * j + r, 2 * s + h);
        else fb[j] = tr_frag<BT>(sb, 16 * s, wn * WT + 32 * j, lane);
      }
#pragma unroll
      for (int i = 0; i < FT; ++i)
#pragma unroll
        for (int j = 0; j < FT; ++j) acc[i][j] = mfma32(fb[j], fa[i], acc[i][j]);   // lane <-> m
    }
    // the NEXT iteration's barrier orders these LDS reads before stage kt's buffer is refilled
  }
}

// lane -> row m, register group q -> columns n .. n + 3 of the 128 x 128 tile at (m0, n0) of c [.][ldc]
DLTB_DEV void store_tile(const f32x16 (&acc)[FT][FT], bf16_t* c, long ldc, int m0, int n0, bool accumulate) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, r = lane & 31;
  const int wm = w & 1, wn = w >> 1;
  constexpr int WT = BT / 2;
#pragma unroll
  for (int i = 0; i < FT; ++i) {
    const int m = m0 + wm * WT + 32 * i + r;
#pragma unroll
    for (int j = 0; j < FT; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * WT + 32 * j + 8 * q + 4 * h;
        float v[4] = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
        bf16_t* cp = c + (size_t)m * ldc + n;
        if (accumulate) {
          const uint2 old = *reinterpret_cast<const uint2*>(cp);
          v[0] += lo_bf(old.x); v[1] += hi_bf(old.x); v[2] += lo_bf(old.y); v[3] += hi_bf(old.y);
        }
        uint2 o;
        o.x = pack_bf2(v[0], v[1]);
        o.y = pack_bf2(v[2], v[3]);
        *reinterpret_cast<uint2*>(cp) = o;
      }
    }
  }
}

// exact zeros into the 128 x 128 tile at (m0, n0): 16 chunks of 16 bytes per row
DLTB_DEV void zero_tile(bf16_t* c, long ldc, int m0, int n0) {
  for (int t = threadIdx.x; t < BT * (BT / 8); t += 256) {
    const int row = t / (BT / 8), ch = t % (BT / 8);
    *reinterpret_cast<uint4*>(c + (size_t)(m0 + row) * ldc + n0 + ch * 8) = make_uint4(0u, 0u, 0u, 0u);
  }
}

DLTB_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256, 1) void gemm_grouped_nt_kernel(GroupedNtArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tiles_n = g.N / BT, tiles = (g.R / BT) * tiles_n;
  const int idx = xcd_grouped(blockIdx.x, tiles);       // row-block-major: segment-major, as segments are contiguous
  const int m0 = (idx / tiles_n) * BT, n0 = (idx % tiles_n) * BT;
  DLTB_DCHECK(m0 + BT <= g.R && n0 + BT <= g.N && g.K % kBK == 0 && g.K > 0 && g.E <= kMaxGroups);
  // the segment holding row m0 (uniform: scalar loads); empty segments have lo == hi and hold nothing
  int e = -1;
  for (int i = 0; i < g.E; ++i) {
    const int lo = g.offsets[i], hi = g.offsets[i + 1];
    if (m0 >= lo && m0 < hi) e = i;
  }
  if (e < 0) {                                          // the tail past offsets[E]: uniform, before any barrier
    zero_tile(g.c, g.ldc, m0, n0);
    return;
  }
  f32x16 acc[FT][FT];
#pragma unroll
  for (int i = 0; i < FT; ++i)
#pragma unroll
    for (int j = 0; j < FT; ++j) acc[i][j] = f32x16{};
  tile_loop<false>(g.a, g.lda, g.b[e], g.ldb, m0, n0, 0, g.K / kBK, smem, acc);
  store_tile(acc, g.c, g.ldc, m0, n0, false);
}

__global__ __launch_bounds__(256, 1) void gemm_grouped_tn_kernel(GroupedTnArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tiles_n = g.N / BT, per = (g.M / BT) * tiles_n, tiles = per * g.E;
  const int idx = xcd_grouped(blockIdx.x, tiles);       // group-major: neighbouring tiles read the same group's rows
  const int e = idx / per, in = idx % per;
  const int m0 = (in / tiles_n) * BT, n0 = (in % tiles_n) * BT;
  DLTB_DCHECK(e < g.E && g.E <= kMaxGroups && m0 + BT <= g.M && n0 + BT <= g.N);
  // the group's row range, whole k-steps inside [0, R] whatever the table holds
  const int kb = clampi(g.offsets[e], 0, g.R) & ~(kBK - 1);
  const int ke = clampi(g.offsets[e + 1], kb, g.R) & ~(kBK - 1);
  const int nk = (ke - kb) / kBK;
  const bool accumulate = (g.accumulate >> e) & 1ull;
  bf16_t* dw = g.dw[e];
  if (nk <= 0) {                                        // empty group: uniform, before any barrier
    if (!accumulate) zero_tile(dw, g.N, m0, n0);
    return;
  }
  f32x16 acc[FT][FT];
#pragma unroll
  for (int i = 0; i < FT; ++i)
#pragma unroll
    for (int j = 0; j < FT; ++j) acc[i][j] = f32x16{};
  tile_loop<true>(g.dy, g.lddy, g.x, g.ldx, m0, n0, kb, nk, smem, acc);
  store_tile(acc, dw, g.N, m0, n0, accumulate);
}

}  // namespace

bool dltb_gemm_grouped_nt_supported(int R, int N, int K, int E) {
  return R > 0 && N > 0 && K > 0 && R % BT == 0 && N % BT == 0 && K % kBK == 0 && E >= 1 && E <= kMaxGroups &&
         (long)(R / BT) * (N / BT) < (1L << 31);
}

int dltb_gemm_grouped_nt(const void* a, const int* offsets, const void* const* b, void* c, long lda, long ldb,
                         long ldc, int R, int N, int K, int E, hipStream_t st) {
  if (!dltb_gemm_grouped_nt_supported(R, N, K, E)) return -1;
  GroupedNtArgs g{};
  g.a = (const bf16_t*)a;
  g.c = (bf16_t*)c;
  g.offsets = offsets;
  g.lda = lda;
  g.ldb = ldb;
  g.ldc = ldc;
  g.R = R;
  g.N = N;
  g.K = K;
  g.E = E;
  for (int e = 0; e < E; ++e) g.b[e] = (const bf16_t*)b[e];
  allow_dynamic_lds<gemm_grouped_nt_kernel>(SMEM_BYTES);
  hipLaunchKernelGGL(gemm_grouped_nt_kernel, dim3((R / BT) * (N / BT)), dim3(256), SMEM_BYTES, st, g);
  return 0;
}

bool dltb_gemm_grouped_tn_supported(int R, int M, int N, int E) {
  return R > 0 && M > 0 && N > 0 && R % BT == 0 && M % BT == 0 && N % BT == 0 && E >= 1 && E <= kMaxGroups &&
         (long)(M / BT) * (N / BT) * E < (1L << 31);
}

int dltb_gemm_grouped_tn(const void* dy, const void* x, const int* offsets, void* const* dw,
                         unsigned long long accumulate, long lddy, long ldx, int R, int M, int N, int E,
                         hipStream_t st) {
  if (!dltb_gemm_grouped_tn_supported(R, M, N, E)) return -1;
  GroupedTnArgs g{};
  g.dy = (const bf16_t*)dy;
  g.x = (const bf16_t*)x;
  g.offsets = offsets;
  g.lddy = lddy;
  g.ldx = ldx;
  g.R = R;
  g.M = M;
  g.N = N;
  g.E = E;
  g.accumulate = accumulate;
  for (int e = 0; e < E; ++e) g.dw[e] = (bf16_t*)dw[e];
  allow_dynamic_lds<gemm_grouped_tn_kernel>(SMEM_BYTES);
  hipLaunchKernelGGL(gemm_grouped_tn_kernel, dim3((M / BT) * (N / BT) * E), dim3(256), SMEM_BYTES, st, g);
  return 0;
}
