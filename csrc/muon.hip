// Muon optimizer kernels (gfx950): momentum -> Newton-Schulz orthogonalisation -> update.
//
// The contract (constants, rounding points) is ops/ref.py muon_momentum / muon_newton_schulz / muon_update.
// One Newton-Schulz step on X [m, n] (m <= n), bf16 between products, fp32 accumulation:
//     A = alpha X X^T            muon_syrk   (alpha = s^2 at step 0: a per-batch device scalar)
//     B = b A + c A A            muon_syrk   (X := A, which is symmetric, so A A = A A^T; D := A, beta = b)
//     X' = alpha (a X + B X)     muon_apply  (alpha = s at step 0)
// Every launch is batched: the same-shape matrices of all layers are stacked, one grid covers batch x tiles.
//
// muon_syrk: the result is symmetric, so the grid walks the t (t + 1) / 2 lower-triangle tiles of BT x BT only
// (half the MFMA work of a full product).  Block = 4 waves (2 x 2), k-step 64, the LDS ring of gemm.hip (LDS-DMA
// one to three k-steps ahead, counted vmcnt across a raw s_barrier), swapped MFMA roles (lane <-> m, register
// group <-> 4 consecutive n).  An off-diagonal tile stages two NT images per k-step (rows m0.. and rows n0.. of
// X); a diagonal tile stages ONE image and both MFMA operands are read from it (half the DMA traffic and a
// shorter vmcnt count).  Epilogue: tile (mb, nb) is stored as 8-byte vectors; its mirror (nb, mb) is the SAME
// rounded values transposed through the (now idle) ring memory and written as 16-byte row stores.  A diagonal
// tile goes through LDS whole: element (i, j) is taken from the accumulator entry of (max, min), so the output
// is bitwise symmetric by construction and does not rest on the MFMA adding a b and b a alike.
//
// muon_apply: gemm_nn.hip's mixed-layout product (B K-contiguous -> NT image / row_frag; X K-strided -> TN image
// staged with KSWAP / tr_frag, BN <= 128) with the a X term read at the output coordinates in the epilogue.
// Y must not be X: other tiles still read X while this one writes.
//
// muon_momentum / muon_update: 64 x 64 tiles over a table of matrices (the style of adamw.hip's block tables),
// transposing through LDS where rows > cols so the Newton-Schulz operand always has m <= n.
#include "common.h"
#include "launchers.h"
#include "mfma_tiles.h"

namespace {

constexpr int kBK = 64;       // k-step of the GEMM rings (as gemm_common.h)

// ------------------------------------------------------------------------------------------------ the ring
// NSTAGE-deep LDS ring (gemm.hip): load(kt, stage) issues GLDS LDS-DMA wave-instructions per wave, step(stage)
// consumes one landed stage.  Ends with every DMA retired; the caller barriers before reusing the memory.
template <int NSTAGE, int GLDS, class Load, class Step>
DLTB_DEV void ring_loop(int nk, Load load, Step step) {
  static_assert(NSTAGE >= 3 && 2 * GLDS < 64, "vmcnt range");
#pragma unroll
  for (int st = 0; st < NSTAGE - 1; ++st)
    if (st < nk) load(st, st);
  for (int kt = 0; kt < nk; ++kt) {
    const int ahead = min(nk - 1 - kt, NSTAGE - 2);     // stages issued after kt that may stay in flight
    if (ahead >= 2) wait_vm<2 * GLDS>();
    else if (ahead == 1) wait_vm<GLDS>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();                       // every wave's part of stage kt has landed
    if (kt + NSTAGE - 1 < nk) load(kt + NSTAGE - 1, (kt + NSTAGE - 1) % NSTAGE);
    step(kt % NSTAGE);
    // the NEXT iteration's barrier orders these LDS reads before stage kt's buffer is refilled
  }
}

// ------------------------------------------------------------------------------------------------ muon_syrk
struct SyrkArgs {
  const bf16_t* x;      // [batch][m][k], row stride ldx, batch stride sx
  const bf16_t* d;      // optional symmetric [batch][m][m], row stride ldd, batch stride sd
  bf16_t* c;            // [batch][m][m], row stride ldc, batch stride sc
  const float* dalpha;  // optional per-batch device scalar: dalpha[batch * dalpha_stride]
  long ldx, ldd, ldc, sx, sd, sc, dalpha_stride;
  float alpha, beta;
  int m, k, batch;
};

template <int BT>
struct GeoSyrk {
  static constexpr int IMG = BT * kBK * 2;          // one NT image: BT rows of 64 k
  static constexpr int STAGE = 2 * IMG;             // (a diagonal tile fills the first half only)
  static constexpr int NSTAGE = 4;                  // 128 KiB at BT = 128, 64 KiB at BT = 64
  static constexpr int SMEM = NSTAGE * STAGE;
  static constexpr int TROW = BT * 2 + 16;          // epilogue tile row pitch in bytes (16 B pad: the two lane
                                                    // halves of a transposed write fall on different banks)
  static_assert(2 * BT * TROW <= SMEM, "two epilogue tiles fit in the idle ring");
};

// lower-triangle tile index (row-major: idx = mb (mb + 1) / 2 + nb) -> (mb, nb <= mb)
DLTB_DEV void tri_tile(int idx, int& mb, int& nb) {
  int r = (int)((sqrtf(8.f * (float)idx + 1.f) - 1.f) * 0.5f);
  while (r * (r + 1) / 2 > idx) --r;
  while ((r + 1) * (r + 2) / 2 <= idx) ++r;
  mb = r;
  nb = idx - r * (r + 1) / 2;
}

template <int BT>
__global__ __launch_bounds__(256, 1) void muon_syrk_kernel(SyrkArgs g) {
  using G = GeoSyrk<BT>;
  constexpr int WT = BT / 2, FT = WT / 32;         // wave tile, 32x32 MFMA tiles per wave and side
  constexpr int NI = GldsTile<64, BT>::NI;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r = lane & 31;
  const int wm = w & 1, wn = w >> 1;
  const int wv = __builtin_amdgcn_readfirstlane(w);
  // (batch, triangle tile) in XCD-grouped order: each XCD's L2 gets a contiguous run of tiles of one matrix
  const int t = g.m / BT, tri = t * (t + 1) / 2;
  const int idx = xcd_grouped(blockIdx.x, tri * g.batch);
  const int bz = idx / tri;
  int mb, nb;
  tri_tile(idx - bz * tri, mb, nb);
  const int m0 = mb * BT, n0 = nb * BT, nk = g.k / kBK;
  const bool diag = mb == nb;
  DLTB_DCHECK(bz < g.batch && nb <= mb && m0 + BT <= g.m && nk > 0);
  const bf16_t* x = g.x + (long)bz * g.sx;

  f32x16 acc[FT][FT];
#pragma unroll
  for (int i = 0; i < FT; ++i)
#pragma unroll
    for (int j = 0; j < FT; ++j) acc[i][j] = f32x16{};

  auto step = [&](const char* sa, const char* sb) {
#pragma unroll
    for (int s = 0; s < kBK / 16; ++s) {
      bfx8 fa[FT], fb[FT];
#pragma unroll
      for (int i = 0; i < FT; ++i) fa[i] = row_frag<64>(sa, wm * WT + 32 * i + r, 2 * s + h);
#pragma unroll
      for (int j = 0; j < FT; ++j) fb[j] = row_frag<64>(sb, wn * WT + 32 * j + r, 2 * s + h);
#pragma unroll
      for (int i = 0; i < FT; ++i)
#pragma unroll
        for (int j = 0; j < FT; ++j) acc[i][j] = mfma32(fb[j], fa[i], acc[i][j]);   // lane <-> m
    }
  };
  if (diag) {       // one image per k-step feeds both operands
    ring_loop<G::NSTAGE, NI>(
        nk, [&](int kt, int st) { GldsTile<64, BT, true>::load(x + kt * kBK, g.ldx, m0, smem + st * G::STAGE, wv, lane); },
        [&](int st) { step(smem + st * G::STAGE, smem + st * G::STAGE); });
  } else {
    ring_loop<G::NSTAGE, 2 * NI>(
        nk,
        [&](int kt, int st) {
          GldsTile<64, BT, true>::load(x + kt * kBK, g.ldx, m0, smem + st * G::STAGE, wv, lane);
          GldsTile<64, BT, true>::load(x + kt * kBK, g.ldx, n0, smem + st * G::STAGE + G::IMG, wv, lane);
        },
        [&](int st) { step(smem + st * G::STAGE, smem + st * G::STAGE + G::IMG); });
  }

  // ---- epilogue: lane -> row m, register group q -> columns n .. n + 3 (tile-local ml, nl)
  const float al = g.alpha * (g.dalpha ? g.dalpha[(long)bz * g.dalpha_stride] : 1.f);
  const bf16_t* d = g.d ? g.d + (long)bz * g.sd : nullptr;
  bf16_t* c = g.c + (long)bz * g.sc;
  char* tT = smem;                       // tT[nl][ml]: the rounded tile transposed
  char* tP = smem + BT * G::TROW;        // tP[ml][nl]: the tile as computed (diagonal tiles only)
  __syncthreads();                       // every wave is done reading the ring
#pragma unroll
  for (int i = 0; i < FT; ++i) {
    const int ml = wm * WT + 32 * i + r;
#pragma unroll
    for (int j = 0; j < FT; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nl = wn * WT + 32 * j + 8 * q + 4 * h;
        float v[4] = {acc[i][j][4 * q] * al, acc[i][j][4 * q + 1] * al, acc[i][j][4 * q + 2] * al,
                      acc[i][j][4 * q + 3] * al};
        if (d) {
          const uint2 dd = *reinterpret_cast<const uint2*>(d + (size_t)(m0 + ml) * g.ldd + n0 + nl);
          v[0] += g.beta * lo_bf(dd.x); v[1] += g.beta * hi_bf(dd.x);
          v[2] += g.beta * lo_bf(dd.y); v[3] += g.beta * hi_bf(dd.y);
        }
        uint2 o;
        o.x = pack_bf2(v[0], v[1]);
        o.y = pack_bf2(v[2], v[3]);
        if (diag) *reinterpret_cast<uint2*>(tP + ml * G::TROW + nl * 2) = o;
        else *reinterpret_cast<uint2*>(c + (size_t)(m0 + ml) * g.ldc + n0 + nl) = o;
        bf16_t* col = reinterpret_cast<bf16_t*>(tT + nl * G::TROW) + ml;
        constexpr int P = G::TROW / 2;
        col[0] = (bf16_t)(o.x & 0xFFFFu);
        col[P] = (bf16_t)(o.x >> 16);
        col[2 * P] = (bf16_t)(o.y & 0xFFFFu);
        col[3 * P] = (bf16_t)(o.y >> 16);
      }
    }
  }
  __syncthreads();
  // row stores of 8 elements: row rr of the mirror tile (nb, mb) is tT[rr]; of a diagonal tile, the lower part
  // (column <= row) of tP[rr] and the mirrored part of tT[rr]
  constexpr int CPR = BT / 8;            // 16-byte chunks per row
  for (int u = tid; u < BT * CPR; u += 256) {
    const int rr = u / CPR, c0 = (u % CPR) * 8;
    uint4 a = *reinterpret_cast<const uint4*>(tT + rr * G::TROW + c0 * 2);
    if (diag) {
      const uint4 p = *reinterpret_cast<const uint4*>(tP + rr * G::TROW + c0 * 2);
      const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, pw[4] = {p.x, p.y, p.z, p.w};
      uint32_t ow[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {      // columns c0 + 2e (low half), c0 + 2e + 1 (high half)
        const uint32_t lo = (c0 + 2 * e <= rr ? pw[e] : aw[e]) & 0xFFFFu;
        const uint32_t hi = (c0 + 2 * e + 1 <= rr ? pw[e] : aw[e]) & 0xFFFF0000u;
        ow[e] = lo | hi;
      }
      a = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
    *reinterpret_cast<uint4*>(c + (size_t)(n0 + rr) * g.ldc + m0 + c0) = a;
  }
}

template <int BT>
void launch_syrk(const SyrkArgs& g, hipStream_t st) {
  constexpr int smem = GeoSyrk<BT>::SMEM;
  allow_dynamic_lds<muon_syrk_kernel<BT>>(smem);
  const int t = g.m / BT;
  hipLaunchKernelGGL((muon_syrk_kernel<BT>), dim3(t * (t + 1) / 2 * g.batch), dim3(256), smem, st, g);
}

// Tile choice by shape, from the measured rows of profiles/muon.txt (medians of five alternated rounds, spreads
// under 1 %): at m = 1024 BT = 128 is 4-12 % faster at every k; at m = 512 BT = 64 is 5-16 % faster up to k = 1792
// and BT = 128 1 % faster at k = 3584.  Only m = 512 and 1024 were measured: the rule between them is a guess.
int syrk_bt(int m, int k) { return (m % 128 == 0 && (m >= 1024 || k >= 3584)) ? 128 : 64; }

bool overlaps(const void* a, long na, const void* b, long nb) {   // element ranges [a, a + na), [b, b + nb) of bf16
  const char* pa = (const char*)a;
  const char* pb = (const char*)b;
  return pa < pb + nb * 2 && pb < pa + na * 2;
}
long span(long batch_stride, int batch, long ld, int rows, int cols) {   // elements a strided batch covers
  return (long)(batch - 1) * batch_stride + (long)(rows - 1) * ld + cols;
}

// ------------------------------------------------------------------------------------------------ muon_apply
struct ApplyArgs {
  const bf16_t* b;      // [batch][m][m] K-contiguous
  const bf16_t* x;      // [batch][m][n] K-strided
  bf16_t* y;            // [batch][m][n]
  const float* dalpha;
  long ldb, ldx, ldy, sb, sx, sy, dalpha_stride;
  float alpha, a;
  int m, n, batch;
};

template <int BM, int BN>
struct GeoApply {
  static constexpr int A_BYTES = BM * kBK * 2;
  static constexpr int B_BYTES = BN * kBK * 2;
  static constexpr int STAGE = A_BYTES + B_BYTES;
  static constexpr int NSTAGE = 4;                  // <= 128 KiB
  static constexpr int SMEM = NSTAGE * STAGE;
};

template <int BM, int BN>
__global__ __launch_bounds__(256, 1) void muon_apply_kernel(ApplyArgs g) {
  using G = GeoApply<BM, BN>;
  constexpr int WM = BM / 2, WN = BN / 2, FM = WM / 32, FN = WN / 32;
  static_assert(BN <= 128, "TN image rows are <= 128 elements");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r = lane & 31;
  const int wm = w & 1, wn = w >> 1;
  const int wv = __builtin_amdgcn_readfirstlane(w);
  const int tiles_n = g.n / BN, tiles = (g.m / BM) * tiles_n;
  const int idx = xcd_grouped(blockIdx.x, tiles * g.batch);
  const int bz = idx / tiles, tl = idx - bz * tiles;
  const int m0 = (tl / tiles_n) * BM, n0 = (tl % tiles_n) * BN, nk = g.m / kBK;
  DLTB_DCHECK(bz < g.batch && m0 + BM <= g.m && n0 + BN <= g.n && nk > 0);
  const bf16_t* bm = g.b + (long)bz * g.sb;
  const bf16_t* x = g.x + (long)bz * g.sx;

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x16{};

  constexpr int GLDS = GldsTile<64, BM>::NI + GldsTile<BN, kBK>::NI;
  ring_loop<G::NSTAGE, GLDS>(
      nk,
      [&](int kt, int st) {
        char* sa = smem + st * G::STAGE;
        GldsTile<64, BM, true>::load(bm + kt * kBK, g.ldb, m0, sa, wv, lane);
        GldsTile<BN, kBK, true, true>::load(x + n0, g.ldx, kt * kBK, sa + G::A_BYTES, wv, lane);   // row_frag's k order
      },
      [&](int st) {
        const char* sa = smem + st * G::STAGE;
        const char* sb = sa + G::A_BYTES;
#pragma unroll
        for (int s = 0; s < kBK / 16; ++s) {
          bfx8 fa[FM], fb[FN];
#pragma unroll
          for (int i = 0; i < FM; ++i) fa[i] = row_frag<64>(sa, wm * WM + 32 * i + r, 2 * s + h);
#pragma unroll
          for (int j = 0; j < FN; ++j) fb[j] = tr_frag<BN>(sb, 16 * s, wn * WN + 32 * j, lane);
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = mfma32(fb[j], fa[i], acc[i][j]);   // lane <-> m
        }
      });

  const float al = g.alpha * (g.dalpha ? g.dalpha[(long)bz * g.dalpha_stride] : 1.f);
  bf16_t* y = g.y + (long)bz * g.sy;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + wm * WM + 32 * i + r;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * WN + 32 * j + 8 * q + 4 * h;
        const uint2 xx = *reinterpret_cast<const uint2*>(x + (size_t)m * g.ldx + n);
        uint2 o;
        o.x = pack_bf2(al * (g.a * lo_bf(xx.x) + acc[i][j][4 * q]), al * (g.a * hi_bf(xx.x) + acc[i][j][4 * q + 1]));
        o.y = pack_bf2(al * (g.a * lo_bf(xx.y) + acc[i][j][4 * q + 2]), al * (g.a * hi_bf(xx.y) + acc[i][j][4 * q + 3]));
        *reinterpret_cast<uint2*>(y + (size_t)m * g.ldy + n) = o;
      }
    }
  }
}

template <int BM, int BN>
void launch_apply(const ApplyArgs& g, hipStream_t st) {
  constexpr int smem = GeoApply<BM, BN>::SMEM;
  allow_dynamic_lds<muon_apply_kernel<BM, BN>>(smem);
  hipLaunchKernelGGL((muon_apply_kernel<BM, BN>), dim3((g.m / BM) * (g.n / BN) * g.batch), dim3(256), smem, st, g);
}

// tile configs (BM x BN): 0 = 128x128, 1 = 128x64, 2 = 64x128, 3 = 64x64; the largest that divides the shape and
// still fills the machine (profiles/muon.txt)
bool apply_tile(int cfg, int& BM, int& BN) {
  static const int t[4][2] = {{128, 128}, {128, 64}, {64, 128}, {64, 64}};
  if (cfg < 0 || cfg > 3) return false;
  BM = t[cfg][0];
  BN = t[cfg][1];
  return true;
}
int apply_cfg(int m, int n, int batch) {
  for (int cfg = 0; cfg < 4; ++cfg) {
    int BM, BN;
    apply_tile(cfg, BM, BN);
    if (m % BM || n % BN) continue;
    if (cfg == 3 || (long)(m / BM) * (n / BN) * batch >= 256) return cfg;
  }
  return 3;
}

// ------------------------------------------------------------------------------------------------ momentum / update
// Matrix table, 8 int64 per matrix: rows, cols, owner offset (master / gradient index of element (0, 0)),
// momentum offset, work offset (element offset of this matrix in the stacked U / X buffers), bf16 destination
// pointer, first block-table row, block count.  Block table: (matrix, tile) per 64 x 64 tile of W as stored,
// a matrix's rows contiguous.  The work image is W^T when rows > cols, so it always has m <= n.
constexpr int kMT = 8;
constexpr int kTile = 64;
constexpr int kTPitch = kTile + 8;       // LDS tile row pitch in elements

struct MuonTile {
  long rows, cols, owner, mom, work;
  bf16_t* dst;
  int r0, c0;
  bool tr;
};
DLTB_DEV MuonTile muon_tile(const int64_t* mat_tab, const int* blk_mat, const int* blk_tile, int bi) {
  const int64_t* mt = mat_tab + (long)blk_mat[bi] * kMT;
  MuonTile t;
  t.rows = mt[0]; t.cols = mt[1]; t.owner = mt[2]; t.mom = mt[3]; t.work = mt[4];
  t.dst = reinterpret_cast<bf16_t*>(mt[5]);
  const int tc = (int)(t.cols / kTile), tile = blk_tile[bi];
  t.r0 = (tile / tc) * kTile;
  t.c0 = (tile % tc) * kTile;
  t.tr = t.rows > t.cols;
  DLTB_DCHECK(bi >= mt[6] && bi < mt[6] + mt[7] && t.r0 + kTile <= t.rows);
  return t;
}
template <typename G>
DLTB_DEV void load16(const G* p, float* g);
template <>
DLTB_DEV void load16<float>(const float* p, float* g) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(p + 4 * q);
    g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; g[4 * q + 3] = v.w;
  }
}
template <>
DLTB_DEV void load16<bf16_t>(const bf16_t* p, float* g) {
  unpack8(*reinterpret_cast<const uint4*>(p), g);
  unpack8(*reinterpret_cast<const uint4*>(p + 8), g + 8);
}

// mom = mu mom + gs g;  u = gs g + mu mom;  U = bf16(u) (transposed where rows > cols);  partial[block] = sum U^2
// thread (tr = tid / 4, seg = tid % 4) owns 16 consecutive columns of one tile row
template <typename G>
__global__ __launch_bounds__(256) void muon_momentum_kernel(
    const G* __restrict__ grad, float* __restrict__ mom, bf16_t* __restrict__ U, float* __restrict__ partial,
    const int64_t* __restrict__ mat_tab, const int* __restrict__ blk_mat, const int* __restrict__ blk_tile,
    const float* __restrict__ gscale, const float* __restrict__ hp, float mu) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[kTile * kTPitch];
  __shared__ float red[4];
  if (hp && hp[3] != 0.f) return;        // skipped step: momentum, U and the norms stay
  const MuonTile t = muon_tile(mat_tab, blk_mat, blk_tile, blockIdx.x);
  const float gs = gscale ? *gscale : 1.f;
  const int tr = threadIdx.x >> 2, seg = (threadIdx.x & 3) * 16;
  const long e = (long)(t.r0 + tr) * t.cols + t.c0 + seg;
  float g[16], m[16], ss = 0.f;
  bf16_t ub[16];
  load16<G>(grad + t.owner + e, g);
  load16<float>(mom + t.mom + e, m);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float gg = gs * g[i];
    m[i] = mu * m[i] + gg;
    ub[i] = f2bf(gg + mu * m[i]);
    const float ur = bf2f(ub[i]);
    ss += ur * ur;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    *reinterpret_cast<float4*>(mom + t.mom + e + 4 * q) = make_float4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
  uint4 o[2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
    o[q] = make_uint4(ub[8 * q] | (uint32_t)ub[8 * q + 1] << 16, ub[8 * q + 2] | (uint32_t)ub[8 * q + 3] << 16,
                      ub[8 * q + 4] | (uint32_t)ub[8 * q + 5] << 16, ub[8 * q + 6] | (uint32_t)ub[8 * q + 7] << 16);
  if (!t.tr) {
    *reinterpret_cast<uint4*>(U + t.work + e) = o[0];
    *reinterpret_cast<uint4*>(U + t.work + e + 8) = o[1];
  } else {                               // U is [cols, rows]: tile rows become columns
    *reinterpret_cast<uint4*>(tile + tr * kTPitch + seg) = o[0];
    *reinterpret_cast<uint4*>(tile + tr * kTPitch + seg + 8) = o[1];
    __syncthreads();
    bf16_t v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = tile[(seg + i) * kTPitch + tr];
    bf16_t* up = U + t.work + (long)(t.c0 + tr) * t.rows + t.r0 + seg;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      *reinterpret_cast<uint4*>(up + 8 * q) =
          make_uint4(v[8 * q] | (uint32_t)v[8 * q + 1] << 16, v[8 * q + 2] | (uint32_t)v[8 * q + 3] << 16,
                     v[8 * q + 4] | (uint32_t)v[8 * q + 5] << 16, v[8 * q + 6] | (uint32_t)v[8 * q + 7] << 16);
  }
  ss = block_sum(ss, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = ss;
}

// norms[2 i] = s = 1 / (sqrt(sum U_i^2) + eps), norms[2 i + 1] = s^2: one block per matrix adds its partials in
// index order (no atomics: the same bits on every run)
__global__ __launch_bounds__(256) void muon_norm_kernel(const float* __restrict__ partial, float* __restrict__ norms,
                                                        const int64_t* __restrict__ mat_tab,
                                                        const float* __restrict__ hp, float eps) {
  __shared__ float red[4];
  if (hp && hp[3] != 0.f) return;
  const int64_t* mt = mat_tab + (long)blockIdx.x * kMT;
  const int first = (int)mt[6], n = (int)mt[7];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[first + i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float s = 1.f / (sqrtf(acc) + eps);
    norms[2 * blockIdx.x] = s;
    norms[2 * blockIdx.x + 1] = s * s;
  }
}

// W -= lr (0.2 sqrt(max(rows, cols)) O + wd W), O read back through the transpose where rows > cols; writes the
// fp32 master and its 16-bit copy
__global__ __launch_bounds__(256) void muon_update_kernel(
    float* __restrict__ master, const bf16_t* __restrict__ O, const int64_t* __restrict__ mat_tab,
    const int* __restrict__ blk_mat, const int* __restrict__ blk_tile, const float* __restrict__ hp, float lr,
    float wd) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[kTile * kTPitch];
  if (hp) {
    if (hp[3] != 0.f) return;
    lr = hp[0];
  }
  const MuonTile t = muon_tile(mat_tab, blk_mat, blk_tile, blockIdx.x);
  const int tr = threadIdx.x >> 2, seg = (threadIdx.x & 3) * 16;
  const long e = (long)(t.r0 + tr) * t.cols + t.c0 + seg;
  float o[16], p[16];
  if (!t.tr) {
    load16<bf16_t>(O + t.work + e, o);
  } else {                               // O is [cols, rows]: stage its tile (c0.., r0..) and read columns
    const bf16_t* op = O + t.work + (long)(t.c0 + tr) * t.rows + t.r0 + seg;
    *reinterpret_cast<uint4*>(tile + tr * kTPitch + seg) = *reinterpret_cast<const uint4*>(op);
    *reinterpret_cast<uint4*>(tile + tr * kTPitch + seg + 8) = *reinterpret_cast<const uint4*>(op + 8);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = bf2f(tile[(seg + i) * kTPitch + tr]);
  }
  load16<float>(master + t.owner + e, p);
  const float sc = 0.2f * sqrtf((float)(t.rows > t.cols ? t.rows : t.cols));
#pragma unroll
  for (int i = 0; i < 16; ++i) p[i] -= lr * (sc * o[i] + wd * p[i]);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    *reinterpret_cast<float4*>(master + t.owner + e + 4 * q) = make_float4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
  *reinterpret_cast<uint4*>(t.dst + e) = pack8(p);
  *reinterpret_cast<uint4*>(t.dst + e + 8) = pack8(p + 8);
}

}  // namespace

bool dltb_muon_syrk_supported(int m, int k, int batch, int bt) {
  return m > 0 && k > 0 && batch > 0 && (bt == 64 || bt == 128) && m % bt == 0 && k % kBK == 0 &&
         (long)(m / bt) * (m / bt + 1) / 2 * batch < (1L << 30);
}

int dltb_muon_syrk(const void* x, const void* d, void* c, long ldx, long ldd, long ldc, long sx, long sd, long sc,
                   int m, int k, int batch, float alpha, float beta, const float* dalpha, long dalpha_stride, int bt,
                   hipStream_t st) {
  if (bt <= 0) bt = syrk_bt(m, k);
  if (!dltb_muon_syrk_supported(m, k, batch, bt)) return -1;
  if (ldx < k || ldc < m || (d && ldd < m) || ldx % 8 || ldc % 8 || (d && ldd % 4)) return -1;
  if (batch > 1 && (sx < 0 || sc < 0 || sd < 0)) return -1;
  // C is written while other tiles still read X and D
  const long cspan = span(sc, batch, ldc, m, m);
  if (overlaps(c, cspan, x, span(sx, batch, ldx, m, k))) return -2;
  if (d && overlaps(c, cspan, d, span(sd, batch, ldd, m, m))) return -2;
  SyrkArgs g{};
  g.x = (const bf16_t*)x;
  g.d = (const bf16_t*)d;
  g.c = (bf16_t*)c;
  g.dalpha = dalpha;
  g.ldx = ldx; g.ldd = ldd; g.ldc = ldc; g.sx = sx; g.sd = sd; g.sc = sc;
  g.dalpha_stride = dalpha_stride;
  g.alpha = alpha;
  g.beta = beta;
  g.m = m; g.k = k; g.batch = batch;
  if (bt == 128) launch_syrk<128>(g, st);
  else launch_syrk<64>(g, st);
  return bt;
}

bool dltb_muon_apply_supported(int m, int n, int batch, int cfg) {
  int BM, BN;
  if (!apply_tile(cfg, BM, BN)) return false;
  return m > 0 && n > 0 && batch > 0 && m % BM == 0 && n % BN == 0 && m % kBK == 0 &&
         (long)(m / BM) * (n / BN) * batch < (1L << 30);
}

int dltb_muon_apply(const void* b, const void* x, void* y, long ldb, long ldx, long ldy, long sb, long sx, long sy,
                    int m, int n, int batch, float alpha, float a, const float* dalpha, long dalpha_stride, int cfg,
                    hipStream_t st) {
  if (cfg < 0) cfg = apply_cfg(m, n, batch);
  if (!dltb_muon_apply_supported(m, n, batch, cfg)) return -1;
  if (ldb < m || ldx < n || ldy < n || ldb % 8 || ldx % 8 || ldy % 4) return -1;
  if (batch > 1 && (sb < 0 || sx < 0 || sy < 0)) return -1;
  // in place is a race: other tiles read X (and B) while this one writes Y
  const long yspan = span(sy, batch, ldy, m, n);
  if (overlaps(y, yspan, x, span(sx, batch, ldx, m, n))) return -2;
  if (overlaps(y, yspan, b, span(sb, batch, ldb, m, m))) return -2;
  ApplyArgs g{};
  g.b = (const bf16_t*)b;
  g.x = (const bf16_t*)x;
  g.y = (bf16_t*)y;
  g.dalpha = dalpha;
  g.ldb = ldb; g.ldx = ldx; g.ldy = ldy; g.sb = sb; g.sx = sx; g.sy = sy;
  g.dalpha_stride = dalpha_stride;
  g.alpha = alpha;
  g.a = a;
  g.m = m; g.n = n; g.batch = batch;
  switch (cfg) {
    case 0: launch_apply<128, 128>(g, st); break;
    case 1: launch_apply<128, 64>(g, st); break;
    case 2: launch_apply<64, 128>(g, st); break;
    default: launch_apply<64, 64>(g, st); break;
  }
  return cfg;
}

bool dltb_muon_matrix_supported(long rows, long cols) {
  return rows > 0 && cols > 0 && rows % kTile == 0 && cols % kTile == 0;
}

void dltb_muon_momentum(const void* grad, bool grad_bf16, float* mom, void* U, float* partial, float* norms,
                        const int64_t* mat_tab, int nmat, const int* blk_mat, const int* blk_tile, int nblocks,
                        const float* gscale, const float* hp, float mu, float eps, hipStream_t st) {
  if (nblocks <= 0 || nmat <= 0) return;
  if (grad_bf16)
    hipLaunchKernelGGL(muon_momentum_kernel<bf16_t>, dim3(nblocks), dim3(256), 0, st, (const bf16_t*)grad, mom,
                       (bf16_t*)U, partial, mat_tab, blk_mat, blk_tile, gscale, hp, mu);
  else
    hipLaunchKernelGGL(muon_momentum_kernel<float>, dim3(nblocks), dim3(256), 0, st, (const float*)grad, mom,
                       (bf16_t*)U, partial, mat_tab, blk_mat, blk_tile, gscale, hp, mu);
  hipLaunchKernelGGL(muon_norm_kernel, dim3(nmat), dim3(256), 0, st, partial, norms, mat_tab, hp, eps);
}

void dltb_muon_update(float* master, const void* O, const int64_t* mat_tab, const int* blk_mat, const int* blk_tile,
                      int nblocks, const float* hp, float lr, float wd, hipStream_t st) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(muon_update_kernel, dim3(nblocks), dim3(256), 0, st, master, (const bf16_t*)O, mat_tab, blk_mat,
                     blk_tile, hp, lr, wd);
}
