// 16-bit GEMM on MFMA, NN layout (gfx950): the tied LM head's data gradient dX = g dL W.
//
//   C[M, N] = alpha * sum_k A[m, k] B[k, n]        fp32 accumulate, alpha an optional device scalar
//
//   A stored [M][K] (K-contiguous, rows may be strided), B stored [K][N] (N-contiguous, rows may be
//   strided): dL [tokens, V] and W [V, d] as the model keeps them, no transposed copy of W.
//
// The machinery is gemm.hip's: block = 4 waves (2 x 2), tile BM x BN x 64, an LDS ring filled by
// LDS-DMA one to three k-steps ahead and retired by a counted vmcnt, swapped MFMA roles so the
// epilogue stores 8-byte vectors, the XCD-major tile walk, and split-K through fp32 partials and
// gemm_splitk_reduce (alpha is applied there when splits > 1, in the epilogue otherwise).
//
// Operand images: A is the NT image (BM rows of 64 k, read by row_frag), B the TN image (64 k-rows
// of BN, read by tr_frag; BN <= 128 for the swizzle).  The two reads deliver different k orders
// inside a 16-deep MFMA step (mfma_tiles.h), so B is staged with GldsTile's KSWAP: image row r of
// each 16-row group holds source k-row swap23(r), and tr_frag then hands out row_frag's order.
// LDS banking, checked against swz<> on paper: both reads are the ones gemm.hip already issues on
// the same images at the same LDS addresses (the permutation is on the global side of the DMA
// only), so both stay conflict-free.  The other way to match the orders, reading A in tr_frag's
// order with two ds_read_b64 per fragment, is 2-way conflicted under swz<64> (each 32-lane half
// covers only 32 of the 64 banks; mfma_tiles.h) and would double the LDS cycles of the operand
// that has FM = up to 4 fragments per k16 step; it is not used.
// On the global side a wave-instruction of the B stage still fetches whole 128- or 256-byte rows.
#include "common.h"
#include "gemm_common.h"
#include "launchers.h"
#include "mfma_tiles.h"

namespace {

template <int BM, int BN>
struct GeoNN {
  static constexpr int A_BYTES = BM * kBK * 2;
  static constexpr int B_BYTES = BN * kBK * 2;
  static constexpr int STAGE = A_BYTES + B_BYTES;
  static constexpr int NSTAGE = STAGE <= 32768 ? 4 : 3;   // <= 144 KiB of the CU's 160 KiB
  static constexpr int SMEM = NSTAGE * STAGE;
};

template <int BM, int BN>
__global__ __launch_bounds__(256, 1) void gemm_nn_kernel(GemmArgs g) {
  using G = GeoNN<BM, BN>;
  constexpr int NSTAGE = G::NSTAGE;
  constexpr int WM = BM / 2, WN = BN / 2;          // wave tile
  constexpr int FM = WM / 32, FN = WN / 32;        // 32x32 MFMA tiles per wave
  static_assert(BN <= 128, "TN image rows are <= 128 elements");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r = lane & 31;
  const int wm = w & 1, wn = w >> 1;
  const int wv = __builtin_amdgcn_readfirstlane(w);
  // ---- tile coordinates (XCD-major walk), split index
  const int tiles_n = g.N / BN, tiles_m = g.M / BM, tiles = tiles_m * tiles_n;
  const int splits = gridDim.x / tiles;
  int L = blockIdx.x;
  const int split = L / tiles;
  L -= split * tiles;
  int idx = L;
  if ((tiles & 7) == 0) idx = (L & 7) * (tiles >> 3) + (L >> 3);
  int mb = idx / tiles_n, nb = idx % tiles_n;
  if (g.gm > 1 && tiles_m % g.gm == 0) {          // grouped order: gm row-blocks x all column-blocks
    const int grp = idx / (g.gm * tiles_n), in = idx % (g.gm * tiles_n);
    mb = grp * g.gm + in % g.gm;
    nb = in / g.gm;
  }
  const int m0 = mb * BM, n0 = nb * BN;
  const int kbeg = split * g.ksplit;
  const int nk = min(g.ksplit, g.K - kbeg) / kBK;
  DLTB_DCHECK(m0 + BM <= g.M && n0 + BN <= g.N && kbeg + nk * kBK <= g.K && nk > 0);

  auto load_stage = [&](int kt, int st) {
    char* sa = smem + st * G::STAGE;
    char* sb = sa + G::A_BYTES;
    const int k0 = kbeg + kt * kBK;
    GldsTile<64, BM, true>::load(g.a + k0, g.lda, m0, sa, wv, lane);
    GldsTile<BN, kBK, true, true>::load(g.b + n0, g.ldb, k0, sb, wv, lane);   // k-rows in row_frag's order
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x16{};

  // NSTAGE-deep ring, counted vmcnt across the raw s_barrier (gemm.hip)
  constexpr int GLDS = GldsTile<64, BM>::NI + GldsTile<BN, kBK>::NI;
  static_assert(2 * GLDS < 64, "vmcnt range");
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
    const char* sa = smem + (kt % NSTAGE) * G::STAGE;
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
    // the NEXT iteration's barrier orders these LDS reads before stage kt's buffer is refilled
  }

  // ---- epilogue: lane -> row m, register group q -> columns n .. n+3
  const float al = (g.alpha && splits == 1) ? *g.alpha : 1.f;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + wm * WM + 32 * i + r;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * WN + 32 * j + 8 * q + 4 * h;
        const float v[4] = {acc[i][j][4 * q] * al, acc[i][j][4 * q + 1] * al, acc[i][j][4 * q + 2] * al,
                            acc[i][j][4 * q + 3] * al};
        if (splits > 1) {
          *reinterpret_cast<float4*>(g.part + ((size_t)split * g.M + m) * g.N + n) = make_float4(v[0], v[1], v[2], v[3]);
          continue;
        }
        uint2 o;
        o.x = pack_bf2(v[0], v[1]);
        o.y = pack_bf2(v[2], v[3]);
        *reinterpret_cast<uint2*>(g.c + (size_t)m * g.ldc + n) = o;
      }
    }
  }
}

template <int BM, int BN>
void launch_nn(const GemmArgs& g, int splits, hipStream_t st) {
  constexpr int smem = GeoNN<BM, BN>::SMEM;
  allow_dynamic_lds<gemm_nn_kernel<BM, BN>>(smem);
  const int tiles = (g.M / BM) * (g.N / BN);
  hipLaunchKernelGGL((gemm_nn_kernel<BM, BN>), dim3(tiles * splits), dim3(256), smem, st, g);
}

// tile configs (BM x BN): 0 = 128x128, 1 = 256x128, 2 = 64x64
bool nn_tile(int cfg, int& BM, int& BN) {
  static const int t[3][2] = {{128, 128}, {256, 128}, {64, 64}};
  if (cfg < 0 || cfg > 2) return false;
  BM = t[cfg][0];
  BN = t[cfg][1];
  return true;
}

}  // namespace

bool dltb_gemm_nn_supported(int M, int N, int K, int cfg) {
  int BM, BN;
  if (!nn_tile(cfg, BM, BN)) return false;
  return M > 0 && N > 0 && K > 0 && M % BM == 0 && N % BN == 0 && K % kBK == 0;
}

int dltb_gemm_nn(const void* a, const void* b, void* c, float* part, long lda, long ldb, long ldc, int M, int N,
                 int K, int splits, int cfg, int gm, const float* alpha, hipStream_t st) {
  if (!dltb_gemm_nn_supported(M, N, K, cfg)) return -1;
  GemmArgs g{};
  g.a = (const bf16_t*)a;
  g.b = (const bf16_t*)b;
  g.c = (bf16_t*)c;
  g.alpha = alpha;
  g.gm = gm;
  g.lda = lda;
  g.ldb = ldb;
  g.ldc = ldc;
  g.M = M;
  g.N = N;
  g.K = K;
  g.ksplit = gemm_ksplit(K, splits);
  g.part = splits > 1 ? part : nullptr;
  if (splits > 1 && !part) return -1;
  switch (cfg) {
    case 1: launch_nn<256, 128>(g, splits, st); break;
    case 2: launch_nn<64, 64>(g, splits, st); break;
    default: launch_nn<128, 128>(g, splits, st); break;
  }
  if (splits > 1) {
    long grid = ((long)M * N / 4 + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(gemm_splitk_reduce, dim3(grid), dim3(256), 0, st, g, splits);
  }
  return splits;
}
