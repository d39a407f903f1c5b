// Row-scaled FP8 (OCP E4M3) linear layers on the CDNA4 FP8 matrix instruction (gfx950); built for bf16 and for
// fp16 like every kernel file (the 16-bit format is that of the quantiser's input and of the GEMM's output).
//
//   fp8_quant_rows:  x[R][K] 16-bit -> q[R][K] E4M3 codes, s[R] fp32; s = 2^e, the smallest power of two with
//                    max|x| / s <= 448 (e in [-126, 127]; 1 for an all-zero row, NaN for a row that holds an
//                    inf or a NaN, whose codes are 0); q = E4M3(x / s), round to nearest even.
//   gemm_fp8_nt:     c[M][N] = round16((acc * sa[m]) * sb[n]),  acc = sum_k dec(qa[m][k]) dec(qb[n][k])  in fp32
//
// Quantiser.  One wave per row, four rows per workgroup, no LDS and no atomics.  A lane holds 16-byte loads (8
// elements) of its row; the first 8 loads of a lane (4096 elements of the row per wave) stay in registers, so
// rows up to K = 4096 are read once and only the tail of a longer row (K up to 28672) is read a second time, from
// L2.  The row maximum is taken on the integer bits of |x| (NaN > inf > every finite value as unsigned integers),
// so the non-finite row needs no second flag; the exponent comes from the bits as in adamw.hip.  Codes are packed
// by v_cvt_pk_fp8_f32 and stored 8 bytes per lane.  A batch of equally spaced matrices (all layers' weights of one
// kind) is one launch.
//
// GEMM.  The k-step is 128 bytes = 128 E4M3 codes, so a stage image of an operand is byte for byte the
// 128-byte-row image GldsTile<64, ROWS> fills by LDS-DMA and swz<64> swizzles (mfma_tiles.h), and the ring is
// gemm.hip's: NSTAGE stages, counted vmcnt across a raw s_barrier.  Per k-step a wave issues two
// v_mfma_f32_32x32x64_f8f6f4 per 32 x 32 output tile; for instruction s (0, 1) the lane (r = lane & 31,
// h = lane >> 5) holds the 32 contiguous bytes [64 s + 32 h, + 32) of its row: chunks 4 s + 2 h and 4 s + 2 h + 1,
// two ds_read_b128.  Both operands use this read, so whatever k the hardware gives byte j of half h, the two
// fragments pair equal k.  Roles are swapped (srcA = B fragment) so the lane carries m: the epilogue reads one
// sa[m] per lane and tile row, four sb[n .. n + 3] per register group, and stores 8-byte vectors.
//
// Banks (on paper, as mfma_tiles.h does for row_frag): a ds_read_b128 is served 16 lanes at a time, conflict free
// when the 16 lanes touch 16 different 16-byte slots of the 256-byte bank row.  Lanes 16 g .. 16 g + 15 read ONE
// logical chunk c of 16 consecutive rows (h is constant inside a group of 16).  Row bit 0 picks the 128-byte half
// of the bank row, and swz<64> maps row bits 1..3 one-to-one onto the 8 values XORed into c, so the 16 rows land
// on 16 distinct slots for every c: each of the two reads is conflict free, exactly row_frag's argument.
//
// Tiles and walk, for the Mistral-7B products (rows 4096 .. 16384; (N, K) = (6144, 4096), (4096, 4096),
// (28672, 4096), (4096, 14336) and the transposes):
//   * 256 x 128 (wave 128 x 64, 3 stages of 48 KiB): per k-step a wave runs 16 MFMAs (1024 cycles) against 24
//     ds_read_b128, i.e. 96 KiB of LDS reads per workgroup = 768 cycles at 128 B/clk: the MFMAs cover the reads.
//     Taken when M % 256 == 0 and the grid still has a tile per CU.
//   * 128 x 128 (wave 64 x 64, 4 stages of 32 KiB): 8 MFMAs (512 cycles) against 512 cycles of LDS reads, the
//     fallback for every other supported shape (all of M, N, K multiples of 128).
//   * a 256 x 256 tile would halve the LDS traffic again but leaves room for two 64 KiB stages only; not built.
//   * walk: XCD-major (consecutive workgroups go to different XCDs) in groups of gm row-blocks x all column
//     blocks, so the 32 tiles an XCD runs together form a gm x (32 / gm) patch: at gm = 4 they request 1.5 MiB
//     per k-step of which 256 KiB is distinct (6 x reuse in the XCD's L2; 2.8 x at gm = 1).
//   * no split-K: the smallest M7B product (4096 x 4096 x 4096) already has 512 tiles of 256 x 128, two per CU.
#include "common.h"
#include "launchers.h"
#include "mfma_tiles.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------ quantiser
constexpr int kQKeep = 8;                       // 16-byte loads of a lane that stay in registers

DLTB_DEV uint32_t abs_bits(float f) { return __float_as_uint(f) & 0x7FFFFFFFu; }
DLTB_DEV uint32_t amax_bits8(const uint4& v) {
  float f[8];
  unpack8(v, f);
  uint32_t a = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) a = max(a, abs_bits(f[k]));
  return a;
}
DLTB_DEV uint2 quant8(const uint4& v, float inv, bool zero) {
  float f[8];
  unpack8(v, f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * inv, f[1] * inv, 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * inv, f[3] * inv, lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * inv, f[5] * inv, 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * inv, f[7] * inv, hi, true);
  return zero ? make_uint2(0u, 0u) : make_uint2((uint32_t)lo, (uint32_t)hi);
}

// rows: nb * R; x row r of matrix b at x + b * xbs + r * ldx (elements); q / s contiguous [nb][R][K] / [nb][R]
__global__ __launch_bounds__(256) void fp8_quant_rows_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ q,
                                                             float* __restrict__ s, int R, int K, long rows, long ldx,
                                                             long xbs) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long b = row / R, r = row % R;
  const bf16_t* xr = x + b * xbs + r * ldx;
  const int nch = K >> 3;                       // 16-byte chunks of the row
  uint4 keep[kQKeep];
  uint32_t a = 0;
#pragma unroll
  for (int i = 0; i < kQKeep; ++i) {
    const int c = i * 64 + lane;
    keep[i] = c < nch ? ld16<uint4>(xr + (long)c * 8) : make_uint4(0u, 0u, 0u, 0u);
    a = max(a, amax_bits8(keep[i]));
  }
  for (int c = kQKeep * 64 + lane; c < nch; c += 64) a = max(a, amax_bits8(ld16<uint4>(xr + (long)c * 8)));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = max(a, (uint32_t)__shfl_xor((int)a, o, 64));
  // exponent of the scale: 0 for a zero row, else the smallest e >= -126 with amax * 2^-e <= 448 = 1.75 * 2^8
  // (a mantissa above 1.75 needs one more); 16-bit inputs stay below 2^128, so e <= 120 and 2^-e is normal
  const bool bad = a >= 0x7F800000u;
  int e = (int)((a + 0x1FFFFFu) >> 23) - 135;
  e = a == 0u ? 0 : (e < -126 ? -126 : e);
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23);
  if (lane == 0) s[row] = bad ? __uint_as_float(0x7FC00000u) : __uint_as_float((uint32_t)(e + 127) << 23);
  uint8_t* qr = q + row * (long)K;
#pragma unroll
  for (int i = 0; i < kQKeep; ++i) {
    const int c = i * 64 + lane;
    if (c < nch) *reinterpret_cast<uint2*>(qr + (long)c * 8) = quant8(keep[i], inv, bad);
  }
  for (int c = kQKeep * 64 + lane; c < nch; c += 64)
    *reinterpret_cast<uint2*>(qr + (long)c * 8) = quant8(ld16<uint4>(xr + (long)c * 8), inv, bad);
}

// ------------------------------------------------------------------------------------------------ GEMM
constexpr int kKB = 128;                        // bytes (= codes) of one k-step

struct Fp8GemmArgs {
  const uint8_t* a;     // [M][K] codes, row stride lda bytes
  const uint8_t* b;     // [N][K] codes, row stride ldb bytes
  const float* sa;      // [M]
  const float* sb;      // [N]
  bf16_t* c;            // [M][N], row stride ldc elements
  long lda, ldb, ldc;
  int M, N, K;
  int gm;               // tile order: groups of gm row-blocks x all column-blocks
};

DLTB_DEV f32x16 mfma_fp8(i32x8 a, i32x8 b, f32x16 c) {
  // cbsz = blgp = 0: both operands E4M3; zero scale operands select the unscaled v_mfma_f32_32x32x64_f8f6f4
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);
}

// the lane's 32 bytes of tile row `row` for instruction s: chunks 4 s + 2 h and 4 s + 2 h + 1
DLTB_DEV i32x8 fp8_frag(const char* tile, int row, int s, int h) {
  const uint4 lo = *reinterpret_cast<const uint4*>(tile + toff<64>(row, 4 * s + 2 * h));
  const uint4 hi = *reinterpret_cast<const uint4*>(tile + toff<64>(row, 4 * s + 2 * h + 1));
  i32x8 f = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  return f;
}

template <int BM, int BN, int NSTAGE>
__global__ __launch_bounds__(256, 1) void gemm_fp8_kernel(Fp8GemmArgs g) {
  constexpr int A_BYTES = BM * kKB, B_BYTES = BN * kKB, STAGE = A_BYTES + B_BYTES;
  constexpr int WM = BM / 2, WN = BN / 2;          // wave tile (2 x 2 waves)
  constexpr int FM = WM / 32, FN = WN / 32;        // 32 x 32 MFMA tiles per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r = lane & 31;
  const int wm = w & 1, wn = w >> 1;
  const int wv = __builtin_amdgcn_readfirstlane(w);
  // ---- tile coordinates: XCD-major walk, then groups of gm row-blocks
  const int tiles_n = g.N / BN, tiles_m = g.M / BM, tiles = tiles_m * tiles_n;
  const int idx = xcd_grouped(blockIdx.x, tiles);
  int mb = idx / tiles_n, nb = idx % tiles_n;
  if (g.gm > 1 && tiles_m % g.gm == 0) {
    const int grp = idx / (g.gm * tiles_n), in = idx % (g.gm * tiles_n);
    mb = grp * g.gm + in % g.gm;
    nb = in / g.gm;
  }
  const int m0 = mb * BM, n0 = nb * BN;
  const int nk = g.K / kKB;
  DLTB_DCHECK(m0 + BM <= g.M && n0 + BN <= g.N && nk > 0);

  // the image rows are 128 bytes = 64 "16-bit elements" to GldsTile: byte strides halve
  auto load_stage = [&](int kt, int st) {
    char* sa = smem + st * STAGE;
    char* sb = sa + A_BYTES;
    const long k0 = (long)kt * kKB;
    GldsTile<64, BM, true>::load(reinterpret_cast<const bf16_t*>(g.a + k0), g.lda >> 1, m0, sa, wv, lane);
    GldsTile<64, BN, true>::load(reinterpret_cast<const bf16_t*>(g.b + k0), g.ldb >> 1, n0, sb, wv, lane);
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x16{};

  // NSTAGE-deep ring, counted vmcnt: only the stage about to be read is retired (gemm.hip)
  constexpr int GLDS = GldsTile<64, BM>::NI + GldsTile<64, BN>::NI;
  static_assert(2 * GLDS < 64, "vmcnt range");
  static_assert(NSTAGE >= 3 && NSTAGE <= 4, "the waits below cover up to two stages in flight");
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
    const char* sa = smem + (kt % NSTAGE) * STAGE;
    const char* sb = sa + A_BYTES;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      i32x8 fa[FM], fb[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) fa[i] = fp8_frag(sa, wm * WM + 32 * i + r, s, h);
#pragma unroll
      for (int j = 0; j < FN; ++j) fb[j] = fp8_frag(sb, wn * WN + 32 * j + r, s, h);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = mfma_fp8(fb[j], fa[i], acc[i][j]);   // lane <-> m
    }
    // the NEXT iteration's barrier orders these LDS reads before stage kt's buffer is refilled
  }

  // ---- epilogue: lane -> row m (one sa), register group q -> columns n .. n + 3 (four sb)
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + wm * WM + 32 * i + r;
    const float sam = g.sa[m];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * WN + 32 * j + 8 * q + 4 * h;
        const float4 sbn = *reinterpret_cast<const float4*>(g.sb + n);
        uint2 o;
        o.x = pack_bf2((acc[i][j][4 * q] * sam) * sbn.x, (acc[i][j][4 * q + 1] * sam) * sbn.y);
        o.y = pack_bf2((acc[i][j][4 * q + 2] * sam) * sbn.z, (acc[i][j][4 * q + 3] * sam) * sbn.w);
        *reinterpret_cast<uint2*>(g.c + (size_t)m * g.ldc + n) = o;
      }
    }
  }
}

template <int BM, int BN, int NSTAGE>
void launch_fp8(const Fp8GemmArgs& g, hipStream_t st) {
  constexpr int smem = NSTAGE * (BM + BN) * kKB;
  allow_dynamic_lds<gemm_fp8_kernel<BM, BN, NSTAGE>>(smem);
  const int tiles = (g.M / BM) * (g.N / BN);
  hipLaunchKernelGGL((gemm_fp8_kernel<BM, BN, NSTAGE>), dim3(tiles), dim3(256), smem, st, g);
}

}  // namespace

void dltb_fp8_quant_rows(const void* x, uint8_t* q, float* s, int R, int K, int nb, long ldx, long xbs,
                         hipStream_t st) {
  const long rows = (long)nb * R;
  if (rows <= 0) return;
  hipLaunchKernelGGL(fp8_quant_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const bf16_t*)x, q, s,
                     R, K, rows, ldx, xbs);
}

bool dltb_gemm_fp8_supported(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && M % 128 == 0 && N % 128 == 0 && K % kKB == 0;
}

// cfg 0 = 128 x 128, 1 = 256 x 128; -1: 256 x 128 where M allows it and the grid keeps a tile per CU
int dltb_gemm_fp8_pick(int M, int N, int K) {
  (void)K;
  return (M % 256 == 0 && (long)(M / 256) * (N / 128) >= 256) ? 1 : 0;
}

int dltb_gemm_fp8(const uint8_t* a, const float* sa, const uint8_t* b, const float* sb, void* c, long lda, long ldb,
                  long ldc, int M, int N, int K, int cfg, hipStream_t st) {
  if (!dltb_gemm_fp8_supported(M, N, K) || cfg > 1) return -1;
  if (cfg < 0) cfg = dltb_gemm_fp8_pick(M, N, K);
  if (cfg == 1 && M % 256) return -1;
  Fp8GemmArgs g{};
  g.a = a;
  g.b = b;
  g.sa = sa;
  g.sb = sb;
  g.c = (bf16_t*)c;
  g.lda = lda;
  g.ldb = ldb;
  g.ldc = ldc;
  g.M = M;
  g.N = N;
  g.K = K;
  const int tiles_m = M / (cfg == 1 ? 256 : 128);
  g.gm = tiles_m % 4 == 0 ? 4 : (tiles_m % 2 == 0 ? 2 : 1);
  if (cfg == 1) launch_fp8<256, 128, 3>(g, st);
  else launch_fp8<128, 128, 4>(g, st);
  return cfg;
}
