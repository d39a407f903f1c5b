// Sandwich norm for gfx950: a sublayer's output goes through its own RMSNorm BEFORE it joins the residual stream
// ("normalise, then add"; Gemma-2 / Gemma-3, the placement of OLMo-2 and Grok-1), where csrc/norm.hip can only add
// first and normalise after.
//
// Forward, sandwich_fwd(x, a, w_out, w_next | none):
//     rstd_a = rsqrt(mean(a^2) + eps)
//     s      = round16(x + a * rstd_a * w_out)        the normalised value lives in fp32 registers only
//     rstd_s = rsqrt(mean(s^2) + eps),  y = round16(s * rstd_s * w_next)      (NEXT; from the STORED s, as norm_fwd)
// One 64-lane wave per row, the row held in registers as 16-byte vectors, fp32 statistics (norm_fwd_row's shape).
// The attention site (NEXT) reads x, a and writes s, y: four row passes in one launch instead of norm_fwd(a) +
// norm_fwd(x, n)'s six in two.  The FFN site (!NEXT) writes s alone: the next layer's input norm belongs to the
// next unit.  y's element expression is norm_apply's on the same fp32 inputs, so norm_apply(s, w_next, rstd_s)
// rebuilds y bit for bit.  Every d % 8 == 0 up to 4096 (the nv_for ladder of csrc/norm.hip).  No LDS, no scratch,
// no atomics.
//
// Backward of the attention site, sandwich_bwd(dy, s, w_next, rstd_s, dres, a, w_out, rstd_a):
//     ds = dres + RMSNormBwd(dy; s, w_next, rstd_s),   dx = round16(ds)
//     da = round16(RMSNormBwd(dx; a, w_out, rstd_a))                          (from the STORED dx)
//     part[0][block] = sum_rows dy * s * rstd_s   (gradient of w_next),
//     part[1][block] = sum_rows dx * a * rstd_a   (gradient of w_out)         fp32, one row per workgroup
// One launch and six row passes (dy, s, dres, a in; dx, da out) where two norm_bwd calls need seven (dx is written
// and read back).  norm_bwd_fused_kernel's shape: a wave owns `rpw` consecutive rows and keeps both weights'
// column sums in registers; the 8 waves fold through one [8][d] fp32 LDS image, one partial at a time; the
// partials reach the gradient slots through colreduce_multi in a fixed order.  No atomics on global memory.
// LIMIT: d % 8 == 0 and d <= 2048 (at most 4 register slices: two column accumulators and two rows' operands fit
// the 256 registers of a 512-thread workgroup without scratch -- the compiler reports 256 VGPRs and no scratch at 4
// slices, 432 bytes of scratch per lane at 6 and 880 at 8, profiles/sandwich_norm_resources.txt -- and the fold
// image fits 64 KiB of LDS).  Wider rows (dltb_sandwich_bwd_supported false; M7B's 4096) take the two norm_bwd
// calls, which obey the same contract.
#include "common.h"
#include "launchers.h"

namespace {

constexpr int kWaves = 4;          // forward: one row per wave
constexpr int kBwdWaves = 8;       // backward: 512-thread blocks, as norm_bwd_fused_kernel

template <int NV, bool NEXT>
__global__ __launch_bounds__(256) void sandwich_fwd_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ a, const bf16_t* __restrict__ w_out,
    const bf16_t* __restrict__ w_next, bf16_t* __restrict__ s_out, bf16_t* __restrict__ y,
    float* __restrict__ rstd_a_out, float* __restrict__ rstd_s_out, int N, int d, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= N) return;
  const int nvec = d >> 3;
  const size_t base = (size_t)row * d;
  float v[NV][8];
  uint4 woraw[NV], wnraw[NV], xraw[NV];   // weights and x issued first: their latency hides under the statistics
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int idx = j * 64 + lane;
    if (idx < nvec) {
      woraw[j] = ld16<uint4>(w_out + idx * 8);
      if (NEXT) wnraw[j] = ld16<uint4>(w_next + idx * 8);
    }
  }
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int idx = j * 64 + lane;
    if (idx < nvec) {
      unpack8(ld16<uint4>(a + base + idx * 8), v[j]);
      xraw[j] = ld16<uint4>(x + base + idx * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) sq += v[j][e] * v[j][e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
    }
  }
  const float rstd_a = rsqrtf(wave_sum(sq) / (float)d + eps);
  sq = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int idx = j * 64 + lane;
    if (idx < nvec) {
      float xv[8], wv[8], o[8];
      unpack8(xraw[j], xv);
      unpack8(woraw[j], wv);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = xv[e] + v[j][e] * rstd_a * wv[e];
      const uint4 ov = pack8(o);
      *reinterpret_cast<uint4*>(s_out + base + idx * 8) = ov;
      if (NEXT) {
        unpack8(ov, v[j]);                               // the statistics of the stored, rounded s
#pragma unroll
        for (int e = 0; e < 8; ++e) sq += v[j][e] * v[j][e];
      }
    }
  }
  if (lane == 0) rstd_a_out[row] = rstd_a;
  if (!NEXT) return;
  const float rstd = rsqrtf(wave_sum(sq) / (float)d + eps);
  if (lane == 0) rstd_s_out[row] = rstd;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int idx = j * 64 + lane;
    if (idx < nvec) {
      float wv[8], o[8];
      unpack8(wnraw[j], wv);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = v[j][e] * rstd * wv[e];
      *reinterpret_cast<uint4*>(y + base + idx * 8) = pack8(o);
    }
  }
}

// part: [2][gridDim.x][d].  The weights are re-read per row (L1 / L2 hits: d * 2 bytes against the row's 6 d * 2
// from and to HBM) so that the registers go to the two accumulators and the rows in flight.
template <int NV>
__global__ __launch_bounds__(kBwdWaves * 64) void sandwich_bwd_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ s, const bf16_t* __restrict__ w_next,
    const float* __restrict__ rstd_s_in, const bf16_t* __restrict__ dres, const bf16_t* __restrict__ a,
    const bf16_t* __restrict__ w_out, const float* __restrict__ rstd_a_in, bf16_t* __restrict__ dx,
    bf16_t* __restrict__ da, float* __restrict__ part, int N, int d, int rpw) {
  extern __shared__ __attribute__((aligned(16))) float fold[];   // [kBwdWaves][d]
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nvec = d >> 3;
  float acc[2][NV][8];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[k][j][e] = 0.f;
  const int r0 = (blockIdx.x * kBwdWaves + wid) * rpw;
  const int r1 = min(N, r0 + rpw);
  for (int row = r0; row < r1; ++row) {                  // wave-uniform trip count
    const size_t base = (size_t)row * d;
    const float rs = rstd_s_in[row], ra = rstd_a_in[row];
    float g[NV][8], xh[NV][8];
    uint4 rraw[NV], araw[NV];                            // the residual gradient and a: issued with dy / s, so
#pragma unroll                                           // their latency hides under the first row reduction
    for (int j = 0; j < NV; ++j) {
      const int idx = j * 64 + lane;
      if (idx < nvec) {
        rraw[j] = ld16<uint4>(dres + base + idx * 8);
        araw[j] = ld16<uint4>(a + base + idx * 8);
      }
    }
    float s2 = 0.f;                                      // sum(w_next * dy * shat)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = j * 64 + lane;
      if (idx < nvec) {
        float dyv[8], sv[8], wv[8];
        unpack8(ld16<uint4>(dy + base + idx * 8), dyv);
        unpack8(ld16<uint4>(s + base + idx * 8), sv);
        unpack8(ld16<uint4>(w_next + idx * 8), wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[j][e] = sv[e] * rs;
          g[j][e] = dyv[e] * wv[e];
          s2 += g[j][e] * xh[j][e];
          acc[0][j][e] += dyv[e] * xh[j][e];
        }
      }
    }
    s2 = wave_sum(s2) / (float)d;
    float t2 = 0.f;                                      // sum(w_out * dx * ahat)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = j * 64 + lane;
      if (idx < nvec) {
        float o[8], rv[8], av[8], wv[8];
        unpack8(rraw[j], rv);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = rs * (g[j][e] - xh[j][e] * s2) + rv[e];
        const uint4 ov = pack8(o);
        *reinterpret_cast<uint4*>(dx + base + idx * 8) = ov;
        unpack8(ov, o);                                  // the second norm's backward reads the stored dx
        unpack8(araw[j], av);
        unpack8(ld16<uint4>(w_out + idx * 8), wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[j][e] = av[e] * ra;
          g[j][e] = o[e] * wv[e];
          t2 += g[j][e] * xh[j][e];
          acc[1][j][e] += o[e] * xh[j][e];
        }
      }
    }
    t2 = wave_sum(t2) / (float)d;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = j * 64 + lane;
      if (idx < nvec) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ra * (g[j][e] - xh[j][e] * t2);
        *reinterpret_cast<uint4*>(da + base + idx * 8) = pack8(o);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (k) __syncthreads();                              // the previous partial has been read
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = j * 64 + lane;
      if (idx < nvec) {
        float4* f = reinterpret_cast<float4*>(fold + wid * d + idx * 8);
        f[0] = make_float4(acc[k][j][0], acc[k][j][1], acc[k][j][2], acc[k][j][3]);
        f[1] = make_float4(acc[k][j][4], acc[k][j][5], acc[k][j][6], acc[k][j][7]);
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += kBwdWaves * 64) {
      float t = 0.f;
#pragma unroll
      for (int v = 0; v < kBwdWaves; ++v) t += fold[v * d + c];
      part[((size_t)k * gridDim.x + blockIdx.x) * d + c] = t;
    }
  }
}

#ifdef DLTB_SANDWICH_BWD_WIDE
// the rungs the launcher does not take, built by scripts/sandwich_resources.py alone to record why (scratch)
#define DLTB_SB_WIDE(NVV)                                                                                          \
  template __global__ void sandwich_bwd_kernel<NVV>(const bf16_t*, const bf16_t*, const bf16_t*, const float*,     \
                                                    const bf16_t*, const bf16_t*, const bf16_t*, const float*,     \
                                                    bf16_t*, bf16_t*, float*, int, int, int)
DLTB_SB_WIDE(6);
DLTB_SB_WIDE(8);
#undef DLTB_SB_WIDE
#endif

int nv_for(int d) {                // csrc/norm.hip's ladder
  int nv = cdiv(d / 8, 64);
  if (nv == 5) nv = 6;
  if (nv == 7) nv = 8;
  return nv;
}

template <bool NEXT>
void launch_fwd(int N, int d, hipStream_t st, const bf16_t* x, const bf16_t* a, const bf16_t* w_out,
                const bf16_t* w_next, bf16_t* s, bf16_t* y, float* rstd_a, float* rstd_s, float eps) {
  const dim3 grid(cdiv(N, kWaves));
#define DLTB_SF(NVV)                                                                                      \
  hipLaunchKernelGGL((sandwich_fwd_kernel<NVV, NEXT>), grid, dim3(256), 0, st, x, a, w_out, w_next, s, y, \
                     rstd_a, rstd_s, N, d, eps)
  switch (nv_for(d)) {
    case 1: DLTB_SF(1); break;
    case 2: DLTB_SF(2); break;
    case 3: DLTB_SF(3); break;
    case 4: DLTB_SF(4); break;
    case 6: DLTB_SF(6); break;
    default: DLTB_SF(8); break;
  }
#undef DLTB_SF
}

int bwd_rpw(int N) {               // rows per wave chosen for >= 256 workgroups
  const int rpw = N / (kBwdWaves * 256);
  return rpw < 1 ? 1 : rpw;
}

}  // namespace

// ---------------------------------------------------------------------------------------- API
void dltb_sandwich_fwd(const void* x, const void* a, const void* w_out, const void* w_next, void* s, void* y,
                       float* rstd_a, float* rstd_s, int N, int d, float eps, hipStream_t st) {
  if (N <= 0) return;
  if (w_next)
    launch_fwd<true>(N, d, st, (const bf16_t*)x, (const bf16_t*)a, (const bf16_t*)w_out, (const bf16_t*)w_next,
                     (bf16_t*)s, (bf16_t*)y, rstd_a, rstd_s, eps);
  else
    launch_fwd<false>(N, d, st, (const bf16_t*)x, (const bf16_t*)a, (const bf16_t*)w_out, nullptr, (bf16_t*)s,
                      nullptr, rstd_a, nullptr, eps);
}

bool dltb_sandwich_bwd_supported(int d) { return d > 0 && d % 8 == 0 && nv_for(d) <= 4; }

int dltb_sandwich_bwd_blocks(int N) { return N > 0 ? cdiv(N, kBwdWaves * bwd_rpw(N)) : 1; }

bool dltb_sandwich_bwd(const void* dy, const void* s, const void* w_next, const float* rstd_s, const void* dres,
                       const void* a, const void* w_out, const float* rstd_a, void* dx, void* da, float* part,
                       int N, int d, hipStream_t st) {
  if (!dltb_sandwich_bwd_supported(d)) return false;
  const dim3 grid(dltb_sandwich_bwd_blocks(N));
  const size_t lds = (size_t)kBwdWaves * d * sizeof(float);          // <= 64 KiB at d <= 2048
#define DLTB_SB(NVV)                                                                                           \
  hipLaunchKernelGGL((sandwich_bwd_kernel<NVV>), grid, dim3(kBwdWaves * 64), lds, st, (const bf16_t*)dy,       \
                     (const bf16_t*)s, (const bf16_t*)w_next, rstd_s, (const bf16_t*)dres, (const bf16_t*)a,   \
                     (const bf16_t*)w_out, rstd_a, (bf16_t*)dx, (bf16_t*)da, part, N, d, bwd_rpw(N))
  switch (nv_for(d)) {
    case 1: DLTB_SB(1); break;
    case 2: DLTB_SB(2); break;
    case 3: DLTB_SB(3); break;
    default: DLTB_SB(4); break;
  }
#undef DLTB_SB
  return true;
}
