// QK-norm fused with RoPE for gfx950: RMSNorm over head_dim of every query and key head, then the rotate-half
// RoPE of elementwise.hip's rope_kernel, in ONE in-place streaming pass over the q|k columns of a fused qkv buffer
// (16-bit I/O as 16-byte vectors, fp32 math, one rounding).
//
//   qknorm_rope_fwd   y = RoPE(x * rsqrt(mean(x^2) + eps) * w) in place; raw = x (contiguous copy, for the backward)
//   qknorm_rope_bwd   g = R(-theta) dy;  rstd from raw;  xh = x rstd;  dx = rstd (g w - xh mean(g w xh)) in place;
//                     fp32 per-workgroup partials of sum_{rows, heads} g xh for the q heads and for the k heads
//
// Lane mapping (rope_kernel's): a lane holds the 8 pairs (p0 + e, p0 + e + D/2) of one head, so a head spans
// L = D / 16 adjacent lanes (4 for D = 64, 8 for D = 128) of one wave, with two 16-byte loads per lane and operand.
// The head's sum of squares and the backward's mean(g w xh) are xor-shuffles inside that lane group: no LDS, no
// block barrier.  The backward's column sums stay in registers over a workgroup's rows (a thread's p0 is fixed:
// 256 % L == 0), are folded over the wave by shuffles and over the four waves through LDS once at the end, in a
// fixed order and without atomics.
#include "common.h"
#include "launchers.h"

namespace {

// sum over the L adjacent lanes of a head (L = 4 or 8; the group is aligned, so xor stays inside it)
template <int L>
DLTB_DEV float head_sum(float v) {
#pragma unroll
  for (int o = 1; o < L; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int D>
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(bf16_t* __restrict__ qkv, bf16_t* __restrict__ raw,
                                                             const bf16_t* __restrict__ wq,
                                                             const bf16_t* __restrict__ wk,
                                                             const float* __restrict__ cosb,
                                                             const float* __restrict__ sinb, int N, int T, int Hq,
                                                             int heads, int stride, float eps) {
  constexpr int half = D / 2, L = D / 16;
  const long total = (long)N * heads * L;                 // a multiple of L, as is every lane's stride
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / (heads * L);
    const int rem = (int)(i - row * heads * L);
    const int h = rem / L;
    const int p0 = (rem - h * L) * 8;
    const int t = (int)(row % T);
    bf16_t* base = qkv + row * stride + (long)h * D;
    bf16_t* rbase = raw + (row * heads + h) * (long)D;
    const uint4 u1 = ld16<uint4>(base + p0), u2 = ld16<uint4>(base + half + p0);
    *reinterpret_cast<uint4*>(rbase + p0) = u1;
    *reinterpret_cast<uint4*>(rbase + half + p0) = u2;
    float x1[8], x2[8], w1[8], w2[8], o1[8], o2[8];
    unpack8(u1, x1);
    unpack8(u2, x2);
    const bf16_t* w = h < Hq ? wq : wk;
    unpack8(ld16<uint4>(w + p0), w1);
    unpack8(ld16<uint4>(w + half + p0), w2);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += x1[e] * x1[e] + x2[e] * x2[e];
    const float rstd = rsqrtf(head_sum<L>(ss) * (1.f / D) + eps);
    const float* cr = cosb + (long)t * half + p0;
    const float* sr = sinb + (long)t * half + p0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float y1 = x1[e] * rstd * w1[e], y2 = x2[e] * rstd * w2[e];
      const float c = cr[e], s = sr[e];
      o1[e] = y1 * c - y2 * s;
      o2[e] = y2 * c + y1 * s;
    }
    *reinterpret_cast<uint4*>(base + p0) = pack8(o1);
    *reinterpret_cast<uint4*>(base + half + p0) = pack8(o2);
  }
}

// Workgroup g owns the rows [g rpw, min(N, (g + 1) rpw)) and writes row g of both partial matrices (zeros when it
// owns no row).  part_q / part_k: [G, D] fp32.
template <int D>
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(bf16_t* __restrict__ dqkv,
                                                             const bf16_t* __restrict__ raw,
                                                             const bf16_t* __restrict__ wq,
                                                             const bf16_t* __restrict__ wk,
                                                             const float* __restrict__ cosb,
                                                             const float* __restrict__ sinb,
                                                             float* __restrict__ part_q,
                                                             float* __restrict__ part_k, int N, int T, int Hq,
                                                             int heads, int stride, float eps, int rpw) {
  constexpr int half = D / 2, L = D / 16;
  __shared__ __attribute__((aligned(16))) float fold[4][2][D];
  const int r0 = blockIdx.x * rpw;
  const int r1 = min(N, r0 + rpw);
  const int per_row = heads * L;
  const int items = r1 > r0 ? (r1 - r0) * per_row : 0;
  const int p0 = (threadIdx.x % L) * 8;                   // fixed per thread: 256 % L == 0
  float aq1[8], aq2[8], ak1[8], ak2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) aq1[e] = aq2[e] = ak1[e] = ak2[e] = 0.f;
  for (int i = threadIdx.x; i < items; i += 256) {
    const int rr = i / per_row;
    const int h = (i - rr * per_row) / L;
    const long row = r0 + rr;
    const int t = (int)(row % T);
    DLTB_DCHECK(row < N && h < heads);
    bf16_t* base = dqkv + row * stride + (long)h * D;
    const bf16_t* rbase = raw + (row * heads + h) * (long)D;
    float d1[8], d2[8], x1[8], x2[8], w1[8], w2[8], o1[8], o2[8];
    unpack8(ld16<uint4>(base + p0), d1);
    unpack8(ld16<uint4>(base + half + p0), d2);
    unpack8(ld16<uint4>(rbase + p0), x1);
    unpack8(ld16<uint4>(rbase + half + p0), x2);
    const bool isq = h < Hq;
    const bf16_t* w = isq ? wq : wk;
    unpack8(ld16<uint4>(w + p0), w1);
    unpack8(ld16<uint4>(w + half + p0), w2);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += x1[e] * x1[e] + x2[e] * x2[e];
    const float rstd = rsqrtf(head_sum<L>(ss) * (1.f / D) + eps);   // the forward's expression
    const float* cr = cosb + (long)t * half + p0;
    const float* sr = sinb + (long)t * half + p0;
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float c = cr[e], s = sr[e];
      const float g1 = d1[e] * c + d2[e] * s;             // R(-theta) dy
      const float g2 = d2[e] * c - d1[e] * s;
      x1[e] *= rstd;                                      // xh
      x2[e] *= rstd;
      const float t1 = g1 * x1[e], t2 = g2 * x2[e];       // the weight-gradient terms
      if (isq) { aq1[e] += t1; aq2[e] += t2; } else { ak1[e] += t1; ak2[e] += t2; }
      o1[e] = g1 * w1[e];                                 // gw
      o2[e] = g2 * w2[e];
      dot += o1[e] * x1[e] + o2[e] * x2[e];
    }
    const float m = head_sum<L>(dot) * (1.f / D);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o1[e] = rstd * (o1[e] - x1[e] * m);
      o2[e] = rstd * (o2[e] - x2[e] * m);
    }
    *reinterpret_cast<uint4*>(base + p0) = pack8(o1);
    *reinterpret_cast<uint4*>(base + half + p0) = pack8(o2);
  }
  // fold the lanes of the wave that share p0 (lane % L), then the four waves through LDS; every lane takes part
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
#pragma unroll
    for (int o = L; o < 64; o <<= 1) {
      aq1[e] += __shfl_xor(aq1[e], o, 64);
      aq2[e] += __shfl_xor(aq2[e], o, 64);
      ak1[e] += __shfl_xor(ak1[e], o, 64);
      ak2[e] += __shfl_xor(ak2[e], o, 64);
    }
  }
  if (lane < L) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      fold[wid][0][p0 + e] = aq1[e];
      fold[wid][0][half + p0 + e] = aq2[e];
      fold[wid][1][p0 + e] = ak1[e];
      fold[wid][1][half + p0 + e] = ak2[e];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * D) {
    const int which = threadIdx.x / D, c = threadIdx.x - which * D;
    const float v = (fold[0][which][c] + fold[1][which][c]) + (fold[2][which][c] + fold[3][which][c]);
    (which ? part_k : part_q)[(size_t)blockIdx.x * D + c] = v;
  }
}

int fwd_grid(long items) {
  long g = (items + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

#ifndef DLTB_QKNORM_RPW
#define DLTB_QKNORM_RPW 8        // rows per workgroup of the backward at least
#endif
#ifndef DLTB_QKNORM_GMAX
#define DLTB_QKNORM_GMAX 1024    // workgroups (= partial rows) of the backward at most
#endif
// workgroups of the backward = rows of its partial matrices: a function of N only
int dltb_qknorm_partials(int N) {
  int G = (N + DLTB_QKNORM_RPW - 1) / DLTB_QKNORM_RPW;
  if (G < 1) G = 1;
  if (G > DLTB_QKNORM_GMAX) G = DLTB_QKNORM_GMAX;
  return G;
}

void dltb_qknorm_rope_fwd(void* qkv, void* raw, const void* wq, const void* wk, const float* cosb,
                          const float* sinb, int N, int T, int Hq, int Hkv, int D, int stride, float eps,
                          hipStream_t st) {
  const int heads = Hq + Hkv;
  const long items = (long)N * heads * (D / 16);
  if (D == 64)
    hipLaunchKernelGGL(qknorm_rope_fwd_kernel<64>, dim3(fwd_grid(items)), dim3(256), 0, st, (bf16_t*)qkv,
                       (bf16_t*)raw, (const bf16_t*)wq, (const bf16_t*)wk, cosb, sinb, N, T, Hq, heads, stride, eps);
  else
    hipLaunchKernelGGL(qknorm_rope_fwd_kernel<128>, dim3(fwd_grid(items)), dim3(256), 0, st, (bf16_t*)qkv,
                       (bf16_t*)raw, (const bf16_t*)wq, (const bf16_t*)wk, cosb, sinb, N, T, Hq, heads, stride, eps);
}

void dltb_qknorm_rope_bwd(void* dqkv, const void* raw, const void* wq, const void* wk, const float* cosb,
                          const float* sinb, float* part_q, float* part_k, int N, int T, int Hq, int Hkv, int D,
                          int stride, float eps, hipStream_t st) {
  const int heads = Hq + Hkv;
  const int G = dltb_qknorm_partials(N);
  const int rpw = (N + G - 1) / G;
  if (D == 64)
    hipLaunchKernelGGL(qknorm_rope_bwd_kernel<64>, dim3(G), dim3(256), 0, st, (bf16_t*)dqkv, (const bf16_t*)raw,
                       (const bf16_t*)wq, (const bf16_t*)wk, cosb, sinb, part_q, part_k, N, T, Hq, heads, stride,
                       eps, rpw);
  else
    hipLaunchKernelGGL(qknorm_rope_bwd_kernel<128>, dim3(G), dim3(256), 0, st, (bf16_t*)dqkv, (const bf16_t*)raw,
                       (const bf16_t*)wq, (const bf16_t*)wk, cosb, sinb, part_q, part_k, N, T, Hq, heads, stride,
                       eps, rpw);
}
