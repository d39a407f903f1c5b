// Shared by the LDS-DMA MFMA GEMMs (gemm.hip: NT / TN, gemm_nn.hip: NN): the kernel argument block
// and the split-K reduction.
#pragma once
#include "common.h"

namespace {

constexpr int kBK = 64;

struct GemmArgs {
  const bf16_t* a;
  const bf16_t* b;
  bf16_t* c;
  const bf16_t* bias;
  const float* alpha;   // optional device scalar multiplying A B (before bias / accumulate)
  float* part;          // split-K partials [splits][M][N] (fp32), null without split-K
  long lda, ldb, ldc;
  int M, N, K;
  int accumulate;
  int ksplit;           // K range per split (multiple of kBK)
  int pf;               // L2 prefetch distance in k-steps (PF kernels)
  int gm;               // tile order: groups of gm row-blocks (each XCD's run covers gm x (run / gm) tiles)
};

// split-K reduction: C = sum_s part[s] (+ bias) (+ C)
__global__ __launch_bounds__(256) void gemm_splitk_reduce(GemmArgs g, int splits) {
  const long total4 = (long)g.M * g.N / 4;
  const float al = g.alpha ? *g.alpha : 1.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const long e = i * 4;
    const int m = (int)(e / g.N), n = (int)(e % g.N);
    float4 s = *reinterpret_cast<const float4*>(g.part + e);
    for (int k = 1; k < splits; ++k) {
      const float4 t = *reinterpret_cast<const float4*>(g.part + (size_t)k * g.M * g.N + e);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    float v[4] = {s.x * al, s.y * al, s.z * al, s.w * al};
    if (g.bias) {
      const uint2 bb = *reinterpret_cast<const uint2*>(g.bias + n);
      v[0] += lo_bf(bb.x); v[1] += hi_bf(bb.x); v[2] += lo_bf(bb.y); v[3] += hi_bf(bb.y);
    }
    bf16_t* cp = g.c + (size_t)m * g.ldc + n;
    if (g.accumulate) {
      const uint2 old = *reinterpret_cast<const uint2*>(cp);
      v[0] += lo_bf(old.x); v[1] += hi_bf(old.x); v[2] += lo_bf(old.y); v[3] += hi_bf(old.y);
    }
    uint2 o;
    o.x = pack_bf2(v[0], v[1]);
    o.y = pack_bf2(v[2], v[3]);
    *reinterpret_cast<uint2*>(cp) = o;
  }
}

// K range per split in elements (whole k-steps, rounded up) and the split count that range gives:
// 500 k-steps over 3 requested splits -> 167 per split, 3 splits, the last one 166 steps.
inline int gemm_ksplit(int K, int& splits) {
  if (splits < 1) splits = 1;
  const int kchunks = K / kBK;
  if (splits > kchunks) splits = kchunks;
  const int ksplit = ((kchunks + splits - 1) / splits) * kBK;
  splits = (K + ksplit - 1) / ksplit;
  return ksplit;
}

}  // namespace
