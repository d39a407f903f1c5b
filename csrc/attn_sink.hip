// Gradient of the learned attention sinks for gfx950 (the forward side is the SINK epilogue of csrc/attention.hip).
//
// A sink is one raw logit s_h per query head that joins the softmax denominator and carries no value:
//   lse[b, h, t] = log(sum_j exp(z_j) + exp(s_h)),   p_sink = exp(s_h - lse),   d s_h = p_sink (0 - delta)
// so with delta = rowsum(dO * O), which the dQ pass writes,
//   ds_h = - sum over (b, t) of exp(s_h - lse[b, h, t]) * delta[b, h, t].
//
// attn_sink_bwd: lse, delta fp32 [B, Hq, Tq] -> fp32 partials [G, Hq], G = dltb_attn_sink_partials(B, Tq).
// Workgroup (g, hg) owns the flat (b, t) rows [g rpw, min(B Tq, (g + 1) rpw)) and the heads 4 hg .. 4 hg + 3, one
// head per wave: a lane sums its rows (row0 + lane, + 64, ...) in order, the wave folds by the xor butterfly, and
// lane 0 stores part[g][h].  Every element of the G rows is written (zero for a workgroup without rows), there are no
// atomics and the summation order depends on (B, Tq) only.  colreduce_multi sums the G rows into the gradient slot.
#include "common.h"
#include "launchers.h"

namespace {

__global__ __launch_bounds__(256) void attn_sink_bwd_kernel(const float* __restrict__ lse,
                                                           const float* __restrict__ delta,
                                                           const bf16_t* __restrict__ sink, float* __restrict__ part,
                                                           int B, int Hq, int Tq, int rpw) {
  const int lane = threadIdx.x & 63, h = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (h >= Hq) return;                    // whole waves leave; no barrier below
  const long R = (long)B * Tq;
  const long r0 = (long)blockIdx.x * rpw;
  const long r1 = r0 + rpw < R ? r0 + rpw : R;
  const float s = bf2f(sink[h]);
  float acc = 0.f;
  for (long i = r0 + lane; i < r1; i += 64) {
    const long b = i / Tq, t = i - b * Tq;
    const long idx = (b * Hq + h) * Tq + t;
    DLTB_DCHECK(b < B && idx < (long)B * Hq * Tq);
    acc += expf(s - lse[idx]) * delta[idx];
  }
  acc = wave_sum(acc);
  if (lane == 0) part[(size_t)blockIdx.x * Hq + h] = 0.f - acc;
}

}  // namespace

#ifndef DLTB_SINK_RPW
#define DLTB_SINK_RPW 256        // (b, t) rows per workgroup at least
#endif
#ifndef DLTB_SINK_GMAX
#define DLTB_SINK_GMAX 256       // workgroups along the rows (= partial rows) at most
#endif
// rows of the partial matrix: a function of (B, Tq) only
int dltb_attn_sink_partials(int B, int Tq) {
  long G = ((long)B * Tq + DLTB_SINK_RPW - 1) / DLTB_SINK_RPW;
  if (G < 1) G = 1;
  if (G > DLTB_SINK_GMAX) G = DLTB_SINK_GMAX;
  return (int)G;
}

void dltb_attn_sink_bwd(const float* lse, const float* delta, const void* sink, float* part, int B, int Hq, int Tq,
                        hipStream_t st) {
  const int G = dltb_attn_sink_partials(B, Tq);
  const long R = (long)B * Tq;
  const int rpw = (int)((R + G - 1) / G);
  hipLaunchKernelGGL(attn_sink_bwd_kernel, dim3(G, cdiv(Hq, 4)), dim3(256), 0, st, lse, delta,
                     (const bf16_t*)sink, part, B, Hq, Tq, rpw);
}
