// Fused AdamW over flat fp32 optimizer shards + gradient-norm helpers for gfx950.
//
// Replaces torch.optim.AdamW(foreach) (train_harness.py:329) and DeepSpeed's FusedAdam
// multi_tensor_adam for the ZeRO paths.  All optimizer state lives in ONE flat fp32 "owner"
// space per rank (the whole model for DDP, this rank's partition for ZeRO/FSDP), so a single
// launch updates master weights, exp_avg and exp_avg_sq in one HBM pass and writes the bf16
// compute copy of every parameter straight into its (possibly non-contiguous) destination:
//
//   segments: owner range [ostart, ostart + len) -> bf16 destination pointer
//   blocks  : host-built table (segment id, owner start) so no block straddles a segment.
//
// Math is torch.optim.AdamW's:  p *= 1 - lr*wd;  m = lerp(m, g, 1-b1);  v = b2 v + (1-b2) g^2;
//                                p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
// with g optionally multiplied by a device-side scale (gradient clipping coefficient / 1/accum),
// read from memory so no host sync is needed.
#include <cstdlib>

#include "common.h"

namespace {

constexpr int kAdamThreads = 256;
constexpr int kAdamChunk = kAdamThreads * 16;   // elements per block (host block tables)

typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

template <typename G>
DLTB_DEV void load4(const G* p, float* g);
template <>
DLTB_DEV void load4<float>(const float* p, float* g) {
  float4 v = *reinterpret_cast<const float4*>(p);
  g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
}
template <>
DLTB_DEV void load4<bf16_t>(const bf16_t* p, float* g) {
  uint2 v = *reinterpret_cast<const uint2*>(p);
  g[0] = lo_bf(v.x); g[1] = hi_bf(v.x); g[2] = lo_bf(v.y); g[3] = hi_bf(v.y);
}
// 8 gradient elements: one 16-byte load for 16-bit gradients, two for fp32
template <typename G>
DLTB_DEV void load8(const G* p, float* g);
template <>
DLTB_DEV void load8<float>(const float* p, float* g) {
  const v4f a = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
  const v4f b = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p + 4));
  g[0] = a[0]; g[1] = a[1]; g[2] = a[2]; g[3] = a[3]; g[4] = b[0]; g[5] = b[1]; g[6] = b[2]; g[7] = b[3];
}
template <>
DLTB_DEV void load8<bf16_t>(const bf16_t* p, float* g) {
  const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
  g[0] = lo_bf(v[0]); g[1] = hi_bf(v[0]); g[2] = lo_bf(v[1]); g[3] = hi_bf(v[1]);
  g[4] = lo_bf(v[2]); g[5] = hi_bf(v[2]); g[6] = lo_bf(v[3]); g[7] = hi_bf(v[3]);
}

struct AdamHp {
  float lr, beta1, beta2, eps, wd, step_size, inv_sqrt_bc2, gs;
};

DLTB_DEV void adam_elem(float& p, float& m, float& v, float g, const AdamHp& h) {
  const float gg = g * h.gs;
  p *= 1.f - h.lr * h.wd;
  m = m + (1.f - h.beta1) * (gg - m);
  v = h.beta2 * v + (1.f - h.beta2) * gg * gg;
  const float denom = sqrtf(v) * h.inv_sqrt_bc2 + h.eps;
  p -= h.step_size * m / denom;
}

// W elements per lane and vector access (8: every stream moved in 16-byte accesses -- master /
// moments as two float4, a 16-bit gradient and the 16-bit parameter copy as one 16-byte access;
// 4: the 8-byte 16-bit accesses of segments not 8-element aligned).  ITERS vectors per lane, all
// loads issued before the first update (ITERS * (6 + 1) 16-byte loads in flight per lane at W = 8).
template <typename G, int W, int T = kAdamThreads>
DLTB_DEV void adamw_block(float* __restrict__ master, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                          const G* __restrict__ grad, bf16_t* __restrict__ dst, int64_t start, int64_t seg_end,
                          int64_t dst_base, const AdamHp& h) {
  constexpr int ITERS = kAdamChunk / (T * W);
  constexpr int NV = W / 4;
  v4f P[ITERS][NV], M[ITERS][NV], V[ITERS][NV];
  float Gr[ITERS][W];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int64_t i = start + ((int64_t)it * T + threadIdx.x) * W;
    if (i < seg_end) {
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        P[it][q] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(master + i + 4 * q));
        M[it][q] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(exp_avg + i + 4 * q));
        V[it][q] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(exp_avg_sq + i + 4 * q));
      }
      if constexpr (W == 8) load8<G>(grad + i, Gr[it]);
      else load4<G>(grad + i, Gr[it]);
    }
  }
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int64_t off = ((int64_t)it * T + threadIdx.x) * W;
    const int64_t i = start + off;
    if (i >= seg_end) break;
    float p[W], m[W], v[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      p[e] = P[it][e >> 2][e & 3];
      m[e] = M[it][e >> 2][e & 3];
      v[e] = V[it][e >> 2][e & 3];
      adam_elem(p[e], m[e], v[e], Gr[it][e], h);
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      __builtin_nontemporal_store((v4f){p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]},
                                  reinterpret_cast<v4f*>(master + i + 4 * q));
      __builtin_nontemporal_store((v4f){m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]},
                                  reinterpret_cast<v4f*>(exp_avg + i + 4 * q));
      __builtin_nontemporal_store((v4f){v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]},
                                  reinterpret_cast<v4f*>(exp_avg_sq + i + 4 * q));
    }
    if constexpr (W == 8) {
      v4u o = {pack_bf2(p[0], p[1]), pack_bf2(p[2], p[3]), pack_bf2(p[4], p[5]), pack_bf2(p[6], p[7])};
      *reinterpret_cast<v4u*>(dst + dst_base + off) = o;
    } else {
      uint2 o;
      o.x = pack_bf2(p[0], p[1]);
      o.y = pack_bf2(p[2], p[3]);
      *reinterpret_cast<uint2*>(dst + dst_base + off) = o;
    }
  }
}

template <typename G>
__global__ __launch_bounds__(kAdamThreads) void adamw_kernel(
    float* __restrict__ master, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
    const G* __restrict__ grad, const int* __restrict__ blk_seg, const int64_t* __restrict__ blk_start,
    const int64_t* __restrict__ seg_ostart, const int64_t* __restrict__ seg_len,
    const int64_t* __restrict__ seg_dst, const float* __restrict__ gscale, const float* __restrict__ hp,
    float lr, float beta1, float beta2, float eps, float wd, float step_size, float inv_sqrt_bc2, int nblk) {
  if (hp) {   // step-dependent hyper-parameters from device memory (HIP-graph replays)
    if (hp[3] != 0.f) return;   // dynamic loss scaling found an inf / nan: the step is skipped
    lr = hp[0];
    step_size = hp[1];
    inv_sqrt_bc2 = hp[2];
  }
  // one table row per block, or (a grid capped below the row count: an update trickled beside other
  // kernels) a block-strided walk over the rows
  for (int bi = blockIdx.x; bi < nblk; bi += gridDim.x) {
  const int seg = blk_seg[bi];
  const int64_t start = blk_start[bi];
  const int64_t s0 = seg_ostart[seg];
  const int64_t seg_end = s0 + seg_len[seg];
  DLTB_DCHECK(seg >= 0 && start >= s0 && start < seg_end);
  bf16_t* dst = reinterpret_cast<bf16_t*>(seg_dst[seg]);
  const int64_t dst_base = start - s0;
  const AdamHp h{lr, beta1, beta2, eps, wd, step_size, inv_sqrt_bc2, gscale ? *gscale : 1.f};
  // every state element is touched once per step: streamed past the caches (nontemporal loads and
  // stores).  W = 4: every fp32 access one coalesced 16-byte vector per lane, the 16-bit streams 8 bytes
  // per lane (a W = 8 path -- two adjacent float4 per lane -- measured 4.22 TB/s against 5.52 on the
  // TinyGPT-A state, and 128-thread blocks no faster: profiles/adamw_r5.txt; both removed in round 6).
  adamw_block<G, 4>(master, exp_avg, exp_avg_sq, grad, dst, start, seg_end, dst_base, h);
  }
}

// ------------------------------------------------------------------ block-scaled FP8 moments
// exp_avg and sqrt(exp_avg_sq) as OCP E4M3 codes (one byte each) with one fp32 power-of-two scale per 256
// consecutive elements of a table row: with the W = 4 layout a quantisation block is one wavefront in one
// iteration, so its absmax is a wave reduction.  The contract (scale rule, stochastic rounding on the fp32 bit
// pattern, the floor of the second moment) is mirrored bit for bit by ops/ref.py (fp8_quantize / adamw_flat_fp8).
constexpr int kFp8Block = 256;
constexpr int kFp8RowBlocks = kAdamChunk / kFp8Block;
constexpr float kFp8MinNormal = 0.015625f;       // 2^-6: below it E4M3 is a fixed-point grid of 2^-9
constexpr float kFp8MinSub = 0.001953125f;       // 2^-9

// exponent e of the block scale 2^e: 0 for an all-zero block, else the smallest e >= -126 with a * 2^-e <= 448
// (448 = 1.75 * 2^8: a mantissa above 1.75 needs one more)
DLTB_DEV int fp8_scale_exp(float a) {
  const int e = (int)((__float_as_uint(a) + 0x1FFFFFu) >> 23) - 135;
  return a == 0.f ? 0 : (e < -126 ? -126 : e);
}
DLTB_DEV float fp8_pow2(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }

// per-launch keys of the two moments (kind 0: exp_avg, 1: sqrt(exp_avg_sq)) and the word of one element
DLTB_DEV uint32_t fp8_key(uint64_t seed, uint32_t counter, uint32_t kind) {
  return fmix32(fmix32(counter * DLTB_C_ROW + (uint32_t)(seed >> 32)) ^ ((uint32_t)seed + (kind + 1u) * DLTB_C_COL));
}
DLTB_DEV uint32_t fp8_rand20(uint32_t key, int64_t idx) {
  const uint32_t x = (uint32_t)idx * DLTB_C_COL + (uint32_t)((uint64_t)idx >> 32) * DLTB_C_ROW;
  return fmix32(key ^ x) >> 12;
}

// y * inv rounded to one of its two E4M3 neighbours: the random word r20 (20 bits; 0x80000 rounds to nearest)
// is added to the fp32 bit pattern and the low 20 mantissa bits are cleared, which leaves E4M3's 3.  Below 2^-6
// the value is first moved into the binade [2^-6, 2^-5), whose 3-bit grid is the subnormal grid 2^-9.  The
// result is exactly representable, so the conversion instruction does not round again.  floor_pos: a positive y
// never becomes 0 (second moment).
DLTB_DEV float fp8_round(float y, float inv, uint32_t r20, bool floor_pos) {
#pragma clang fp contract(off)
  const float t = fabsf(y) * inv;
  const bool sub = t < kFp8MinNormal;
  const float w = sub ? t + kFp8MinNormal : t;
  float q = __uint_as_float((__float_as_uint(w) + r20) & 0xFFF00000u);
  if (sub) q -= kFp8MinNormal;
  if (floor_pos && y > 0.f && q == 0.f) q = kFp8MinSub;
  return q == 0.f ? 0.f : copysignf(q, y);
}
DLTB_DEV uint32_t fp8_pack4(const float* q) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], w, true);
  return (uint32_t)w;
}
DLTB_DEV void fp8_unpack4(uint32_t w, float scale, float* f) {
  f[0] = __builtin_amdgcn_cvt_f32_fp8((int)w, 0) * scale;
  f[1] = __builtin_amdgcn_cvt_f32_fp8((int)w, 1) * scale;
  f[2] = __builtin_amdgcn_cvt_f32_fp8((int)w, 2) * scale;
  f[3] = __builtin_amdgcn_cvt_f32_fp8((int)w, 3) * scale;
}
// this lane's four values y (owner indices idx .. idx + 3; zeros in a lane past the end) of a block that is the
// whole wave -> four codes and (every lane) the block's scale
DLTB_DEV uint32_t fp8_quant_wave(const float* y, int64_t idx, uint32_t key, bool nearest, bool floor_pos,
                                 float* scale_out) {
  const float a = wave_max(fmaxf(fmaxf(fabsf(y[0]), fabsf(y[1])), fmaxf(fabsf(y[2]), fabsf(y[3]))));
  const int e = fp8_scale_exp(a);
  const float inv = fp8_pow2(-e);
  float q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    q[k] = fp8_round(y[k], inv, nearest ? 0x80000u : fp8_rand20(key, idx + k), floor_pos);
  *scale_out = fp8_pow2(e);
  return fp8_pack4(q);
}

template <typename G, int T = kAdamThreads>
DLTB_DEV void adamw_fp8_block(float* __restrict__ master, uint32_t* __restrict__ mq, uint32_t* __restrict__ sq,
                              float* __restrict__ mscale, float* __restrict__ sscale,
                              const G* __restrict__ grad, bf16_t* __restrict__ dst, int64_t start, int64_t seg_end,
                              int64_t dst_base, const AdamHp& h, uint32_t key_m, uint32_t key_s) {
  constexpr int W = 4;
  constexpr int ITERS = kAdamChunk / (T * W);
  static_assert(T / 64 * ITERS == kFp8RowBlocks && 64 * W == kFp8Block, "one wave and iteration per block");
  const int wave = threadIdx.x >> 6;
  v4f P[ITERS];
  uint32_t MC[ITERS], SC[ITERS];
  float MS[ITERS], SS[ITERS];
  float Gr[ITERS][W];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int64_t i = start + ((int64_t)it * T + threadIdx.x) * W;
    if (i < seg_end) {
      P[it] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(master + i));
      MC[it] = __builtin_nontemporal_load(mq + (i >> 2));
      SC[it] = __builtin_nontemporal_load(sq + (i >> 2));
      MS[it] = mscale[it * (T / 64) + wave];
      SS[it] = sscale[it * (T / 64) + wave];
      load4<G>(grad + i, Gr[it]);
    }
  }
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int64_t off = ((int64_t)it * T + threadIdx.x) * W;
    const int64_t i = start + off;
    // the block (this wave, this iteration) lies past the segment: so do the later ones (wave-uniform)
    if (start + ((int64_t)it * T + wave * 64) * W >= seg_end) break;
    const bool live = i < seg_end;
    float p[W] = {0.f, 0.f, 0.f, 0.f}, m[W] = {0.f, 0.f, 0.f, 0.f}, s[W] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      float d[W];
      fp8_unpack4(MC[it], MS[it], m);
      fp8_unpack4(SC[it], SS[it], d);
#pragma unroll
      for (int e = 0; e < W; ++e) {
        p[e] = P[it][e];
        float v = d[e] * d[e];
        adam_elem(p[e], m[e], v, Gr[it][e], h);
        s[e] = sqrtf(v);
      }
    }
    float ms, ss;
    const uint32_t mc = fp8_quant_wave(m, i, key_m, false, false, &ms);
    const uint32_t sc = fp8_quant_wave(s, i, key_s, false, true, &ss);
    if (live) {
      __builtin_nontemporal_store((v4f){p[0], p[1], p[2], p[3]}, reinterpret_cast<v4f*>(master + i));
      __builtin_nontemporal_store(mc, mq + (i >> 2));
      __builtin_nontemporal_store(sc, sq + (i >> 2));
      uint2 o;
      o.x = pack_bf2(p[0], p[1]);
      o.y = pack_bf2(p[2], p[3]);
      *reinterpret_cast<uint2*>(dst + dst_base + off) = o;
      if ((threadIdx.x & 63) == 0) {       // the block's first lane is live whenever the block is
        mscale[it * (T / 64) + wave] = ms;
        sscale[it * (T / 64) + wave] = ss;
      }
    }
  }
}

// adamw_kernel with one-byte moments: the same tables and W = 4 streaming layout; row_off is the global table
// row of blk_seg[0] (a launch over a slice of the tables addresses the scales of the global row).  hp[4] holds
// the launch counter as integer bits.
template <typename G>
__global__ __launch_bounds__(kAdamThreads) void adamw_fp8_kernel(
    float* __restrict__ master, uint32_t* __restrict__ mq, uint32_t* __restrict__ sq,
    float* __restrict__ mscale, float* __restrict__ sscale,
    const G* __restrict__ grad, const int* __restrict__ blk_seg, const int64_t* __restrict__ blk_start,
    const int64_t* __restrict__ seg_ostart, const int64_t* __restrict__ seg_len,
    const int64_t* __restrict__ seg_dst, const float* __restrict__ gscale, const float* __restrict__ hp,
    float lr, float beta1, float beta2, float eps, float wd, float step_size, float inv_sqrt_bc2, int nblk,
    int64_t row_off, uint64_t seed, uint32_t counter) {
  if (hp) {
    if (hp[3] != 0.f) return;   // skipped step: codes, scales and master stay
    lr = hp[0];
    step_size = hp[1];
    inv_sqrt_bc2 = hp[2];
    counter = __float_as_uint(hp[4]);
  }
  const uint32_t key_m = fp8_key(seed, counter, 0u), key_s = fp8_key(seed, counter, 1u);
  for (int bi = blockIdx.x; bi < nblk; bi += gridDim.x) {
    const int seg = blk_seg[bi];
    const int64_t start = blk_start[bi];
    const int64_t s0 = seg_ostart[seg];
    const int64_t seg_end = s0 + seg_len[seg];
    DLTB_DCHECK(seg >= 0 && start >= s0 && start < seg_end);
    bf16_t* dst = reinterpret_cast<bf16_t*>(seg_dst[seg]);
    const AdamHp h{lr, beta1, beta2, eps, wd, step_size, inv_sqrt_bc2, gscale ? *gscale : 1.f};
    const int64_t row = row_off + bi;
    adamw_fp8_block<G>(master, mq, sq, mscale + row * kFp8RowBlocks, sscale + row * kFp8RowBlocks, grad, dst,
                       start, seg_end, start - s0, h, key_m, key_s);
  }
}

// the quantiser and the decoder alone, on a flat tensor whose blocks start at its first element (one segment's
// rows): element j belongs to scale j / 256 and has the owner index owner_off + j
__global__ __launch_bounds__(kAdamThreads) void fp8_quant_kernel(
    const float* __restrict__ x, uint32_t* __restrict__ codes, float* __restrict__ scales, int64_t n,
    int64_t nblocks, int kind, bool nearest, uint64_t seed, uint32_t counter, int64_t owner_off) {
  const uint32_t key = fp8_key(seed, counter, (uint32_t)kind);
  const int lane = threadIdx.x & 63;
  for (int64_t b = (int64_t)blockIdx.x * (kAdamThreads / 64) + (threadIdx.x >> 6); b < nblocks;
       b += (int64_t)gridDim.x * (kAdamThreads / 64)) {
    const int64_t j = b * kFp8Block + lane * 4;
    float y[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < n) load4<float>(x + j, y);
    float sc;
    const uint32_t c = fp8_quant_wave(y, owner_off + j, key, nearest, kind == 1, &sc);
    if (j < n) codes[j >> 2] = c;
    if (lane == 0) scales[b] = sc;
  }
}

__global__ __launch_bounds__(kAdamThreads) void fp8_dequant_kernel(
    const uint32_t* __restrict__ codes, const float* __restrict__ scales, float* __restrict__ out, int64_t n4) {
  for (int64_t j = (int64_t)blockIdx.x * kAdamThreads + threadIdx.x; j < n4; j += (int64_t)gridDim.x * kAdamThreads) {
    float f[4];
    fp8_unpack4(codes[j], scales[j / (kFp8Block / 4)], f);
    *reinterpret_cast<float4*>(out + 4 * j) = make_float4(f[0], f[1], f[2], f[3]);
  }
}

// sum of squares in a FIXED order (bitwise reproducible: eager runs, graph replays and ranks agree):
// a grid-stride pass writes one partial per block, a one-block pass adds them in index order.
constexpr int kSumsqBlocks = 1024;

template <typename G>
__global__ __launch_bounds__(256) void sumsq_kernel(const G* __restrict__ x, long n4,
                                                   float* __restrict__ part) {
  __shared__ float red[4];
  // four grid-strided loads issued before any is consumed (four independent accumulators): the
  // pass is HBM-latency bound with one 8-byte load in flight per lane
  const long stride = (long)gridDim.x * blockDim.x;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (; i + 3 * stride < n4; i += 4 * stride) {
    float g[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) load4<G>(x + (i + u * stride) * 4, g[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] += g[u][0] * g[u][0] + g[u][1] * g[u][1] + g[u][2] * g[u][2] + g[u][3] * g[u][3];
  }
  for (; i < n4; i += stride) {
    float g[4];
    load4<G>(x + i * 4, g);
    a[0] += g[0] * g[0] + g[1] * g[1] + g[2] * g[2] + g[3] * g[3];
  }
  float acc = (a[0] + a[1]) + (a[2] + a[3]);
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* __restrict__ part, int n,
                                                         float* __restrict__ out) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) out[0] += acc;
}

// norm_sq[0] (already all-reduced) -> coef = min(1, max_norm / (sqrt(norm_sq) + 1e-6)), norm
__global__ void clip_coef_kernel(const float* __restrict__ norm_sq, float max_norm,
                                 float* __restrict__ coef, float* __restrict__ norm_out,
                                 float extra_scale) {
  const float nrm = sqrtf(norm_sq[0]) * extra_scale;
  float c = max_norm > 0.f ? max_norm / (nrm + 1e-6f) : 1.f;
  c = fminf(c, 1.f);
  coef[0] = c * extra_scale;
  if (norm_out) norm_out[0] = nrm;
}

// Dynamic loss scaling with torch.amp.GradScaler's semantics (train_harness.py:334-335, 371-376),
// decided on the device so no step ever waits on the host:
//   state = [scale S, growth tracker, optimizer steps taken, steps skipped]
//   norm_sq = sum of squares of the S-scaled gradients (all-reduced where sharded); an inf or nan
//   gradient makes it non-finite (fp16 gradients cannot overflow the fp32 sum: 65504^2 * 2^28).
// found inf -> hp[3] = 1 (the AdamW kernel returns at once: master, moments and step count stay),
//              S *= backoff, tracker = 0;
// otherwise -> coef = extra * clip(unscaled norm) / S, hp[1..2] = bias corrections of the device
//              step count, tracker += 1, S *= growth when it reaches growth_interval.
// hp[0] (lr) is the host's upload (FlatAdamW.prepare) and is left alone.
__global__ void amp_step_kernel(const float* __restrict__ norm_sq, float* __restrict__ state,
                                float* __restrict__ coef, float* __restrict__ norm_out,
                                float* __restrict__ hp, float max_norm, float extra_scale, float beta1,
                                float beta2, float growth, float backoff, float growth_interval) {
  const float S = state[0];
  const float nsq = norm_sq[0];
  if (!isfinite(nsq)) {
    state[0] = S * backoff;
    state[1] = 0.f;
    state[3] += 1.f;
    hp[3] = 1.f;
    coef[0] = 0.f;
    if (norm_out) norm_out[0] = nsq;
    return;
  }
  const float inv = 1.f / S;
  const float nrm = sqrtf(nsq) * inv * extra_scale;
  const float c = max_norm > 0.f ? fminf(1.f, max_norm / (nrm + 1e-6f)) : 1.f;
  coef[0] = c * extra_scale * inv;
  if (norm_out) norm_out[0] = nrm;
  const float t = state[2] + 1.f;
  state[2] = t;
  hp[1] = hp[0] / (1.f - powf(beta1, t));
  hp[2] = 1.f / sqrtf(1.f - powf(beta2, t));
  hp[3] = 0.f;
  float tr = state[1] + 1.f;
  if (tr >= growth_interval) {
    state[0] = S * growth;
    tr = 0.f;
  }
  state[1] = tr;
}

__global__ __launch_bounds__(256) void fill_f32_kernel(float* __restrict__ x, long n, float v) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    x[i] = v;
}

}  // namespace

int dltb_adamw_chunk() { return kAdamChunk; }

void dltb_adamw(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, bool grad_bf16,
                const int* blk_seg, const int64_t* blk_start, int nblocks, const int64_t* seg_ostart,
                const int64_t* seg_len, const int64_t* seg_dst, const float* gscale, const float* hp,
                float lr, float beta1, float beta2, float eps, float wd, float step_size,
                float inv_sqrt_bc2, int grid_cap, hipStream_t st) {
  if (nblocks <= 0) return;
  const int grid = grid_cap > 0 && grid_cap < nblocks ? grid_cap : nblocks;
  const int thr = kAdamThreads;
  if (grad_bf16)
    hipLaunchKernelGGL(adamw_kernel<bf16_t>, dim3(grid), dim3(thr), 0, st, master,
                       exp_avg, exp_avg_sq, (const bf16_t*)grad, blk_seg, blk_start, seg_ostart,
                       seg_len, seg_dst, gscale, hp, lr, beta1, beta2, eps, wd, step_size, inv_sqrt_bc2, nblocks);
  else
    hipLaunchKernelGGL(adamw_kernel<float>, dim3(grid), dim3(thr), 0, st, master,
                       exp_avg, exp_avg_sq, (const float*)grad, blk_seg, blk_start, seg_ostart,
                       seg_len, seg_dst, gscale, hp, lr, beta1, beta2, eps, wd, step_size, inv_sqrt_bc2, nblocks);
}

void dltb_adamw_fp8(float* master, uint8_t* mq, uint8_t* sq, float* mscale, float* sscale, const void* grad,
                    bool grad_bf16, const int* blk_seg, const int64_t* blk_start, int nblocks,
                    const int64_t* seg_ostart, const int64_t* seg_len, const int64_t* seg_dst,
                    const float* gscale, const float* hp, float lr, float beta1, float beta2, float eps, float wd,
                    float step_size, float inv_sqrt_bc2, int grid_cap, int64_t row_off, uint64_t seed,
                    uint32_t counter, hipStream_t st) {
  if (nblocks <= 0) return;
  const int grid = grid_cap > 0 && grid_cap < nblocks ? grid_cap : nblocks;
  const int thr = kAdamThreads;
  uint32_t* mq4 = reinterpret_cast<uint32_t*>(mq);
  uint32_t* sq4 = reinterpret_cast<uint32_t*>(sq);
  if (grad_bf16)
    hipLaunchKernelGGL(adamw_fp8_kernel<bf16_t>, dim3(grid), dim3(thr), 0, st, master, mq4, sq4, mscale, sscale,
                       (const bf16_t*)grad, blk_seg, blk_start, seg_ostart, seg_len, seg_dst, gscale, hp, lr,
                       beta1, beta2, eps, wd, step_size, inv_sqrt_bc2, nblocks, row_off, seed, counter);
  else
    hipLaunchKernelGGL(adamw_fp8_kernel<float>, dim3(grid), dim3(thr), 0, st, master, mq4, sq4, mscale, sscale,
                       (const float*)grad, blk_seg, blk_start, seg_ostart, seg_len, seg_dst, gscale, hp, lr,
                       beta1, beta2, eps, wd, step_size, inv_sqrt_bc2, nblocks, row_off, seed, counter);
}

void dltb_fp8_quant(const float* x, uint8_t* codes, float* scales, int64_t n, int kind, bool nearest,
                    uint64_t seed, uint32_t counter, int64_t owner_off, hipStream_t st) {
  if (n <= 0) return;
  const int64_t nblocks = (n + kFp8Block - 1) / kFp8Block;
  int64_t g = (nblocks + kAdamThreads / 64 - 1) / (kAdamThreads / 64);
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(fp8_quant_kernel, dim3((int)g), dim3(kAdamThreads), 0, st, x,
                     reinterpret_cast<uint32_t*>(codes), scales, n, nblocks, kind, nearest, seed, counter, owner_off);
}

void dltb_fp8_dequant(const uint8_t* codes, const float* scales, float* out, int64_t n, hipStream_t st) {
  if (n <= 0) return;
  const int64_t n4 = n / 4;
  int64_t g = (n4 + kAdamThreads - 1) / kAdamThreads;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(fp8_dequant_kernel, dim3((int)g), dim3(kAdamThreads), 0, st,
                     reinterpret_cast<const uint32_t*>(codes), scales, out, n4);
}

int dltb_sumsq_partials() { return kSumsqBlocks; }

void dltb_sumsq(const void* x, bool bf16, long n, float* out, float* part, hipStream_t st) {
  const long n4 = n / 4;
  long g = (n4 + 255) / 256;
  if (g > kSumsqBlocks) g = kSumsqBlocks;
  if (g < 1) g = 1;
  if (bf16)
    hipLaunchKernelGGL(sumsq_kernel<bf16_t>, dim3(g), dim3(256), 0, st, (const bf16_t*)x, n4, part);
  else
    hipLaunchKernelGGL(sumsq_kernel<float>, dim3(g), dim3(256), 0, st, (const float*)x, n4, part);
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, st, part, (int)g, out);
}

void dltb_clip_coef(const float* norm_sq, float max_norm, float* coef, float* norm_out,
                    float extra_scale, hipStream_t st) {
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, st, norm_sq, max_norm, coef, norm_out,
                     extra_scale);
}

void dltb_amp_step(const float* norm_sq, float* state, float* coef, float* norm_out, float* hp,
                   float max_norm, float extra_scale, float beta1, float beta2, float growth,
                   float backoff, int growth_interval, hipStream_t st) {
  hipLaunchKernelGGL(amp_step_kernel, dim3(1), dim3(1), 0, st, norm_sq, state, coef, norm_out, hp,
                     max_norm, extra_scale, beta1, beta2, growth, backoff, (float)growth_interval);
}

void dltb_fill_f32(float* x, long n, float v, hipStream_t st) {
  long g = (n + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(fill_f32_kernel, dim3(g), dim3(256), 0, st, x, n, v);
}
