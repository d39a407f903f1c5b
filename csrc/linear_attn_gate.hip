// Chunked linear attention with data-dependent scalar decay gates (the Mamba-2 / gated-RetNet form) for gfx950
// (CDNA4), 16-bit in / fp32 accumulate: the gated instantiations of the four kernels of linear_attn.hip and the gate's
// own kernels.
//
//   z[t,g] = xn[t] . Wg[g]                                     (fp32)
//   l[t,g] = log2 sigmoid(z + b_g) = min(u, 0) - log2(1 + exp2(-|u|)),  u = (z + b_g) log2(e)            (<= 0)
//   L[t,g] = sum_{s <= t} l[s,g]
//   o[i]   = scale sum_{j <= i} exp2(L[i] - L[j]) (q[i] . k[j]) v[j]
//
// for query head h of KV group g = h / (Hq / Hkv); there is no row normaliser.  The kernels never see L: they read
// Lambda [B T, Hkv] fp32, the inclusive prefix sum of l inside each chunk of C = 64 rows, so every decay factor is exp2
// of a difference of two values of one chunk, non-positive by construction:
//   intra-chunk weight           exp2(Lambda_a - Lambda_b), b <= a
//   query-side inter-chunk       exp2(Lambda_a)
//   chunk-local state            K_c^T (exp2(Lambda_{C-1} - Lambda_b) . V_c)
//   scan                         S_c = exp2(Lambda_{C-1}^(c)) S_{c-1} + local_c
// A workgroup stages its chunk's 64 Lambda values in LDS once (state: as the 64 factors it needs) and forms the decays
// from them where linear_attn.hip evaluates exp2(l2g n).  Work split, LDS images, MFMA order and the rounding points
// are those of linear_attn.hip, so the MFMA work is the same.
//
// Gate gradient.  With ln 2 folded away, dL[m,g] = sum_{h in g} dq[h,m] . q[h,m] - dk[m] . k[m]: the two terms nearly
// cancel, so qside<bwd> and kside take their row dots from the fp32 accumulators before the 16-bit rounding -- a
// per-lane partial over the 8 D / 16 registers the lane holds, combined across the two half-waves -- and write
// gq [B T, Hq] and gk [B T, Hkv].  Then
//   gate_dl    dl[s] = sum_{t >= s} dL[t] over the whole row, one workgroup per (KV head, batch): chunk totals by wave
//              reductions, their suffix scan by one wave (64 chunks per step, last to first), then a wave scan inside
//              each chunk; one fixed order, no atomics.  dz = dl (1 - a), a = sigmoid(z + b_g) rebuilt from z.
//   gate_dxn   dxn[t] = round16(float(dxn[t]) + sum_g dz[t,g] Wg[g]) in place, Wg staged in LDS.
//   gate_fwd   one workgroup per (chunk, batch): Wg staged in LDS (Hkv n_embd 2 bytes), the 64 rows' dot products as
//              wave reductions (16 rows per wave, up to 8 heads per pass over a row), the log-sigmoid, then the chunk's
//              prefix sum in LDS; writes z and Lambda.
// The weight gradient dWg = dz^T xn is moe.hip's dense router weight gradient (fp32 [N, E] times 16-bit rows).
#include "linear_attn_common.h"

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kGateLds = 160 * 1024;         // the most dynamic LDS a gate kernel may be launched with

struct LgArgs {
  LaArgs a;           // l2g unused
  const float* cum;   // [B T, Hkv] Lambda
  float* gq;          // [B T, Hq]  dq . q from the fp32 accumulators (qside<bwd>)
  float* gk;          // [B T, Hkv] dk . k (kside)
};

DLTB_DEV float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// sum_d acc^T[d][row] x[row][d] over the registers the lane holds, then over the two half-waves (both get the sum)
template <int D>
DLTB_DEV float acc_row_dot(const f32x16* acc, const bf16_t* xrow, int h) {
  float part = 0.f;
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    const bfx8 xf = ld_perm_frag(xrow, s, h);
#pragma unroll
    for (int j = 0; j < 8; ++j) part = fmaf(acc[s >> 1][8 * (s & 1) + j], (float)xf[j], part);
  }
  return part + __shfl_xor(part, 32, 64);
}

// =============================================================================== chunk-local states
// la_state_kernel with fac[b] = exp2(Lambda_{C-1} - Lambda_b) (fwd) / scale exp2(Lambda_a) (bwd)
template <int D, bool BWD>
__global__ __launch_bounds__(256) void lg_state_kernel(LgArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const LaArgs& P = A.a;
  char* xt = smem;
  char* yt = smem + kC * D * 2;
  float* fac = reinterpret_cast<float*>(smem + 2 * kC * D * 2);
  constexpr int NDB = D == 128 ? 4 : 1;
  const int c = blockIdx.x, g = blockIdx.y, b = blockIdx.z, nc = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5;
  const int eb = D == 128 ? w : (w & 1), db0 = D == 128 ? 0 : (w >> 1);
  const int G = P.Hq / P.Hkv;
  const long row0 = (long)b * P.T + (long)c * kC;
  if (tid < kC) {
    const float lam = A.cum[(row0 + tid) * P.Hkv + g];
    fac[tid] = BWD ? P.scale * ex2(lam) : ex2(A.cum[(row0 + kC - 1) * P.Hkv + g] - lam);
  }
  f32x16 acc[NDB];
#pragma unroll
  for (int n = 0; n < NDB; ++n) acc[n] = zero16();
  for (int hh = 0; hh < (BWD ? G : 1); ++hh) {
    const bf16_t* X = BWD ? P.q + row0 * P.q_stride + (long)(g * G + hh) * D : P.k + row0 * P.k_stride + (long)g * D;
    const bf16_t* Y = BWD ? P.dout + row0 * P.do_stride + (long)(g * G + hh) * D : P.v + row0 * P.v_stride + (long)g * D;
    __syncthreads();
    load_tile<D, kC, 256>(X, BWD ? P.q_stride : P.k_stride, xt, tid);
    load_tile<D, kC, 256>(Y, BWD ? P.do_stride : P.v_stride, yt, tid);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kC / 16; ++s) {
      bfx8 yf = tr_frag<D>(yt, 16 * s, 32 * eb, lane);
#pragma unroll
      for (int j = 0; j < 8; ++j) yf[j] = (h16_t)((float)yf[j] * fac[16 * s + acc_row(j, h)]);
#pragma unroll
      for (int n = 0; n < NDB; ++n) acc[n] = mfma32(tr_frag<D>(xt, 16 * s, 32 * (db0 + n), lane), yf, acc[n]);
    }
  }
  float* out = P.local + (((long)b * P.Hkv + g) * nc + c) * (long)(D * D);
#pragma unroll
  for (int n = 0; n < NDB; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(32 * (db0 + n) + acc_row(r, h)) * D + 32 * eb + (lane & 31)] = acc[n][r];
}

// =============================================================================== scan along the chunks
// la_scan_kernel with the chunk's own total decay exp2(Lambda_{C-1}^(c)), read per (batch, g, chunk); in either
// direction the step at chunk c multiplies by chunk c's decay.
__global__ __launch_bounds__(256) void lg_scan_kernel(const float* __restrict__ local, bf16_t* __restrict__ state,
                                                      const float* __restrict__ cum, int nc, int DD, int T,
                                                      int reverse) {
  const int idx = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, b = blockIdx.z, Hkv = gridDim.y;
  const long base = ((long)b * Hkv + g) * nc * (long)DD + idx;
  const float* last = cum + ((long)b * T + kC - 1) * Hkv + g;     // Lambda_{C-1} of chunk 0
  float s = 0.f;
  for (int i = 0; i < nc; ++i) {
    const int c = reverse ? nc - 1 - i : i;
    const long at = base + (long)c * DD;
    state[at] = f2bf(s);
    s = fmaf(ex2(last[(long)c * kC * Hkv]), s, local[at]);
  }
}

// =============================================================================== query side: o (fwd) and dq (bwd)
// la_qside_kernel with the decays from the staged Lambda; bwd also writes gq.
template <int D, bool BWD>
__global__ __launch_bounds__(128) void lg_qside_kernel(LgArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const LaArgs& P = A.a;
  char* sc = smem;                    // score operand rows (fwd K, bwd V)
  char* vl = smem + kC * D * 2;       // value rows (fwd V, bwd K)
  char* st = smem + 2 * kC * D * 2;   // S_{c-1} [D][D]
  float* lam = reinterpret_cast<float*>(smem + 2 * kC * D * 2 + D * D * 2);
  const int c = blockIdx.x, hq = blockIdx.y, b = blockIdx.z, nc = gridDim.x;
  const int G = P.Hq / P.Hkv, g = hq / G;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ql = 32 * w + (lane & 31);
  const long row0 = (long)b * P.T + (long)c * kC;
  if (tid < kC) lam[tid] = A.cum[(row0 + tid) * P.Hkv + g];
  const bf16_t* xrow = BWD ? P.dout + (row0 + ql) * P.do_stride + (long)hq * D : P.q + (row0 + ql) * P.q_stride + (long)hq * D;
  bfx8 xr[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) xr[s] = ld_row_frag(xrow, s, h);
  const bf16_t* kbase = P.k + row0 * P.k_stride + (long)g * D;
  const bf16_t* vbase = P.v + row0 * P.v_stride + (long)g * D;
  load_tile<D, kC, 128>(BWD ? vbase : kbase, BWD ? P.v_stride : P.k_stride, sc, tid);
  load_tile<D, kC, 128>(BWD ? kbase : vbase, BWD ? P.k_stride : P.v_stride, vl, tid);
  load_tile<D, D, 128>(P.state + (((long)b * P.Hkv + g) * nc + c) * (long)(D * D), D, st, tid);
  __syncthreads();
  f32x16 acc[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) acc[dt] = zero16();
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    if constexpr (BWD) {   // dq^T[d][i] = sum_e S[d][e] dO[i][e]
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) acc[dt] = mfma32(row_frag<D>(st, 32 * dt + (lane & 31), 2 * s + h), xr[s], acc[dt]);
    } else {               // o^T[e][i] = sum_d S[d][e] q[i][d]
      const bfx8 xp = ld_perm_frag(xrow, s, h);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) acc[dt] = mfma32(tr_frag<D>(st, 16 * s, 32 * dt, lane), xp, acc[dt]);
    }
  }
  const float lq = lam[ql], dq0 = ex2(lq);
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) acc[dt] *= dq0;
  for (int kb = 0; kb <= w; ++kb) {
    f32x16 p = zero16();
#pragma unroll
    for (int s = 0; s < D / 16; ++s) p = mfma32(row_frag<D>(sc, 32 * kb + (lane & 31), 2 * s + h), xr[s], p);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = 32 * kb + acc_row(r, h);
      p[r] = key <= ql ? p[r] * ex2(lq - lam[key]) : 0.f;
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const bfx8 pf = pack_frag(p, s2);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) acc[dt] = mfma32(tr_frag<D>(vl, 32 * kb + 16 * s2, 32 * dt, lane), pf, acc[dt]);
    }
  }
  store_acc_rows<D>(P.out + (row0 + ql) * P.out_stride + (long)hq * D, acc, P.scale, h);
  if constexpr (BWD) {
    const float gq = P.scale * acc_row_dot<D>(acc, P.q + (row0 + ql) * P.q_stride + (long)hq * D, h);
    if (h == 0) A.gq[(row0 + ql) * P.Hq + hq] = gq;
  }
}

// =============================================================================== key side: dk and dv
// la_kside_kernel with the decays from the staged Lambda; also writes gk.
template <int D>
__global__ __launch_bounds__(128) void lg_kside_kernel(LgArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const LaArgs& P = A.a;
  char* qt = smem;
  char* dot = smem + kC * D * 2;
  char* ds = smem + 2 * kC * D * 2;   // dS_c [D][D]
  float* lam = reinterpret_cast<float*>(smem + 2 * kC * D * 2 + D * D * 2);
  const int c = blockIdx.x, g = blockIdx.y, b = blockIdx.z, nc = gridDim.x;
  const int G = P.Hq / P.Hkv;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = 32 * w + (lane & 31);
  const long row0 = (long)b * P.T + (long)c * kC;
  const bf16_t* krow = P.k + (row0 + kl) * P.k_stride + (long)g * D;
  const bf16_t* vrow = P.v + (row0 + kl) * P.v_stride + (long)g * D;
  bfx8 kr[D / 16], vr[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    kr[s] = ld_row_frag(krow, s, h);
    vr[s] = ld_row_frag(vrow, s, h);
  }
  if (tid < kC) lam[tid] = A.cum[(row0 + tid) * P.Hkv + g];
  load_tile<D, D, 128>(P.state + (((long)b * P.Hkv + g) * nc + c) * (long)(D * D), D, ds, tid);
  __syncthreads();
  f32x16 dk[D / 32], dv[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) dk[dt] = dv[dt] = zero16();
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    const bfx8 kp = ld_perm_frag(krow, s, h);
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) {
      dk[dt] = mfma32(row_frag<D>(ds, 32 * dt + (lane & 31), 2 * s + h), vr[s], dk[dt]);   // sum_e dS[d][e] v[j][e]
      dv[dt] = mfma32(tr_frag<D>(ds, 16 * s, 32 * dt, lane), kp, dv[dt]);                  // sum_d dS[d][e] k[j][d]
    }
  }
  const float lk = lam[kl], dk0 = ex2(lam[kC - 1] - lk);
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) {
    dk[dt] *= dk0;
    dv[dt] *= dk0;
  }
  for (int hh = 0; hh < G; ++hh) {
    const long col = (long)(g * G + hh) * D;
    __syncthreads();
    load_tile<D, kC, 128>(P.q + row0 * P.q_stride + col, P.q_stride, qt, tid);
    load_tile<D, kC, 128>(P.dout + row0 * P.do_stride + col, P.do_stride, dot, tid);
    __syncthreads();
    for (int qb = w; qb < kC / 32; ++qb) {
      f32x16 sp = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        sp = mfma32(row_frag<D>(qt, 32 * qb + (lane & 31), 2 * s + h), kr[s], sp);    // q_i . k_j
        dp = mfma32(row_frag<D>(dot, 32 * qb + (lane & 31), 2 * s + h), vr[s], dp);   // do_i . v_j
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = 32 * qb + acc_row(r, h);
        const float f = i >= kl ? P.scale * ex2(lam[i] - lk) : 0.f;
        sp[r] *= f;
        dp[r] *= f;
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bfx8 sf = pack_frag(sp, s2), df = pack_frag(dp, s2);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
          dv[dt] = mfma32(tr_frag<D>(dot, 32 * qb + 16 * s2, 32 * dt, lane), sf, dv[dt]);
          dk[dt] = mfma32(tr_frag<D>(qt, 32 * qb + 16 * s2, 32 * dt, lane), df, dk[dt]);
        }
      }
    }
  }
  store_acc_rows<D>(P.out + (row0 + kl) * P.out_stride + (long)g * D, dk, 1.f, h);
  store_acc_rows<D>(P.out2 + (row0 + kl) * P.out2_stride + (long)g * D, dv, 1.f, h);
  const float gk = acc_row_dot<D>(dk, krow, h);
  if (h == 0) A.gk[(row0 + kl) * P.Hkv + g] = gk;
}

// =============================================================================== the gate: z and Lambda
// 16-byte chunks of Wg [Hkv][d] -> LDS, 256 threads
DLTB_DEV void stage_wg(const bf16_t* wg, bf16_t* w, int n, int tid) {
  for (int i = tid; i < n / 8; i += 256) reinterpret_cast<uint4*>(w)[i] = ld16<uint4>(wg + 8 * i);
}

__global__ __launch_bounds__(256) void lg_gate_fwd_kernel(const bf16_t* __restrict__ xn, const bf16_t* __restrict__ wg,
                                                          const float* __restrict__ bias, float* __restrict__ z,
                                                          float* __restrict__ cum, int T, int d, int Hkv) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* w = reinterpret_cast<bf16_t*>(smem);                          // Wg [Hkv][d]
  float* lg = reinterpret_cast<float*>(smem + (size_t)Hkv * d * 2);     // l [kC][Hkv]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long row0 = (long)blockIdx.y * T + (long)blockIdx.x * kC;
  stage_wg(wg, w, Hkv * d, tid);
  __syncthreads();
  for (int rr = 0; rr < kC / 4; ++rr) {
    const int r = (kC / 4) * wv + rr;
    const bf16_t* x = xn + (row0 + r) * d;
    for (int g0 = 0; g0 < Hkv; g0 += 8) {      // wave-uniform bounds throughout
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      for (int col = lane * 8; col < d; col += 512) {
        float xv[8];
        unpack8(ld16<uint4>(x + col), xv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (g0 + j < Hkv) {
            float wf[8];
            unpack8(*reinterpret_cast<const uint4*>(w + (size_t)(g0 + j) * d + col), wf);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[j] = fmaf(xv[i], wf[i], acc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (g0 + j < Hkv) {
          const float zz = wave_sum(acc[j]);
          if (lane == 0) {
            const float u = (zz + bias[g0 + j]) * kLog2e;
            z[(row0 + r) * Hkv + g0 + j] = zz;
            lg[r * Hkv + g0 + j] = fminf(u, 0.f) - __builtin_amdgcn_logf(1.f + ex2(-fabsf(u)));
          }
        }
      }
    }
  }
  __syncthreads();
  if (tid < Hkv) {      // the chunk's inclusive prefix sum, rows in order
    float s = 0.f;
    for (int r = 0; r < kC; ++r) {
      s += lg[r * Hkv + tid];
      cum[(row0 + r) * Hkv + tid] = s;
    }
  }
}

// =============================================================================== the gate's backward
// dl[s] = sum_{t >= s} (sum_{h in g} gq[t][h] - gk[t][g]) along a row of T tokens; dz = dl (1 - a), or dl when z is null
__global__ __launch_bounds__(256) void lg_gate_dl_kernel(const float* __restrict__ gq, const float* __restrict__ gk,
                                                         const float* __restrict__ z, const float* __restrict__ bias,
                                                         float* __restrict__ dz, int T, int Hq, int Hkv) {
  extern __shared__ float tot[];      // [T / kC] chunk totals, then per chunk the sum of the chunks after it
  const int g = blockIdx.x, b = blockIdx.y, G = Hq / Hkv, nc = T / kC;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  auto dL = [&](long row) {
    float v = 0.f;
    for (int hh = 0; hh < G; ++hh) v += gq[row * Hq + g * G + hh];
    return v - gk[row * Hkv + g];
  };
  for (int c = wv; c < nc; c += 4) {
    const float s = wave_sum(dL((long)b * T + (long)c * kC + lane));
    if (lane == 0) tot[c] = s;
  }
  __syncthreads();
  if (wv == 0) {
    float carry = 0.f;
    for (int c1 = nc; c1 > 0; c1 -= 64) {      // lane -> chunk c1 - 1 - lane
      const int c = c1 - 1 - lane;
      const float v = c >= 0 ? tot[c] : 0.f;
      float inc = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      if (c >= 0) tot[c] = carry + (inc - v);
      carry += __shfl(inc, 63, 64);
    }
  }
  __syncthreads();
  for (int c = wv; c < nc; c += 4) {
    const long row = (long)b * T + (long)c * kC + lane;
    float inc = dL(row);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float t = __shfl_down(inc, o, 64);
      if (lane + o < 64) inc += t;
    }
    float om = 1.f;
    if (z != nullptr) om = 1.f - 1.f / (1.f + ex2(-(z[row * Hkv + g] + bias[g]) * kLog2e));
    dz[row * Hkv + g] = (inc + tot[c]) * om;
  }
}

// dxn[r] = round16(float(dxn[r]) + sum_g dz[r][g] Wg[g]), heads in index order; 64 rows per workgroup
__global__ __launch_bounds__(256) void lg_gate_dxn_kernel(bf16_t* __restrict__ dxn, const bf16_t* __restrict__ wg,
                                                          const float* __restrict__ dz, long N, int d, int Hkv) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* w = reinterpret_cast<bf16_t*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  stage_wg(wg, w, Hkv * d, tid);
  __syncthreads();
  for (int rr = 0; rr < kC / 4; ++rr) {
    const long r = (long)blockIdx.x * kC + (kC / 4) * wv + rr;
    if (r >= N) break;
    for (int col = lane * 8; col < d; col += 512) {
      float a[8];
      unpack8(ld16<uint4>(dxn + r * d + col), a);
      for (int g = 0; g < Hkv; ++g) {
        const float s = dz[r * Hkv + g];
        float wf[8];
        unpack8(*reinterpret_cast<const uint4*>(w + (size_t)g * d + col), wf);
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = fmaf(s, wf[i], a[i]);
      }
      *reinterpret_cast<uint4*>(dxn + r * d + col) = pack8(a);
    }
  }
}

// =============================================================================== launches
template <int D, bool BWD>
void launch_state(const LgArgs& A, int nc, hipStream_t st) {
  allow_dynamic_lds<lg_state_kernel<D, BWD>>(state_lds<D>());
  hipLaunchKernelGGL((lg_state_kernel<D, BWD>), dim3(nc, A.a.Hkv, A.a.B), dim3(256), state_lds<D>(), st, A);
}
template <int D>
void launch_scan(const LgArgs& A, int nc, int reverse, hipStream_t st) {
  hipLaunchKernelGGL(lg_scan_kernel, dim3(D * D / 256, A.a.Hkv, A.a.B), dim3(256), 0, st, A.a.local, A.a.state, A.cum,
                     nc, D * D, A.a.T, reverse);
}
template <int D, bool BWD>
void launch_qside(const LgArgs& A, int nc, hipStream_t st) {
  allow_dynamic_lds<lg_qside_kernel<D, BWD>>(side_lds<D>());
  hipLaunchKernelGGL((lg_qside_kernel<D, BWD>), dim3(nc, A.a.Hq, A.a.B), dim3(128), side_lds<D>(), st, A);
}

template <int D>
void fwd_d(const LgArgs& A, hipStream_t st) {
  const int nc = A.a.T / kC;
  launch_state<D, false>(A, nc, st);
  launch_scan<D>(A, nc, 0, st);
  launch_qside<D, false>(A, nc, st);
}

template <int D>
void bwd_d(LgArgs A, bf16_t* dq, bf16_t* dk, bf16_t* dv, long dqs, long dks, long dvs, hipStream_t st) {
  const int nc = A.a.T / kC;
  launch_state<D, false>(A, nc, st);          // the forward's states, rebuilt
  launch_scan<D>(A, nc, 0, st);
  A.a.out = dq;
  A.a.out_stride = dqs;
  launch_qside<D, true>(A, nc, st);
  launch_state<D, true>(A, nc, st);           // the state gradients, in the same two buffers
  launch_scan<D>(A, nc, 1, st);
  A.a.out = dk;
  A.a.out_stride = dks;
  A.a.out2 = dv;
  A.a.out2_stride = dvs;
  allow_dynamic_lds<lg_kside_kernel<D>>(side_lds<D>());
  hipLaunchKernelGGL(lg_kside_kernel<D>, dim3(nc, A.a.Hkv, A.a.B), dim3(128), side_lds<D>(), st, A);
}

}  // namespace

bool dltb_linear_attn_gate_supported(int T, int d, int Hkv) {
  return T > 0 && T % kC == 0 && Hkv >= 1 && Hkv <= 64 && d >= 8 && d % 8 == 0 &&
         (long)Hkv * d * 2 + (long)kC * Hkv * 4 <= kGateLds && (long)(T / kC) * 4 <= kGateLds;
}

void dltb_linear_attn_gate_fwd(const void* xn, const void* wg, const float* bias, float* z, float* cum, int B, int T,
                               int d, int Hkv, hipStream_t st) {
  allow_dynamic_lds<lg_gate_fwd_kernel>(kGateLds);
  hipLaunchKernelGGL(lg_gate_fwd_kernel, dim3(T / kC, B), dim3(256), (size_t)Hkv * d * 2 + (size_t)kC * Hkv * 4, st,
                     (const bf16_t*)xn, (const bf16_t*)wg, bias, z, cum, T, d, Hkv);
}

void dltb_linear_attn_gate_bwd(const float* gq, const float* gk, const float* z, const float* bias, const void* wg,
                               float* dz, void* dxn, int B, int T, int d, int Hq, int Hkv, hipStream_t st) {
  allow_dynamic_lds<lg_gate_dl_kernel>(kGateLds);
  hipLaunchKernelGGL(lg_gate_dl_kernel, dim3(Hkv, B), dim3(256), (size_t)(T / kC) * 4, st, gq, gk, z, bias, dz, T, Hq,
                     Hkv);
  if (dxn == nullptr) return;
  allow_dynamic_lds<lg_gate_dxn_kernel>(kGateLds);
  hipLaunchKernelGGL(lg_gate_dxn_kernel, dim3(B * (T / kC)), dim3(256), (size_t)Hkv * d * 2, st, (bf16_t*)dxn,
                     (const bf16_t*)wg, dz, (long)B * T, d, Hkv);
}

void dltb_linear_attn_gate_dxn(void* dxn, const void* wg, const float* dz, long N, int d, int rows, hipStream_t st) {
  allow_dynamic_lds<lg_gate_dxn_kernel>(kGateLds);
  hipLaunchKernelGGL(lg_gate_dxn_kernel, dim3((unsigned)((N + kC - 1) / kC)), dim3(256), (size_t)rows * d * 2, st,
                     (bf16_t*)dxn, (const bf16_t*)wg, dz, N, d, rows);
}

void dltb_linear_attn_gated_fwd(const void* q, const void* k, const void* v, void* o, const float* cum, float* local,
                                void* state, long qs, long ks, long vs, long os, int B, int T, int Hq, int Hkv, int D,
                                float scale, hipStream_t st) {
  LgArgs A = {};
  LaArgs& P = A.a;
  A.cum = cum;
  P.q = (const bf16_t*)q; P.k = (const bf16_t*)k; P.v = (const bf16_t*)v;
  P.out = (bf16_t*)o; P.local = local; P.state = (bf16_t*)state;
  P.q_stride = qs; P.k_stride = ks; P.v_stride = vs; P.out_stride = os;
  P.B = B; P.T = T; P.Hq = Hq; P.Hkv = Hkv; P.scale = scale;
  if (D == 64) fwd_d<64>(A, st);
  else fwd_d<128>(A, st);
}

void dltb_linear_attn_gated_bwd(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk,
                                void* dv, const float* cum, float* gq, float* gk, float* local, void* state, long qs,
                                long ks, long vs, long dos, long dqs, long dks, long dvs, int B, int T, int Hq, int Hkv,
                                int D, float scale, hipStream_t st) {
  LgArgs A = {};
  LaArgs& P = A.a;
  A.cum = cum; A.gq = gq; A.gk = gk;
  P.q = (const bf16_t*)q; P.k = (const bf16_t*)k; P.v = (const bf16_t*)v; P.dout = (const bf16_t*)dout;
  P.local = local; P.state = (bf16_t*)state;
  P.q_stride = qs; P.k_stride = ks; P.v_stride = vs; P.do_stride = dos;
  P.B = B; P.T = T; P.Hq = Hq; P.Hkv = Hkv; P.scale = scale;
  if (D == 64) bwd_d<64>(A, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, dqs, dks, dvs, st);
  else bwd_d<128>(A, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, dqs, dks, dvs, st);
}
