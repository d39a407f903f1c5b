// Fused softmax cross-entropy forward + backward for gfx950 (F.cross_entropy with
// ignore_index, train_harness.py:99-103).
//
// One 512-thread workgroup per row; the whole bf16 row (V = 32000 -> 8 x 16-byte vectors per
// thread) stays in registers, so logits are read from HBM exactly once:
//     loss[r]      = logsumexp(z_r) - z_r[t_r]              (0 for ignored rows)
//     z_r (in place) <- softmax(z_r) - onehot(t_r)           (unscaled dlogits; 0 for ignored)
// The 1/count mean-reduction and the incoming grad_output are applied by the caller as a device
// scalar folded into the head GEMMs, so no host sync is needed anywhere.
//
// A head that processes its rows in chunks splits the two halves (xent_lse_kernel: loss and log-sum-exp, the
// logits only read; xent_bwd_lse_kernel: dlogits from the recomputed logits and the kept log-sum-exp).
#include "common.h"

namespace {

template <int VPT>
__global__ __launch_bounds__(512) void xent_kernel(bf16_t* __restrict__ logits,
                                                  const int64_t* __restrict__ targets,
                                                  float* __restrict__ loss, int V,
                                                  int64_t ignore_index) {
  __shared__ float red[8], red2[8];
  __shared__ float s_tlogit;
  const int row = blockIdx.x;
  bf16_t* z = logits + (long)row * V;
  const int64_t t = targets[row];
  const bool valid = (t != ignore_index) && t >= 0 && t < V;
  if (threadIdx.x == 0) s_tlogit = valid ? bf2f(z[t]) : 0.f;
  const int nvec = V >> 3;
  // one pass over the row: per-thread max m_t and e = exp(z - m_t) kept in registers, then ONE
  // block reduction of (m_t, sum e) pairs (online-softmax merge); the output rescales e by
  // exp(m_t - m) / sum instead of recomputing the exponentials
  float e[VPT][8];
  float mt = -INFINITY;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = j * 512 + threadIdx.x;
    if (i < nvec) {
      unpack8(ld16<uint4>(z + i * 8), e[j]);
#pragma unroll
      for (int k = 0; k < 8; ++k) mt = fmaxf(mt, e[j][k]);
    }
  }
  float st = 0.f;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = j * 512 + threadIdx.x;
    if (i < nvec) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        e[j][k] = __expf(e[j][k] - mt);
        st += e[j][k];
      }
    }
  }
  // (m, s) pairs: wave butterfly, then the 8 waves through LDS (fixed order)
  float m = mt, sm = st;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float mo = __shfl_xor(m, off);
    const float so = __shfl_xor(sm, off);
    const float mn = fmaxf(m, mo);
    sm = (m == -INFINITY ? 0.f : sm * __expf(m - mn)) + (mo == -INFINITY ? 0.f : so * __expf(mo - mn));
    m = mn;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    red[wid] = m;
    red2[wid] = sm;
  }
  __syncthreads();
  float M = -INFINITY;
#pragma unroll
  for (int w = 0; w < 8; ++w) M = fmaxf(M, red[w]);
  float S = 0.f;
#pragma unroll
  for (int w = 0; w < 8; ++w) S += red[w] == -INFINITY ? 0.f : red2[w] * __expf(red[w] - M);
  if (threadIdx.x == 0) loss[row] = valid ? (M + __logf(S) - s_tlogit) : 0.f;
  const float scale = mt == -INFINITY ? 0.f : __expf(mt - M) / S;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = j * 512 + threadIdx.x;
    if (i < nvec) {
      float f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float p = valid ? e[j][k] * scale : 0.f;
        if (valid && i * 8 + k == t) p -= 1.f;
        f[k] = p;
      }
      *reinterpret_cast<uint4*>(z + i * 8) = pack8(f);
    }
  }
}

// Block merge of the per-thread online-softmax pairs (m_t, sum exp(z - m_t)) into the row's (M, S): wave
// butterfly, then the 8 waves through LDS in a fixed order.  xent_kernel's merge statement for statement (that
// kernel keeps its own text, so its code object does not change): xent_lse_kernel's loss rows carry its bits.
DLTB_DEV void xent_merge(float mt, float st, float* red, float* red2, float& M, float& S) {
  float m = mt, sm = st;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float mo = __shfl_xor(m, off);
    const float so = __shfl_xor(sm, off);
    const float mn = fmaxf(m, mo);
    sm = (m == -INFINITY ? 0.f : sm * __expf(m - mn)) + (mo == -INFINITY ? 0.f : so * __expf(mo - mn));
    m = mn;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    red[wid] = m;
    red2[wid] = sm;
  }
  __syncthreads();
  M = -INFINITY;
#pragma unroll
  for (int w = 0; w < 8; ++w) M = fmaxf(M, red[w]);
  S = 0.f;
#pragma unroll
  for (int w = 0; w < 8; ++w) S += red[w] == -INFINITY ? 0.f : red2[w] * __expf(red[w] - M);
}

// The read-only half of xent_kernel, for a head that processes its rows in chunks and keeps no logits
// (models/mistral.py, head_chunk): the same per-thread (max, sum) pass in the same order and the same block
// merge, so loss[r] carries xent_kernel's bits, plus lse[r] = M + log S for xent_bwd_lse_kernel.  Nothing is
// written back, so the row is held as its 16-bit words (VPT x 4 registers) and unpacked in both passes.
template <int VPT>
__global__ __launch_bounds__(512) void xent_lse_kernel(const bf16_t* __restrict__ logits,
                                                      const int64_t* __restrict__ targets,
                                                      float* __restrict__ loss, float* __restrict__ lse,
                                                      int V, int64_t ignore_index) {
  __shared__ float red[8], red2[8];
  __shared__ float s_tlogit;
  const int row = blockIdx.x;
  const bf16_t* z = logits + (long)row * V;
  const int64_t t = targets[row];
  const bool valid = (t != ignore_index) && t >= 0 && t < V;
  if (threadIdx.x == 0) s_tlogit = valid ? bf2f(z[t]) : 0.f;
  const int nvec = V >> 3;
  uint4 raw[VPT];
  float mt = -INFINITY;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = j * 512 + threadIdx.x;
    if (i < nvec) {
      raw[j] = ld16<uint4>(z + i * 8);
      float f[8];
      unpack8(raw[j], f);
#pragma unroll
      for (int k = 0; k < 8; ++k) mt = fmaxf(mt, f[k]);
    }
  }
  float st = 0.f;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = j * 512 + threadIdx.x;
    if (i < nvec) {
      float f[8];
      unpack8(raw[j], f);
#pragma unroll
      for (int k = 0; k < 8; ++k) st += __expf(f[k] - mt);
    }
  }
  float M, S;
  xent_merge(mt, st, red, red2, M, S);
  if (threadIdx.x == 0) {
    loss[row] = valid ? (M + __logf(S) - s_tlogit) : 0.f;
    lse[row] = M + __logf(S);
  }
}

// dlogits of a chunk from its recomputed logits and the forward's lse, in place:
//   z[r][c] <- exp(z[r][c] - lse[r]) - (c == t_r)          (0 for ignored rows and out-of-range targets)
// No reduction, so the grid runs over the chunk's 16-byte vectors, not its rows (3 rows of V = 131072 are 192
// workgroups): a workgroup takes 256 consecutive vectors, finds its first (row, column) by one wave-uniform
// division and each thread its own by a 32-bit one; lse and the target are loaded per vector (cache hits).
__global__ __launch_bounds__(256) void xent_bwd_lse_kernel(bf16_t* __restrict__ logits,
                                                          const int64_t* __restrict__ targets,
                                                          const float* __restrict__ lse, int N, int V,
                                                          int64_t ignore_index) {
  const uint32_t nvec = (uint32_t)V >> 3;
  const long base = (long)blockIdx.x * 256;
  const long row0 = base / nvec;
  const uint32_t c = (uint32_t)(base - row0 * nvec) + threadIdx.x;      // < nvec + 256
  const uint32_t q = c / nvec;
  const long row = row0 + q;
  if (row >= N) return;
  const int col = (int)(c - q * nvec) * 8;
  bf16_t* p = logits + row * V + col;
  const int64_t t = targets[row];
  const bool valid = (t != ignore_index) && t >= 0 && t < V;
  float f[8];
  if (valid) {
    const float l = lse[row];
    unpack8(ld16<uint4>(p), f);
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = __expf(f[k] - l) - (col + k == t ? 1.f : 0.f);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = 0.f;
  }
  *reinterpret_cast<uint4*>(p) = pack8(f);
}

// mean over non-ignored rows in one 1024-thread workgroup (fixed summation order):
//   out[0] = sum(loss) / max(count, 1),  out[1] = max(count, 1)
__global__ __launch_bounds__(1024) void xent_mean_kernel(const float* __restrict__ loss,
                                                        const int64_t* __restrict__ targets, int N,
                                                        int64_t ignore_index, float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f, c = 0.f;
  for (int i = threadIdx.x; i < N; i += 1024) {
    s += loss[i];
    c += targets[i] != ignore_index ? 1.f : 0.f;
  }
  s = block_sum(s, red);
  c = block_sum(c, red);
  if (threadIdx.x == 0) {
    c = fmaxf(c, 1.f);
    out[0] = s / c;
    out[1] = c;
  }
}

// ---------------------------------------------------------------- head-loss options: final-logit cap, z-loss
// The three kernels above with two options (models/mistral.py, final_softcap / lm_z_loss_coef); they keep their
// text, so their code objects do not change, and the option-taking variants are kernels of their own:
//   c_j  = CAP ? cap tanh(z_j / cap) : z_j           fp32 in registers, never rounded to 16 bits
//   lse  = logsumexp_j c_j
//   loss = lse - c_t + zc lse^2
//   dz_j = (softmax(c)_j (1 + 2 zc lse) - [j == t]) (1 - tanh(z_j / cap)^2)       (last factor 1 without CAP)
// tanh in the form of the attention CAP kernels: e = exp2(2 log2(e) z / cap), r = rcp(1 + e), t = 1 - 2 r; r is
// exactly 0 / 1 and t exactly +-1 when exp2 overflows / underflows, so 1 - t^2 and dz are exactly 0 there.
// CAP is a compile-time switch and zc a runtime float: with zc == 0 the factor 1 + 2 zc lse is exactly 1.0f and
// zc lse^2 exactly 0 (one multiply / one fma, no bits).
// The fused kernel keeps ONE fp32 array per thread.  Without CAP it is xent_kernel's e = exp(z - m_t).  With CAP it
// is t (the output needs 1 - t^2, and c = cap t): the exponential of the sum pass is not kept but formed again in
// the output pass as exp(cap t - lse), one more v_exp per element instead of 64 more live registers at VPT = 8.
constexpr float kXeLog2e = 1.4426950408889634f;

DLTB_DEV float xent_tanh(float z, float capc) {     // capc = 2 log2(e) / cap
  return __builtin_fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(z * capc)), 1.f);
}

// The per-thread pass of a row, shared by the fused and the read-only kernel statement for statement (with
// xent_merge it makes their loss rows equal bit for bit): the thread's max m_t of c and its sum of exp(c - m_t).
// a[j][k] is left as exp(z - m_t) without CAP (xent_kernel's e) and as tanh(z / cap) with it.
template <int VPT, bool CAP>
DLTB_DEV void xent_thread_pass(const bf16_t* z, int nvec, float cap, float capc, float (&a)[VPT][8], float& mt,
                               float& st) {
  mt = -INFINITY;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = j * 512 + threadIdx.x;
    if (i < nvec) {
      unpack8(ld16<uint4>(z + i * 8), a[j]);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (CAP) {
          a[j][k] = xent_tanh(a[j][k], capc);
          mt = fmaxf(mt, cap * a[j][k]);
        } else {
          mt = fmaxf(mt, a[j][k]);
        }
      }
    }
  }
  st = 0.f;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = j * 512 + threadIdx.x;
    if (i < nvec) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (CAP) {
          st += __expf(__builtin_fmaf(cap, a[j][k], -mt));      // explicit fma: the same in both kernels
        } else {
          a[j][k] = __expf(a[j][k] - mt);
          st += a[j][k];
        }
      }
    }
  }
}

// loss row from the merged (M, S) and the target's c: lse - c_t + zc lse^2 in one fma (lse - c_t exactly when zc == 0)
DLTB_DEV float xent_loss_row(float lse, float ct, float zc) { return __builtin_fmaf(zc * lse, lse, lse - ct); }

template <int VPT, bool CAP>
__global__ __launch_bounds__(512) void xent_opt_kernel(bf16_t* __restrict__ logits,
                                                      const int64_t* __restrict__ targets,
                                                      float* __restrict__ loss, int V, int64_t ignore_index,
                                                      float cap, float zc) {
  __shared__ float red[8], red2[8];
  __shared__ float s_tlogit;
  const int row = blockIdx.x;
  bf16_t* z = logits + (long)row * V;
  const int64_t t = targets[row];
  const bool valid = (t != ignore_index) && t >= 0 && t < V;
  const float capc = CAP ? 2.f * kXeLog2e / cap : 0.f;
  if (threadIdx.x == 0) {
    const float zt = valid ? bf2f(z[t]) : 0.f;
    s_tlogit = CAP ? cap * xent_tanh(zt, capc) : zt;
  }
  const int nvec = V >> 3;
  float a[VPT][8];
  float mt, st;
  xent_thread_pass<VPT, CAP>(z, nvec, cap, capc, a, mt, st);
  float M, S;
  xent_merge(mt, st, red, red2, M, S);
  const float lse = M + __logf(S);
  if (threadIdx.x == 0) loss[row] = valid ? xent_loss_row(lse, s_tlogit, zc) : 0.f;
  const float kz = __builtin_fmaf(2.f * zc, lse, 1.f);                  // d(lse + zc lse^2) / d lse
  const float scale = (mt == -INFINITY ? 0.f : __expf(mt - M) / S) * kz;  // without CAP: xent_kernel's scale
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = j * 512 + threadIdx.x;
    if (i < nvec) {
      float f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float p = 0.f;
        if (valid) {
          p = CAP ? __expf(__builtin_fmaf(cap, a[j][k], -lse)) * kz : a[j][k] * scale;
          if (i * 8 + k == t) p -= 1.f;
          if (CAP) p *= __builtin_fmaf(-a[j][k], a[j][k], 1.f);
        }
        f[k] = p;
      }
      *reinterpret_cast<uint4*>(z + i * 8) = pack8(f);
    }
  }
}

// xent_lse_kernel with the options: xent_opt_kernel's thread pass and merge, so its loss rows; lse is that of c.
template <int VPT, bool CAP>
__global__ __launch_bounds__(512) void xent_lse_opt_kernel(const bf16_t* __restrict__ logits,
                                                          const int64_t* __restrict__ targets,
                                                          float* __restrict__ loss, float* __restrict__ lse_out,
                                                          int V, int64_t ignore_index, float cap, float zc) {
  __shared__ float red[8], red2[8];
  __shared__ float s_tlogit;
  const int row = blockIdx.x;
  const bf16_t* z = logits + (long)row * V;
  const int64_t t = targets[row];
  const bool valid = (t != ignore_index) && t >= 0 && t < V;
  const float capc = CAP ? 2.f * kXeLog2e / cap : 0.f;
  if (threadIdx.x == 0) {
    const float zt = valid ? bf2f(z[t]) : 0.f;
    s_tlogit = CAP ? cap * xent_tanh(zt, capc) : zt;
  }
  const int nvec = V >> 3;
  float a[VPT][8];
  float mt, st;
  xent_thread_pass<VPT, CAP>(z, nvec, cap, capc, a, mt, st);
  float M, S;
  xent_merge(mt, st, red, red2, M, S);
  const float lse = M + __logf(S);
  if (threadIdx.x == 0) {
    loss[row] = valid ? xent_loss_row(lse, s_tlogit, zc) : 0.f;
    lse_out[row] = lse;
  }
}

// xent_bwd_lse_kernel with the options (same grid over the chunk's vectors): from the kept lse of c,
//   z[r][j] <- (exp(c_j - lse[r]) (1 + 2 zc lse[r]) - (j == t_r)) (1 - tanh(z_j / cap)^2)
template <bool CAP>
__global__ __launch_bounds__(256) void xent_bwd_lse_opt_kernel(bf16_t* __restrict__ logits,
                                                              const int64_t* __restrict__ targets,
                                                              const float* __restrict__ lse, int N, int V,
                                                              int64_t ignore_index, float cap, float zc) {
  const uint32_t nvec = (uint32_t)V >> 3;
  const long base = (long)blockIdx.x * 256;
  const long row0 = base / nvec;
  const uint32_t c = (uint32_t)(base - row0 * nvec) + threadIdx.x;      // < nvec + 256
  const uint32_t q = c / nvec;
  const long row = row0 + q;
  if (row >= N) return;
  const int col = (int)(c - q * nvec) * 8;
  bf16_t* p = logits + row * V + col;
  const int64_t t = targets[row];
  const bool valid = (t != ignore_index) && t >= 0 && t < V;
  float f[8];
  if (valid) {
    const float l = lse[row];
    const float kz = __builtin_fmaf(2.f * zc, l, 1.f);
    const float capc = CAP ? 2.f * kXeLog2e / cap : 0.f;
    unpack8(ld16<uint4>(p), f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float th = CAP ? xent_tanh(f[k], capc) : 0.f;
      float g = __expf(CAP ? __builtin_fmaf(cap, th, -l) : f[k] - l) * kz - (col + k == t ? 1.f : 0.f);
      if (CAP) g *= __builtin_fmaf(-th, th, 1.f);
      f[k] = g;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = 0.f;
  }
  *reinterpret_cast<uint4*>(p) = pack8(f);
}

}  // namespace

void dltb_xent_mean(const float* loss, const int64_t* targets, int N, int64_t ignore_index, float* out,
                    hipStream_t st) {
  hipLaunchKernelGGL(xent_mean_kernel, dim3(1), dim3(1024), 0, st, loss, targets, N, ignore_index, out);
}

void dltb_xent_fwd_bwd(void* logits, const int64_t* targets, float* loss, int N, int V,
                       int64_t ignore_index, hipStream_t st) {
  const int vpt = cdiv(V / 8, 512);
#define DLTB_XE(K)                                                                              \
  hipLaunchKernelGGL(xent_kernel<K>, dim3(N), dim3(512), 0, st, (bf16_t*)logits, targets, loss, \
                     V, ignore_index)
  if (vpt <= 1) DLTB_XE(1);
  else if (vpt <= 2) DLTB_XE(2);
  else if (vpt <= 4) DLTB_XE(4);
  else if (vpt <= 8) DLTB_XE(8);
  else if (vpt <= 16) DLTB_XE(16);
  else DLTB_XE(32);
#undef DLTB_XE
}

void dltb_xent_lse(const void* logits, const int64_t* targets, float* loss, float* lse, int N, int V,
                   int64_t ignore_index, hipStream_t st) {
  const int vpt = cdiv(V / 8, 512);
#define DLTB_XL(K)                                                                              \
  hipLaunchKernelGGL(xent_lse_kernel<K>, dim3(N), dim3(512), 0, st, (const bf16_t*)logits, targets, \
                     loss, lse, V, ignore_index)
  if (vpt <= 1) DLTB_XL(1);
  else if (vpt <= 2) DLTB_XL(2);
  else if (vpt <= 4) DLTB_XL(4);
  else if (vpt <= 8) DLTB_XL(8);
  else if (vpt <= 16) DLTB_XL(16);
  else DLTB_XL(32);
#undef DLTB_XL
}

void dltb_xent_bwd_lse(void* logits, const int64_t* targets, const float* lse, int N, int V,
                       int64_t ignore_index, hipStream_t st) {
  const long blocks = ((long)N * (V / 8) + 255) / 256;
  hipLaunchKernelGGL(xent_bwd_lse_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (bf16_t*)logits, targets,
                     lse, N, V, ignore_index);
}

// the option-taking variants: softcap > 0 selects the CAP instantiations, z_coef is a runtime operand
void dltb_xent_fwd_bwd_opt(void* logits, const int64_t* targets, float* loss, int N, int V,
                           int64_t ignore_index, float softcap, float z_coef, hipStream_t st) {
  const int vpt = cdiv(V / 8, 512);
#define DLTB_XE(K, C)                                                                                   \
  hipLaunchKernelGGL((xent_opt_kernel<K, C>), dim3(N), dim3(512), 0, st, (bf16_t*)logits, targets, loss, \
                     V, ignore_index, softcap, z_coef)
#define DLTB_XEV(C)               \
  if (vpt <= 1) DLTB_XE(1, C);      \
  else if (vpt <= 2) DLTB_XE(2, C); \
  else if (vpt <= 4) DLTB_XE(4, C); \
  else if (vpt <= 8) DLTB_XE(8, C); \
  else if (vpt <= 16) DLTB_XE(16, C); \
  else DLTB_XE(32, C)
  if (softcap > 0.f) {
    DLTB_XEV(true);
  } else {
    DLTB_XEV(false);
  }
#undef DLTB_XEV
#undef DLTB_XE
}

void dltb_xent_lse_opt(const void* logits, const int64_t* targets, float* loss, float* lse, int N, int V,
                       int64_t ignore_index, float softcap, float z_coef, hipStream_t st) {
  const int vpt = cdiv(V / 8, 512);
#define DLTB_XL(K, C)                                                                                         \
  hipLaunchKernelGGL((xent_lse_opt_kernel<K, C>), dim3(N), dim3(512), 0, st, (const bf16_t*)logits, targets, \
                     loss, lse, V, ignore_index, softcap, z_coef)
#define DLTB_XLV(C)               \
  if (vpt <= 1) DLTB_XL(1, C);      \
  else if (vpt <= 2) DLTB_XL(2, C); \
  else if (vpt <= 4) DLTB_XL(4, C); \
  else if (vpt <= 8) DLTB_XL(8, C); \
  else if (vpt <= 16) DLTB_XL(16, C); \
  else DLTB_XL(32, C)
  if (softcap > 0.f) {
    DLTB_XLV(true);
  } else {
    DLTB_XLV(false);
  }
#undef DLTB_XLV
#undef DLTB_XL
}

void dltb_xent_bwd_lse_opt(void* logits, const int64_t* targets, const float* lse, int N, int V,
                           int64_t ignore_index, float softcap, float z_coef, hipStream_t st) {
  const long blocks = ((long)N * (V / 8) + 255) / 256;
  if (softcap > 0.f)
    hipLaunchKernelGGL(xent_bwd_lse_opt_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, (bf16_t*)logits,
                       targets, lse, N, V, ignore_index, softcap, z_coef);
  else
    hipLaunchKernelGGL(xent_bwd_lse_opt_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, (bf16_t*)logits,
                       targets, lse, N, V, ignore_index, softcap, z_coef);
}
