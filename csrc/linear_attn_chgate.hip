// Chunked linear attention with per-channel decay gates (the GLA / RWKV-6 form) for gfx950 (CDNA4), 16-bit in / fp32
// accumulate: one decay per token, KV head and key channel.
//
//   z1[t,:] = xn[t] . W1^T  (fp32, W1 [R, n_embd]),   z[t,c] = sum_r z1[t,r] W2[c,r]  (W2 [Hkv D, R]),  c = g D + d
//   l[t,c]  = log2 sigmoid(z + b_g) = min(u, 0) - log2(1 + exp2(-|u|)),  u = (z + b_g) log2(e)                   (<= 0)
//   o[i]    = scale sum_{j <= i} (sum_d q[i,d] k[j,d] exp2(L[i,d] - L[j,d])) v[j],   L = the running sum of l
//
// The kernels read Lambda [B T, Hkv D] fp32, the inclusive prefix sum of l inside each chunk of C = 64 rows, and every
// decay factor is exp2 of a non-positive difference of two values of one chunk's Lambda (dec() below also clamps, so a
// masked-out pair cannot overflow either).  A workgroup stages its chunk's [64][D] Lambda tile in LDS once (row stride
// D + 4 floats: 16-byte aligned rows whose by-row reads are at most 2-way bank conflicted).
//
//   state   local[d,e] = sum_b (k[b,d] exp2(Lambda[C-1,d] - Lambda[b,d])) v[b,e]: the factor sits on the K fragment,
//           rounded once where it becomes the MFMA operand (bwd: scale q[a,d] exp2(Lambda[a,d]) against dO).
//   scan    S_c[d,:] = exp2(Lambda^(c)[C-1,d]) S_{c-1}[d,:] + local_c[d,:], one decay per state row.
//   qside   fwd: (q exp2(Lambda_i)) S_{c-1} + the intra-chunk scores;  bwd: dq and gq = dq * q per channel.
//   kside   dk, dv and gk = dk * k per channel, the group's query heads summed in index order.
//
// Intra-chunk scores: secondary chunking with sub-blocks of s = 16 rows.  A wave owns 32 query (key) rows, as in
// linear_attn_gate.hip, and meets three kinds of 16 x 16 sub-block:
//   * the other 32-row block of the chunk (wave 1's queries against keys 0..31): one 32x32x16 MFMA set with the
//     reference rho_d = Lambda[31, d], q~ = q exp2(Lambda_i - rho), k~ = k exp2(rho - Lambda_j), each rounded once;
//   * the lower-left quadrant of its own 32 x 32 block (queries 16..31 against keys 0..15): the same MFMA set with
//     rho_d = Lambda[15, d] of the block and the other rows' operands set to zero;
//   * the two diagonal sub-blocks: no reference keeps both exponents non-positive, so they are exact in fp32 on the
//     vector ALU, sum_d q k exp2(Lambda_id - Lambda_jd) per (i, j <= i).  A lane owns one row and the D / 2 channels of
//     its half-wave (the channel set of its accumulator registers, so the backward adds straight into dq / dk); the 16
//     partner rows come from the LDS tiles as broadcast reads; tile values pass between the MFMA register layout and
//     the per-row loop through a [32][33] fp32 exchange tile per wave.
// s = 16 rather than 32: the exact part is the vector-ALU cost of this form (one exp2 per (i, j, d)), and 16 halves it
// for one more MFMA set per wave, which is cheap beside it.
// In the backward dP = dO V^T is an undecayed MFMA tile; the off-diagonal parts of dq / dk are MFMA products against the
// decayed operand (k~ / q~) whose accumulator takes the per-(row, d) factor exp2(Lambda_id - rho_d) / exp2(rho_d -
// Lambda_jd), the diagonal parts use the fp32 dP and the exact weights.  dv uses the decayed scores.
//
// The gate: gate_fwd (one workgroup per (chunk, batch): W1 in LDS, z1 by wave reductions, then one thread per channel
// forms the 64 rows' z, l and the prefix sum in row order) and gate_bwd (dl = suffix sum of dL = sum_{h in g} gq - gk
// per (batch, channel): chunk totals, their scan, then inside each chunk; dz = dl (1 - a); dz1 = dz W2; dW2 = dz^T z1 by
// a fixed-order two-stage reduction).  dxn and dW1 go through lg_gate_dxn_kernel and the dense router weight gradient.
#include "linear_attn_common.h"

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kGateLds = 160 * 1024;
constexpr int kXl = 33;                          // row stride of an exchange tile
constexpr int kXchBytes = 2 * 2 * 32 * kXl * 4;  // two tiles per wave, two waves

template <int D>
constexpr int lam_ld() { return D + 4; }
template <int D>
constexpr int lam_bytes() { return kC * lam_ld<D>() * 4; }
template <int D>
constexpr int cstate_lds() { return 2 * kC * D * 2 + lam_bytes<D>(); }
template <int D>
constexpr int cside_lds() { return 2 * kC * D * 2 + D * D * 2 + lam_bytes<D>() + kXchBytes; }

struct LcArgs {
  LaArgs a;           // l2g unused
  const float* cum;   // [B T, Hkv D] Lambda
  float* gq;          // [B T, Hq D]  dq * q from the fp32 accumulators (qside<bwd>)
  float* gk;          // [B T, Hkv D] dk * k (kside)
};

DLTB_DEV float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
DLTB_DEV float dec(float x) { return ex2(fminf(x, 0.f)); }     // a decay: exp2 of a non-positive difference

template <int D, int NT>
DLTB_DEV void stage_lam(const float* src, long stride, float* lam, int tid) {
  for (int i = tid; i < kC * D / 4; i += NT) {
    const int row = i / (D / 4), c4 = i % (D / 4);
    *reinterpret_cast<float4*>(lam + row * lam_ld<D>() + 4 * c4) =
        *reinterpret_cast<const float4*>(src + (long)row * stride + 4 * c4);
  }
}

// the lane's channel set: for u < D / 8 the four channels 8 u + 4 h .. + 3.  It is the set of its accumulator
// registers (acc[u >> 2][4 (u & 3) + c]) and of its ld_perm_frag elements (frag[u >> 1][4 (u & 1) + c]).
template <int D>
DLTB_DEV void lam4(const float* lam, int row, int u, int h, float (&o)[4]) {
  const float4 v = *reinterpret_cast<const float4*>(lam + row * lam_ld<D>() + 8 * u + 4 * h);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
template <int D>
DLTB_DEV void tile4(const char* tile, int row, int u, int h, float (&o)[4]) {
  typedef h16_t h16x4 __attribute__((ext_vector_type(4)));
  const h16x4 v = *reinterpret_cast<const h16x4*>(tile + toff<D>(row, u) + 8 * h);
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = (float)v[c];
}
// 8 consecutive values of a Lambda row (the channels 16 s + 8 h .. + 7 of a row-order fragment)
template <int D>
DLTB_DEV void lam8(const float* lam, int row, int s, int h, float (&o)[8]) {
  const float* p = lam + row * lam_ld<D>() + 16 * s + 8 * h;
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

// a row-order fragment of row `row` times exp2(sign (Lambda[row] - Lambda[ref])), or zero when the row is masked out
template <int D>
DLTB_DEV bfx8 decay_row_frag(bfx8 f, const float* lam, int row, int ref, int s, int h, float sign, bool on) {
  float lr[8], lf[8];
  lam8<D>(lam, row, s, h, lr);
  lam8<D>(lam, ref, s, h, lf);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (h16_t)(on ? (float)f[j] * dec(sign * (lr[j] - lf[j])) : 0.f);
  return f;
}
// a transposed fragment (tile rows row_base + acc_row(j, h), column d) times exp2(sign (Lambda[row, d] - Lambda[ref, d]))
template <int D>
DLTB_DEV bfx8 decay_tr_frag(bfx8 f, const float* lam, int row_base, int ref, int d, int h, float sign) {
  const float lf = lam[ref * lam_ld<D>() + d];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    f[j] = (h16_t)((float)f[j] * dec(sign * (lam[(row_base + acc_row(j, h)) * lam_ld<D>() + d] - lf)));
  return f;
}

// =============================================================================== chunk-local states
template <int D, bool BWD>
__global__ __launch_bounds__(256) void lc_state_kernel(LcArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const LaArgs& P = A.a;
  char* xt = smem;
  char* yt = smem + kC * D * 2;
  float* lam = reinterpret_cast<float*>(smem + 2 * kC * D * 2);
  constexpr int NDB = D == 128 ? 4 : 1, LL = lam_ld<D>();
  const int c = blockIdx.x, g = blockIdx.y, b = blockIdx.z, nc = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5;
  const int eb = D == 128 ? w : (w & 1), db0 = D == 128 ? 0 : (w >> 1);
  const int G = P.Hq / P.Hkv;
  const long row0 = (long)b * P.T + (long)c * kC, ldc = (long)P.Hkv * D;
  stage_lam<D, 256>(A.cum + row0 * ldc + (long)g * D, ldc, lam, tid);
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
      const bfx8 yf = tr_frag<D>(yt, 16 * s, 32 * eb, lane);
#pragma unroll
      for (int n = 0; n < NDB; ++n) {
        const int d = 32 * (db0 + n) + (lane & 31);
        bfx8 xf = tr_frag<D>(xt, 16 * s, 32 * (db0 + n), lane);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float lr = lam[(16 * s + acc_row(j, h)) * LL + d];
          const float f = BWD ? P.scale * dec(lr) : dec(lam[(kC - 1) * LL + d] - lr);
          xf[j] = (h16_t)((float)xf[j] * f);
        }
        acc[n] = mfma32(xf, yf, acc[n]);
      }
    }
  }
  float* out = P.local + (((long)b * P.Hkv + g) * nc + c) * (long)(D * D);
#pragma unroll
  for (int n = 0; n < NDB; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(32 * (db0 + n) + acc_row(r, h)) * D + 32 * eb + (lane & 31)] = acc[n][r];
}

// =============================================================================== scan along the chunks
__global__ __launch_bounds__(256) void lc_scan_kernel(const float* __restrict__ local, bf16_t* __restrict__ state,
                                                      const float* __restrict__ cum, int nc, int D, int T,
                                                      int reverse) {
  const int idx = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, b = blockIdx.z, Hkv = gridDim.y;
  const long DD = (long)D * D, base = ((long)b * Hkv + g) * nc * DD + idx, ldc = (long)Hkv * D;
  const float* last = cum + ((long)b * T + kC - 1) * ldc + (long)g * D + idx / D;     // Lambda_{C-1, d} of chunk 0
  float s = 0.f;
  for (int i = 0; i < nc; ++i) {
    const int c = reverse ? nc - 1 - i : i;
    const long at = base + (long)c * DD;
    state[at] = f2bf(s);
    s = fmaf(dec(last[(long)c * kC * ldc]), s, local[at]);
  }
}

// =============================================================================== query side: o (fwd) and dq (bwd)
template <int D, bool BWD>
__global__ __launch_bounds__(128) void lc_qside_kernel(LcArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const LaArgs& P = A.a;
  char* sc = smem;                    // score operand rows (fwd K, bwd V)
  char* vl = smem + kC * D * 2;       // value rows (fwd V, bwd K)
  char* st = smem + 2 * kC * D * 2;   // S_{c-1} [D][D]
  float* lam = reinterpret_cast<float*>(smem + 2 * kC * D * 2 + D * D * 2);
  const int c = blockIdx.x, hq = blockIdx.y, b = blockIdx.z, nc = gridDim.x;
  const int G = P.Hq / P.Hkv, g = hq / G;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l31 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* xch = reinterpret_cast<float*>(smem + 2 * kC * D * 2 + D * D * 2 + lam_bytes<D>()) + w * 2 * 32 * kXl;
  const int ql = 32 * w + l31, qsub = l31 >> 4, base = 32 * w + 16 * qsub;
  const long row0 = (long)b * P.T + (long)c * kC, ldc = (long)P.Hkv * D;
  const bf16_t* qrow = P.q + (row0 + ql) * P.q_stride + (long)hq * D;
  const bf16_t* xrow = BWD ? P.dout + (row0 + ql) * P.do_stride + (long)hq * D : qrow;
  bfx8 xr[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) xr[s] = ld_row_frag(xrow, s, h);
  const bf16_t* kbase = P.k + row0 * P.k_stride + (long)g * D;
  const bf16_t* vbase = P.v + row0 * P.v_stride + (long)g * D;
  load_tile<D, kC, 128>(BWD ? vbase : kbase, BWD ? P.v_stride : P.k_stride, sc, tid);
  load_tile<D, kC, 128>(BWD ? kbase : vbase, BWD ? P.k_stride : P.v_stride, vl, tid);
  load_tile<D, D, 128>(P.state + (((long)b * P.Hkv + g) * nc + c) * (long)(D * D), D, st, tid);
  stage_lam<D, 128>(A.cum + row0 * ldc + (long)g * D, ldc, lam, tid);
  __syncthreads();
  const char* ktile = BWD ? vl : sc;
  f32x16 acc[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) acc[dt] = zero16();
  // ---- the state's term
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    if constexpr (BWD) {   // dq^T[d][i] = sum_e S[d][e] dO[i][e]
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) acc[dt] = mfma32(row_frag<D>(st, 32 * dt + l31, 2 * s + h), xr[s], acc[dt]);
    } else {               // o^T[e][i] = sum_d S[d][e] (q[i][d] exp2(Lambda[i][d]))
      bfx8 xp = ld_perm_frag(xrow, s, h);
#pragma unroll
      for (int u2 = 0; u2 < 2; ++u2) {
        float li[4];
        lam4<D>(lam, ql, 2 * s + u2, h, li);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) xp[4 * u2 + cc] = (h16_t)((float)xp[4 * u2 + cc] * dec(li[cc]));
      }
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) acc[dt] = mfma32(tr_frag<D>(st, 16 * s, 32 * dt, lane), xp, acc[dt]);
    }
  }
  if constexpr (BWD) {
#pragma unroll
    for (int u = 0; u < D / 8; ++u) {
      float li[4];
      lam4<D>(lam, ql, u, h, li);
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) acc[u >> 2][4 * (u & 3) + cc] *= dec(li[cc]);
    }
  }
  // ---- the chunk's own keys
  for (int kb = 0; kb <= w; ++kb) {
    const bool diag = kb == w;
    const int rho = diag ? 32 * w + 15 : 31;              // the reference row of this block's MFMA part
    const bool qon = !diag || qsub == 1, kon = !diag || qsub == 0;      // (kon: the lane as an A-operand key row)
    f32x16 p = zero16();
    if constexpr (!BWD) {
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        const bfx8 kf = decay_row_frag<D>(row_frag<D>(sc, 32 * kb + l31, 2 * s + h), lam, 32 * kb + l31, rho, s, h, -1.f, kon);
        const bfx8 qf = decay_row_frag<D>(xr[s], lam, ql, rho, s, h, 1.f, qon);
        p = mfma32(kf, qf, p);
      }
    } else {
#pragma unroll
      for (int s = 0; s < D / 16; ++s) p = mfma32(row_frag<D>(sc, 32 * kb + l31, 2 * s + h), xr[s], p);   // dP, undecayed
    }
    if (diag) {
      if constexpr (BWD) {      // the whole fp32 dP block -> exchange tile, then keep the quadrant for the MFMA part
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          xch[l31 * kXl + acc_row(r, h)] = p[r];
          if (!(qsub == 1 && acc_row(r, h) < 16)) p[r] = 0.f;
        }
        __builtin_amdgcn_wave_barrier();
      } else {                  // exact diagonal scores: the lane's row against the 16 rows of its sub-block
        bfx8 qp[D / 16];
#pragma unroll
        for (int s = 0; s < D / 16; ++s) qp[s] = ld_perm_frag(qrow, s, h);
#pragma unroll 1
        for (int jj = 0; jj < 16; ++jj) {
          const int pr = base + jj;
          float part = 0.f;
#pragma unroll
          for (int u = 0; u < D / 8; ++u) {
            float li[4], lj[4], k4[4];
            lam4<D>(lam, ql, u, h, li);
            lam4<D>(lam, pr, u, h, lj);
            tile4<D>(ktile, pr, u, h, k4);
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
              part = fmaf((float)qp[u >> 1][4 * (u & 1) + cc] * k4[cc], dec(li[cc] - lj[cc]), part);
          }
          part += __shfl_xor(part, 32, 64);
          if (h == 0) xch[l31 * kXl + 16 * qsub + jj] = pr <= ql ? part : 0.f;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if ((acc_row(r, h) >> 4) == qsub) p[r] = xch[l31 * kXl + acc_row(r, h)];
      }
    }
    if constexpr (!BWD) {       // o += P V
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bfx8 pf = pack_frag(p, s2);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) acc[dt] = mfma32(tr_frag<D>(vl, 32 * kb + 16 * s2, 32 * dt, lane), pf, acc[dt]);
      }
    } else {                    // dq += exp2(Lambda_i - rho) . (dP (k exp2(rho - Lambda_j)))
      f32x16 tmp[D / 32];
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) tmp[dt] = zero16();
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bfx8 pf = pack_frag(p, s2);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
          tmp[dt] = mfma32(decay_tr_frag<D>(tr_frag<D>(vl, 32 * kb + 16 * s2, 32 * dt, lane), lam, 32 * kb + 16 * s2, rho,
                                            32 * dt + l31, h, -1.f), pf, tmp[dt]);
      }
#pragma unroll
      for (int u = 0; u < D / 8; ++u) {
        float li[4], lr[4];
        lam4<D>(lam, ql, u, h, li);
        lam4<D>(lam, rho, u, h, lr);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          acc[u >> 2][4 * (u & 3) + cc] = fmaf(tmp[u >> 2][4 * (u & 3) + cc], dec(li[cc] - lr[cc]), acc[u >> 2][4 * (u & 3) + cc]);
      }
      if (diag) {               // the exact diagonal part, straight into the accumulators
#pragma unroll 1
        for (int jj = 0; jj < 16; ++jj) {
          const int pr = base + jj;
          const float dp = pr <= ql ? xch[l31 * kXl + 16 * qsub + jj] : 0.f;
#pragma unroll
          for (int u = 0; u < D / 8; ++u) {
            float li[4], lj[4], k4[4];
            lam4<D>(lam, ql, u, h, li);
            lam4<D>(lam, pr, u, h, lj);
            tile4<D>(ktile, pr, u, h, k4);
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
              acc[u >> 2][4 * (u & 3) + cc] = fmaf(dp * k4[cc], dec(li[cc] - lj[cc]), acc[u >> 2][4 * (u & 3) + cc]);
          }
        }
      }
    }
  }
  store_acc_rows<D>(P.out + (row0 + ql) * P.out_stride + (long)hq * D, acc, P.scale, h);
  if constexpr (BWD) {          // gq = dq * q per channel, from the accumulators
    float* gq = A.gq + (row0 + ql) * ((long)P.Hq * D) + (long)hq * D;
#pragma unroll
    for (int u = 0; u < D / 8; ++u) {
      const bfx8 qp = ld_perm_frag(qrow, u >> 1, h);
      float4 o;
      o.x = P.scale * acc[u >> 2][4 * (u & 3) + 0] * (float)qp[4 * (u & 1) + 0];
      o.y = P.scale * acc[u >> 2][4 * (u & 3) + 1] * (float)qp[4 * (u & 1) + 1];
      o.z = P.scale * acc[u >> 2][4 * (u & 3) + 2] * (float)qp[4 * (u & 1) + 2];
      o.w = P.scale * acc[u >> 2][4 * (u & 3) + 3] * (float)qp[4 * (u & 1) + 3];
      *reinterpret_cast<float4*>(gq + 8 * u + 4 * h) = o;
    }
  }
}

// =============================================================================== key side: dk and dv
// WHAT: 0 both outputs, 1 dk (and gk) only, 2 dv only.  At D = 128 both sets of accumulators beside the exact loop's
// operands do not fit the register file, so the launch runs the kernel twice, once per output.
template <int D, int WHAT>
__global__ __launch_bounds__(128) void lc_kside_kernel(LcArgs A) {
  constexpr bool DK = WHAT != 2, DV = WHAT != 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const LaArgs& P = A.a;
  char* qt = smem;
  char* dot = smem + kC * D * 2;
  char* ds = smem + 2 * kC * D * 2;   // dS_c [D][D]
  float* lam = reinterpret_cast<float*>(smem + 2 * kC * D * 2 + D * D * 2);
  const int c = blockIdx.x, g = blockIdx.y, b = blockIdx.z, nc = gridDim.x;
  const int G = P.Hq / P.Hkv;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l31 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* xch = reinterpret_cast<float*>(smem + 2 * kC * D * 2 + D * D * 2 + lam_bytes<D>()) + w * 2 * 32 * kXl;
  float* xs = xch + 32 * kXl;
  const int kl = 32 * w + l31, qsub = l31 >> 4, base = 32 * w + 16 * qsub;
  const long row0 = (long)b * P.T + (long)c * kC, ldc = (long)P.Hkv * D;
  const bf16_t* krow = P.k + (row0 + kl) * P.k_stride + (long)g * D;
  const bf16_t* vrow = P.v + (row0 + kl) * P.v_stride + (long)g * D;
  bfx8 kr[D / 16], vr[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    kr[s] = ld_row_frag(krow, s, h);
    vr[s] = ld_row_frag(vrow, s, h);
  }
  stage_lam<D, 128>(A.cum + row0 * ldc + (long)g * D, ldc, lam, tid);
  load_tile<D, D, 128>(P.state + (((long)b * P.Hkv + g) * nc + c) * (long)(D * D), D, ds, tid);
  __syncthreads();
  f32x16 dk[D / 32], dv[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) dk[dt] = dv[dt] = zero16();
  // ---- the later chunks' term: dk[j,d] = exp2(Lambda[C-1,d] - Lambda[j,d]) sum_e dS[d][e] v[j][e],
  //      dv[j,e] = sum_d dS[d][e] (k[j][d] exp2(Lambda[C-1,d] - Lambda[j,d]))
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    bfx8 kp = ld_perm_frag(krow, s, h);
#pragma unroll
    for (int u2 = 0; u2 < 2; ++u2) {
      float lj[4], le[4];
      lam4<D>(lam, kl, 2 * s + u2, h, lj);
      lam4<D>(lam, kC - 1, 2 * s + u2, h, le);
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) kp[4 * u2 + cc] = (h16_t)((float)kp[4 * u2 + cc] * dec(le[cc] - lj[cc]));
    }
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) {
      if constexpr (DK) dk[dt] = mfma32(row_frag<D>(ds, 32 * dt + l31, 2 * s + h), vr[s], dk[dt]);
      if constexpr (DV) dv[dt] = mfma32(tr_frag<D>(ds, 16 * s, 32 * dt, lane), kp, dv[dt]);
    }
  }
#pragma unroll
  for (int u = 0; u < D / 8; ++u) {
    float lj[4], le[4];
    lam4<D>(lam, kl, u, h, lj);
    lam4<D>(lam, kC - 1, u, h, le);
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) dk[u >> 2][4 * (u & 3) + cc] *= dec(le[cc] - lj[cc]);
  }
  // ---- the chunk's own queries, head by head
  for (int hh = 0; hh < G; ++hh) {
    const long col = (long)(g * G + hh) * D;
    __syncthreads();
    load_tile<D, kC, 128>(P.q + row0 * P.q_stride + col, P.q_stride, qt, tid);
    load_tile<D, kC, 128>(P.dout + row0 * P.do_stride + col, P.do_stride, dot, tid);
    __syncthreads();
    for (int qb = w; qb < kC / 32; ++qb) {
      const bool diag = qb == w;
      const int rho = diag ? 32 * w + 15 : 31;
      const bool qon = !diag || qsub == 1, kon = !diag || qsub == 0;    // (qon: the lane as an A-operand query row)
      f32x16 sp = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        const bfx8 qf = decay_row_frag<D>(row_frag<D>(qt, 32 * qb + l31, 2 * s + h), lam, 32 * qb + l31, rho, s, h, 1.f, qon);
        const bfx8 kf = decay_row_frag<D>(kr[s], lam, kl, rho, s, h, -1.f, kon);
        if constexpr (DV) sp = mfma32(qf, kf, sp);                                                          // decayed q_i . k_j
        if constexpr (DK) dp = mfma32(row_frag<D>(dot, 32 * qb + l31, 2 * s + h), vr[s], dp);               // do_i . v_j, undecayed
      }
      if (diag) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          xch[l31 * kXl + acc_row(r, h)] = dp[r];
          if (!(qsub == 0 && acc_row(r, h) >= 16)) dp[r] = 0.f;
        }
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sp[r] *= P.scale;
        dp[r] *= P.scale;
      }
      if constexpr (DK) {   // dk += exp2(rho - Lambda_j) . (dP^T (q exp2(Lambda_i - rho)))
        f32x16 tmp[D / 32];
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) tmp[dt] = zero16();
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const bfx8 df = pack_frag(dp, s2);
#pragma unroll
          for (int dt = 0; dt < D / 32; ++dt)
            tmp[dt] = mfma32(decay_tr_frag<D>(tr_frag<D>(qt, 32 * qb + 16 * s2, 32 * dt, lane), lam, 32 * qb + 16 * s2, rho,
                                              32 * dt + l31, h, 1.f), df, tmp[dt]);
        }
#pragma unroll
        for (int u = 0; u < D / 8; ++u) {
          float lj[4], lr[4];
          lam4<D>(lam, kl, u, h, lj);
          lam4<D>(lam, rho, u, h, lr);
#pragma unroll
          for (int cc = 0; cc < 4; ++cc)
            dk[u >> 2][4 * (u & 3) + cc] = fmaf(tmp[u >> 2][4 * (u & 3) + cc], dec(lr[cc] - lj[cc]), dk[u >> 2][4 * (u & 3) + cc]);
        }
      }
      if (diag) {   // exact diagonal: the lane's key row against the 16 query rows of its sub-block
        bfx8 kp[D / 16];
#pragma unroll
        for (int s = 0; s < D / 16; ++s) kp[s] = ld_perm_frag(krow, s, h);
#pragma unroll 1
        for (int ii = 0; ii < 16; ++ii) {
          const int pr = base + ii;
          const float dpij = DK && pr >= kl ? P.scale * xch[l31 * kXl + 16 * qsub + ii] : 0.f;
          float part = 0.f;
#pragma unroll
          for (int u = 0; u < D / 8; ++u) {
            float li[4], lj[4], q4[4];
            lam4<D>(lam, pr, u, h, li);
            lam4<D>(lam, kl, u, h, lj);
            tile4<D>(qt, pr, u, h, q4);
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
              const float t = q4[cc] * dec(li[cc] - lj[cc]);
              if constexpr (DV) part = fmaf(t, (float)kp[u >> 1][4 * (u & 1) + cc], part);
              if constexpr (DK) dk[u >> 2][4 * (u & 3) + cc] = fmaf(dpij, t, dk[u >> 2][4 * (u & 3) + cc]);
            }
          }
          part += __shfl_xor(part, 32, 64);
          if (h == 0) xs[l31 * kXl + 16 * qsub + ii] = pr >= kl ? P.scale * part : 0.f;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if ((acc_row(r, h) >> 4) == qsub) sp[r] = xs[l31 * kXl + acc_row(r, h)];
      }
#pragma unroll
      for (int s2 = 0; s2 < 2 && DV; ++s2) {      // dv += S^T dO
        const bfx8 sf = pack_frag(sp, s2);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) dv[dt] = mfma32(tr_frag<D>(dot, 32 * qb + 16 * s2, 32 * dt, lane), sf, dv[dt]);
      }
    }
  }
  if constexpr (DV) store_acc_rows<D>(P.out2 + (row0 + kl) * P.out2_stride + (long)g * D, dv, 1.f, h);
  if constexpr (!DK) return;
  store_acc_rows<D>(P.out + (row0 + kl) * P.out_stride + (long)g * D, dk, 1.f, h);
  float* gk = A.gk + (row0 + kl) * ldc + (long)g * D;
#pragma unroll
  for (int u = 0; u < D / 8; ++u) {
    const bfx8 kp = ld_perm_frag(krow, u >> 1, h);
    float4 o;
    o.x = dk[u >> 2][4 * (u & 3) + 0] * (float)kp[4 * (u & 1) + 0];
    o.y = dk[u >> 2][4 * (u & 3) + 1] * (float)kp[4 * (u & 1) + 1];
    o.z = dk[u >> 2][4 * (u & 3) + 2] * (float)kp[4 * (u & 1) + 2];
    o.w = dk[u >> 2][4 * (u & 3) + 3] * (float)kp[4 * (u & 1) + 3];
    *reinterpret_cast<float4*>(gk + 8 * u + 4 * h) = o;
  }
}

// =============================================================================== the gate: z1 and Lambda
DLTB_DEV float log2_sigmoid(float zb) {
  const float u = zb * kLog2e;
  return fminf(u, 0.f) - __builtin_amdgcn_logf(1.f + ex2(-fabsf(u)));
}

__global__ __launch_bounds__(256) void lc_gate_fwd_kernel(const bf16_t* __restrict__ xn, const bf16_t* __restrict__ w1,
                                                          const bf16_t* __restrict__ w2, const float* __restrict__ bias,
                                                          float* __restrict__ z1, float* __restrict__ cum, int T, int d,
                                                          int R, int kvd, int D) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* w = reinterpret_cast<bf16_t*>(smem);                         // W1 [R][d]
  float* zs = reinterpret_cast<float*>(smem + (size_t)R * d * 2);      // z1 [kC][R]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long row0 = (long)blockIdx.y * T + (long)blockIdx.x * kC;
  for (int i = tid; i < R * d / 8; i += 256) reinterpret_cast<uint4*>(w)[i] = ld16<uint4>(w1 + 8 * i);
  __syncthreads();
  for (int rr = 0; rr < kC / 4; ++rr) {       // the row dots: 16 rows per wave, 8 rows of W1 per pass over a row
    const int r = (kC / 4) * wv + rr;
    const bf16_t* x = xn + (row0 + r) * d;
    for (int g0 = 0; g0 < R; g0 += 8) {
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      for (int col = lane * 8; col < d; col += 512) {
        float xv[8];
        unpack8(ld16<uint4>(x + col), xv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float wf[8];
          unpack8(*reinterpret_cast<const uint4*>(w + (size_t)(g0 + j) * d + col), wf);
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[j] = fmaf(xv[i], wf[i], acc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float zz = wave_sum(acc[j]);
        if (lane == 0) {
          z1[(row0 + r) * R + g0 + j] = zz;
          zs[r * R + g0 + j] = zz;
        }
      }
    }
  }
  __syncthreads();
  for (int ch = tid; ch < kvd; ch += 256) {   // one thread per channel: the 64 rows' z, l and prefix sum, rows in order
    float za[kC];
#pragma unroll
    for (int r = 0; r < kC; ++r) za[r] = 0.f;
    for (int r0 = 0; r0 < R; r0 += 8) {
      float wf[8];
      unpack8(ld16<uint4>(w2 + (long)ch * R + r0), wf);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < kC; ++r) za[r] = fmaf(zs[r * R + r0 + i], wf[i], za[r]);
    }
    const float bg = bias[ch / D];
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < kC; ++r) {
      s += log2_sigmoid(za[r] + bg);
      cum[(row0 + r) * kvd + ch] = s;
    }
  }
}

// =============================================================================== the gate's backward
// dl[s,c] = sum_{t >= s} (sum_{h in g} gq[t][h D + d] - gk[t][c]) along a row of T tokens; dz = dl (1 - a).  One
// workgroup per (64 channels, batch): thread = (channel, quarter); chunks are dealt to the quarters.
__global__ __launch_bounds__(256) void lc_gate_dl_kernel(const float* __restrict__ gq, const float* __restrict__ gk,
                                                         const float* __restrict__ z1, const bf16_t* __restrict__ w2,
                                                         const float* __restrict__ bias, float* __restrict__ dl,
                                                         float* __restrict__ dz, int T, int Hq, int Hkv, int D, int R) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nc = T / kC, kvd = Hkv * D, G = Hq / Hkv;
  float* tot = reinterpret_cast<float*>(smem);              // [nc][64] chunk totals, then the sum of the chunks after
  float* ws = tot + (size_t)nc * 64;                        // W2 slice [R][64]
  const int cl = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.y;
  const int ch = blockIdx.x * 64 + cl, g = ch / D, dd = ch % D;
  for (int i = threadIdx.x; i < 64 * R; i += 256) ws[(i % R) * 64 + i / R] = bf2f(w2[(long)(blockIdx.x * 64 + i / R) * R + i % R]);
  auto dL = [&](long row) {
    float v = 0.f;
    for (int hh = 0; hh < G; ++hh) v += gq[row * ((long)Hq * D) + (long)(g * G + hh) * D + dd];
    return v - gk[row * kvd + ch];
  };
  for (int c = wv; c < nc; c += 4) {
    const long r0 = (long)b * T + (long)c * kC;
    float s = 0.f;
    for (int r = kC - 1; r >= 0; --r) s += dL(r0 + r);
    tot[c * 64 + cl] = s;
  }
  __syncthreads();
  if (wv == 0) {
    float carry = 0.f;
    for (int c = nc - 1; c >= 0; --c) {
      const float v = tot[c * 64 + cl];
      tot[c * 64 + cl] = carry;
      carry += v;
    }
  }
  __syncthreads();
  const float bg = bias[g];
  for (int c = wv; c < nc; c += 4) {
    const long r0 = (long)b * T + (long)c * kC;
    float s = tot[c * 64 + cl];
    for (int r = kC - 1; r >= 0; --r) {
      const long row = r0 + r;
      s += dL(row);
      float z = 0.f;
      for (int i = 0; i < R; ++i) z = fmaf(z1[row * R + i], ws[i * 64 + cl], z);
      const float a = 1.f / (1.f + ex2(-(z + bg) * kLog2e));
      if (dl != nullptr) dl[row * kvd + ch] = s;
      dz[row * kvd + ch] = s * (1.f - a);
    }
  }
}

// dz1[t][r] = sum_c dz[t][c] W2[c][r], channels in index order; 4 rows per workgroup, thread = (row, r)
__global__ __launch_bounds__(256) void lc_gate_dz1_kernel(const float* __restrict__ dz, const bf16_t* __restrict__ w2,
                                                          float* __restrict__ dz1, long N, int kvd, int R) {
  const int r = threadIdx.x & 63;
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= N || r >= R) return;
  float s = 0.f;
  for (int c = 0; c < kvd; ++c) s = fmaf(dz[t * kvd + c], bf2f(w2[(long)c * R + r]), s);
  dz1[t * R + r] = s;
}

// dW2 = dz^T z1 in two stages.  Stage 1: workgroup (64 channels, slab of tokens), thread (channel, quarter q) holds the
// partials of r = q, q + 4, ...; stage 2 adds the slabs in index order and writes (or adds into) the 16-bit slot.
constexpr int kSlab = 512;
__global__ __launch_bounds__(256) void lc_gate_dw2_part_kernel(const float* __restrict__ dz, const float* __restrict__ z1,
                                                               float* __restrict__ part, long N, int kvd, int R) {
  const int cl = threadIdx.x & 63, q = threadIdx.x >> 6, ch = blockIdx.x * 64 + cl;
  const long t0 = (long)blockIdx.y * kSlab, t1 = t0 + kSlab < N ? t0 + kSlab : N;
  float acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.f;
  for (long t = t0; t < t1; ++t) {
    const float v = dz[t * kvd + ch];
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (q + 4 * k < R) acc[k] = fmaf(v, z1[t * R + q + 4 * k], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (q + 4 * k < R) part[((long)blockIdx.y * kvd + ch) * R + q + 4 * k] = acc[k];
}
__global__ __launch_bounds__(256) void lc_gate_dw2_fold_kernel(const float* __restrict__ part, bf16_t* __restrict__ dw2,
                                                               int slabs, long n, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int p = 0; p < slabs; ++p) s += part[(long)p * n + i];
  if (accumulate) s += bf2f(dw2[i]);
  dw2[i] = f2bf(s);
}

// =============================================================================== launches
template <int D, bool BWD>
void launch_state(const LcArgs& A, int nc, hipStream_t st) {
  allow_dynamic_lds<lc_state_kernel<D, BWD>>(cstate_lds<D>());
  hipLaunchKernelGGL((lc_state_kernel<D, BWD>), dim3(nc, A.a.Hkv, A.a.B), dim3(256), cstate_lds<D>(), st, A);
}
template <int D>
void launch_scan(const LcArgs& A, int nc, int reverse, hipStream_t st) {
  hipLaunchKernelGGL(lc_scan_kernel, dim3(D * D / 256, A.a.Hkv, A.a.B), dim3(256), 0, st, A.a.local, A.a.state, A.cum,
                     nc, D, A.a.T, reverse);
}
template <int D, bool BWD>
void launch_qside(const LcArgs& A, int nc, hipStream_t st) {
  allow_dynamic_lds<lc_qside_kernel<D, BWD>>(cside_lds<D>());
  hipLaunchKernelGGL((lc_qside_kernel<D, BWD>), dim3(nc, A.a.Hq, A.a.B), dim3(128), cside_lds<D>(), st, A);
}

template <int D>
void fwd_d(const LcArgs& A, hipStream_t st) {
  const int nc = A.a.T / kC;
  launch_state<D, false>(A, nc, st);
  launch_scan<D>(A, nc, 0, st);
  launch_qside<D, false>(A, nc, st);
}

template <int D>
void bwd_d(LcArgs A, bf16_t* dq, bf16_t* dk, bf16_t* dv, long dqs, long dks, long dvs, hipStream_t st) {
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
  if constexpr (D == 64) {
    allow_dynamic_lds<lc_kside_kernel<D, 0>>(cside_lds<D>());
    hipLaunchKernelGGL((lc_kside_kernel<D, 0>), dim3(nc, A.a.Hkv, A.a.B), dim3(128), cside_lds<D>(), st, A);
  } else {
    allow_dynamic_lds<lc_kside_kernel<D, 1>>(cside_lds<D>());
    hipLaunchKernelGGL((lc_kside_kernel<D, 1>), dim3(nc, A.a.Hkv, A.a.B), dim3(128), cside_lds<D>(), st, A);
    allow_dynamic_lds<lc_kside_kernel<D, 2>>(cside_lds<D>());
    hipLaunchKernelGGL((lc_kside_kernel<D, 2>), dim3(nc, A.a.Hkv, A.a.B), dim3(128), cside_lds<D>(), st, A);
  }
}

}  // namespace

// R a multiple of 8 up to 64, W1 and the chunk's z1 within 160 KB of LDS; kv_dim a multiple of 64 (D is 64 or 128);
// the backward's chunk totals and W2 slice within 160 KB
bool dltb_linear_attn_chgate_supported(int T, int d, int R, int kvd) {
  return T > 0 && T % kC == 0 && R >= 8 && R <= 64 && R % 8 == 0 && d >= 8 && d % 8 == 0 && kvd > 0 && kvd % 64 == 0 &&
         (long)R * d * 2 + (long)kC * R * 4 <= kGateLds && (long)(T / kC) * 64 * 4 + (long)R * 64 * 4 <= kGateLds;
}
int dltb_linear_attn_chgate_slabs(long N) { return (int)((N + kSlab - 1) / kSlab); }

void dltb_linear_attn_chgate_gate_fwd(const void* xn, const void* w1, const void* w2, const float* bias, float* z1,
                                      float* cum, int B, int T, int d, int R, int kvd, int D, hipStream_t st) {
  allow_dynamic_lds<lc_gate_fwd_kernel>(kGateLds);
  hipLaunchKernelGGL(lc_gate_fwd_kernel, dim3(T / kC, B), dim3(256), (size_t)R * d * 2 + (size_t)kC * R * 4, st,
                     (const bf16_t*)xn, (const bf16_t*)w1, (const bf16_t*)w2, bias, z1, cum, T, d, R, kvd, D);
}

void dltb_linear_attn_chgate_gate_bwd(const float* gq, const float* gk, const float* z1, const void* w2,
                                      const float* bias, float* dl, float* dz, float* dz1, float* part, void* dw2,
                                      int accumulate, int B, int T, int Hq, int Hkv, int D, int R, hipStream_t st) {
  const int kvd = Hkv * D;
  const long N = (long)B * T;
  allow_dynamic_lds<lc_gate_dl_kernel>(kGateLds);
  hipLaunchKernelGGL(lc_gate_dl_kernel, dim3(kvd / 64, B), dim3(256), (size_t)(T / kC) * 64 * 4 + (size_t)R * 64 * 4, st,
                     gq, gk, z1, (const bf16_t*)w2, bias, dl, dz, T, Hq, Hkv, D, R);
  hipLaunchKernelGGL(lc_gate_dz1_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, dz, (const bf16_t*)w2, dz1, N,
                     kvd, R);
  if (dw2 == nullptr) return;
  const int slabs = dltb_linear_attn_chgate_slabs(N);
  hipLaunchKernelGGL(lc_gate_dw2_part_kernel, dim3(kvd / 64, slabs), dim3(256), 0, st, dz, z1, part, N, kvd, R);
  const long n = (long)kvd * R;
  hipLaunchKernelGGL(lc_gate_dw2_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, (bf16_t*)dw2,
                     slabs, n, accumulate);
}

void dltb_linear_attn_chgate_fwd(const void* q, const void* k, const void* v, void* o, const float* cum, float* local,
                                 void* state, long qs, long ks, long vs, long os, int B, int T, int Hq, int Hkv, int D,
                                 float scale, hipStream_t st) {
  LcArgs A = {};
  LaArgs& P = A.a;
  A.cum = cum;
  P.q = (const bf16_t*)q; P.k = (const bf16_t*)k; P.v = (const bf16_t*)v;
  P.out = (bf16_t*)o; P.local = local; P.state = (bf16_t*)state;
  P.q_stride = qs; P.k_stride = ks; P.v_stride = vs; P.out_stride = os;
  P.B = B; P.T = T; P.Hq = Hq; P.Hkv = Hkv; P.scale = scale;
  if (D == 64) fwd_d<64>(A, st);
  else fwd_d<128>(A, st);
}

void dltb_linear_attn_chgate_bwd(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk,
                                 void* dv, const float* cum, float* gq, float* gk, float* local, void* state, long qs,
                                 long ks, long vs, long dos, long dqs, long dks, long dvs, int B, int T, int Hq, int Hkv,
                                 int D, float scale, hipStream_t st) {
  LcArgs A = {};
  LaArgs& P = A.a;
  A.cum = cum; A.gq = gq; A.gk = gk;
  P.q = (const bf16_t*)q; P.k = (const bf16_t*)k; P.v = (const bf16_t*)v; P.dout = (const bf16_t*)dout;
  P.local = local; P.state = (bf16_t*)state;
  P.q_stride = qs; P.k_stride = ks; P.v_stride = vs; P.do_stride = dos;
  P.B = B; P.T = T; P.Hq = Hq; P.Hkv = Hkv; P.scale = scale;
  if (D == 64) bwd_d<64>(A, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, dqs, dks, dvs, st);
  else bwd_d<128>(A, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, dqs, dks, dvs, st);
}
