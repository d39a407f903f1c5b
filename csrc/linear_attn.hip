// Chunked fixed-decay linear attention (the RetNet / lightning form) for gfx950 (CDNA4), 16-bit in / fp32 accumulate.
//
//   o[i] = r[g,i] * scale * sum_{j <= i} gamma_g^(i-j) (q[i] . k[j]) v[j],   r[g,i] = sqrt((1 - gamma_g) / (1 - gamma_g^(i+1)))
//
// for query head h of KV group g = h / (Hq / Hkv); the decays arrive as log2(gamma) [Hkv] fp32.  No softmax, no lse.
// Layout as in attention.hip: token-major rows with head h at column h * D, so the kernels read the fused qkv buffer
// and write dq | dk | dv straight into dqkv.
//
// T is cut into chunks of C = 64 rows.  With a = i mod C, the state S_c = sum_{j < (c+1) C} gamma^((c+1) C - 1 - j) k_j^T v_j
// ([D, D], one per KV head) and rs = r * scale:
//   forward   1. state<fwd>   local_c = K_c^T (gamma^(C-1-b) . V_c)              grid (chunks, Hkv, B), fp32 out
//             2. scan         S_c = gamma^C S_{c-1} + local_c along the chunks    one thread per state element, fixed
//                             order, no atomics; writes S_{c-1} rounded to 16 bits as chunk c's MFMA operand
//             3. qside<fwd>   o_i = rs_i (gamma^(a+1) q_i S_{c-1} + sum_{b <= a} gamma^(a-b) (q_i . k_b) v_b)
//   backward  the states are rebuilt (1, 2), then with do'_i = rs_i do_i
//             4. qside<bwd>   dq_i = rs_i (gamma^(a+1) do_i S_{c-1}^T + sum_{b <= a} gamma^(a-b) (do_i . v_b) k_b)
//             5. state<bwd>   dlocal_c = sum_{h in group} Q_c^T (rs gamma^(a+1) . dO_c), heads summed in index order
//             6. scan, reversed: dS_{c-1} = gamma^C dS_c + dlocal_c
//             7. kside        dk_b = gamma^(C-1-b) dS_c v_b + sum_h sum_{a >= b} rs_a gamma^(a-b) (do_a . v_b) q_a
//                             dv_b = gamma^(C-1-b) k_b dS_c + sum_h sum_{a >= b} rs_a gamma^(a-b) (q_a . k_b) do_a
// Every kernel is parallel over the chunks; only the elementwise scan walks T, T / 64 fused multiply-adds per thread.
//
// MFMA: v_mfma_f32_32x32x16 throughout.  qside / kside: 2 waves per workgroup, 32 rows each, the row on the LANE
// (the products are formed transposed, as in attention.hip), so the decay mask, the row normaliser and the inter-chunk
// decay are per-lane scalars; the score tile goes from its accumulator registers into the next MFMA as the B operand
// and the other operand comes from LDS by ds_read_b64_tr_b16.  The wave's own rows (q or dO; k and v in kside) are
// read from global memory as fragments once, in the row order and -- where a transposed state read needs it -- in the
// accumulator's permuted k order.  state: 4 waves, the [D, D] tile split by 32-column blocks.
//
// Rounding: a decayed score tile and a state are rounded to the 16-bit format once, where they become MFMA operands;
// so is the decayed V (dO) operand of the state products.  Each output is rounded once.  Every decay factor is exp2
// of a non-positive fp32 argument; 1 - gamma^n is formed as -expm1 so the slowest decays keep their precision.
//
// The argument block and the tile / fragment helpers live in linear_attn_common.h, which the gated kernels of
// linear_attn_gate.hip share.
#include "linear_attn_common.h"

namespace {

// rs = r * scale of global position i
DLTB_DEV float row_norm(float l2g, int i, float scale) {
  const float num = expm1f(l2g * kLn2), den = expm1f(l2g * (float)(i + 1) * kLn2);   // both negative
  return sqrtf(num / den) * scale;
}
DLTB_DEV float decay(float l2g, int n) { return __builtin_amdgcn_exp2f(l2g * (float)n); }   // n >= 0

// =============================================================================== chunk-local states
// fwd: local[d][e] = sum_b K[b][d] (gamma^(C-1-b) V[b][e]);  bwd: sum over the group's heads of
// sum_a Q[a][d] (rs_a gamma^(a+1) dO[a][e]).  4 waves; D = 128: wave w owns columns 32 w .. +31 of all four row
// blocks, D = 64: one 32 x 32 block each.
template <int D, bool BWD>
__global__ __launch_bounds__(256) void la_state_kernel(LaArgs P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* xt = smem;
  char* yt = smem + kC * D * 2;
  float* fac = reinterpret_cast<float*>(smem + 2 * kC * D * 2);
  constexpr int NDB = D == 128 ? 4 : 1;
  const int c = blockIdx.x, g = blockIdx.y, b = blockIdx.z, nc = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5;
  const int eb = D == 128 ? w : (w & 1), db0 = D == 128 ? 0 : (w >> 1);
  const int G = P.Hq / P.Hkv;
  const float l2g = P.l2g[g];
  if (tid < kC)
    fac[tid] = BWD ? row_norm(l2g, c * kC + tid, P.scale) * decay(l2g, tid + 1) : decay(l2g, kC - 1 - tid);
  f32x16 acc[NDB];
#pragma unroll
  for (int n = 0; n < NDB; ++n) acc[n] = zero16();
  const long row0 = (long)b * P.T + (long)c * kC;
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
// state[c] = the running state BEFORE chunk c joins it, rounded to 16 bits; s = gamma^C s + local[c] in fp32.
// reverse: the chunks from last to first (the state gradients).
__global__ __launch_bounds__(256) void la_scan_kernel(const float* __restrict__ local, bf16_t* __restrict__ state,
                                                      const float* __restrict__ l2g, int nc, int DD, int reverse) {
  const int idx = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, b = blockIdx.z, Hkv = gridDim.y;
  const long base = ((long)b * Hkv + g) * nc * (long)DD + idx;
  const float gC = decay(l2g[g], kC);
  float s = 0.f;
  for (int i = 0; i < nc; ++i) {
    const long at = base + (long)(reverse ? nc - 1 - i : i) * DD;
    state[at] = f2bf(s);
    s = fmaf(gC, s, local[at]);
  }
}

// =============================================================================== query side: o (fwd) and dq (bwd)
// Lane = query row.  fwd: scores against K, values V, the state read transposed; bwd: scores dO . V, values K, the
// state read by rows.  acc^T[col][query]: the inter-chunk product first, times gamma^(a+1), then the masked
// intra-chunk blocks, and rs on the way out.
template <int D, bool BWD>
__global__ __launch_bounds__(128) void la_qside_kernel(LaArgs P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sc = smem;                    // score operand rows (fwd K, bwd V)
  char* vl = smem + kC * D * 2;       // value rows (fwd V, bwd K)
  char* st = smem + 2 * kC * D * 2;   // S_{c-1} [D][D]
  const int c = blockIdx.x, hq = blockIdx.y, b = blockIdx.z, nc = gridDim.x;
  const int G = P.Hq / P.Hkv, g = hq / G;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ql = 32 * w + (lane & 31);
  const long row0 = (long)b * P.T + (long)c * kC;
  const float l2g = P.l2g[g];
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
  const float dq0 = decay(l2g, ql + 1);
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) acc[dt] *= dq0;
  for (int kb = 0; kb <= w; ++kb) {
    f32x16 p = zero16();
#pragma unroll
    for (int s = 0; s < D / 16; ++s) p = mfma32(row_frag<D>(sc, 32 * kb + (lane & 31), 2 * s + h), xr[s], p);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = 32 * kb + acc_row(r, h);
      p[r] = key <= ql ? p[r] * decay(l2g, ql - key) : 0.f;
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const bfx8 pf = pack_frag(p, s2);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) acc[dt] = mfma32(tr_frag<D>(vl, 32 * kb + 16 * s2, 32 * dt, lane), pf, acc[dt]);
    }
  }
  store_acc_rows<D>(P.out + (row0 + ql) * P.out_stride + (long)hq * D, acc, row_norm(l2g, c * kC + ql, P.scale), h);
}

// =============================================================================== key side: dk and dv
// Lane = key row; the group's query heads in index order, one Q / dO tile pair at a time.
template <int D>
__global__ __launch_bounds__(128) void la_kside_kernel(LaArgs P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qt = smem;
  char* dot = smem + kC * D * 2;
  char* ds = smem + 2 * kC * D * 2;   // dS_c [D][D]
  float* rsf = reinterpret_cast<float*>(smem + 2 * kC * D * 2 + D * D * 2);
  const int c = blockIdx.x, g = blockIdx.y, b = blockIdx.z, nc = gridDim.x;
  const int G = P.Hq / P.Hkv;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = 32 * w + (lane & 31);
  const long row0 = (long)b * P.T + (long)c * kC;
  const float l2g = P.l2g[g];
  const bf16_t* krow = P.k + (row0 + kl) * P.k_stride + (long)g * D;
  const bf16_t* vrow = P.v + (row0 + kl) * P.v_stride + (long)g * D;
  bfx8 kr[D / 16], vr[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    kr[s] = ld_row_frag(krow, s, h);
    vr[s] = ld_row_frag(vrow, s, h);
  }
  if (tid < kC) rsf[tid] = row_norm(l2g, c * kC + tid, P.scale);
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
  const float dk0 = decay(l2g, kC - 1 - kl);
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
        const float f = i >= kl ? rsf[i] * decay(l2g, i - kl) : 0.f;
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
}

// =============================================================================== launches
template <int D, bool BWD>
void launch_state(const LaArgs& P, int nc, hipStream_t st) {
  allow_dynamic_lds<la_state_kernel<D, BWD>>(state_lds<D>());
  hipLaunchKernelGGL((la_state_kernel<D, BWD>), dim3(nc, P.Hkv, P.B), dim3(256), state_lds<D>(), st, P);
}
template <int D>
void launch_scan(const LaArgs& P, int nc, int reverse, hipStream_t st) {
  hipLaunchKernelGGL(la_scan_kernel, dim3(D * D / 256, P.Hkv, P.B), dim3(256), 0, st, P.local, P.state, P.l2g, nc,
                     D * D, reverse);
}
template <int D, bool BWD>
void launch_qside(const LaArgs& P, int nc, hipStream_t st) {
  allow_dynamic_lds<la_qside_kernel<D, BWD>>(side_lds<D>());
  hipLaunchKernelGGL((la_qside_kernel<D, BWD>), dim3(nc, P.Hq, P.B), dim3(128), side_lds<D>(), st, P);
}

template <int D>
void fwd_d(LaArgs P, hipStream_t st) {
  const int nc = P.T / kC;
  launch_state<D, false>(P, nc, st);
  launch_scan<D>(P, nc, 0, st);
  launch_qside<D, false>(P, nc, st);
}

template <int D>
void bwd_d(LaArgs P, bf16_t* dq, bf16_t* dk, bf16_t* dv, long dqs, long dks, long dvs, hipStream_t st) {
  const int nc = P.T / kC;
  launch_state<D, false>(P, nc, st);          // the forward's states, rebuilt
  launch_scan<D>(P, nc, 0, st);
  P.out = dq;
  P.out_stride = dqs;
  launch_qside<D, true>(P, nc, st);
  launch_state<D, true>(P, nc, st);           // the state gradients, in the same two buffers
  launch_scan<D>(P, nc, 1, st);
  P.out = dk;
  P.out_stride = dks;
  P.out2 = dv;
  P.out2_stride = dvs;
  allow_dynamic_lds<la_kside_kernel<D>>(side_lds<D>());
  hipLaunchKernelGGL(la_kside_kernel<D>, dim3(nc, P.Hkv, P.B), dim3(128), side_lds<D>(), st, P);
}

}  // namespace

int dltb_linear_attn_chunk() { return kC; }
bool dltb_linear_attn_supported(int D, int T) { return (D == 64 || D == 128) && T > 0 && T % kC == 0; }

void dltb_linear_attn_fwd(const void* q, const void* k, const void* v, void* o, const float* l2g, float* local,
                          void* state, long qs, long ks, long vs, long os, int B, int T, int Hq, int Hkv, int D,
                          float scale, hipStream_t st) {
  LaArgs P = {};
  P.q = (const bf16_t*)q; P.k = (const bf16_t*)k; P.v = (const bf16_t*)v;
  P.out = (bf16_t*)o; P.l2g = l2g; P.local = local; P.state = (bf16_t*)state;
  P.q_stride = qs; P.k_stride = ks; P.v_stride = vs; P.out_stride = os;
  P.B = B; P.T = T; P.Hq = Hq; P.Hkv = Hkv; P.scale = scale;
  if (D == 64) fwd_d<64>(P, st);
  else fwd_d<128>(P, st);
}

void dltb_linear_attn_bwd(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk, void* dv,
                          const float* l2g, float* local, void* state, long qs, long ks, long vs, long dos, long dqs,
                          long dks, long dvs, int B, int T, int Hq, int Hkv, int D, float scale, hipStream_t st) {
  LaArgs P = {};
  P.q = (const bf16_t*)q; P.k = (const bf16_t*)k; P.v = (const bf16_t*)v; P.dout = (const bf16_t*)dout;
  P.l2g = l2g; P.local = local; P.state = (bf16_t*)state;
  P.q_stride = qs; P.k_stride = ks; P.v_stride = vs; P.do_stride = dos;
  P.B = B; P.T = T; P.Hq = Hq; P.Hkv = Hkv; P.scale = scale;
  if (D == 64) bwd_d<64>(P, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, dqs, dks, dvs, st);
  else bwd_d<128>(P, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, dqs, dks, dvs, st);
}
