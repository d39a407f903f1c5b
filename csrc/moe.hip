// Top-k mixture-of-experts routing with a fixed expert capacity (models/mistral.py, n_experts).
//
// Every shape is static (N token rows, E experts, K choices per token, C slots per expert), nothing is
// atomic and nothing depends on the dispatch order, so a captured micro-step replays bit for bit:
//   moe_route         logits = h Wr^T in fp32 (one wave per RR token rows), the K largest per row (ties to the
//                     lower expert), gates = softmax over the K chosen logits
//   moe_assign        slot of every (token, choice) in row-major order: per-wave expert histograms (ballots),
//                     one block scanning them per expert, then positions; position >= C is dropped (-1).
//                     Writes the inverse too: src / src_k of every slot (-1 when the slot stays empty)
//   moe_assign_dropless  the same order without a capacity: expert e's assignments fill a 128-aligned segment of
//                     one packed [R] row space (R static), the bounds written to offsets [E + 1] for the grouped
//                     GEMMs (gemm_grouped.hip); nothing is dropped, unreached rows get src = -1
//   moe_dispatch      xe[slot] = h[src[slot]]; empty slots are zero rows
//   moe_combine       m[n] = sum_k gate[n, k] ye[slot[n, k]], fp32 in k order, rounded once
//   moe_combine_bwd   dye[slot] = gate dm[src], dgate = <dm, ye[slot]>, and the softmax backward into a dense
//                     dlogits row (one pass over dm and ye; empty slots get zero rows)
//   moe_dispatch_bwd  dh[n] = sum_k dxe[slot[n, k]] + sum_e dlogits[n, e] Wr[e], fp32, rounded once
//   moe_router_wgrad  dWr = dlogits^T h: fp32 row-range partials per expert (only rows with a non-zero dlogit
//                     are read), then colreduce_multi's fixed-order sum into the gradient slot; a dense form
//                     for a dlogits without zeros (8 experts per pass over h), same partials and fold
//   moe_aux_fwd       load-balancing loss and router z-loss of the logits and the counts (fixed-order partials)
//   moe_aux_bwd       their gradient added to the dense dlogits, softmax recomputed from the kept log-sum-exp
// Rows are moved as 16-byte chunks, lane -> chunk, chunks strided by the wave; index arrays are trusted only
// as far as a bound check (an index outside its range counts as dropped / empty).
#include "common.h"
#include "launchers.h"

namespace {

constexpr int RR = 4;       // token rows per wave in the router: Wr is read once per RR rows
constexpr int KMAX = 4;     // top-k at most

DLTB_DEV uint4 zero16() { return make_uint4(0u, 0u, 0u, 0u); }

__global__ __launch_bounds__(256) void moe_route_kernel(const bf16_t* __restrict__ h, const bf16_t* __restrict__ wr,
                                                        int* __restrict__ expert, float* __restrict__ gate,
                                                        float* __restrict__ logits, int N, int d, int E, int K) {
  const int lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RR;
  if (n0 >= N) return;                                   // wave-uniform; the kernel has no block barrier
  DLTB_DCHECK(d % 8 == 0 && E >= 1 && E <= 64 && K >= 1 && K <= KMAX && K <= E);
  const int nch = d >> 3;
  float lg[RR];                                          // lane e: logit e of row n0 + r
#pragma unroll
  for (int r = 0; r < RR; ++r) lg[r] = -INFINITY;
  for (int e0 = 0; e0 < E; e0 += 8) {
    float acc[RR][8];
#pragma unroll
    for (int r = 0; r < RR; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
    for (int c = lane; c < nch; c += 64) {
      float hv[RR][8];
#pragma unroll
      for (int r = 0; r < RR; ++r)
        unpack8(n0 + r < N ? ld16<uint4>(h + (size_t)(n0 + r) * d + c * 8) : zero16(), hv[r]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (e0 + j < E) {
          float wv[8];
          unpack8(ld16<uint4>(wr + (size_t)(e0 + j) * d + c * 8), wv);
#pragma unroll
          for (int r = 0; r < RR; ++r)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[r][j] = fmaf(hv[r][i], wv[i], acc[r][j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        const float t = wave_sum(acc[r][j]);             // xor butterfly: the same bits in every lane
        if (lane == e0 + j && e0 + j < E) lg[r] = t;
      }
  }
#pragma unroll
  for (int r = 0; r < RR; ++r) {
    const int n = n0 + r;
    if (n >= N) break;
    const float v = lg[r];
    if (lane < E) logits[(size_t)n * E + lane] = v;
    bool taken = lane >= E;
    float sel[KMAX];
    int seli[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      sel[k] = 0.f;
      seli[k] = 0;
      if (k < K) {
        const float cand = taken ? -INFINITY : v;
        const float mx = wave_max(cand);
        unsigned long long b = __ballot(!taken && cand == mx);
        if (b == 0ull) b = __ballot(!taken);             // only NaN logits left: the lowest free expert (K <= E)
        const int idx = __ffsll((long long)b) - 1;       // ties: the lower expert index
        sel[k] = __shfl(v, idx, 64);
        seli[k] = idx;
        if (lane == idx) taken = true;
      }
    }
    float ex[KMAX], sum = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      ex[k] = k < K ? expf(sel[k] - sel[0]) : 0.f;
      if (k < K) sum += ex[k];
    }
    float g = 0.f;
    int ei = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (lane == k) {
        g = ex[k] / sum;
        ei = seli[k];
      }
    if (lane < K) {
      expert[(size_t)n * K + lane] = ei;
      gate[(size_t)n * K + lane] = g;
    }
  }
}

// ---------------------------------------------------------------- slot assignment
// wave w holds assignments [64 w, 64 w + 64) of the row-major (token, choice) list
__global__ __launch_bounds__(256) void moe_hist_kernel(const int* __restrict__ expert, int* __restrict__ wavecnt,
                                                       int NK, int E) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w * 64 >= NK) return;
  const int i = w * 64 + lane;
  const int e = i < NK ? expert[i] : -1;
  int mine = 0;
  for (int x = 0; x < E; ++x) {
    const int c = __popcll(__ballot(e == x));
    if (lane == x) mine = c;
  }
  if (lane < E) wavecnt[(size_t)w * E + lane] = mine;
}

// one block: exclusive scan of wavecnt over the waves, per expert (thread = (segment, expert), 16 segments)
__global__ __launch_bounds__(1024) void moe_scan_kernel(const int* __restrict__ wavecnt, int* __restrict__ base,
                                                        int* __restrict__ counts, int W, int E) {
  __shared__ int tot[16][64];
  const int e = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int per = (W + 15) / 16;
  const int w0 = seg * per, w1 = min(W, w0 + per);
  int t = 0;
  if (e < E)
    for (int w = w0; w < w1; ++w) t += wavecnt[(size_t)w * E + e];
  tot[seg][e] = t;
  __syncthreads();
  if (e >= E) return;
  int run = 0;
  for (int s = 0; s < seg; ++s) run += tot[s][e];
  if (seg == 15) counts[e] = run + t;
  for (int w = w0; w < w1; ++w) {
    const int c = wavecnt[(size_t)w * E + e];
    base[(size_t)w * E + e] = run;
    run += c;
  }
}

__global__ __launch_bounds__(256) void moe_place_kernel(const int* __restrict__ expert, const int* __restrict__ base,
                                                        const int* __restrict__ counts, int* __restrict__ slot,
                                                        int* __restrict__ src, int* __restrict__ src_k, int NK, int K,
                                                        int E, int C) {
  const int lane = threadIdx.x & 63;
  // slots no assignment reaches: position >= the expert's count (disjoint from the slots written below)
  const int rows = E * C;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < rows; g += gridDim.x * 256)
    if (g % C >= counts[g / C]) {
      src[g] = -1;
      src_k[g] = -1;
    }
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w * 64 >= NK) return;
  const int i = w * 64 + lane;
  const int e = i < NK ? expert[i] : -1;
  int rank = 0;
  for (int x = 0; x < E; ++x) {
    const unsigned long long b = __ballot(e == x);
    if (e == x) rank = __popcll(b & ((1ull << lane) - 1ull));
  }
  if (i >= NK) return;
  int s = -1;
  if ((unsigned)e < (unsigned)E) {
    const int p = base[(size_t)w * E + e] + rank;
    if (p < C) {
      s = e * C + p;
      src[s] = i / K;
      src_k[s] = i % K;
    }
  }
  slot[i] = s;
}

// Dropless placement into the packed layout: expert e owns the rows [offsets[e], offsets[e + 1]), offsets = the
// exclusive prefix sum of the counts rounded up to SEG rows, and assignment (n, k) at position p of its expert gets
// row offsets[e] + p, whatever p is.  Every block rebuilds the E + 1 offsets from the counts in LDS (block 0 writes
// them out); rows [0, rows) no assignment reaches -- a segment's padding and the tail past offsets[E] -- get -1.
constexpr int SEG = 128;    // segment granularity: the grouped GEMMs' tile rows (gemm_grouped.hip)

__global__ __launch_bounds__(256) void moe_place_dropless_kernel(const int* __restrict__ expert,
                                                                 const int* __restrict__ base,
                                                                 const int* __restrict__ counts, int* __restrict__ slot,
                                                                 int* __restrict__ src, int* __restrict__ src_k,
                                                                 int* __restrict__ offsets, int NK, int K, int E,
                                                                 int rows) {
  __shared__ int off[65], cnt[64];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x <= E) {                      // E <= 64 serial adds per thread: the scan of a 64-entry table
    int run = 0;
    for (int x = 0; x < (int)threadIdx.x; ++x) run += (counts[x] + SEG - 1) / SEG * SEG;
    off[threadIdx.x] = run;
    if (threadIdx.x < E) cnt[threadIdx.x] = counts[threadIdx.x];
    if (blockIdx.x == 0) offsets[threadIdx.x] = run;
  }
  __syncthreads();
  DLTB_DCHECK(off[E] <= rows);
  for (int g = blockIdx.x * 256 + threadIdx.x; g < rows; g += gridDim.x * 256) {
    bool filled = false;                       // disjoint from the rows written below
    for (int x = 0; x < E; ++x) filled |= g >= off[x] && g < off[x] + cnt[x];
    if (!filled) {
      src[g] = -1;
      src_k[g] = -1;
    }
  }
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w * 64 >= NK) return;
  const int i = w * 64 + lane;
  const int e = i < NK ? expert[i] : -1;
  int rank = 0;
  for (int x = 0; x < E; ++x) {
    const unsigned long long b = __ballot(e == x);
    if (e == x) rank = __popcll(b & ((1ull << lane) - 1ull));
  }
  if (i >= NK) return;
  int s = -1;
  if ((unsigned)e < (unsigned)E) {
    const int p = off[e] + base[(size_t)w * E + e] + rank;
    if (p < rows) {                            // always, for counts that sum to NK (rows >= NK + 127 E)
      s = p;
      src[s] = i / K;
      src_k[s] = i % K;
    }
  }
  slot[i] = s;
}

// ---------------------------------------------------------------- row movers (one wave per row)
__global__ __launch_bounds__(256) void moe_dispatch_kernel(const bf16_t* __restrict__ h, const int* __restrict__ src,
                                                           bf16_t* __restrict__ xe, int rows, int N, int d) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= rows) return;
  const int n = src[s];
  const bool valid = (unsigned)n < (unsigned)N;
  const int nch = d >> 3;
  for (int c = lane; c < nch; c += 64) {
    const uint4 v = valid ? ld16<uint4>(h + (size_t)n * d + c * 8) : zero16();
    *reinterpret_cast<uint4*>(xe + (size_t)s * d + c * 8) = v;
  }
}

__global__ __launch_bounds__(256) void moe_combine_kernel(const bf16_t* __restrict__ ye, const int* __restrict__ slot,
                                                          const float* __restrict__ gate, bf16_t* __restrict__ m,
                                                          int N, int d, int K, int rows) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  int sk[KMAX];
  float gk[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    sk[k] = k < K ? slot[(size_t)n * K + k] : -1;
    gk[k] = k < K ? gate[(size_t)n * K + k] : 0.f;
    if ((unsigned)sk[k] >= (unsigned)rows) sk[k] = -1;
  }
  const int nch = d >> 3;
  for (int c = lane; c < nch; c += 64) {
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (sk[k] >= 0) {
        float yv[8];
        unpack8(ld16<uint4>(ye + (size_t)sk[k] * d + c * 8), yv);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(gk[k], yv[i], acc[i]);
      }
    *reinterpret_cast<uint4*>(m + (size_t)n * d + c * 8) = pack8(acc);
  }
}

// waves [0, N): one token each; waves [N, N + rows): one slot each, zeroing the rows of empty slots
__global__ __launch_bounds__(256) void moe_combine_bwd_kernel(const bf16_t* __restrict__ dm, const bf16_t* __restrict__ ye,
                                                              const int* __restrict__ slot, const int* __restrict__ src,
                                                              const int* __restrict__ expert,
                                                              const float* __restrict__ gate, bf16_t* __restrict__ dye,
                                                              float* __restrict__ dgate, float* __restrict__ dlogits,
                                                              int N, int d, int E, int K, int rows) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nch = d >> 3;
  if (w >= N) {
    const int s = w - N;
    if (s >= rows || (unsigned)src[s] < (unsigned)N) return;
    for (int c = lane; c < nch; c += 64) *reinterpret_cast<uint4*>(dye + (size_t)s * d + c * 8) = zero16();
    return;
  }
  const int n = w;
  int sk[KMAX], ek[KMAX];
  float gk[KMAX], dg[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    sk[k] = k < K ? slot[(size_t)n * K + k] : -1;
    ek[k] = k < K ? expert[(size_t)n * K + k] : -1;
    gk[k] = k < K ? gate[(size_t)n * K + k] : 0.f;
    if ((unsigned)sk[k] >= (unsigned)rows) sk[k] = -1;
    dg[k] = 0.f;
  }
  for (int c = lane; c < nch; c += 64) {
    float dv[8];
    unpack8(ld16<uint4>(dm + (size_t)n * d + c * 8), dv);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (sk[k] >= 0) {
        float yv[8], o[8];
        unpack8(ld16<uint4>(ye + (size_t)sk[k] * d + c * 8), yv);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          dg[k] = fmaf(dv[i], yv[i], dg[k]);
          o[i] = gk[k] * dv[i];
        }
        *reinterpret_cast<uint4*>(dye + (size_t)sk[k] * d + c * 8) = pack8(o);
      }
  }
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    dg[k] = sk[k] >= 0 ? wave_sum(dg[k]) : 0.f;          // sk is wave-uniform
    t = fmaf(gk[k], dg[k], t);
  }
  float mine = 0.f, dl = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (lane == k) mine = dg[k];
    if (k < K && lane == ek[k]) dl = gk[k] * (dg[k] - t);
  }
  if (lane < K) dgate[(size_t)n * K + lane] = mine;
  if (lane < E) dlogits[(size_t)n * E + lane] = dl;
}

__global__ __launch_bounds__(256) void moe_dispatch_bwd_kernel(const bf16_t* __restrict__ dxe, const int* __restrict__ slot,
                                                               const float* __restrict__ dlogits,
                                                               const bf16_t* __restrict__ wr, bf16_t* __restrict__ dh,
                                                               int N, int d, int E, int K, int rows) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  int sk[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    sk[k] = k < K ? slot[(size_t)n * K + k] : -1;
    if ((unsigned)sk[k] >= (unsigned)rows) sk[k] = -1;
  }
  // the experts this row's router gradient touches (all 64 lanes are active here; inside the chunk loop below only
  // the lanes with a chunk are, so a value is read there by a wave-uniform load, never from another lane)
  const float* __restrict__ dlrow = dlogits + (size_t)n * E;
  const unsigned long long nz = __ballot(lane < E && dlrow[lane < E ? lane : 0] != 0.f);
  const int nch = d >> 3;
  for (int c = lane; c < nch; c += 64) {
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (sk[k] >= 0) {
        float xv[8];
        unpack8(ld16<uint4>(dxe + (size_t)sk[k] * d + c * 8), xv);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += xv[i];
      }
    for (unsigned long long mm = nz; mm != 0ull; mm &= mm - 1ull) {     // ascending expert index
      const int e = __ffsll((long long)mm) - 1;
      const float v = dlrow[e];
      float wv[8];
      unpack8(ld16<uint4>(wr + (size_t)e * d + c * 8), wv);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(v, wv[i], acc[i]);
    }
    *reinterpret_cast<uint4*>(dh + (size_t)n * d + c * 8) = pack8(acc);
  }
}

// part[by][e][d]: the rows [by rps, +rps) of dlogits[:, e]^T h; block = 512 columns, 4 waves on every 4th row.
// A wave looks at 64 of its rows' dlogits at once and reads only the h rows whose dlogit is not zero.
__global__ __launch_bounds__(256) void moe_router_wgrad_kernel(const float* __restrict__ dlogits,
                                                               const bf16_t* __restrict__ h, float* __restrict__ part,
                                                               int N, int d, int E, int P) {
  __shared__ __attribute__((aligned(16))) float red[4][512];
  const int lane = threadIdx.x & 63, phase = threadIdx.x >> 6;
  const int e = blockIdx.z;
  const int col = blockIdx.x * 512 + lane * 8;
  const int rps = (N + P - 1) / P;
  const int r0 = blockIdx.y * rps, r1 = min(N, r0 + rps);
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (int rb = r0 + phase; rb < r1; rb += 256) {
    const int r = rb + 4 * lane;
    const float dl = r < r1 ? dlogits[(size_t)r * E + e] : 0.f;
    for (unsigned long long mm = __ballot(dl != 0.f); mm != 0ull; mm &= mm - 1ull) {   // ascending rows
      const int j = __ffsll((long long)mm) - 1;
      const float v = __shfl(dl, j, 64);
      if (col < d) {
        float hv[8];
        unpack8(ld16<uint4>(h + (size_t)(rb + 4 * j) * d + col), hv);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(v, hv[i], acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) red[phase][lane * 8 + i] = acc[i];
  __syncthreads();
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int gc = blockIdx.x * 512 + c;
    if (gc < d) part[((size_t)blockIdx.y * E + e) * d + gc] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
  }
}

}  // namespace

void dltb_moe_route(const void* h, const void* wr, int* expert, float* gate, float* logits, int N, int d, int E,
                    int K, hipStream_t st) {
  if (N <= 0) return;
  hipLaunchKernelGGL(moe_route_kernel, dim3(cdiv(N, 4 * RR)), dim3(256), 0, st, (const bf16_t*)h, (const bf16_t*)wr,
                     expert, gate, logits, N, d, E, K);
}

void dltb_moe_assign(const int* expert, int* scratch, int* slot, int* src, int* src_k, int* counts, int N, int K,
                     int E, int C, hipStream_t st) {
  const int NK = N * K;
  const int W = cdiv(NK, 64);
  int* wavecnt = scratch;                     // [W][E]
  int* base = scratch + (size_t)W * E;        // [W][E]
  hipLaunchKernelGGL(moe_hist_kernel, dim3(cdiv(W, 4)), dim3(256), 0, st, expert, wavecnt, NK, E);
  hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)wavecnt, base, counts, W, E);
  hipLaunchKernelGGL(moe_place_kernel, dim3(cdiv(W, 4)), dim3(256), 0, st, expert, (const int*)base,
                     (const int*)counts, slot, src, src_k, NK, K, E, C);
}

int dltb_moe_dropless_rows(int N, int K, int E) { return (N * K + SEG - 1) / SEG * SEG + SEG * E; }

void dltb_moe_assign_dropless(const int* expert, int* scratch, int* slot, int* src, int* src_k, int* counts,
                              int* offsets, int N, int K, int E, int rows, hipStream_t st) {
  const int NK = N * K;
  const int W = cdiv(NK, 64);
  int* wavecnt = scratch;                     // [W][E]
  int* base = scratch + (size_t)W * E;        // [W][E]
  hipLaunchKernelGGL(moe_hist_kernel, dim3(cdiv(W, 4)), dim3(256), 0, st, expert, wavecnt, NK, E);
  hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)wavecnt, base, counts, W, E);
  hipLaunchKernelGGL(moe_place_dropless_kernel, dim3(cdiv(W, 4)), dim3(256), 0, st, expert, (const int*)base,
                     (const int*)counts, slot, src, src_k, offsets, NK, K, E, rows);
}

void dltb_moe_dispatch(const void* h, const int* src, void* xe, int rows, int N, int d, hipStream_t st) {
  hipLaunchKernelGGL(moe_dispatch_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, (const bf16_t*)h, src, (bf16_t*)xe,
                     rows, N, d);
}

void dltb_moe_combine(const void* ye, const int* slot, const float* gate, void* m, int N, int d, int K, int rows,
                      hipStream_t st) {
  hipLaunchKernelGGL(moe_combine_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, (const bf16_t*)ye, slot, gate,
                     (bf16_t*)m, N, d, K, rows);
}

void dltb_moe_combine_bwd(const void* dm, const void* ye, const int* slot, const int* src, const int* expert,
                          const float* gate, void* dye, float* dgate, float* dlogits, int N, int d, int E, int K,
                          int rows, hipStream_t st) {
  hipLaunchKernelGGL(moe_combine_bwd_kernel, dim3(cdiv((long)N + rows, 4)), dim3(256), 0, st, (const bf16_t*)dm,
                     (const bf16_t*)ye, slot, src, expert, gate, (bf16_t*)dye, dgate, dlogits, N, d, E, K, rows);
}

void dltb_moe_dispatch_bwd(const void* dxe, const int* slot, const float* dlogits, const void* wr, void* dh, int N,
                           int d, int E, int K, int rows, hipStream_t st) {
  hipLaunchKernelGGL(moe_dispatch_bwd_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, (const bf16_t*)dxe, slot, dlogits,
                     (const bf16_t*)wr, (bf16_t*)dh, N, d, E, K, rows);
}

int dltb_moe_wgrad_partials(int N, int E, int d) {
  int P = N / 64;
  if (P < 1) P = 1;
  if (P > 128) P = 128;
  while (P > 1 && (size_t)P * E * d * sizeof(float) > ((size_t)64 << 20)) P >>= 1;   // partials: 64 MiB at most
  return P;
}

void dltb_moe_router_wgrad(const float* dlogits, const void* h, float* part, void* dwr, int accumulate, int N, int d,
                           int E, int P, hipStream_t st) {
  hipLaunchKernelGGL(moe_router_wgrad_kernel, dim3(cdiv(d, 512), P, E), dim3(256), 0, st, dlogits, (const bf16_t*)h,
                     part, N, d, E, P);
  DltbColRedSeg seg{};
  seg.part = part;
  seg.out = (uint16_t*)dwr;
  seg.P = P;
  seg.k = E * d;
  seg.accumulate = accumulate;
  dltb_colreduce_multi(&seg, 1, st);
}

// ---------------------------------------------------------------- auxiliary router losses
// balance = E sum_e f[e] P[e] (f[e] = counts[e] / (N K), a constant; P[e] = mean_n softmax(logits[n])[e]) and
// z = mean_n lse[n]^2, lse = logsumexp(logits[n]).  Forward: per-block partials of sum_n p[n, e] and sum_n lse^2,
// folded in block order by a second, one-block launch.  Backward: p = exp(logits - lse) again, added in place.
namespace {

constexpr int AUX_ROWS = 16;                 // rows per wave in the forward: 64 rows per block and per partial
constexpr int AUX_PART = 65;                 // a partial: 64 column sums of p, then the sum of lse^2

__global__ __launch_bounds__(256) void moe_aux_fwd_kernel(const float* __restrict__ logits, float* __restrict__ lse,
                                                          float* __restrict__ part, int N, int E) {
  __shared__ float red[4][AUX_PART];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  DLTB_DCHECK(E >= 1 && E <= 64);
  const int n0 = (blockIdx.x * 4 + wv) * AUX_ROWS;
  const int n1 = min(N, n0 + AUX_ROWS);      // wave-uniform; every wave reaches the barrier below
  float psum = 0.f, zsum = 0.f;
  for (int n = n0; n < n1; ++n) {
    const float v = lane < E ? logits[(size_t)n * E + lane] : -INFINITY;
    const float mx = wave_max(v);
    const float ex = lane < E ? expf(v - mx) : 0.f;
    const float s = wave_sum(ex);             // xor butterfly: the same bits in every lane
    const float l = mx + logf(s);
    if (lane == 0) lse[n] = l;
    psum += ex / s;
    zsum = fmaf(l, l, zsum);
  }
  red[wv][lane] = psum;
  if (lane == 0) red[wv][64] = zsum;
  __syncthreads();
  if (threadIdx.x < AUX_PART) {
    const int c = threadIdx.x;
    part[(size_t)blockIdx.x * AUX_PART + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
  }
}

// one block: wave w folds the partials b = w, w + 4, ... in ascending order (lane = column), the waves are added in
// wave order; the z column is strided over the 256 threads and summed by block_sum
__global__ __launch_bounds__(256) void moe_aux_fin_kernel(const float* __restrict__ part, const int* __restrict__ counts,
                                                          float* __restrict__ out, float* __restrict__ out2, int nb,
                                                          int N, int E, int K) {
  __shared__ float red[4][64];
  __shared__ float redz[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float ps = 0.f, zs = 0.f;
  for (int b = wv; b < nb; b += 4) ps += part[(size_t)b * AUX_PART + lane];
  for (int b = threadIdx.x; b < nb; b += 256) zs += part[(size_t)b * AUX_PART + 64];
  red[wv][lane] = ps;
  const float z = block_sum(zs, redz);       // its barriers also order red
  if (wv != 0) return;
  const float invn = 1.f / (float)N;
  const float P = ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) * invn;
  const float f = lane < E ? (float)counts[lane] / ((float)N * (float)K) : 0.f;
  const float bal = (float)E * wave_sum(lane < E ? f * P : 0.f);
  if (lane == 0) {
    out[0] = bal;
    out[1] = z * invn;
    if (out2 != nullptr) {
      out2[0] = bal;
      out2[1] = z * invn;
    }
  }
}

// one wave per row, lane = expert: dlogits[n, e] += g_b (E / N) p (f[e] - sum_j f[j] p[j]) + g_z (2 / N) lse p
__global__ __launch_bounds__(256) void moe_aux_bwd_kernel(float* __restrict__ dlogits, const float* __restrict__ logits,
                                                          const float* __restrict__ lse, const int* __restrict__ counts,
                                                          const float* __restrict__ g, int N, int E, int K) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;                                    // wave-uniform; the kernel has no block barrier
  DLTB_DCHECK(E >= 1 && E <= 64);
  const bool on = lane < E;
  const size_t i = (size_t)n * E + (on ? lane : 0);
  const float l = lse[n];
  const float p = on ? expf(logits[i] - l) : 0.f;
  const float f = on ? (float)counts[lane] / ((float)N * (float)K) : 0.f;
  const float dot = wave_sum(f * p);
  const float cb = g[0] * ((float)E / (float)N);         // the incoming gradients enter as one factor each: a power
  const float cz = g[1] * (2.f / (float)N);              // of two on them scales the added term exactly
  const float add = fmaf(cb, p * (f - dot), cz * (l * p));
  if (on) dlogits[i] += add;
}

// The router weight gradient for dense dlogits (every entry non-zero once an auxiliary loss is on): a block takes the
// rows [by rps, +rps) for 8 experts at once (64 fp32 accumulators per lane), so h is read ceil(E / 8) times, not E
// times.  Same part[P][E][d] layout, row order and fold as moe_router_wgrad_kernel.
__global__ __launch_bounds__(256) void moe_router_wgrad_dense_kernel(const float* __restrict__ dlogits,
                                                                     const bf16_t* __restrict__ h,
                                                                     float* __restrict__ part, int N, int d, int E,
                                                                     int P) {
  __shared__ __attribute__((aligned(16))) float red[4][512];
  const int lane = threadIdx.x & 63;
  const int phase = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int e0 = blockIdx.z * 8;
  const int col = blockIdx.x * 512 + lane * 8;
  const int rps = (N + P - 1) / P;
  const int r0 = blockIdx.y * rps, r1 = min(N, r0 + rps);
  float acc[8][8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = 0.f;
  if (col < d) {
#pragma unroll 2
    for (int r = r0 + phase; r < r1; r += 4) {            // ascending rows
      float hv[8];
      unpack8(ld16<uint4>(h + (size_t)r * d + col), hv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = e0 + j < E ? dlogits[(size_t)r * E + e0 + j] : 0.f;      // wave-uniform
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j][i] = fmaf(v, hv[i], acc[j][i]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (e0 + j >= E) break;                               // block-uniform
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) red[phase][lane * 8 + i] = acc[j][i];
    __syncthreads();
    for (int c = threadIdx.x; c < 512; c += 256) {
      const int gc = blockIdx.x * 512 + c;
      if (gc < d)
        part[((size_t)blockIdx.y * E + e0 + j) * d + gc] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
  }
}

}  // namespace

int dltb_moe_aux_partials(int N) { return cdiv(N, 4 * AUX_ROWS); }

void dltb_moe_aux_fwd(const float* logits, const int* counts, float* lse, float* part, float* out, float* out2, int N,
                      int E, int K, hipStream_t st) {
  const int nb = dltb_moe_aux_partials(N);
  hipLaunchKernelGGL(moe_aux_fwd_kernel, dim3(nb), dim3(256), 0, st, logits, lse, part, N, E);
  hipLaunchKernelGGL(moe_aux_fin_kernel, dim3(1), dim3(256), 0, st, (const float*)part, counts, out, out2, nb, N, E,
                     K);
}

void dltb_moe_aux_bwd(float* dlogits, const float* logits, const float* lse, const int* counts, const float* g, int N,
                      int E, int K, hipStream_t st) {
  hipLaunchKernelGGL(moe_aux_bwd_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, dlogits, logits, lse, counts, g, N, E, K);
}

void dltb_moe_router_wgrad_dense(const float* dlogits, const void* h, float* part, void* dwr, int accumulate, int N,
                                 int d, int E, int P, hipStream_t st) {
  hipLaunchKernelGGL(moe_router_wgrad_dense_kernel, dim3(cdiv(d, 512), P, cdiv(E, 8)), dim3(256), 0, st, dlogits,
                     (const bf16_t*)h, part, N, d, E, P);
  DltbColRedSeg seg{};
  seg.part = part;
  seg.out = (uint16_t*)dwr;
  seg.P = P;
  seg.k = E * d;
  seg.accumulate = accumulate;
  dltb_colreduce_multi(&seg, 1, st);
}
