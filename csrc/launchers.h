// Host launch entry points of the dltb HIP kernels (implemented in csrc/*.hip, compiled by hipcc
// for gfx950 without torch headers; bindings.cpp adapts them to at::Tensor).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

// norm.hip
void dltb_norm_fwd(const void* x, const void* r, const void* w, const void* b, void* s_out,
                   void* y, float* mean, float* rstd, int N, int d, float eps, bool rms,
                   uint32_t thr16, float drop_scale, const int64_t* seed, int64_t site,
                   hipStream_t st);
// y = norm_fwd's y rebuilt from the row statistics norm_fwd wrote (no row reduction); ys: y's row stride
void dltb_norm_apply(const void* s, const void* w, const void* b, const float* mean, const float* rstd,
                     void* y, long ys, int N, int d, bool rms, hipStream_t st);
// norm_fwd + the attention-dropout mask of (B, T, Hq) in one launch (horizontal fusion)
void dltb_norm_fwd_mask(const void* x, const void* r, const void* w, const void* b, void* s_out, void* y,
                        float* mean, float* rstd, int N, int d, float eps, bool rms, uint32_t thr16,
                        float drop_scale, const int64_t* seed, int64_t site, uint32_t* mask, int B, int T,
                        int Hq, uint32_t mask_thr16, const int64_t* mask_seed, int64_t mask_site, hipStream_t st,
                        int g_begin = 0, int g_end = -1);   // tile groups [g_begin, g_end) of the mask
int dltb_norm_bwd_partials(int N);
void dltb_norm_bwd_dx(const void* dy, const void* s, const void* w, const float* mean,
                      const float* rstd, const void* dres, void* dx, int N, int d, bool rms,
                      hipStream_t st);
void dltb_norm_bwd_dgamma(const void* dy, const void* s, const float* mean, const float* rstd,
                          float* part, void* gw, void* gb, int accumulate, int N, int d, bool rms,
                          hipStream_t st);
void dltb_norm_bwd(const void* dy, const void* s, const void* w, const float* mean,
                   const float* rstd, const void* dres, void* dx, float* part, void* gw, void* gb,
                   int accumulate, int N, int d, bool rms, hipStream_t st);
// fused dx + column partials; part: [(rms ? 1 : 2) + dxsum][blocks(N)][d] fp32
bool dltb_norm_bwd_fused_supported(int d);
int dltb_norm_bwd_fused_blocks(int N);
// dm != nullptr: also dm = dropout_bwd(dx) (site / thr16 / drop_scale / seed) and its column sums
bool dltb_norm_bwd_fused(const void* dy, const void* s, const void* w, const float* mean,
                         const float* rstd, const void* dres, void* dx, float* part, int N, int d,
                         bool rms, bool dxsum, hipStream_t st, void* dm = nullptr, uint32_t thr16 = 0,
                         float drop_scale = 1.f, const int64_t* seed = nullptr, int64_t site = 0,
                         bool dm_sum = true);   // false: dm without its column partials

// elementwise.hip
void dltb_gelu_fwd(const void* f, void* g, long n, hipStream_t st);
void dltb_gelu_fwd_grad(const void* f, void* g, void* gp, long n, hipStream_t st);   // g = GELU(f), gp = GELU'(f)
int dltb_colsum_partials(int N);
void dltb_gelu_bwd(const void* dg, const void* f, void* df, float* part, void* db, int accumulate,
                   int N, int k, hipStream_t st);
void dltb_colsum(const void* src, float* part, void* out, int accumulate, int N, int k,
                 hipStream_t st);
void dltb_dropout(const void* x, const void* r, void* out, long n, int cols, uint32_t thr16,
                  float scale, const int64_t* seed, int64_t site, hipStream_t st);
// geglu: the gate's activation is gelu_tanh instead of SiLU (the GEGLU instantiations)
void dltb_swiglu_fwd(const void* gu, void* h, int N, int F, hipStream_t st, bool geglu = false);
void dltb_swiglu_bwd(const void* dh, const void* gu, void* dgu, int N, int F, hipStream_t st, bool geglu = false);
// swiglu_bwd plus h = swiglu_fwd(gu) rebuilt in the same pass (activation recomputation)
void dltb_swiglu_bwd_h(const void* dh, const void* gu, void* dgu, void* h, int N, int F, hipStream_t st,
                       bool geglu = false);
void dltb_rope(void* qkv, const float* cosb, const float* sinb, int N, int T, int heads, int D,
               int stride, bool inverse, hipStream_t st);
void dltb_f32_from_bf16(float* dst, const void* src, long n, int accumulate, hipStream_t st);
void dltb_transpose(const void* src, void* dst, int R, int C, hipStream_t st);
// nb matrices [R, C] at element stride sbs (src) / dbs (dst) -> [C, R] each, one launch
void dltb_transpose_batched(const void* src, void* dst, int R, int C, int nb, long sbs, long dbs,
                            hipStream_t st);

// qknorm.hip: per-head RMSNorm over D (64 or 128) of the q and k heads fused with the rotate-half RoPE, in place on
// rows of width `stride`; raw: contiguous [N, (Hq + Hkv) D] copy of the q|k columns as they were
void dltb_qknorm_rope_fwd(void* qkv, void* raw, const void* wq, const void* wk, const float* cosb,
                          const float* sinb, int N, int T, int Hq, int Hkv, int D, int stride, float eps,
                          hipStream_t st);
int dltb_qknorm_partials(int N);    // G: workgroups of the backward = rows of part_q / part_k ([G, D] fp32)
void dltb_qknorm_rope_bwd(void* dqkv, const void* raw, const void* wq, const void* wk, const float* cosb,
                          const float* sinb, float* part_q, float* part_k, int N, int T, int Hq, int Hkv, int D,
                          int stride, float eps, hipStream_t st);

// sandwich_norm.hip: "normalise, then add".  s = x + RMSNorm(a; w_out); with w_next also y = RMSNorm(s; w_next) of
// the stored s and rstd_s (w_next == nullptr: y and rstd_s are not touched).  d % 8 == 0, d <= 4096
void dltb_sandwich_fwd(const void* x, const void* a, const void* w_out, const void* w_next, void* s, void* y,
                       float* rstd_a, float* rstd_s, int N, int d, float eps, hipStream_t st);
// the backward of the w_next form: dx = dres + RMSNormBwd(dy; s), da = RMSNormBwd(dx; a) of the stored dx, and the
// fp32 partials part[2][blocks(N)][d] of the w_next and the w_out gradient.  d % 8 == 0, d <= 2048 (else false)
bool dltb_sandwich_bwd_supported(int d);
int dltb_sandwich_bwd_blocks(int N);
bool dltb_sandwich_bwd(const void* dy, const void* s, const void* w_next, const float* rstd_s, const void* dres,
                       const void* a, const void* w_out, const float* rstd_a, void* dx, void* da, float* part,
                       int N, int d, hipStream_t st);

// comm_emu.hip: one emulated RCCL collective (DLTB_COMM=emulate:N) -- `channels` paced workgroups
// that read `traffic` (`passes` times) and write dst[r * rep_stride + j] = scale * src[j]
void dltb_comm_emu(const void* traffic, long traffic_bytes, int passes, void* dst, const void* src, long n,
                   int elem, float scale, int replicas, long rep_stride, float alpha_us, float beta_us,
                   int channels, hipStream_t st);

// embedding.hip
void dltb_embed_fwd(const int64_t* idx, const void* wte, const void* wpe, void* x, int N, int T,
                    int d, uint32_t thr16, float scale, const int64_t* seed, int64_t site,
                    hipStream_t st);
void dltb_embed_bwd_pos(const void* dx, void* dwpe, int B, int T, int P, int d, int accumulate,
                        uint32_t thr16, float scale, const int64_t* seed, int64_t site,
                        hipStream_t st);
bool dltb_embed_bwd_tok_scan(const void* dx, const int64_t* ids, void* dwte, int N, int d, long V,
                             uint32_t thr16, float scale, const int64_t* seed, int64_t site,
                             hipStream_t st);
void dltb_embed_bwd_tok(const void* dx, const int64_t* sorted_ids, const int64_t* perm,
                        void* dwte, int N, int d, long V, uint32_t thr16, float scale,
                        const int64_t* seed, int64_t site, hipStream_t st);

// xent.hip
void dltb_xent_fwd_bwd(void* logits, const int64_t* targets, float* loss, int N, int V,
                       int64_t ignore_index, hipStream_t st);
// the two halves for a head that runs in row chunks: loss + log-sum-exp (logits only read), then dlogits in place
void dltb_xent_lse(const void* logits, const int64_t* targets, float* loss, float* lse, int N, int V,
                   int64_t ignore_index, hipStream_t st);
void dltb_xent_bwd_lse(void* logits, const int64_t* targets, const float* lse, int N, int V,
                       int64_t ignore_index, hipStream_t st);
// the three with the head-loss options: c = softcap tanh(z / softcap) in place of z (softcap > 0; 0 = off) and the
// z-loss z_coef lse^2 (kernels of their own: the three above keep their code objects)
void dltb_xent_fwd_bwd_opt(void* logits, const int64_t* targets, float* loss, int N, int V,
                           int64_t ignore_index, float softcap, float z_coef, hipStream_t st);
void dltb_xent_lse_opt(const void* logits, const int64_t* targets, float* loss, float* lse, int N, int V,
                       int64_t ignore_index, float softcap, float z_coef, hipStream_t st);
void dltb_xent_bwd_lse_opt(void* logits, const int64_t* targets, const float* lse, int N, int V,
                           int64_t ignore_index, float softcap, float z_coef, hipStream_t st);

// adamw.hip
int dltb_adamw_chunk();
void dltb_adamw(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, bool grad_bf16,
                const int* blk_seg, const int64_t* blk_start, int nblocks, const int64_t* seg_ostart,
                const int64_t* seg_len, const int64_t* seg_dst, const float* gscale, const float* hp,
                float lr, float beta1, float beta2, float eps, float wd, float step_size,
                float inv_sqrt_bc2, int grid_cap, hipStream_t st);   // grid_cap 0: one block per row
// block-scaled FP8 moments: E4M3 codes + one fp32 scale per 256 elements of a table row ([rows, 16]); row_off is
// the global table row of blk_seg[0]; counter is read from hp[4] (integer bits) where hp is given
void dltb_adamw_fp8(float* master, uint8_t* mq, uint8_t* sq, float* mscale, float* sscale, const void* grad,
                    bool grad_bf16, const int* blk_seg, const int64_t* blk_start, int nblocks,
                    const int64_t* seg_ostart, const int64_t* seg_len, const int64_t* seg_dst,
                    const float* gscale, const float* hp, float lr, float beta1, float beta2, float eps, float wd,
                    float step_size, float inv_sqrt_bc2, int grid_cap, int64_t row_off, uint64_t seed,
                    uint32_t counter, hipStream_t st);
// the quantiser / decoder of the kernel above on a flat tensor (blocks from its first element); kind 0: m, 1: s
void dltb_fp8_quant(const float* x, uint8_t* codes, float* scales, int64_t n, int kind, bool nearest,
                    uint64_t seed, uint32_t counter, int64_t owner_off, hipStream_t st);
void dltb_fp8_dequant(const uint8_t* codes, const float* scales, float* out, int64_t n, hipStream_t st);
int dltb_sumsq_partials();
void dltb_sumsq(const void* x, bool bf16, long n, float* out, float* part, hipStream_t st);
void dltb_clip_coef(const float* norm_sq, float max_norm, float* coef, float* norm_out,
                    float extra_scale, hipStream_t st);
void dltb_fill_f32(float* x, long n, float v, hipStream_t st);
// dynamic loss scaling step (adamw.hip): state f32[4] = [scale, tracker, steps taken, skipped]
void dltb_amp_step(const float* norm_sq, float* state, float* coef, float* norm_out, float* hp,
                   float max_norm, float extra_scale, float beta1, float beta2, float growth,
                   float backoff, int growth_interval, hipStream_t st);

// attention.hip
bool dltb_attn_supported(int D, int T);
long dltb_attn_mask_words(int B, int Hq, int T);
void dltb_attn_mask(uint32_t* mask, int B, int T, int Hq, uint32_t thr16, const int64_t* seed,
                    int64_t site, hipStream_t st);
// q_begin / q_end (trailing, default absent): a query range [q_begin, q_end) of the length-T problem, multiples of
// 128, causal and thr16 == 0 only.  q / o / dout / dq / lse / delta then hold only those rows of each batch row
// (positions stay global in every mask), k / v / dk / dv all T; dk / dv rows no query of the range sees are
// written as zeros.  q_end <= 0 or (0, T): the square kernels, unchanged.
void dltb_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                   const uint32_t* mask, long qs, long ks, long vs, long os, int B, int T, int Hq,
                   int Hkv, int D, float scale, int causal, uint32_t thr16, float drop_scale,
                   hipStream_t st, int window = 0, const int* bounds = nullptr, int q_begin = 0,
                   int q_end = 0, const void* sink = nullptr, float softcap = 0.f);
// softcap (trailing, default 0 = off; dltb_attn_fwd and dltb_attn_bwd_part): logit soft-capping, every score
// x = scale q.k becomes softcap * tanh(x / softcap) before the masks and the softmax (causal, thr16 == 0, no sink:
// the CAP instantiations of all three kernels).  lse is that of the capped scores; the backward recomputes the tanh
// from the same product and saves nothing more.  With softcap == 0 the launches are exactly those without it.
// sink (trailing, default absent): [Hq] learned sink logits in the build's 16-bit format (causal, thr16 == 0 only).
// One raw logit per query head joins the softmax denominator and carries no value; o and lse include it, and the
// backward kernels above take that lse and o unchanged.  attn_sink.hip forms the sink gradient from lse and delta:
// part[g][h] = - sum over workgroup g's (b, t) rows of exp(sink[h] - lse[b, h, t]) * delta[b, h, t], fp32 [G][Hq]
// with G = dltb_attn_sink_partials(B, Tq); every element of the G rows is written, no atomics, one fixed order.
int dltb_attn_sink_partials(int B, int Tq);
void dltb_attn_sink_bwd(const float* lse, const float* delta, const void* sink, float* part, int B, int Hq, int Tq,
                        hipStream_t st);
void dltb_attn_bwd_delta(const void* o, const void* dout, float* delta, long os, long dos, int B,
                         int T, int Hq, int D, hipStream_t st);
void dltb_attn_bwd_part(int part, const void* q, const void* k, const void* v, const void* dout,
                        const float* lse, const float* delta, const uint32_t* mask, void* out,
                        void* out2, long qs, long ks, long vs, long dos, long outs, long out2s,
                        int B, int T, int Hq, int Hkv, int D, float scale, int causal,
                        uint32_t thr16, float drop_scale, hipStream_t st, const void* o = nullptr,
                        long os = 0, int gsplit = 1, float* part_buf = nullptr, int window = 0,
                        const int* bounds = nullptr, int q_begin = 0, int q_end = 0, float softcap = 0.f);
// dK/dV workgroups per KV head for a causal GQA backward (1 = one workgroup sums the whole group)
int dltb_attn_dkdv_gsplit(int B, int T, int Hq, int Hkv, int causal, int window = 0, int bounds = 0);
// document bounds of packed sequences: int32 [2][B][T] (lo plane, hi plane) from idx [B][T], one launch and no
// host sync.  ``bounds`` arguments above: that buffer (causal only, window = 0: it is folded in here).  The
// attention kernels trust it (non-decreasing planes, lo[i] <= i < hi[i]); hand-made bounds are not validated.
void dltb_attn_doc_bounds(const int64_t* idx, int* bounds, int B, int T, int64_t eos, int window,
                          hipStream_t st);
void dltb_attn_init_attributes();

// ---- batched column reductions (colreduce.hip)
#ifndef DLTB_LAUNCHER_TYPES   // types once (launchers_f16.h repeats only the declarations)
#define DLTB_LAUNCHER_TYPES
enum { DLTB_COLPART_PLAIN = 0, DLTB_COLPART_GELU = 1, DLTB_COLPART_DROP = 2, DLTB_COLPART_LN = 3,
       DLTB_COLPART_RMS = 4 };
#define DLTB_COLRED_MAX 64   // segments per colreduce_multi launch (kernel-argument struct: 2 KiB)
struct DltbColPartSeg {
  const uint16_t* a;
  const uint16_t* b;
  uint16_t* dst;
  const float* mean;
  const float* rstd;
  float* part;
  int N, k, kind;
  int64_t site;
};
struct DltbColRedSeg {
  const float* part;
  uint16_t* out;
  int P, k, accumulate;
};
#endif
int dltb_colpart_partials(int N);
// sums = false: GELU / DROP segments only, the elementwise work without column partials (part unused)
void dltb_colpart(const DltbColPartSeg* segs, int nseg, int P, uint32_t thr16, float drop_scale,
                  const int64_t* seed, bool sums, hipStream_t st);
void dltb_colreduce_multi(const DltbColRedSeg* segs, int nseg, hipStream_t st);

// ---- moe.hip: top-k routing with a fixed capacity of C slots per expert (rows = E * C); N token rows of width d
// (a multiple of 8), 1 <= K <= 4, K <= E <= 64.  expert / slot [N][K], src / src_k [rows], counts [E] are int32,
// gate [N][K], logits / dlogits [N][E] fp32.  slot = -1: dropped; src = -1: empty slot.
void dltb_moe_route(const void* h, const void* wr, int* expert, float* gate, float* logits, int N, int d, int E,
                    int K, hipStream_t st);
// scratch: int32 [2][ceil(N K / 64)][E]
void dltb_moe_assign(const int* expert, int* scratch, int* slot, int* src, int* src_k, int* counts, int N, int K,
                     int E, int C, hipStream_t st);
// dropless: the packed layout of rows = dltb_moe_dropless_rows(N, K, E) = roundup(N K, 128) + 128 E slot rows;
// offsets [E + 1] = exclusive prefix sum of the counts rounded up to 128; src / src_k [rows]; same scratch
int dltb_moe_dropless_rows(int N, int K, int E);
void dltb_moe_assign_dropless(const int* expert, int* scratch, int* slot, int* src, int* src_k, int* counts,
                              int* offsets, int N, int K, int E, int rows, hipStream_t st);
void dltb_moe_dispatch(const void* h, const int* src, void* xe, int rows, int N, int d, hipStream_t st);
void dltb_moe_combine(const void* ye, const int* slot, const float* gate, void* m, int N, int d, int K, int rows,
                      hipStream_t st);
void dltb_moe_combine_bwd(const void* dm, const void* ye, const int* slot, const int* src, const int* expert,
                          const float* gate, void* dye, float* dgate, float* dlogits, int N, int d, int E, int K,
                          int rows, hipStream_t st);
void dltb_moe_dispatch_bwd(const void* dxe, const int* slot, const float* dlogits, const void* wr, void* dh, int N,
                           int d, int E, int K, int rows, hipStream_t st);
int dltb_moe_wgrad_partials(int N, int E, int d);
// part: fp32 [P][E][d], P = dltb_moe_wgrad_partials(N, E, d)
void dltb_moe_router_wgrad(const float* dlogits, const void* h, float* part, void* dwr, int accumulate, int N, int d,
                           int E, int P, hipStream_t st);
// the same for dense dlogits: 8 experts per block, so h is read ceil(E / 8) times (same part, same fold)
void dltb_moe_router_wgrad_dense(const float* dlogits, const void* h, float* part, void* dwr, int accumulate, int N,
                                 int d, int E, int P, hipStream_t st);
// auxiliary router losses: lse [N], out (and out2 when not null) [2] = (balance, z); part: fp32
// [dltb_moe_aux_partials(N)][65].  g [2]: the incoming gradients of (balance, z), on the device.
int dltb_moe_aux_partials(int N);
void dltb_moe_aux_fwd(const float* logits, const int* counts, float* lse, float* part, float* out, float* out2, int N,
                      int E, int K, hipStream_t st);
void dltb_moe_aux_bwd(float* dlogits, const float* logits, const float* lse, const int* counts, const float* g, int N,
                      int E, int K, hipStream_t st);

// ---- gemm.hip: C[M,N] = A B (+bias) (+C); NT: A [M][K], B [N][K]; TN: A [K][M], B [K][N]
bool dltb_gemm_supported(int M, int N, int K, bool tn, int cfg);
int dltb_gemm(const void* a, const void* b, void* c, const void* bias, float* part, long lda, long ldb,
              long ldc, int M, int N, int K, bool tn, int accumulate, int splits, int cfg, int pf, int gm,
              const float* alpha, hipStream_t st, int stages = 0);

// ---- gemm_grouped.hip: one launch over E <= 64 row segments [offsets[e], offsets[e + 1]) of [0, R) (int32 on the
// device, multiples of 128, offsets[E] <= R); R, M, N multiples of 128, K of 64; 16-byte aligned operand rows,
// 16-byte aligned outputs; return 0, or -1 when refused.
//   NT: c[r, :] = a[r, :] B_e^T for r in segment e (a [R][K], B_e = b[e] [N][K], c [R][N]); rows past offsets[E]: 0
//   TN: dW_e (+)= dy[segment e]^T x[segment e] (dy [R][M], x [R][N], dW_e = dw[e] [M][N] contiguous); bit e of
//       `accumulate`: += ; an empty segment writes zeros, or nothing when accumulating
bool dltb_gemm_grouped_nt_supported(int R, int N, int K, int E);
int dltb_gemm_grouped_nt(const void* a, const int* offsets, const void* const* b, void* c, long lda, long ldb,
                         long ldc, int R, int N, int K, int E, hipStream_t st);
bool dltb_gemm_grouped_tn_supported(int R, int M, int N, int E);
int dltb_gemm_grouped_tn(const void* dy, const void* x, const int* offsets, void* const* dw,
                         unsigned long long accumulate, long lddy, long ldx, int R, int M, int N, int E,
                         hipStream_t st);

// ---- gemm_nn.hip: C[M,N] = alpha A B; A [M][K], B [K][N] (the tied head's dgrad without a transposed W);
// cfg 0 = 128x128, 1 = 256x128, 2 = 64x64 tiles; returns the split count used, -1 when refused
bool dltb_gemm_nn_supported(int M, int N, int K, int cfg);
int dltb_gemm_nn(const void* a, const void* b, void* c, float* part, long lda, long ldb, long ldc, int M, int N,
                 int K, int splits, int cfg, int gm, const float* alpha, hipStream_t st);

// ---- gemm_tn.hip: C[b][M][N] (+)= A[b][K][M]^T B[b][K][N] (weight gradients dY^T X), bf16, 256 x 256 tiles,
// M, N multiples of 256, K of 64 (>= 128).  colsum (or null): 16-bit [batch][M] at batch stride scs,
// colsum[b][m] (+)= sum_k A[b][k][m] (the bias gradient of the same linear), fp32 sum rounded once
bool dltb_gemm_tn_supported(int M, int N, int K);
int dltb_gemm_tn(const void* a, const void* b, void* c, long lda, long ldb, long ldc, long sa, long sb, long sc,
                 int M, int N, int K, int batch, int accumulate, void* colsum, long scs, int cs_accumulate,
                 hipStream_t st);

// ---- gemm_rs.hip: C[M,N] = A[M][K] B[N][K]^T (+bias) (+C), bf16, register-staged operands (the step's per-layer kernel)
int dltb_gemm_rs_pick(int M, int N, int K);
bool dltb_gemm_rs_supported(int M, int N, int K, int cfg);
int dltb_gemm_rs(const void* a, const void* b, void* c, const void* bias, long lda, long ldb, long ldc, int M,
                 int N, int K, int accumulate, int cfg, int gm, hipStream_t st, const void* aux = nullptr,
                 float* part = nullptr, void* gout = nullptr);
// C = A B^T + bias and gout = GELU(C) (of the rounded C) from one launch (fp32-image kernels)
bool dltb_gemm_rs_gelu_supported(int M, int N, int K, int cfg);
int dltb_gemm_rs_bm(int cfg);
// C = (A B^T) * aux (elementwise, rounded once) with per-m-tile fp32 column partials of C (the dGELU epilogue)
bool dltb_gemm_rs_aux_supported(int M, int N, int K, int cfg);

// device-scalar helpers (head backward: no host sync)
void dltb_xent_mean(const float* loss, const int64_t* targets, int N, int64_t ignore_index, float* out,
                    hipStream_t st);
void dltb_scale(const void* x, void* y, long n, const float* num, const float* den, float* g_out,
                hipStream_t st);

