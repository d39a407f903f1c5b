// What the chunked linear-attention kernels share: the fixed-decay ones of linear_attn.hip and the gated ones of
// linear_attn_gate.hip.  The argument block, the tile and fragment loads, the transposed-accumulator store and the
// dynamic-LDS sizes; the layouts are described at the top of linear_attn.hip.
#pragma once
#include "common.h"
#include "mfma_tiles.h"

namespace {

constexpr int kC = 64;                       // chunk rows
constexpr float kLn2 = 0.6931471805599453f;

struct LaArgs {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  const bf16_t* dout;
  bf16_t* out;        // qside: o (fwd) / dq (bwd); kside: dk
  bf16_t* out2;       // kside: dv
  const float* l2g;   // [Hkv] log2(gamma)
  float* local;       // [B, Hkv, chunks, D, D] fp32 chunk-local states (state kernel out, scan in)
  bf16_t* state;      // [B, Hkv, chunks, D, D] 16-bit: the state each chunk multiplies (scan out)
  long q_stride, k_stride, v_stride, do_stride, out_stride, out2_stride;
  int B, T, Hq, Hkv;
  float scale;
};

// ROWS rows of D elements (row stride `stride`) -> swizzled LDS image, NT threads, 16-byte chunks
template <int D, int ROWS, int NT>
DLTB_DEV void load_tile(const bf16_t* base, long stride, char* tile, int tid) {
  constexpr int CH = D / 8;
  static_assert(ROWS * CH % NT == 0, "whole chunks per thread");
#pragma unroll
  for (int i = 0; i < ROWS * CH / NT; ++i) {
    const int cid = tid + i * NT;
    const int row = cid / CH, ch = cid % CH;
    *reinterpret_cast<uint4*>(tile + toff<D>(row, ch)) = ld16<uint4>(base + (long)row * stride + ch * 8);
  }
}

// the lane's row as B-operand fragments of k-step s: row order (k = 8 h + j) ...
DLTB_DEV bfx8 ld_row_frag(const bf16_t* row, int s, int h) {
  return __builtin_bit_cast(bfx8, ld16<uint4>(row + 16 * s + 8 * h));
}
// ... and the accumulator's permuted order (k = (j & 3) + 8 (j >> 2) + 4 h), which pairs with tr_frag
DLTB_DEV bfx8 ld_perm_frag(const bf16_t* row, int s, int h) {
  const uint2 a = ld16<uint2>(row + 16 * s + 4 * h), b = ld16<uint2>(row + 16 * s + 8 + 4 * h);
  const uint4 v = {a.x, a.y, b.x, b.y};
  return __builtin_bit_cast(bfx8, v);
}

// accumulator registers 8s .. 8s+7 -> 16-bit B operand of k-step s (the one rounding of a score tile)
DLTB_DEV bfx8 pack_frag(const f32x16& x, int s) {
  bfx8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (h16_t)x[8 * s + j];
  return f;
}

DLTB_DEV int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }   // row of register r in a 32 x 32 block

// a transposed accumulator set (lane = output row, register = column) -> one 16-bit row, scaled; all 64 lanes active
template <int D>
DLTB_DEV void store_acc_rows(bf16_t* dst_row, const f32x16* acc, float scale, int h) {
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) {
#pragma unroll
    for (int g0 = 0; g0 < 4; g0 += 2) {
      const uint32_t x0 = pack_bf2(acc[dt][4 * g0 + 0] * scale, acc[dt][4 * g0 + 1] * scale);
      const uint32_t x1 = pack_bf2(acc[dt][4 * g0 + 2] * scale, acc[dt][4 * g0 + 3] * scale);
      const uint32_t y0 = pack_bf2(acc[dt][4 * g0 + 4] * scale, acc[dt][4 * g0 + 5] * scale);
      const uint32_t y1 = pack_bf2(acc[dt][4 * g0 + 6] * scale, acc[dt][4 * g0 + 7] * scale);
      const auto s0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
      const uint4 o = {s0[0], s1[0], s0[1], s1[1]};
      *reinterpret_cast<uint4*>(dst_row + dt * 32 + 8 * (g0 + h)) = o;
    }
  }
}

DLTB_DEV f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// dynamic LDS: two [kC, D] tiles + kC floats (state), plus a [D, D] state image (qside / kside)
template <int D>
constexpr int state_lds() { return 2 * kC * D * 2 + kC * 4; }
template <int D>
constexpr int side_lds() { return 2 * kC * D * 2 + D * D * 2 + kC * 4; }

}  // namespace
