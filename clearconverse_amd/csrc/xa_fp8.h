// xa_fp8.h -- the block-scaled FP8 form of the encoder output (include/ccx.h "FP8 encoder-output stream": the format rule) and the
// layout of its image in HBM.  Integer and bit operations only, host and device: the quantiser depends on no rounding or overflow mode
// of the conversion instructions, and tests/xa_fp8_reference.py restates it line by line.
#pragma once
#include <cstdint>
#include <cstring>
#ifndef __host__
#define __host__
#define __device__
#endif

#define XA_FP8_BLOCK 32        // features that share one scale
#define XA_FP8_EMIN (-64)      // clamp of the block exponent e
#define XA_FP8_EMAX 64

// Block exponent from the largest magnitude of the block, given as bf16 bits without the sign: the smallest e with
// amax <= 448 * 2^e = 1.75 * 2^(e + 8), clamped.  amax = 1.m * 2^E: e = E - 8, one more when 1.m > 1.75 (mantissa bits > 0x60).
// Zero and subnormal amax have exponent bits 0, which the same expression sends below the clamp.
__host__ __device__ static inline int xa_fp8_block_exp(uint32_t amax_bits) {
  int e = (int)(amax_bits >> 7) - 127 - 8 + ((amax_bits & 0x7f) > 0x60 ? 1 : 0);
  e = e < XA_FP8_EMIN ? XA_FP8_EMIN : e;
  return e > XA_FP8_EMAX ? XA_FP8_EMAX : e;
}

// OCP E4M3 (e4m3fn) code of x / 2^e, x as bf16 bits: round to nearest even, clamped to +-448 (0x7e).  Finite x only.
__host__ __device__ static inline uint32_t xa_fp8_code(uint32_t x_bits, int e) {
  const uint32_t sign = (x_bits >> 8) & 0x80, eb = (x_bits >> 7) & 0xff;
  if (eb == 0) return sign;                                  // zero and bf16 subnormals: below half of 2^-9 at every allowed e
  const int ev = (int)eb - 127 - e;                          // exponent of the scaled value
  const uint32_t sig = 0x80 | (x_bits & 0x7f);               // 1.m as 8 bits: value sig * 2^(ev - 7)
  int sh = ev >= -6 ? 4 : 4 + (-6 - ev);                     // bits dropped: 3 mantissa bits above 2^-6, steps of 2^-9 below
  sh = sh > 9 ? 9 : sh;                                      // sig < 2^8: nothing survives 9 bits
  const uint32_t n = (sig + ((1u << (sh - 1)) - 1) + ((sig >> sh) & 1)) >> sh;
  const uint32_t code = ((uint32_t)((ev >= -6 ? ev : -6) + 6) << 3) + n;   // a carry out of the mantissa lands in the exponent
  return sign | (code > 0x7e ? 0x7e : code);
}

// code * 2^e as bf16 bits: exact (at most 4 significant bits, exponent within [-73, 69])
__host__ __device__ static inline uint32_t xa_fp8_value_bits(uint32_t code, int e) {
  const uint32_t e4 = (code >> 3) & 0xf, m3 = code & 7;
  const float m = (float)(e4 ? 8 + m3 : m3);
  const uint32_t pb = (uint32_t)((e4 ? (int)e4 - 10 : -9) + e + 127) << 23;
  float p2;
  memcpy(&p2, &pb, 4);
  const float v = m * p2;
  uint32_t vb;
  memcpy(&vb, &v, 4);
  return (vb >> 16) | ((code & 0x80) << 8);
}

// The image.  Per sequence: ceil(S / 16) key tiles of xa_fp8_tile_bytes(D) bytes, the last padded with copies of key S - 1.  A tile is
// the four wave quarters of the streaming kernel (quarter w: features [w D/4, (w+1) D/4), NKS = D / 128 scale blocks per key), each
//   [128 B of scales][NKS / 2 groups of 1 KB][512 B when NKS is odd]
// so that every load of a wave is whole, consecutive 128-byte lines at every width:
//   group i2 (features 64 i2 .. 64 i2 + 63 of the quarter): lane l of the 16-byte wave load holds the 8 codes of 16-byte bf16 chunk
//     l % 8 of key l / 8, then those of key l / 8 + 8 -- after conversion the two images of the bf16 full-line form;
//   the odd last block (D = 128, 384): lane l of the 8-byte wave load holds chunk l % 4 of key l / 8 + 8 ((l / 4) % 2);
//   scales: the 8 bytes at 8 (l / 4) are the E8M0 bytes that lane l needs: byte i2 / byte 4 + i2 for its two keys in group i2, byte 3
//     for the odd last block; the rest zero.
__host__ __device__ static inline long xa_fp8_quarter_bytes(int D) { return 128 + 4L * D; }
__host__ __device__ static inline long xa_fp8_tile_bytes(int D) { return 4 * xa_fp8_quarter_bytes(D); }
__host__ __device__ static inline long xa_fp8_seq_bytes(int S, int D) { return (long)((S + 15) >> 4) * xa_fp8_tile_bytes(D); }
// byte of (key k of the tile, feature f of the quarter) within the quarter; nks = D / 128
__host__ __device__ static inline int xa_fp8_code_off(int k, int f, int nks) {
  const int lb = f >> 5;
  if (lb < (nks & ~1)) return 128 + (lb >> 1) * 1024 + ((k & 7) * 8 + ((f & 63) >> 3)) * 16 + (k >> 3) * 8 + (f & 7);
  return 128 + (nks >> 1) * 1024 + ((k & 7) * 8 + (k >> 3) * 4 + ((f & 31) >> 3)) * 8 + (f & 7);
}
// byte of the scale of (key k, block lb of the quarter) within the quarter
__host__ __device__ static inline int xa_fp8_scale_off(int k, int lb, int nks) {
  if (lb < (nks & ~1)) return ((k & 7) * 2 + (lb & 1)) * 8 + (k >> 3) * 4 + (lb >> 1);
  return ((k & 7) * 2 + (k >> 3)) * 8 + 3;
}
