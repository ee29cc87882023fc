// cross_x.h -- decode cross attention against the ENCODER OUTPUT (cross_x.hip).
#pragma once
#include <cstring>
#include <vector>
#include "ccx_common.h"
#include "xa_fp8.h"

// Whisper's decoder cross attention (openai-whisper model.py MultiHeadAttention with xa; called once per layer and decode step from
// back/api.py:1286-1292 / 1432-1438 / 1474-1480 through transcribe()) reads, per layer, K = xa Wk^T and V = xa Wv^T + bv of every
// sequence: 2 x 1500 x 768 bf16 per layer and sequence, 12 different caches for the 12 layers -- 94 % of a decode step's HBM bytes.
// Both are linear images of the SAME xa, so
//     scores_h[j] = q_h . K_j,h           = (q_h Wk_h) . xa_j            -- "expanded query" q'_h = q_h Wk_h, one 768-vector per head
//     out_h       = sum_j p_hj V_j,h      = (sum_j p_hj xa_j) Wv_h^T + bv -- (sum_j p_hj = 1)
// and one pass over xa (1500 x 768 bf16, shared by all layers) serves all heads: half the bytes per layer, and 1/24 of the cache.
// The price is 12 x the matrix work (every head against all 768 features instead of its 64), which goes to the matrix cores:
// heads are the N index of the MFMAs.
struct XsParams {
  const float* q;        // [rows][D] f32 queries (bias included, not scaled) -- used when x is null
  // query projection inside the expansion (dec_xq_fused_kernel): q = LN(x + pending slabs) Wq^T + bq computed per (head, 16 rows) block
  const float* x; const float* pend; int pend_n; long pend_stride;   // residual rows [rows][D] and split-K partial slabs (decoder.h)
  float* x_out;          // if non-null: the resolved residual rows are written here (must differ from x)
  const float* ln_g; const float* ln_b; float eps;
  const bf16_t* Wq;      // cross_attn.query.weight [D][D] as its fragment image (see below)
  const float* bq;       // [D]
  // LayerNorm-free chain (dec_xq_lnfree_kernel): the residual rows, centred by a per-row shift, as bf16 + their per-tile statistics; Wq then holds gamma o Wq,
  // bq the folded constant c, and q = rstd (xb Wq^T - mean ln_s) + c  (decoder.h, ACT_BF16_LN)
  const bf16_t* xb; const float2* ln_stats; const float* ln_s;
  const bf16_t* WkT;     // [H][D][64]: WkT[h][f][d] = Wk[h*64 + d][f]   (cross_attn.key.weight re-laid per head), the fragment image of
                         // that [H * D][64] matrix
  bf16_t* xq;            // [rows][H][D]: expanded queries
  float* part_o;         // [rows][XS_SPLIT][H][D]: unnormalised contexts of each key half (ccx_xs_part_o_elems)
  float* part_ml;        // [rows][XS_SPLIT][16][2]: reference maximum and denominator of each key half (ccx_xs_part_ml_elems)
  const bf16_t* X;       // [sequences][x_seq_stride]: encoder output rows [S][D] per sequence
  long x_seq_stride;     // elements between sequences
  // FP8 stream (xa_fp8.h): non-null: the streaming blocks read this block-scaled E4M3 image of the same sequences instead of X and
  // convert it to bf16 in registers.  The image decodes to X exactly, so the results are the bits of the bf16 stream on X.
  const unsigned char* X8;
  long x8_seq_stride;    // bytes between sequences
  const int* row_seq;    // row -> sequence (prompt prefill: several rows per sequence); null: identity
  const int* seq_S;      // device, indexed by sequence exactly as X / X8 are (after row_seq, relative to the same base): the keys of that
                         // sequence, each in [1, S] (reduced audio context: the stream stops after them); null: S for every sequence.
                         // Rows of X between a sequence's count and the end of its last 16-key tile must be finite (their p is 0).
  int rows_per_seq;      // > 1: rows s * rows_per_seq .. + rows_per_seq - 1 all belong to sequence row_seq[s * rows_per_seq] (prefill)
  const bf16_t* Wv;      // cross_attn.value.weight [D][D] as its fragment image
  const float* bv;       // [D]
  bf16_t* out;           // [rows][D] attention output (input of cross_attn.out)
  int rows, H, S, D;
  float scale_log2e;     // (d_head ^ -0.25)^2 * log2(e)
  int lds_pad;           // LDS the streaming blocks claim without using it (occupancy cap while decode lanes overlap)
  int full_lines;        // how the streaming blocks ask for xa (ccx_xs_full_lines_switch): 0 half lines, 1 full lines; no effect on
                         // the FP8 stream, whose image has one load form
  // rows a multiple of 16 only.  xb_packed: `xb` is the fragment image of the rows (decoder.h dec_frag_off) instead of row-major;
  // out_packed: `out` is written as that image.  The values a lane holds, and so the results, are the same either way.
  int xb_packed, out_packed;
};

// Wq, WkT and Wv are constants of the checkpoint, and every (head, 16 rows) block of the query and value kernels reads its head's whole
// slice out of L2.  They are stored as fragment images (decoder.h pack_mfma_rows, row_pad 16: tile (n / 16, k / 32) = the 64 lanes'
// 16-byte MFMA operands back to back), so that a wave load is 1 KB contiguous and not 16 rows x 64 B, which a CU pulls out of L2
// three to four times as fast (profiles/dec_full_lines_experiment.txt section 0b).  A lane receives the 16 bytes a row-major load gave it.

// CCX_XS_FULL_LINES (default 1; read per decode and per call of the stand-alone operator): the value for XsParams::full_lines.
// It chooses between the two load forms of the bf16 stream and has no effect on the FP8 stream (XsParams::X8).
int ccx_xs_full_lines_switch();

// cross_attn_ln folded into the cross-attention query (dec_xq_lnfree_kernel): Wg = gamma o Wq [D][D], s_n = sum_k Wg_nk over the bf16
// values the MFMAs see, c_n = sum_k beta_k Wq_nk + bq_n.  Host, f32 in and out.
static inline void ccx_xs_fold_query_ln(const float* gamma, const float* beta, const float* wq, const float* bq, int D, std::vector<float>& Wg,
                                        std::vector<float>& s, std::vector<float>& c) {
  Wg.resize((size_t)D * D); s.resize(D); c.resize(D);
  for (int n = 0; n < D; n++) {
    double ss = 0.0, cc = 0.0;
    for (int k = 0; k < D; k++) {
      const float v = gamma[k] * wq[(size_t)n * D + k];
      Wg[(size_t)n * D + k] = v;
      const uint32_t bits = (uint32_t)ccx_host_f32_to_bf16(v) << 16;
      float r;
      memcpy(&r, &bits, 4);
      ss += (double)r;                                   // what the MFMA sums: the bf16-rounded products
      cc += (double)beta[k] * (double)wq[(size_t)n * D + k];
    }
    s[n] = (float)ss;
    c[n] = (float)(cc + (double)bq[n]);
  }
}
// cross_attn.key.weight [D][D] re-laid per head: WkT[h][f][d] = Wk[h*64 + d][f]  (f32, before it is packed)
static inline std::vector<float> ccx_xs_relay_key(const float* wk, int H, int D) {
  std::vector<float> wkt((size_t)H * D * 64);
  for (int hh = 0; hh < H; hh++)
    for (int f = 0; f < D; f++)
      for (int dd = 0; dd < 64; dd++) wkt[((size_t)hh * D + f) * 64 + dd] = wk[(size_t)(hh * 64 + dd) * D + f];
  return wkt;
}

// key ranges per row, each streamed by a block of its own (fixed: a row's arithmetic must not depend on the launch)
#define XS_SPLIT 2
static inline size_t ccx_xs_part_o_elems(size_t rows, int H, int D) { return rows * XS_SPLIT * (size_t)H * D; }
static inline size_t ccx_xs_part_ml_elems(size_t rows) { return rows * XS_SPLIT * 16 * 2; }
// the three launches of one layer's cross attention: q' = expand(q); partial contexts of the key halves; out = merge(partials) Wv^T + bv
int ccx_launch_xs_cross_attention(ccx_ctx* ctx, const XsParams& p, hipStream_t stream);
// widths the kernels are instantiated for
bool ccx_xs_supported(int D, int H);

// FP8 encoder-output stream (xa_fp8.h; the format rule is in include/ccx.h).  quantise: rows [n_seq][S][D] of xa (x_seq_stride elements
// between sequences) -> the image (img_seq_stride bytes between sequences, >= xa_fp8_seq_bytes(S, D)), and xa overwritten with the
// dequantised values, which bf16 holds exactly (xhat_f32, optional: a dense [n_seq][S][D] f32 copy of them).  The image's unused scale
// bytes are not written: allocate it zeroed.  readback: the image decoded to bf16 rows with the streaming kernel's conversion.
int ccx_launch_xa_fp8_quantise(ccx_ctx* ctx, bf16_t* xa, long x_seq_stride, unsigned char* img, long img_seq_stride, float* xhat_f32, int n_seq,
                               int S, int D, hipStream_t stream);
int ccx_launch_xa_fp8_readback(ccx_ctx* ctx, const unsigned char* img, long img_seq_stride, bf16_t* out, long out_seq_stride, int n_seq, int S,
                               int D, hipStream_t stream);
