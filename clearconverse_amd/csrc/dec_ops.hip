// dec_ops.hip -- the decode step's attention forms, its skinny linear and its token-select kernel as stand-alone operators of the C ABI
// (include/ccx.h: ccx_dec_attention_desc, ccx_dec_ln_linear, ccx_dec_linear_op, ccx_dec_select_step).  For kernel parity tests: each entry point fills the parameter block the model handle
// fills (whisper.hip dec_step / dec_head) and calls the production launchers of decoder.hip unchanged.  Everything the kernels assume is
// checked on the host first; scratch is owned here and freed on every path.
#include "../../include/ccx.h"
#include "ccx_common.h"
#include "decoder.h"
#include "dec_head_row.h"
#include "cross_x.h"
#include "op_scratch.h"

static_assert(sizeof(ccx_dec_seq_state) == sizeof(DecSeqState), "ccx_dec_seq_state mirrors DecSeqState field for field");

namespace {

__global__ void dec_ops_bf16_to_f32_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = bf16_to_f32(in[i]);
}

}  // namespace

extern "C" int ccx_dec_attention_desc(ccx_ctx* ctx, int form, const ccx_dec_attn_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_attention_desc: desc is NULL");
  CCX_REQUIRE(ctx, (form >= CCX_DEC_ATTN_SELF && form <= CCX_DEC_ATTN_TWO_LAUNCH_Q) || form == CCX_DEC_ATTN_STREAM_MAPPED || form == CCX_DEC_ATTN_SELF_IND,
              "ccx_dec_attention_desc: unknown form %d", form);
  const bool is_ind = form == CCX_DEC_ATTN_SELF_IND;
  const bool is_self = form == CCX_DEC_ATTN_SELF || is_ind, is_split = form == CCX_DEC_ATTN_SPLIT, is_mapped = form == CCX_DEC_ATTN_STREAM_MAPPED,
             is_stream = form == CCX_DEC_ATTN_STREAM || is_mapped;
  const bool is_prefill = form == CCX_DEC_ATTN_PREFILL, with_q = form == CCX_DEC_ATTN_FUSED_Q || form == CCX_DEC_ATTN_TWO_LAUNCH_Q;
  const bool partials = is_split || with_q;
  const bool final_out = is_self || is_stream || is_prefill || (is_split && d->combine);
  const int rows = d->rows, H = d->H, n_seq = d->n_seq, kv_T = d->kv_T;
  CCX_REQUIRE(ctx, rows >= 1 && rows <= 65536 && n_seq >= 1 && n_seq <= 65536 && H >= 1 && H <= 64 && kv_T >= 1 && kv_T <= (1 << 20),
              "ccx_dec_attention_desc: rows=%d, n_seq=%d, H=%d or kv_T=%d out of range", rows, n_seq, H, kv_T);
  CCX_REQUIRE(ctx, d->k && d->v && ccx_aligned16(d->k) && ccx_aligned16(d->v), "ccx_dec_attention_desc: k / v null or not 16-byte aligned");
  // K / V are indexed [sequence][H][kv_T][64] up to the last sequence a row may name
  const int64_t kv_need = (int64_t)n_seq * H * kv_T * 64;
  CCX_REQUIRE(ctx, kv_need <= d->kv_elems, "ccx_dec_attention_desc: k / v are read up to element %ld, kv_elems=%ld", (long)kv_need, (long)d->kv_elems);
  // rows -> sequences
  if (is_ind) {
    CCX_REQUIRE(ctx, d->row_seq == nullptr, "ccx_dec_attention_desc: row_seq is not taken by form %d (the rows read through ind)", form);
  } else if (is_self || is_split || is_prefill || is_mapped) {
    if (d->row_seq)
      for (int i = 0; i < rows; i++)
        CCX_REQUIRE(ctx, d->row_seq[i] >= 0 && d->row_seq[i] < n_seq, "ccx_dec_attention_desc: row_seq[%d] = %d out of range [0, %d)", i, d->row_seq[i], n_seq);
    else CCX_REQUIRE(ctx, rows <= n_seq, "ccx_dec_attention_desc: row_seq is NULL with more rows (%d) than sequences (%d)", rows, n_seq);
  } else {
    CCX_REQUIRE(ctx, d->row_seq == nullptr, "ccx_dec_attention_desc: row_seq is not taken by form %d (row r reads sequence r)", form);
    CCX_REQUIRE(ctx, rows <= n_seq, "ccx_dec_attention_desc: more rows (%d) than sequences (%d)", rows, n_seq);
  }
  if (is_prefill) {
    const int P = d->rows_per_seq;
    CCX_REQUIRE(ctx, P >= 2 && P <= 4096, "ccx_dec_attention_desc: rows_per_seq = %d, the prefill form needs >= 2", P);
    CCX_REQUIRE(ctx, d->row_seq && rows % P == 0, "ccx_dec_attention_desc: rows_per_seq needs row_seq and a multiple of it in rows");
    for (int i = 0; i < rows; i++) {
      CCX_REQUIRE(ctx, d->row_seq[i] == d->row_seq[i - i % P], "ccx_dec_attention_desc: row %d is not in its group's sequence (row_seq)", i);
      // the prefill kernels take the sequence from the block index: group g reads sequence g
      CCX_REQUIRE(ctx, d->row_seq[i] == i / P, "ccx_dec_attention_desc: row_seq[%d] = %d, the prefill form needs group g on sequence g", i, d->row_seq[i]);
    }
  } else CCX_REQUIRE(ctx, d->rows_per_seq <= 1, "ccx_dec_attention_desc: rows_per_seq = %d is taken by the prefill form only", d->rows_per_seq);
  // key range
  if (is_self) {
    CCX_REQUIRE(ctx, d->pos != nullptr, "ccx_dec_attention_desc: pos is NULL");
    for (int i = 0; i < rows; i++)
      CCX_REQUIRE(ctx, d->pos[i] >= 0 && d->pos[i] < kv_T, "ccx_dec_attention_desc: pos[%d] = %d out of range [0, kv_T = %d)", i, d->pos[i], kv_T);
    if (is_ind) {
      CCX_REQUIRE(ctx, d->ind != nullptr && d->ind_ld >= 1 && d->ind_ld <= kv_T, "ccx_dec_attention_desc: ind is NULL or ind_ld = %d out of range [1, kv_T = %d]", d->ind_ld, kv_T);
      for (int i = 0; i < rows; i++) {
        CCX_REQUIRE(ctx, d->pos[i] < d->ind_ld, "ccx_dec_attention_desc: pos[%d] = %d needs ind_ld > it (ind_ld = %d)", i, d->pos[i], d->ind_ld);
        for (int t = 0; t <= d->pos[i]; t++)
          CCX_REQUIRE(ctx, d->ind[(size_t)i * d->ind_ld + t] < n_seq, "ccx_dec_attention_desc: ind[%d][%d] = %d out of range [0, n_seq = %d)", i, t,
                      (int)d->ind[(size_t)i * d->ind_ld + t], n_seq);
      }
    }
  } else {
    CCX_REQUIRE(ctx, d->pos == nullptr, "ccx_dec_attention_desc: pos is taken by the self form only");
    CCX_REQUIRE(ctx, d->T >= 1 && d->T <= kv_T, "ccx_dec_attention_desc: T = %d out of range [1, kv_T = %d]", d->T, kv_T);
  }
  if (is_prefill) CCX_REQUIRE(ctx, d->T <= 1536, "ccx_dec_attention_desc: T = %d, the prefill form streams at most 1536 keys per block", d->T);
  const int nsplit = partials ? d->nsplit : 1;
  CCX_REQUIRE(ctx, nsplit >= 1 && nsplit <= 8, "ccx_dec_attention_desc: nsplit = %d out of range [1, 8]", d->nsplit);
  CCX_REQUIRE(ctx, d->lds_pad >= 0 && d->lds_pad <= 128 * 1024 && ((is_split || is_stream) || d->lds_pad == 0),
              "ccx_dec_attention_desc: lds_pad = %d out of range [0, 131072] or given to a form that has none", d->lds_pad);
  // operands and outputs
  if (!with_q) {
    CCX_REQUIRE(ctx, d->q && ccx_aligned16(d->q), "ccx_dec_attention_desc: q null or not 16-byte aligned");
    CCX_REQUIRE(ctx, (int64_t)rows * H * 64 <= d->q_elems, "ccx_dec_attention_desc: q is read up to element %ld, q_elems=%ld", (long)rows * H * 64, (long)d->q_elems);
  }
  if (final_out) {
    CCX_REQUIRE(ctx, d->out != nullptr, "ccx_dec_attention_desc: out is NULL");
    CCX_REQUIRE(ctx, (int64_t)rows * H * 64 <= d->out_elems, "ccx_dec_attention_desc: out is written up to element %ld, out_elems=%ld", (long)rows * H * 64, (long)d->out_elems);
  }
  if (partials) {
    CCX_REQUIRE(ctx, d->part_o && d->part_ml && ccx_aligned16(d->part_o) && ccx_aligned16(d->part_ml), "ccx_dec_attention_desc: part_o / part_ml null or not 16-byte aligned");
    const int64_t po = (int64_t)rows * H * nsplit * 64, pml = (int64_t)rows * H * nsplit * 2;
    CCX_REQUIRE(ctx, po <= d->part_o_elems, "ccx_dec_attention_desc: part_o is written up to element %ld, part_o_elems=%ld", (long)po, (long)d->part_o_elems);
    CCX_REQUIRE(ctx, pml <= d->part_ml_elems, "ccx_dec_attention_desc: part_ml is written up to element %ld, part_ml_elems=%ld", (long)pml, (long)d->part_ml_elems);
  }
  if (with_q) {
    // exactly what ccx_launch_dec_cross_fused_q requires, plus the extents
    CCX_REQUIRE(ctx, rows <= 16 && H == 12, "ccx_dec_attention_desc: the fused query needs rows <= 16 (got %d) and H == 12 (got %d)", rows, H);
    CCX_REQUIRE(ctx, d->x && d->pend && d->ln_g && d->ln_b && d->bq && d->wq_host, "ccx_dec_attention_desc: x, pend, ln_g, ln_b, bq or wq_host is NULL");
    CCX_REQUIRE(ctx, ccx_aligned16(d->x) && ccx_aligned16(d->pend) && ccx_aligned16(d->ln_g) && ccx_aligned16(d->ln_b) && ccx_aligned16(d->bq),
                "ccx_dec_attention_desc: x, pend, ln_g, ln_b or bq not 16-byte aligned");
    CCX_REQUIRE(ctx, d->pend_n >= 0 && d->pend_n <= 4, "ccx_dec_attention_desc: pend_n = %d out of range [0, 4]", d->pend_n);
    CCX_REQUIRE(ctx, d->pend_stride >= (int64_t)rows * 768 && d->pend_stride % 4 == 0, "ccx_dec_attention_desc: pend_stride = %ld smaller than a slab or not a multiple of 4", (long)d->pend_stride);
    CCX_REQUIRE(ctx, (int64_t)rows * 768 <= d->x_elems, "ccx_dec_attention_desc: x is read up to element %ld, x_elems=%ld", (long)rows * 768, (long)d->x_elems);
    const int64_t pn = (int64_t)((d->pend_n > 1 ? d->pend_n : 1) - 1) * d->pend_stride + (int64_t)rows * 768;
    CCX_REQUIRE(ctx, pn <= d->pend_elems, "ccx_dec_attention_desc: pend is read up to element %ld, pend_elems=%ld", (long)pn, (long)d->pend_elems);
    if (d->q_x_out) {
      CCX_REQUIRE(ctx, ccx_aligned16(d->q_x_out) && d->q_x_out != d->x, "ccx_dec_attention_desc: q_x_out not 16-byte aligned or aliasing x");
      CCX_REQUIRE(ctx, (int64_t)rows * 768 <= d->q_x_out_elems, "ccx_dec_attention_desc: q_x_out is written up to element %ld, q_x_out_elems=%ld", (long)rows * 768, (long)d->q_x_out_elems);
    }
  }

  ccx_op_scratch sc;
#define DO_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
  DecAttnParams ap;
  memset(&ap, 0, sizeof(ap));
  ap.q = (const float*)d->q; ap.k = (const bf16_t*)d->k; ap.v = (const bf16_t*)d->v; ap.H = H; ap.kv_T = kv_T; ap.T = is_self ? 0 : d->T;
  ap.scale_log2e = 0.125f * 1.4426950408889634f;
  ap.part_o = (float*)d->part_o; ap.part_ml = (float*)d->part_ml; ap.lds_pad = d->lds_pad;
  const long n_out = (long)rows * H * 64;
  bf16_t* d_out16 = nullptr;
  if (final_out) {
    DO_HIP(sc.alloc(&d_out16, (size_t)n_out));
    DO_HIP(hipMemsetAsync(d_out16, 0xFF, (size_t)n_out * 2, stream));     // NaN bit patterns: a block that never stores shows in out
    ap.out_bf16 = d_out16;
  }
  int* d_pos = nullptr; int* d_rs = nullptr;
  if (is_self) { DO_HIP(sc.upload(&d_pos, d->pos, (size_t)rows)); ap.pos = d_pos; }
  if (d->row_seq) { DO_HIP(sc.upload(&d_rs, d->row_seq, (size_t)rows)); ap.row_seq = d_rs; }
  unsigned short* d_ind = nullptr;
  if (is_ind) { DO_HIP(sc.upload(&d_ind, (const unsigned short*)d->ind, (size_t)rows * d->ind_ld)); ap.ind = d_ind; ap.ind_ld = d->ind_ld; }
  bf16_t* d_wq = nullptr; float* d_q = nullptr;
  if (with_q) {
    const std::vector<bf16_t> packed = pack_mfma_rows(d->wq_host, 768, 768, 16);
    DO_HIP(sc.upload(&d_wq, packed.data(), packed.size()));
  }
  int rc = CCX_OK;
  if (is_self) rc = ccx_launch_dec_attention(ctx, ap, rows, 1, true, stream);
  else if (is_split) {
    rc = ccx_launch_dec_attention(ctx, ap, rows, nsplit, false, stream);
    if (rc == CCX_OK && d->combine) rc = ccx_launch_dec_combine(ctx, ap.part_o, ap.part_ml, nsplit, d_out16, rows, H, stream);
  } else if (is_stream) {
    ap.stream_mode = 1; ap.kv_map = is_mapped ? 1 : 0;
    rc = ccx_launch_dec_attention(ctx, ap, rows, 1, true, stream);
  } else if (is_prefill) {
    ap.stream_mode = 1; ap.rows_per_seq = d->rows_per_seq;
    rc = ccx_launch_dec_attention(ctx, ap, rows / d->rows_per_seq, 1, true, stream);
  } else if (form == CCX_DEC_ATTN_FUSED_Q) {
    ap.qx = (const float*)d->x; ap.q_pend = (const float*)d->pend; ap.q_pend_n = d->pend_n; ap.q_pend_stride = (long)d->pend_stride;
    ap.q_x_out = (float*)d->q_x_out; ap.q_ln_g = (const float*)d->ln_g; ap.q_ln_b = (const float*)d->ln_b; ap.q_eps = d->eps;
    ap.q_W = d_wq; ap.q_bias = (const float*)d->bq; ap.q_K = 768;
    rc = ccx_launch_dec_cross_fused_q(ctx, ap, rows, nsplit, stream);
  } else {
    DO_HIP(sc.alloc(&d_q, (size_t)rows * 768));
    DecLinearParams lp;
    memset(&lp, 0, sizeof(lp));
    lp.M = rows; lp.N = 768; lp.K = 768; lp.W = d_wq; lp.ldw = 768; lp.bias = (const float*)d->bq; lp.out = d_q; lp.ldo = 768;
    lp.x = (const float*)d->x; lp.pend = (const float*)d->pend; lp.pend_n = d->pend_n; lp.pend_stride = (long)d->pend_stride;
    lp.x_out = (float*)d->q_x_out; lp.ln_g = (const float*)d->ln_g; lp.ln_b = (const float*)d->ln_b; lp.eps = d->eps;
    rc = ccx_launch_dec_linear(ctx, ACT_LN, DEPI_F32, lp, stream);
    ap.q = d_q;
    if (rc == CCX_OK) rc = ccx_launch_dec_attention(ctx, ap, rows, nsplit, false, stream);
  }
  if (rc == CCX_OK && final_out) {
    hipLaunchKernelGGL(dec_ops_bf16_to_f32_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, stream, d_out16, (float*)d->out, n_out);
    DO_HIP(hipGetLastError());
  }
  DO_HIP(hipStreamSynchronize(stream));      // the scratch is freed on return
  return rc;
}

namespace {

// bf16 rows [M][K], row-major or as the fragment image, widened to row-major f32
__global__ void dec_ops_rows_to_f32_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, int M, int K, int packed) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)M * K) return;
  const int m = (int)(i / K), k = (int)(i - (long)m * K);
  out[i] = bf16_to_f32(in[packed ? dec_frag_off(m, k, K >> 5) : i]);
}

}  // namespace

extern "C" int ccx_dec_ln_linear(ccx_ctx* ctx, const ccx_dec_ln_linear_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_ln_linear: desc is NULL");
  const int M = d->M, K = d->K, F = d->F, N = d->N, epi = d->epi, packed = d->packed;
  CCX_REQUIRE(ctx, M >= 1 && M <= 4096, "ccx_dec_ln_linear: M = %d out of range [1, 4096]", M);
  CCX_REQUIRE(ctx, K >= 32 && K % 32 == 0 && K <= 1280, "ccx_dec_ln_linear: K = %d must be a multiple of 32 in [32, 1280]", K);
  CCX_REQUIRE(ctx, F == 0 || (F >= 32 && F % 32 == 0 && F <= 5120), "ccx_dec_ln_linear: F = %d must be 0 or a multiple of 32 up to 5120", F);
  CCX_REQUIRE(ctx, N >= 4 && N % 4 == 0 && N <= 8192, "ccx_dec_ln_linear: N = %d must be a multiple of 4 in [4, 8192]", N);
  CCX_REQUIRE(ctx, epi >= CCX_DEC_EPI_PARTIAL && epi <= CCX_DEC_EPI_GELU, "ccx_dec_ln_linear: unknown epi %d", epi);
  CCX_REQUIRE(ctx, packed == 0 || packed == 1, "ccx_dec_ln_linear: packed = %d must be 0 or 1", packed);
  CCX_REQUIRE(ctx, epi != CCX_DEC_EPI_SELF_QKV || (F == 0 && K % 64 == 0 && N == 3 * K), "ccx_dec_ln_linear: SELF_QKV needs F == 0, K a multiple of 64 and N == 3 K");
  CCX_REQUIRE(ctx, epi != CCX_DEC_EPI_GELU || N % 32 == 0, "ccx_dec_ln_linear: the GELU epilogue needs N = %d to be a multiple of 32", N);
  const int Kin = F > 0 ? F : K;                       // input columns of the last linear
  const int depi = epi == CCX_DEC_EPI_PARTIAL ? DEPI_PARTIAL : epi == CCX_DEC_EPI_F32 ? DEPI_F32 : epi == CCX_DEC_EPI_SELF_QKV ? DEPI_SELF_QKV : DEPI_BF16_GELU;
  const int ksplit = ccx_dec_linear_ksplit(Kin, depi);
  CCX_REQUIRE(ctx, epi == CCX_DEC_EPI_PARTIAL || ksplit == 1, "ccx_dec_ln_linear: %d input columns need the PARTIAL epilogue", Kin);
  CCX_REQUIRE(ctx, ksplit <= 4, "ccx_dec_ln_linear: %d input columns leave %d slabs (at most 4)", Kin, ksplit);
  {
    // the launcher's rule (ccx_dec_linear_starved_slice), here before the LayerNorm kernel is launched
    int len = 0;
    CCX_REQUIRE(ctx, F == 0 || ccx_dec_linear_starved_slice(K, 1, &len) < 0, "ccx_dec_ln_linear: K = %d is a K slice of %d k-steps, too few for each of the 4 waves to own one", K, len);
    CCX_REQUIRE(ctx, ccx_dec_linear_starved_slice(Kin, ksplit, &len) < 0, "ccx_dec_ln_linear: %s = %d leaves a K slice of %d k-steps, too few for each of the 4 waves to own one",
                F > 0 ? "F" : "K", Kin, len);
  }
  CCX_REQUIRE(ctx, d->x && d->ln_g && d->ln_b && d->w_host && d->out, "ccx_dec_ln_linear: x, ln_g, ln_b, w_host or out is NULL");
  CCX_REQUIRE(ctx, F == 0 || d->w1_host, "ccx_dec_ln_linear: w1_host is NULL with F = %d", F);
  CCX_REQUIRE(ctx, ccx_aligned16(d->x) && ccx_aligned16(d->ln_g) && ccx_aligned16(d->ln_b) && ccx_aligned16(d->out) && ccx_aligned16(d->b1) && ccx_aligned16(d->bias),
              "ccx_dec_ln_linear: x, ln_g, ln_b, b1, bias or out not 16-byte aligned");
  CCX_REQUIRE(ctx, (int64_t)M * K <= d->x_elems, "ccx_dec_ln_linear: x is read up to element %ld, x_elems=%ld", (long)M * K, (long)d->x_elems);
  const int64_t n_out = epi == CCX_DEC_EPI_PARTIAL ? (int64_t)ksplit * M * N : epi == CCX_DEC_EPI_SELF_QKV ? (int64_t)3 * M * K : (int64_t)M * N;
  CCX_REQUIRE(ctx, n_out <= d->out_elems, "ccx_dec_ln_linear: out is written up to element %ld, out_elems=%ld", (long)n_out, (long)d->out_elems);

  ccx_op_scratch sc;
  const size_t Mp = (size_t)(M + 15) / 16 * 16;        // whole 16-row tiles
  bf16_t *d_xn = nullptr, *d_ffn = nullptr, *d_w1 = nullptr, *d_w = nullptr, *d_g16 = nullptr, *d_ck = nullptr, *d_cv = nullptr;
  float* d_pend = nullptr; int* d_pos = nullptr;
  DO_HIP(sc.alloc(&d_xn, Mp * K));
  DO_HIP(hipMemsetAsync(d_xn, 0xFF, Mp * K * 2, stream));
  DO_HIP(sc.alloc(&d_pend, (size_t)M * K));             // slab 0 is read with weight 0
  DO_HIP(hipMemsetAsync(d_pend, 0, (size_t)M * K * 4, stream));
  DO_HIP(hipMemsetAsync(d->out, 0xFF, (size_t)n_out * 4, stream));
  {
    const std::vector<bf16_t> pw = pack_mfma_rows(d->w_host, N, Kin, 32);
    DO_HIP(sc.upload(&d_w, pw.data(), pw.size()));
  }
  int rc = ccx_launch_dec_resolve_ln(ctx, (const float*)d->x, d_pend, 0, (long)M * K, (const float*)d->ln_g, (const float*)d->ln_b, d_xn, nullptr, M, K,
                                     d->eps, stream, nullptr, packed);
  const bf16_t* act = d_xn;
  if (rc == CCX_OK && F > 0) {
    const std::vector<bf16_t> pw1 = pack_mfma_rows(d->w1_host, F, K, 32);
    DO_HIP(sc.upload(&d_w1, pw1.data(), pw1.size()));
    DO_HIP(sc.alloc(&d_ffn, Mp * F));
    DO_HIP(hipMemsetAsync(d_ffn, 0xFF, Mp * F * 2, stream));
    DecLinearParams lp;
    memset(&lp, 0, sizeof(lp));
    lp.M = M; lp.N = F; lp.K = K; lp.W = d_w1; lp.ldw = K; lp.bias = (const float*)d->b1; lp.act = d_xn; lp.lda = K; lp.act_packed = packed;
    lp.out = d_ffn; lp.ldo = F; lp.out_packed = packed;
    rc = ccx_launch_dec_linear(ctx, ACT_BF16, DEPI_BF16_GELU, lp, stream);
    act = d_ffn;
  }
  if (rc == CCX_OK) {
    DecLinearParams lp;
    memset(&lp, 0, sizeof(lp));
    lp.M = M; lp.N = N; lp.K = Kin; lp.W = d_w; lp.ldw = Kin; lp.bias = (const float*)d->bias; lp.act = act; lp.lda = Kin; lp.act_packed = packed;
    lp.out = d->out; lp.ldo = N; lp.pend_stride = (long)M * N;
    if (epi == CCX_DEC_EPI_SELF_QKV) {
      const std::vector<int> pos((size_t)M, 0);
      DO_HIP(sc.upload(&d_pos, pos.data(), pos.size()));
      DO_HIP(sc.alloc(&d_ck, (size_t)M * K)); DO_HIP(sc.alloc(&d_cv, (size_t)M * K));
      DO_HIP(hipMemsetAsync(d_ck, 0xFF, (size_t)M * K * 2, stream)); DO_HIP(hipMemsetAsync(d_cv, 0xFF, (size_t)M * K * 2, stream));
      lp.ldo = K; lp.cache_k = d_ck; lp.cache_v = d_cv; lp.cache_T = 1; lp.pos = d_pos;
    } else if (epi == CCX_DEC_EPI_GELU) {
      DO_HIP(sc.alloc(&d_g16, Mp * N));
      DO_HIP(hipMemsetAsync(d_g16, 0xFF, Mp * N * 2, stream));
      lp.out = d_g16; lp.out_packed = packed;
    }
    rc = ccx_launch_dec_linear(ctx, ACT_BF16, depi, lp, stream);
    if (rc == CCX_OK && epi == CCX_DEC_EPI_SELF_QKV) {
      const long n = (long)M * K;
      hipLaunchKernelGGL(dec_ops_rows_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_ck, (float*)d->out + n, M, K, 0);
      hipLaunchKernelGGL(dec_ops_rows_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_cv, (float*)d->out + 2 * n, M, K, 0);
      DO_HIP(hipGetLastError());
    } else if (rc == CCX_OK && epi == CCX_DEC_EPI_GELU) {
      const long n = (long)M * N;
      hipLaunchKernelGGL(dec_ops_rows_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_g16, (float*)d->out, M, N, packed);
      DO_HIP(hipGetLastError());
    }
  }
  DO_HIP(hipStreamSynchronize(stream));      // the scratch is freed on return
  return rc;
}

// One launch of dec_linear_kernel as the <= 16-row chain makes it (whisper.hip dec_step: the ln_linear / partial_linear lambdas): the
// caller's device buffers in their native types, so that a test can pre-fill them with sentinels and see which bytes changed.
extern "C" int ccx_dec_linear_op(ccx_ctx* ctx, const ccx_dec_linear_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_linear_op: desc is NULL");
  const int act = d->act, epi = d->epi, M = d->M, N = d->N, K = d->K;
  CCX_REQUIRE(ctx, act == CCX_DEC_ACT_LN || act == CCX_DEC_ACT_BF16 || act == CCX_DEC_ACT_COMBINE, "ccx_dec_linear_op: unknown act %d", act);
  CCX_REQUIRE(ctx, epi >= CCX_DEC_EPI_PARTIAL && epi <= CCX_DEC_EPI_GELU, "ccx_dec_linear_op: unknown epi %d", epi);
  const bool is_ln = act == CCX_DEC_ACT_LN, is_bf16 = act == CCX_DEC_ACT_BF16, is_comb = act == CCX_DEC_ACT_COMBINE;
  const bool is_part = epi == CCX_DEC_EPI_PARTIAL, is_qkv = epi == CCX_DEC_EPI_SELF_QKV;
  // the pairs ccx_launch_dec_linear dispatches
  CCX_REQUIRE(ctx, is_bf16 || (is_ln && !is_part) || (is_comb && is_part), "ccx_dec_linear_op: act %d with epi %d is not a pair the launcher has", act, epi);
  const int kact = is_ln ? ACT_LN : is_bf16 ? ACT_BF16 : ACT_COMBINE;
  const int depi = is_part ? DEPI_PARTIAL : epi == CCX_DEC_EPI_F32 ? DEPI_F32 : is_qkv ? DEPI_SELF_QKV : DEPI_BF16_GELU;
  CCX_REQUIRE(ctx, M >= 1 && M <= (is_bf16 ? 4096 : 16), "ccx_dec_linear_op: M = %d out of range [1, %d]", M, is_bf16 ? 4096 : 16);
  CCX_REQUIRE(ctx, K >= 32 && K % 32 == 0 && K <= (is_bf16 ? 5120 : 1280), "ccx_dec_linear_op: K = %d must be a multiple of 32 in [32, %d]", K, is_bf16 ? 5120 : 1280);
  CCX_REQUIRE(ctx, (!is_comb && !is_qkv) || K % 64 == 0, "ccx_dec_linear_op: K = %d must be a multiple of 64 (whole heads)", K);
  CCX_REQUIRE(ctx, N >= 4 && N % 4 == 0 && N <= 8192, "ccx_dec_linear_op: N = %d must be a multiple of 4 in [4, 8192]", N);
  CCX_REQUIRE(ctx, !is_qkv || N == 3 * K, "ccx_dec_linear_op: SELF_QKV needs N == 3 K (N = %d, K = %d)", N, K);
  const int ksplit = ccx_dec_linear_ksplit(K, depi);
  CCX_REQUIRE(ctx, is_part || ksplit == 1, "ccx_dec_linear_op: K = %d needs the PARTIAL epilogue", K);
  CCX_REQUIRE(ctx, ksplit <= 4, "ccx_dec_linear_op: K = %d leaves %d slabs (at most 4)", K, ksplit);
  {
    int len = 0;
    const int z = ccx_dec_linear_starved_slice(K, ksplit, &len);
    CCX_REQUIRE(ctx, z < 0, "ccx_dec_linear_op: K = %d leaves K slice %d of %d with %d k-steps, too few for each of the 4 waves to own one", K, z, ksplit, len);
  }
  CCX_REQUIRE(ctx, d->w_host != nullptr, "ccx_dec_linear_op: w_host is NULL");
  if (d->bias) {
    CCX_REQUIRE(ctx, ccx_aligned16(d->bias), "ccx_dec_linear_op: bias not 16-byte aligned");
    CCX_REQUIRE(ctx, N <= d->bias_elems, "ccx_dec_linear_op: bias is read up to element %d, bias_elems=%ld", N, (long)d->bias_elems);
  }
  const int64_t MK = (int64_t)M * K;
  if (is_ln) {
    CCX_REQUIRE(ctx, d->x && d->pend && d->ln_g && d->ln_b, "ccx_dec_linear_op: x, pend, ln_g or ln_b is NULL");
    CCX_REQUIRE(ctx, ccx_aligned16(d->x) && ccx_aligned16(d->pend) && ccx_aligned16(d->ln_g) && ccx_aligned16(d->ln_b), "ccx_dec_linear_op: x, pend, ln_g or ln_b not 16-byte aligned");
    CCX_REQUIRE(ctx, d->pend_n >= 0 && d->pend_n <= 4, "ccx_dec_linear_op: pend_n = %d out of range [0, 4]", d->pend_n);
    CCX_REQUIRE(ctx, d->pend_stride >= MK && d->pend_stride % 4 == 0, "ccx_dec_linear_op: pend_stride = %ld smaller than a slab or not a multiple of 4", (long)d->pend_stride);
    CCX_REQUIRE(ctx, MK <= d->x_elems, "ccx_dec_linear_op: x is read up to element %ld, x_elems=%ld", (long)MK, (long)d->x_elems);
    const int64_t pn = (int64_t)((d->pend_n > 1 ? d->pend_n : 1) - 1) * d->pend_stride + MK;     // slab 0 is read also when pend_n == 0
    CCX_REQUIRE(ctx, pn <= d->pend_elems, "ccx_dec_linear_op: pend is read up to element %ld, pend_elems=%ld", (long)pn, (long)d->pend_elems);
    CCX_REQUIRE(ctx, K <= d->ln_elems, "ccx_dec_linear_op: ln_g / ln_b are read up to element %d, ln_elems=%ld", K, (long)d->ln_elems);
    if (d->x_out) {
      CCX_REQUIRE(ctx, ccx_aligned16(d->x_out) && d->x_out != d->x, "ccx_dec_linear_op: x_out not 16-byte aligned or aliasing x");
      CCX_REQUIRE(ctx, MK <= d->x_out_elems, "ccx_dec_linear_op: x_out is written up to element %ld, x_out_elems=%ld", (long)MK, (long)d->x_out_elems);
    }
    if (d->ln_mean_out)
      CCX_REQUIRE(ctx, M <= d->ln_mean_out_elems, "ccx_dec_linear_op: ln_mean_out is written up to element %d, ln_mean_out_elems=%ld", M, (long)d->ln_mean_out_elems);
  } else if (is_bf16) {
    CCX_REQUIRE(ctx, d->act_rows && ccx_aligned16(d->act_rows), "ccx_dec_linear_op: act_rows null or not 16-byte aligned");
    CCX_REQUIRE(ctx, d->lda >= K && d->lda % 8 == 0, "ccx_dec_linear_op: lda = %ld must be >= K and a multiple of 8", (long)d->lda);
    const int64_t an = (int64_t)(M - 1) * d->lda + K;
    CCX_REQUIRE(ctx, an <= d->act_elems, "ccx_dec_linear_op: act_rows are read up to element %ld, act_elems=%ld", (long)an, (long)d->act_elems);
  } else {
    CCX_REQUIRE(ctx, d->nsplit >= 1 && d->nsplit <= 8, "ccx_dec_linear_op: nsplit = %d out of range [1, 8]", d->nsplit);
    CCX_REQUIRE(ctx, d->part_o && d->part_ml && ccx_aligned16(d->part_o) && ccx_aligned16(d->part_ml), "ccx_dec_linear_op: part_o / part_ml null or not 16-byte aligned");
    const int64_t po = MK * d->nsplit, pml = (int64_t)M * (K / 64) * d->nsplit * 2;
    CCX_REQUIRE(ctx, po <= d->part_o_elems, "ccx_dec_linear_op: part_o is read up to element %ld, part_o_elems=%ld", (long)po, (long)d->part_o_elems);
    CCX_REQUIRE(ctx, pml <= d->part_ml_elems, "ccx_dec_linear_op: part_ml is read up to element %ld, part_ml_elems=%ld", (long)pml, (long)d->part_ml_elems);
  }
  // output
  CCX_REQUIRE(ctx, d->out && ccx_aligned16(d->out), "ccx_dec_linear_op: out null or not 16-byte aligned");
  const int ncol = is_qkv ? K : N;                     // columns of a row of `out`
  CCX_REQUIRE(ctx, d->ldo >= ncol && d->ldo % 4 == 0, "ccx_dec_linear_op: ldo = %ld must be >= %d and a multiple of 4", (long)d->ldo, ncol);
  // (the SELF_QKV epilogue does not read ldo: its q rows lie K apart)
  int64_t n_out = (int64_t)(M - 1) * (is_qkv ? K : d->ldo) + ncol;
  if (is_part) {
    CCX_REQUIRE(ctx, d->out_stride >= (int64_t)M * d->ldo && d->out_stride % 4 == 0, "ccx_dec_linear_op: out_stride = %ld smaller than a slab (M ldo) or not a multiple of 4", (long)d->out_stride);
    n_out += (int64_t)(ksplit - 1) * d->out_stride;
  }
  CCX_REQUIRE(ctx, n_out <= d->out_elems, "ccx_dec_linear_op: out is written up to element %ld, out_elems=%ld", (long)n_out, (long)d->out_elems);
  if (is_qkv) {
    const int H = K / 64, Tc = d->cache_T, n_seq = d->n_seq;
    CCX_REQUIRE(ctx, Tc >= 1 && Tc <= 4096 && n_seq >= 1 && n_seq <= 4096, "ccx_dec_linear_op: cache_T = %d or n_seq = %d out of range [1, 4096]", Tc, n_seq);
    CCX_REQUIRE(ctx, d->cache_k && d->cache_v && ccx_aligned16(d->cache_k) && ccx_aligned16(d->cache_v), "ccx_dec_linear_op: cache_k / cache_v null or not 16-byte aligned");
    const int64_t cn = (int64_t)n_seq * H * Tc * 64;
    CCX_REQUIRE(ctx, cn <= d->cache_elems, "ccx_dec_linear_op: cache_k / cache_v are written up to element %ld, cache_elems=%ld", (long)cn, (long)d->cache_elems);
    CCX_REQUIRE(ctx, d->pos != nullptr, "ccx_dec_linear_op: pos is NULL");
    if (!d->row_seq) CCX_REQUIRE(ctx, M <= n_seq, "ccx_dec_linear_op: row_seq is NULL with more rows (%d) than sequences (%d)", M, n_seq);
    std::vector<unsigned char> taken((size_t)n_seq * Tc, 0);
    for (int m = 0; m < M; m++) {
      CCX_REQUIRE(ctx, d->pos[m] >= 0 && d->pos[m] < Tc, "ccx_dec_linear_op: pos[%d] = %d out of range [0, cache_T = %d)", m, d->pos[m], Tc);
      const int sq = d->row_seq ? d->row_seq[m] : m;
      CCX_REQUIRE(ctx, sq >= 0 && sq < n_seq, "ccx_dec_linear_op: row_seq[%d] = %d out of range [0, %d)", m, sq, n_seq);
      unsigned char& t = taken[(size_t)sq * Tc + d->pos[m]];
      CCX_REQUIRE(ctx, !t, "ccx_dec_linear_op: row %d names (sequence %d, pos %d) a second time", m, sq, d->pos[m]);
      t = 1;
    }
  }

  ccx_op_scratch sc;
  bf16_t* d_w = nullptr; int* d_pos = nullptr; int* d_rs = nullptr;
  {
    const std::vector<bf16_t> pw = pack_mfma_rows(d->w_host, N, K, 32);
    DO_HIP(sc.upload(&d_w, pw.data(), pw.size()));
  }
  DecLinearParams lp;
  memset(&lp, 0, sizeof(lp));
  lp.M = M; lp.N = N; lp.K = K; lp.W = d_w; lp.ldw = K; lp.bias = (const float*)d->bias; lp.out = d->out; lp.ldo = (long)d->ldo;
  if (is_ln) {
    lp.x = (const float*)d->x; lp.pend = (const float*)d->pend; lp.pend_n = d->pend_n; lp.pend_stride = (long)d->pend_stride;
    lp.x_out = (float*)d->x_out; lp.ln_g = (const float*)d->ln_g; lp.ln_b = (const float*)d->ln_b; lp.eps = d->eps;
    lp.ln_mean_out = (float*)d->ln_mean_out;
  } else if (is_bf16) {
    lp.act = (const bf16_t*)d->act_rows; lp.lda = (long)d->lda;
  } else {
    lp.part_o = (const float*)d->part_o; lp.part_ml = (const float*)d->part_ml; lp.nsplit = d->nsplit;
  }
  if (is_part) lp.pend_stride = (long)d->out_stride;   // (ACT_LN has no PARTIAL pair: the field is free)
  if (is_qkv) {
    DO_HIP(sc.upload(&d_pos, d->pos, (size_t)M));
    if (d->row_seq) DO_HIP(sc.upload(&d_rs, d->row_seq, (size_t)M));
    lp.cache_k = (bf16_t*)d->cache_k; lp.cache_v = (bf16_t*)d->cache_v; lp.cache_T = d->cache_T; lp.pos = d_pos; lp.row_seq = d_rs;
  }
  const int rc = ccx_launch_dec_linear(ctx, kact, depi, lp, stream);
  DO_HIP(hipStreamSynchronize(stream));      // the scratch is freed on return
  return rc;
}

extern "C" int64_t ccx_dec_mid_chain_out_elems(int M, int D, int H) {
  return (int64_t)M * D * 5 + (int64_t)M * (D / 16) * 2 + (int64_t)M * H * D;
}

extern "C" int ccx_dec_mid_chain(ccx_ctx* ctx, const ccx_dec_mid_chain_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_mid_chain: desc is NULL");
  const int M = d->M, D = d->D, H = d->H, S = d->S, Tc = d->kv_T;
  CCX_REQUIRE(ctx, M >= 1 && M <= 4096, "ccx_dec_mid_chain: M = %d out of range [1, 4096]", M);
  CCX_REQUIRE(ctx, H >= 1 && H <= 64 && D == 64 * H && ccx_xs_supported(D, H), "ccx_dec_mid_chain: D = %d with H = %d heads is not a width the X-stream kernels have (D == 64 H, H in {2, 4, 6, 8, 12})", D, H);
  CCX_REQUIRE(ctx, S >= 16 && S <= 4096, "ccx_dec_mid_chain: S = %d out of range [16, 4096]", S);
  CCX_REQUIRE(ctx, Tc >= 1 && Tc <= 4096, "ccx_dec_mid_chain: kv_T = %d out of range [1, 4096]", Tc);
  CCX_REQUIRE(ctx, d->packed == 0 || d->packed == 1, "ccx_dec_mid_chain: packed = %d must be 0 or 1", d->packed);
  CCX_REQUIRE(ctx, d->q && d->self_k && d->self_v && d->x && d->xa && d->out && d->pos && d->packed_used, "ccx_dec_mid_chain: q, self_k, self_v, x, xa, pos, out or packed_used is NULL");
  CCX_REQUIRE(ctx, d->wo && d->bo && d->lnc_g && d->lnc_b && d->cq_w && d->cq_b && d->ck_w && d->cv_w && d->cv_b && d->co_w && d->co_b, "ccx_dec_mid_chain: a host weight is NULL");
  CCX_REQUIRE(ctx, ccx_aligned16(d->q) && ccx_aligned16(d->self_k) && ccx_aligned16(d->self_v) && ccx_aligned16(d->x) && ccx_aligned16(d->shift) && ccx_aligned16(d->xa) && ccx_aligned16(d->out),
              "ccx_dec_mid_chain: q, self_k, self_v, x, shift, xa or out not 16-byte aligned");
  for (int i = 0; i < M; i++) CCX_REQUIRE(ctx, d->pos[i] >= 0 && d->pos[i] < Tc, "ccx_dec_mid_chain: pos[%d] = %d out of range [0, kv_T = %d)", i, d->pos[i], Tc);
  const int64_t MD = (int64_t)M * D;
  CCX_REQUIRE(ctx, MD <= d->q_elems, "ccx_dec_mid_chain: q is read up to element %ld, q_elems=%ld", (long)MD, (long)d->q_elems);
  CCX_REQUIRE(ctx, MD * Tc <= d->kv_elems, "ccx_dec_mid_chain: self_k / self_v are read up to element %ld, kv_elems=%ld", (long)(MD * Tc), (long)d->kv_elems);
  CCX_REQUIRE(ctx, MD <= d->x_elems, "ccx_dec_mid_chain: x is read up to element %ld, x_elems=%ld", (long)MD, (long)d->x_elems);
  CCX_REQUIRE(ctx, MD * S <= d->xa_elems, "ccx_dec_mid_chain: xa is read up to element %ld, xa_elems=%ld", (long)(MD * S), (long)d->xa_elems);
  const int64_t n_out = ccx_dec_mid_chain_out_elems(M, D, H);
  CCX_REQUIRE(ctx, n_out <= d->out_elems, "ccx_dec_mid_chain: out is written up to element %ld, out_elems=%ld", (long)n_out, (long)d->out_elems);

  // the rule of the model's chain (whisper.hip dec_step)
  const int pk = ccx_dec_rows_as_image(d->packed, M);
  *d->packed_used = pk;
  float* o_attn = (float*)d->out;
  float* o_x = o_attn + MD;
  float* o_xb = o_x + MD;
  float* o_st = o_xb + MD;
  float* o_xq = o_st + (int64_t)M * (D / 16) * 2;
  float* o_cross = o_xq + MD * H;
  float* o_co = o_cross + MD;

  ccx_op_scratch sc;
  const size_t Mp = (size_t)(M + 15) / 16 * 16;        // whole 16-row tiles
  bf16_t *d_attn = nullptr, *d_xb = nullptr, *d_xq = nullptr, *d_wo = nullptr, *d_wco = nullptr, *d_wg = nullptr, *d_wkt = nullptr, *d_wv = nullptr;
  float *d_bo = nullptr, *d_bco = nullptr, *d_s = nullptr, *d_c = nullptr, *d_bv = nullptr, *d_po = nullptr, *d_pml = nullptr;
  float2* d_st = nullptr; int* d_pos = nullptr;
  DO_HIP(hipMemsetAsync(d->out, 0xFF, (size_t)n_out * 4, stream));
  DO_HIP(sc.alloc(&d_attn, Mp * D)); DO_HIP(hipMemsetAsync(d_attn, 0xFF, Mp * D * 2, stream));
  DO_HIP(sc.alloc(&d_xb, Mp * D)); DO_HIP(hipMemsetAsync(d_xb, 0xFF, Mp * D * 2, stream));
  DO_HIP(sc.alloc(&d_st, (size_t)M * (D / 16))); DO_HIP(hipMemsetAsync(d_st, 0xFF, (size_t)M * (D / 16) * 8, stream));
  DO_HIP(sc.alloc(&d_xq, (size_t)MD * H)); DO_HIP(hipMemsetAsync(d_xq, 0xFF, (size_t)MD * H * 2, stream));
  DO_HIP(sc.alloc(&d_po, ccx_xs_part_o_elems(M, H, D))); DO_HIP(hipMemsetAsync(d_po, 0xFF, ccx_xs_part_o_elems(M, H, D) * 4, stream));
  DO_HIP(sc.alloc(&d_pml, ccx_xs_part_ml_elems(M))); DO_HIP(hipMemsetAsync(d_pml, 0xFF, ccx_xs_part_ml_elems(M) * 4, stream));
  DO_HIP(sc.upload(&d_pos, d->pos, (size_t)M));
  float bo_mean;
  {
    // the weights as ccx_whisper_finalize stores them
    const std::vector<bf16_t> wo = pack_mfma_rows(d->wo, D, D, 16), wco = pack_mfma_rows(d->co_w, D, D, 16), wv = pack_mfma_rows(d->cv_w, D, D, 16);
    const std::vector<float> wkt_f = ccx_xs_relay_key(d->ck_w, H, D);
    const std::vector<bf16_t> wkt = pack_mfma_rows(wkt_f.data(), H * D, 64, 16);
    std::vector<float> Wg, sv, cv;
    ccx_xs_fold_query_ln(d->lnc_g, d->lnc_b, d->cq_w, d->cq_b, D, Wg, sv, cv);
    const std::vector<bf16_t> wg = pack_mfma_rows(Wg.data(), D, D, 16);
    double sb = 0.0;
    for (int k = 0; k < D; k++) sb += d->bo[k];
    bo_mean = (float)(sb / D);
    DO_HIP(sc.upload(&d_wo, wo.data(), wo.size())); DO_HIP(sc.upload(&d_wco, wco.data(), wco.size())); DO_HIP(sc.upload(&d_wv, wv.data(), wv.size()));
    DO_HIP(sc.upload(&d_wkt, wkt.data(), wkt.size())); DO_HIP(sc.upload(&d_wg, wg.data(), wg.size()));
    DO_HIP(sc.upload(&d_s, sv.data(), sv.size())); DO_HIP(sc.upload(&d_c, cv.data(), cv.size()));
    DO_HIP(sc.upload(&d_bo, d->bo, (size_t)D)); DO_HIP(sc.upload(&d_bco, d->co_b, (size_t)D)); DO_HIP(sc.upload(&d_bv, d->cv_b, (size_t)D));
  }
  const float scale_log2e = 0.125f * 1.4426950408889634f;
  const dim3 cgrid((unsigned)((MD + 255) / 256));
  // self attention
  DecAttnParams ap;
  memset(&ap, 0, sizeof(ap));
  ap.q = (const float*)d->q; ap.k = (const bf16_t*)d->self_k; ap.v = (const bf16_t*)d->self_v; ap.H = H; ap.kv_T = Tc; ap.pos = d_pos;
  ap.scale_log2e = scale_log2e; ap.out_bf16 = d_attn; ap.out_packed = pk;
  int rc = ccx_launch_dec_attention(ctx, ap, M, 1, true, stream);
  if (rc == CCX_OK) { hipLaunchKernelGGL(dec_ops_rows_to_f32_kernel, cgrid, dim3(256), 0, stream, d_attn, o_attn, M, D, pk); DO_HIP(hipGetLastError()); }
  // out projection, residual resolved in place
  if (rc == CCX_OK) {
    DO_HIP(hipMemcpyAsync(o_x, d->x, (size_t)MD * 4, hipMemcpyDeviceToDevice, stream));
    DecLinearParams lp;
    memset(&lp, 0, sizeof(lp));
    lp.M = M; lp.N = D; lp.K = D; lp.W = d_wo; lp.ldw = D; lp.bias = d_bo; lp.act = d_attn; lp.lda = D; lp.act_packed = pk; lp.out_packed = pk;
    lp.xres = o_x; lp.xb = d_xb; lp.st_out = d_st; lp.shift = (const float*)d->shift; lp.shift_c = bo_mean;
    rc = ccx_launch_dec_linear(ctx, ACT_BF16, DEPI_RESOLVE, lp, stream);
  }
  if (rc == CCX_OK) {
    hipLaunchKernelGGL(dec_ops_rows_to_f32_kernel, cgrid, dim3(256), 0, stream, d_xb, o_xb, M, D, pk); DO_HIP(hipGetLastError());
    DO_HIP(hipMemcpyAsync(o_st, d_st, (size_t)M * (D / 16) * 8, hipMemcpyDeviceToDevice, stream));
    // query + expansion, streaming kernel, merge + value projection
    XsParams xp;
    memset(&xp, 0, sizeof(xp));
    xp.xb = d_xb; xp.xb_packed = pk; xp.ln_stats = d_st; xp.ln_s = d_s; xp.Wq = d_wg; xp.bq = d_c; xp.eps = 1e-5f;
    xp.WkT = d_wkt; xp.xq = d_xq; xp.part_o = d_po; xp.part_ml = d_pml;
    xp.X = (const bf16_t*)d->xa; xp.x_seq_stride = (long)S * D;
    xp.Wv = d_wv; xp.bv = d_bv; xp.out = d_attn; xp.out_packed = pk;
    xp.rows = M; xp.H = H; xp.S = S; xp.D = D; xp.scale_log2e = scale_log2e; xp.full_lines = ccx_xs_full_lines_switch();
    rc = ccx_launch_xs_cross_attention(ctx, xp, stream);
  }
  if (rc == CCX_OK) {
    const long nq = (long)MD * H;
    hipLaunchKernelGGL(dec_ops_bf16_to_f32_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, d_xq, o_xq, nq);
    hipLaunchKernelGGL(dec_ops_rows_to_f32_kernel, cgrid, dim3(256), 0, stream, d_attn, o_cross, M, D, pk);
    DO_HIP(hipGetLastError());
    // cross-attention out projection
    DecLinearParams lp;
    memset(&lp, 0, sizeof(lp));
    lp.M = M; lp.N = D; lp.K = D; lp.W = d_wco; lp.ldw = D; lp.bias = d_bco; lp.act = d_attn; lp.lda = D; lp.act_packed = pk;
    lp.out = o_co; lp.ldo = D; lp.pend_stride = (long)MD;
    rc = ccx_launch_dec_linear(ctx, ACT_BF16, DEPI_PARTIAL, lp, stream);
  }
  DO_HIP(hipStreamSynchronize(stream));      // the scratch is freed on return
  return rc;
}

extern "C" int ccx_dec_select_step(ccx_ctx* ctx, const ccx_dec_select_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_select_step: desc is NULL");
  const int V = d->n_vocab, B = d->B, D = d->D;
  CCX_REQUIRE(ctx, B >= 1 && B <= 65536, "ccx_dec_select_step: B = %d out of range", B);
  CCX_REQUIRE(ctx, V >= 4 && V % 4 == 0 && V <= kHeadMaxVocab, "ccx_dec_select_step: n_vocab = %d must be a multiple of 4 and <= 53248", V);
  CCX_REQUIRE(ctx, d->ld >= V && d->ld % 4 == 0, "ccx_dec_select_step: ld = %ld must be >= n_vocab and a multiple of 4", (long)d->ld);
  CCX_REQUIRE(ctx, d->logits && ccx_aligned16(d->logits), "ccx_dec_select_step: logits null or not 16-byte aligned");
  CCX_REQUIRE(ctx, (int64_t)(B - 1) * d->ld + V <= d->logits_elems, "ccx_dec_select_step: logits are read up to element %ld, logits_elems=%ld",
              (long)((int64_t)(B - 1) * d->ld + V), (long)d->logits_elems);
  CCX_REQUIRE(ctx, d->rules && d->state && d->gen && d->cur_tok && d->pos && d->n_done, "ccx_dec_select_step: rules, state, gen, cur_tok, pos or n_done is NULL");
  const ccx_decode_rules& r = *d->rules;
  std::vector<unsigned char> mask;
  CCX_TRY(ccx_build_suppress_mask(ctx, "ccx_dec_select_step", &r, V, mask));
  int max_init_ts = r.max_initial_timestamp_index, no_rules = 0, sup_blank = 1;
  if (const ccx_decode_options* o = d->opts) {     // the call's options: their mask, the kernels without the rules, the index
    CCX_TRY(ccx_build_options_mask(ctx, "ccx_dec_select_step", &r, o, V, mask));
    no_rules = o->without_timestamps; sup_blank = o->suppress_blank;
    if (o->max_initial_timestamp_index != -2) max_init_ts = o->max_initial_timestamp_index;
  }
  CCX_REQUIRE(ctx, r.no_speech >= 0 && r.timestamp_begin >= 0 && r.blank >= 0, "ccx_dec_select_step: rules.no_speech, timestamp_begin or blank negative");
  CCX_REQUIRE(ctx, d->sample_len >= 1 && d->sample_len <= (1 << 20), "ccx_dec_select_step: sample_len = %d out of range", d->sample_len);
  CCX_REQUIRE(ctx, d->max_prompt >= 0 && (d->max_prompt == 0 || d->prompt), "ccx_dec_select_step: prompt is NULL with max_prompt = %d", d->max_prompt);
  CCX_REQUIRE(ctx, D >= 4 && D % 4 == 0 && D <= 4096, "ccx_dec_select_step: D = %d must be a multiple of 4 in [4, 4096]", D);
  CCX_REQUIRE(ctx, d->tok_emb && d->pos_emb && d->x && ccx_aligned16(d->tok_emb) && ccx_aligned16(d->pos_emb) && ccx_aligned16(d->x),
              "ccx_dec_select_step: tok_emb, pos_emb or x null or not 16-byte aligned");
  CCX_REQUIRE(ctx, (int64_t)V * D <= d->tok_emb_elems, "ccx_dec_select_step: tok_emb is read up to element %ld, tok_emb_elems=%ld", (long)V * D, (long)d->tok_emb_elems);
  CCX_REQUIRE(ctx, (int64_t)B * D <= d->x_elems, "ccx_dec_select_step: x is written up to element %ld, x_elems=%ld", (long)B * D, (long)d->x_elems);
  const int64_t pos_rows = d->pos_emb_elems / D;
  CCX_REQUIRE(ctx, d->sample == 0 || d->sample == 1, "ccx_dec_select_step: sample = %d must be 0 or 1", d->sample);
  CCX_REQUIRE(ctx, d->sample || d->temperature == 0.f, "ccx_dec_select_step: temperature %g needs sample = 1", (double)d->temperature);
  CCX_REQUIRE(ctx, d->temperature >= 0.f && d->row0 >= 0, "ccx_dec_select_step: temperature or row0 negative");
  ccx_decode_sampling_options trunc{0, 1.0f, 0.0f};
  if (d->sampling) {
    CCX_REQUIRE(ctx, d->sample == 1, "ccx_dec_select_step: sampling options need sample = 1");
    trunc = *d->sampling;
    CCX_TRY(ccx_check_sampling_options(ctx, "ccx_dec_select_step", &trunc));
  }
  CCX_REQUIRE(ctx, d->sampling || (!d->cut_out && !d->kept_out && !d->kept_mass_out), "ccx_dec_select_step: cut_out, kept_out and kept_mass_out need sampling options");
  int top_n = 0;
  if (d->logprobs) {
    CCX_TRY(ccx_check_logprob_options(ctx, "ccx_dec_select_step", d->logprobs));
    top_n = d->logprobs->top_n;
    CCX_REQUIRE(ctx, d->tok_logprob_out, "ccx_dec_select_step: logprobs set with tok_logprob_out NULL");
    CCX_REQUIRE(ctx, top_n == 0 || (d->top_id_out && d->top_lp_out), "ccx_dec_select_step: logprobs.top_n = %d with top_id_out or top_lp_out NULL", top_n);
    // the kernel's tables are [B][sample_len] and [B][sample_len][8], staged whole
    CCX_REQUIRE(ctx, (int64_t)B * d->sample_len <= (1 << 22), "ccx_dec_select_step: logprobs with B * sample_len = %ld above %d", (long)B * d->sample_len, 1 << 22);
  }
  CCX_REQUIRE(ctx, d->logprobs || (!d->tok_logprob_out && !d->top_id_out && !d->top_lp_out), "ccx_dec_select_step: tok_logprob_out, top_id_out and top_lp_out need logprobs");
  if (d->stream_ids)
    for (int b = 0; b < B; b++) CCX_REQUIRE(ctx, d->stream_ids[b] >= 0, "ccx_dec_select_step: stream_ids[%d] = %d is negative", b, d->stream_ids[b]);
  for (int b = 0; b < B; b++) {
    const ccx_dec_seq_state& s = d->state[b];
    CCX_REQUIRE(ctx, s.n_gen >= 0 && s.n_gen <= d->sample_len, "ccx_dec_select_step: state[%d].n_gen = %d out of range [0, sample_len = %d]", b, s.n_gen, d->sample_len);
    CCX_REQUIRE(ctx, s.pos >= 0 && s.pos + 1 < pos_rows, "ccx_dec_select_step: state[%d].pos = %d, pos + 1 must be a row of pos_emb (%ld rows)", b, s.pos, (long)pos_rows);
    CCX_REQUIRE(ctx, s.prompt_len >= 0 && s.prompt_len <= d->max_prompt, "ccx_dec_select_step: state[%d].prompt_len = %d out of range [0, max_prompt = %d]", b, s.prompt_len, d->max_prompt);
    CCX_REQUIRE(ctx, s.done == 0 || s.done == 1, "ccx_dec_select_step: state[%d].done = %d must be 0 or 1", b, s.done);
    const bool prompt_phase = s.pos < s.prompt_len - 1;
    if (prompt_phase) {
      const int tok = d->prompt[(size_t)b * d->max_prompt + s.pos + 1];
      CCX_REQUIRE(ctx, tok >= 0 && tok < V, "ccx_dec_select_step: prompt[%d][%d] = %d out of range", b, s.pos + 1, tok);
    } else if (!s.done) {
      // a live row in the sampling phase writes gen[n_gen]
      CCX_REQUIRE(ctx, s.n_gen < d->sample_len, "ccx_dec_select_step: state[%d].n_gen = %d leaves no room in gen (sample_len = %d)", b, s.n_gen, d->sample_len);
      CCX_REQUIRE(ctx, s.last_tok < V && s.pen_tok < V && s.last_ts_tok < V, "ccx_dec_select_step: state[%d] holds a token id >= n_vocab", b);
    }
  }

  ccx_op_scratch sc;
  unsigned char* d_mask = nullptr; DecSeqState* d_state = nullptr;
  int *d_prompt = nullptr, *d_cur = nullptr, *d_pos = nullptr, *d_gen = nullptr, *d_ndone = nullptr;
  unsigned* d_cfg = nullptr; int* d_sid = nullptr;
  const size_t n_gen_tab = (size_t)B * d->sample_len;
  constexpr int kGuard = 16;                 // sentinel words behind the gen table: a write past sample_len of the last row
  std::vector<int> gen_h(n_gen_tab + kGuard, 0x5a5a5a5a);
  memcpy(gen_h.data(), d->gen, n_gen_tab * 4);
  DO_HIP(sc.upload(&d_mask, mask.data(), mask.size()));
  DO_HIP(sc.upload(&d_state, (const DecSeqState*)d->state, (size_t)B));
  if (d->max_prompt > 0) DO_HIP(sc.upload(&d_prompt, d->prompt, (size_t)B * d->max_prompt));
  DO_HIP(sc.upload(&d_cur, d->cur_tok, (size_t)B));
  DO_HIP(sc.upload(&d_pos, d->pos, (size_t)B));
  DO_HIP(sc.upload(&d_gen, gen_h.data(), gen_h.size()));
  DO_HIP(sc.upload(&d_ndone, d->n_done, (size_t)1));
  unsigned cfg[8];
  ccx_fill_sample_cfg(cfg, d->temperature, d->seed, trunc);
  DO_HIP(sc.upload(&d_cfg, cfg, (size_t)8));
  // the truncation outputs: uploaded as the caller left them, so that rows which do not sample come back untouched
  float *d_cut = nullptr, *d_mass = nullptr; int* d_kept = nullptr;
  if (d->cut_out) DO_HIP(sc.upload(&d_cut, d->cut_out, (size_t)B));
  if (d->kept_out) DO_HIP(sc.upload(&d_kept, d->kept_out, (size_t)B));
  if (d->kept_mass_out) DO_HIP(sc.upload(&d_mass, d->kept_mass_out, (size_t)B));
  // the log-probability tables as the kernel indexes them, [row][step] and [row][step][8], under a fill pattern: behind the launch
  // only the slots of the rows that sampled may differ from it
  constexpr unsigned kFill = 0x5a5a5a5au;
  unsigned *d_tlp = nullptr, *d_tid = nullptr, *d_tpl = nullptr;
  std::vector<unsigned> tlp_h, tid_h, tpl_h;
  if (d->logprobs) {
    tlp_h.assign(n_gen_tab, kFill);
    DO_HIP(sc.upload(&d_tlp, tlp_h.data(), tlp_h.size()));
    if (top_n > 0) {
      tid_h.assign(n_gen_tab * kLogprobMaxTop, kFill); tpl_h = tid_h;
      DO_HIP(sc.upload(&d_tid, tid_h.data(), tid_h.size()));
      DO_HIP(sc.upload(&d_tpl, tpl_h.data(), tpl_h.size()));
    }
  }
  std::vector<int> step_of(B, -1);           // the step a row samples in this launch (-1: prompt phase or done)
  for (int b = 0; b < B; b++)
    if (!(d->state[b].pos < d->state[b].prompt_len - 1) && !d->state[b].done) step_of[b] = d->state[b].n_gen;

  DecSelectParams sp;
  memset(&sp, 0, sizeof(sp));
  sp.logits = (const float*)d->logits; sp.ld_logits = (long)d->ld; sp.n_vocab = V; sp.state = d_state; sp.prompt = d_prompt;
  sp.max_prompt = d->max_prompt; sp.cur_tok = d_cur; sp.pos = d_pos; sp.gen = d_gen; sp.sample_len = d->sample_len;
  sp.n_done = d_ndone; sp.suppress_mask = d_mask; sp.eot = r.eot; sp.blank = r.blank;
  sp.no_speech = r.no_speech; sp.timestamp_begin = r.timestamp_begin;
  sp.max_initial_ts = max_init_ts; sp.no_rules = no_rules; sp.suppress_blank = sup_blank;
  sp.tok_emb = (const float*)d->tok_emb; sp.pos_emb = (const float*)d->pos_emb; sp.x = (float*)d->x; sp.D = D;
  sp.sample_cfg = d_cfg; sp.row0 = d->row0; sp.sample = d->sample;
  sp.trunc = d->sampling ? 1 : 0; sp.cut_out = d_cut; sp.kept_out = d_kept; sp.kept_mass_out = d_mass;
  if (d->stream_ids) { DO_HIP(sc.upload(&d_sid, d->stream_ids, (size_t)B)); sp.stream_id = d_sid; }
  sp.tok_logprob = (float*)d_tlp; sp.top_id = (int*)d_tid; sp.top_lp = (float*)d_tpl; sp.top_n = top_n;
  CCX_TRY(ccx_launch_dec_select(ctx, sp, B, stream));
  DO_HIP(hipStreamSynchronize(stream));
  DO_HIP(hipMemcpy(gen_h.data(), d_gen, gen_h.size() * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < kGuard; i++)
    if (gen_h[n_gen_tab + i] != 0x5a5a5a5a) return ccx_fail(ctx, CCX_ERR_STATE, "ccx_dec_select_step: the kernel wrote behind the gen table (word %d)", i);
  memcpy(d->gen, gen_h.data(), n_gen_tab * 4);
  DO_HIP(hipMemcpy(d->state, d_state, (size_t)B * sizeof(DecSeqState), hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->cur_tok, d_cur, (size_t)B * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->pos, d_pos, (size_t)B * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->n_done, d_ndone, 4, hipMemcpyDeviceToHost));
  if (d_cut) DO_HIP(hipMemcpy(d->cut_out, d_cut, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (d_kept) DO_HIP(hipMemcpy(d->kept_out, d_kept, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (d_mass) DO_HIP(hipMemcpy(d->kept_mass_out, d_mass, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (d->logprobs) {
    DO_HIP(hipMemcpy(tlp_h.data(), d_tlp, tlp_h.size() * 4, hipMemcpyDeviceToHost));
    if (top_n > 0) {
      DO_HIP(hipMemcpy(tid_h.data(), d_tid, tid_h.size() * 4, hipMemcpyDeviceToHost));
      DO_HIP(hipMemcpy(tpl_h.data(), d_tpl, tpl_h.size() * 4, hipMemcpyDeviceToHost));
    }
    for (int b = 0; b < B; b++)
      for (int i = 0; i < d->sample_len; i++) {
        const size_t at = (size_t)b * d->sample_len + i;
        const bool mine = i == step_of[b];
        if (!mine && tlp_h[at] != kFill)
          return ccx_fail(ctx, CCX_ERR_STATE, "ccx_dec_select_step: the kernel wrote tok_logprob[%d][%d], a slot of no sampled step", b, i);
        for (int k = 0; k < (top_n > 0 ? kLogprobMaxTop : 0); k++) {
          const size_t ak = at * kLogprobMaxTop + k;
          if (!(mine && k < top_n) && (tid_h[ak] != kFill || tpl_h[ak] != kFill))
            return ccx_fail(ctx, CCX_ERR_STATE, "ccx_dec_select_step: the kernel wrote top[%d][%d][%d], a slot of no sampled step or behind top_n = %d", b, i, k, top_n);
        }
        if (!mine) continue;
        memcpy(&d->tok_logprob_out[b], &tlp_h[at], 4);
        for (int k = 0; k < top_n; k++) {
          memcpy(&d->top_id_out[(size_t)b * top_n + k], &tid_h[at * kLogprobMaxTop + k], 4);
          memcpy(&d->top_lp_out[(size_t)b * top_n + k], &tpl_h[at * kLogprobMaxTop + k], 4);
        }
      }
  }
#undef DO_HIP
  return CCX_OK;
}

extern "C" int ccx_dec_beam_step(ccx_ctx* ctx, const ccx_dec_beam_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_beam_step: desc is NULL");
  const int V = d->n_vocab, G = d->G, beam = d->beam_size, mc = d->max_candidates, D = d->D, SL = d->sample_len;
  CCX_REQUIRE(ctx, beam >= 1 && beam <= kBeamMax, "ccx_dec_beam_step: beam_size = %d out of range [1, %d]", beam, kBeamMax);
  CCX_REQUIRE(ctx, mc >= 1 && mc <= kBeamCandMax, "ccx_dec_beam_step: max_candidates = %d out of range [1, %d]", mc, kBeamCandMax);
  CCX_REQUIRE(ctx, G >= 1 && (int64_t)G * beam <= 65536, "ccx_dec_beam_step: G = %d out of range (G * beam_size <= 65536)", G);
  const int R = G * beam, K = beam + 1;
  CCX_REQUIRE(ctx, V >= 4 && V % 4 == 0 && V <= kHeadMaxVocab, "ccx_dec_beam_step: n_vocab = %d must be a multiple of 4 and <= 53248", V);
  CCX_REQUIRE(ctx, d->ld >= V && d->ld % 4 == 0, "ccx_dec_beam_step: ld = %ld must be >= n_vocab and a multiple of 4", (long)d->ld);
  CCX_REQUIRE(ctx, d->logits && ccx_aligned16(d->logits), "ccx_dec_beam_step: logits null or not 16-byte aligned");
  CCX_REQUIRE(ctx, (int64_t)(R - 1) * d->ld + V <= d->logits_elems, "ccx_dec_beam_step: logits are read up to element %ld, logits_elems=%ld",
              (long)((int64_t)(R - 1) * d->ld + V), (long)d->logits_elems);
  CCX_REQUIRE(ctx, d->rules && d->state && d->hist && d->cur_tok && d->pos && d->n_done, "ccx_dec_beam_step: rules, state, hist, cur_tok, pos or n_done is NULL");
  CCX_REQUIRE(ctx, d->ind && d->fin_tok && d->fin_score && d->fin_n && d->fin_count, "ccx_dec_beam_step: ind, fin_tok, fin_score, fin_n or fin_count is NULL");
  CCX_REQUIRE(ctx, d->cand_id && d->cand_lp && d->tok_out && d->parent_out, "ccx_dec_beam_step: cand_id, cand_lp, tok_out or parent_out is NULL");
  const ccx_decode_rules& r = *d->rules;
  std::vector<unsigned char> mask;
  CCX_TRY(ccx_build_suppress_mask(ctx, "ccx_dec_beam_step", &r, V, mask));
  int max_init_ts = r.max_initial_timestamp_index, no_rules = 0, sup_blank = 1;
  if (const ccx_decode_options* o = d->opts) {     // the call's options: their mask, the kernels without the rules, the index
    CCX_TRY(ccx_build_options_mask(ctx, "ccx_dec_beam_step", &r, o, V, mask));
    no_rules = o->without_timestamps; sup_blank = o->suppress_blank;
    if (o->max_initial_timestamp_index != -2) max_init_ts = o->max_initial_timestamp_index;
  }
  CCX_REQUIRE(ctx, r.no_speech >= 0 && r.timestamp_begin >= 0 && r.blank >= 0, "ccx_dec_beam_step: rules.no_speech, timestamp_begin or blank negative");
  CCX_REQUIRE(ctx, SL >= 1 && SL <= 1024, "ccx_dec_beam_step: sample_len = %d out of range [1, 1024]", SL);
  CCX_REQUIRE(ctx, d->ind_ld >= 1 && d->ind_ld <= 2048, "ccx_dec_beam_step: ind_ld = %d out of range [1, 2048]", d->ind_ld);
  CCX_REQUIRE(ctx, D >= 4 && D % 4 == 0 && D <= 4096, "ccx_dec_beam_step: D = %d must be a multiple of 4 in [4, 4096]", D);
  CCX_REQUIRE(ctx, d->tok_emb && d->pos_emb && d->x && ccx_aligned16(d->tok_emb) && ccx_aligned16(d->pos_emb) && ccx_aligned16(d->x),
              "ccx_dec_beam_step: tok_emb, pos_emb or x null or not 16-byte aligned");
  CCX_REQUIRE(ctx, (int64_t)V * D <= d->tok_emb_elems, "ccx_dec_beam_step: tok_emb is read up to element %ld, tok_emb_elems=%ld", (long)V * D, (long)d->tok_emb_elems);
  CCX_REQUIRE(ctx, (int64_t)R * D <= d->x_elems, "ccx_dec_beam_step: x is written up to element %ld, x_elems=%ld", (long)R * D, (long)d->x_elems);
  const int64_t pos_rows = d->pos_emb_elems / D;
  for (int g = 0; g < G; g++) {
    const ccx_dec_seq_state& s0 = d->state[(size_t)g * beam];
    CCX_REQUIRE(ctx, d->fin_count[g] >= 0 && d->fin_count[g] <= mc, "ccx_dec_beam_step: fin_count[%d] = %d out of range [0, max_candidates = %d]", g, d->fin_count[g], mc);
    for (int j = 0; j < beam; j++) {
      const int b = g * beam + j;
      const ccx_dec_seq_state& s = d->state[b];
      CCX_REQUIRE(ctx, s.done == 0 || s.done == 1, "ccx_dec_beam_step: state[%d].done = %d must be 0 or 1", b, s.done);
      CCX_REQUIRE(ctx, s.done == s0.done && s.n_gen == s0.n_gen && s.pos == s0.pos, "ccx_dec_beam_step: state[%d] differs from its window's first row in done, n_gen or pos", b);
      CCX_REQUIRE(ctx, s.n_gen >= 0 && s.n_gen <= SL, "ccx_dec_beam_step: state[%d].n_gen = %d out of range [0, sample_len = %d]", b, s.n_gen, SL);
      if (s.done) continue;
      CCX_REQUIRE(ctx, s.n_gen < SL, "ccx_dec_beam_step: state[%d].n_gen = %d leaves no room in hist (sample_len = %d)", b, s.n_gen, SL);
      CCX_REQUIRE(ctx, s.prompt_len >= 1 && s.pos == s.prompt_len - 1 + s.n_gen, "ccx_dec_beam_step: state[%d] is not in the sampling phase (pos = %d, prompt_len = %d, n_gen = %d)", b,
                  s.pos, s.prompt_len, s.n_gen);
      CCX_REQUIRE(ctx, s.pos + 1 < pos_rows, "ccx_dec_beam_step: state[%d].pos = %d, pos + 1 must be a row of pos_emb (%ld rows)", b, s.pos, (long)pos_rows);
      CCX_REQUIRE(ctx, s.pos + 1 < d->ind_ld, "ccx_dec_beam_step: state[%d].pos = %d, pos + 1 must be a column of ind (ind_ld = %d)", b, s.pos, d->ind_ld);
      CCX_REQUIRE(ctx, s.last_tok < V && s.pen_tok < V && s.last_ts_tok < V, "ccx_dec_beam_step: state[%d] holds a token id >= n_vocab", b);
    }
  }
  const size_t lds = (size_t)beam * SL * 4 + ccx_align((size_t)beam * d->ind_ld * 2, 16);
  CCX_REQUIRE(ctx, lds <= 48 * 1024, "ccx_dec_beam_step: beam_size %d x (sample_len %d, ind_ld %d) needs %zu bytes of LDS (at most 49152)", beam, SL, d->ind_ld, lds);

#define DO_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
  ccx_op_scratch sc;
  constexpr int kGuard = 16;                 // sentinel words behind the tables the update kernel writes row by row
  const size_t n_hist = (size_t)R * SL, n_ind = (size_t)R * d->ind_ld, n_fin = (size_t)G * mc * SL;
  std::vector<int> hist_h(n_hist + kGuard, 0x5a5a5a5a), fin_h(n_fin + kGuard, 0x5a5a5a5a);
  std::vector<unsigned short> ind_h(n_ind + kGuard, 0x5a5a);
  memcpy(hist_h.data(), d->hist, n_hist * 4);
  memcpy(fin_h.data(), d->fin_tok, n_fin * 4);
  memcpy(ind_h.data(), d->ind, n_ind * 2);
  unsigned char* d_mask = nullptr; DecSeqState* d_state = nullptr;
  int *d_cur = nullptr, *d_pos = nullptr, *d_hist = nullptr, *d_ndone = nullptr, *d_fin = nullptr, *d_finn = nullptr, *d_finc = nullptr;
  int *d_cid = nullptr, *d_tok = nullptr, *d_par = nullptr;
  float *d_fins = nullptr, *d_clp = nullptr;
  unsigned short* d_ind = nullptr;
  DO_HIP(sc.upload(&d_mask, mask.data(), mask.size()));
  DO_HIP(sc.upload(&d_state, (const DecSeqState*)d->state, (size_t)R));
  DO_HIP(sc.upload(&d_cur, d->cur_tok, (size_t)R));
  DO_HIP(sc.upload(&d_pos, d->pos, (size_t)R));
  DO_HIP(sc.upload(&d_hist, hist_h.data(), hist_h.size()));
  DO_HIP(sc.upload(&d_ndone, d->n_done, (size_t)1));
  DO_HIP(sc.upload(&d_ind, ind_h.data(), ind_h.size()));
  DO_HIP(sc.upload(&d_fin, fin_h.data(), fin_h.size()));
  DO_HIP(sc.upload(&d_fins, d->fin_score, (size_t)G * mc));
  DO_HIP(sc.upload(&d_finn, d->fin_n, (size_t)G * mc));
  DO_HIP(sc.upload(&d_finc, d->fin_count, (size_t)G));
  DO_HIP(sc.alloc(&d_cid, (size_t)R * K));
  DO_HIP(sc.alloc(&d_clp, (size_t)R * K));
  DO_HIP(sc.alloc(&d_tok, (size_t)R));
  DO_HIP(sc.alloc(&d_par, (size_t)R));
  DO_HIP(hipMemsetAsync(d_cid, 0xFF, (size_t)R * K * 4, stream));
  DO_HIP(hipMemsetAsync(d_clp, 0xFF, (size_t)R * K * 4, stream));
  DO_HIP(hipMemsetAsync(d_tok, 0xFF, (size_t)R * 4, stream));
  DO_HIP(hipMemsetAsync(d_par, 0xFF, (size_t)R * 4, stream));

  DecBeamParams bp;
  memset(&bp, 0, sizeof(bp));
  DecSelectParams& sp = bp.sel;
  sp.logits = (const float*)d->logits; sp.ld_logits = (long)d->ld; sp.n_vocab = V; sp.state = d_state;
  sp.cur_tok = d_cur; sp.pos = d_pos; sp.gen = d_hist; sp.sample_len = SL;
  sp.n_done = d_ndone; sp.suppress_mask = d_mask; sp.eot = r.eot; sp.blank = r.blank;
  sp.no_speech = r.no_speech; sp.timestamp_begin = r.timestamp_begin;
  sp.max_initial_ts = max_init_ts; sp.no_rules = no_rules; sp.suppress_blank = sup_blank;
  sp.tok_emb = (const float*)d->tok_emb; sp.pos_emb = (const float*)d->pos_emb; sp.x = (float*)d->x; sp.D = D;
  bp.beam = beam; bp.max_cand = mc; bp.cand_id = d_cid; bp.cand_lp = d_clp; bp.ind = d_ind; bp.ind_ld = d->ind_ld; bp.row0 = 0;
  bp.fin_tok = d_fin; bp.fin_score = d_fins; bp.fin_n = d_finn; bp.fin_count = d_finc; bp.step_tok = d_tok; bp.step_parent = d_par;
  CCX_TRY(ccx_launch_dec_beam(ctx, bp, G, stream));
  DO_HIP(hipStreamSynchronize(stream));
  DO_HIP(hipMemcpy(hist_h.data(), d_hist, hist_h.size() * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(fin_h.data(), d_fin, fin_h.size() * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(ind_h.data(), d_ind, ind_h.size() * 2, hipMemcpyDeviceToHost));
  for (int i = 0; i < kGuard; i++)
    if (hist_h[n_hist + i] != 0x5a5a5a5a || fin_h[n_fin + i] != 0x5a5a5a5a || ind_h[n_ind + i] != 0x5a5a)
      return ccx_fail(ctx, CCX_ERR_STATE, "ccx_dec_beam_step: a kernel wrote behind the hist, fin_tok or ind table (word %d)", i);
  memcpy(d->hist, hist_h.data(), n_hist * 4);
  memcpy(d->fin_tok, fin_h.data(), n_fin * 4);
  memcpy(d->ind, ind_h.data(), n_ind * 2);
  DO_HIP(hipMemcpy(d->state, d_state, (size_t)R * sizeof(DecSeqState), hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->cur_tok, d_cur, (size_t)R * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->pos, d_pos, (size_t)R * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->n_done, d_ndone, 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->fin_score, d_fins, (size_t)G * mc * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->fin_n, d_finn, (size_t)G * mc * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->fin_count, d_finc, (size_t)G * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->cand_id, d_cid, (size_t)R * K * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->cand_lp, d_clp, (size_t)R * K * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->tok_out, d_tok, (size_t)R * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->parent_out, d_par, (size_t)R * 4, hipMemcpyDeviceToHost));
#undef DO_HIP
  return CCX_OK;
}
