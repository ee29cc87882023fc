// api.hip -- context management, error reporting and the primitive-operator entry points of
// the C ABI declared in include/ccx.h.
#include <stdarg.h>
#include "../../include/ccx.h"
#include "attention.h"
#include "ccx_common.h"
#include "elementwise.h"
#include "gemm_bf16.h"

static thread_local std::string g_create_error;

int ccx_fail(ccx_ctx* ctx, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->last_error = buf;
  } else g_create_error = buf;
  return code;
}

extern "C" {

const char* ccx_version(void) { return "ccx 0.1 (gfx950)"; }

int ccx_ctx_create(int device, ccx_ctx** out) {
  if (!out) return ccx_fail(nullptr, CCX_ERR_ARG, "ccx_ctx_create: out is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return ccx_fail(nullptr, CCX_ERR_HIP, "ccx_ctx_create: no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= n) return ccx_fail(nullptr, CCX_ERR_ARG, "ccx_ctx_create: device %d out of range [0,%d)", device, n);
  e = hipSetDevice(device);
  if (e != hipSuccess) return ccx_fail(nullptr, CCX_ERR_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return ccx_fail(nullptr, CCX_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return ccx_fail(nullptr, CCX_ERR_HIP, "libccx is built for gfx950 only; device %d is %s", device, prop.gcnArchName);
  ccx_ctx* c = new ccx_ctx();
  c->device = device;
  *out = c;
  return CCX_OK;
}

static void prof_clear(ccx_ctx* ctx) {
  for (auto& r : ctx->prof) { hipEventDestroy(r.start); hipEventDestroy(r.stop); }
  ctx->prof.clear();
}

void ccx_ctx_destroy(ccx_ctx* ctx) {
  if (!ctx) return;
  prof_clear(ctx);
  delete ctx;
}

int ccx_prof_enable(ccx_ctx* ctx, int on) {
  if (!ctx) return CCX_ERR_ARG;
  prof_clear(ctx);
  ctx->prof_on = on != 0;
  return CCX_OK;
}

int ccx_prof_count(ccx_ctx* ctx) { return ctx ? (int)ctx->prof.size() : 0; }

int ccx_prof_get(ccx_ctx* ctx, int i, char* name_out, int name_cap, double* flops, double* bytes, float* ms) {
  if (!ctx) return CCX_ERR_ARG;
  CCX_REQUIRE(ctx, i >= 0 && i < (int)ctx->prof.size() && name_out && name_cap > 1, "ccx_prof_get: bad index %d", i);
  const ccx_prof_rec& r = ctx->prof[i];
  CCX_HIP(ctx, hipEventSynchronize(r.stop));
  float t = 0.f;
  CCX_HIP(ctx, hipEventElapsedTime(&t, r.start, r.stop));
  snprintf(name_out, name_cap, "%s", r.name);
  if (flops) *flops = r.flops;
  if (bytes) *bytes = r.bytes;
  if (ms) *ms = t;
  return CCX_OK;
}

const char* ccx_last_error(const ccx_ctx* ctx) { return ctx ? ctx->last_error.c_str() : g_create_error.c_str(); }

int ccx_gemm_bf16(ccx_ctx* ctx, int epi, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                  void* out, int64_t ldo, const float* resid, int64_t ldr, int M, int N, int K, void* stream) {
  if (!ctx) return CCX_ERR_ARG;
  CCX_REQUIRE(ctx, epi == EPI_BF16 || epi == EPI_BF16_GELU || epi == EPI_F32_RESID || epi == EPI_F32 || epi == EPI_BF16_RELU,
              "ccx_gemm_bf16: epilogue %d not available through this entry point", epi);
  CCX_REQUIRE(ctx, epi != EPI_F32_RESID || resid != nullptr, "ccx_gemm_bf16: epilogue 2 needs resid");
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw;
  p.M = M; p.N = N; p.K = K; p.bias = bias; p.out = out; p.ldo = ldo; p.resid = resid; p.ldr = ldr;
  return ccx_launch_gemm(ctx, epi, p, (hipStream_t)stream);
}

int ccx_gemm_bf16_desc(ccx_ctx* ctx, int epi, const ccx_gemm_desc* d, void* stream) {
  if (!ctx) return CCX_ERR_ARG;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_gemm_bf16_desc: desc is NULL");
  CCX_REQUIRE(ctx, epi >= EPI_BF16 && epi <= EPI_BF16_ADD_RELU, "ccx_gemm_bf16_desc: unknown epilogue %d", epi);
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16_t*)d->A; p.W = (const bf16_t*)d->W; p.lda = (long)d->lda; p.ldw = (long)d->ldw;
  p.M = d->M; p.N = d->N; p.K = d->K; p.ntaps = d->ntaps; p.a_tap_stride = (long)d->a_tap_stride;
  p.bias = (const float*)d->bias; p.out = (void*)d->out; p.ldo = (long)d->ldo;
  p.resid = (const float*)d->resid; p.ldr = (long)d->ldr; p.resid_mod = d->resid_mod;
  p.scale = (const float*)d->scale; p.shift = (const float*)d->shift; p.slope = d->slope;
  p.rpb_in = d->rpb_in; p.rpb_out = d->rpb_out; p.roff = d->roff; p.rpb_valid = d->rpb_valid;
  p.img_rows_in = d->img_rows_in; p.img_rows_valid = d->img_rows_valid; p.img_rows_out = d->img_rows_out;
  p.resid_bf16 = (const bf16_t*)d->resid_bf16; p.ldrb = (long)d->ldrb;
  p.hq = (bf16_t*)d->hq; p.hk = (bf16_t*)d->hk; p.hv = (bf16_t*)d->hv;
  p.d_model = d->d_model; p.n_head = d->n_head; p.S = d->S; p.Spad = d->Spad;
  p.v_transposed = d->v_transposed; p.first_block = d->first_block;

  // ---- the largest element index the kernel can touch in each buffer, against the stated counts ----
  CCX_REQUIRE(ctx, p.A && p.W && p.M > 0 && p.N > 0 && p.K > 0, "ccx_gemm_bf16_desc: A/W null or empty problem M=%d N=%d K=%d", p.M, p.N, p.K);
  CCX_REQUIRE(ctx, p.lda >= 0 && p.ldw >= 0 && p.a_tap_stride >= 0 && p.ldo >= 0 && p.ldr >= 0 && p.ldrb >= 0 && p.ntaps >= 0,
              "ccx_gemm_bf16_desc: negative stride or tap count");
  CCX_REQUIRE(ctx, p.rpb_in >= 0 && p.rpb_out >= 0 && p.roff >= 0 && p.rpb_valid >= 0 && p.img_rows_in >= 0 && p.img_rows_valid >= 0 &&
              p.img_rows_out >= 0 && p.resid_mod >= 0, "ccx_gemm_bf16_desc: negative row-remap field or resid_mod");
  const long taps = p.ntaps > 1 ? p.ntaps : 1;
  const long Nw = ((long)p.N + 15) / 16 * 16;
  const long a_need = (long)(p.M - 1) * p.lda + (taps - 1) * p.a_tap_stride + p.K;
  CCX_REQUIRE(ctx, a_need <= d->a_elems, "ccx_gemm_bf16_desc: A is read up to element %ld, a_elems=%ld", a_need, (long)d->a_elems);
  const long w_need = (long)(p.N - 1) * p.ldw + taps * p.K;
  CCX_REQUIRE(ctx, w_need <= d->w_elems, "ccx_gemm_bf16_desc: W is read up to element %ld, w_elems=%ld", w_need, (long)d->w_elems);
  if (epi == EPI_HEADS) {
    CCX_REQUIRE(ctx, p.S > 0 && p.Spad >= p.S && p.n_head > 0 && p.M % p.S == 0, "ccx_gemm_bf16_desc: heads need S > 0, Spad >= S, n_head > 0, M %% S == 0");
    const long h_need = (long)(p.M / p.S) * p.n_head * p.Spad * 64;
    CCX_REQUIRE(ctx, h_need <= d->heads_elems, "ccx_gemm_bf16_desc: hq/hk/hv are written up to element %ld, heads_elems=%ld", h_need, (long)d->heads_elems);
  } else {
    // rows: the kernels' own remap; a row that is dropped stores nothing and reads row 0 of the residual
    long max_orow = -1, max_rrow = 0;
    const bool mod = p.resid_mod > 0 && (epi == EPI_F32_RESID || epi == EPI_F32_GELU_POS);
    for (int m = 0; m < p.M; m++) {
      bool valid;
      const long orow = ccx_gemm_remap_row(p, m, valid);
      if (!valid) continue;
      if (orow > max_orow) max_orow = orow;
      const long rrow = mod ? orow % p.resid_mod : orow;
      if (rrow > max_rrow) max_rrow = rrow;
    }
    const long o_need = max_orow < 0 ? 0 : max_orow * p.ldo + Nw;
    CCX_REQUIRE(ctx, o_need <= d->out_elems, "ccx_gemm_bf16_desc: out is written up to element %ld, out_elems=%ld", o_need, (long)d->out_elems);
    const bool res_f32 = epi == EPI_F32_RESID || epi == EPI_F32_GELU_POS || epi == EPI_BF16_LRELU_AFFINE;
    if (res_f32 && p.resid) {
      const long r_need = max_rrow * p.ldr + Nw;
      CCX_REQUIRE(ctx, r_need <= d->resid_elems, "ccx_gemm_bf16_desc: resid is read up to element %ld, resid_elems=%ld", r_need, (long)d->resid_elems);
    }
    if (epi == EPI_BF16_ADD_RELU && p.resid_bf16) {
      const long r_need = max_rrow * p.ldrb + Nw;
      CCX_REQUIRE(ctx, r_need <= d->resid_bf16_elems, "ccx_gemm_bf16_desc: resid_bf16 is read up to element %ld, resid_bf16_elems=%ld", r_need,
                  (long)d->resid_bf16_elems);
    }
  }
  return ccx_launch_gemm(ctx, epi, p, (hipStream_t)stream);
}

int ccx_layernorm(ccx_ctx* ctx, const float* x, const float* gamma, const float* beta, void* out_bf16, float* out_f32,
                  int M, int D, float eps, void* stream) {
  if (!ctx) return CCX_ERR_ARG;
  return ccx_launch_layernorm(ctx, x, D, gamma, beta, (bf16_t*)out_bf16, out_f32, D, M, D, eps, (hipStream_t)stream);
}

int ccx_peak_normalize(ccx_ctx* ctx, const float* x, float* y, int64_t stride, const int* n_samples_dev, int B, float eps, void* stream) {
  if (!ctx) return CCX_ERR_ARG;
  return ccx_launch_peak_normalize(ctx, x, y, (long)stride, n_samples_dev, B, eps, (hipStream_t)stream);
}

int ccx_row_variance(ccx_ctx* ctx, const float* x, int64_t stride, const int* n_samples_dev, int B, float* out, void* stream) {
  if (!ctx) return CCX_ERR_ARG;
  return ccx_launch_row_variance(ctx, x, (long)stride, n_samples_dev, B, out, (hipStream_t)stream);
}

int ccx_cosine_rows(ccx_ctx* ctx, const float* a, const float* b, int R, int D, int b_rows, float* out, void* stream) {
  if (!ctx) return CCX_ERR_ARG;
  return ccx_launch_cosine_rows(ctx, a, b, R, D, b_rows, out, (hipStream_t)stream);
}

int ccx_speaker_profiles(ccx_ctx* ctx, const float* emb, const float* w, const int* spk_dev, int C, int T, int D, int S, float* out, void* stream) {
  if (!ctx) return CCX_ERR_ARG;
  return ccx_launch_speaker_profiles(ctx, emb, w, spk_dev, C, T, D, S, out, (hipStream_t)stream);
}

int ccx_gather_rows(ccx_ctx* ctx, const int64_t* src_ptrs_dev, const int* lens_dev, int n_rows, int max_len, float* dst_dev,
                    int64_t stride, void* stream) {
  if (!ctx) return CCX_ERR_ARG;
  return ccx_launch_gather_rows(ctx, (const long*)src_ptrs_dev, lens_dev, n_rows, max_len, dst_dev, (long)stride, (hipStream_t)stream);
}

int ccx_enc_attention(ccx_ctx* ctx, const void* q, const void* k, const void* vt, void* o, int B, int H, int S, int Spad,
                      void* stream) {
  if (!ctx) return CCX_ERR_ARG;
  return ccx_launch_enc_attention(ctx, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)o, B, H, S, Spad,
                                  (hipStream_t)stream);
}

int ccx_enc_attention_keys(ccx_ctx* ctx, const void* q, const void* k, const void* vt, void* o, int B, int H, int S, int Spad,
                           const int* n_keys_host, void* stream) {
  if (!ctx) return CCX_ERR_ARG;
  CCX_REQUIRE(ctx, n_keys_host && B > 0, "enc_attention_keys: n_keys_host is null or the batch is empty");
  for (int b = 0; b < B; b++)
    CCX_REQUIRE(ctx, n_keys_host[b] >= 1 && n_keys_host[b] <= S, "enc_attention_keys: n_keys[%d]=%d outside [1, %d]", b, n_keys_host[b], S);
  int* d_n = nullptr;
  CCX_HIP(ctx, hipMalloc(&d_n, (size_t)B * sizeof(int)));
  hipError_t e = hipMemcpyAsync(d_n, n_keys_host, (size_t)B * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream);
  int rc = e == hipSuccess ? ccx_launch_enc_attention(ctx, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)o, B, H, S, Spad,
                                                      (hipStream_t)stream, d_n)
                           : ccx_fail(ctx, CCX_ERR_HIP, "enc_attention_keys: copy of the counts failed: %s", hipGetErrorString(e));
  hipStreamSynchronize((hipStream_t)stream);     // the counts are freed below
  hipFree(d_n);
  return rc;
}

}  // extern "C"
