// spectral_gate.hip -- spectral-gate denoiser: stationary mode (K2 in SURVEY.md section 2a), non-stationary mode, noise clip.
//
// Replaces `nr.reduce_noise(y=..., sr=16000, stationary=True, prop_decrease=p)` (reference
// back/api.py:349 on speaker-profile crops and 832-833 on the whole clip).  Semantics follow
// noisereduce's SpectralGateStationary [UPSTREAM-RECALL]; CPU restatement (on scipy.signal):
// oracle/spectral_gate_ref.py.
//
// Pipeline per clip (all HBM-bound, one launch per stage over all clips):
//   STFT (n_fft 1024, hop 256, periodic Hann, zero boundary, "spectrum" scaling) of the clip itself
//     -> per-bin dB statistics -> threshold = mean + 1.5 std          (noise profile = the signal)
//   STFT of the clip padded with 30000 zeros each side -> dB (floored at per-bin max - 80)
//     -> mask = dB > threshold ? 1 : 1 - p -> separable 33 x 7 triangular smoothing -> X * mask
//     -> inverse FFT, Hann, overlap-add / window-square normalisation -> crop back to the clip.
// The 1024-point FFTs run in LDS (radix-2, 256 threads, bit-reversed load), one block per frame.
//
// Options (ccx_specgate_opts, ccx_specgate_reduce_ex / _reduce_long_ex):
//   * stationary with a separate noise clip (y_noise): the first STFT + statistics pass reads the noise clip instead of the signal
//     (one clip shared by all rows, or one per row); everything after the threshold is the same kernels with the same arguments.
//   * non-stationary (`stationary=False`, noisereduce's SpectralGateNonStationary [UPSTREAM-RECALL], parity unpinned; CPU
//     restatement on scipy.signal.filtfilt: tests/nonstationary_gate_reference.py).  Per padded chunk:
//       A = |X| (sg_stft_kernel<true> writes the amplitude where the stationary instantiation writes dB: no extra matrix)
//       S = filtfilt([b], [1, b - 1], A) along time, b from time_constant_s          (time smoothing, below)
//       M = sigmoid(((A - S) / S - thresh_n_mult) * slope) -> the same 33 x 7 triangle -> M * p + (1 - p)  (scaled AFTER smoothing)
//       -> X * M -> the stationary path's ISTFT and overlap-add.
//     A bin with S == 0 (all-zero row; upstream: 0 / 0 = NaN) takes mask 0: its X is zero, so the output is exactly zero.
//
// Time smoothing -- the one new hot path.  Per (clip, bin) it is a forward first-order recursion f[t] = b A[t] + d f[t-1] (d = 1 - b,
// f[-1] = A[0]; evaluated as f += b (A - f)) and the same recursion backwards over f (S[T] = f[T-1]): 2 x T dependent steps, T up to 2580, and one thread per
// (clip, bin) would leave about one wave per CU walking that chain.  The coefficient is constant, so a segment of L frames acts on
// what follows it as  state_out = d^L * state_in + local,  `local` being the segment scanned from state 0.  Time is cut into
// segments of SG_SEG = 64 frames and every (clip, segment, bin) is one thread (threads of a wave = 64 neighbouring bins of one
// frame: every load and store is a full coalesced line); three launches:
//   1. sg_smooth_fwd_local_kernel   `local` of every full segment, forward                      (reads A)
//   2. sg_smooth_mid_kernel         carry-in = Horner over the <= 40 preceding locals (L2-resident, 2 KB per step and block), then
//                                   the true forward recursion of the segment in registers; f is NOT written: the backward
//                                   `local` of the segment is taken from the registers          (reads A)
//   3. sg_smooth_bwd_apply_kernel   recomputes the segment's f from its saved carry-in, Horner over the following backward
//                                   locals, then the true backward recursion                     (reads A, writes S)
// i.e. A is read three times and S written once (4 matrix passes; a stored f would make it 5) and the longest dependent chain is
// 40 + 2 x 64 FMAs instead of 5160.  Three launches rather than one kernel with the carries in LDS: a block that owned all
// segments of its bins would be 9 x B blocks of 41 segment-waves -- more than a block holds -- or would loop over segments and
// bring the serial chain back; the carries are 85 KB per clip and stay in L2 between the launches.  Segment starts are multiples of
// SG_SEG counted from frame 0 in both directions, so a clip's result does not depend on its neighbours in the batch.
#include <math.h>
#include "../../include/ccx.h"
#include "ccx_common.h"
#include "model_store.h"

namespace {

#define SG_N 1024
#define SG_HOP 256
#define SG_BINS 513
#define SG_LD 520       // row stride (bins) of the [frame][bin] matrices
#define SG_PAD 30000

__device__ __forceinline__ void fft1024(float2* s, const float2* __restrict__ tw, int tid, bool inverse) {
  // in-place decimation-in-time on bit-reversed input; 512 butterflies per stage, 2 per thread
  for (int len = 2; len <= SG_N; len <<= 1) {
    const int half = len >> 1, step = SG_N / len;
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int b = tid + 256 * r;
      const int grp = b / half, k = b - grp * half;
      const int i0 = grp * len + k, i1 = i0 + half;
      float2 w = tw[k * step];
      if (inverse) w.y = -w.y;
      const float2 a = s[i0], c = s[i1];
      const float2 t = make_float2(c.x * w.x - c.y * w.y, c.x * w.y + c.y * w.x);
      s[i0] = make_float2(a.x + t.x, a.y + t.y);
      s[i1] = make_float2(a.x - t.x, a.y - t.y);
    }
    __syncthreads();
  }
}

// One block per (frame, clip).  pad = 0 (noise profile pass) or SG_PAD (signal pass).
// Writes dB = 20 log10(|X| + eps) and optionally X.
// `origin` (optional): clip c is the window [origin[c], origin[c] + n_samples[c]) of a longer signal of `total` samples that
// starts at y + c * stride (chunks of one long file: stride 0); samples outside the window but inside the signal are READ
// (noisereduce pads a chunk with its real neighbours, zeros only beyond the ends of the signal).
// AMP (non-stationary mode): `db` receives the amplitude |X| instead; the <false> instantiation is the stationary kernel unchanged.
template <bool AMP>
__global__ __launch_bounds__(256) void sg_stft_kernel(const float* __restrict__ y, long stride, const int* __restrict__ n_samples,
                                                      const int* __restrict__ n_frames, int pad, const float2* __restrict__ tw,
                                                      const float* __restrict__ win, float* __restrict__ db, float2* __restrict__ X,
                                                      long clip_stride_rows, const long* __restrict__ origin, long total) {
  __shared__ float2 s[SG_N];
  const int clip = blockIdx.y, fr = blockIdx.x, tid = threadIdx.x;
  if (fr >= n_frames[clip]) return;
  const long org = origin ? origin[clip] : 0;
  const long n = origin ? total - org : (long)n_samples[clip];     // readable samples counted from the window start
  const float* x = y + (long)clip * stride + org;
  const long base = (long)fr * SG_HOP - SG_N / 2 - pad;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int i = tid + 256 * r;
    const long o = base + i;
    bool in = o >= -org && o < n;
    // A chunk's first and last two frames reach up to 512 samples beyond its 30000 of context, where scipy's STFT of the cut-out
    // chunk sees zeros and the line above reads the signal.  The stationary gate never shows it (those frames' mask stays inside
    // the padding); the non-stationary smoothing STARTS from frame 0 and from the last frame, so there the window is exact.
    if constexpr (AMP) in = in && o >= -(long)pad && o < (long)n_samples[clip] + pad;
    const float v = in ? x[o] * win[i] * (1.0f / 512.0f) : 0.f;
    s[__brev((unsigned)i) >> 22] = make_float2(v, 0.f);
  }
  __syncthreads();
  fft1024(s, tw, tid, false);
  const long row = (long)clip * clip_stride_rows + fr;
  for (int b = tid; b < SG_BINS; b += 256) {
    const float2 v = s[b];
    if constexpr (AMP) db[row * SG_LD + b] = sqrtf(v.x * v.x + v.y * v.y);
    else db[row * SG_LD + b] = 20.0f * log10f(sqrtf(v.x * v.x + v.y * v.y) + 2.220446049250313e-16f);
    if (X) X[row * SG_LD + b] = v;
  }
}

// Per (clip, bin): max over frames; then (noise pass) mean/std of max(dB, max-80) -> thresh, or
// (signal pass) floor = max - 80.  Block = 32 bins x 8 frame groups, coalesced along bins.
__global__ __launch_bounds__(256) void sg_bin_stats_kernel(const float* __restrict__ db, const int* __restrict__ n_frames,
                                                           long clip_stride_rows, float n_std, float* __restrict__ thresh,
                                                           float* __restrict__ floor_out) {
  __shared__ float red[8][32];
  const int clip = blockIdx.y, bl = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int b = blockIdx.x * 32 + bl;
  const int nf = n_frames[clip];
  const float* p = db + (long)clip * clip_stride_rows * SG_LD + b;
  const bool live = b < SG_BINS;
  float mx = -INFINITY;
  if (live) for (int f = grp; f < nf; f += 8) mx = fmaxf(mx, p[(long)f * SG_LD]);
  red[grp][bl] = mx;
  __syncthreads();
  mx = red[0][bl];
#pragma unroll
  for (int g = 1; g < 8; g++) mx = fmaxf(mx, red[g][bl]);
  const float fl = mx - 80.0f;
  __syncthreads();
  if (floor_out) {
    if (live && grp == 0) floor_out[clip * SG_LD + b] = fl;
    return;
  }
  float s = 0.f;
  if (live) for (int f = grp; f < nf; f += 8) s += fmaxf(p[(long)f * SG_LD], fl);
  red[grp][bl] = s;
  __syncthreads();
  s = 0.f;
#pragma unroll
  for (int g = 0; g < 8; g++) s += red[g][bl];
  const float mean = s / (float)nf;
  __syncthreads();
  float q = 0.f;
  if (live) for (int f = grp; f < nf; f += 8) { const float d = fmaxf(p[(long)f * SG_LD], fl) - mean; q += d * d; }
  red[grp][bl] = q;
  __syncthreads();
  q = 0.f;
#pragma unroll
  for (int g = 0; g < 8; g++) q += red[g][bl];
  if (live && grp == 0) thresh[clip * SG_LD + b] = mean + n_std * sqrtf(q / (float)nf);
}

// mask (hard gate scaled by prop_decrease) convolved along bins with the 33-tap triangle.  A block of 128 threads = 128 bins of
// one frame: the 160 mask values it needs (16 bins of halo on either side) are computed once into LDS -- every thread used to
// recompute the mask of all 33 bins of its window from three global arrays.  Same taps in the same order: bit-identical.
__global__ __launch_bounds__(128) void sg_mask_freq_kernel(const float* __restrict__ db, const float* __restrict__ floorv,
                                                           const float* __restrict__ thresh, const int* __restrict__ n_frames,
                                                           long clip_stride_rows, float prop, const float* __restrict__ ff,
                                                           float* __restrict__ tmp) {
  __shared__ float m[160];
  const int clip = blockIdx.z, fr = blockIdx.y, b0 = blockIdx.x * 128, t = threadIdx.x;
  if (fr >= n_frames[clip]) return;                      // block-uniform
  const long row = ((long)clip * clip_stride_rows + fr) * SG_LD;
  for (int i = t; i < 160; i += 128) {
    const int bb = b0 + i - 16;
    float v = 0.f;
    if (bb >= 0 && bb < SG_BINS) {
      const float d = fmaxf(db[row + bb], floorv[clip * SG_LD + bb]);
      v = d > thresh[clip * SG_LD + bb] ? 1.0f : 1.0f - prop;
    }
    m[i] = v;
  }
  __syncthreads();
  const int b = b0 + t;
  if (b >= SG_BINS) return;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 33; i++) {
    const int bb = b + i - 16;
    if (bb >= 0 && bb < SG_BINS) acc += ff[i] * m[t + i];
  }
  tmp[row + b] = acc;
}

// 7-tap triangle along frames, multiply the spectrum in place
__global__ void sg_mask_time_apply_kernel(const float* __restrict__ tmp, const int* __restrict__ n_frames, long clip_stride_rows,
                                          const float* __restrict__ ft, float2* __restrict__ X) {
  const int clip = blockIdx.z, fr = blockIdx.y, b = blockIdx.x * blockDim.x + threadIdx.x;
  const int nf = n_frames[clip];
  if (fr >= nf || b >= SG_BINS) return;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 7; j++) {
    const int f2 = fr + j - 3;
    if (f2 >= 0 && f2 < nf) acc += ft[j] * tmp[((long)clip * clip_stride_rows + f2) * SG_LD + b];
  }
  const long idx = ((long)clip * clip_stride_rows + fr) * SG_LD + b;
  const float2 v = X[idx];
  X[idx] = make_float2(v.x * acc, v.y * acc);
}

// ---- non-stationary mode: time smoothing (structure: header comment) ----------------------------------------------------------
#define SG_SEG 64            // frames of one segment
#define SG_SEG_CAP 41        // segments of one clip: ceil(2580 / 64), 2580 = frame rows of a 600000-sample chunk with its padding
#define SG_MAX_FRAMES 2580

struct sg_pow { float p[SG_SEG + 1]; };   // p[k] = (1 - b)^k, rounded from double on the host

// the forward recursion of one segment from state c; frames at and beyond `len` leave f[i] = 0 and the state alone
__device__ __forceinline__ float sg_seg_forward(const float* __restrict__ p, int len, float b, float c, float (&f)[SG_SEG]) {
  float a[SG_SEG];
#pragma unroll
  for (int i = 0; i < SG_SEG; i++) a[i] = i < len ? p[(long)i * SG_LD] : 0.f;
#pragma unroll
  for (int i = 0; i < SG_SEG; i++) {
    if (i < len) { c = fmaf(b, a[i] - c, c); f[i] = c; }
    else f[i] = 0.f;
  }
  return c;
}

// launch 1: `local` of every segment that has a successor (all of them full), forward from state 0
__global__ __launch_bounds__(128) void sg_smooth_fwd_local_kernel(const float* __restrict__ A, const int* __restrict__ n_frames,
                                                                  long clip_stride_rows, float b, float* __restrict__ part_f) {
  const int clip = blockIdx.z, seg = blockIdx.y, bin = blockIdx.x * 128 + threadIdx.x;
  const int t0 = seg * SG_SEG;
  if (t0 + SG_SEG >= n_frames[clip] || bin >= SG_BINS) return;
  const float* p = A + ((long)clip * clip_stride_rows + t0) * SG_LD + bin;
  float a[SG_SEG];
#pragma unroll
  for (int i = 0; i < SG_SEG; i++) a[i] = p[(long)i * SG_LD];
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < SG_SEG; i++) acc = fmaf(b, a[i] - acc, acc);
  part_f[((long)clip * SG_SEG_CAP + seg) * SG_LD + bin] = acc;
}

// launch 2: forward carry-in of the segment (saved to cf), its forward recursion in registers, its backward `local`; the clip's
// last segment also leaves f[T-1], the state the backward pass starts from
__global__ __launch_bounds__(128) void sg_smooth_mid_kernel(const float* __restrict__ A, const int* __restrict__ n_frames,
                                                            long clip_stride_rows, float b, float dL,
                                                            const float* __restrict__ part_f, float* __restrict__ cf,
                                                            float* __restrict__ part_b, float* __restrict__ f_last) {
  const int clip = blockIdx.z, seg = blockIdx.y, bin = blockIdx.x * 128 + threadIdx.x;
  const int nf = n_frames[clip], t0 = seg * SG_SEG;
  if (t0 >= nf || bin >= SG_BINS) return;
  const int len = nf - t0 < SG_SEG ? nf - t0 : SG_SEG;
  const float* a0 = A + (long)clip * clip_stride_rows * SG_LD + bin;
  const long cbase = (long)clip * SG_SEG_CAP * SG_LD + bin;
  float c = a0[0];                                          // f[-1] = A[0]: lfilter_zi of this filter is 1 - b
  for (int j = 0; j < seg; j++) c = fmaf(c, dL, part_f[cbase + (long)j * SG_LD]);
  cf[cbase + (long)seg * SG_LD] = c;
  float f[SG_SEG];
  c = sg_seg_forward(a0 + (long)t0 * SG_LD, len, b, c, f);
  if (t0 + len == nf) f_last[clip * SG_LD + bin] = c;
  float acc = 0.f;                                          // the zeros beyond `len` keep the state at 0 until the first real frame
#pragma unroll
  for (int i = SG_SEG - 1; i >= 0; i--) acc = fmaf(b, f[i] - acc, acc);
  part_b[cbase + (long)seg * SG_LD] = acc;
}

// launch 3: the segment's f again (same code, same carry-in: the same bits), the backward carry-in from the segments after it, the
// backward recursion.  Frames at and beyond n_frames are not written.
__global__ __launch_bounds__(128) void sg_smooth_bwd_apply_kernel(const float* __restrict__ A, const int* __restrict__ n_frames,
                                                                  long clip_stride_rows, float b, sg_pow pw,
                                                                  const float* __restrict__ cf, const float* __restrict__ part_b,
                                                                  const float* __restrict__ f_last, float* __restrict__ S) {
  const int clip = blockIdx.z, seg = blockIdx.y, bin = blockIdx.x * 128 + threadIdx.x;
  const int nf = n_frames[clip], t0 = seg * SG_SEG;
  if (t0 >= nf || bin >= SG_BINS) return;
  const int len = nf - t0 < SG_SEG ? nf - t0 : SG_SEG;
  const long cbase = (long)clip * SG_SEG_CAP * SG_LD + bin;
  const long off = ((long)clip * clip_stride_rows + t0) * SG_LD + bin;
  float f[SG_SEG];
  sg_seg_forward(A + off, len, b, cf[cbase + (long)seg * SG_LD], f);
  const int last = (nf - 1) / SG_SEG;
  float g = f_last[clip * SG_LD + bin];                     // S[T] = f[T-1]
  if (seg < last) {
    g = fmaf(g, pw.p[nf - last * SG_SEG], part_b[cbase + (long)last * SG_LD]);        // through the (short) last segment
    for (int j = last - 1; j > seg; j--) g = fmaf(g, pw.p[SG_SEG], part_b[cbase + (long)j * SG_LD]);
  }
  float* s = S + off;
#pragma unroll
  for (int i = SG_SEG - 1; i >= 0; i--)
    if (i < len) { g = fmaf(b, f[i] - g, g); s[(long)i * SG_LD] = g; }
}

__device__ __forceinline__ float sg_sigmoid_mask(float a, float s, float thr, float slope) {
  if (!(s > 0.f)) return 0.f;                               // all-zero bin: upstream divides 0 by 0; X is zero there, any finite mask does
  const float r = fminf((a - s) / s, 3.0e38f);
  return 1.0f / (1.0f + expf(-(r - thr) * slope));
}

// sibling of sg_mask_freq_kernel: the sigmoid mask of (A, S), staged in LDS the same way, convolved along bins
__global__ __launch_bounds__(128) void sg_ns_mask_freq_kernel(const float* __restrict__ A, const float* __restrict__ S,
                                                              const int* __restrict__ n_frames, long clip_stride_rows, float thr,
                                                              float slope, const float* __restrict__ ff, float* __restrict__ tmp) {
  __shared__ float m[160];
  const int clip = blockIdx.z, fr = blockIdx.y, b0 = blockIdx.x * 128, t = threadIdx.x;
  if (fr >= n_frames[clip]) return;                      // block-uniform
  const long row = ((long)clip * clip_stride_rows + fr) * SG_LD;
  for (int i = t; i < 160; i += 128) {
    const int bb = b0 + i - 16;
    m[i] = (bb >= 0 && bb < SG_BINS) ? sg_sigmoid_mask(A[row + bb], S[row + bb], thr, slope) : 0.f;
  }
  __syncthreads();
  const int b = b0 + t;
  if (b >= SG_BINS) return;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 33; i++) {
    const int bb = b + i - 16;
    if (bb >= 0 && bb < SG_BINS) acc += ff[i] * m[t + i];
  }
  tmp[row + b] = acc;
}

// sibling of sg_mask_time_apply_kernel: prop_decrease scales the SMOOTHED mask
__global__ void sg_ns_mask_time_apply_kernel(const float* __restrict__ tmp, const int* __restrict__ n_frames, long clip_stride_rows,
                                             const float* __restrict__ ft, float prop, float2* __restrict__ X) {
  const int clip = blockIdx.z, fr = blockIdx.y, b = blockIdx.x * blockDim.x + threadIdx.x;
  const int nf = n_frames[clip];
  if (fr >= nf || b >= SG_BINS) return;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 7; j++) {
    const int f2 = fr + j - 3;
    if (f2 >= 0 && f2 < nf) acc += ft[j] * tmp[((long)clip * clip_stride_rows + f2) * SG_LD + b];
  }
  acc = acc * prop + (1.0f - prop);
  const long idx = ((long)clip * clip_stride_rows + fr) * SG_LD + b;
  const float2 v = X[idx];
  X[idx] = make_float2(v.x * acc, v.y * acc);
}

// inverse FFT of one masked frame -> windowed time-domain frame [1024]
__global__ __launch_bounds__(256) void sg_istft_kernel(const float2* __restrict__ X, const int* __restrict__ n_frames,
                                                       long clip_stride_rows, const float2* __restrict__ tw, const float* __restrict__ win,
                                                       float* __restrict__ td) {
  __shared__ float2 s[SG_N];
  const int clip = blockIdx.y, fr = blockIdx.x, tid = threadIdx.x;
  if (fr >= n_frames[clip]) return;
  const long row = (long)clip * clip_stride_rows + fr;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int i = tid + 256 * r;
    float2 v;
    if (i <= 512) v = X[row * SG_LD + i];
    else { v = X[row * SG_LD + (SG_N - i)]; v.y = -v.y; }   // Hermitian extension of the one-sided spectrum
    if (i == 0 || i == 512) v.y = 0.f;
    s[__brev((unsigned)i) >> 22] = v;
  }
  __syncthreads();
  fft1024(s, tw, tid, true);
  // irfft scaling 1/N times sum(win) = 512 ("spectrum" scaling undone), then the synthesis window
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int i = tid + 256 * r;
    td[row * SG_N + i] = s[i].x * (512.0f / 1024.0f) * win[i];
  }
}

// overlap-add, divide by the overlap-added squared window, crop the zero padding away
__global__ void sg_overlap_add_kernel(const float* __restrict__ td, const int* __restrict__ n_samples, const int* __restrict__ n_frames,
                                      long clip_stride_rows, const float* __restrict__ win, float* __restrict__ out, long stride,
                                      const long* __restrict__ origin, long span) {
  const int clip = blockIdx.y;
  const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = n_samples[clip];
  if (origin) {                                    // chunk of a long signal: only the chunk's own samples are written
    if (o >= n) return;
    out += origin[clip];
  }
  if (o >= span) return;
  float v = 0.f;
  if (o < n) {
    const int nf = n_frames[clip];
    const long t_out = o + SG_PAD;                 // index in the istft output (boundary already removed)
    if (t_out < (long)(nf - 1) * SG_HOP) {
      const long q = t_out + SG_N / 2;             // index in the boundary-extended signal
      const int j_hi = (int)(q / SG_HOP);
      float num = 0.f, den = 0.f;
#pragma unroll
      for (int d = 0; d < 4; d++) {
        const int j = j_hi - d;
        const long i = q - (long)j * SG_HOP;
        if (j >= 0 && j < nf && i < SG_N) {
          num += td[((long)clip * clip_stride_rows + j) * SG_N + i];
          den += win[i] * win[i];
        }
      }
      v = den > 1e-10f ? num / den : num;
    }
  }
  out[(long)clip * stride + o] = v;
}

}  // namespace

struct ccx_specgate {
  ccx_ctx* ctx = nullptr;
  int max_clips = 0;
  long max_samples = 0, rows = 0;  // rows = frame capacity per clip
  ccx_dev_store store{"specgate"};
  float2* tw = nullptr; float* win = nullptr; float* ff = nullptr; float* ft = nullptr;
  float *db = nullptr, *tmp = nullptr, *td = nullptr, *thresh = nullptr, *floorv = nullptr;
  float2* X = nullptr;
  int *n_dev = nullptr, *nf_noise = nullptr, *nf_sig = nullptr;
  long* origin = nullptr;          // reduce_long: first sample of each chunk
  int clip_noise = 1;              // reduce_long: noise statistics from the first 600000 samples only (noisereduce's clip_noise_stationary)
  int* nn_dev = nullptr;           // samples of each noise clip (n_dev holds the signal's)
  // non-stationary mode, allocated at its first use: S [rows x max_clips][SG_LD] and the carries of the time smoothing
  float* smooth = nullptr;
  float *part_f = nullptr, *part_b = nullptr, *cf = nullptr, *f_last = nullptr;
};

namespace {

// FFT twiddles, Hann window, smoothing ramps and every workspace of `g`
int specgate_build(ccx_specgate* g) {
  std::vector<float2> tw(512);
  std::vector<float> win(SG_N), ff(33), ft(7);
  for (int k = 0; k < 512; k++) { const double a = -2.0 * M_PI * k / SG_N; tw[k] = make_float2((float)cos(a), (float)sin(a)); }
  for (int i = 0; i < SG_N; i++) win[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * i / SG_N));
  // triangular ramps of noisereduce's _smoothing_filter: n_grad_freq = int(500 / (sr / 512)) = 16, n_grad_time = int(50 / 16) = 3
  auto tri = [](int n, float* dst) {
    std::vector<double> v;
    for (int i = 0; i < n + 1; i++) v.push_back((double)i / (n + 1));            // linspace(0,1,n+1,endpoint=False)
    for (int i = 0; i < n + 2; i++) v.push_back(1.0 - (double)i / (n + 1));        // linspace(1,0,n+2)
    double s = 0;
    for (size_t i = 1; i + 1 < v.size(); i++) s += v[i];
    for (size_t i = 1; i + 1 < v.size(); i++) dst[i - 1] = (float)(v[i] / s);
  };
  tri(16, ff.data());
  tri(3, ft.data());
  ccx_dev_store& st = g->store;
  CCX_TRY(st.upload(&g->tw, tw)); CCX_TRY(st.upload(&g->win, win)); CCX_TRY(st.upload(&g->ff, ff)); CCX_TRY(st.upload(&g->ft, ft));
  const size_t R = (size_t)g->rows * g->max_clips, C = (size_t)g->max_clips;
  CCX_TRY(st.alloc(&g->db, R * SG_LD, true)); CCX_TRY(st.alloc(&g->tmp, R * SG_LD, true)); CCX_TRY(st.alloc(&g->X, R * SG_LD, true));
  CCX_TRY(st.alloc(&g->td, R * SG_N, true));
  CCX_TRY(st.alloc(&g->thresh, C * SG_LD, true)); CCX_TRY(st.alloc(&g->floorv, C * SG_LD, true));
  CCX_TRY(st.alloc(&g->n_dev, C, true)); CCX_TRY(st.alloc(&g->nf_noise, C, true)); CCX_TRY(st.alloc(&g->nf_sig, C, true));
  CCX_TRY(st.alloc(&g->nn_dev, C, true));
  return CCX_OK;
}

int specgate_smooth_build(ccx_specgate* g, bool with_S) {
  ccx_dev_store& st = g->store;
  const size_t P = (size_t)g->max_clips * SG_SEG_CAP * SG_LD;
  if (!g->part_f) CCX_TRY(st.alloc(&g->part_f, P, true));
  if (!g->part_b) CCX_TRY(st.alloc(&g->part_b, P, true));
  if (!g->cf) CCX_TRY(st.alloc(&g->cf, P, true));
  if (!g->f_last) CCX_TRY(st.alloc(&g->f_last, (size_t)g->max_clips * SG_LD, true));
  if (with_S && !g->smooth) CCX_TRY(st.alloc(&g->smooth, (size_t)g->rows * g->max_clips * SG_LD, true));
  return CCX_OK;
}

// the three launches of the time smoothing over B clips of at most max_nf <= SG_MAX_FRAMES frames (nf_dev: frames per clip)
int specgate_time_smooth(ccx_specgate* g, const float* A, float* S, const int* nf_dev, int max_nf, int B, long rows, double b,
                         hipStream_t st) {
  ccx_ctx* ctx = g->ctx;
  // The recursion runs as f += b (A - f): unit gain whatever the rounding of b (with d = 1 - b rounded on its own, b + d misses 1
  // by up to 3e-8 and a constant row comes out 3e-8 / b = 4e-6 off).  The carries decay by the powers of 1 - (that fp32 b).
  const float bf = (float)b;
  sg_pow pw;
  for (int k = 0; k <= SG_SEG; k++) pw.p[k] = (float)pow(1.0 - (double)bf, (double)k);
  const dim3 grid(ccx_cdiv(SG_BINS, 128), ccx_cdiv(max_nf, SG_SEG), B);
  const double mat = 4.0 * B * (double)max_nf * SG_BINS;     // bytes of one pass over the matrix
  {
    ccx_prof_scope ps(ctx, st, "sg_smooth_fwd_local_kernel", 3.0 * mat / 4, mat);
    hipLaunchKernelGGL(sg_smooth_fwd_local_kernel, grid, dim3(128), 0, st, A, nf_dev, rows, bf, g->part_f);
  }
  CCX_CHECK_LAUNCH(ctx);
  {
    ccx_prof_scope ps(ctx, st, "sg_smooth_mid_kernel", 6.0 * mat / 4, mat);
    hipLaunchKernelGGL(sg_smooth_mid_kernel, grid, dim3(128), 0, st, A, nf_dev, rows, bf, pw.p[SG_SEG], (const float*)g->part_f, g->cf,
                       g->part_b, g->f_last);
  }
  CCX_CHECK_LAUNCH(ctx);
  {
    ccx_prof_scope ps(ctx, st, "sg_smooth_bwd_apply_kernel", 6.0 * mat / 4, 2.0 * mat);
    hipLaunchKernelGGL(sg_smooth_bwd_apply_kernel, grid, dim3(128), 0, st, A, nf_dev, rows, bf, pw, (const float*)g->cf,
                       (const float*)g->part_b, (const float*)g->f_last, S);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

// one call's options after the host checks
struct sg_run {
  bool stationary;
  float prop, n_std, thr, slope;
  double b;                        // coefficient of the time smoothing
};

int specgate_check_opts(ccx_specgate* g, const char* who, const ccx_specgate_opts* o, int B, long noise_cap, sg_run* r) {
  ccx_ctx* ctx = g->ctx;
  CCX_REQUIRE(ctx, o != nullptr, "%s: opts is NULL", who);
  CCX_REQUIRE(ctx, std::isfinite(o->prop_decrease), "%s: prop_decrease is not finite", who);
  CCX_REQUIRE(ctx, std::isfinite(o->n_std_thresh), "%s: n_std_thresh is not finite", who);
  CCX_REQUIRE(ctx, std::isfinite(o->time_constant_s) && o->time_constant_s > 0.f, "%s: time_constant_s = %g must be positive", who, (double)o->time_constant_s);
  CCX_REQUIRE(ctx, std::isfinite(o->thresh_n_mult), "%s: thresh_n_mult is not finite", who);
  CCX_REQUIRE(ctx, std::isfinite(o->sigmoid_slope), "%s: sigmoid_slope is not finite", who);
  CCX_REQUIRE(ctx, o->noise_rows == 0 || o->noise_rows == 1 || o->noise_rows == B, "%s: noise_rows = %d must be 0, 1 or B = %d", who, o->noise_rows, B);
  if (o->noise_rows > 0) {
    CCX_REQUIRE(ctx, o->noise_dev != nullptr && o->n_noise != nullptr, "%s: noise_rows = %d but noise_dev or n_noise is NULL", who, o->noise_rows);
    for (int i = 0; i < o->noise_rows; i++) {
      CCX_REQUIRE(ctx, o->n_noise[i] >= 1 && o->n_noise[i] <= noise_cap, "%s: n_noise[%d] = %d out of range [1, %ld]", who, i, o->n_noise[i], noise_cap);
      CCX_REQUIRE(ctx, o->noise_rows == 1 || o->n_noise[i] <= o->noise_stride, "%s: n_noise[%d] = %d exceeds noise_stride = %ld", who, i, o->n_noise[i], (long)o->noise_stride);
    }
  }
  r->stationary = o->stationary != 0;
  r->prop = o->prop_decrease; r->n_std = o->n_std_thresh; r->thr = o->thresh_n_mult; r->slope = o->sigmoid_slope;
  const double t = (double)o->time_constant_s * 16000.0 / SG_HOP;
  r->b = (sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t);
  return CCX_OK;
}

// noise pass: unpadded STFT of `nclips` clips -> per-bin threshold rows 0 .. nclips-1 (n_dev_: samples, g->nf_noise: frames per clip)
int specgate_noise_pass(ccx_specgate* g, const float* y, long stride, const int* n_dev_, int nclips, int max_fn, long rows, float n_std,
                        hipStream_t st) {
  ccx_ctx* ctx = g->ctx;
  {
    ccx_prof_scope ps(ctx, st, "sg_stft_kernel", 5.0 * SG_N * 10 * max_fn * nclips, 4.0 * nclips * (double)max_fn * (SG_HOP + SG_BINS));
    hipLaunchKernelGGL((sg_stft_kernel<false>), dim3(max_fn, nclips), dim3(256), 0, st, y, stride, n_dev_, (const int*)g->nf_noise, 0,
                       (const float2*)g->tw, (const float*)g->win, g->db, (float2*)nullptr, rows, (const long*)nullptr, 0L);
  }
  CCX_CHECK_LAUNCH(ctx);
  {
    ccx_prof_scope ps(ctx, st, "sg_bin_stats_kernel", 0.0, 3.0 * 4.0 * nclips * (double)max_fn * SG_BINS);
    hipLaunchKernelGGL(sg_bin_stats_kernel, dim3(ccx_cdiv(SG_BINS, 32), nclips), dim3(256), 0, st, g->db, g->nf_noise, rows, n_std, g->thresh,
                       (float*)nullptr);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

// signal pass of nb clips (or chunks of one long signal: origin / total): padded STFT -> mask -> X * mask -> ISTFT -> overlap-add.
// g->n_dev / g->nf_sig hold the clips' samples / frames; stationary mode reads g->thresh rows 0 .. nb-1.
int specgate_gate_clips(ccx_specgate* g, const sg_run& r, const float* y, long stride, int nb, int max_fs, long rows, const long* origin,
                        long total, float* out, long out_stride, int oa_len, hipStream_t st) {
  ccx_ctx* ctx = g->ctx;
  const double mat = 4.0 * nb * (double)max_fs * SG_BINS;
  const double stft_flops = 5.0 * SG_N * 10 * max_fs * nb, stft_bytes = 4.0 * nb * (double)max_fs * SG_HOP + 3.0 * mat;
  const dim3 mgrid(ccx_cdiv(SG_BINS, 128), max_fs, nb);
  if (r.stationary) {
    {
      ccx_prof_scope ps(ctx, st, "sg_stft_kernel", stft_flops, stft_bytes);
      hipLaunchKernelGGL((sg_stft_kernel<false>), dim3(max_fs, nb), dim3(256), 0, st, y, stride, (const int*)g->n_dev, (const int*)g->nf_sig,
                         SG_PAD, (const float2*)g->tw, (const float*)g->win, g->db, g->X, rows, origin, total);
    }
    CCX_CHECK_LAUNCH(ctx);
    {
      ccx_prof_scope ps(ctx, st, "sg_bin_stats_kernel", 0.0, mat);
      hipLaunchKernelGGL(sg_bin_stats_kernel, dim3(ccx_cdiv(SG_BINS, 32), nb), dim3(256), 0, st, g->db, g->nf_sig, rows, 0.f, (float*)nullptr,
                         g->floorv);
    }
    CCX_CHECK_LAUNCH(ctx);
    {
      ccx_prof_scope ps(ctx, st, "sg_mask_freq_kernel", 66.0 * mat / 4, 2.0 * mat);
      hipLaunchKernelGGL(sg_mask_freq_kernel, mgrid, dim3(128), 0, st, g->db, g->floorv, g->thresh, g->nf_sig, rows, r.prop, g->ff, g->tmp);
    }
    CCX_CHECK_LAUNCH(ctx);
    {
      ccx_prof_scope ps(ctx, st, "sg_mask_time_apply_kernel", 16.0 * mat / 4, 5.0 * mat);
      hipLaunchKernelGGL(sg_mask_time_apply_kernel, mgrid, dim3(128), 0, st, g->tmp, g->nf_sig, rows, g->ft, g->X);
    }
    CCX_CHECK_LAUNCH(ctx);
  } else {
    CCX_TRY(specgate_smooth_build(g, true));
    {
      ccx_prof_scope ps(ctx, st, "sg_stft_kernel<amp>", stft_flops, stft_bytes);
      hipLaunchKernelGGL((sg_stft_kernel<true>), dim3(max_fs, nb), dim3(256), 0, st, y, stride, (const int*)g->n_dev, (const int*)g->nf_sig,
                         SG_PAD, (const float2*)g->tw, (const float*)g->win, g->db, g->X, rows, origin, total);
    }
    CCX_CHECK_LAUNCH(ctx);
    CCX_TRY(specgate_time_smooth(g, g->db, g->smooth, g->nf_sig, max_fs, nb, rows, r.b, st));
    {
      ccx_prof_scope ps(ctx, st, "sg_ns_mask_freq_kernel", 66.0 * mat / 4, 3.0 * mat);
      hipLaunchKernelGGL(sg_ns_mask_freq_kernel, mgrid, dim3(128), 0, st, g->db, g->smooth, g->nf_sig, rows, r.thr, r.slope, g->ff, g->tmp);
    }
    CCX_CHECK_LAUNCH(ctx);
    {
      ccx_prof_scope ps(ctx, st, "sg_ns_mask_time_apply_kernel", 18.0 * mat / 4, 5.0 * mat);
      hipLaunchKernelGGL(sg_ns_mask_time_apply_kernel, mgrid, dim3(128), 0, st, g->tmp, g->nf_sig, rows, g->ft, r.prop, g->X);
    }
    CCX_CHECK_LAUNCH(ctx);
  }
  {
    ccx_prof_scope ps(ctx, st, "sg_istft_kernel", stft_flops, 2.0 * mat + 4.0 * nb * (double)max_fs * SG_N);
    hipLaunchKernelGGL(sg_istft_kernel, dim3(max_fs, nb), dim3(256), 0, st, g->X, g->nf_sig, rows, g->tw, g->win, g->td);
  }
  CCX_CHECK_LAUNCH(ctx);
  {
    ccx_prof_scope ps(ctx, st, "sg_overlap_add_kernel", 0.0, 4.0 * nb * (double)max_fs * SG_N + 4.0 * nb * (double)oa_len);
    hipLaunchKernelGGL(sg_overlap_add_kernel, dim3(ccx_cdiv(oa_len, 256), nb), dim3(256), 0, st, g->td, g->n_dev, g->nf_sig, rows, g->win, out,
                       out_stride, origin, (long)oa_len);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_specgate_create(ccx_ctx* ctx, int64_t max_samples, int max_clips, int sample_rate, ccx_specgate** out) {
  if (!ctx) return CCX_ERR_ARG;
  CCX_REQUIRE(ctx, out && max_clips >= 1 && max_samples >= 1, "ccx_specgate_create: bad arguments");
  CCX_REQUIRE(ctx, max_samples <= 600000, "specgate: clips longer than one 600000-sample chunk are not supported (hot path feeds <= 30 s)");
  CCX_REQUIRE(ctx, sample_rate == 16000, "specgate: smoothing widths are built for 16 kHz");
  ccx_specgate* g = new ccx_specgate();
  g->ctx = ctx; g->store.ctx = ctx; g->max_clips = max_clips; g->max_samples = max_samples;
  g->rows = (max_samples + 2 * SG_PAD) / SG_HOP + 2;
  const int rc = specgate_build(g);
  if (rc) {                      // the caller never sees a half-built handle: free it and what it already owns
    ccx_specgate_destroy(g);
    return rc;
  }
  *out = g;
  return CCX_OK;
}

void ccx_specgate_destroy(ccx_specgate* g) {
  if (!g) return;
  g->store.free_all();
  delete g;
}

void ccx_specgate_opts_default(ccx_specgate_opts* o) {
  if (!o) return;
  o->stationary = 1;
  o->prop_decrease = 1.0f; o->n_std_thresh = 1.5f; o->time_constant_s = 2.0f; o->thresh_n_mult = 2.0f; o->sigmoid_slope = 10.0f;
  o->noise_dev = nullptr; o->noise_stride = 0; o->n_noise = nullptr; o->noise_rows = 0;
}

int ccx_specgate_reduce_ex(ccx_specgate* g, const ccx_specgate_opts* opts, const float* y, int64_t stride, const int* n_samples, int B,
                           float* out, void* stream_) {
  if (!g) return CCX_ERR_ARG;
  ccx_ctx* ctx = g->ctx;
  hipStream_t st = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, y && out && n_samples && B >= 1 && B <= g->max_clips, "specgate_reduce: bad arguments (B=%d, max %d)", B, g->max_clips);
  sg_run r;
  CCX_TRY(specgate_check_opts(g, "specgate_reduce", opts, B, g->max_samples, &r));
  const int NR = opts->noise_rows;                          // noise clips: the signal's rows themselves when 0
  const int nclips = NR ? NR : B;
  const int* nn = NR ? opts->n_noise : n_samples;
  std::vector<int> nfn(nclips), nfs(B);
  int max_fn = 0, max_fs = 0;
  for (int b = 0; b < B; b++) {
    CCX_REQUIRE(ctx, n_samples[b] >= 1 && n_samples[b] <= stride && n_samples[b] <= g->max_samples, "specgate_reduce: clip %d has %d samples (capacity %ld)", b, n_samples[b], g->max_samples);
    nfs[b] = 1 + (n_samples[b] + 2 * SG_PAD) / SG_HOP;
    max_fs = nfs[b] > max_fs ? nfs[b] : max_fs;
  }
  for (int b = 0; b < nclips; b++) {
    nfn[b] = 1 + nn[b] / SG_HOP;                             // scipy.signal.stft, boundary zeros, padded=False
    max_fn = nfn[b] > max_fn ? nfn[b] : max_fn;
  }
  CCX_HIP(ctx, hipMemcpyAsync(g->n_dev, n_samples, B * 4, hipMemcpyHostToDevice, st));
  CCX_HIP(ctx, hipMemcpyAsync(g->nf_sig, nfs.data(), B * 4, hipMemcpyHostToDevice, st));
  if (r.stationary) {
    if (NR) CCX_HIP(ctx, hipMemcpyAsync(g->nn_dev, nn, nclips * 4, hipMemcpyHostToDevice, st));
    CCX_HIP(ctx, hipMemcpyAsync(g->nf_noise, nfn.data(), nclips * 4, hipMemcpyHostToDevice, st));
  }
  CCX_HIP(ctx, hipStreamSynchronize(st));
  const long rows = g->rows;
  if (r.stationary) {                                        // the non-stationary mode has no noise profile: a noise clip is ignored
    CCX_TRY(specgate_noise_pass(g, NR ? opts->noise_dev : y, NR ? (NR == 1 ? 0L : (long)opts->noise_stride) : (long)stride, NR ? g->nn_dev : g->n_dev, nclips,
                                max_fn, rows, r.n_std, st));
    for (int k = nclips; k < B; k++)                         // one shared noise clip: every row reads its threshold
      CCX_HIP(ctx, hipMemcpyAsync(g->thresh + (size_t)k * SG_LD, g->thresh, SG_LD * 4, hipMemcpyDeviceToDevice, st));
  }
  return specgate_gate_clips(g, r, y, (long)stride, B, max_fs, rows, (const long*)nullptr, 0L, out, (long)stride, (int)stride, st);
}

int ccx_specgate_reduce(ccx_specgate* g, const float* y, int64_t stride, const int* n_samples, int B, float prop_decrease,
                        float* out, void* stream_) {
  ccx_specgate_opts o;
  ccx_specgate_opts_default(&o);
  o.prop_decrease = prop_decrease;
  return ccx_specgate_reduce_ex(g, &o, y, stride, n_samples, B, out, stream_);
}

// One signal of any length the workspace holds: noisereduce's chunked path (chunk_size 600000, padding 30000).  The threshold
// comes from the noise clip, which is the signal itself (y_noise = None) or the caller's -- cut to its FIRST chunk_size samples when
// clip_noise_stationary is on (noisereduce's default; ccx_specgate_set_clip_noise(g, 0) takes the whole clip instead: the package
// is not importable here and the reference holds no fixture, so which of the two upstream does is parity unpinned) --; every
// 600000-sample chunk is then gated on its own -- padded with 30000 real neighbour samples on each side (zeros beyond the ends of the signal), its dB floor (max - 80)
// taken per chunk -- and only the chunk's own samples are written.  Chunks are processed as the "clips" of the batched kernels.
// The non-stationary mode has no threshold pass; its chunks are smoothed and gated one by one in the same way.
int ccx_specgate_set_clip_noise(ccx_specgate* g, int on) {
  if (!g) return CCX_ERR_ARG;
  g->clip_noise = on ? 1 : 0;
  return CCX_OK;
}

int ccx_specgate_reduce_long_ex(ccx_specgate* g, const ccx_specgate_opts* opts, const float* y, int64_t n, float* out, void* stream_) {
  if (!g) return CCX_ERR_ARG;
  ccx_ctx* ctx = g->ctx;
  hipStream_t st = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, y && out && n >= 1, "specgate_reduce_long: bad arguments");
  const long CH = 600000;
  const long R = g->rows * g->max_clips;                 // frame rows of the workspace
  sg_run r;
  CCX_TRY(specgate_check_opts(g, "specgate_reduce_long", opts, 1, (R - 1) * SG_HOP, &r));
  const bool own_noise = opts->noise_rows == 1;
  const long n_src = own_noise ? (long)opts->n_noise[0] : (long)n;
  const long nfn = r.stationary ? 1 + n_src / SG_HOP : 1;
  const long rows_c = (CH + 2 * SG_PAD) / SG_HOP + 2;
  CCX_REQUIRE(ctx, nfn <= R && rows_c <= R, "specgate_reduce_long: %ld samples need %ld frame rows, the workspace holds %ld (max_samples x max_clips)", (long)n, nfn > rows_c ? nfn : rows_c, R);
  CCX_REQUIRE(ctx, n < (1L << 31) - CH, "specgate_reduce_long: signal too long");
  if (!g->origin) CCX_TRY(g->store.alloc(&g->origin, (size_t)g->max_clips, true));
  const long nchunks = (n + CH - 1) / CH;
  long per = R / rows_c;
  if (per > g->max_clips) per = g->max_clips;
  if (r.stationary) {
    // ---- threshold from the noise clip (the signal itself unless the caller gave one), cut to its first chunk when
    // clip_noise_stationary is on (one "clip" that owns all rows) ----
    const long n_noise = (g->clip_noise && n_src > CH) ? CH : n_src;
    const int n_i = (int)n_noise, nfn_i = (int)(1 + n_noise / SG_HOP);
    CCX_HIP(ctx, hipMemcpyAsync(g->nn_dev, &n_i, 4, hipMemcpyHostToDevice, st));
    CCX_HIP(ctx, hipMemcpyAsync(g->nf_noise, &nfn_i, 4, hipMemcpyHostToDevice, st));
    CCX_HIP(ctx, hipStreamSynchronize(st));
    CCX_TRY(specgate_noise_pass(g, own_noise ? opts->noise_dev : y, 0L, g->nn_dev, 1, nfn_i, R, r.n_std, st));
    for (int k = 1; k < per && k < nchunks; k++)           // every chunk clip reads the signal's threshold row
      CCX_HIP(ctx, hipMemcpyAsync(g->thresh + (size_t)k * SG_LD, g->thresh, SG_LD * 4, hipMemcpyDeviceToDevice, st));
  }
  // ---- chunks, as many at a time as the workspace holds ----
  for (long c0 = 0; c0 < nchunks; c0 += per) {
    const int nb = (int)((nchunks - c0 < per) ? nchunks - c0 : per);
    std::vector<int> len(nb), nfs(nb);
    std::vector<long> org(nb);
    int max_fs = 0, max_len = 0;
    for (int k = 0; k < nb; k++) {
      org[k] = (c0 + k) * CH;
      len[k] = (int)((n - org[k] < CH) ? n - org[k] : CH);
      nfs[k] = 1 + (len[k] + 2 * SG_PAD) / SG_HOP;
      max_fs = nfs[k] > max_fs ? nfs[k] : max_fs;
      max_len = len[k] > max_len ? len[k] : max_len;
    }
    CCX_HIP(ctx, hipMemcpyAsync(g->n_dev, len.data(), nb * 4, hipMemcpyHostToDevice, st));
    CCX_HIP(ctx, hipMemcpyAsync(g->nf_sig, nfs.data(), nb * 4, hipMemcpyHostToDevice, st));
    CCX_HIP(ctx, hipMemcpyAsync(g->origin, org.data(), nb * 8, hipMemcpyHostToDevice, st));
    CCX_HIP(ctx, hipStreamSynchronize(st));
    CCX_TRY(specgate_gate_clips(g, r, y, 0L, nb, max_fs, rows_c, (const long*)g->origin, (long)n, out, 0L, max_len, st));
  }
  return CCX_OK;
}

int ccx_specgate_reduce_long(ccx_specgate* g, const float* y, int64_t n, float prop_decrease, float* out, void* stream_) {
  ccx_specgate_opts o;
  ccx_specgate_opts_default(&o);
  o.prop_decrease = prop_decrease;
  return ccx_specgate_reduce_long_ex(g, &o, y, n, out, stream_);
}

// The product's smoothing launches on a caller's matrices (kernel parity tests): a_dev / s_dev [B][clip_stride_rows][520] f32.
int ccx_specgate_time_smooth(ccx_specgate* g, const float* a_dev, float* s_dev, const int* n_frames, int B, int64_t clip_stride_rows,
                             float b, void* stream_) {
  if (!g) return CCX_ERR_ARG;
  ccx_ctx* ctx = g->ctx;
  hipStream_t st = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, a_dev && s_dev && a_dev != s_dev && n_frames, "ccx_specgate_time_smooth: a_dev, s_dev or n_frames is NULL, or s_dev aliases a_dev");
  CCX_REQUIRE(ctx, B >= 1 && B <= g->max_clips, "ccx_specgate_time_smooth: B = %d out of range [1, max_clips = %d]", B, g->max_clips);
  CCX_REQUIRE(ctx, b > 0.f && b <= 1.f, "ccx_specgate_time_smooth: b = %g out of range (0, 1]", (double)b);
  int max_nf = 0;
  for (int i = 0; i < B; i++) {
    CCX_REQUIRE(ctx, n_frames[i] >= 1 && n_frames[i] <= SG_MAX_FRAMES && n_frames[i] <= clip_stride_rows,
                "ccx_specgate_time_smooth: n_frames[%d] = %d out of range [1, min(%d, clip_stride_rows = %ld)]", i, n_frames[i], SG_MAX_FRAMES, (long)clip_stride_rows);
    max_nf = n_frames[i] > max_nf ? n_frames[i] : max_nf;
  }
  CCX_TRY(specgate_smooth_build(g, false));
  CCX_HIP(ctx, hipMemcpyAsync(g->nf_sig, n_frames, B * 4, hipMemcpyHostToDevice, st));
  CCX_HIP(ctx, hipStreamSynchronize(st));
  CCX_TRY(specgate_time_smooth(g, a_dev, s_dev, g->nf_sig, max_nf, B, (long)clip_stride_rows, (double)b, st));
  CCX_HIP(ctx, hipStreamSynchronize(st));
  return CCX_OK;
}

}  // extern "C"

