// Phase 0 of profiles/dec_full_lines_experiment.txt: do the decode chain's remaining operand streams gain from full-line requests?
// Loads only, values xor-ed into a sink, CU-masked streams (the first N mask bits = N / 8 CUs of every XCD) as in microbench_linehalves.hip.
//  (a) a self-attention K/V stream from HBM: cache [layer][256 rows x 12 heads][Tc = 448][64] bf16, a key or value row is one 128-byte
//      line, a (row, head) owns pos contiguous keys.  A wave takes 64-key pieces (8 K and 8 V instructions, two pieces in flight) as
//      16 keys x 64 B per instruction (half lines: lane -> key l % 16, chunk l / 16, the other half with the next instruction), as
//      8 keys x 128 B (full lines: lane -> key l / 8, chunk l % 8 -- what dec_attention_kernel's loop issues), and the latter with the
//      non-temporal hint.  Launches rotate over 4 layers (0.7 GB), so no launch finds its lines in a cache.
//  (b) the bf16 activation operand of the > 16-row skinny linears out of L2: [256][K] read by NB column blocks x 4 row blocks of
//      4 waves, wave w the k-steps of its quarter of K (K = 768: 6; K = 3072: three z slices of 8), as dec_linear_kernel<4, 2, ., ACT_BF16>
//      asks for them: row-major fragments (16 rows x 64 B per instruction) against a fragment-packed image (tile (m / 16, k / 32) =
//      64 lanes x 16 B back to back, 1 KB per instruction).  REPS passes per launch; "same" re-reads one matrix (L2 hits after the
//      first pass), "rotate" walks 8 matrices (12 MB at K = 3072: past one XCD's 4 MB L2).
//  (c) (profiles/dec_chain_images_experiment.txt) the same [256][768] operand at the out projections' grid: 24 column blocks x 4 row
//      blocks of 64 rows (dec_linear_kernel<4, 2, 6, ACT_BF16>), and the two ways of filling the chip: 24 x 8 blocks of 32 rows, 24 x 16
//      of 16.
//  (d) one (head, 16 rows) block of the LayerNorm-free query + expansion (dec_xq_lnfree_kernel<768>), 12 heads x 16 row tiles: 64 x 768
//      of Wcq_g and 16 x 768 of xb (24 k-steps each, wave w the head's rows 16 w ..), then WckT's [768][64] head slice (wave w: 12 M
//      tiles x 2 k-steps), row-major as the kernel asked for them against fragment-packed images.
// build: hipcc -w --offload-arch=gfx950 -O3 tools/microbench_dec_lines.hip -o microbench_dec_lines && ./microbench_dec_lines
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
typedef __attribute__((ext_vector_type(4))) unsigned u4;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// FORM 0: half lines, 1: full lines, 2: full lines non-temporal
template <int FORM>
__global__ __launch_bounds__(256) void kv_kernel(const unsigned short* Kc, const unsigned short* Vc, unsigned* sink, int T, int Tc, int npairs) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cpp = (T + 63) >> 6;                      // 64-key pieces per (row, head)
  const int npieces = npairs * cpp, stride = gridDim.x * 4;
  u4 acc = {0, 0, 0, 0};
  u4 img[2][16];
  auto load = [&](u4 (&r)[16], int p) {
    const int pair = p / cpp, base = (p - pair * cpp) * 64;
#pragma unroll
    for (int kv = 0; kv < 2; kv++) {
      const unsigned short* src = (kv ? Vc : Kc) + (long)pair * Tc * 64;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        int key, chunk;
        if (FORM == 0) { key = base + (i >> 1) * 16 + (lane & 15); chunk = (i & 1) * 4 + (lane >> 4); }
        else { key = base + i * 8 + (lane >> 3); chunk = lane & 7; }
        key = key < T ? key : T - 1;
        const u4* a = (const u4*)(src + (long)key * 64 + chunk * 8);
        r[kv * 8 + i] = FORM == 2 ? __builtin_nontemporal_load(a) : *a;
      }
    }
  };
  int p = blockIdx.x * 4 + wave;
  if (p < npieces) load(img[0], p);
  if (p + stride < npieces) load(img[1], p + stride);
  for (; p < npieces; p += 2 * stride) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
      if (p + j * stride < npieces) {
#pragma unroll
        for (int i = 0; i < 16; i++) acc ^= img[j][i];
        if (p + (j + 2) * stride < npieces) load(img[j], p + (j + 2) * stride);
      }
    }
  }
  if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) sink[0] = acc.x;
}

// PACKED 0: row-major fragments, 1: fragment-packed image.  grid (NB, 4, ksplit); KMAX k-steps per wave.
template <int PACKED, int KMAX, int MT = 4>
__global__ __launch_bounds__(256) void act_kernel(const unsigned short* A, unsigned* sink, int K, int reps, long rot_stride) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l15 = lane & 15, h4 = lane >> 4;
  const int ksteps = K >> 5;
  const int ks0 = (blockIdx.z * 4 + wave) * KMAX;
  const int m0 = blockIdx.y * 16 * MT;
  u4 acc = {0, 0, 0, 0};
  for (int r = 0; r < reps; r++) {
    const unsigned short* Ar = A + (long)((r + blockIdx.x) & 7) * rot_stride;
    u4 af[MT][KMAX];
#pragma unroll
    for (int j = 0; j < MT; j++) {
#pragma unroll
      for (int k = 0; k < KMAX; k++) {
        const unsigned short* a = PACKED ? Ar + ((((long)(blockIdx.y * MT + j)) * ksteps + ks0 + k) * 64 + lane) * 8
                                         : Ar + (long)(m0 + 16 * j + l15) * K + 8 * h4 + 32 * (ks0 + k);
        af[j][k] = *(const u4*)a;
      }
    }
#pragma unroll
    for (int j = 0; j < MT; j++)
#pragma unroll
      for (int k = 0; k < KMAX; k++) acc ^= af[j][k];
    if (acc.x == 0x12345678u) sink[1] = r;   // keeps the passes apart
  }
  if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) sink[0] = acc.x;
}

// PACKED 0: the operands row-major (Wq [768][768], xb [256][768], WkT [12][768][64]), 1: their fragment images.  grid (12, 16).
template <int PACKED>
__global__ __launch_bounds__(256) void xq_kernel(const unsigned short* Wq, const unsigned short* xb, const unsigned short* WkT, unsigned* sink, int reps) {
  constexpr int D = 768, NKS = 24, FW = 192, NMT = 12;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  const int h = blockIdx.x, row = blockIdx.y * 16 + n;
  u4 acc = {0, 0, 0, 0};
  for (int r = 0; r < reps; r++) {
    u4 wq[NKS], xr[NKS], wk[NMT][2];
    const unsigned short* wsrc = PACKED ? Wq + ((long)(h * 4 + wave) * NKS * 64 + lane) * 8 : Wq + (long)(h * 64 + wave * 16 + n) * D + g * 8;
    const unsigned short* xsrc = PACKED ? xb + ((long)blockIdx.y * NKS * 64 + lane) * 8 : xb + (long)row * D + g * 8;
    const unsigned short* ksrc = PACKED ? WkT + ((long)h * D + wave * FW) * 64 + lane * 8 : WkT + ((long)h * D + wave * FW + n) * 64 + g * 8;
#pragma unroll
    for (int ks = 0; ks < NKS; ks++) wq[ks] = *(const u4*)(wsrc + ks * (PACKED ? 512 : 32));
#pragma unroll
    for (int ks = 0; ks < NKS; ks++) xr[ks] = *(const u4*)(xsrc + ks * (PACKED ? 512 : 32));
#pragma unroll
    for (int mt = 0; mt < NMT; mt++) {
      wk[mt][0] = *(const u4*)(ksrc + mt * 1024);
      wk[mt][1] = *(const u4*)(ksrc + mt * 1024 + (PACKED ? 512 : 32));
    }
#pragma unroll
    for (int ks = 0; ks < NKS; ks++) acc ^= wq[ks] ^ xr[ks];
#pragma unroll
    for (int mt = 0; mt < NMT; mt++) acc ^= wk[mt][0] ^ wk[mt][1];
    if (acc.x == 0x12345678u) sink[1] = r;   // keeps the passes apart
  }
  if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) sink[0] = acc.x;
}

static float median(std::vector<float>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main() {
  const int ROWS = 256, H = 12, Tc = 448, LAYERS = 4, npairs = ROWS * H;
  const size_t layer_elems = (size_t)npairs * Tc * 64;
  unsigned short *Kc, *Vc, *A; unsigned* sink;
  CHECK(hipMalloc(&Kc, layer_elems * 2 * LAYERS)); CHECK(hipMalloc(&Vc, layer_elems * 2 * LAYERS));
  CHECK(hipMalloc(&A, (size_t)8 * 256 * 3072 * 2)); CHECK(hipMalloc(&sink, 8));
  CHECK(hipMemset(Kc, 1, layer_elems * 2 * LAYERS)); CHECK(hipMemset(Vc, 2, layer_elems * 2 * LAYERS)); CHECK(hipMemset(A, 3, (size_t)8 * 256 * 3072 * 2));
  hipEvent_t ea, eb; CHECK(hipEventCreate(&ea)); CHECK(hipEventCreate(&eb));
  const char* kv_names[3] = {"half lines   ", "full lines   ", "full lines nt"};
  for (int pass = 0; pass < 2; pass++) {          // everything twice: the spread of repeated runs of one form
    printf("== pass %d ==\n", pass);
    for (int ncu : {64, 128, 192, 256}) {
      unsigned mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int i = 0; i < ncu; i++) mask[i >> 5] |= 1u << (i & 31);
      hipStream_t st;
      CHECK(hipExtStreamCreateWithCUMask(&st, 8, mask));
      // (a)
      for (int pos : {32, 112, 224}) {
        const int cpp = (pos + 63) / 64;
        for (int per : {1, 2, 8}) {
          int grid = ncu * per;
          if (grid * 4 > npairs * cpp) grid = (npairs * cpp + 3) / 4;
          printf("(a) %3d CUs x %d blocks  pos %3d :", ncu, per, pos);
          for (int form = 0; form < 3; form++) {
            std::vector<float> t;
            for (int it = 0; it < 9; it++) {
              const unsigned short* k = Kc + (size_t)(it % LAYERS) * layer_elems; const unsigned short* v = Vc + (size_t)(it % LAYERS) * layer_elems;
              CHECK(hipEventRecord(ea, st));
              if (form == 0) hipLaunchKernelGGL(kv_kernel<0>, dim3(grid), dim3(256), 0, st, k, v, sink, pos, Tc, npairs);
              else if (form == 1) hipLaunchKernelGGL(kv_kernel<1>, dim3(grid), dim3(256), 0, st, k, v, sink, pos, Tc, npairs);
              else hipLaunchKernelGGL(kv_kernel<2>, dim3(grid), dim3(256), 0, st, k, v, sink, pos, Tc, npairs);
              CHECK(hipEventRecord(eb, st)); CHECK(hipEventSynchronize(eb));
              float ms; CHECK(hipEventElapsedTime(&ms, ea, eb));
              if (it >= 2) t.push_back(ms);
            }
            const float lo = *std::min_element(t.begin(), t.end()), hi = *std::max_element(t.begin(), t.end()), md = median(t);
            const double bytes = (double)npairs * pos * 128 * 2;
            printf("  %s %6.1f us (%6.1f .. %6.1f) %5.2f TB/s |", kv_names[form], md * 1e3, lo * 1e3, hi * 1e3, bytes / (md * 1e-3) / 1e12);
          }
          printf("\n");
        }
      }
      // (b)
      for (int K : {768, 3072}) {
        for (int nb : {72, 96}) {
          for (int rot = 0; rot < 2; rot++) {
            const int reps = 16, ksplit = K == 768 ? 1 : 3;
            const long rs = rot ? (long)256 * K : 0;
            printf("(b) %3d CUs  256 x %4d, %2d column blocks, %s :", ncu, K, nb, rot ? "rotate" : "same  ");
            for (int packed = 0; packed < 2; packed++) {
              std::vector<float> t;
              for (int it = 0; it < 9; it++) {
                CHECK(hipEventRecord(ea, st));
                if (K == 768) {
                  if (packed) hipLaunchKernelGGL((act_kernel<1, 6>), dim3(nb, 4, ksplit), dim3(256), 0, st, A, sink, K, reps, rs);
                  else hipLaunchKernelGGL((act_kernel<0, 6>), dim3(nb, 4, ksplit), dim3(256), 0, st, A, sink, K, reps, rs);
                } else {
                  if (packed) hipLaunchKernelGGL((act_kernel<1, 8>), dim3(nb, 4, ksplit), dim3(256), 0, st, A, sink, K, reps, rs);
                  else hipLaunchKernelGGL((act_kernel<0, 8>), dim3(nb, 4, ksplit), dim3(256), 0, st, A, sink, K, reps, rs);
                }
                CHECK(hipEventRecord(eb, st)); CHECK(hipEventSynchronize(eb));
                float ms; CHECK(hipEventElapsedTime(&ms, ea, eb));
                if (it >= 2) t.push_back(ms);
              }
              const float lo = *std::min_element(t.begin(), t.end()), hi = *std::max_element(t.begin(), t.end()), md = median(t);
              const double bytes = (double)reps * nb * 256 * K * 2;
              printf("  %s %6.2f us per pass (%6.2f .. %6.2f) %5.2f TB/s |", packed ? "packed   " : "row-major", md * 1e3 / reps, lo * 1e3 / reps, hi * 1e3 / reps,
                     bytes / (md * 1e-3) / 1e12);
            }
            printf("\n");
          }
        }
      }
      // (c)
      for (int mt : {4, 2, 1}) {
        const int reps = 16;
        printf("(c) %3d CUs  256 x  768, 24 column blocks x %2d row blocks :", ncu, 16 / mt);
        for (int packed = 0; packed < 2; packed++) {
          std::vector<float> t;
          for (int it = 0; it < 9; it++) {
            const dim3 grid(24, 16 / mt, 1);
            CHECK(hipEventRecord(ea, st));
            if (mt == 4) { if (packed) hipLaunchKernelGGL((act_kernel<1, 6, 4>), grid, dim3(256), 0, st, A, sink, 768, reps, 0L); else hipLaunchKernelGGL((act_kernel<0, 6, 4>), grid, dim3(256), 0, st, A, sink, 768, reps, 0L); }
            else if (mt == 2) { if (packed) hipLaunchKernelGGL((act_kernel<1, 6, 2>), grid, dim3(256), 0, st, A, sink, 768, reps, 0L); else hipLaunchKernelGGL((act_kernel<0, 6, 2>), grid, dim3(256), 0, st, A, sink, 768, reps, 0L); }
            else { if (packed) hipLaunchKernelGGL((act_kernel<1, 6, 1>), grid, dim3(256), 0, st, A, sink, 768, reps, 0L); else hipLaunchKernelGGL((act_kernel<0, 6, 1>), grid, dim3(256), 0, st, A, sink, 768, reps, 0L); }
            CHECK(hipEventRecord(eb, st)); CHECK(hipEventSynchronize(eb));
            float ms; CHECK(hipEventElapsedTime(&ms, ea, eb));
            if (it >= 2) t.push_back(ms);
          }
          const float lo = *std::min_element(t.begin(), t.end()), hi = *std::max_element(t.begin(), t.end()), md = median(t);
          printf("  %s %6.2f us per pass (%6.2f .. %6.2f) |", packed ? "packed   " : "row-major", md * 1e3 / reps, lo * 1e3 / reps, hi * 1e3 / reps);
        }
        printf("\n");
      }
      // (d): Wq, xb and WkT side by side in A (1.2 + 0.4 + 1.2 MB)
      {
        const int reps = 16;
        const unsigned short *Wq = A, *xb = A + 768 * 768, *WkT = A + 768 * 768 + 256 * 768;
        printf("(d) %3d CUs  query + expansion operands, 12 heads x 16 row tiles :", ncu);
        for (int packed = 0; packed < 2; packed++) {
          std::vector<float> t;
          for (int it = 0; it < 9; it++) {
            CHECK(hipEventRecord(ea, st));
            if (packed) hipLaunchKernelGGL(xq_kernel<1>, dim3(12, 16), dim3(256), 0, st, Wq, xb, WkT, sink, reps);
            else hipLaunchKernelGGL(xq_kernel<0>, dim3(12, 16), dim3(256), 0, st, Wq, xb, WkT, sink, reps);
            CHECK(hipEventRecord(eb, st)); CHECK(hipEventSynchronize(eb));
            float ms; CHECK(hipEventElapsedTime(&ms, ea, eb));
            if (it >= 2) t.push_back(ms);
          }
          const float lo = *std::min_element(t.begin(), t.end()), hi = *std::max_element(t.begin(), t.end()), md = median(t);
          printf("  %s %6.2f us per pass (%6.2f .. %6.2f) |", packed ? "packed   " : "row-major", md * 1e3 / reps, lo * 1e3 / reps, hi * 1e3 / reps);
        }
        printf("\n");
      }
      CHECK(hipStreamDestroy(st));
    }
  }
  return 0;
}
