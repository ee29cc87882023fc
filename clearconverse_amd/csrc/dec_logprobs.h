// dec_logprobs.h -- the n best allowed ids of one filtered logit row held in the registers of a 1024-thread block, with their
// log-probabilities (the LOGP instantiations of dec_select_kernel, decoder.hip; the rule: include/ccx.h ccx_decode_logprob_options).
//
// The row is the one sum_logprob is defined over: after every filter (banned ids -inf, the text ids of a forced-timestamp row
// included -- the caller masks them where its draw has not), not divided by the temperature, not truncated, without noise.  Round k
// takes the block arg-max of what is left (the thread's 52 registers in index order, ids ascending, so the lowest id of equal values
// stays; then block_argmax, which breaks ties the same way), thread 0 writes (id, (value - mx_all) - lnorm) -- the expression the
// kernel forms the chosen token's log-probability with, so an id that is both chosen and listed carries the same bits -- and the
// winner's register becomes -inf.  Once nothing is left the rounds write (-1, -inf).  The rounds run after the draw: val[] is dead
// behind them and is consumed.  These are the rounds dec_beam_topk_kernel (dec_beam.hip) runs for its beam + 1 proposals.
#pragma once
#include "dec_head_row.h"

namespace dec_logp {

// out_id / out_lp: the row's [kLogprobMaxTop] slots of this step (thread 0 writes the first n); sh_v / sh_i: 16 words of LDS each
__device__ __forceinline__ void top_rounds(int tid, float (&val)[kHeadV4 * 4], int n, float mx_all, float lnorm, int* out_id, float* out_lp,
                                           float* sh_v, int* sh_i) {
#pragma unroll 1
  for (int k = 0; k < n; k++) {
    float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < kHeadV4 * 4; i++) {
      const int v = head_id(tid, i);
      const bool up = val[i] > bv;            // ids ascend with i: the lowest id of equal values stays
      bv = up ? val[i] : bv; bi = up ? v : bi;
    }
    float ov; int oi;
    block_argmax(tid, bv, bi, ov, oi, sh_v, sh_i);
    if (tid == 0) {
      const bool some = ov > -INFINITY;
      out_id[k] = some ? oi : -1;
      out_lp[k] = some ? (ov - mx_all) - lnorm : -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < kHeadV4 * 4; i++) val[i] = (head_id(tid, i) == oi) ? -INFINITY : val[i];
  }
}

}  // namespace dec_logp
