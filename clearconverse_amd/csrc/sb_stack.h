// sb_stack.h -- one SpeechBrain SBTransformerBlock stack as both separator families keep it on the device (sepformer.hip: 128 wide,
// dualpath.hip: 256 wide): the layers, the stack's final LayerNorm and the outer norm (gLN / GroupNorm) of the block that wraps it,
// the loader that fills them from a handle's ccx_dev_store, and the sinusoidal positional-encoding table.  Host-only.
#pragma once
#include <math.h>
#include <string>
#include <vector>
#include "model_store.h"

struct SbLayer {
  float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *bqkv, *bo, *b1, *b2;
  bf16_t *Wqkv, *Wo, *W1, *W2;
};
struct SbStack {
  std::vector<SbLayer> layers;
  float *lnf_g, *lnf_b, *norm_g, *norm_b;   // final LayerNorm of the stack; gamma / beta of the outer norm
};

// `prefix`.mdl.layers.<l>.* and `prefix`.mdl.norm.norm.* are the stack, `norm`.weight / .bias the outer norm (D values each)
inline int sb_load_stack(ccx_dev_store& store, const std::string& prefix, const std::string& norm, int n_layers, int D, int F, SbStack& B) {
  B.layers.resize(n_layers);
  for (int l = 0; l < n_layers; l++) {
    const std::string p = prefix + ".mdl.layers." + std::to_string(l);
    SbLayer& L = B.layers[l];
    CCX_NEED(store, wi, p + ".self_att.att.in_proj_weight", 3 * D, D); CCX_NEED(store, bi, p + ".self_att.att.in_proj_bias", 3 * D);
    CCX_NEED(store, wo, p + ".self_att.att.out_proj.weight", D, D); CCX_NEED(store, bo, p + ".self_att.att.out_proj.bias", D);
    CCX_NEED(store, w1, p + ".pos_ffn.ffn.0.weight", F, D); CCX_NEED(store, b1, p + ".pos_ffn.ffn.0.bias", F);
    CCX_NEED(store, w2, p + ".pos_ffn.ffn.3.weight", D, F); CCX_NEED(store, b2, p + ".pos_ffn.ffn.3.bias", D);
    CCX_NEED(store, g1, p + ".norm1.norm.weight", D); CCX_NEED(store, be1, p + ".norm1.norm.bias", D);
    CCX_NEED(store, g2, p + ".norm2.norm.weight", D); CCX_NEED(store, be2, p + ".norm2.norm.bias", D);
    CCX_TRY(store.upload_bf16(&L.Wqkv, wi->data)); CCX_TRY(store.upload(&L.bqkv, bi->data));
    CCX_TRY(store.upload_bf16(&L.Wo, wo->data)); CCX_TRY(store.upload(&L.bo, bo->data));
    CCX_TRY(store.upload_bf16(&L.W1, w1->data)); CCX_TRY(store.upload(&L.b1, b1->data));
    CCX_TRY(store.upload_bf16(&L.W2, w2->data)); CCX_TRY(store.upload(&L.b2, b2->data));
    CCX_TRY(store.upload(&L.ln1_g, g1->data)); CCX_TRY(store.upload(&L.ln1_b, be1->data));
    CCX_TRY(store.upload(&L.ln2_g, g2->data)); CCX_TRY(store.upload(&L.ln2_b, be2->data));
  }
  CCX_NEED(store, fg, prefix + ".mdl.norm.norm.weight", D); CCX_NEED(store, fb, prefix + ".mdl.norm.norm.bias", D);
  CCX_NEED(store, gg, norm + ".weight", D); CCX_NEED(store, gb, norm + ".bias", D);
  CCX_TRY(store.upload(&B.lnf_g, fg->data)); CCX_TRY(store.upload(&B.lnf_b, fb->data));
  CCX_TRY(store.upload(&B.norm_g, gg->data)); CCX_TRY(store.upload(&B.norm_b, gb->data));
  return CCX_OK;
}

// pe[p][i] = sin(p den_i), pe[p][i + 1] = cos(p den_i) for even i, den_i = exp(-i ln(10000) / D): `len` rows of D floats
inline std::vector<float> sb_pos_enc_table(int len, int D) {
  std::vector<float> pe((size_t)len * D);
  for (int p = 0; p < len; p++)
    for (int i = 0; i < D; i += 2) {
      const float den = expf((float)i * -(logf(10000.0f) / (float)D));
      pe[(size_t)p * D + i] = sinf((float)p * den);
      pe[(size_t)p * D + i + 1] = cosf((float)p * den);
    }
  return pe;
}
