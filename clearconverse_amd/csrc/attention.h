// attention.h -- launchers for the attention kernels (see attention.hip).
#pragma once
#include "ccx_common.h"

// Encoder self-attention, head_dim 64, non-causal.
// Q,K: [B*H, Spad, 64] bf16 (rows >= S zero); Vt: [B*H, 64, Spad] bf16; O: [B*S, H*64] bf16.
// n_keys_dev (optional, device [B], each in [1, S]): sequence b attends over its first n_keys[b] positions only (reduced audio
// context); rows of O at or beyond n_keys[b] are zeros, and rows of K / Vt between n_keys[b] and Spad need only be finite.  Null:
// every sequence uses S.
int ccx_launch_enc_attention(ccx_ctx* ctx, const bf16_t* Q, const bf16_t* K, const bf16_t* Vt, bf16_t* O,
                             int B, int n_head, int S, int Spad, hipStream_t stream, const int* n_keys_dev = nullptr);
