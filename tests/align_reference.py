"""References for the word-alignment kernels (clearconverse_amd/csrc/align.hip) and the host rules of clearconverse_amd/word_timing.py,
in plain torch / numpy.  Restated from openai-whisper's timing.py [UPSTREAM-RECALL: find_alignment, median_filter, dtw_cpu, backtrace,
merge_punctuations, get_end]; tests/test_align_reference_cpu.py pins the median filter and the DTW against the independently written
`transformers` implementation.

  scores / matrix   fp64, from the operands the kernels see
  dtw               an fp32 numpy loop -- this loop IS the definition the kernel must equal bit for bit
  word rules        a second statement of merge_punctuations / get_end, written apart from the product's
"""
import numpy as np
import torch
import torch.nn.functional as F


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


def scores_ref(q: torch.Tensor, k: torch.Tensor, n_keys) -> torch.Tensor:
    """q [n_seq, H, 64] f32, k [n_seq, H, Spad, 64] (bf16 values) -> fp64 [n_seq, H, max(n_keys)]: softmax(q . k_j / 8) over the first
    n_keys[s] keys, 0 behind.  Keys behind n_keys are not touched (they may hold NaN)."""
    n_seq, H, _ = q.shape
    out = torch.zeros(n_seq, H, max(n_keys), dtype=torch.float64)
    for s in range(n_seq):
        n = int(n_keys[s])
        sc = torch.einsum("hd,hjd->hj", q[s].double(), k[s, :, :n].double()) / 8.0
        out[s, :, :n] = torch.softmax(sc, dim=-1)
    return out


def scores_abs_sum(q: torch.Tensor, k: torch.Tensor, n_keys) -> float:
    """max over (sequence, head, key) of S = sum_i |q_i k_i| / 8: what the rounding error of a score scales with"""
    worst = 0.0
    for s in range(q.shape[0]):
        n = int(n_keys[s])
        worst = max(worst, float(torch.einsum("hd,hjd->hj", q[s].double().abs(), k[s, :, :n].double().abs()).max()) / 8.0)
    return worst


def median_filter_ref(x: torch.Tensor, width: int = 7) -> torch.Tensor:
    """timing.py::median_filter along the last axis: reflect padding of width // 2, the input itself when it is not longer than that"""
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    lead = x.shape[:-1]
    xp = F.pad(x.reshape(1, -1, x.shape[-1]), (pad, pad), mode="reflect").reshape(*lead, -1)
    return xp.unfold(-1, width, 1).sort(dim=-1)[0][..., pad]


def matrix_ref(P: torch.Tensor) -> torch.Tensor:
    """P [Hsel, T, M] -> fp64 [T, M]: (p - mean_t) / std_t (population, over ALL T rows), median of 7 over frames, mean over heads"""
    w = P.double()
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    return median_filter_ref((w - mean) / std, 7).mean(dim=0)


def dtw_ref(x: np.ndarray):
    """timing.py::dtw_cpu + backtrace over an fp32 cost matrix x [N, M]: (text_idx, time_idx) of the path, in fp32 arithmetic."""
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = -np.ones((N + 1, M + 1), dtype=np.int8)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = np.float32(x[i - 1, j - 1] + c)
            trace[i, j] = t
    i, j = N, M
    trace[0, :] = 2
    trace[:, 0] = 1
    path = []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    path = np.array(path[::-1], dtype=np.int64).reshape(-1, 2)
    return path[:, 0], path[:, 1]


def dtw_ref_fast(x: np.ndarray):
    """dtw_ref with the column loop vectorised over anti-diagonals -- the same fp32 adds of the same operands, so the same bits
    (tests/test_align_reference_cpu.py checks it against the plain loop); for the 448 x 1500 cases."""
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.full((N + 1, M + 1), 2, dtype=np.int8)
    cost[0, 0] = 0
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        diag = (c0 < c1) & (c0 < c2)
        up = ~diag & (c1 < c0) & (c1 < c2)
        c = np.where(diag, c0, np.where(up, c1, c2))
        cost[i, j] = x[i - 1, j - 1] + c
        trace[i, j] = np.where(diag, 0, np.where(up, 1, 2))
    i, j = N, M
    trace[0, :] = 2
    trace[:, 0] = 1
    path = []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    path = np.array(path[::-1], dtype=np.int64).reshape(-1, 2)
    return path[:, 0], path[:, 1]


def jump_frames(text_idx: np.ndarray, time_idx: np.ndarray) -> np.ndarray:
    """find_alignment: jumps = pad(diff(text_indices), (1, 0), constant_values=1).astype(bool); time_indices[jumps]"""
    jumps = np.pad(np.diff(text_idx), (1, 0), constant_values=1).astype(bool)
    return time_idx[jumps]


# ---- the teacher-forced pass: WhisperRef's decoder arithmetic (oracle/whisper_ref.py decoder_logits) with the cross-attention
# probabilities kept -- model.py's MultiHeadAttention returns qk, timing.py's hooks collect it per layer ----
def cross_attention_probs(ref, tokens: torch.Tensor, xa: torch.Tensor, heads, n_keys: int) -> torch.Tensor:
    """ref: oracle.whisper_ref.WhisperRef (any dtype); tokens [T] int64, xa [1500, D] of ONE window -> [len(heads), T, n_keys]:
    softmax over the first n_keys encoder positions of q . k / 8 for the (layer, head) pairs in `heads`, and S = the largest
    sum_i |q_i k_i| / 8 of the selected layers (what a score's rounding error scales with)."""
    d = ref.dims
    T = tokens.shape[-1]
    xa = xa.to(ref.dtype)[None]
    x = (ref.sd["decoder.token_embedding.weight"][tokens] + ref.sd["decoder.positional_embedding"][:T])[None]
    mask = torch.full((d.n_text_ctx, d.n_text_ctx), float("-inf"), dtype=ref.dtype).triu_(1)
    per_layer, s_abs = {}, 0.0
    for l in range(d.n_text_layer):
        p = f"decoder.blocks.{l}"
        x = x + ref._attn(ref._ln(x, p + ".attn_ln"), p + ".attn", d.n_text_head, mask=mask)
        h = ref._ln(x, p + ".cross_attn_ln")
        q = ref._lin(h, p + ".cross_attn.query").view(T, d.n_text_head, 64).permute(1, 0, 2)
        k = ref._lin(xa, p + ".cross_attn.key", bias=False)[0].view(-1, d.n_text_head, 64).permute(1, 0, 2)
        per_layer[l] = torch.softmax((q @ k[:, :n_keys].transpose(1, 2)) / 8.0, dim=-1)
        if any(hl == l for hl, _ in heads):
            s_abs = max(s_abs, float((q.abs() @ k[:, :n_keys].abs().transpose(1, 2)).max()) / 8.0)
        x = x + ref._attn(h, p + ".cross_attn", d.n_text_head, xa=xa)
        x = x + ref._mlp(ref._ln(x, p + ".mlp_ln"), p)
    return torch.stack([per_layer[l][h] for l, h in heads]), s_abs


# ---- word rules, stated a second time ----
PREPENDED = "\"'“¿([{-"
APPENDED = "\"'.。,，!！?？:：”)]}、"


def merge_punctuations_ref(words):
    """words: list of [word, tokens] -> the same list after timing.py::merge_punctuations (merged-away entries keep '' / [])"""
    w = [[a, list(b)] for a, b in words]
    j = len(w) - 1
    for i in range(len(w) - 2, -1, -1):
        if w[i][0].startswith(" ") and w[i][0].strip() in PREPENDED:
            w[j] = [w[i][0] + w[j][0], w[i][1] + w[j][1]]
            w[i] = ["", []]
        else:
            j = i
    i = 0
    for j in range(1, len(w)):
        if not w[i][0].endswith(" ") and w[j][0] in APPENDED:
            w[i] = [w[i][0] + w[j][0], w[i][1] + w[j][1]]
            w[j] = ["", []]
        else:
            i = j
    return w


def get_end_ref(segments):
    for s in reversed(segments):
        for w in reversed(s.get("words", [])):
            return w["end"]
    return segments[-1]["end"] if segments else None
