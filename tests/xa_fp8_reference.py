"""The FP8 encoder-output format of include/ccx.h ("FP8 encoder-output stream"), stated twice on the CPU:

  quantise_bits   by hand, on the bf16 bit patterns, integer and bit operations in numpy only;
  quantise_torch  on torch.frexp and the torch.float8_e4m3fn cast (round to nearest even on the CPU).

Blocks of 32 consecutive features; scale 2^e with e the smallest integer such that amax <= 448 * 2^e, clamped to [-64, 64] (amax == 0:
-64), stored as e + 127; code = e4m3fn(x / 2^e) clamped to +-448; xhat = code * 2^e, which bf16 holds exactly.  Finite inputs only.
The hand-worked blocks the tests plant are here as well (HAND_BLOCKS)."""
import numpy as np
import torch

BLOCK, EMIN, EMAX = 32, -64, 64


def bf16_bits(x: torch.Tensor) -> np.ndarray:
    """float32 tensor holding bf16-representable values -> uint16 bit patterns"""
    x = x.detach().cpu().contiguous().to(torch.float32)
    b = x.view(torch.int32).numpy().view(np.uint32)
    assert not (b & 0xFFFF).any(), "not bf16 values"
    return (b >> 16).astype(np.uint16)


def bits_to_f32(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy((bits.astype(np.uint32) << 16).view(np.float32).copy())


def block_exp_bits(amax_bits: np.ndarray) -> np.ndarray:
    """amax as bf16 magnitude bits (15 bits).  amax = 1.m * 2^E: amax <= 1.75 * 2^(e + 8) first holds at e = E - 8, or one more when
    the mantissa exceeds 1.75's (0x60).  Exponent bits 0 (zero, subnormal) fall below the clamp."""
    a = amax_bits.astype(np.int32)
    e = (a >> 7) - 127 - 8 + ((a & 0x7F) > 0x60)
    return np.clip(e, EMIN, EMAX)


def code_bits(x_bits: np.ndarray, e: np.ndarray) -> np.ndarray:
    """E4M3 code of x / 2^e (x as bf16 bits, e broadcastable): round to nearest even, clamped to 0x7e = 448"""
    x = x_bits.astype(np.int32)
    sign, eb = (x >> 8) & 0x80, (x >> 7) & 0xFF
    ev = eb - 127 - e
    sig = 0x80 | (x & 0x7F)                                    # value = sig * 2^(ev - 7)
    sh = np.minimum(np.where(ev >= -6, 4, 4 + (-6 - ev)), 9)   # 3 mantissa bits above 2^-6, steps of 2^-9 below
    n = (sig + ((1 << (sh - 1)) - 1) + ((sig >> sh) & 1)) >> sh
    code = np.minimum(((np.maximum(ev, -6) + 6) << 3) + n, 0x7E)
    return (sign | np.where(eb == 0, 0, code)).astype(np.uint8)


def value_bits(code: np.ndarray, e: np.ndarray) -> np.ndarray:
    """code * 2^e as bf16 bits, assembled field by field (no float arithmetic)"""
    c = code.astype(np.int32)
    sign, e4, m3 = (c & 0x80) << 8, (c >> 3) & 0xF, c & 7
    # normal codes: 1.m3 * 2^(e4 - 7); subnormal ones: m3 * 2^-9, normalised by the position of m3's leading bit
    lead = np.where(m3 >= 4, 2, np.where(m3 >= 2, 1, 0))
    sub_exp = lead - 9
    sub_man = np.where(m3 > 0, (m3 << (3 - lead)) & 7, 0)
    ex = np.where(e4 > 0, e4 - 7, sub_exp) + e + 127
    man = np.where(e4 > 0, m3, sub_man) << 4
    bits = (ex << 7) | man
    return (sign | np.where((e4 == 0) & (m3 == 0), 0, bits)).astype(np.uint16)


def quantise_bits(x_bits: np.ndarray):
    """[..., D] bf16 bits -> (codes uint8 [..., D], e int [..., D / 32], xhat bits uint16 [..., D])"""
    D = x_bits.shape[-1]
    assert D % BLOCK == 0
    blk = x_bits.reshape(x_bits.shape[:-1] + (D // BLOCK, BLOCK))
    amax = (blk & 0x7FFF).max(axis=-1)
    e = block_exp_bits(amax)
    codes = code_bits(blk, e[..., None])
    xhat = value_bits(codes, e[..., None])
    return codes.reshape(x_bits.shape), e, xhat.reshape(x_bits.shape)


def quantise_torch(x: torch.Tensor):
    """the same on torch.frexp and the float8 cast: [..., D] float32 -> (codes uint8, e int32, xhat float32)"""
    D = x.shape[-1]
    blk = x.to(torch.float32).reshape(x.shape[:-1] + (D // BLOCK, BLOCK))
    amax = blk.abs().amax(dim=-1)
    m, ex = torch.frexp(amax)                                 # amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
    e = torch.where(m <= 0.875, ex - 9, ex - 8)
    e = torch.where(amax == 0, torch.full_like(e, EMIN), e).clamp(EMIN, EMAX)
    scaled = torch.ldexp(blk, -e[..., None]).clamp(-448.0, 448.0)
    q = scaled.to(torch.float8_e4m3fn)
    xhat = torch.ldexp(q.to(torch.float32), e[..., None])
    return q.view(torch.uint8).reshape(x.shape), e, xhat.reshape(x.shape)


def xhat_of(x: torch.Tensor) -> torch.Tensor:
    """the reference dequantised values of bf16-valued float32 rows (the by-hand statement)"""
    return bits_to_f32(quantise_bits(bf16_bits(x))[2]).reshape(x.shape)


def _bf(v: float) -> float:
    return float(torch.tensor(v).bfloat16())


def _block(fill, **at):
    b = [float(fill)] * BLOCK
    for k, v in at.items():
        b[int(k[1:])] = float(v)
    return b


_STEP_ABOVE_448x8 = float(bits_to_f32(np.array([0x4560 + 1], dtype=np.uint16))[0])    # 448 * 2^3 = 0x4560; one bf16 step above: 3600

# name -> (32 input values, 32 expected dequantised values, expected e), worked by hand
HAND_BLOCKS = {
    # e = 0 (224 < 256 <= 448).  Step 0.125 at 1.x: 1.0625 and 1.1875 are ties -> even mantissa: 1.0 and 1.25
    "rne_ties": (_block(0.0, i0=256.0, i1=1.0625, i2=1.1875, i3=-1.0625, i4=-1.1875, i5=1.125, i31=-256.0),
                 _block(0.0, i0=256.0, i1=1.0, i2=1.25, i3=-1.0, i4=-1.25, i5=1.125, i31=-256.0), 0),
    # amax exactly 448 * 2^3: e = 3, the top code; 20 / 8 = 2.5 is a code
    "amax_448": (_block(20.0, i7=3584.0), _block(20.0, i7=3584.0), 3),
    # one bf16 step above (3600): e = 4, 3600 / 16 = 225 -> step 16 there -> 224 -> 3584; 20 / 16 = 1.25
    "amax_above_448": (_block(20.0, i7=_STEP_ABOVE_448x8), _block(20.0, i7=3584.0), 4),
    "all_zero": (_block(0.0), _block(0.0), EMIN),
    # one outlier 2^10 above the rest: e = 2 (896 < 1024 <= 1792), the smallest step is 2^-9 * 4 = 2^-7.  What lies below half a step
    # flushes to zero: 2^-8 is the tie (-> even = 0), 0.003 -> 0; 0.006 -> one step; 1.0 and 0.5 survive
    "outlier": (_block(_bf(0.003), i3=1024.0, i4=1.0, i5=0.5, i6=2.0 ** -7, i7=2.0 ** -8, i8=_bf(0.006), i9=-0.5),
                _block(0.0, i3=1024.0, i4=1.0, i5=0.5, i6=2.0 ** -7, i7=0.0, i8=2.0 ** -7, i9=-0.5), 2),
    # the exponent clamp below: amax 2^-70 asks for e = -78, gets -64: 2^-70 is code 2^-6, 2^-73 the smallest code, 2^-74 the tie -> 0
    "clamp_low": (_block(0.0, i0=2.0 ** -70, i1=2.0 ** -73, i2=2.0 ** -74, i3=-(2.0 ** -80)),
                  _block(0.0, i0=2.0 ** -70, i1=2.0 ** -73, i2=0.0, i3=-0.0), EMIN),
    # ... and above: amax 2^100 asks for e = 92, gets 64: the code clamp bites (448 * 2^64), 2^70 = 64 * 2^64 is exact
    "clamp_high": (_block(1.0, i0=2.0 ** 100, i1=-(2.0 ** 100), i2=2.0 ** 70),
                   _block(0.0, i0=448.0 * 2.0 ** 64, i1=-448.0 * 2.0 ** 64, i2=2.0 ** 70), EMAX),
}
for _name, (_x, _want, _e) in HAND_BLOCKS.items():
    assert len(_x) == BLOCK and len(_want) == BLOCK, _name


def plant(x: torch.Tensor, places):
    """x [n_seq, S, D] (modified in place): places = [(seq, key, feature block, name of a hand block)]"""
    for seq, key, blk, name in places:
        x[seq, key, blk * BLOCK:(blk + 1) * BLOCK] = torch.tensor(HAND_BLOCKS[name][0], dtype=torch.float32)
    return x


def hand_places(S: int, D: int):
    """sequence i carries hand block i in the first and in the last feature block of a row, on the first and the last key of the
    first, an interior and the (ragged) last 16-key tile -- len(HAND_BLOCKS) sequences"""
    nt = (S + 15) // 16
    keys = sorted({k for t in (0, nt // 2, nt - 1) for k in (16 * t, min(16 * t + 15, S - 1))})
    return [(i, key, blk, name) for i, name in enumerate(HAND_BLOCKS) for key in keys for blk in (0, D // BLOCK - 1)]
