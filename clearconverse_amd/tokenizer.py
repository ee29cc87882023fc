"""Token-id boundary of the Whisper path.

The English-only openai-whisper tokenizer is GPT-2 BPE plus special tokens [UPSTREAM-RECALL].  The
BPE vocabulary is not available offline, so text<->ids goes through `GPT2BPE` only when
`vocab.json`/`merges.txt` exist under MODEL_CACHE_DIR; otherwise `IdTokenizer` provides a reversible
synthetic codec (documented deviation: transcripts are strings of token placeholders).  The
special-token ids and the suppress list do not depend on the vocabulary file.

Multilingual checkpoints (`tiny` ... `medium`, n_vocab 51865; 51866 for the 100-language family) use the
"multilingual" vocabulary: one more text id, so every special sits one higher than its English-only
counterpart, and the SOT sequence is [sot, <|language|>, <|transcribe|> or <|translate|>].
`DecodeRules.multilingual()` / `DecodeRules.for_dims(dims)` give the id table, `LANGUAGES` the language
codes in the order of their tokens, `rules.sot_sequence(language, task)` the sequence.  The tokenizers
take the `eot` below which an id is text (default: the English-only one).
"""
from __future__ import annotations

import json
import os
import re
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

# English-only specials (openai-whisper tokenizer.py): eot 50256, sot 50257, 99 language tags,
# translate 50357, transcribe 50358, startoflm 50359, startofprev 50360, nospeech 50361,
# notimestamps 50362, <|0.00|> 50363 ... <|30.00|> 51863
EOT = 50256
SOT = 50257
TRANSLATE = 50357
TRANSCRIBE = 50358
SOT_LM = 50359
SOT_PREV = 50360
NO_SPEECH = 50361
NO_TIMESTAMPS = 50362
TIMESTAMP_BEGIN = 50363
BLANK = 220  # GPT-2 id of " "

# Tokenizer.non_speech_tokens for the GPT-2 vocabulary.  The id list is the one the locally
# installed `transformers` package carries for the english-only checkpoints
# (transformers/models/whisper/configuration_whisper.py NON_SPEECH_TOKENS, entries < 50257).
NON_SPEECH_TEXT_TOKENS = [
    1, 2, 7, 8, 9, 10, 14, 25, 26, 27, 28, 29, 31, 58, 59, 60, 61, 62, 63, 90, 91, 92, 93, 357, 366, 438,
    532, 685, 705, 796, 930, 1058, 1220, 1267, 1279, 1303, 1343, 1377, 1391, 1635, 1782, 1875, 2162,
    2361, 2488, 3467, 4008, 4211, 4600, 4808, 5299, 5855, 6329, 7203, 9609, 9959, 10563, 10786, 11420,
    11709, 11907, 13163, 13697, 13700, 14808, 15306, 16410, 16791, 17992, 19203, 19510, 20724, 22305,
    22935, 27007, 30109, 30420, 33409, 34949, 40283, 40493, 40549, 47282, 49146,
]
# decoding.py::_get_suppress_tokens adds these specials to the "-1" default list
SUPPRESS_TOKENS = sorted(NON_SPEECH_TEXT_TOKENS + [TRANSCRIBE, TRANSLATE, SOT, SOT_PREV, SOT_LM, NO_SPEECH])


# Multilingual vocabulary (openai-whisper tokenizer.py, `get_encoding("multilingual", num_languages)`) [UPSTREAM-RECALL]: eot 50257,
# sot 50258, the language tokens from 50259 in the order of LANGUAGES, then translate, transcribe, startoflm, startofprev, nospeech,
# notimestamps and <|0.00|> = 50265 + num_languages (50364 for 99 languages; 50364 + 1501 = 51865 = n_vocab).
MULTI_EOT = 50257
MULTI_BLANK = 220  # " " in the multilingual vocabulary as well

# Language codes in the order of their tokens (whisper/tokenizer.py LANGUAGES; restated from the locally installed `transformers`,
# models/whisper/tokenization_whisper.py::LANGUAGES, which tests/test_multilingual_cpu.py compares against).  The first 99 belong to
# the 51865-token checkpoints; "yue" is the 100th language of the 51866-token family.
LANGUAGES = {
    "en": "english", "zh": "chinese", "de": "german", "es": "spanish", "ru": "russian", "ko": "korean", "fr": "french",
    "ja": "japanese", "pt": "portuguese", "tr": "turkish", "pl": "polish", "ca": "catalan", "nl": "dutch", "ar": "arabic",
    "sv": "swedish", "it": "italian", "id": "indonesian", "hi": "hindi", "fi": "finnish", "vi": "vietnamese", "he": "hebrew",
    "uk": "ukrainian", "el": "greek", "ms": "malay", "cs": "czech", "ro": "romanian", "da": "danish", "hu": "hungarian",
    "ta": "tamil", "no": "norwegian", "th": "thai", "ur": "urdu", "hr": "croatian", "bg": "bulgarian", "lt": "lithuanian",
    "la": "latin", "mi": "maori", "ml": "malayalam", "cy": "welsh", "sk": "slovak", "te": "telugu", "fa": "persian",
    "lv": "latvian", "bn": "bengali", "sr": "serbian", "az": "azerbaijani", "sl": "slovenian", "kn": "kannada", "et": "estonian",
    "mk": "macedonian", "br": "breton", "eu": "basque", "is": "icelandic", "hy": "armenian", "ne": "nepali", "mn": "mongolian",
    "bs": "bosnian", "kk": "kazakh", "sq": "albanian", "sw": "swahili", "gl": "galician", "mr": "marathi", "pa": "punjabi",
    "si": "sinhala", "km": "khmer", "sn": "shona", "yo": "yoruba", "so": "somali", "af": "afrikaans", "oc": "occitan",
    "ka": "georgian", "be": "belarusian", "tg": "tajik", "sd": "sindhi", "gu": "gujarati", "am": "amharic", "yi": "yiddish",
    "lo": "lao", "uz": "uzbek", "fo": "faroese", "ht": "haitian creole", "ps": "pashto", "tk": "turkmen", "nn": "nynorsk",
    "mt": "maltese", "sa": "sanskrit", "lb": "luxembourgish", "my": "myanmar", "bo": "tibetan", "tl": "tagalog", "mg": "malagasy",
    "as": "assamese", "tt": "tatar", "haw": "hawaiian", "ln": "lingala", "ha": "hausa", "ba": "bashkir", "jw": "javanese",
    "su": "sundanese", "yue": "cantonese",
}
# language name (and upstream's aliases) -> code
TO_LANGUAGE_CODE = {
    **{name: code for code, name in LANGUAGES.items()},
    "burmese": "my", "valencian": "ca", "flemish": "nl", "haitian": "ht", "letzeburgesch": "lb", "pushto": "ps", "panjabi": "pa",
    "moldavian": "ro", "moldovan": "ro", "sinhalese": "si", "castilian": "es", "mandarin": "zh",
}

# Tokenizer.non_speech_tokens for the multilingual vocabulary: the entries below eot of the list `transformers` carries for the
# multilingual checkpoints (configuration_whisper.py NON_SPEECH_TOKENS_MULTI), taken as NON_SPEECH_TEXT_TOKENS was
NON_SPEECH_TEXT_TOKENS_MULTI = [
    1, 2, 7, 8, 9, 10, 14, 25, 26, 27, 28, 29, 31, 58, 59, 60, 61, 62, 63, 90, 91, 92, 93, 359, 503, 522, 542, 873, 893, 902, 918,
    922, 931, 1350, 1853, 1982, 2460, 2627, 3246, 3253, 3268, 3536, 3846, 3961, 4183, 4667, 6585, 6647, 7273, 9061, 9383, 10428,
    10929, 11938, 12033, 12331, 12562, 13793, 14157, 14635, 15265, 15618, 16553, 16604, 18362, 18956, 20075, 21675, 22520, 26130,
    26161, 26435, 28279, 29464, 31650, 32302, 32470, 36865, 42863, 47425, 49870, 50254,
]


@dataclass
class DecodeRules:
    eot: int = EOT
    sot: int = SOT
    sot_prev: int = SOT_PREV
    no_speech: int = NO_SPEECH
    no_timestamps: int = NO_TIMESTAMPS
    timestamp_begin: int = TIMESTAMP_BEGIN
    blank: int = BLANK
    max_initial_timestamp_index: int = 50  # 1.0 s / 0.02 s
    suppress: Sequence[int] = field(default_factory=lambda: list(SUPPRESS_TOKENS))
    # multilingual vocabularies only (0 languages: English-only, the SOT sequence is [sot])
    num_languages: int = 0
    translate: int = TRANSLATE
    transcribe: int = TRANSCRIBE
    sot_lm: int = SOT_LM

    @property
    def is_multilingual(self) -> bool:
        return self.num_languages > 0

    @property
    def language_begin(self) -> int:
        """id of the first language token (they are contiguous, in the order of LANGUAGES)"""
        return self.sot + 1

    @property
    def languages(self) -> List[str]:
        return list(LANGUAGES)[: self.num_languages]

    @staticmethod
    def multilingual(num_languages: int = 99) -> "DecodeRules":
        """The multilingual id table [UPSTREAM-RECALL: tokenizer.py]: each English-only id one higher, `num_languages` language tokens."""
        if not 1 <= num_languages <= len(LANGUAGES):
            raise ValueError(f"num_languages = {num_languages} out of range [1, {len(LANGUAGES)}]")
        sot = MULTI_EOT + 1
        translate = sot + 1 + num_languages
        transcribe, sot_lm, sot_prev, no_speech, no_timestamps, timestamp_begin = (translate + i for i in range(1, 7))
        suppress = sorted(NON_SPEECH_TEXT_TOKENS_MULTI + [transcribe, translate, sot, sot_prev, sot_lm, no_speech])
        return DecodeRules(eot=MULTI_EOT, sot=sot, sot_prev=sot_prev, no_speech=no_speech, no_timestamps=no_timestamps,
                           timestamp_begin=timestamp_begin, blank=MULTI_BLANK, suppress=suppress, num_languages=num_languages,
                           translate=translate, transcribe=transcribe, sot_lm=sot_lm)

    @staticmethod
    def for_dims(dims) -> "DecodeRules":
        """model.py::Whisper.is_multilingual / num_languages: the rules of a checkpoint follow from its n_vocab."""
        n_vocab = int(dims.n_vocab)
        if n_vocab < 51865:
            return DecodeRules()
        return DecodeRules.multilingual(n_vocab - 51765 - 1)

    def sot_sequence(self, language: Optional[str] = None, task: str = "transcribe") -> List[int]:
        """tokenizer.py::Tokenizer.sot_sequence: [sot] for an English-only model, else [sot, <|language|>, <|task|>]."""
        if not self.is_multilingual:
            return [self.sot]
        if task not in ("transcribe", "translate"):
            raise ValueError(f"task must be 'transcribe' or 'translate', not {task!r}")
        return [self.sot, self.language_token(language or "en"), self.transcribe if task == "transcribe" else self.translate]

    def language_token(self, language: str) -> int:
        code = language.lower()
        code = TO_LANGUAGE_CODE.get(code, code)
        langs = self.languages
        if code not in langs:
            raise ValueError(f"unsupported language {language!r}")
        return self.language_begin + langs.index(code)

    def language_code(self, token: int) -> str:
        i = int(token) - self.language_begin
        if not 0 <= i < self.num_languages:
            raise ValueError(f"token {token} is no language token")
        return self.languages[i]


class IdTokenizer:
    """Reversible placeholder codec used when no BPE vocabulary is on disk.

    decode: text ids -> " <id>" words.  encode: " <id>" words map back to the id; any other word
    maps to a stable pseudo-id (crc32 of the lower-cased word, folded below the special range and
    away from the suppressed ids) so fixed prompts are deterministic."""
    name = "id-placeholder"
    _word = re.compile(r"<(\d+)>")

    def __init__(self, eot: int = EOT):
        self.eot = int(eot)       # ids below it are text

    def decode(self, ids: Sequence[int]) -> str:
        return "".join(f" <{int(t)}>" for t in ids if int(t) < self.eot)

    def encode(self, text: str) -> List[int]:
        out = []
        for w in text.split():
            m = self._word.fullmatch(w)
            if m:
                out.append(int(m.group(1)))
            else:
                h = zlib.crc32(w.lower().encode("utf-8")) % 40000 + 1000
                out.append(h)
        return out


class GPT2BPE:
    """Byte-level BPE from vocab.json + merges.txt (GPT-2 files) when present under the cache dir."""
    name = "gpt2-bpe"

    def __init__(self, vocab_path: str, merges_path: str, eot: int = EOT):
        self.eot = int(eot)
        with open(vocab_path, encoding="utf-8") as f:
            self.enc = json.load(f)
        self.dec = {v: k for k, v in self.enc.items()}
        with open(merges_path, encoding="utf-8") as f:
            lines = [l for l in f.read().split("\n") if l and not l.startswith("#version")]
        self.ranks = {tuple(l.split()): i for i, l in enumerate(lines)}
        bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
        cs = bs[:]
        n = 0
        for b in range(256):
            if b not in bs:
                bs.append(b)
                cs.append(256 + n)
                n += 1
        self.b2u = dict(zip(bs, map(chr, cs)))
        self.u2b = {v: k for k, v in self.b2u.items()}
        self.pat = _gpt2_pattern()

    def _bpe(self, token: str) -> List[str]:
        word = list(token)
        while len(word) > 1:
            pairs = [(self.ranks.get((a, b), 1 << 30), i) for i, (a, b) in enumerate(zip(word, word[1:]))]
            r, i = min(pairs)
            if r == 1 << 30:
                break
            word[i:i + 2] = [word[i] + word[i + 1]]
        return word

    def encode(self, text: str) -> List[int]:
        ids = []
        for tok in self.pat.findall(text):
            t = "".join(self.b2u[b] for b in tok.encode("utf-8"))
            ids.extend(self.enc[p] for p in self._bpe(t))
        return ids

    def decode(self, ids: Sequence[int]) -> str:
        s = "".join(self.dec[int(t)] for t in ids if int(t) < self.eot)
        return bytearray(self.u2b[c] for c in s).decode("utf-8", errors="replace")


def _gpt2_pattern():
    """GPT-2 pre-tokeniser (whisper/tokenizer.py pat_str).  Needs \\p classes: the `regex` module when importable,
    else the ASCII approximation (identical on ASCII text)."""
    try:
        import regex
        return regex.compile(r"""'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+""")
    except ImportError:
        return re.compile(r"'s|'t|'re|'ve|'m|'ll|'d| ?[A-Za-z]+| ?\d+| ?[^\sA-Za-z\d]+|\s+(?!\S)|\s+")


class TiktokenBPE:
    """Byte-level BPE from a `.tiktoken` rank file -- the format openai-whisper ships its vocabulary in
    (`whisper/assets/gpt2.tiktoken`: one `base64(token bytes) rank` pair per line).  Encoding follows tiktoken's
    byte-pair merge: within a pre-token, repeatedly merge the adjacent pair whose concatenation has the lowest rank."""
    name = "tiktoken-bpe"

    def __init__(self, path: str, eot: int = EOT):
        import base64
        self.eot = int(eot)
        self.ranks: dict = {}
        with open(path, "rb") as f:
            for line in f.read().splitlines():
                if line.strip():
                    tok, rank = line.split()
                    self.ranks[base64.b64decode(tok)] = int(rank)
        self.dec = {v: k for k, v in self.ranks.items()}
        self.pat = _gpt2_pattern()

    def _bpe(self, piece: bytes) -> List[int]:
        parts = [piece[i:i + 1] for i in range(len(piece))]
        while len(parts) > 1:
            best, at = None, -1
            for i in range(len(parts) - 1):
                r = self.ranks.get(parts[i] + parts[i + 1])
                if r is not None and (best is None or r < best):
                    best, at = r, i
            if best is None:
                break
            parts[at:at + 2] = [parts[at] + parts[at + 1]]
        return [self.ranks[p] for p in parts]

    def encode(self, text: str) -> List[int]:
        ids: List[int] = []
        for tok in self.pat.findall(text):
            ids.extend(self._bpe(tok.encode("utf-8")))
        return ids

    def decode(self, ids: Sequence[int]) -> str:
        return b"".join(self.dec[int(t)] for t in ids if int(t) < self.eot).decode("utf-8", errors="replace")


def get_tokenizer(cache_dir: Optional[str] = None, rules: Optional[DecodeRules] = None):
    """The vocabulary files the reference's whisper package would use, if a copy sits under MODEL_CACHE_DIR:
    `gpt2.tiktoken` (openai-whisper's own asset) or GPT-2's `vocab.json` + `merges.txt`; else the placeholder codec.
    rules: those of the model (default English-only).  A multilingual model reads `multilingual.tiktoken`, upstream's asset for it,
    and filters text with its own eot; the GPT-2 files are the English-only vocabulary and are not offered to it."""
    cache_dir = cache_dir or os.environ.get("MODEL_CACHE_DIR", "models")
    multi = rules is not None and rules.is_multilingual
    eot = rules.eot if rules is not None else EOT
    for sub in ("whisper", os.path.join("whisper", "assets"), "gpt2", ""):
        t = os.path.join(cache_dir, sub, "multilingual.tiktoken" if multi else "gpt2.tiktoken")
        if os.path.exists(t):
            return TiktokenBPE(t, eot)
        v, m = os.path.join(cache_dir, sub, "vocab.json"), os.path.join(cache_dir, sub, "merges.txt")
        if not multi and os.path.exists(v) and os.path.exists(m):
            return GPT2BPE(v, m, eot)
    return IdTokenizer(eot)
