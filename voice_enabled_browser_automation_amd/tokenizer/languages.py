"""Whisper's language tokens: the ordered ISO codes of the multilingual special-token layout
(``<|en|>`` = ``cfg.lang_en``, then one id per code) shared by the tokenizer trainer
(tokenizer/train.py) and the runtime (asr/engine.py language detection).

The 51865-token layout has the first 99 codes; large-v3's 51866 adds ``yue`` as the 100th.
English-only checkpoints have no language tokens and are not covered.
"""
from __future__ import annotations

from typing import Tuple

WHISPER_LANGUAGES: Tuple[str, ...] = (
    "en", "zh", "de", "es", "ru", "ko", "fr", "ja", "pt", "tr", "pl", "ca", "nl", "ar", "sv", "it", "id",
    "hi", "fi", "vi", "he", "uk", "el", "ms", "cs", "ro", "da", "hu", "ta", "no", "th", "ur", "hr", "bg",
    "lt", "la", "mi", "ml", "cy", "sk", "te", "fa", "lv", "bn", "sr", "az", "sl", "kn", "et", "mk", "br",
    "eu", "is", "hy", "ne", "mn", "bs", "kk", "sq", "sw", "gl", "mr", "pa", "si", "km", "sn", "yo", "so",
    "af", "oc", "ka", "be", "tg", "sd", "gu", "am", "yi", "lo", "uz", "fo", "ht", "ps", "tk", "nn", "mt",
    "sa", "lb", "my", "bo", "tl", "mg", "as", "tt", "haw", "ln", "ha", "ba", "jw", "su", "yue",
)


def language_codes(n_langs: int) -> Tuple[str, ...]:
    """The codes of a model with ``n_langs`` language tokens (99, or 100 with ``yue``)."""
    if not 1 <= n_langs <= len(WHISPER_LANGUAGES):
        raise ValueError(f"{n_langs} language tokens: the layout has 1..{len(WHISPER_LANGUAGES)}")
    return WHISPER_LANGUAGES[:n_langs]


def language_index(cfg, code: str) -> int:
    """Index of ``code`` among the model's language tokens; ValueError for a code the model lacks."""
    codes = language_codes(cfg.n_langs)
    c = str(code).strip().lower()
    if c not in codes:
        raise ValueError(f"unknown language code {code!r} for {cfg.name} ({len(codes)} languages)")
    return codes.index(c)


def language_token(cfg, code: str) -> int:
    """Token id of ``<|code|>`` in the model's layout."""
    return cfg.lang_en + language_index(cfg, code)


def language_code(cfg, token: int) -> str:
    """The code whose token id is ``token``; ValueError for an id that is no language token."""
    i = int(token) - cfg.lang_en
    if not 0 <= i < cfg.n_langs:
        raise ValueError(f"token {token} is not a language token of {cfg.name} "
                         f"([{cfg.lang_en}, {cfg.lang_en + cfg.n_langs}))")
    return language_codes(cfg.n_langs)[i]
