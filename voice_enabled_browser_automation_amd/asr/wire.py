"""The wire format of incoming audio: Deepgram's ``encoding`` / ``sample_rate`` / ``channels``
options of ``listen.live`` (apps/voice/src/deepgram.ts:36-45), defined and validated here and
nowhere else.

``AudioFormat`` names what a window of bytes holds; ``ops.ingest(raw, fmt)`` turns such a window into
the 16 kHz f32 mono samples the recogniser reads (csrc/ingest/ingest.h).  The host side of a session
needs less: a mono int16 view of each packet for the energy VAD (``mono_int16``: a 256-entry table
for the G.711 laws, an integer mean over the channels).
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np

ENCODINGS = ("linear16", "mulaw", "alaw")  # the index is the kernel's encoding code
SAMPLE_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
MAX_CHANNELS = 8
OUT_RATE = 16000


class FormatError(ValueError):
    """An unsupported wire format; ``param`` names the offending option."""

    def __init__(self, param: str, message: str):
        super().__init__(message)
        self.param = param


@dataclass(frozen=True)
class AudioFormat:
    """encoding: linear16 (s16le) | mulaw | alaw (G.711); sample_rate: one of SAMPLE_RATES;
    channels: 1..8, interleaved; channel: None -- the channels' mean -- or the one channel to take."""

    encoding: str = "linear16"
    sample_rate: int = OUT_RATE
    channels: int = 1
    channel: Optional[int] = None

    def __post_init__(self):
        if self.encoding not in ENCODINGS:
            raise FormatError("encoding", f"encoding must be one of {', '.join(ENCODINGS)}, not {self.encoding!r}")
        if isinstance(self.sample_rate, bool) or not isinstance(self.sample_rate, int) \
                or self.sample_rate not in SAMPLE_RATES:
            raise FormatError("sample_rate", f"sample_rate must be one of {', '.join(map(str, SAMPLE_RATES))}, "
                                             f"not {self.sample_rate!r}")
        if isinstance(self.channels, bool) or not isinstance(self.channels, int) \
                or not 1 <= self.channels <= MAX_CHANNELS:
            raise FormatError("channels", f"channels must be in 1..{MAX_CHANNELS}, not {self.channels!r}")
        if self.channel is not None and (isinstance(self.channel, bool) or not isinstance(self.channel, int)
                                         or not 0 <= self.channel < self.channels):
            raise FormatError("channel", f"channel must be in 0..{self.channels - 1}, not {self.channel!r}")

    @property
    def code(self) -> int:
        return ENCODINGS.index(self.encoding)

    @property
    def sample_bytes(self) -> int:
        return 2 if self.encoding == "linear16" else 1

    @property
    def frame_bytes(self) -> int:
        """Bytes of one frame: one sample of every channel."""
        return self.sample_bytes * self.channels

    @property
    def ratio(self) -> Tuple[int, int]:
        """(L, M): 16000 / sample_rate in lowest terms."""
        f = Fraction(OUT_RATE, self.sample_rate)
        return f.numerator, f.denominator

    @property
    def half_taps(self) -> int:
        """H: the resampling filter reads input samples pos - H + 1 .. pos + H."""
        L, M = self.ratio
        return 16 if L >= M else -(-16 * M // L)

    def n_out(self, n_in: int) -> int:
        """16 kHz samples that n_in frames give."""
        L, M = self.ratio
        return n_in * L // M

    @property
    def is_default(self) -> bool:
        return self == DEFAULT_FORMAT


DEFAULT_FORMAT = AudioFormat()


def format_from_query(query) -> Optional[AudioFormat]:
    """The format a ``/stream`` query string asks for (a mapping with ``get``); None when it names
    none of the options -- today's mono PCM16 at 16 kHz through today's path.  Raises FormatError,
    naming the parameter, for a value that is not supported and for ``multichannel=true``
    (per-channel transcripts are not served)."""
    multi = query.get("multichannel")
    if multi is not None and str(multi).strip().lower() not in ("false", "0", ""):
        raise FormatError("multichannel", "multichannel transcripts are not supported: send channels=N with an "
                                          "optional channel=i, which gives one transcript")
    if not any(query.get(k) is not None for k in ("encoding", "sample_rate", "channels", "channel")):
        return None

    def integer(name, default):
        raw = query.get(name)
        if raw is None:
            return default
        try:
            return int(str(raw).strip(), 10)
        except ValueError:
            raise FormatError(name, f"{name} must be an integer, not {raw!r}") from None

    enc = query.get("encoding")
    return AudioFormat("linear16" if enc is None else str(enc).strip().lower(), integer("sample_rate", OUT_RATE),
                       integer("channels", 1), integer("channel", None))


# ----------------------------------------------------------------------------- host decode
def _mulaw_table() -> np.ndarray:
    u = ~np.arange(256) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def _alaw_table() -> np.ndarray:
    a = np.arange(256) ^ 0x55
    seg = (a >> 4) & 7
    t = (a & 0x0F) << 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


G711_TABLES = {"mulaw": _mulaw_table(), "alaw": _alaw_table()}  # code -> the standard's 16-bit value


def decode_int16(raw, fmt: AudioFormat) -> np.ndarray:
    """Whole frames of wire bytes -> int16 [n_frames, channels]."""
    b = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw.view(np.uint8).reshape(-1)
    if len(b) % fmt.frame_bytes:
        raise ValueError(f"{len(b)} bytes are not whole frames of {fmt.frame_bytes}")
    v = b.view("<i2") if fmt.encoding == "linear16" else G711_TABLES[fmt.encoding][b]
    return v.reshape(-1, fmt.channels)


def mono_int16(raw, fmt: AudioFormat) -> np.ndarray:
    """What the VAD reads: the selected channel, or the channels' integer mean (floor), as int16."""
    v = decode_int16(raw, fmt)
    if fmt.channel is not None:
        return v[:, fmt.channel]
    if fmt.channels == 1:
        return v[:, 0]
    return (v.sum(axis=1, dtype=np.int32) // fmt.channels).astype(np.int16)


class WireAudio:
    """A window of wire frames on its way to a recogniser: ``raw`` (uint8, whole frames) and its
    format.  ``len()`` is the window's length in 16 kHz samples, as of the int16 array it stands for."""

    __slots__ = ("raw", "fmt")

    def __init__(self, raw: np.ndarray, fmt: AudioFormat):
        self.raw, self.fmt = raw, fmt

    @property
    def n_frames(self) -> int:
        return len(self.raw) // self.fmt.frame_bytes

    def __len__(self) -> int:
        return self.fmt.n_out(self.n_frames)

    def copy(self) -> "WireAudio":
        return WireAudio(np.array(self.raw, dtype=np.uint8, copy=True), self.fmt)
