"""Host mirror of go-dsp's `wav` package (wav/wav.go): the WAV reader that
feeds spectral.Pwelch.

Header parsing is byte-level host work (a few dozen bytes), exactly as
wav.New does it (wav.go:59-107). The sample conversion of ReadFloats
(wav.go:135-161) runs on the GPU through gdsp_wav_read_floats; the device
feeder `device_floats` decodes a data chunk straight into an HBM-resident
float64 Pwelch input (gdsp_wav_read_floats_device), so a long recording
never round-trips through host float conversion.

Go returns `error` values here (not panics); the mirror raises WavError
with the reference's message ("wav: missing RIFF", ..., and io's "EOF" /
"unexpected EOF" for short reads).
"""
from __future__ import annotations

import ctypes
import struct
from dataclasses import dataclass

import numpy as np

from . import _lib, spectral
from ._lib import check, lib

wavFormatPCM = 1
wavFormatIEEEFloat = 3


class WavError(Exception):
    """An error value the reference returns (message = Go's err.Error())."""


@dataclass
class Header:
    """wav.Header — the fmt chunk (wav.go:37-45)."""
    AudioFormat: int = 0
    NumChannels: int = 0
    SampleRate: int = 0
    ByteRate: int = 0
    BlockAlign: int = 0
    BitsPerSample: int = 0


def _read_full(r, n: int) -> bytes:
    """io.ReadFull: "EOF" if nothing was read, "unexpected EOF" if short."""
    b = r.read(n)
    if len(b) == 0 and n > 0:
        raise WavError("EOF")
    if len(b) < n:
        raise WavError("unexpected EOF")
    return b


class _LimitReader:
    """io.LimitReader over the data chunk (wav.go:103)."""

    def __init__(self, r, n: int):
        self.r, self.n = r, n

    def read(self, k: int) -> bytes:
        k = min(k, self.n)
        if k <= 0:
            return b""
        b = self.r.read(k)
        self.n -= len(b)
        return b


@dataclass
class Wav(Header):
    """wav.Wav (wav.go:48-56). Duration is a Go time.Duration (int64 ns)."""
    Samples: int = 0
    Duration: int = 0
    _r: object = None

    def _sample_type(self):
        if self.AudioFormat == wavFormatPCM:
            if self.BitsPerSample == 8:
                return np.uint8
            if self.BitsPerSample == 16:
                return np.int16
            raise WavError(f"wav: unknown bits per sample: {self.BitsPerSample}")
        if self.AudioFormat == wavFormatIEEEFloat:
            return np.float32
        raise WavError("wav: unknown audio format")

    def _read_raw(self, n: int):
        typ = np.dtype(self._sample_type()).newbyteorder("<")
        # binary.Read: io.ReadFull of the whole slice
        return _read_full(self._r, n * typ.itemsize), typ

    def ReadSamples(self, n: int) -> np.ndarray:
        """wav.go:110-131: n samples as uint8, int16 or float32."""
        raw, typ = self._read_raw(n)
        return np.frombuffer(raw, dtype=typ).astype(typ.newbyteorder("="))

    def ReadFloats(self, n: int) -> np.ndarray:
        """wav.go:135-161: n samples converted to float32 (on the GPU)."""
        raw, _ = self._read_raw(n)
        return read_floats(raw, n, self.AudioFormat, self.BitsPerSample)


def New(r) -> Wav:
    """wav.New — wav.go:59-107: reads the RIFF/WAVE header and the fmt chunk,
    skips other chunks, and stops at the data chunk. r: a binary file-like
    object (read(n))."""
    w = Wav()
    header = _read_full(r, 12)
    if header[0:4] != b"RIFF":
        raise WavError("wav: missing RIFF")
    if header[8:12] != b"WAVE":
        raise WavError("wav: missing WAVE")
    has_fmt = False
    while True:
        ch = _read_full(r, 8)
        sz = struct.unpack("<I", ch[4:8])[0]
        typ = ch[:4]
        if typ == b"fmt ":
            if sz < 16:
                raise WavError("wav: bad fmt size")
            f = _read_full(r, sz)
            (w.AudioFormat, w.NumChannels, w.SampleRate, w.ByteRate, w.BlockAlign,
             w.BitsPerSample) = struct.unpack("<HHIIHH", f[:16])
            if w.AudioFormat not in (wavFormatPCM, wavFormatIEEEFloat):
                raise WavError(f"wav: unknown audio format: {w.AudioFormat:02x}")
            has_fmt = True
        elif typ == b"data":
            if not has_fmt:
                raise WavError("wav: unexpected fmt chunk")
            if w.BitsPerSample == 0:
                raise WavError("runtime error: integer divide by zero")
            w.Samples = int(sz) // int(w.BitsPerSample) * 8
            if w.SampleRate == 0 or w.NumChannels == 0:
                raise WavError("runtime error: integer divide by zero")
            w.Duration = _go_div(_go_div(w.Samples * 1_000_000_000, w.SampleRate), w.NumChannels)
            w._r = _LimitReader(r, int(sz))
            return w
        else:
            r.read(sz)  # io.CopyN(ioutil.Discard, r, sz); its error is ignored


def _go_div(a: int, b: int) -> int:
    """Go integer division (truncates toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _format_ok(audio_format: int, bits: int):
    if audio_format == wavFormatPCM and bits not in (8, 16):
        raise WavError(f"wav: unknown bits per sample: {bits}")
    if audio_format not in (wavFormatPCM, wavFormatIEEEFloat):
        raise WavError("wav: unknown audio format")


def read_floats(raw, count: int, audio_format: int, bits: int, f64: bool = False) -> np.ndarray:
    """ReadFloats's conversion of `count` little-endian samples in `raw`
    (bytes-like) on the GPU: float32, or float64 (the float32 values widened,
    a Pwelch input) with f64=True."""
    _format_ok(audio_format, bits)
    buf = np.frombuffer(bytes(raw), dtype=np.uint8)
    out = np.empty(count, np.float64 if f64 else np.float32)
    if count:
        check(lib().gdsp_wav_read_floats(buf.ctypes.data_as(_lib._P), count, audio_format, bits,
                                         out.ctypes.data_as(_lib._P), int(f64)),
              "wav.ReadFloats")
    return out


def device_floats(raw_dev, count: int, audio_format: int, bits: int, out=None, stream=None):
    """The GPU feeder: decode `count` samples from a uint8 CUDA tensor holding
    a data chunk into a float64 CUDA tensor (gdsp_wav_read_floats_device),
    ordered on `stream` — the HBM-resident input of device Pwelch."""
    import torch

    from . import device
    _format_ok(audio_format, bits)
    assert raw_dev.is_cuda and raw_dev.dtype == torch.uint8 and raw_dev.is_contiguous()
    if out is None:
        out = torch.empty(count, dtype=torch.float64, device=raw_dev.device)
    assert out.dtype == torch.float64 and out.numel() >= count
    with torch.cuda.device(raw_dev.device):
        check(lib().gdsp_wav_read_floats_device(
            ctypes.c_void_p(raw_dev.data_ptr()), count, audio_format, bits,
            ctypes.c_void_p(out.data_ptr()), 1, device._stream_ptr(stream, raw_dev.device)),
            "wav_read_floats_device")
    return out


def device_floats_planar(raw_dev, frames: int, channels: int, audio_format: int, bits: int,
                         out=None, stream=None):
    """device_floats for a multi-channel data chunk: `frames` interleaved
    frames of `channels` samples from a uint8 CUDA tensor into a (channels,
    frames) float64 CUDA tensor, out[c, i] = sample c of frame i
    (gdsp_wav_read_floats_planar_device). out: any row stride >= frames."""
    import torch

    from . import device
    _format_ok(audio_format, bits)
    assert raw_dev.is_cuda and raw_dev.dtype == torch.uint8 and raw_dev.is_contiguous()
    assert raw_dev.numel() >= frames * channels * (4 if audio_format == wavFormatIEEEFloat
                                                   else bits // 8)
    if out is None:
        out = torch.empty((channels, frames), dtype=torch.float64, device=raw_dev.device)
    assert out.dtype == torch.float64 and tuple(out.shape) == (channels, frames)
    assert frames == 0 or out.stride(1) == 1
    ld = out.stride(0) if channels > 1 else frames
    with torch.cuda.device(raw_dev.device):
        check(lib().gdsp_wav_read_floats_planar_device(
            ctypes.c_void_p(raw_dev.data_ptr()), frames, channels, audio_format, bits,
            ctypes.c_void_p(out.data_ptr()), ld, device._stream_ptr(stream, raw_dev.device)),
            "wav_read_floats_planar_device")
    return out


def PwelchChannels(w: Wav, frames: int, o, Fs: float = 0.0):
    """The per-channel spectra of a multi-channel file: the next `frames`
    frames of w (frames * w.NumChannels samples), decoded planar on the GPU
    and run through device.pwelch_batch. Returns (Pxx[NumChannels, lp],
    freqs) as numpy arrays; row c equals spectral.Pwelch(float64(
    w.ReadFloats(frames * C))[c::C], Fs, o). Fs defaults to w.SampleRate."""
    import torch

    from . import device
    spectral.resolve_options(o)
    C = int(w.NumChannels)
    raw, _ = w._read_raw(frames * C)
    if frames == 0:  # pwelch.go:75-77
        return np.zeros((C, 0)), np.zeros(0)
    fs = float(Fs or w.SampleRate)
    dev = torch.device("cuda", torch.cuda.current_device())
    rd = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    x = device_floats_planar(rd, frames, C, w.AudioFormat, w.BitsPerSample)
    pxx, freqs = device.pwelch_batch(x, fs, o)
    return pxx.cpu().numpy(), freqs


def SpectrogramChannels(w: Wav, frames: int, o, Fs: float = 0.0):
    """The per-channel spectrograms of a multi-channel file: the next `frames`
    frames of w, decoded planar on the GPU as for PwelchChannels and run
    through device.spectrogram_batch. Returns (P[NumChannels, nsegs, lp],
    freqs, times) as numpy arrays; P[c] equals spectral.Spectrogram of channel
    c's decoded samples, and its mean over the segments PwelchChannels' row c.
    Fs defaults to w.SampleRate."""
    import torch

    from . import device
    spectral.resolve_options(o)
    C = int(w.NumChannels)
    raw, _ = w._read_raw(frames * C)
    if frames == 0:  # pwelch.go:75-77
        return np.zeros((C, 0, 0)), np.zeros(0), np.zeros(0)
    fs = float(Fs or w.SampleRate)
    dev = torch.device("cuda", torch.cuda.current_device())
    rd = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    x = device_floats_planar(rd, frames, C, w.AudioFormat, w.BitsPerSample)
    p, freqs, times = device.spectrogram_batch(x, fs, o)
    return p.cpu().numpy(), freqs, times


def CoherenceChannels(w: Wav, frames: int, o, ref: int = 0, Fs: float = 0.0):
    """The magnitude-squared coherence of every channel of a multi-channel
    file with channel `ref`: the next `frames` frames of w, decoded planar on
    the GPU as for PwelchChannels and run through device.cpsd_batch. Returns
    (Cxy[NumChannels, lp], freqs) as numpy arrays; row c equals
    spectral.Coherence(channel c, channel ref, Fs, o) (row ref is 1 wherever
    the channel holds power). Fs defaults to w.SampleRate."""
    import torch

    from . import device
    spectral.resolve_options(o)
    C = int(w.NumChannels)
    if not 0 <= ref < C:
        raise _lib.GDSPError(_lib.GDSP_ERR_INVALID, f"reference channel {ref} of {C}")
    raw, _ = w._read_raw(frames * C)
    if frames == 0:  # pwelch.go:75-77
        return np.zeros((C, 0)), np.zeros(0)
    fs = float(Fs or w.SampleRate)
    dev = torch.device("cuda", torch.cuda.current_device())
    rd = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    x = device_floats_planar(rd, frames, C, w.AudioFormat, w.BitsPerSample)
    r = device.cpsd_batch(x, x[ref], fs, o)
    return r.Cxy.cpu().numpy(), r.freqs


def FilterChannels(w: Wav, frames: int, h, full: bool = False):
    """Every channel of a multi-channel file through a FIR filter: the next
    `frames` frames of w, decoded planar on the GPU as for PwelchChannels and
    run through device.fir_batch with the real taps h ((m,): one filter for
    all channels, or (NumChannels, m)). Returns a (NumChannels, out_len)
    numpy array, out_len = frames, or frames + m - 1 with full=True; row c
    equals fft.FIRFilterBatch of channel c's decoded samples."""
    import torch

    from . import device
    if np.iscomplexobj(h):
        raise TypeError("FilterChannels: complex taps are not supported")
    h = np.asarray(h, dtype=np.float64)
    C = int(w.NumChannels)
    if h.ndim not in (1, 2) or (h.ndim == 2 and h.shape[0] != C):
        raise _lib.Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size")
    h = np.ascontiguousarray(h)
    raw, _ = w._read_raw(frames * C)
    dev = torch.device("cuda", torch.cuda.current_device())
    rd = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    x = device_floats_planar(rd, frames, C, w.AudioFormat, w.BitsPerSample)
    out = device.fir_batch(x, torch.from_numpy(h).to(dev), full=full)
    return out.cpu().numpy()


def EnvelopeChannels(w: Wav, frames: int, N=None):
    """The envelope of every channel of a multi-channel file: the next
    `frames` frames of w, decoded planar on the GPU as for FilterChannels and
    run through device.hilbert_batch(kind="envelope") at transform length N
    (None: frames). Returns a (NumChannels, N) numpy array; row c equals
    fft.EnvelopeBatch of channel c's decoded samples."""
    import torch

    from . import device
    C = int(w.NumChannels)
    raw, _ = w._read_raw(frames * C)
    nfft = frames if N is None else int(N)
    if frames == 0 or nfft == 0:
        raise _lib.Panic(_lib.GDSP_ERR_EMPTY, "empty input array")
    dev = torch.device("cuda", torch.cuda.current_device())
    rd = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    x = device_floats_planar(rd, frames, C, w.AudioFormat, w.BitsPerSample)
    return device.hilbert_batch(x, nfft, kind="envelope").cpu().numpy()


def IIRFilterChannels(w: Wav, frames: int, sos, zero_phase: bool = False):
    """Every channel of a multi-channel file through a recursive filter: the
    next `frames` frames of w, decoded planar on the GPU as for FilterChannels
    and run through device.sosfilt_batch with the sections sos ((S, 6)), or
    through device.sosfiltfilt_batch with zero_phase=True. Returns a
    (NumChannels, frames) numpy array; row c equals fft.SosFiltBatch (or
    SosFiltFiltBatch) of channel c's decoded samples."""
    import torch

    from . import device
    C = int(w.NumChannels)
    raw, _ = w._read_raw(frames * C)
    if frames == 0:
        raise _lib.Panic(_lib.GDSP_ERR_EMPTY, "empty input array")
    dev = torch.device("cuda", torch.cuda.current_device())
    rd = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    x = device_floats_planar(rd, frames, C, w.AudioFormat, w.BitsPerSample)
    if zero_phase:
        return device.sosfiltfilt_batch(x, sos).cpu().numpy()
    return device.sosfilt_batch(x, sos, out=x).cpu().numpy()


def ZoomChannels(w: Wav, frames: int, fn, m=None, endpoint: bool = False):
    """The zoomed spectrum of every channel of a multi-channel file: the next
    `frames` frames of w, decoded planar on the GPU as for FilterChannels and
    run through device.zoom_fft_batch at m frequencies (None: frames) from f1
    to f2 Hz (fn = [f1, f2] or f2), at the file's sample rate. Returns a
    (NumChannels, m) complex128 numpy array; row c equals fft.ZoomFFTBatch of
    channel c's decoded samples."""
    import torch

    from . import device
    C = int(w.NumChannels)
    raw, _ = w._read_raw(frames * C)
    mm = frames if m is None else int(m)
    if frames == 0 or mm == 0:
        raise _lib.Panic(_lib.GDSP_ERR_EMPTY, "empty input array")
    dev = torch.device("cuda", torch.cuda.current_device())
    rd = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    x = device_floats_planar(rd, frames, C, w.AudioFormat, w.BitsPerSample)
    return device.zoom_fft_batch(x, fn, mm, float(w.SampleRate), endpoint).cpu().numpy()


def ResampleChannels(w: Wav, frames: int, rate: int):
    """Every channel of a multi-channel file at the sample rate `rate`: the
    next `frames` frames of w, decoded planar on the GPU as for FilterChannels
    and run through device.resample_poly_batch with up / down = rate /
    w.SampleRate reduced. Returns a (NumChannels, ceil(frames up / down))
    numpy array; row c equals fft.ResamplePolyBatch of channel c's decoded
    samples."""
    import torch

    from . import device, fft
    up, down = fft._rate_pair(int(rate), int(w.SampleRate))
    C = int(w.NumChannels)
    raw, _ = w._read_raw(frames * C)
    if frames == 0:
        return np.zeros((C, 0))
    dev = torch.device("cuda", torch.cuda.current_device())
    rd = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    x = device_floats_planar(rd, frames, C, w.AudioFormat, w.BitsPerSample)
    return device.resample_poly_batch(x, up, down).cpu().numpy()


def Pwelch(w: Wav, n: int, o, Fs: float = 0.0):
    """The feeder end to end: the next n samples of w, decoded on the GPU
    into float64 and run through the device Pwelch (no host float pass);
    Fs defaults to w.SampleRate. Equals spectral.Pwelch(float64(
    w.ReadFloats(n)), Fs, o) — the reference's pipeline (pwelch.go:74)."""
    import torch

    from . import distributed
    nfft, pad, nov, _, _ = spectral.resolve_options(o)
    raw, _ = w._read_raw(n)
    if n == 0:  # pwelch.go:75-77
        return np.zeros(0), np.zeros(0)
    fs = float(Fs or w.SampleRate)
    dev = torch.device("cuda", torch.cuda.current_device())
    rd = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    x = device_floats(rd, n, w.AudioFormat, w.BitsPerSample)
    if n < nfft:  # pwelch.go:97-99: zero-padded to nfft
        x = torch.cat([x, torch.zeros(nfft - n, dtype=torch.float64, device=dev)])
    sh = distributed.plan_pwelch(n, 1, 0, nfft, pad, nov)
    return distributed.pwelch(x, fs, o, sh)
