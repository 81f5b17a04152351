"""QAM modulation and soft demapping on the device (3GPP TS 38.211 §5.1.3-5.1.6: QPSK, 16-, 64-, 256-QAM), the channel
between ratematch.rate_match and ratematch.rate_recover for qm = 2, 4, 6, 8 (qm = 1, BPSK, is channel.awgn_llr).

points         host: the 2^qm constellation points (nldpc_qam_points; no GPU needed).
modulate       sent bits [B, E] -> symbols [B, E/qm, 2] (I, Q) (nldpc_qam_modulate).
demap          symbols -> LLRs [B, E] in the order of the bits, max-log or log-MAP (nldpc_qam_demap).
qam_llr        the fused channel: bits -> symbols -> AWGN -> LLRs in one kernel (nldpc_qam_channel_llr); the noise comes
               from Philox-4x32-10 at the global symbol index, so a batch sharded over ranks draws the noise of the
               unsharded batch.  scramble= a table of scrambling.sequence: Gold-sequence scrambling in front of the
               mapper and descrambling behind the demapper inside the same kernel.
sigma_for      Eb/N0 -> noise standard deviation per real dimension at unit symbol energy.

A symbol carries qm consecutive bits of a row, f[b, s*qm : (s+1)*qm]: the grouping RateMatch(qm=qm)'s interleaver
produces.  LLR > 0 means bit 1, the decoders' convention.  The definitions are in include/nldpc.h.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib

ORDERS = (2, 4, 6, 8)
METHODS = {"maxlog": 0, "logmap": 1}
_FP = ctypes.POINTER(ctypes.c_float)


def _order(qm) -> int:
    if isinstance(qm, bool) or int(qm) != qm or int(qm) not in ORDERS:
        raise ValueError(f"qm must be one of {ORDERS} (qm = 1 is channel.awgn_llr), got {qm!r}")
    return int(qm)


def _method(method) -> int:
    if method not in METHODS:
        raise ValueError(f"method must be one of {sorted(METHODS)}, got {method!r}")
    return METHODS[method]


def _sigma(sigma) -> float:
    s = float(sigma)
    if not s > 0.0 or not float(np.float32(s)) > 0.0:
        raise ValueError(f"sigma must be positive, got {sigma!r}")
    return s


def _device_of(t, what: str) -> torch.device:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{what} must be a tensor on the ROCm device (no CPU path)")
    return t.device


def _out(out, shape, dev, what="out") -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if _device_of(out, what) != dev or out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or \
            not out.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 {list(shape)} tensor on {dev}")
    return out


def _bits(f, qm: int):
    dev = _device_of(f, "f")
    if f.dtype != torch.uint8 or f.dim() != 2 or f.shape[0] < 1 or f.shape[1] < 1 or not f.is_contiguous():
        raise ValueError("f must be a contiguous uint8 [B, E] tensor")
    B, E = int(f.shape[0]), int(f.shape[1])
    if E % qm or E >= 2 ** 31:
        raise ValueError(f"E = {E} must be a multiple of qm = {qm} below 2^31")
    return dev, B, E


def sigma_for(ebn0_db: float, code_rate: float, qm: int) -> float:
    """Noise standard deviation per real dimension for unit average symbol energy: Es/N0 = qm * R * Eb/N0, N0 = 2 sigma^2."""
    return math.sqrt(1.0 / (2.0 * qm * code_rate * 10.0 ** (ebn0_db / 10.0)))


def points(qm: int) -> np.ndarray:
    """complex64 [2^qm]: point v is the symbol of the bits b_i = (v >> (qm-1-i)) & 1.  Host only."""
    qm = _order(qm)
    iq = np.zeros((2 ** qm, 2), dtype=np.float32)
    _lib.check(_lib.lib().nldpc_qam_points(qm, iq.ctypes.data_as(_FP)), "nldpc_qam_points")
    return iq.view(np.complex64).reshape(-1)


def modulate(f: torch.Tensor, qm: int, *, out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [B, E/qm, 2] symbols (I, Q) of the bits f: contiguous uint8 [B, E] on the device, any non-zero byte counts
    as 1 (ratematch.rate_match's output)."""
    qm = _order(qm)
    dev, B, E = _bits(f, qm)
    out = _out(out, (B, E // qm, 2), dev)
    with torch.cuda.device(dev):  # (the launch goes to the current device)
        _lib.check(_lib.lib().nldpc_qam_modulate(qm, f.data_ptr(), B, E, out.data_ptr(), _lib.stream_of(dev)),
                   "nldpc_qam_modulate")
    return out


def demap(sym: torch.Tensor, qm: int, sigma: float, *, method: str = "maxlog",
          out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [B, S*qm] LLRs (> 0: bit 1) of the received symbols sym: contiguous fp32 [B, S, 2] on the device; sigma is
    the noise standard deviation per real dimension.  method "maxlog" or "logmap"."""
    qm, m, sigma = _order(qm), _method(method), _sigma(sigma)
    dev = _device_of(sym, "sym")
    if sym.dtype != torch.float32 or sym.dim() != 3 or sym.shape[2] != 2 or sym.shape[0] < 1 or sym.shape[1] < 1 or \
            not sym.is_contiguous():
        raise ValueError("sym must be a contiguous float32 [B, S, 2] tensor")
    B, S = int(sym.shape[0]), int(sym.shape[1])
    out = _out(out, (B, S * qm), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_qam_demap(qm, m, sigma, sym.data_ptr(), B, S, out.data_ptr(),
                                              _lib.stream_of(dev)), "nldpc_qam_demap")
    return out


def qam_llr(f: torch.Tensor | None, qm: int, sigma: float, *, B: int | None = None, E: int | None = None,
            seed: int = 2042, b_offset: int = 0, method: str = "maxlog", device=None,
            out: torch.Tensor | None = None, return_symbols: bool | torch.Tensor = False,
            scramble: torch.Tensor | None = None):
    """fp32 [B, E] LLRs of the bits f (contiguous uint8 [B, E] on the device, or None: the all-zero word, with B and E
    given) sent as 2^qm-QAM symbols over AWGN of standard deviation sigma per real dimension and demapped, in one
    kernel.  The noise of codeword b is that of codeword b_offset + b of the stream of `seed`.  return_symbols: True
    (or a contiguous fp32 [B, E/qm, 2] tensor to fill) also returns the noisy symbols, as (llr, symbols); the LLRs are
    bit for bit demap(symbols, qm, sigma, method=method).  scramble: a table of scrambling.sequence for rows of E bits:
    f ^ c goes into the mapper and the LLRs come out descrambled (nldpc_qam_channel_llr_scrambled), bit for bit
    scrambling.descramble(qam_llr(scrambling.scramble(f, table), ...), table) with b_offset also selecting the row's
    sequence; the symbols returned are then those of the scrambled bits, and the LLRs are no longer their demap."""
    qm, m, sigma = _order(qm), _method(method), _sigma(sigma)
    if f is not None:
        dev, fB, fE = _bits(f, qm)
        if (B is not None and B != fB) or (E is not None and E != fE):
            raise ValueError(f"f is [{fB}, {fE}], not [B, E] = [{B}, {E}]")
        B, E = fB, fE
    else:
        if B is None or E is None:
            raise ValueError("qam_llr needs f, or B and E for the all-zero word")
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise ValueError("qam_llr runs on the ROCm device (no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        B, E = int(B), int(E)
        if B < 1 or E < 1 or E % qm or E >= 2 ** 31:
            raise ValueError(f"B must be positive and E = {E} a positive multiple of qm = {qm} below 2^31")
    if int(b_offset) < 0:
        raise ValueError("b_offset must not be negative")
    out = _out(out, (B, E), dev)
    sym = None
    if isinstance(return_symbols, torch.Tensor):
        sym = _out(return_symbols, (B, E // qm, 2), dev, "return_symbols")
    elif return_symbols:
        sym = torch.empty((B, E // qm, 2), dtype=torch.float32, device=dev)
    if scramble is not None:
        from .scrambling import _on, _table
        n_seq = _table(scramble, E)
        _on(dev, scramble)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().nldpc_qam_channel_llr_scrambled(
                qm, m, _lib.ptr(f), B, E, sigma, int(seed) & (2 ** 64 - 1), int(b_offset), scramble.data_ptr(), n_seq,
                out.data_ptr(), _lib.ptr(sym), _lib.stream_of(dev)), "nldpc_qam_channel_llr_scrambled")
        return out if sym is None else (out, sym)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_qam_channel_llr(qm, m, _lib.ptr(f), B, E, sigma, int(seed) & (2 ** 64 - 1),
                                                    int(b_offset), out.data_ptr(), _lib.ptr(sym),
                                                    _lib.stream_of(dev)), "nldpc_qam_channel_llr")
    return out if sym is None else (out, sym)
