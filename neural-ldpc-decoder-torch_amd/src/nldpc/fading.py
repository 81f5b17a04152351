"""Flat block fading with perfect channel state information for the QAM channel on the device: modulation.qam_llr with a
real gain g >= 0 between the mapper and the noise (the channel's magnitude after the receiver's exact phase
de-rotation) and a demapper that knows g.  qm = 2, 4, 6, 8; BPSK is not covered.

n_blocks       fading blocks per row: ceil(S / L), 1 when L >= S.
gains          the drawn gain table [B, n_blk] (nldpc_fading_gains): Rician with factor K (K = 0: Rayleigh), E[g^2] = 1.
demap          symbols [B, S, 2] and a gain table -> LLRs [B, S*qm] (nldpc_qam_demap_csi): the demapper of
               modulation.demap on the levels g * level.
qam_llr        the fused channel: bits -> (scramble) -> symbols -> gain -> AWGN -> CSI demap -> (descramble) in one
               kernel (nldpc_qam_fading_channel_llr), with drawn or given gains.

Gains are constant over L consecutive symbols of a row (the coherence length; the last block of a row may be short,
blocks never span rows): L = 1 is fast fading, L >= S one gain per row.  The noise of a symbol is the one
modulation.qam_llr draws for it at the same seed and b_offset, and unit gains reproduce it bit for bit.  The gains come
from Philox-4x32-10 at the global block index, so a batch sharded over ranks draws the gains (and the noise) of the
unsharded batch.  sigma means what it means there (modulation.sigma_for).  The definitions are in include/nldpc.h.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .modulation import _bits, _device_of, _method, _order, _out, _sigma


def _length(L) -> int:
    if isinstance(L, bool) or int(L) != L or not 1 <= int(L) < 2 ** 63:
        raise ValueError(f"L must be an integer >= 1, got {L!r}")
    return int(L)


def _rician(K) -> float:
    k = float(K)
    if not (k >= 0.0 and math.isfinite(k)):
        raise ValueError(f"K must be finite and not negative, got {K!r}")
    return k


def _offset(b_offset) -> int:
    if int(b_offset) < 0:
        raise ValueError("b_offset must not be negative")
    return int(b_offset)


def _device(device, *tensors) -> torch.device:
    for t in tensors:
        if isinstance(t, torch.Tensor):
            return _device_of(t, "out")
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise ValueError("nldpc.fading runs on the ROCm device (no CPU path)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _table(gain, B: int, n_blk: int, dev: torch.device) -> torch.Tensor:
    """a given gain table; its values must be finite and >= 0, which is not checked (it would take a synchronisation)"""
    if _device_of(gain, "gain") != dev or gain.dtype != torch.float32 or tuple(gain.shape) != (B, n_blk) or \
            not gain.is_contiguous():
        raise ValueError(f"gain must be a contiguous float32 {[B, n_blk]} tensor on {dev}")
    return gain


def n_blocks(S: int, L: int = 1) -> int:
    """fading blocks per row of S symbols with coherence length L: ceil(S / L)"""
    S, L = int(S), _length(L)
    if S < 1:
        raise ValueError("S must be positive")
    return 1 if L >= S else -(-S // L)


def gains(B: int, S: int, *, L: int = 1, K: float = 0.0, seed: int = 2042, b_offset: int = 0, device=None,
          out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [B, n_blocks(S, L)]: the gains qam_llr draws for rows b_offset .. b_offset + B - 1 of the stream of `seed`
    with Rician factor K (0: Rayleigh)."""
    B, n_blk, K, b_offset = int(B), n_blocks(S, L), _rician(K), _offset(b_offset)
    if B < 1 or B * n_blk >= 2 ** 31:
        raise ValueError("B must be positive and B * n_blocks(S, L) below 2^31")
    dev = _device(device, out)
    out = _out(out, (B, n_blk), dev)
    with torch.cuda.device(dev):  # (the launch goes to the current device)
        _lib.check(_lib.lib().nldpc_fading_gains(K, int(seed) & (2 ** 64 - 1), B, n_blk, b_offset, out.data_ptr(),
                                                 _lib.stream_of(dev)), "nldpc_fading_gains")
    return out


def demap(sym: torch.Tensor, qm: int, sigma: float, gain: torch.Tensor, *, L: int = 1, method: str = "maxlog",
          out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [B, S*qm] LLRs (> 0: bit 1) of the received symbols sym (contiguous fp32 [B, S, 2] on the device) that
    passed through the gains `gain` (contiguous fp32 [B, n_blocks(S, L)], finite and >= 0); sigma is the noise standard
    deviation per real dimension.  method "maxlog" or "logmap"."""
    qm, m, sigma, L = _order(qm), _method(method), _sigma(sigma), _length(L)
    dev = _device_of(sym, "sym")
    if sym.dtype != torch.float32 or sym.dim() != 3 or sym.shape[2] != 2 or sym.shape[0] < 1 or sym.shape[1] < 1 or \
            not sym.is_contiguous():
        raise ValueError("sym must be a contiguous float32 [B, S, 2] tensor")
    B, S = int(sym.shape[0]), int(sym.shape[1])
    gain = _table(gain, B, n_blocks(S, L), dev)
    out = _out(out, (B, S * qm), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_qam_demap_csi(qm, m, sigma, sym.data_ptr(), gain.data_ptr(), B, S, L,
                                                  out.data_ptr(), _lib.stream_of(dev)), "nldpc_qam_demap_csi")
    return out


def qam_llr(f: torch.Tensor | None, qm: int, sigma: float, *, L: int = 1, K: float = 0.0,
            gain: torch.Tensor | None = None, B: int | None = None, E: int | None = None, seed: int = 2042,
            b_offset: int = 0, method: str = "maxlog", scramble: torch.Tensor | None = None, device=None,
            out: torch.Tensor | None = None, return_symbols: bool | torch.Tensor = False,
            return_gains: bool | torch.Tensor = False):
    """fp32 [B, E] LLRs of the bits f (contiguous uint8 [B, E] on the device, or None: the all-zero word, with B and E
    given) sent as 2^qm-QAM symbols through a flat block-fading channel of coherence length L and AWGN of standard
    deviation sigma per real dimension, and demapped with the gains known, in one kernel.  gain None: the gains are
    drawn, Rician with factor K, those of gains(B, E // qm, L=L, K=K, seed=seed, b_offset=b_offset); else gain is the
    table, contiguous fp32 [B, n_blocks(E // qm, L)], finite and >= 0.  The noise is modulation.qam_llr's at the same
    seed and b_offset.  scramble: a table of scrambling.sequence, used as modulation.qam_llr uses it.  return_symbols /
    return_gains: True (or a tensor to fill) also returns the received symbols [B, E/qm, 2] / the gains [B, n_blk]; the
    result is then the tuple (llr[, symbols][, gains]), and without scramble the LLRs are bit for bit
    demap(symbols, qm, sigma, gains, L=L, method=method)."""
    qm, m, sigma, L, K = _order(qm), _method(method), _sigma(sigma), _length(L), _rician(K)
    if f is not None:
        dev, fB, fE = _bits(f, qm)
        if (B is not None and B != fB) or (E is not None and E != fE):
            raise ValueError(f"f is [{fB}, {fE}], not [B, E] = [{B}, {E}]")
        B, E = fB, fE
    else:
        if B is None or E is None:
            raise ValueError("qam_llr needs f, or B and E for the all-zero word")
        dev = _device(device)
        B, E = int(B), int(E)
        if B < 1 or E < 1 or E % qm or E >= 2 ** 31:
            raise ValueError(f"B must be positive and E = {E} a positive multiple of qm = {qm} below 2^31")
    b_offset = _offset(b_offset)
    S = E // qm
    n_blk = n_blocks(S, L)
    if B * n_blk >= 2 ** 31:
        raise ValueError("B * n_blocks(E // qm, L) must be below 2^31")
    if gain is not None:
        gain = _table(gain, B, n_blk, dev)
    out = _out(out, (B, E), dev)
    sym = g_out = None
    if isinstance(return_symbols, torch.Tensor):
        sym = _out(return_symbols, (B, S, 2), dev, "return_symbols")
    elif return_symbols:
        sym = torch.empty((B, S, 2), dtype=torch.float32, device=dev)
    if isinstance(return_gains, torch.Tensor):
        g_out = _out(return_gains, (B, n_blk), dev, "return_gains")
        if gain is not None and g_out.data_ptr() == gain.data_ptr():
            raise ValueError("return_gains must not be the gain table itself")
    elif return_gains:
        g_out = torch.empty((B, n_blk), dtype=torch.float32, device=dev)
    n_seq = 0
    if scramble is not None:
        from .scrambling import _on, _table as _seq_table
        n_seq = _seq_table(scramble, E)
        _on(dev, scramble)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_qam_fading_channel_llr(
            qm, m, _lib.ptr(f), B, E, sigma, int(seed) & (2 ** 64 - 1), b_offset, L, K, _lib.ptr(gain),
            _lib.ptr(scramble), n_seq, out.data_ptr(), _lib.ptr(sym), _lib.ptr(g_out), _lib.stream_of(dev)),
            "nldpc_qam_fading_channel_llr")
    extra = tuple(t for t in (sym, g_out) if t is not None)
    return (out,) + extra if extra else out
