"""Circular-buffer rate matching and LLR rate recovery (3GPP TS 38.212 §5.4.2) on the device: the step that decides
which bits of an encoded word are sent, and its inverse in front of the decoder.

RateMatch      the parameters (nldpc_rm of include/nldpc.h); RateMatch.nr5g resolves a 5G redundancy version.
index          host: the codeword bit index every sent bit carries (nldpc_rm_index; no GPU needed).
code_rate      (K*Z - F) / E, for channel.sigma_for.
rate_match     codewords [B, N*Z] -> sent bits [B, E] (nldpc_rate_match).
rate_recover   received LLRs [B, E] -> decoder input [B, N, Z], repetitions and further redundancy versions
               soft-combined (nldpc_rate_recover).

The channel between the two is channel.awgn_llr(B, E, 1, sigma, y=f).reshape(B, E) for BPSK (qm = 1), or
modulation.qam_llr(f, qm, sigma) for 2^qm-QAM with qm = 2, 4, 6, 8: a symbol takes qm consecutive bits of f, the
groups the interleaver forms with RateMatch(qm=qm).

Unsent positions get `erasure_value`.  An exact 0 is NOT an erasure for the Neural decoder: the reference's check node
masks zeros out of its minimum (NeuralLDPCDecoder.py:74-75), so an unsent degree-1 extension column drops out of its
check and the check asserts a wrong parity.  Rate-matched Neural decoding needs a small non-zero value (1e-3, what the
reference's datagen uses for SP); the default stays 0.0 like awgn_llr's puncture_value.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import torch

from . import _lib


@dataclasses.dataclass(frozen=True)
class RateMatch:
    """E bits sent per codeword, from buffer position k0 on; punct_cols leading base columns are never sent (5G: 2),
    the last n_filler info bits are known zeros and skipped, ncb limits the buffer (0 = all of it), qm is the number of
    interleaver rows (1 = no interleaver; divides E)."""
    E: int
    k0: int = 0
    punct_cols: int = 0
    n_filler: int = 0
    ncb: int = 0
    qm: int = 1

    @classmethod
    def nr5g(cls, graph, E: int, *, bg: int = 2, rv: int = 0, n_filler: int = 0, ncb: int = 0, qm: int = 1):
        """5G NR: two punctured columns, k0 of redundancy version rv from Table 5.4.2.1-2 over the resolved Ncb."""
        resolved = int(ncb) if ncb else graph.N * graph.Z - 2 * graph.Z
        k0 = ctypes.c_int64()
        _lib.check(_lib.lib().nldpc_rm_k0(int(bg), int(rv), resolved, graph.Z, ctypes.byref(k0)), "nldpc_rm_k0")
        return cls(E=int(E), k0=int(k0.value), punct_cols=2, n_filler=int(n_filler), ncb=int(ncb), qm=int(qm))

    def _c(self) -> _lib.NldpcRm:
        vals = (self.punct_cols, self.qm, self.n_filler, self.ncb, self.k0, self.E)
        if any(int(v) != v for v in vals) or not all(-2 ** 31 <= v < 2 ** 31 for v in vals[:2]) or \
                not all(-2 ** 63 <= v < 2 ** 63 for v in vals[2:]):
            raise ValueError(f"rate matching parameters must be integers in range: {self}")
        return _lib.NldpcRm(*(int(v) for v in vals))


def index(graph, rm: RateMatch) -> np.ndarray:
    """np.int32 [E]: idx[m] is the codeword bit (0 .. N*Z-1) sent as bit m.  Host only."""
    c = rm._c()
    # (an E the library rejects is rejected before anything is written: one element is room enough for that answer)
    idx = np.zeros(rm.E if 1 <= rm.E < 2 ** 31 else 1, dtype=np.int32)
    _lib.check(_lib.lib().nldpc_rm_index(graph.M, graph.N, graph.Z, ctypes.byref(c),
                                         idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "nldpc_rm_index")
    return idx


def code_rate(graph, rm: RateMatch) -> float:
    """Information bits per sent bit, (K*Z - F) / E."""
    return (graph.K * graph.Z - rm.n_filler) / rm.E


def _device_of(t: torch.Tensor, what: str) -> torch.device:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{what} must be a tensor on the ROCm device (no CPU path)")
    return t.device


def rate_match(graph, rm: RateMatch, y: torch.Tensor, *, out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 [B, E] sent bits (0 / 1) of the codewords y: contiguous uint8 [B, N*Z] on the device, any non-zero byte
    counts as 1 (channel.encode's output)."""
    dev = _device_of(y, "y")
    L = graph.N * graph.Z
    if y.dtype != torch.uint8 or y.dim() != 2 or y.shape[1] != L or y.shape[0] < 1 or not y.is_contiguous():
        raise ValueError(f"y must be a contiguous uint8 [B, N*Z] = [B, {L}] tensor")
    B, c = int(y.shape[0]), rm._c()
    if out is None:
        if not 1 <= rm.E < 2 ** 31:
            raise ValueError("E must be in [1, 2^31)")
        out = torch.empty((B, rm.E), dtype=torch.uint8, device=dev)
    elif _device_of(out, "out") != dev or out.dtype != torch.uint8 or tuple(out.shape) != (B, rm.E) or \
            not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 [{B}, {rm.E}] tensor on {dev}")
    _lib.check(_lib.lib().nldpc_rate_match(graph.handle(dev), ctypes.byref(c), y.data_ptr(), B, out.data_ptr(),
                                           _lib.stream_of(dev)), "nldpc_rate_match")
    return out


def rate_recover(graph, rm: RateMatch, llr: torch.Tensor, *, out: torch.Tensor | None = None,
                 accumulate: bool = False, erasure_value: float = 0.0, filler_value: float = -20.0,
                 clip: float = 0.0) -> torch.Tensor:
    """fp32 [B, N, Z] decoder input from the received LLRs llr: contiguous fp32 [B, E] on the device, in the order
    of rate_match's output.  Every received copy of a bit is added (ascending selection index, fp32) to +0, or with
    accumulate=True to what `out` already holds (HARQ: call once per redundancy version on the same `out`); clip > 0
    clamps the sums to [-clip, clip].  Filler positions are set to filler_value (-|llr_hi|); positions that received
    nothing are set to erasure_value, or with accumulate=True left as they are.  For the Neural decoder erasure_value
    must be a small non-zero number (1e-3), not 0: its check node does not treat an exact zero as an erasure (module
    docstring)."""
    dev = _device_of(llr, "llr")
    if llr.dtype != torch.float32 or llr.dim() != 2 or llr.shape[1] != rm.E or llr.shape[0] < 1 or \
            not llr.is_contiguous():
        raise ValueError(f"llr must be a contiguous float32 [B, E] = [B, {rm.E}] tensor")
    B, c = int(llr.shape[0]), rm._c()
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True adds to `out`: pass the tensor an earlier rate_recover filled")
        out = torch.empty((B, graph.N, graph.Z), dtype=torch.float32, device=dev)
    elif _device_of(out, "out") != dev or out.dtype != torch.float32 or \
            tuple(out.shape) != (B, graph.N, graph.Z) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 [{B}, {graph.N}, {graph.Z}] tensor on {dev}")
    _lib.check(_lib.lib().nldpc_rate_recover(graph.handle(dev), ctypes.byref(c), llr.data_ptr(), B,
                                             float(erasure_value), float(filler_value), float(clip),
                                             1 if accumulate else 0, out.data_ptr(), _lib.stream_of(dev)),
               "nldpc_rate_recover")
    return out
