"""Bit scrambling with the length-31 Gold sequence of 3GPP TS 38.211 §5.2.1 (PUSCH §6.3.1.1, PDSCH §7.3.1.1) on the
device: the step between transport.rate_match_blocks and the mapper, and its inverse on the LLRs in front of
transport.rate_recover_blocks.

c_init         host: rnti * 2^15 + q * 2^14 + n_id (nldpc_gold_cinit).
gold           host: c(n0) .. c(n0 + n - 1) as uint8 (nldpc_gold_ref; no GPU needed).
sequence       c_init values -> the packed table int32 [n_seq, ceil(E / 32)] on the device (nldpc_gold_sequence).
scramble       bits [B, E] -> bits ^ c (nldpc_scramble); f = None scrambles the all-zero word.
descramble     LLRs [B, E] -> LLRs with the sign bit XORed with c (nldpc_descramble_llr).

Row b of a batch uses sequence (b_offset + b) mod n_seq of the table: one row for every codeword, or one per transport
block.  modulation.qam_llr(scramble=table) does both steps inside the fused channel.  Bit n of a sequence is bit n & 31
of word n >> 5 of its row.  The definitions are in include/nldpc.h.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .modulation import _device_of, _out


def _words(E: int) -> int:
    return (int(E) + 31) // 32


def _length(E) -> int:
    if isinstance(E, bool) or int(E) != E or not 1 <= int(E) < 2 ** 31:
        raise ValueError(f"E must be an integer in [1, 2^31), got {E!r}")
    return int(E)


def _table(seq, E: int) -> int:
    """n_seq of a sequence table for rows of E bits (its device is checked by _on)"""
    if not isinstance(seq, torch.Tensor) or seq.dtype != torch.int32 or seq.dim() != 2 or seq.shape[0] < 1 or \
            not seq.is_contiguous():
        raise ValueError("seq must be a contiguous int32 [n_seq, ceil(E / 32)] tensor (scrambling.sequence)")
    if seq.shape[1] != _words(E):
        raise ValueError(f"seq has {seq.shape[1]} words per sequence, E = {E} needs {_words(E)}")
    return int(seq.shape[0])


def _on(dev: torch.device, seq) -> None:
    if _device_of(seq, "seq") != dev:
        raise ValueError(f"seq must be on {dev}")


def _offset(b_offset) -> int:
    if int(b_offset) < 0:
        raise ValueError("b_offset must not be negative")
    return int(b_offset)


def c_init(rnti: int, n_id: int, q: int = 0) -> int:
    """rnti * 2^15 + q * 2^14 + n_id (TS 38.211 §7.3.1.1; §6.3.1.1 with q = 0).  Host only."""
    for v in (rnti, n_id, q):
        if isinstance(v, bool) or int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
            raise ValueError("rnti, n_id and q must be integers")
    out = ctypes.c_uint32()
    _lib.check(_lib.lib().nldpc_gold_cinit(int(rnti), int(q), int(n_id), ctypes.byref(out)), "nldpc_gold_cinit")
    return int(out.value)


def gold(c_init: int, n: int, n0: int = 0) -> np.ndarray:
    """uint8 [n]: c(n0) .. c(n0 + n - 1) of the sequence started from c_init (< 2^31).  Host only."""
    if isinstance(c_init, bool) or int(c_init) != c_init or not 0 <= int(c_init) < 2 ** 31:
        raise ValueError(f"c_init must be an integer in [0, 2^31), got {c_init!r}")
    n, n0 = int(n), int(n0)
    if n < 1 or n0 < 0 or n0 + n > 2 ** 31:
        raise ValueError("n >= 1, n0 >= 0 and n0 + n <= 2^31 must hold")
    out = np.zeros(n, dtype=np.uint8)
    _lib.check(_lib.lib().nldpc_gold_ref(int(c_init), n0, n, out.ctypes.data), "nldpc_gold_ref")
    return out


def sequence(c_inits, E: int, *, device=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """int32 [n_seq, ceil(E / 32)]: the first E bits of the sequence of every c_init, packed; the bits beyond E in the
    last word are 0.  c_inits: an int, a sequence of ints (each in [0, 2^31)), or a contiguous int32 [n_seq] tensor on the
    device, of whose entries the low 31 bits are used."""
    E = _length(E)
    if isinstance(c_inits, torch.Tensor):
        if c_inits.dtype != torch.int32 or c_inits.dim() != 1 or c_inits.shape[0] < 1 or not c_inits.is_contiguous():
            raise ValueError("c_inits must be a contiguous int32 [n_seq] tensor")
        dev = _device_of(c_inits, "c_inits")
        ci = c_inits
    else:
        vals = list(c_inits) if hasattr(c_inits, "__iter__") else [c_inits]
        if not vals or any(isinstance(v, bool) or int(v) != v or not 0 <= int(v) < 2 ** 31 for v in vals):
            raise ValueError("c_inits must be integers in [0, 2^31)")
        dev = torch.device(device if device is not None else (out.device if isinstance(out, torch.Tensor) else "cuda"))
        if dev.type != "cuda":
            raise ValueError("sequence runs on the ROCm device (no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        ci = torch.tensor([int(v) for v in vals], dtype=torch.int32).to(dev)
    shape = (int(ci.shape[0]), _words(E))
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=dev)
    elif _device_of(out, "out") != dev or out.dtype != torch.int32 or tuple(out.shape) != shape or \
            not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int32 {list(shape)} tensor on {dev}")
    with torch.cuda.device(dev):  # (the launch goes to the current device)
        _lib.check(_lib.lib().nldpc_gold_sequence(ci.data_ptr(), shape[0], E, out.data_ptr(), _lib.stream_of(dev)),
                   "nldpc_gold_sequence")
    return out


def scramble(f: torch.Tensor | None, seq: torch.Tensor, *, B: int | None = None, E: int | None = None,
             b_offset: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 [B, E]: (f != 0) ^ c as 0 / 1, row b with sequence (b_offset + b) mod n_seq of seq.  f: contiguous uint8
    [B, E] on the device, or None (the all-zero word, with B and E given: the sequences unpacked).  out may be f."""
    if f is not None:
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 2 or f.shape[0] < 1 or \
                f.shape[1] < 1 or not f.is_contiguous():
            raise ValueError("f must be a contiguous uint8 [B, E] tensor")
        fB, fE = int(f.shape[0]), int(f.shape[1])
        if (B is not None and B != fB) or (E is not None and E != fE):
            raise ValueError(f"f is [{fB}, {fE}], not [B, E] = [{B}, {E}]")
        B, E = fB, _length(fE)
    else:
        if B is None or E is None:
            raise ValueError("scramble needs f, or B and E for the all-zero word")
        B, E = int(B), _length(E)
        if B < 1:
            raise ValueError("B must be positive")
    n_seq, b_offset = _table(seq, E), _offset(b_offset)
    dev = _device_of(f if f is not None else seq, "f" if f is not None else "seq")
    _on(dev, seq)
    if out is None:
        out = torch.empty((B, E), dtype=torch.uint8, device=dev)
    elif _device_of(out, "out") != dev or out.dtype != torch.uint8 or tuple(out.shape) != (B, E) or \
            not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 {[B, E]} tensor on {dev}")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_scramble(_lib.ptr(f), seq.data_ptr(), n_seq, B, E, b_offset, out.data_ptr(),
                                             _lib.stream_of(dev)), "nldpc_scramble")
    return out


def descramble(llr: torch.Tensor, seq: torch.Tensor, *, b_offset: int = 0,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [B, E]: llr with the sign bit of element [b, i] XORed with c(i) of sequence (b_offset + b) mod n_seq -- an
    integer operation on the bit pattern, its own inverse bit for bit.  out may be llr."""
    if not isinstance(llr, torch.Tensor) or llr.dtype != torch.float32 or llr.dim() != 2 or llr.shape[0] < 1 or \
            llr.shape[1] < 1 or not llr.is_contiguous():
        raise ValueError("llr must be a contiguous float32 [B, E] tensor")
    B, E = int(llr.shape[0]), _length(llr.shape[1])
    n_seq, b_offset = _table(seq, E), _offset(b_offset)
    dev = _device_of(llr, "llr")
    _on(dev, seq)
    out = _out(out, (B, E), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_descramble_llr(llr.data_ptr(), seq.data_ptr(), n_seq, B, E, b_offset,
                                                   out.data_ptr(), _lib.stream_of(dev)), "nldpc_descramble_llr")
    return out
