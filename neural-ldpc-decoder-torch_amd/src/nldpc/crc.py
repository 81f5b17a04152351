"""CRC attachment and checking on the device (3GPP TS 38.212 §5.1: CRC24A, 24B, 24C, 16, 11, 6), the step in front of
channel.encode and behind the decoder.

CRCS           name -> (id, L, polynomial without its leading term).
parity         host: the L parity bits of a bit array as an integer (nldpc_crc_ref; no GPU needed).
payload_len    the payload bits A that fit a graph's K*Z info bits beside the CRC and n_filler filler bits.
attach         payload [B, A] (or None: drawn on the device from the encoder's info-bit stream) -> info [B, W] =
               payload | parity | zeros (nldpc_crc_attach): with W = K*Z what channel.encode takes, and
               RateMatch.n_filler = W - A - L.
check          posteriors or bits -> ok [B] and, beside it, counts (CRC failures, undetected errors, block errors)
               against the true bits (nldpc_crc_check).  No transmitted word is needed for ok.
first_pass     of T posteriors, per block the first whose CRC passes (a genie-free stopping rule by composition).

The register starts at zero, nothing is reflected, there is no final XOR: leading zero bits change nothing and the
all-zero block passes.  A CRC pass is not syndrome weight 0 (channel.syndrome_weight): a wrong codeword has syndrome 0
and fails its CRC, but for a chance of 2^-L.  The definitions are in include/nldpc.h.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

CRCS = {"24A": (0, 24, 0x864CFB), "24B": (1, 24, 0x800063), "24C": (2, 24, 0xB2B117), "16": (3, 16, 0x1021),
        "11": (4, 11, 0x621), "6": (5, 6, 0x21)}


def _crc(crc):
    """(id, L) of a name of CRCS"""
    if not isinstance(crc, str) or crc not in CRCS:
        raise ValueError(f"crc must be one of {sorted(CRCS)}, got {crc!r}")
    return CRCS[crc][0], CRCS[crc][1]


def _device_of(t, what: str) -> torch.device:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{what} must be a tensor on the ROCm device (no CPU path)")
    return t.device


def _count(v, what: str, lo: int = 1) -> int:
    try:
        n = None if isinstance(v, bool) else int(v)
    except (TypeError, ValueError, OverflowError):  # (a str, None, inf, nan)
        n = None
    if n is None or n != v or n < lo:
        raise ValueError(f"{what} must be an integer >= {lo}, got {v!r}")
    return n


def parity(bits, crc: str, *, chunk: int | None = None):
    """The parity of `bits` (a 1-D array, any non-zero value is 1) as an integer whose bit L-1 is p_0; a 2-D array gives
    a uint32 array, one value per row.  Host only.  chunk: the piece length of nldpc_crc_ref (every value gives the same
    parity; None = 2048, the kernels' step)."""
    cid, _ = _crc(crc)
    arr = np.asarray(bits)
    if arr.ndim not in (1, 2) or arr.shape[-1] < 1:
        raise ValueError("bits must be a non-empty 1-D or 2-D array")
    chunk = 2048 if chunk is None else _count(chunk, "chunk")
    rows = np.ascontiguousarray(np.atleast_2d(arr) != 0).astype(np.uint8)
    out = np.zeros(rows.shape[0], dtype=np.uint32)
    p = ctypes.c_uint32(0)
    for b in range(rows.shape[0]):
        _lib.check(_lib.lib().nldpc_crc_ref(cid, rows[b].ctypes.data, rows.shape[1], chunk, ctypes.byref(p)),
                   "nldpc_crc_ref")
        out[b] = p.value
    return int(out[0]) if arr.ndim == 1 else out


def payload_len(graph, crc: str, n_filler: int = 0) -> int:
    """A = K*Z - n_filler - L: the payload bits of one code block of `graph`."""
    _, L = _crc(crc)
    A = graph.K * graph.Z - _count(n_filler, "n_filler", 0) - L
    if A < 1:
        raise ValueError(f"no payload bit is left: K*Z = {graph.K * graph.Z}, n_filler = {n_filler}, L = {L}")
    return A


def attach(payload: torch.Tensor | None, crc: str, *, W: int | None = None, graph=None, B: int | None = None,
           A: int | None = None, seed: int = 2042, b_offset: int = 0, device=None,
           out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 [B, W] info blocks payload | parity | zeros.  payload: contiguous uint8 [B, A] on the device (any non-zero
    byte is 1), or None with B and A given: the payloads are drawn on the device and equal the first A info bits of
    channel.encode(graph, B=B, seed=seed, b_offset=b_offset) for a graph with K*Z = W.  W, or graph for W = K*Z;
    default A + L."""
    cid, L = _crc(crc)
    if payload is not None:
        dev = _device_of(payload, "payload")
        if payload.dtype != torch.uint8 or payload.dim() != 2 or payload.shape[0] < 1 or payload.shape[1] < 1 or \
                not payload.is_contiguous():
            raise ValueError("payload must be a contiguous uint8 [B, A] tensor")
        pB, pA = int(payload.shape[0]), int(payload.shape[1])
        if (B is not None and B != pB) or (A is not None and A != pA):
            raise ValueError(f"payload is [{pB}, {pA}], not [B, A] = [{B}, {A}]")
        B, A = pB, pA
    else:
        if B is None or A is None:
            raise ValueError("attach needs payload, or B and A for drawn payloads")
        B, A = _count(B, "B"), _count(A, "A")
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise ValueError("attach runs on the ROCm device (no CPU path)")
    if W is not None and graph is not None and int(W) != graph.K * graph.Z:
        raise ValueError(f"W = {W} is not the graph's K*Z = {graph.K * graph.Z}")
    W = graph.K * graph.Z if graph is not None else A + L if W is None else _count(W, "W")
    if A + L > W or W >= 2 ** 31:
        raise ValueError(f"A + L = {A + L} must not exceed W = {W}, and W must be below 2^31")
    b_offset = _count(b_offset, "b_offset", 0)
    if dev.index is None:  # (only now: every argument error above is raised without touching a device)
        dev = torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty((B, W), dtype=torch.uint8, device=dev)
    elif _device_of(out, "out") != dev or out.dtype != torch.uint8 or tuple(out.shape) != (B, W) or \
            not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 [{B}, {W}] tensor on {dev}")
    with torch.cuda.device(dev):  # (the launch goes to the current device)
        _lib.check(_lib.lib().nldpc_crc_attach(cid, _lib.ptr(payload), B, A, W, int(seed) & (2 ** 64 - 1), b_offset,
                                               out.data_ptr(), _lib.stream_of(dev)), "nldpc_crc_attach")
    return out


def _rows(t, what: str, dtypes):
    """(device, B, elements per row) of a contiguous [B, L] or [B, N, Z] tensor"""
    dev = _device_of(t, what)
    if t.dtype not in dtypes or t.dim() not in (2, 3) or t.shape[0] < 1 or t.numel() < 1 or not t.is_contiguous():
        names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{what} must be a contiguous {names} [B, L] or [B, N, Z] tensor")
    return dev, int(t.shape[0]), t.numel() // int(t.shape[0])


def check(x, crc: str, A: int, *, ref: torch.Tensor | None = None, convention: int = 0, counts=None, ok=True):
    """The CRC verdict of the first A + L positions of every row of x: one contiguous [B, L] or [B, N, Z] tensor on the
    device -- float32 LLRs (hard decision LLR > 0, or LLR < 0 with convention=1; an exact zero or a NaN is bit 0) or
    uint8 bits (non-zero is 1); a decoder posterior goes in as it is, its row length is its stride -- or a list of T of
    them.  Returns ok: uint8 [B] (a list: [T, B]), 1 = the block passes.

    counts: True (or an int64 [3] tensor, a list: [T, 3], to add to) also returns, as (ok, counts), the number of blocks
    whose CRC fails, of blocks whose CRC passes although their A + L bits differ from ref (undetected errors) and of
    blocks whose bits differ from ref; the last two stay 0 without ref.  ref: contiguous uint8 [B, L'] (or [B, N, Z])
    true bits, e.g. channel.encode's codewords.  ok: True, or a uint8 [B] ([T, B]) tensor to fill; None / False with
    counts: only counts is computed and returned."""
    cid, L = _crc(crc)
    A = _count(A, "A")
    if convention not in (0, 1):
        raise ValueError(f"convention must be 0 or 1, got {convention!r}")
    single = isinstance(x, torch.Tensor)
    xs = [x] if single else list(x)
    if not xs:
        raise ValueError("x must be a tensor or a non-empty list of tensors")
    dev, B, stride = _rows(xs[0], "x", (torch.float32, torch.uint8))
    for t in xs[1:]:
        if _rows(t, "x", (torch.float32, torch.uint8)) != (dev, B, stride) or t.dtype != xs[0].dtype:
            raise ValueError("every tensor of x must have the first one's device, dtype and shape")
    if stride < A + L or A + L >= 2 ** 31:
        raise ValueError(f"a row of x has {stride} elements, fewer than A + L = {A + L} (or A + L is not below 2^31)")
    ref_stride = 0
    if ref is not None:
        rdev, rB, ref_stride = _rows(ref, "ref", (torch.uint8,))
        if rdev != dev or rB != B or ref_stride < A + L:
            raise ValueError(f"ref must hold at least A + L = {A + L} bits for each of the {B} rows, on {dev}")
    T = len(xs)
    if isinstance(ok, torch.Tensor):
        ok_t = ok
        if _device_of(ok_t, "ok") != dev or ok_t.dtype != torch.uint8 or not ok_t.is_contiguous() or \
                tuple(ok_t.shape) != ((B,) if single else (T, B)):
            raise ValueError(f"ok must be a contiguous uint8 {[B] if single else [T, B]} tensor on {dev}")
    else:
        ok_t = torch.empty((T, B), dtype=torch.uint8, device=dev) if ok else None
    if isinstance(counts, torch.Tensor):
        cnt = counts
        if _device_of(cnt, "counts") != dev or cnt.dtype != torch.int64 or not cnt.is_contiguous() or \
                tuple(cnt.shape) != ((3,) if single else (T, 3)):
            raise ValueError(f"counts must be a contiguous int64 {[3] if single else [T, 3]} tensor on {dev}")
    else:
        cnt = torch.zeros((T, 3), dtype=torch.int64, device=dev) if counts else None
    if ok_t is None and cnt is None:
        raise ValueError("check computes ok, counts or both")
    ok2 = None if ok_t is None else ok_t.view(T, B)
    cnt2 = None if cnt is None else cnt.view(T, 3)
    is_llr = xs[0].dtype == torch.float32
    with torch.cuda.device(dev):
        s = _lib.stream_of(dev)
        for t, xt in enumerate(xs):
            _lib.check(_lib.lib().nldpc_crc_check(cid, xt.data_ptr() if is_llr else None, None if is_llr else xt.data_ptr(),
                                                  B, A, stride, int(convention), _lib.ptr(ref), ref_stride,
                                                  None if ok2 is None else ok2[t].data_ptr(),
                                                  None if cnt2 is None else cnt2[t].data_ptr(), s), "nldpc_crc_check")
    if single:  # (a tensor the caller passed is returned as it is)
        ok_t = ok_t if ok_t is None or ok_t.dim() == 1 else ok_t[0]
        cnt = cnt if cnt is None or cnt.dim() == 1 else cnt[0]
    if cnt is None:
        return ok_t
    return cnt if ok_t is None else (ok_t, cnt)


def first_pass(outs, crc: str, A: int, *, convention: int = 0):
    """Of the T posteriors `outs` (a list of [B, N*Z] / [B, N, Z] tensors, or decode's stacked [T, B, N*Z]) the first per
    block whose CRC passes: with t*(b) the smallest t whose check(outs[t])[b] is 1, or T-1 if there is none, returns
    (out [B, ...] = outs[t*(b)][b]; iters int32 [B] = t*(b) + 1; ok uint8 [B] = the verdict of out[b]).  The selection
    runs on the device; it needs all T posteriors, so it saves no decode time (decode.decode_early_stop stops on the
    syndrome instead, inside the kernel)."""
    outs = list(outs)
    ok = check(outs, crc, A, convention=convention)  # [T, B]
    T, B = int(ok.shape[0]), int(ok.shape[1])
    dev = ok.device
    good = ok != 0
    tstar = torch.where(good.any(0), good.to(torch.int32).argmax(0), torch.full((B,), T - 1, device=dev)).to(torch.int64)
    stack = torch.stack(outs).view(T, B, -1)
    out = stack.gather(0, tstar.view(1, B, 1).expand(1, B, stack.shape[2]))[0].view(outs[0].shape)
    return out, (tstar + 1).to(torch.int32), ok.gather(0, tstar.view(1, B))[0]
