"""MIMO spatial multiplexing with LMMSE soft detection for the QAM channel on the device: one codeword over nt layers
(3GPP TS 38.211 §6.3.1.3 / §7.3.1.3, identity precoding), an nr x nt flat block-fading channel and a linear MMSE
detector in front of the unchanged soft demapper.  nt, nr in {1, 2, 4} with nr >= nt; qm = 2, 4, 6, 8.

n_blocks       fading blocks per row: ceil(R / L) over the R = E / (qm nt) resource elements, 1 when L >= R.
channels       the drawn channel table [B, n_blk, nr, nt, 2] (nldpc_mimo_channels): Rayleigh, i.i.d. CN(0, 1/nt).
filter         a channel table -> the LMMSE filter W [B, n_blk, nt, nr, 2], the layer gains mu [B, n_blk, nt] and the
               demapper weights w [B, n_blk, nt] (nldpc_mimo_filter).
detect         received samples [B, R, nr, 2] and a channel table -> LLRs [B, R*nt*qm] (nldpc_mimo_detect).
qam_llr        the fused channel: bits -> (scramble) -> symbols -> H x -> AWGN -> filter -> equalise -> demap ->
               (descramble) in one kernel (nldpc_mimo_channel_llr), with drawn or given channels.
detect_ml      the same inputs -> the exact max-log ML (joint) LLRs (nldpc_mimo_detect_ml): no Gaussian approximation
               of the interference; two sliced passes of 2^(qm (nt - 1)) candidates per RE; nt = 4 up to qm = 4.
qam_llr_ml     qam_llr with that detector (nldpc_mimo_channel_llr_ml): the same samples and channels, max-log only.
sigma_for      Eb/N0 -> noise standard deviation per real dimension and receive antenna.

A resource element (RE) carries nt consecutive symbols of a row, one per layer, so the layer mapping is the identity in
memory: RateMatch(qm=qm) / transport.rate_match_blocks(n_layers=nt) produce the bits in this order and
ratematch.rate_recover takes the LLRs back.  H is constant over L consecutive REs of a row (the last block of a row may
be short, blocks never span rows).  Noise and channels come from Philox-4x32-10 at the global RE / block index, so a
batch sharded over ranks draws those of the unsharded batch.  The LLRs are those of a biased-LMMSE receiver under the
Gaussian approximation of the residual interference.  The definitions are in include/nldpc.h.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .fading import _device, _length, _offset
from .modulation import _bits, _device_of, _method, _order, _out, _sigma

DIMS = ((1, 1), (1, 2), (1, 4), (2, 2), (2, 4), (4, 4))


def _dims(nt, nr):
    for v in (nt, nr):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"nt and nr must be integers, got {nt!r}, {nr!r}")
    if (int(nt), int(nr)) not in DIMS:
        raise ValueError(f"(nt, nr) must be one of {DIMS}, got ({nt!r}, {nr!r})")
    return int(nt), int(nr)


def _table(h, shape, dev: torch.device, what="h") -> torch.Tensor:
    if _device_of(h, what) != dev or h.dtype != torch.float32 or tuple(h.shape) != tuple(shape) or \
            not h.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 {list(shape)} tensor on {dev}")
    return h


def sigma_for(ebn0_db: float, code_rate: float, qm: int, nt: int) -> float:
    """Noise standard deviation per real dimension and receive antenna.  Convention: the nt layers together put unit
    energy per RE on each receive antenna (E|h|^2 = 1/nt, unit symbol energy per layer) and carry qm * nt coded bits,
    so Es/N0 per receive antenna = qm * nt * R * Eb/N0 with N0 = 2 sigma^2: modulation.sigma_for with qm * nt bits per
    unit of received energy.  The array gain of nr antennas is not counted into Eb."""
    return math.sqrt(1.0 / (2.0 * qm * nt * code_rate * 10.0 ** (ebn0_db / 10.0)))


def n_blocks(R: int, L: int = 1) -> int:
    """fading blocks per row of R resource elements with coherence length L: ceil(R / L)"""
    R, L = int(R), _length(L)
    if R < 1:
        raise ValueError("R must be positive")
    return 1 if L >= R else -(-R // L)


def channels(B: int, R: int, *, nt: int, nr: int, L: int = 1, seed: int = 2042, b_offset: int = 0, device=None,
             out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [B, n_blocks(R, L), nr, nt, 2] (re, im): the channels qam_llr draws for rows b_offset .. b_offset + B - 1 of
    the stream of `seed`; h[..., r, t, :] is the path from layer t to antenna r."""
    (nt, nr), B, n_blk, b_offset = _dims(nt, nr), int(B), n_blocks(R, L), _offset(b_offset)
    if B < 1 or B * n_blk >= 2 ** 31:
        raise ValueError("B must be positive and B * n_blocks(R, L) below 2^31")
    dev = _device(device, out)
    out = _out(out, (B, n_blk, nr, nt, 2), dev)
    with torch.cuda.device(dev):  # (the launch goes to the current device)
        _lib.check(_lib.lib().nldpc_mimo_channels(nt, nr, int(seed) & (2 ** 64 - 1), B, n_blk, b_offset, out.data_ptr(),
                                                  _lib.stream_of(dev)), "nldpc_mimo_channels")
    return out


def filter(h: torch.Tensor, sigma: float):  # noqa: A001  (the name the stage has in the ABI)
    """(W, mu, w) of the channel table h (contiguous fp32 [B, n_blk, nr, nt, 2] on the device): the LMMSE filter
    W = (H^H H + 2 sigma^2 I)^-1 H^H as fp32 [B, n_blk, nt, nr, 2], the layer gains mu = diag(W H) [B, n_blk, nt] and the
    demapper weights w = 1 / (mu (1 - mu)) [B, n_blk, nt] (0 where mu (1 - mu) is not positive and finite)."""
    sigma = _sigma(sigma)
    dev = _device_of(h, "h")
    if h.dtype != torch.float32 or h.dim() != 5 or h.shape[4] != 2 or h.shape[0] < 1 or h.shape[1] < 1 or \
            not h.is_contiguous():
        raise ValueError("h must be a contiguous float32 [B, n_blk, nr, nt, 2] tensor")
    B, n_blk = int(h.shape[0]), int(h.shape[1])
    nt, nr = _dims(int(h.shape[3]), int(h.shape[2]))
    if B * n_blk >= 2 ** 31:
        raise ValueError("B * n_blk must be below 2^31")
    W = torch.empty((B, n_blk, nt, nr, 2), dtype=torch.float32, device=dev)
    mu = torch.empty((B, n_blk, nt), dtype=torch.float32, device=dev)
    w = torch.empty((B, n_blk, nt), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_mimo_filter(nt, nr, sigma, h.data_ptr(), B, n_blk, W.data_ptr(), mu.data_ptr(),
                                                w.data_ptr(), _lib.stream_of(dev)), "nldpc_mimo_filter")
    return W, mu, w


def _samples(y, h):
    """(B, R, nt, nr, device) of the received samples y [B, R, nr, 2] and a channel table h [., ., nr, nt, 2]"""
    dev = _device_of(y, "y")
    if y.dtype != torch.float32 or y.dim() != 4 or y.shape[3] != 2 or y.shape[0] < 1 or y.shape[1] < 1 or \
            not y.is_contiguous():
        raise ValueError("y must be a contiguous float32 [B, R, nr, 2] tensor")
    B, R, nr = int(y.shape[0]), int(y.shape[1]), int(y.shape[2])
    if not isinstance(h, torch.Tensor) or h.dim() != 5:
        raise ValueError("h must be a contiguous float32 [B, n_blk, nr, nt, 2] tensor")
    nt, nr = _dims(int(h.shape[3]), nr)
    return B, R, nt, nr, dev


def detect(y: torch.Tensor, qm: int, sigma: float, h: torch.Tensor, *, L: int = 1, method: str = "maxlog",
           out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [B, R*nt*qm] LLRs (> 0: bit 1) of the received samples y (contiguous fp32 [B, R, nr, 2] on the device) that
    passed through the channels h (contiguous fp32 [B, n_blocks(R, L), nr, nt, 2]); sigma is the noise standard
    deviation per real dimension and antenna.  method "maxlog" or "logmap"."""
    qm, m, sigma, L = _order(qm), _method(method), _sigma(sigma), _length(L)
    B, R, nt, nr, dev = _samples(y, h)
    n_blk = n_blocks(R, L)
    if R * nt * qm >= 2 ** 31 or B * n_blk >= 2 ** 31:
        raise ValueError("R * nt * qm and B * n_blocks(R, L) must be below 2^31")
    h = _table(h, (B, n_blk, nr, nt, 2), dev)
    out = _out(out, (B, R * nt * qm), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_mimo_detect(qm, m, nt, nr, sigma, y.data_ptr(), h.data_ptr(), B, R, L,
                                                out.data_ptr(), _lib.stream_of(dev)), "nldpc_mimo_detect")
    return out


def detect_ml(y: torch.Tensor, qm: int, sigma: float, h: torch.Tensor, *, L: int = 1,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [B, R*nt*qm] exact max-log ML LLRs (> 0: bit 1) of the received samples y and the channels h, both as
    detect takes them: LLR(b) = (min_{x: b=0} |y - H x|^2 - min_{x: b=1} |y - H x|^2) / (2 sigma^2) over all 2^(qm nt)
    symbol vectors of the resource element.  nt = 4 is detected up to qm = 4 (_lib.NldpcUnsupported beyond)."""
    qm, sigma, L = _order(qm), _sigma(sigma), _length(L)
    B, R, nt, nr, dev = _samples(y, h)
    n_blk = n_blocks(R, L)
    if R * nt * qm >= 2 ** 31 or B * n_blk >= 2 ** 31:
        raise ValueError("R * nt * qm and B * n_blocks(R, L) must be below 2^31")
    h = _table(h, (B, n_blk, nr, nt, 2), dev)
    out = _out(out, (B, R * nt * qm), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_mimo_detect_ml(qm, nt, nr, sigma, y.data_ptr(), h.data_ptr(), B, R, L,
                                                   out.data_ptr(), _lib.stream_of(dev)), "nldpc_mimo_detect_ml")
    return out


def qam_llr(f: torch.Tensor | None, qm: int, sigma: float, *, nt: int, nr: int, L: int = 1,
            h: torch.Tensor | None = None, B: int | None = None, E: int | None = None, seed: int = 2042,
            b_offset: int = 0, method: str = "maxlog", scramble: torch.Tensor | None = None, device=None,
            out: torch.Tensor | None = None, return_symbols: bool | torch.Tensor = False,
            return_channels: bool | torch.Tensor = False):
    """fp32 [B, E] LLRs of the bits f (contiguous uint8 [B, E] on the device, or None: the all-zero word, with B and E
    given) sent as 2^qm-QAM symbols on nt layers through an nr x nt flat block-fading channel of coherence length L (in
    resource elements) and AWGN of standard deviation sigma per real dimension and antenna, LMMSE-equalised and demapped
    in one kernel.  E / qm must be a multiple of nt.  h None: the channels are drawn, those of
    channels(B, E // (qm nt), nt=nt, nr=nr, L=L, seed=seed, b_offset=b_offset); else h is the table, contiguous fp32
    [B, n_blocks(E // (qm nt), L), nr, nt, 2].  scramble: a table of scrambling.sequence, used as modulation.qam_llr
    uses it.  return_symbols / return_channels: True (or a tensor to fill) also returns the received samples
    [B, R, nr, 2] / the channels; the result is then the tuple (llr[, samples][, channels]), and without scramble the
    LLRs are bit for bit detect(samples, qm, sigma, channels, L=L, method=method)."""
    qm, m = _order(qm), _method(method)
    return _fused("nldpc_mimo_channel_llr", (qm, m), f, qm, sigma, nt, nr, L, h, B, E, seed, b_offset, scramble, device,
                  out, return_symbols, return_channels)


def qam_llr_ml(f: torch.Tensor | None, qm: int, sigma: float, *, nt: int, nr: int, L: int = 1,
               h: torch.Tensor | None = None, B: int | None = None, E: int | None = None, seed: int = 2042,
               b_offset: int = 0, scramble: torch.Tensor | None = None, device=None,
               out: torch.Tensor | None = None, return_symbols: bool | torch.Tensor = False,
               return_channels: bool | torch.Tensor = False):
    """qam_llr with the exact max-log ML detector of detect_ml in place of the LMMSE one, in one kernel: the same
    arguments without method, the same noise and channel streams, so the returned samples and channels are bit for bit
    those of qam_llr, and without scramble the LLRs are bit for bit detect_ml(samples, qm, sigma, channels, L=L).
    nt = 4 is detected up to qm = 4 (_lib.NldpcUnsupported beyond)."""
    qm = _order(qm)
    return _fused("nldpc_mimo_channel_llr_ml", (qm,), f, qm, sigma, nt, nr, L, h, B, E, seed, b_offset, scramble, device,
                  out, return_symbols, return_channels)


def _fused(entry, lead, f, qm, sigma, nt, nr, L, h, B, E, seed, b_offset, scramble, device, out, return_symbols,
           return_channels):
    """the argument checks and the call shared by the fused channels; lead = the entry's arguments before nt"""
    sigma, L, (nt, nr) = _sigma(sigma), _length(L), _dims(nt, nr)
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
    if (E // qm) % nt:
        raise ValueError(f"E / qm = {E // qm} symbols must be a multiple of nt = {nt}")
    b_offset = _offset(b_offset)
    R = E // qm // nt
    n_blk = n_blocks(R, L)
    if B * n_blk >= 2 ** 31:
        raise ValueError("B * n_blocks(E // (qm nt), L) must be below 2^31")
    if h is not None:
        h = _table(h, (B, n_blk, nr, nt, 2), dev)
    out = _out(out, (B, E), dev)
    sym = h_out = None
    if isinstance(return_symbols, torch.Tensor):
        sym = _out(return_symbols, (B, R, nr, 2), dev, "return_symbols")
    elif return_symbols:
        sym = torch.empty((B, R, nr, 2), dtype=torch.float32, device=dev)
    if isinstance(return_channels, torch.Tensor):
        h_out = _out(return_channels, (B, n_blk, nr, nt, 2), dev, "return_channels")
        if h is not None and h_out.data_ptr() == h.data_ptr():
            raise ValueError("return_channels must not be the channel table itself")
    elif return_channels:
        h_out = torch.empty((B, n_blk, nr, nt, 2), dtype=torch.float32, device=dev)
    n_seq = 0
    if scramble is not None:
        from .scrambling import _on, _table as _seq_table
        n_seq = _seq_table(scramble, E)
        _on(dev, scramble)
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), entry)(
            *lead, nt, nr, _lib.ptr(f), B, E, sigma, int(seed) & (2 ** 64 - 1), b_offset, L, _lib.ptr(h),
            _lib.ptr(scramble), n_seq, out.data_ptr(), _lib.ptr(sym), _lib.ptr(h_out), _lib.stream_of(dev)), entry)
    extra = tuple(t for t in (sym, h_out) if t is not None)
    return (out,) + extra if extra else out
