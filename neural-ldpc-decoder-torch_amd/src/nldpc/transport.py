"""Transport blocks on the device (3GPP TS 38.212 §5.1, §5.2.2, §5.4.2.1, §5.5): one TB CRC over a payload, segmentation
into C code blocks with their own CRC24B and filler bits, per-block rate matching to the two lengths E_r, concatenation,
and at the receiver the inverses and the TB verdict.

TBPlan              the sizes (nldpc_tb of include/nldpc.h); TBPlan.make / TBPlan.round_down (host, no GPU needed).
lifting_size        Kb and the smallest lifting size Zc for B' bits (host).
split_E             (E_lo, E_hi, C_lo): the first C_lo code blocks are rate matched to E_lo, the others to E_hi (host).
remainder           host: the code-block verdicts and the TB remainder of one TB's C rows (nldpc_tb_crc_ref).
segment             payload (or None: drawn) -> (info [C*Btb, W], tb [Btb, B']): crc.attach for the TB CRC, then
                    nldpc_tb_segment.
concat / deconcat   ragged copies between the per-block rows and g [Btb, G] (nldpc_tb_concat / nldpc_tb_deconcat).
rate_match_blocks   codewords [C*Btb, N*Z] -> g [Btb, G]: two rate_match calls, then concat.
rate_recover_blocks LLRs [Btb, G] -> xa [C*Btb, N, Z]: deconcat, then two rate_recover calls.
check               posteriors or bits -> code-block verdicts, TB verdicts, the reassembled TBs and four counts
                    (nldpc_tb_check).

Layout: a batch of Btb transport blocks is BLOCK-MAJOR: code block r of TB t is row r * Btb + t of info, of the
codewords y, of xa and of the posteriors.  The C_lo blocks with the smaller E_r are then one contiguous range of rows and
the others a second one, so channel.encode, ratematch.rate_match / rate_recover, every decoder and crc.check run
unchanged on at most two contiguous slices.

A TB whose blocks are all zero passes (as every CRC here does), and a TB in which a code block was replaced by another
valid code block passes every code-block CRC and fails only the TB CRC: that is what the TB CRC is for.
"""
from __future__ import annotations

import collections
import ctypes
import dataclasses

import numpy as np
import torch

from . import _lib
from .crc import CRCS, _count, _crc, _device_of, _rows, attach
from .ratematch import RateMatch, rate_match, rate_recover

TBCheck = collections.namedtuple("TBCheck", "cb_ok tb_ok counts tb_out")


def _width(W, graph) -> int:
    if graph is not None:
        if W is not None and int(W) != graph.K * graph.Z:
            raise ValueError(f"W = {W} is not the graph's K*Z = {graph.K * graph.Z}")
        return graph.K * graph.Z
    if W is None:
        raise ValueError("a plan needs W, or graph for W = K*Z")
    return _count(W, "W")


@dataclasses.dataclass(frozen=True)
class TBPlan:
    """A payload bits + the TB CRC `tb_crc` (a name of crc.CRCS) = B' bits, cut into C parts of Kp - L bits; a code block
    is a part, its CRC24B of L bits (24, or 0 when C == 1) and F filler zeros: a row of W bits."""
    A: int
    tb_crc: str
    W: int
    C: int
    L: int
    Kp: int
    F: int

    @property
    def Bp(self) -> int:
        """B' = A + L_tb = C * part"""
        return self.A + CRCS[self.tb_crc][1]

    @property
    def part(self) -> int:
        """the TB bits a code block carries, K' - L"""
        return self.Kp - self.L

    @classmethod
    def make(cls, A: int, *, W: int | None = None, graph=None, tb_crc: str | None = None, kcb: int = 0) -> "TBPlan":
        """§5.2.2 for rows of W bits (or graph: W = K*Z) and a largest code block of kcb bits (0: W; 5G: 8448 for BG1,
        3840 for BG2).  tb_crc: default "24A" for A > 3824, else "16" (§5.1).  ValueError when the sizes do not fit:
        C must divide B' + C L (round_down finds a payload that does)."""
        A = _count(A, "A")
        W, kcb = _width(W, graph), _count(kcb, "kcb", 0)
        name = ("24A" if A > 3824 else "16") if tb_crc is None else tb_crc
        cid, _ = _crc(name)
        c = _lib.NldpcTb()
        _lib.check(_lib.lib().nldpc_tb_plan(A, cid, W, kcb, ctypes.byref(c)), "nldpc_tb_plan")
        return cls(A=int(c.A), tb_crc=name, W=int(c.W), C=int(c.C), L=int(c.L), Kp=int(c.Kp), F=int(c.F))

    @classmethod
    def round_down(cls, A: int, **kw) -> "TBPlan":
        """The plan of the largest payload <= A that make accepts with the same arguments."""
        A = _count(A, "A")
        _width(kw.get("W"), kw.get("graph"))  # (what no smaller payload cures is raised as it is)
        _count(kw.get("kcb", 0), "kcb", 0)
        if kw.get("tb_crc") is not None:
            _crc(kw["tb_crc"])
        for a in range(A, 0, -1):
            try:
                return cls.make(a, **kw)
            except ValueError:
                pass
        raise ValueError(f"no payload of at most {A} bits fits")

    def _c(self) -> _lib.NldpcTb:
        cid, _ = _crc(self.tb_crc)
        vals = (self.A, self.W, self.C, self.L, self.Kp, self.F)
        if any(isinstance(v, bool) or int(v) != v or not 0 <= v < 2 ** 31 for v in vals):
            raise ValueError(f"the sizes of a plan are integers in [0, 2^31): {self}")
        return _lib.NldpcTb(A=int(self.A), tb_crc=cid, W=int(self.W), C=int(self.C), L=int(self.L), Kp=int(self.Kp),
                            F=int(self.F))


def lifting_size(bg: int, Bp: int) -> tuple[int, int]:
    """(Kb, Zc) of §5.2.2 for a TB of Bp = B' bits with its CRC on base graph bg (1 or 2).  A helper: the plan takes
    whatever graph the caller has."""
    kb, zc = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.lib().nldpc_tb_lifting_size(_count(bg, "bg"), _count(Bp, "Bp"), ctypes.byref(kb), ctypes.byref(zc)),
               "nldpc_tb_lifting_size")
    return int(kb.value), int(zc.value)


def split_E(plan: TBPlan, G: int, qm: int, n_layers: int = 1) -> tuple[int, int, int]:
    """(E_lo, E_hi, C_lo) of §5.4.2.1 for G sent bits per TB: code blocks r < C_lo get E_lo, the others E_hi."""
    lo, hi, clo = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    _lib.check(_lib.lib().nldpc_tb_er(_count(G, "G"), _count(n_layers, "n_layers"), _count(qm, "qm"), plan.C,
                                      ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(clo)), "nldpc_tb_er")
    return int(lo.value), int(hi.value), int(clo.value)


def remainder(plan: TBPlan, blocks) -> tuple[np.ndarray, int]:
    """Host only.  blocks: [C, n >= K'] array (any non-zero value is 1), the code blocks of one TB.  Returns (cb_ok
    bool [C], crc.parity(the reassembled B' bits, plan.tb_crc); 0 = the TB passes), the TB remainder combined from the
    per-part remainders as the device does."""
    arr = np.asarray(blocks)
    if arr.ndim != 2 or arr.shape[0] != plan.C or arr.shape[1] < plan.Kp:
        raise ValueError(f"blocks must be a [C, >= K'] = [{plan.C}, >= {plan.Kp}] array")
    rows = np.ascontiguousarray(arr != 0).astype(np.uint8)
    ok = np.zeros(plan.C, dtype=np.uint8)
    rem = ctypes.c_uint32(0)
    c = plan._c()
    _lib.check(_lib.lib().nldpc_tb_crc_ref(ctypes.byref(c), rows.ctypes.data, rows.shape[1], ok.ctypes.data,
                                           ctypes.byref(rem)), "nldpc_tb_crc_ref")
    return ok.astype(bool), int(rem.value)


def _out(out, shape, dtype, dev, what: str) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if _device_of(out, what) != dev or out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {str(dtype).replace('torch.', '')} {list(shape)} tensor on {dev}")
    return out


def segment(plan: TBPlan, payload: torch.Tensor | None = None, *, Btb: int | None = None, seed: int = 2042,
            b_offset: int = 0, device=None, out: torch.Tensor | None = None):
    """(info uint8 [C*Btb, W], tb uint8 [Btb, B']).  tb = crc.attach(payload, plan.tb_crc, W=B'): the payload (uint8
    [Btb, A], any non-zero byte is 1; or None with Btb: drawn on the device, shard-invariant in b_offset counted in TBs)
    and its TB CRC.  info is block-major: row r * Btb + t holds part r of TB t, its CRC24B and F zeros; with W = K*Z it
    is channel.encode's info."""
    c = plan._c()
    tb = attach(payload, plan.tb_crc, W=plan.Bp, B=Btb, A=plan.A, seed=seed, b_offset=b_offset, device=device)
    dev, B = tb.device, int(tb.shape[0])
    if plan.C * B >= 2 ** 31:
        raise ValueError("C * Btb must be below 2^31")
    info = _out(out, (plan.C * B, plan.W), torch.uint8, dev, "out")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_tb_segment(ctypes.byref(c), tb.data_ptr(), B, info.data_ptr(), _lib.stream_of(dev)),
                   "nldpc_tb_segment")
    return info, tb


def _group(t, Btb: int, what: str):
    """(device, dtype, blocks, E) of a contiguous [blocks * Btb, E] tensor of uint8 or float32"""
    dev = _device_of(t, what)
    if t.dtype not in (torch.uint8, torch.float32) or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or \
            t.shape[0] % Btb != 0 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous uint8 or float32 [blocks * Btb, E] tensor")
    return dev, t.dtype, int(t.shape[0]) // Btb, int(t.shape[1])


def concat(f_lo: torch.Tensor | None, f_hi: torch.Tensor | None, Btb: int, *,
           out: torch.Tensor | None = None) -> torch.Tensor:
    """g [Btb, G] from the block-major rows f_lo [C_lo * Btb, E_lo] and f_hi [(C - C_lo) * Btb, E_hi] (one of them may
    be None), both uint8 or both float32: block r of TB t at g[t, sum_{j<r} E_j ...] (§5.5)."""
    Btb = _count(Btb, "Btb")
    if f_lo is None and f_hi is None:
        raise ValueError("concat needs f_lo, f_hi or both")
    lo = _group(f_lo, Btb, "f_lo") if f_lo is not None else None
    hi = _group(f_hi, Btb, "f_hi") if f_hi is not None else None
    if lo is not None and hi is not None and lo[:2] != hi[:2]:
        raise ValueError("f_lo and f_hi must have one device and dtype")
    dev, dtype = (lo or hi)[:2]
    C_lo, E_lo = (lo[2], lo[3]) if lo else (0, 1)
    C_hi, E_hi = (hi[2], hi[3]) if hi else (0, 1)
    G = C_lo * E_lo + C_hi * E_hi
    if G >= 2 ** 31 or (C_lo + C_hi) * Btb >= 2 ** 31:
        raise ValueError("G and C * Btb must be below 2^31")
    g = _out(out, (Btb, G), dtype, dev, "out")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_tb_concat(g.element_size(), _lib.ptr(f_lo), _lib.ptr(f_hi), Btb, C_lo + C_hi, C_lo,
                                              E_lo, E_hi, g.data_ptr(), _lib.stream_of(dev)), "nldpc_tb_concat")
    return g


def deconcat(g: torch.Tensor, C: int, C_lo: int, E_lo: int, E_hi: int, *, out=None):
    """The inverse of concat: g [Btb, G], uint8 or float32 -> (f_lo [C_lo * Btb, E_lo], f_hi [(C - C_lo) * Btb, E_hi]);
    an empty group is None.  out: a pair of tensors to fill (None for an empty group)."""
    dev = _device_of(g, "g")
    C, C_lo, E_lo, E_hi = _count(C, "C"), _count(C_lo, "C_lo", 0), _count(E_lo, "E_lo"), _count(E_hi, "E_hi")
    if C_lo > C:
        raise ValueError(f"C_lo = {C_lo} exceeds C = {C}")
    G = C_lo * E_lo + (C - C_lo) * E_hi
    if g.dtype not in (torch.uint8, torch.float32) or g.dim() != 2 or g.shape[0] < 1 or g.shape[1] != G or \
            not g.is_contiguous():
        raise ValueError(f"g must be a contiguous uint8 or float32 [Btb, G] = [Btb, {G}] tensor")
    Btb = int(g.shape[0])
    if G >= 2 ** 31 or C * Btb >= 2 ** 31:
        raise ValueError("G and C * Btb must be below 2^31")
    o_lo, o_hi = (None, None) if out is None else out
    f_lo = _out(o_lo, (C_lo * Btb, E_lo), g.dtype, dev, "out[0]") if C_lo else None
    f_hi = _out(o_hi, ((C - C_lo) * Btb, E_hi), g.dtype, dev, "out[1]") if C_lo < C else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nldpc_tb_deconcat(g.element_size(), g.data_ptr(), Btb, C, C_lo, E_lo, E_hi, _lib.ptr(f_lo),
                                                _lib.ptr(f_hi), _lib.stream_of(dev)), "nldpc_tb_deconcat")
    return f_lo, f_hi


def _rms(graph, plan: TBPlan, G: int, qm: int, n_layers: int, bg: int, rv: int, ncb: int):
    if plan.W != graph.K * graph.Z:
        raise ValueError(f"the plan's W = {plan.W} is not the graph's K*Z = {graph.K * graph.Z}")
    E_lo, E_hi, C_lo = split_E(plan, G, qm, n_layers)
    rms = [RateMatch.nr5g(graph, E, bg=bg, rv=rv, n_filler=plan.F, ncb=ncb, qm=qm) for E in (E_lo, E_hi)]
    return rms, C_lo


def rate_match_blocks(graph, plan: TBPlan, y: torch.Tensor, G: int, *, qm: int, rv: int = 0, bg: int = 2,
                      n_layers: int = 1, ncb: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """g uint8 [Btb, G]: the codewords y [C*Btb, N*Z] (block-major) rate matched per block to E_r (RateMatch.nr5g with
    n_filler = plan.F, the same rv for every block) and concatenated: the bits of one TB in sending order."""
    dev = _device_of(y, "y")
    (rm_lo, rm_hi), C_lo = _rms(graph, plan, G, qm, n_layers, bg, rv, ncb)
    if y.dim() != 2 or y.shape[0] < plan.C or y.shape[0] % plan.C != 0:
        raise ValueError(f"y must be a [C*Btb, N*Z] tensor with C = {plan.C}")
    Btb = int(y.shape[0]) // plan.C
    out = _out(out, (Btb, G), torch.uint8, dev, "out")
    f_lo = rate_match(graph, rm_lo, y[:C_lo * Btb])
    f_hi = rate_match(graph, rm_hi, y[C_lo * Btb:]) if C_lo < plan.C else None
    return concat(f_lo, f_hi, Btb, out=out)


def rate_recover_blocks(graph, plan: TBPlan, llr: torch.Tensor, G: int, *, qm: int, rv: int = 0, bg: int = 2,
                        n_layers: int = 1, ncb: int = 0, out: torch.Tensor | None = None, accumulate: bool = False,
                        erasure_value: float = 0.0, filler_value: float = -20.0, clip: float = 0.0) -> torch.Tensor:
    """xa fp32 [C*Btb, N, Z] (block-major), the decoders' input, from the received LLRs llr fp32 [Btb, G] in the order of
    rate_match_blocks' output.  The other arguments are ratematch.rate_recover's (accumulate=True adds a further
    redundancy version to `out`)."""
    dev = _device_of(llr, "llr")
    (rm_lo, rm_hi), C_lo = _rms(graph, plan, G, qm, n_layers, bg, rv, ncb)
    if llr.dtype != torch.float32 or llr.dim() != 2 or llr.shape[0] < 1 or llr.shape[1] != G or not llr.is_contiguous():
        raise ValueError(f"llr must be a contiguous float32 [Btb, G] = [Btb, {G}] tensor")
    Btb = int(llr.shape[0])
    if out is None and accumulate:
        raise ValueError("accumulate=True adds to `out`: pass the tensor an earlier rate_recover_blocks filled")
    out = _out(out, (plan.C * Btb, graph.N, graph.Z), torch.float32, dev, "out")
    l_lo, l_hi = deconcat(llr, plan.C, C_lo, rm_lo.E, rm_hi.E)
    kw = dict(accumulate=accumulate, erasure_value=erasure_value, filler_value=filler_value, clip=clip)
    rate_recover(graph, rm_lo, l_lo, out=out[:C_lo * Btb], **kw)
    if l_hi is not None:
        rate_recover(graph, rm_hi, l_hi, out=out[C_lo * Btb:], **kw)
    return out


def check(plan: TBPlan, x, *, ref_tb: torch.Tensor | None = None, counts=None, tb_out=False, convention: int = 0,
          cb_ok=True, tb_ok=True) -> TBCheck:
    """The verdicts of a batch of transport blocks from the first K' positions of its C*Btb rows x (block-major): one
    contiguous [C*Btb, L] or [C*Btb, N, Z] tensor on the device -- float32 LLRs (hard decision LLR > 0, or LLR < 0 with
    convention=1) or uint8 bits -- or a list of T of them (a decoder's posteriors go in as they are).  Returns
    TBCheck(cb_ok, tb_ok, counts, tb_out), None for what was not asked for; a list adds a leading dimension T:
      cb_ok   uint8 [C*Btb]: the code block's CRC24B passes (C == 1: the TB verdict); True, or a tensor to fill
      tb_ok   uint8 [Btb]: the TB CRC over the reassembled B' bits passes; True, or a tensor to fill
      counts  int64 [4], with counts=True or a tensor to add to: TBs whose CRC fails, TBs that pass although their B'
              bits differ from ref_tb (undetected), TBs that differ from ref_tb, code blocks whose CRC fails; the middle
              two stay 0 without ref_tb (uint8 [Btb, B'], segment's tb)
      tb_out  uint8 [Btb, B'], with tb_out=True or a tensor to fill: the reassembled hard decisions (desegmentation)"""
    c = plan._c()
    if convention not in (0, 1):
        raise ValueError(f"convention must be 0 or 1, got {convention!r}")
    single = isinstance(x, torch.Tensor)
    xs = [x] if single else list(x)
    if not xs:
        raise ValueError("x must be a tensor or a non-empty list of tensors")
    dev, rows, stride = _rows(xs[0], "x", (torch.float32, torch.uint8))
    for t in xs[1:]:
        if _rows(t, "x", (torch.float32, torch.uint8)) != (dev, rows, stride) or t.dtype != xs[0].dtype:
            raise ValueError("every tensor of x must have the first one's device, dtype and shape")
    if rows % plan.C != 0 or stride < plan.Kp or rows >= 2 ** 31:
        raise ValueError(f"x must have C*Btb rows (C = {plan.C}) of at least K' = {plan.Kp} elements, got [{rows}, {stride}]")
    Btb, T, Bp = rows // plan.C, len(xs), plan.Bp
    if ref_tb is not None:
        if _device_of(ref_tb, "ref_tb") != dev or ref_tb.dtype != torch.uint8 or tuple(ref_tb.shape) != (Btb, Bp) or \
                not ref_tb.is_contiguous():
            raise ValueError(f"ref_tb must be a contiguous uint8 [{Btb}, {Bp}] tensor on {dev}")

    def want(arg, shape, dtype, what, zero=False):
        shape = tuple(shape) if single else (T,) + tuple(shape)
        if isinstance(arg, torch.Tensor):
            return _out(arg, shape, dtype, dev, what)
        if not arg:
            return None
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=dev)

    cb_t = want(cb_ok, (rows,), torch.uint8, "cb_ok")
    tb_t = want(tb_ok, (Btb,), torch.uint8, "tb_ok")
    out_t = want(tb_out, (Btb, Bp), torch.uint8, "tb_out")
    cnt = want(counts, (4,), torch.int64, "counts", zero=True)
    if cb_t is None and tb_t is None and out_t is None and cnt is None:
        raise ValueError("check computes cb_ok, tb_ok, tb_out, counts or some of them")
    need = ctypes.c_size_t(0)
    _lib.check(_lib.lib().nldpc_tb_workspace(ctypes.byref(c), Btb, ctypes.byref(need)), "nldpc_tb_workspace")
    is_llr = xs[0].dtype == torch.float32

    def at(t, i):
        return None if t is None else (t if single else t[i]).data_ptr()

    with torch.cuda.device(dev):
        work = torch.empty((max(need.value // 4, 1),), dtype=torch.int32, device=dev)
        s = _lib.stream_of(dev)
        for i, xt in enumerate(xs):
            _lib.check(_lib.lib().nldpc_tb_check(ctypes.byref(c), xt.data_ptr() if is_llr else None,
                                                 None if is_llr else xt.data_ptr(), Btb, stride, int(convention),
                                                 _lib.ptr(ref_tb), at(cb_t, i), at(tb_t, i), at(out_t, i), at(cnt, i),
                                                 work.data_ptr(), work.numel() * 4, s), "nldpc_tb_check")
    return TBCheck(cb_t, tb_t, cnt, out_t)
