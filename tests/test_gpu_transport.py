"""Transport blocks on the GPU (nldpc_tb_segment / concat / deconcat / check, nldpc.transport), bit for bit against
tb_model.py (TS 38.212 restated literally, on crc_model.py's long division), with guard bytes around every output.

Plans (A, TB CRC, kcb = W): C = 1 (no code-block CRC), C = 3 with an even and an odd part (every later block starts off
alignment: both the 4-elements-per-lane and the one-element path), C = 2 with a part of two 2048-bit steps, C = 3 with
five steps, C = 3 with 1749 fillers.  Btb = 1, 3, 5 (block-major rows; 4 code blocks per workgroup: partial workgroups).
"""
import functools
import os

import numpy as np
import pytest
import torch

import crc_model as cm
import tb_model as tm
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BG2 = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
PLANS = [(100, "16", 160), (300, "24A", 160), (297, "24A", 160), (7608, "24A", 3840), (25248, "24A", 8448),
         (20001, "24A", 8448)]
IDS = [f"A{p[0]}" for p in PLANS]
BATCHES = (1, 3, 5)
SPLITS = [(824, 4, 3), (274, 1, 3), (816, 4, 3)]  # (G, qm, C): E = 272, 276, 276; 91, 91, 92; all 272
GUARD = 0xAA


@functools.lru_cache(maxsize=None)
def _graph(Z):
    from nldpc.graph import LiftedGraph
    return LiftedGraph(BG2, Z)


def _plan(A, crc, W):
    from nldpc.transport import TBPlan
    return TBPlan.make(A, W=W, tb_crc=crc, kcb=W)


def _guarded(shape, dtype, fill, shift):
    """a tensor of `shape` that is a view into a larger buffer filled with `fill`, `shift` elements from its start"""
    n = int(np.prod(shape))
    buf = torch.full((shift + n + 19,), fill, dtype=dtype, device=DEV)
    return buf, buf[shift:shift + n].view(shape)


def _guards_intact(buf, view, fill, shift):
    n = view.numel()
    return bool((buf[:shift] == fill).all()) and bool((buf[shift + n:] == fill).all())


def _sub(rows, C, Btb, n=5):
    """the block-major rows of the first Btb of n transport blocks"""
    return rows.reshape(C, n, -1)[:, :Btb].reshape(C * Btb, -1)


@functools.lru_cache(maxsize=None)
def _blocks(A, crc, W, seed=0):
    """(model plan; raw payload bytes [5, A] with values 0, 1, 2, 255; the TBs with their CRC [5, B']; the model's code
    blocks [C * 5, W]) -- computed once, read-only"""
    p = tm.plan(A, crc, W)
    rng = np.random.default_rng(A + 7 * seed)
    raw = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), (5, A))
    tb = cm.attach(raw, crc)
    info = tm.segment(tb, p)
    assert cm.passes(tb, crc, A).all() and (p.C == 1 or cm.passes(info, "24B", p.Kp - 24).all())
    for arr in (raw, tb, info):
        arr.setflags(write=False)
    return p, raw, tb, info


@pytest.mark.parametrize("A,crc,W", PLANS, ids=IDS)
def test_segment_equals_the_model(A, crc, W):
    from nldpc.crc import attach
    from nldpc.transport import segment
    p, raw, tb_want, info_want = _blocks(A, crc, W)
    plan = _plan(A, crc, W)
    for Btb, shift in zip(BATCHES, (0, 3, 1)):
        buf, out = _guarded((p.C * Btb, W), torch.uint8, GUARD, shift)
        info, tb = segment(plan, torch.from_numpy(raw[:Btb].copy()).to(DEV), out=out)
        assert info.data_ptr() == out.data_ptr() and tb.dtype == torch.uint8 and tuple(tb.shape) == (Btb, plan.Bp)
        assert np.array_equal(tb.cpu().numpy(), tb_want[:Btb])
        assert np.array_equal(info.cpu().numpy(), _sub(info_want, p.C, Btb)), Btb
        assert _guards_intact(buf, out, GUARD, shift)
    # drawn payloads: the bits crc.attach draws for rows of B' bits; segment of those bits; the model's blocks
    info, tb = segment(plan, Btb=5, seed=11)
    assert tuple(info.shape) == (p.C * 5, W)
    tb_np = tb.cpu().numpy()
    assert np.array_equal(tb_np, attach(None, crc, W=plan.Bp, B=5, A=A, seed=11, device=DEV).cpu().numpy())
    assert np.array_equal(segment(plan, tb[:, :A].contiguous())[0].cpu().numpy(), info.cpu().numpy())
    assert np.array_equal(info.cpu().numpy(), tm.segment(tb_np, p))
    # the shards 0..2 and 3..4 draw the unsharded batch
    whole = info.cpu().numpy().reshape(p.C, 5, W)
    for off, n in ((0, 3), (3, 2)):
        part, tb_part = segment(plan, Btb=n, seed=11, b_offset=off)
        assert np.array_equal(tb_part.cpu().numpy(), tb_np[off:off + n])
        assert np.array_equal(part.cpu().numpy().reshape(p.C, n, W), whole[:, off:off + n])
    if A > 64:
        assert not np.array_equal(segment(plan, Btb=5, seed=12)[1].cpu().numpy(), tb_np)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["uint8", "fp32"])
@pytest.mark.parametrize("G,qm,C", SPLITS)
def test_concat_and_deconcat_equal_the_model(G, qm, C, dtype):
    from nldpc.transport import concat, deconcat
    E = tm.split_E(G, qm, C)
    C_lo = sum(1 for e in E if e == E[0])
    fill = GUARD if dtype == torch.uint8 else -7.5
    rng = np.random.default_rng(G)
    for Btb in BATCHES:
        if dtype == torch.uint8:
            f = [rng.integers(0, 256, (Btb, e)).astype(np.uint8) for e in E]
        else:
            f = [rng.standard_normal((Btb, e)).astype(np.float32) for e in E]
        want = tm.concat(f, Btb)
        f_lo = torch.from_numpy(np.concatenate(f[:C_lo])).to(DEV)
        f_hi = torch.from_numpy(np.concatenate(f[C_lo:])).to(DEV) if C_lo < C else None
        for shift in (0, 1, 3):  # the first output element 0, 1, 3 elements from a 16-byte boundary
            buf, out = _guarded((Btb, G), dtype, fill, shift)
            assert out.data_ptr() % 16 == (shift * out.element_size()) % 16
            g = concat(f_lo, f_hi, Btb, out=out)
            assert g.data_ptr() == out.data_ptr() and np.array_equal(g.cpu().numpy(), want), (Btb, shift)
            assert _guards_intact(buf, out, fill, shift)
            # the inverse, into views shifted the same way; deconcat(concat(x)) == x
            b_lo, o_lo = _guarded((C_lo * Btb, E[0]), dtype, fill, shift)
            b_hi, o_hi = _guarded(((C - C_lo) * Btb, E[-1]), dtype, fill, 3 - shift) if C_lo < C else (None, None)
            d_lo, d_hi = deconcat(g, C, C_lo, E[0], E[-1], out=(o_lo, o_hi))
            parts = tm.deconcat(want, E)
            assert d_lo.data_ptr() == o_lo.data_ptr() and np.array_equal(d_lo.cpu().numpy(), np.concatenate(parts[:C_lo]))
            assert torch.equal(d_lo, f_lo) and _guards_intact(b_lo, o_lo, fill, shift)
            if C_lo < C:
                assert np.array_equal(d_hi.cpu().numpy(), np.concatenate(parts[C_lo:])) and torch.equal(d_hi, f_hi)
                assert _guards_intact(b_hi, o_hi, fill, 3 - shift)
            else:
                assert d_hi is None
        fresh = concat(f_lo, f_hi, Btb)
        assert fresh.dtype == dtype and np.array_equal(fresh.cpu().numpy(), want)
        r_lo, r_hi = deconcat(fresh, C, C_lo, E[0], E[-1])
        assert torch.equal(r_lo, f_lo) and (r_hi is None if f_hi is None else torch.equal(r_hi, f_hi))
    # one group alone through f_hi: every block has E_hi
    only = concat(None, f_lo, Btb)
    assert np.array_equal(only.cpu().numpy(), tm.concat(f[:C_lo], Btb))


def _posterior(bits, stride, rng, tail_flip=False):
    """fp32 [rows, stride] = +-(1 + |noise|) whose hard decision (LLR > 0) is `bits` in the first columns and 0 behind
    them (1 with tail_flip: flips only beyond K')"""
    full = np.full((bits.shape[0], stride), 1 if tail_flip else 0, dtype=np.uint8)
    full[:, :bits.shape[1]] = bits
    mag = 1.0 + np.abs(rng.standard_normal(full.shape))
    return (np.where(full != 0, mag, -mag)).astype(np.float32)


CHECK_PLANS = [(100, "16", 160, 832), (300, "24A", 160, 832), (297, "24A", 160, 832), (7608, "24A", 3840, 3841),
               (25248, "24A", 8448, 8449)]


@pytest.mark.parametrize("A,crc,W,stride", CHECK_PLANS, ids=[f"A{p[0]}" for p in CHECK_PLANS])
def test_check_equals_the_model(A, crc, W, stride):
    """Damage to TB t* = Btb - 1 of a batch of clean TBs: (i) none; (ii) one payload bit of block r, for each r; (iii) one
    code-block parity bit; (iv) block r replaced by the valid block r of another TB; (v) flips only beyond K'."""
    from nldpc.transport import check
    p, _, tb5, info5 = _blocks(A, crc, W)
    _, _, _, other5 = _blocks(A, crc, W, seed=1)
    plan = _plan(A, crc, W)
    C, Kp, part = p.C, p.Kp, p.Kp - p.L
    rng = np.random.default_rng(A)
    damage = [("none", None)] + [("payload", r) for r in range(C)] + ([("parity", C - 1)] if C > 1 else []) + \
        [("swap", C // 2), ("tail", None)]
    for i, (kind, r) in enumerate(damage):
        Btb = BATCHES[i % 3]
        t = Btb - 1
        ref_tb = tb5[:Btb]
        blocks = _sub(info5, C, Btb)[:, :Kp].copy()
        if kind == "payload":
            blocks[r * Btb + t, int(rng.integers(0, part))] ^= 1
        elif kind == "parity":
            blocks[r * Btb + t, part + int(rng.integers(0, 24))] ^= 1
        elif kind == "swap":
            blocks[r * Btb + t] = _sub(other5, C, Btb)[r * Btb + t, :Kp]
            assert not np.array_equal(blocks[r * Btb + t, :part], _sub(info5, C, Btb)[r * Btb + t, :part])
        llr = _posterior(blocks, stride, rng, tail_flip=kind == "tail")
        hard = (llr > 0).astype(np.uint8)
        cb_want, tb_want, out_want, cnt_want = tm.check(hard, p, ref_tb)
        cnt_noref = tm.check(hard, p)[3]
        # the named outcomes, by themselves
        if kind in ("none", "tail"):
            assert cb_want.all() and tb_want.all() and cnt_want.tolist() == [0, 0, 0, 0]
        elif kind == "payload":
            assert not cb_want[r * Btb + t] and cb_want.sum() == C * Btb - 1 and cnt_want.tolist() == [1, 0, 1, 1]
        elif kind == "parity":
            assert not cb_want[r * Btb + t] and tb_want.all() and np.array_equal(out_want, ref_tb)
            assert cnt_want.tolist() == [0, 0, 0, 1]
        elif C > 1:  # another valid block: every code block passes, only the TB CRC fails
            assert cb_want.all() and not tb_want[t] and tb_want.sum() == Btb - 1 and cnt_want.tolist() == [1, 0, 1, 0]
        else:  # C == 1: another valid TB is an undetected error
            assert tb_want.all() and cnt_want.tolist() == [0, 1, 1, 0]
        ref_dev = torch.from_numpy(ref_tb.copy()).to(DEV)
        bits = hard * np.uint8(255 if i % 2 else 1)
        for arr, convention in ((llr, 0), (-llr, 1), (bits, 0)):
            x = torch.from_numpy(arr).to(DEV)
            bufs = [_guarded((C * Btb,), torch.uint8, GUARD, 3), _guarded((Btb,), torch.uint8, GUARD, 1),
                    _guarded((Btb, plan.Bp), torch.uint8, GUARD, 3 if i % 2 else 0), _guarded((4,), torch.int64, 0x55, 2)]
            bufs[3][1].copy_(torch.tensor([10, 20, 30, 40], device=DEV))
            if stride == 832:
                x = x.view(C * Btb, 52, 16)  # a decoder posterior's other shape
            res = check(plan, x, ref_tb=ref_dev, convention=convention, cb_ok=bufs[0][1], tb_ok=bufs[1][1],
                        tb_out=bufs[2][1], counts=bufs[3][1])
            what = (kind, r, Btb, str(x.dtype), convention)
            assert res.cb_ok.data_ptr() == bufs[0][1].data_ptr() and res.counts.data_ptr() == bufs[3][1].data_ptr()
            assert np.array_equal(res.cb_ok.cpu().numpy(), cb_want.astype(np.uint8)), what
            assert np.array_equal(res.tb_ok.cpu().numpy(), tb_want.astype(np.uint8)), what
            assert np.array_equal(res.tb_out.cpu().numpy(), out_want), what
            assert np.array_equal(res.counts.cpu().numpy(), cnt_want + np.array([10, 20, 30, 40])), what
            for (buf, view), fill, shift in zip(bufs, (GUARD, GUARD, GUARD, 0x55), (3, 1, 3 if i % 2 else 0, 2)):
                assert _guards_intact(buf, view, fill, shift), what
            # without ref_tb the middle counts stay 0; fresh outputs; only what was asked for
            res = check(plan, x, convention=convention, counts=True)
            assert res.tb_out is None and res.counts.dtype == torch.int64
            assert np.array_equal(res.counts.cpu().numpy(), cnt_noref), what
            assert np.array_equal(res.cb_ok.cpu().numpy(), cb_want.astype(np.uint8))
            assert np.array_equal(res.tb_ok.cpu().numpy(), tb_want.astype(np.uint8))
            res = check(plan, x, convention=convention, cb_ok=False, tb_ok=False, tb_out=True)
            assert res.cb_ok is None and res.tb_ok is None and res.counts is None
            assert np.array_equal(res.tb_out.cpu().numpy(), out_want), what
    # a list of T inputs: a leading dimension T
    clean = torch.from_numpy(_posterior(_sub(info5, C, 3)[:, :Kp], stride, rng)).to(DEV)
    dirty = clean.clone()
    dirty[C * 3 - 1, 0] *= -1  # the first bit of the last block of TB 2
    res = check(plan, [dirty, clean], ref_tb=torch.from_numpy(tb5[:3].copy()).to(DEV), counts=True, tb_out=True)
    assert tuple(res.cb_ok.shape) == (2, 3 * C) and tuple(res.tb_ok.shape) == (2, 3)
    assert tuple(res.counts.shape) == (2, 4) and tuple(res.tb_out.shape) == (2, 3, plan.Bp)
    assert res.counts.tolist() == [[1, 0, 1, 1], [0, 0, 0, 0]] and res.tb_ok.tolist() == [[1, 1, 0], [1, 1, 1]]
    assert np.array_equal(res.tb_out[1].cpu().numpy(), tb5[:3])


def _neural(xa, T=10):
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    g = _graph(16)
    w, b = torch.full((T, g.E), 0.75, device=DEV), torch.zeros((T, g.E), device=DEV)
    outs, _, _ = decode(g, DecodeCfg(kind=KIND_NEURAL, keep_state=False), xa, T, w_cn=w, bias=b)
    return list(outs)


def test_pipeline_counts_equal_the_model():
    """BG2 z=16, A = 300 (C = 3, F = 28), Btb = 8, 16-QAM, G = 824 (E = 272, 276, 276): segment -> encode ->
    rate_match_blocks -> qam_llr -> rate_recover_blocks -> Neural T=10 -> check(the 10 posteriors, ref_tb=tb) at 0 dB
    and 20 dB.  Verdicts and counts are compared with the model applied to the downloaded posteriors, never with a fixed
    count.  At 20 dB the last iteration's counts are [0, 0, 0, 0]: only noise far beyond what that SNR produces could
    flip a 16-QAM decision.  0 dB is below the capacity limit of rate-1/2 16-QAM (1.76 dB): at least one TB fails."""
    from nldpc.channel import encode
    from nldpc.modulation import qam_llr, sigma_for
    from nldpc.ratematch import RateMatch, rate_match
    from nldpc.transport import check, rate_match_blocks, rate_recover_blocks, segment
    g, Btb, T, G, qm = _graph(16), 8, 10, 824, 4
    plan = _plan(300, "24A", 160)
    p = tm.plan(300, "24A", 160)
    assert (plan.C, plan.F) == (3, 28)
    info, tb = segment(plan, Btb=Btb, seed=7)
    y = encode(g, info)
    f = rate_match_blocks(g, plan, y, G, qm=qm)
    assert f.dtype == torch.uint8 and tuple(f.shape) == (Btb, G)
    # the rows of the two E groups, rate matched by plain rate_match with the model's E_r, concatenate to g
    E = tm.split_E(G, qm, 3)
    assert E == [272, 276, 276]
    per_block = [rate_match(g, RateMatch.nr5g(g, E[r], rv=0, n_filler=28, qm=qm), y[r * Btb:(r + 1) * Btb]).cpu().numpy()
                 for r in range(3)]
    assert np.array_equal(f.cpu().numpy(), tm.concat(per_block, Btb))
    tb_np = tb.cpu().numpy()
    assert np.array_equal(info.cpu().numpy(), tm.segment(tb_np, p))
    for ebn0_db in (0.0, 20.0):
        sigma = sigma_for(ebn0_db, 3 * plan.Kp / G, qm)  # (rate 0.48)
        llr = qam_llr(f, qm, sigma, seed=77)
        xa = rate_recover_blocks(g, plan, llr, G, qm=qm, erasure_value=1e-3, filler_value=-20.0)
        assert tuple(xa.shape) == (3 * Btb, g.N, g.Z)
        outs = _neural(xa, T)
        res = check(plan, outs, ref_tb=tb, counts=True, tb_out=True)
        for t, o in enumerate(outs):
            cb_want, tb_want, out_want, cnt_want = tm.check((o.cpu().numpy() > 0).astype(np.uint8), p, tb_np)
            assert np.array_equal(res.cb_ok[t].cpu().numpy(), cb_want.astype(np.uint8)), (ebn0_db, t)
            assert np.array_equal(res.tb_ok[t].cpu().numpy(), tb_want.astype(np.uint8)), (ebn0_db, t)
            assert np.array_equal(res.tb_out[t].cpu().numpy(), out_want), (ebn0_db, t)
            assert np.array_equal(res.counts[t].cpu().numpy(), cnt_want), (ebn0_db, t)
        print(f"{ebn0_db} dB: (TB failures, undetected, TB errors, CB failures) per iteration:", res.counts.cpu().tolist())
        if ebn0_db == 20.0:
            assert res.counts[-1].tolist() == [0, 0, 0, 0]
        else:
            assert int(res.counts[-1, 0]) >= 1


def test_bad_arguments_raise_value_error():
    from nldpc.transport import check, concat, deconcat, rate_match_blocks, rate_recover_blocks, segment
    g = _graph(16)
    plan = _plan(300, "24A", 160)
    u8 = torch.zeros((6, 160), dtype=torch.uint8, device=DEV)
    llr = torch.zeros((6, 832), device=DEV)
    y = torch.zeros((6, 832), dtype=torch.uint8, device=DEV)
    for bad in (lambda: segment(plan, u8[:2, :150].contiguous()), lambda: segment(plan, u8.float()),
                lambda: segment(plan, Btb=2, out=torch.empty((6, 161), dtype=torch.uint8, device=DEV)),
                lambda: segment(plan, Btb=2, out=torch.empty((6, 160), dtype=torch.uint8)),
                lambda: concat(u8, u8.float(), 2), lambda: concat(u8, None, 4), lambda: concat(u8.t(), None, 2),
                lambda: concat(u8, None, 2, out=torch.empty((2, 481), dtype=torch.uint8, device=DEV)),
                lambda: deconcat(u8, 3, 1, 50, 56), lambda: deconcat(u8.double(), 3, 1, 50, 55),
                lambda: deconcat(u8, 3, 1, 50, 55, out=(u8, None)),
                lambda: check(plan, llr[:5].contiguous()), lambda: check(plan, llr[:, :131].contiguous()),
                lambda: check(plan, llr.double()), lambda: check(plan, llr, cb_ok=False, tb_ok=False),
                lambda: check(plan, llr, ref_tb=u8[:2, :150].contiguous()), lambda: check(plan, llr, ref_tb=u8[:2].float()),
                lambda: check(plan, llr, counts=torch.zeros((3,), dtype=torch.int64, device=DEV)),
                lambda: check(plan, llr, tb_ok=torch.zeros((3,), dtype=torch.uint8, device=DEV)),
                lambda: check(plan, llr, tb_out=torch.zeros((2, 324), dtype=torch.uint8)),
                lambda: rate_match_blocks(g, plan, y, 825, qm=4),   # qm does not divide G
                lambda: rate_match_blocks(g, plan, y, 8, qm=4),     # fewer than one symbol per block
                lambda: rate_match_blocks(g, plan, y[:5].contiguous(), 824, qm=4),
                lambda: rate_match_blocks(g, _plan(100, "16", 116), y, 824, qm=4),  # W is not K*Z
                lambda: rate_recover_blocks(g, plan, llr, 824, qm=4), lambda: rate_recover_blocks(g, plan, llr, 825, qm=4),
                lambda: rate_recover_blocks(g, plan, llr[:, :824].contiguous(), 824, qm=4, accumulate=True)):
        with pytest.raises(ValueError):
            bad()
