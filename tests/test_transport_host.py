"""Transport-block arithmetic on the host (nldpc_tb_plan, nldpc_tb_lifting_size, nldpc_tb_er, nldpc_tb_crc_ref: the
inline functions of csrc/nldpc_tb.h the kernels run) and the argument rules of nldpc.transport, without a GPU.  Expected
values come from tb_model.py (TS 38.212 restated literally) and from the table of plans below.
"""
import ctypes
import functools

import numpy as np
import pytest

import crc_model as cm
import tb_model as tm

# A, TB CRC, kcb = W -> C, K', part, F
PLANS = [
    (100, "16", 160, 1, 116, 116, 44),       # L = 0
    (300, "24A", 160, 3, 132, 108, 28),
    (297, "24A", 160, 3, 131, 107, 29),      # an odd part: every later block starts off alignment
    (7608, "24A", 3840, 2, 3840, 3816, 0),   # a part longer than one 2048-bit step
    (25248, "24A", 8448, 3, 8448, 8424, 0),  # five steps
    (20001, "24A", 8448, 3, 6699, 6675, 1749),
    (61032, "24A", 3840, 16, 3840, 3816, 0),
]
IDS = [f"A{p[0]}" for p in PLANS]


def _make(A, crc, W):
    from nldpc.transport import TBPlan
    return TBPlan.make(A, W=W, tb_crc=crc, kcb=W)


@pytest.mark.parametrize("A,crc,W,C,Kp,part,F", PLANS, ids=IDS)
def test_plan_values(A, crc, W, C, Kp, part, F):
    from nldpc.transport import TBPlan
    p = _make(A, crc, W)
    L = 24 if C > 1 else 0
    assert (p.A, p.tb_crc, p.W, p.C, p.L, p.Kp, p.F) == (A, crc, W, C, L, Kp, F)
    assert p.part == part and p.Bp == A + cm.length(crc) == C * part
    assert tuple(tm.plan(A, crc, W)) == (A, crc, W, C, L, Kp, F)
    # kcb = 0 means W; the default TB CRC is 24A above 3824 payload bits, else 16
    assert TBPlan.make(A, W=W, tb_crc=crc) == p
    assert TBPlan.make(3824, W=8448).tb_crc == "16" and TBPlan.make(3825, W=8448).tb_crc == "24A"

    class G:
        K, Z = W // 16, 16

    if W % 16 == 0:
        assert TBPlan.make(A, graph=G, tb_crc=crc) == p


def test_plans_the_rule_rejects():
    from nldpc import _lib
    from nldpc.transport import TBPlan
    for kw in (dict(A=20000, W=8448, kcb=8448, tb_crc="24A"),  # C = 3 does not divide B'' = 20096
               dict(A=300, W=100, kcb=160, tb_crc="24A"),      # K' = 132 > W (kcb > W)
               dict(A=300, W=160, kcb=161, tb_crc="24A"),      # kcb > W
               dict(A=300, W=160, kcb=24, tb_crc="24A"),       # kcb <= 24 and segmentation needed
               dict(A=300, W=160, kcb=10, tb_crc="24A"),
               dict(A=2 ** 31 - 24, W=2 ** 31 - 1, tb_crc="24A"),  # B' >= 2^31
               dict(A=5, W=2 ** 31, tb_crc="16"), dict(A=0, W=160), dict(A=-3, W=160), dict(A=100),
               dict(A=100, W=160, tb_crc="24D"), dict(A=100, W=160, kcb=-1), dict(A="100", W=160),
               dict(A=100, W=160.5), dict(A=True, W=160)):
        with pytest.raises(ValueError):
            TBPlan.make(kw.pop("A"), **kw)
    with pytest.raises(ValueError):
        tm.plan(20000, "24A", 8448)
    Lb = _lib.lib()
    c = _lib.NldpcTb()
    assert Lb.nldpc_tb_plan(20000, 0, 8448, 8448, ctypes.byref(c)) == _lib.NLDPC_EINVAL
    assert b"nldpc_tb_plan" in Lb.nldpc_last_error()
    assert Lb.nldpc_tb_plan(300, 0, 160, 0, None) == _lib.NLDPC_EINVAL
    for crc in (-1, 6):
        assert Lb.nldpc_tb_plan(300, crc, 160, 0, ctypes.byref(c)) == _lib.NLDPC_EINVAL
    assert Lb.nldpc_tb_plan(2 ** 40, 0, 160, 0, ctypes.byref(c)) == _lib.NLDPC_EINVAL


def test_round_down():
    from nldpc.transport import TBPlan
    assert TBPlan.round_down(20001, W=8448, tb_crc="24A").A == 20001
    p = TBPlan.round_down(20000, W=8448, tb_crc="24A")
    assert p.A == 19998 and p.C == 3 and (p.Bp + 72) % 3 == 0  # (20000 and 19999 leave B'' = 20096, 20095)
    for A in (299, 298, 297, 61040, 3830, 3825, 3824):
        for kw in (dict(W=160, tb_crc="24A"), dict(W=160), dict(W=3840, kcb=3840)):
            got = TBPlan.round_down(A, **kw)
            want = next(a for a in range(A, 0, -1) if _fits(a, kw))
            assert got.A == want and got == TBPlan.make(want, **kw)
    for bad in (dict(W=160, kcb=161), dict(), dict(W=160, tb_crc="x"), dict(W=160, kcb=-2)):
        with pytest.raises(ValueError):
            TBPlan.round_down(300, **bad)


def _fits(a, kw):
    try:
        tm.plan(a, kw.get("tb_crc") or ("24A" if a > 3824 else "16"), kw["W"], kw.get("kcb", 0))
        return True
    except ValueError:
        return False


def test_lifting_size_equals_the_search_over_the_51_sizes():
    from nldpc.transport import lifting_size
    assert len(tm.LIFTING_SIZES) == 51 and tm.LIFTING_SIZES[0] == 2 and tm.LIFTING_SIZES[-1] == 384
    # the Kb thresholds of BG2
    assert [lifting_size(2, b)[0] for b in (192, 193, 560, 561, 640, 641)] == [6, 8, 8, 9, 9, 10]
    assert lifting_size(1, 100)[0] == 22
    rng = np.random.default_rng(5)
    sizes = {1, 2, 12, 13, 192, 193, 560, 561, 640, 641, 3840, 3841, 8448, 8449, 61056, 25272, 2 ** 20}
    sizes |= {int(v) for v in rng.integers(1, 20000, 300)} | {6 * z + d for z in tm.LIFTING_SIZES for d in (0, 1)}
    sizes |= {10 * z + d for z in tm.LIFTING_SIZES for d in (0, 1)} | {22 * z + d for z in tm.LIFTING_SIZES for d in (0, 1)}
    for bg in (1, 2):
        for b in sorted(sizes):
            assert lifting_size(bg, b) == tm.lifting_size(bg, b), (bg, b)
    assert lifting_size(2, 61056) == (10, 384) and lifting_size(1, 25272) == (22, 384)
    for bad in ((0, 100), (3, 100), (2, 0), (2, 2 ** 31), ("2", 100)):
        with pytest.raises(ValueError):
            lifting_size(*bad)


def test_split_E_equals_the_rule():
    from nldpc.transport import split_E
    p3 = _make(300, "24A", 160)
    assert split_E(p3, 824, 4) == (272, 276, 1) and tm.split_E(824, 4, 3) == [272, 276, 276]
    assert split_E(p3, 274, 1) == (91, 92, 2) and tm.split_E(274, 1, 3) == [91, 91, 92]
    assert split_E(p3, 816, 4) == (272, 272, 3) and tm.split_E(816, 4, 3) == [272, 272, 272]
    p16, p1 = _make(61032, "24A", 3840), _make(100, "16", 160)
    assert split_E(p16, 16 * 7680, 6) == (7680, 7680, 16)
    for p in (p1, p3, p16):
        for qm, nl in ((1, 1), (2, 1), (4, 2), (6, 1), (8, 4)):
            for Gp in (p.C, p.C + 1, 2 * p.C - 1, 97, 1000, 1001, 1003):
                if Gp < p.C:
                    continue
                G = Gp * qm * nl
                lo, hi, clo = split_E(p, G, qm, nl)
                assert [lo] * clo + [hi] * (p.C - clo) == tm.split_E(G, qm, p.C, nl), (p.C, G, qm, nl)
                assert 1 <= clo <= p.C and clo * lo + (p.C - clo) * hi == G
    for bad in (dict(G=825, qm=4), dict(G=8, qm=4), dict(G=0, qm=1), dict(G=824, qm=0), dict(G=824, qm=4, n_layers=0),
                dict(G=2 ** 31, qm=1), dict(G="824", qm=4)):
        with pytest.raises(ValueError):
            split_E(p3, **bad)


@functools.lru_cache(maxsize=None)
def _tb(A, crc, W):
    """(model plan, one TB's bits with its CRC [1, B'], its code blocks [C, W]) from seeded random payload bits"""
    p = tm.plan(A, crc, W)
    rng = np.random.default_rng(A)
    tb = cm.attach(rng.integers(0, 2, (1, A)).astype(np.uint8), crc)
    info = tm.segment(tb, p)
    tb.setflags(write=False)
    info.setflags(write=False)
    return p, tb, info


@pytest.mark.parametrize("A,crc,W,C,Kp,part,F", PLANS, ids=IDS)
def test_combined_remainder_equals_long_division(A, crc, W, C, Kp, part, F):
    """nldpc_tb_crc_ref combines the parts' remainders (R(part r) * x^{(C-1-r) part}); the model divides the reassembled
    TB as a whole.  Clean blocks, one flipped bit in each part, a flipped code-block parity bit, random rows."""
    from nldpc.transport import remainder
    p, tb, info = _tb(A, crc, W)
    lib_plan = _make(A, crc, W)

    ok, rem = remainder(lib_plan, info)
    assert ok.all() and rem == 0 and np.array_equal(tm.desegment(info, p), tb)
    rng = np.random.default_rng(A + 1)
    cases = []
    for r in range(C):  # one payload bit of part r: block r fails, and the TB
        for pos in sorted({0, part - 1, int(rng.integers(0, part))}):
            hit = info.copy()
            hit[r, pos] ^= 1
            cases.append(hit)
    if C > 1:  # a parity bit of block C - 1: the block fails, the TB passes
        hit = info.copy()
        hit[C - 1, part + 5] ^= 1
        cases.append(hit)
    cases.append(rng.integers(0, 2, info.shape).astype(np.uint8))
    cases.append(np.zeros_like(info))  # the all-zero TB passes
    # the model on all cases at once: case t is TB t of a block-major batch
    n = len(cases)
    batch = np.stack(cases, axis=1).reshape(C * n, W)
    whole = tm.desegment(batch, p)
    rems = cm.parity_int(whole, crc)  # (what nldpc_crc_ref gives for the B' bits: TB(x) x^L_tb mod g; 0 = divisible)
    cbs = cm.passes(batch, "24B", Kp - 24).reshape(C, n) if C > 1 else (rems == 0)[None]
    assert rems[0] != 0 and rems[-1] == 0 and (C == 1 or (rems[-3] == 0 and not cbs[C - 1, -3] and cbs[:C - 1, -3].all()))
    for t, hit in enumerate(cases):
        ok, rem = remainder(lib_plan, hit * np.uint8(3))  # (any non-zero byte is 1)
        assert rem == rems[t] and np.array_equal(ok, cbs[:, t]), t
    # bits beyond K' are not read
    wide = np.concatenate([info[:, :Kp], np.ones((C, 3), np.uint8)], axis=1)
    assert remainder(lib_plan, wide)[1] == 0
    for bad in (info[:, :Kp - 1], info[:1] if C > 1 else info[:0], info.reshape(-1)):
        with pytest.raises(ValueError):
            remainder(lib_plan, bad)


def test_argument_rules_of_the_entry_points():
    """every NLDPC_EINVAL case of the launches is refused before a device is touched (the pointers are host memory and
    never dereferenced)"""
    from nldpc import _lib
    Lb = _lib.lib()
    EINVAL = _lib.NLDPC_EINVAL
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data
    assert p % 8 == 0
    good = _make(300, "24A", 160)._c()
    ref = ctypes.byref

    def broken(**kw):
        c = _make(300, "24A", 160)._c()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    bad_plans = [broken(C=2), broken(L=0), broken(Kp=131), broken(F=27), broken(tb_crc=9), broken(A=301), broken(C=0)]
    need = ctypes.c_size_t(0)
    assert Lb.nldpc_tb_workspace(ref(good), 5, ref(need)) == _lib.NLDPC_OK and need.value == 4 * 3 * 5
    for args in [(ref(c), 5, ref(need)) for c in bad_plans] + [(None, 5, ref(need)), (ref(good), 0, ref(need)),
                                                                 (ref(good), 5, None), (ref(good), 2 ** 30, ref(need))]:
        assert Lb.nldpc_tb_workspace(*args) == EINVAL
    # nldpc_tb_segment(plan, tb, Btb, info, stream)
    for args in [(ref(c), p, 2, p) for c in bad_plans] + [(None, p, 2, p), (ref(good), None, 2, p), (ref(good), p, 2, None),
                                                            (ref(good), p, 0, p), (ref(good), p, 2 ** 30, p)]:
        assert Lb.nldpc_tb_segment(*args, None) == EINVAL
    assert b"nldpc_tb_segment" in Lb.nldpc_last_error()
    # nldpc_tb_concat(elem_bytes, f_lo, f_hi, Btb, C, C_lo, E_lo, E_hi, g, stream)
    for args in ((2, p, p, 2, 3, 1, 8, 9, p), (1, p, p, 0, 3, 1, 8, 9, p), (1, p, p, 2, 0, 0, 8, 9, p),
                 (1, p, p, 2, 3, 4, 8, 9, p), (1, p, p, 2, 3, -1, 8, 9, p), (1, p, p, 2, 3, 1, 0, 9, p),
                 (1, p, p, 2, 3, 1, 8, 0, p), (1, p, p, 2, 3, 1, 8, 2 ** 31, p), (1, p, p, 2, 3, 1, 8, 2 ** 30, p),
                 (1, None, p, 2, 3, 1, 8, 9, p), (1, p, None, 2, 3, 1, 8, 9, p), (1, p, p, 2, 3, 1, 8, 9, None),
                 (4, p + 2, p, 2, 3, 1, 8, 9, p), (4, p, p, 2, 3, 1, 8, 9, p + 1), (1, p, p, 2 ** 30, 3, 1, 8, 9, p)):
        assert Lb.nldpc_tb_concat(*args, None) == EINVAL, args
        e, lo, hi, B, C, Clo, Elo, Ehi, g = args
        assert Lb.nldpc_tb_deconcat(e, g, B, C, Clo, Elo, Ehi, lo, hi, None) == EINVAL, args
    # nldpc_tb_check(plan, llr, bits, Btb, stride, convention, ref_tb, cb_ok, tb_ok, tb_out, counts, work, work_bytes)
    ok_args = [ref(good), p, None, 2, 160, 0, None, p, p, None, None, p, 24]
    for pos, val in ((0, None), (1, None), (2, p), (3, 0), (3, 2 ** 30), (4, 131), (5, 2), (5, -1), (1, p + 2),
                     (10, p + 4), (11, None), (11, p + 2), (12, 23)) + tuple((0, ref(c)) for c in bad_plans):
        args = list(ok_args)
        args[pos] = val
        assert Lb.nldpc_tb_check(*args, None) == EINVAL, (pos, val)
    args = list(ok_args)
    args[7] = args[8] = None  # every output NULL
    assert Lb.nldpc_tb_check(*args, None) == EINVAL
    assert b"nldpc_tb_check" in Lb.nldpc_last_error()
    rem = ctypes.c_uint32(0)
    for args in ((None, p, 160, p, ref(rem)), (ref(good), None, 160, p, ref(rem)), (ref(good), p, 131, p, ref(rem)),
                 (ref(bad_plans[0]), p, 160, p, ref(rem))):
        assert Lb.nldpc_tb_crc_ref(*args) == EINVAL
    assert Lb.nldpc_tb_crc_ref(ref(good), p, 160, None, None) == _lib.NLDPC_OK


def test_python_argument_errors():
    """CPU tensors and wrong shapes are refused with ValueError before anything is launched"""
    import torch
    from nldpc import transport as tr
    p = _make(300, "24A", 160)
    u8 = torch.zeros((6, 160), dtype=torch.uint8)
    f32 = torch.zeros((6, 832))

    class G:
        K, Z, N, M = 10, 16, 52, 42

    for bad in (lambda: tr.segment(p, torch.zeros((2, 300), dtype=torch.uint8)), lambda: tr.segment(p),
                lambda: tr.segment(p, Btb=0), lambda: tr.segment(p, Btb=2, device="cpu"),
                lambda: tr.segment(p, Btb=2, b_offset=-1),
                lambda: tr.segment(dataclasses_replace(p, C=2 ** 31), Btb=2),
                lambda: tr.concat(u8, None, 3), lambda: tr.concat(None, None, 3), lambda: tr.concat(u8, u8, 0),
                lambda: tr.deconcat(u8, 3, 1, 50, 55), lambda: tr.deconcat(u8, 3, 4, 50, 55),
                lambda: tr.check(p, f32), lambda: tr.check(p, u8), lambda: tr.check(p, []),
                lambda: tr.check(p, f32, convention=2), lambda: tr.check(p, [f32, u8]),
                lambda: tr.rate_match_blocks(G, p, u8, 824, qm=4), lambda: tr.rate_recover_blocks(G, p, f32, 824, qm=4),
                lambda: tr.rate_match_blocks(G, p, u8, 825, qm=4),  # a G the split rejects
                lambda: tr.rate_match_blocks(G, _make(300, "24A", 176), u8, 824, qm=4)):
        with pytest.raises(ValueError):
            bad()


def dataclasses_replace(p, **kw):
    import dataclasses
    return dataclasses.replace(p, **kw)
