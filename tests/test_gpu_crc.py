"""CRC attachment and checking (nldpc_crc_attach / nldpc_crc_check, nldpc.crc) on the GPU, bit for bit against the long
division of crc_model.py, with guard bytes around every output.

Lengths: A = 1 (a row shorter than one word), 9, 40 (A + L no multiple of 32), 2024 (A + 24 = 2048, exactly one 2048-bit
step of a wave), 2049 (two steps, the first almost all padding), 4099 (three steps).  B = 1, 3 and 130 (a workgroup
holds 4 rows: a partial last workgroup).  Strides A + L, A + L + 1 (odd: rows start off every alignment) and a
codeword's N*Z.  All six polynomials at the three short lengths, 24A and 16 at the long ones, and one row of more than
one step for each of the other four.
"""
import functools
import os

import numpy as np
import pytest
import torch

import crc_model as cm
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BG2 = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
SHORT, LONG = (1, 9, 40), (2024, 2049, 4099)
CASES = [(A, name) for A in SHORT for name in cm.NAMES] + [(A, name) for A in LONG for name in ("24A", "16")] + \
    [(2049, "24B"), (2049, "24C"), (4099, "11"), (2049, "6")]  # (the step-to-step tables of the other four)
BATCHES = (1, 3, 130)
GUARD = 0xAA


@functools.lru_cache(maxsize=None)
def _graph(Z):
    from nldpc.graph import LiftedGraph
    return LiftedGraph(BG2, Z)


def _guarded(shape, dtype, fill, shift):
    """a tensor of `shape` that is a view into a larger buffer filled with `fill`, `shift` elements from its start"""
    n = int(np.prod(shape))
    buf = torch.full((shift + n + 19,), fill, dtype=dtype, device=DEV)
    return buf, buf[shift:shift + n].view(shape)


def _guards_intact(buf, view, fill, shift):
    n = view.numel()
    return bool((buf[:shift] == fill).all()) and bool((buf[shift + n:] == fill).all())


@functools.lru_cache(maxsize=None)
def _blocks(A, name):
    """(raw payload bytes [130, A] with values 0, 1, 2, 255; the model's attached blocks [130, A + L]; the blocks with
    1 or 2 flipped bits in a seeded half of the rows; the model's verdict of those) -- computed once, read-only"""
    L = cm.length(name)
    rng = np.random.default_rng(A * 100 + L)
    raw = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), (130, A))
    clean = cm.attach(raw, name)
    hit = clean.copy()
    for b in np.flatnonzero(rng.integers(0, 2, 130)):
        pos = rng.choice(A + L, size=min(int(rng.integers(1, 3)), A + L), replace=False)
        hit[b, pos] ^= 1
    ok = cm.passes(hit, name, A)
    assert ok.any() and not ok.all() and cm.passes(clean, name, A).all()
    for arr in (raw, clean, hit, ok):
        arr.setflags(write=False)
    return raw, clean, hit, ok


@pytest.mark.parametrize("A,name", CASES)
def test_attach_equals_long_division(A, name):
    from nldpc.crc import attach
    L = cm.length(name)
    raw, clean, _, _ = _blocks(A, name)
    for B in BATCHES:
        pay = torch.from_numpy(raw[:B].copy()).to(DEV)
        for W, shift in ((A + L, 0), (A + L + 37, 3)):
            buf, out = _guarded((B, W), torch.uint8, GUARD, shift)
            got = attach(pay, name, W=W, out=out)
            assert got.data_ptr() == out.data_ptr()
            want = np.concatenate([clean[:B], np.zeros((B, W - A - L), np.uint8)], axis=1)
            assert np.array_equal(got.cpu().numpy(), want), (B, W)
            assert _guards_intact(buf, out, GUARD, shift)
    fresh = attach(torch.from_numpy(raw[:3].copy()).to(DEV), name)
    assert fresh.dtype == torch.uint8 and tuple(fresh.shape) == (3, A + L)
    assert np.array_equal(fresh.cpu().numpy(), clean[:3])


@pytest.mark.parametrize("Z,A,B", [(16, 135, 6), (16, 136, 5), (384, 3815, 6), (384, 1, 3)])
def test_drawn_payloads_are_the_encoders_info_bits(Z, A, B):
    from nldpc.channel import encode
    from nldpc.crc import attach, payload_len
    g = _graph(Z)
    W = g.K * Z
    assert payload_len(g, "24A") == W - 24 and payload_len(g, "24A", W - 24 - A) == A
    y = encode(g, B=B, seed=99).cpu().numpy()
    buf, out = _guarded((B, W), torch.uint8, GUARD, 5)
    info = attach(None, "24A", graph=g, B=B, A=A, seed=99, out=out).cpu().numpy()
    assert _guards_intact(buf, out, GUARD, 5)
    assert np.array_equal(info[:, :A], y[:, :A])
    assert np.array_equal(info, cm.attach(y[:, :A], "24A", W))
    # two shards (A = 135 and 3815 are odd, B even there) draw the unsharded batch; another seed draws other bits
    h = B // 2
    parts = [attach(None, "24A", W=W, B=n, A=A, seed=99, b_offset=o, device=DEV) for o, n in ((0, h), (h, B - h))]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), info)
    if A > 64:
        assert not np.array_equal(attach(None, "24A", W=W, B=B, A=A, seed=98, device=DEV).cpu().numpy(), info)


def _as_llr(bits, convention, rng):
    """fp32 LLRs whose hard decision under `convention` is `bits`, with +0, -0, NaN (bit 0 either way) and both
    infinities planted"""
    sign = np.where(bits != 0, 1.0, -1.0) * (1.0 if convention == 0 else -1.0)
    llr = (sign * rng.uniform(0.05, 9.0, bits.shape)).astype(np.float32)
    kind = rng.integers(0, 12, bits.shape)
    llr[kind == 0] = np.where(llr[kind == 0] > 0, np.inf, -np.inf)
    zero = bits == 0
    llr[zero & (kind == 1)] = 0.0
    llr[zero & (kind == 2)] = -0.0
    llr[zero & (kind == 3)] = np.nan
    with np.errstate(invalid="ignore"):
        assert np.array_equal(llr > 0 if convention == 0 else llr < 0, bits != 0)
    return llr


def _strided(rows, stride, fill, rng):
    """rows [B, n] placed at the start of the rows of a [B, stride] array whose tail holds junk"""
    out = rng.choice(np.asarray(fill, dtype=rows.dtype), (rows.shape[0], stride))
    out[:, :rows.shape[1]] = rows
    return out


@pytest.mark.parametrize("A,name", CASES)
def test_check_equals_long_division(A, name):
    from nldpc.crc import check
    L = cm.length(name)
    n = A + L
    _, _, hit, want = _blocks(A, name)
    NZ = 832 if n <= 832 else 19968  # BG2 z=16 / z=384 codeword lengths
    rng = np.random.default_rng(n)
    for B in BATCHES:
        for stride in (n, n + 1, NZ):
            bits = _strided(hit[:B] * np.uint8(255 if stride == n + 1 else 1), stride, [0, 1, 7], rng)
            ok = check(torch.from_numpy(bits).to(DEV), name, A)
            assert ok.dtype == torch.uint8 and tuple(ok.shape) == (B,)
            assert np.array_equal(ok.cpu().numpy(), want[:B].astype(np.uint8)), ("bits", B, stride)
            for convention in (0, 1):
                llr = _strided(_as_llr(hit[:B], convention, rng), stride, [-3.0, 0.0, 2.5, np.nan], rng)
                buf, out = _guarded((B,), torch.uint8, GUARD, 3)
                x = torch.from_numpy(llr).to(DEV)
                if stride == NZ:
                    x = x.view(B, 52, NZ // 52)  # a decoder posterior's other shape
                got = check(x, name, A, convention=convention, ok=out)
                assert got.data_ptr() == out.data_ptr()
                assert np.array_equal(got.cpu().numpy(), want[:B].astype(np.uint8)), ("llr", B, stride, convention)
                assert _guards_intact(buf, out, GUARD, 3)


@pytest.mark.parametrize("A,name", [(9, "6"), (40, "11"), (2049, "16"), (4099, "24A")])
def test_counts_equal_numpy(A, name):
    from nldpc.crc import check
    L = cm.length(name)
    n, B = A + L, 130
    _, clean, hit, _ = _blocks(A, name)
    # an undetected error: row 0 of the input is another valid block than the reference's row 0
    other = hit.copy()
    other[0] = clean[1]
    assert not np.array_equal(clean[0], clean[1])
    rng = np.random.default_rng(n)
    x = torch.from_numpy(_strided(other, n + 5, [0, 1], rng)).to(DEV)
    llr = torch.from_numpy(_strided(_as_llr(other, 0, rng), n + 1, [1.0, -1.0], rng)).to(DEV)
    ref = torch.from_numpy(_strided(clean, n + 2, [0, 1], rng)).to(DEV)
    with_ref, without = cm.counts(other, name, A, clean), cm.counts(other, name, A)
    assert with_ref[1] >= 1 and with_ref[2] > with_ref[0] > 0 and without[0] == with_ref[0]
    ok_want = cm.passes(other, name, A).astype(np.uint8)
    for inp in (x, llr):
        ok, c = check(inp, name, A, counts=True)
        assert c.dtype == torch.int64 and tuple(c.shape) == (3,)
        assert np.array_equal(c.cpu().numpy(), without) and np.array_equal(ok.cpu().numpy(), ok_want)
        ok, c = check(inp, name, A, ref=ref, counts=True)
        assert np.array_equal(c.cpu().numpy(), with_ref) and np.array_equal(ok.cpu().numpy(), ok_want)
        # another ref_stride (a contiguous copy of the first n columns); ref bytes other than 0 / 1
        ok, c = check(inp, name, A, ref=(ref[:, :n] * 3).contiguous(), counts=True)
        assert np.array_equal(c.cpu().numpy(), with_ref)
        # counts accumulate over two calls, into a guarded tensor; ok=False computes the counts alone
        buf, acc = _guarded((3,), torch.int64, 0x55, 2)
        acc.zero_()
        assert check(inp, name, A, ref=ref, counts=acc, ok=False) is acc
        assert check(inp[:7].contiguous(), name, A, ref=ref[:7].contiguous(), counts=acc, ok=None) is acc
        assert np.array_equal(acc.cpu().numpy(), with_ref + cm.counts(other[:7], name, A, clean[:7]))
        assert _guards_intact(buf, acc, 0x55, 2)
        # counts=None: ok alone
        assert np.array_equal(check(inp, name, A, ref=ref).cpu().numpy(), ok_want)
    # a list of T inputs: ok [T, B], counts [T, 3]
    ok, c = check([x, torch.from_numpy(_strided(clean, n + 5, [0, 1], rng)).to(DEV)], name, A, ref=ref, counts=True)
    assert tuple(ok.shape) == (2, B) and tuple(c.shape) == (2, 3)
    assert np.array_equal(c.cpu().numpy(), np.stack([with_ref, np.zeros(3, np.int64)]))
    assert np.array_equal(ok.cpu().numpy(), np.stack([ok_want, np.ones(B, np.uint8)]))


def test_bad_tensors_raise_value_error():
    from nldpc.crc import attach, check
    bits = torch.zeros((4, 64), dtype=torch.uint8, device=DEV)
    llr = torch.zeros((4, 64), device=DEV)
    for bad in (bits.float(), bits[:, :-1], bits.reshape(-1), bits.t().contiguous().t()):
        with pytest.raises(ValueError):
            attach(bad, "16")
    for out in (torch.empty((4, 81), dtype=torch.uint8, device=DEV), torch.empty((4, 80), device=DEV),
                torch.empty((4, 80), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            attach(bits, "16", out=out)
    for bad in (llr.double(), llr[:, :-1], llr.reshape(-1), [llr, bits], [llr, llr[:2].contiguous()]):
        with pytest.raises(ValueError):
            check(bad, "16", 40)
    for kw in (dict(A=49), dict(A=40, ref=bits[:, :55].contiguous()), dict(A=40, ref=llr), dict(A=40, ref=bits[:2].contiguous()),
               dict(A=40, ok=torch.empty((5,), dtype=torch.uint8, device=DEV)), dict(A=40, ok=False),
               dict(A=40, counts=torch.zeros((3,), dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            check(llr, "16", **kw)


def test_a_wrong_codeword_is_a_codeword():
    """Random info bits without a CRC, encoded: every row has syndrome weight 0, and the CRC verdict is the model's --
    a failure for every row whose 24 'parity' positions are not, by chance, the parity of the 136 before them.  Seed 11:
    on the CPU the model fails all 32 rows."""
    from nldpc.channel import encode, syndrome_weight
    from nldpc.crc import check
    g = _graph(16)
    info = np.random.default_rng(11).integers(0, 2, (32, 160)).astype(np.uint8)
    want = cm.passes(info, "24A", 136)
    assert not want.any()
    y = encode(g, torch.from_numpy(info).to(DEV))
    llr = (y.float() * 2 - 1) * 4.0
    assert not syndrome_weight(llr, g).any()
    assert np.array_equal(check(y, "24A", 136).cpu().numpy(), want.astype(np.uint8))
    assert np.array_equal(check(llr.view(32, 52, 16), "24A", 136).cpu().numpy(), want.astype(np.uint8))


def _neural(xa, T=10):
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    g = _graph(16)
    w, b = torch.full((T, g.E), 0.75, device=DEV), torch.zeros((T, g.E), device=DEV)
    outs, _, _ = decode(g, DecodeCfg(kind=KIND_NEURAL, keep_state=False), xa, T, w_cn=w, bias=b)
    return list(outs)


def test_pipeline_counts_equal_the_model():
    """BG2 z=16: attach (A = 112, CRC24A, 24 fillers) -> encode -> rate 1/2 match (E = 272, qm = 2) -> BPSK AWGN ->
    recover -> Neural T=10 -> check(the 10 posteriors, ref=y) at 1 dB and 8 dB.  The [T, 3] counts and first_pass are
    compared with the model applied to the downloaded posteriors, never with a fixed error count.  The same chain
    decodes 8 words without error from iteration 4 on at 6 dB (test_rate_half_end_to_end_decodes); at 8 dB the last
    iteration's row is (0, 0, 0)."""
    from nldpc.channel import awgn_llr, encode
    from nldpc.crc import attach, check, first_pass, payload_len
    from nldpc.ratematch import RateMatch, code_rate, rate_match, rate_recover
    g, B, T = _graph(16), 32, 10
    A = payload_len(g, "24A", 24)
    assert A == 112
    info = attach(None, "24A", graph=g, B=B, A=A, seed=7)
    y = encode(g, info)
    rm = RateMatch.nr5g(g, 272, rv=0, n_filler=24, qm=2)
    f = rate_match(g, rm, y)
    y_np = y.cpu().numpy()
    assert cm.passes(y_np, "24A", A).all() and not y_np[:, A + 24:160].any()
    for ebn0_db in (1.0, 8.0):
        sigma = float(np.float32(np.sqrt(1 / (2 * code_rate(g, rm) * 10 ** (ebn0_db / 10)))))
        llr = awgn_llr(B, 272, 1, sigma, seed=77, device=DEV, y=f).reshape(B, 272)
        outs = _neural(rate_recover(g, rm, llr, erasure_value=1e-3, filler_value=-20.0), T)
        ok, counts = check(outs, "24A", A, ref=y, counts=True)
        hard = [(o.cpu().numpy() > 0).astype(np.uint8) for o in outs]
        want = np.stack([cm.counts(h, "24A", A, y_np) for h in hard])
        ok_want = np.stack([cm.passes(h, "24A", A) for h in hard]).astype(np.uint8)
        print(f"{ebn0_db} dB: (CRC failures, undetected, block errors) per iteration:", want.tolist())
        assert np.array_equal(counts.cpu().numpy(), want)
        assert np.array_equal(ok.cpu().numpy(), ok_want)
        if ebn0_db == 8.0:
            assert counts[-1].tolist() == [0, 0, 0]
        else:
            assert want[0, 0] > 0  # (the low SNR exercises failures)
        out, iters, fin = first_pass(outs, "24A", A)
        tstar = np.where(ok_want.any(0), ok_want.argmax(0), T - 1)
        stack = np.stack([o.cpu().numpy() for o in outs])
        assert np.array_equal(out.cpu().numpy(), stack[tstar, np.arange(B)])
        assert iters.dtype == torch.int32 and np.array_equal(iters.cpu().numpy(), tstar + 1)
        assert np.array_equal(fin.cpu().numpy(), ok_want[tstar, np.arange(B)])
