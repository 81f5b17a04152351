"""Gold-sequence scrambling on the GPU (nldpc_gold_sequence / nldpc_scramble / nldpc_descramble_llr /
nldpc_qam_channel_llr_scrambled; nldpc.scrambling, modulation.qam_llr(scramble=)).  Expected values come from
gold_model.py (TS 38.211 §5.2.1 bit by bit) and qam_model.py, never from the library.

Sequence lengths put a run boundary (a thread owns 4 words = 128 bits), a word boundary and a partial last run in every
position.  Element shapes (B, E, b_offset, n_seq): one element; rows shorter than a thread's 16 bytes so that a thread
crosses several row ends; odd E with rows off every alignment; one sequence for all rows; the headline row length.  The
fused channel runs every shape of test_gpu_modulation (half pairs, pairs straddling two rows -- two sequences in one
thread --, the misaligned element path).
"""
import functools
import os

import numpy as np
import pytest
import torch

import gold_model as gm
import qam_model as qm_
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
C_INITS = [0, 0x12345, 0x7FFFFFFF, 0x1F4002A, 1]
LENGTHS = [1, 31, 32, 33, 127, 128, 129, 4097, 25344]
ELEM_SHAPES = [(1, 1, 0, 1), (5, 67, 3, 3), (131, 6, 1, 4), (3, 2000, 0, 1), (3, 7680, 2, 2)]
QAM_SHAPES = [(2, 1, 1, 0), (4, 67, 5, 3), (6, 1, 131, 1), (8, 250, 3, 0), (6, 1280, 3, 0)]  # test_gpu_modulation.SHAPES
SIGMA = {2: 0.5, 4: 0.25, 6: 0.12, 8: 0.06}
SEED = 4242
GUARD = 0x5A


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the references are read-only)


def _u32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(shape, dtype, fill, shift):
    """a tensor of `shape` that is a view into a larger buffer filled with `fill`, `shift` elements from its start"""
    n = int(np.prod(shape))
    buf = torch.full((shift + n + 19,), fill, dtype=dtype, device=DEV)
    return buf, buf[shift:shift + n].view(shape)


def _guards_intact(buf, view, fill, shift):
    n = view.numel()
    return bool((buf[:shift] == fill).all()) and bool((buf[shift + n:] == fill).all())


@functools.lru_cache(maxsize=None)
def _table(n_seq, E):
    t = gm.table(C_INITS[:n_seq], E)
    t.setflags(write=False)
    return t


# ---------------------------------------------------------------- 1. the sequence table
@pytest.mark.parametrize("n_seq", [1, 5])
@pytest.mark.parametrize("E", LENGTHS)
def test_sequence_equals_the_packed_model(E, n_seq):
    from nldpc.scrambling import sequence
    want = _table(n_seq, E)
    Wc = (E + 31) // 32
    assert want.shape == (n_seq, Wc)
    for shift in (0, 1, 3):  # the table 0, 4, 12 bytes from a 16-byte boundary
        buf, out = _guarded((n_seq, Wc), torch.int32, 0x5A5A5A5A, shift)
        got = sequence(C_INITS[:n_seq], E, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(_u32(got), want), (E, n_seq, shift)
        assert _guards_intact(buf, out, 0x5A5A5A5A, shift)
    fresh = sequence(torch.tensor(C_INITS[:n_seq], dtype=torch.int32, device=DEV), E)
    assert fresh.dtype == torch.int32 and tuple(fresh.shape) == (n_seq, Wc) and np.array_equal(_u32(fresh), want)
    if E % 32:
        assert not (_u32(fresh)[:, -1] >> np.uint32(E % 32)).any()  # the tail bits of the last word
    if n_seq == 1:
        one = sequence(C_INITS[0], E, device=DEV)  # a bare int
        assert np.array_equal(_u32(one), want)
        # of a negative entry the low 31 bits are used
        neg = sequence(torch.tensor([0x12345 - 2 ** 31], dtype=torch.int32, device=DEV), E)
        assert np.array_equal(_u32(neg)[0], _table(2, E)[1])


def test_sequence_does_not_depend_on_the_run_length():
    """4096 rows of 129 words: beyond 65536 runs of 4 words the library gives a thread 16 words (the last run of a row
    is then one word), and every row still equals the model's row of its c_init"""
    from nldpc.scrambling import sequence
    E, n_seq = 4097, 4096
    want = _table(5, E)
    ci = torch.tensor(C_INITS, dtype=torch.int32, device=DEV).repeat(n_seq // 5 + 1)[:n_seq].contiguous()
    buf, out = _guarded((n_seq, (E + 31) // 32), torch.int32, 0x5A5A5A5A, 1)
    got = _u32(sequence(ci, E, out=out))
    assert np.array_equal(got, want[np.arange(n_seq) % 5])
    assert _guards_intact(buf, out, 0x5A5A5A5A, 1)


# ---------------------------------------------------------------- 2. scramble / descramble
@functools.lru_cache(maxsize=None)
def _elem_case(B, E, off, n_seq):
    rng = np.random.default_rng(B * 100000 + E)
    cis = C_INITS[:n_seq]
    f = rng.choice(np.array([0, 1, 255], dtype=np.uint8), (B, E))
    llr = (rng.standard_normal((B, E)) * 4).astype(np.float32)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC00002, 0x7F800003, 0xFFBFFFFF,
                        0x00000001, 0x80000001], dtype=np.uint32).view(np.float32)
    flat = llr.reshape(-1)
    pos = rng.permutation(flat.size)[:min(flat.size, 4 * special.size)]
    flat[pos] = np.resize(special, pos.size)  # +0, -0, +-inf, NaNs with distinct payloads, +- the smallest subnormal
    c = dict(cis=cis, f=f, llr=llr, fs=gm.scramble(f, cis, off), unpacked=gm.rows(cis, B, E, off),
             ds=gm.descramble(llr, cis, off))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@pytest.mark.parametrize("B,E,off,n_seq", ELEM_SHAPES)
def test_scramble_equals_the_model(B, E, off, n_seq):
    from nldpc.scrambling import scramble, sequence
    c = _elem_case(B, E, off, n_seq)
    seq = sequence(c["cis"], E, device=DEV)
    f = _dev(c["f"])
    got = scramble(f, seq, b_offset=off)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, E)
    assert np.array_equal(got.cpu().numpy(), c["fs"])
    assert torch.equal(f, _dev(c["f"]))  # the input is untouched
    # the all-zero word is the sequence unpacked
    assert np.array_equal(scramble(None, seq, B=B, E=E, b_offset=off).cpu().numpy(), c["unpacked"])
    # in place
    g = f.clone()
    assert scramble(g, seq, b_offset=off, out=g).data_ptr() == g.data_ptr()
    assert np.array_equal(g.cpu().numpy(), c["fs"])
    # input and output one byte off, in guarded buffers
    for shift_in, shift_out in ((1, 1), (1, 0), (0, 3)):
        ibuf, fin = _guarded((B, E), torch.uint8, GUARD, shift_in)
        fin.copy_(f)
        obuf, out = _guarded((B, E), torch.uint8, GUARD, shift_out)
        assert scramble(fin, seq, b_offset=off, out=out).data_ptr() == out.data_ptr()
        assert np.array_equal(out.cpu().numpy(), c["fs"]), (shift_in, shift_out)
        assert _guards_intact(obuf, out, GUARD, shift_out) and _guards_intact(ibuf, fin, GUARD, shift_in)
        assert torch.equal(fin, f)
    # twice is the 0 / 1 form of the input
    assert np.array_equal(scramble(got, seq, b_offset=off).cpu().numpy(), (c["f"] != 0).astype(np.uint8))


@pytest.mark.parametrize("B,E,off,n_seq", ELEM_SHAPES)
def test_descramble_equals_the_model_bit_for_bit(B, E, off, n_seq):
    from nldpc.scrambling import descramble, sequence
    c = _elem_case(B, E, off, n_seq)
    seq = sequence(c["cis"], E, device=DEV)
    llr = _dev(c["llr"])
    got = descramble(llr, seq, b_offset=off)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, E)
    assert np.array_equal(_u32(got), _u32(c["ds"]))
    assert np.array_equal(_u32(llr), _u32(c["llr"]))
    # only sign bits change, and where the sequence says
    assert np.array_equal((_u32(got) ^ _u32(c["llr"])) >> np.uint32(31), c["unpacked"].astype(np.uint32))
    assert not ((_u32(got) ^ _u32(c["llr"])) & np.uint32(0x7FFFFFFF)).any()
    # twice is the identity, bit for bit
    assert np.array_equal(_u32(descramble(got, seq, b_offset=off)), _u32(c["llr"]))
    # in place
    g = llr.clone()
    assert descramble(g, seq, b_offset=off, out=g).data_ptr() == g.data_ptr()
    assert np.array_equal(_u32(g), _u32(c["ds"]))
    # input and output 3 elements (12 bytes) off a 16-byte boundary, in guarded buffers
    for shift_in, shift_out in ((3, 3), (3, 0), (0, 1)):
        ibuf, lin = _guarded((B, E), torch.float32, 777.25, shift_in)
        lin.view(torch.int32).copy_(llr.view(torch.int32))
        obuf, out = _guarded((B, E), torch.float32, 777.25, shift_out)
        assert descramble(lin, seq, b_offset=off, out=out).data_ptr() == out.data_ptr()
        assert np.array_equal(_u32(out), _u32(c["ds"])), (shift_in, shift_out)
        assert _guards_intact(obuf, out, 777.25, shift_out) and _guards_intact(ibuf, lin, 777.25, shift_in)


# ---------------------------------------------------------------- 3. the fused channel
@functools.lru_cache(maxsize=None)
def _qam_case(qm, S, B, off, n_seq):
    """the shared, read-only reference of one shape: the model's chain scramble -> noisy symbols -> demap -> sign flip"""
    rng = np.random.default_rng(qm * 1000 + S + B)
    cis = C_INITS[:n_seq]
    f = rng.choice(np.array([0, 1, 255], dtype=np.uint8), (B, S * qm))
    sigma = float(np.float32(SIGMA[qm]))
    fs = gm.scramble(f, cis, off)
    noisy = qm_.noisy_symbols(fs, qm, sigma, SEED, off)
    sign = 1.0 - 2.0 * gm.rows(cis, B, S * qm, off).astype(np.float64)
    ll64, dmax = qm_.logmap64(noisy, qm, sigma)
    c = dict(cis=cis, f=f, sigma=sigma, noisy=noisy, maxlog=gm.descramble(qm_.maxlog(noisy, qm, sigma), cis, off),
             logmap=ll64 * sign, bound=qm_.logmap_bound(qm, ll64, dmax))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@pytest.mark.parametrize("n_seq", [1, 3])
@pytest.mark.parametrize("method", ["maxlog", "logmap"])
@pytest.mark.parametrize("qm,S,B,off", QAM_SHAPES)
def test_fused_channel_equals_the_composition_and_the_model(qm, S, B, off, method, n_seq):
    from nldpc.modulation import qam_llr
    from nldpc.scrambling import descramble, scramble, sequence
    c = _qam_case(qm, S, B, off, n_seq)
    E, sigma = S * qm, c["sigma"]
    seq = sequence(c["cis"], E, device=DEV)
    f = _dev(c["f"])
    llr, sym = qam_llr(f, qm, sigma, seed=SEED, b_offset=off, method=method, return_symbols=True, scramble=seq)
    assert llr.dtype == sym.dtype == torch.float32 and tuple(llr.shape) == (B, E) and tuple(sym.shape) == (B, S, 2)
    # the three-launch composition, bit for bit; the symbols are those of the scrambled bits
    l3, s3 = qam_llr(scramble(f, seq, b_offset=off), qm, sigma, seed=SEED, b_offset=off, method=method,
                     return_symbols=True)
    assert np.array_equal(_u32(llr), _u32(descramble(l3, seq, b_offset=off)))
    assert np.array_equal(_u32(sym), _u32(s3))
    alone = qam_llr(f, qm, sigma, seed=SEED, b_offset=off, method=method, scramble=seq)
    assert isinstance(alone, torch.Tensor) and np.array_equal(_u32(alone), _u32(llr))
    # the model's chain
    got = llr.cpu().numpy()
    if method == "maxlog":
        differ = int((_u32(got) != _u32(c["maxlog"])).sum())
        print(f"qm={qm} S={S} B={B} n_seq={n_seq}: {differ} of {got.size} max-log LLRs differ from the model's, "
              f"{int((sym.cpu().numpy() != c['noisy']).sum())} symbol components")
        assert differ == 0
    else:
        err = np.abs(got.astype(np.float64) - c["logmap"])
        print(f"qm={qm} S={S} B={B} n_seq={n_seq}: max err / bound = {(err / c['bound']).max():.3f}")
        assert (err <= c["bound"]).all()
    # the all-zero word: f = None equals f = zeros
    zeros = torch.zeros((B, E), dtype=torch.uint8, device=DEV)
    a, sa = qam_llr(None, qm, sigma, B=B, E=E, seed=SEED, b_offset=off, method=method, return_symbols=True,
                    scramble=seq, device=DEV)
    z, sz = qam_llr(zeros, qm, sigma, seed=SEED, b_offset=off, method=method, return_symbols=True, scramble=seq)
    assert np.array_equal(_u32(a), _u32(z)) and np.array_equal(_u32(sa), _u32(sz))


@pytest.mark.parametrize("qm,S,B,off", QAM_SHAPES)
def test_fused_channel_writes_nothing_outside_its_outputs(qm, S, B, off):
    from nldpc.modulation import qam_llr
    from nldpc.scrambling import sequence
    c = _qam_case(qm, S, B, off, 3)
    E = S * qm
    seq = sequence(c["cis"], E, device=DEV)
    ref, rs = qam_llr(_dev(c["f"]), qm, c["sigma"], seed=SEED, b_offset=off, return_symbols=True, scramble=seq)
    fbuf = torch.full((B * E + 8,), GUARD, dtype=torch.uint8, device=DEV)
    f = fbuf[1:1 + B * E].view(B, E)  # the bits start off a dword boundary
    f.copy_(_dev(c["f"]))
    lbuf, llr = _guarded((B, E), torch.float32, 777.25, 3)
    sbuf, so = _guarded((B, S, 2), torch.float32, 777.25, 3)
    got, gs = qam_llr(f, qm, c["sigma"], seed=SEED, b_offset=off, out=llr, return_symbols=so, scramble=seq)
    assert got.data_ptr() == llr.data_ptr() and gs.data_ptr() == so.data_ptr()
    assert _guards_intact(lbuf, llr, 777.25, 3) and _guards_intact(sbuf, so, 777.25, 3)
    assert np.array_equal(_u32(got), _u32(ref)) and np.array_equal(_u32(gs), _u32(rs))


# ---------------------------------------------------------------- 4. sharding
def test_a_shard_uses_the_sequences_and_the_noise_of_the_unsharded_batch():
    from nldpc.modulation import qam_llr
    from nldpc.scrambling import descramble, scramble, sequence
    qm, S, B, n_seq = 4, 67, 5, 3
    c = _qam_case(qm, S, B, 0, n_seq)
    seq = sequence(c["cis"], S * qm, device=DEV)
    f = _dev(c["f"])
    llr, sym = qam_llr(f, qm, c["sigma"], seed=SEED, return_symbols=True, scramble=seq)
    part = f[2:].contiguous()
    l2, s2 = qam_llr(part, qm, c["sigma"], seed=SEED, b_offset=2, return_symbols=True, scramble=seq)
    assert np.array_equal(_u32(l2), _u32(llr[2:])) and np.array_equal(_u32(s2), _u32(sym[2:]))
    assert np.array_equal(scramble(part, seq, b_offset=2).cpu().numpy(), scramble(f, seq)[2:].cpu().numpy())
    assert np.array_equal(_u32(descramble(llr[2:].contiguous(), seq, b_offset=2)), _u32(descramble(llr, seq)[2:]))
    # b_offset selects the sequence: another offset gives other bits on the air
    assert not np.array_equal(_u32(qam_llr(part, qm, c["sigma"], seed=SEED, b_offset=2, return_symbols=True,
                                           scramble=seq)[1]),
                              _u32(qam_llr(part, qm, c["sigma"], seed=SEED, b_offset=2, return_symbols=True,
                                           scramble=seq.roll(1, 0).contiguous())[1]))


# ---------------------------------------------------------------- 5. the all-zero word
def _nearest(sym, qm):
    from nldpc.modulation import points
    s = sym.cpu().numpy().reshape(-1, 2).astype(np.float64)
    p = points(qm)
    p = np.stack([p.real, p.imag], axis=1).astype(np.float64)
    return ((s[:, None, :] - p[None, :, :]) ** 2).sum(-1).argmin(1)


@pytest.mark.parametrize("qm", [4, 6, 8])
def test_the_scrambled_all_zero_word_visits_every_constellation_point(qm):
    """f = None, B = 2, E = qm * 4096, sigma = fp32 0.01, c_init = 0x12345.  Unscrambled, every symbol is the point of the
    all-zero label; scrambled, all 2^qm points occur, and the decoder still sees bit 0 (a negative LLR) everywhere but
    where the noise flipped a decision: the model's count of those, which may be 0 at this noise level."""
    from nldpc.modulation import qam_llr
    from nldpc.scrambling import sequence
    B, S, ci = 2, 4096, 0x12345
    E, sigma = qm * S, float(np.float32(0.01))
    bits = gm.rows([ci], B, E)
    labels = (bits.reshape(B * S, qm) * (1 << np.arange(qm - 1, -1, -1))).sum(1)
    assert len(np.unique(labels)) == 2 ** qm  # the model: this sequence's bit groups cover every label
    zeros = np.zeros((B, E), dtype=np.uint8)
    seq = sequence(ci, E, device=DEV)
    for table, sent in ((None, zeros), (seq, bits)):
        llr, sym = qam_llr(None, qm, sigma, B=B, E=E, seed=SEED, return_symbols=True, scramble=table, device=DEV)
        near = _nearest(sym, qm)
        want_llr = qm_.maxlog(qm_.noisy_symbols(sent, qm, sigma, SEED), qm, sigma)
        if table is not None:
            want_llr = gm.descramble(want_llr, [ci])
        flips_want = int((_u32(want_llr) >> np.uint32(31) == 0).sum())
        flips = int((_u32(llr) >> np.uint32(31) == 0).sum())
        print(f"qm={qm} scrambled={table is not None}: {len(np.unique(near))} distinct points, {flips} LLRs not negative "
              f"(model {flips_want})")
        if table is None:
            assert len(np.unique(near)) == 1 and near[0] == 0
        else:
            assert len(np.unique(near)) == 2 ** qm
            assert np.array_equal(near, labels)  # point v is the symbol of the label v: the bits on the air are c
        assert flips == flips_want


# ---------------------------------------------------------------- 6. the chain
BG2 = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")


def test_transport_chain_with_one_sequence_per_transport_block():
    """test_gpu_transport's pipeline plan (BG2 z=16, A = 300, C = 3, G = 824, 16-QAM) at its error-free 20 dB, one c_init
    per TB: segment -> encode -> rate_match_blocks -> qam_llr(scramble=) -> rate_recover_blocks -> Neural T=10 -> check:
    every TB passes.  Then the unfused receiver descrambles TB 0 with another c_init: half its LLR signs are wrong, its
    TB CRC fails, and the other TBs still pass."""
    from nldpc.channel import encode
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    from nldpc.graph import LiftedGraph
    from nldpc.modulation import qam_llr, sigma_for
    from nldpc.scrambling import c_init, descramble, scramble, sequence
    from nldpc.transport import TBPlan, check, rate_match_blocks, rate_recover_blocks, segment
    g, Btb, T, G, qm = LiftedGraph(BG2, 16), 8, 10, 824, 4
    plan = TBPlan.make(300, W=160, tb_crc="24A", kcb=160)
    assert (plan.C, plan.F) == (3, 28)
    info, tb = segment(plan, Btb=Btb, seed=7)
    f = rate_match_blocks(g, plan, encode(g, info), G, qm=qm)
    cis = [c_init(1000 + t, 42) for t in range(Btb)]
    seq = sequence(cis, G, device=DEV)
    assert tuple(seq.shape) == (Btb, (G + 31) // 32) and np.array_equal(_u32(seq), gm.table(cis, G))
    sigma = sigma_for(20.0, 3 * plan.Kp / G, qm)

    def receive(llr):
        xa = rate_recover_blocks(g, plan, llr, G, qm=qm, erasure_value=1e-3, filler_value=-20.0)
        w, b = torch.full((T, g.E), 0.75, device=DEV), torch.zeros((T, g.E), device=DEV)
        outs, _, _ = decode(g, DecodeCfg(kind=KIND_NEURAL, keep_state=False), xa, T, w_cn=w, bias=b)
        return check(plan, list(outs)[-1], ref_tb=tb, tb_out=True)

    res = receive(qam_llr(f, qm, sigma, seed=77, scramble=seq))
    assert res.tb_ok.cpu().tolist() == [1] * Btb and torch.equal(res.tb_out, tb)
    wrong = sequence([c_init(999, 42)] + cis[1:], G, device=DEV)
    llr = descramble(qam_llr(scramble(f, seq), qm, sigma, seed=77), wrong)
    res = receive(llr)
    print("tb_ok with TB 0 descrambled by another c_init:", res.tb_ok.cpu().tolist())
    assert res.tb_ok.cpu().tolist() == [0] + [1] * (Btb - 1)
    assert torch.equal(res.tb_out[1:], tb[1:])


def test_bad_arguments_raise_value_error():
    from nldpc.modulation import qam_llr
    from nldpc.scrambling import descramble, scramble, sequence
    B, E = 2, 24
    f = torch.zeros((B, E), dtype=torch.uint8, device=DEV)
    llr = torch.zeros((B, E), device=DEV)
    seq = sequence([1, 2], E, device=DEV)
    for bad in (lambda: scramble(f, seq.cpu()), lambda: scramble(f, seq.long()), lambda: scramble(f, seq[:, 0]),
                lambda: scramble(f, sequence([1], 40, device=DEV)), lambda: scramble(f, seq, b_offset=-1),
                lambda: scramble(f.t().contiguous().t(), seq), lambda: scramble(f, seq, out=torch.empty((B, E + 1), dtype=torch.uint8, device=DEV)),
                lambda: scramble(f, seq, out=torch.empty((B, E), dtype=torch.uint8)), lambda: scramble(f, seq, out=llr),
                lambda: descramble(llr, seq.cpu()), lambda: descramble(llr, sequence([1], 40, device=DEV)),
                lambda: descramble(llr, seq, b_offset=-1), lambda: descramble(llr, seq, out=torch.empty((B, E))),
                lambda: descramble(llr.double(), seq), lambda: descramble(f, seq),
                lambda: sequence([1], E, out=torch.empty((1, 2), dtype=torch.int32, device=DEV)),
                lambda: sequence([1], E, out=torch.empty((1, 1), dtype=torch.int64, device=DEV)),
                lambda: sequence(torch.tensor([1], device=DEV), E),  # int64
                lambda: qam_llr(f, 4, 0.5, scramble=seq.cpu()), lambda: qam_llr(f, 4, 0.5, scramble=seq.long()),
                lambda: qam_llr(f, 4, 0.5, scramble=sequence([1], 40, device=DEV)),
                lambda: qam_llr(None, 4, 0.5, B=B, E=E, scramble=seq[:, :0])):
        with pytest.raises(ValueError):
            bad()
