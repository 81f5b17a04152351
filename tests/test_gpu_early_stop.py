"""Parity-check syndrome kernel (nldpc_syndrome) and the early-stopping decode (nldpc_forward_early_stop,
nldpc.decode.decode_early_stop, the two modules' decode_early_stop) on the GPU.

Expected values never come from the code under test: the posterior of every iteration comes from the existing
decode(...) with all T outputs (on the z=16 Neural case additionally pinned to oracle.neural_forward), the
syndrome weights and the stopping iteration t* from the numpy restatement of test_early_stop_gen.py.  Codeword b
takes Eb/N0 number b mod 5, so fast, slow and never-converging codewords share a workgroup; every case first
asserts that its expected values hold such a mix.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_early_stop_gen import unsat_numpy

pytestmark = pytest.mark.gpu

BG2 = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
WIMAX = np.loadtxt(os.path.join(ROOT, "resources", "wman_N0576_R34_z24.txt"), int, delimiter="\t")
GEN16 = np.loadtxt(os.path.join(ROOT, "resources", "gen_matrix_bg2_z16.txt"), int, delimiter=",")
DEV = torch.device("cuda")
T = 8
KINDS = {"SP": 0, "MS": 1, "QMS": 2, "Neural": 3}

# name -> (base graph, Z, code rate of sigma_for, Eb/N0 list, B, random codewords, puncturing, least number of
# distinct 0 < t* < T-1)
CASES = {
    "z16": (BG2, 16, 10 / 50, (-4, 3.5, 5, 9, 16), 30, True, None, 3),
    "z16p": (BG2, 16, 10 / 50, (-4, 3.5, 5, 9, 16), 30, True, (1, 32), 3),
    "z24": (WIMAX, 24, 0.75, (-4, 3, 4.5, 7, 16), 27, False, None, 3),
    "z384": (BG2, 384, 10 / 50, (-4, 4, 6, 9, 16), 5, False, None, 2),
}
RUNS = [("z16", "Neural"), ("z16", "MS"), ("z16", "QMS"), ("z16", "SP"), ("z16p", "Neural"), ("z24", "Neural"),
        ("z384", "Neural"), ("z384", "QMS")]


@functools.lru_cache(maxsize=None)
def _graph(case):
    from nldpc.graph import LiftedGraph
    hb, Z = CASES[case][:2]
    return LiftedGraph(hb, Z)


@functools.lru_cache(maxsize=None)
def _codewords(case):
    hb, Z, _, _, B, rand, _, _ = CASES[case]
    if not rand:
        return None
    info = np.random.default_rng(11).integers(0, 2, size=(B, GEN16.shape[0]))
    y = info @ GEN16 % 2
    assert not unsat_numpy(y, hb, Z).any()
    return y


@functools.lru_cache(maxsize=None)
def _inputs(case, kind):
    """Channel LLRs [B, N, Z] (device): codeword b at Eb/N0 number b mod 5."""
    from nldpc.channel import awgn_llr, sigma_for
    hb, Z, rate, ebn0s, B, _, punct, _ = CASES[case]
    N = hb.shape[1]
    y = _codewords(case)
    x = torch.empty((B, N, Z), dtype=torch.float32, device=DEV)
    for k, e in enumerate(ebn0s):
        rows = torch.arange(k, B, 5, device=DEV)
        yk = None if y is None else torch.from_numpy(y[k::5]).to(DEV)
        x[rows] = awgn_llr(len(rows), N, Z, sigma_for(e, rate), seed=2042, b_offset=1000 * k, device=DEV, y=yk,
                           qbit=5 if kind == "QMS" else 0, puncturing=punct)
    return x


def _weights(case, kind):
    g = _graph(case)
    if kind == "Neural":  # weights 0.5, bias 0; Boosted: NW(0, 0, 0), no weights
        return dict(w_cn=torch.full((T, g.E), 0.5, device=DEV), bias=torch.zeros((T, g.E), device=DEV))
    return {}


def _cfg(kind, path="auto", **kw):
    from nldpc.decode import DecodeCfg
    return DecodeCfg(kind=KINDS[kind], qbit=5, path=path, keep_state=False, **kw)


@functools.lru_cache(maxsize=None)
def _reference(case, kind, path):
    """(outs [T, B, N*Z] of the existing decode on `path`, unsat [T, B], t* [B]) -- computed once per case."""
    from nldpc.decode import decode
    hb, Z = CASES[case][:2]
    outs, _, _ = decode(_graph(case), _cfg(kind, path), _inputs(case, kind), T, **_weights(case, kind))
    outs = outs.cpu()
    bits = (outs.numpy() > 0).astype(np.int64)
    unsat = np.stack([unsat_numpy(bits[t], hb, Z) for t in range(T)])
    ok = unsat == 0
    tstar = np.where(ok.any(0), ok.argmax(0), T - 1)
    return outs, unsat, tstar


def _expected(case, kind, path):
    outs, unsat, tstar = _reference(case, kind, path)
    B = outs.shape[1]
    idx = torch.from_numpy(tstar)
    return outs[idx, torch.arange(B)], (tstar + 1).astype(np.int32), unsat[tstar, np.arange(B)].astype(np.int32)


def _check_mix(case, kind, path):
    """The expected values hold never-converging, immediately converging and slowly converging codewords."""
    _, unsat, tstar = _reference(case, kind, path)
    print(f"{case} {kind} {path}: t* = {tstar.tolist()} unsat(t*) = {unsat[tstar, np.arange(len(tstar))].tolist()}")
    assert (unsat != 0).all(0).any(), "no codeword that never converges"
    if case == "z16p":
        assert (tstar[(unsat == 0).any(0)] <= 2).any(), "no codeword with t* <= 2"
    else:
        assert (unsat[0] == 0).any(), "no codeword with t* = 0"
    mid = set(int(t) for t, c in zip(tstar, (unsat == 0).any(0)) if c and 0 < t < T - 1)
    assert len(mid) >= CASES[case][7], mid


@pytest.mark.parametrize("case,kind", RUNS)
def test_early_stop_equals_selected_iteration(case, kind):
    from nldpc.decode import decode_early_stop
    for path in ("fused", "stream"):
        _check_mix(case, kind, path)
        if kind != "SP":  # one set of expected values for both paths
            assert torch.equal(_reference(case, kind, path)[0], _reference(case, kind, "fused")[0])
        want_out, want_it, want_un = _expected(case, kind, path)
        out, iters, unsat = decode_early_stop(_graph(case), _cfg(kind, path), _inputs(case, kind), T,
                                              **_weights(case, kind))
        assert iters.dtype == torch.int32 and unsat.dtype == torch.int32
        assert np.array_equal(iters.cpu().numpy(), want_it), (path, iters.cpu().numpy(), want_it)
        assert np.array_equal(unsat.cpu().numpy(), want_un), (path, unsat.cpu().numpy(), want_un)
        assert torch.equal(out.cpu(), want_out), path


def test_reference_outputs_match_the_oracle_z16():
    from oracle.ldpc_oracle import OracleGraph, neural_forward
    outs = _reference("z16", "Neural", "fused")[0]
    w = _weights("z16", "Neural")
    ref = torch.stack(neural_forward(OracleGraph(BG2, 16), _inputs("z16", "Neural").cpu(), list(w["w_cn"].cpu()),
                                     list(w["bias"].cpu())))
    assert torch.equal(outs, ref)


def test_fused_request_runs_the_fused_kernel():
    """path="fused" runs one fused launch (the library's profile counters) and is refused with UCN; nldpc_fast_path
    answers for the early stop under saving = 4."""
    from nldpc import _lib
    from nldpc.decode import decode_early_stop
    L = _lib.lib()
    for case, kind in (("z16", "MS"), ("z24", "Neural"), ("z384", "Neural")):
        g = _graph(case)
        c = _cfg(kind, "fused").c_struct(False)
        fast = ctypes.c_int32(-1)
        _lib.check(L.nldpc_fast_path(g.handle(DEV), ctypes.byref(c), 4, T, 4, ctypes.byref(fast)))
        assert fast.value == 1, (case, kind)
        _lib.check(L.nldpc_profile_begin(8))
        decode_early_stop(g, _cfg(kind, "fused"), _inputs(case, kind), T, **_weights(case, kind))
        ms, cnt = (ctypes.c_float * 7)(), (ctypes.c_int32 * 7)()
        _lib.check(L.nldpc_profile_end(7, ms, cnt))
        assert list(cnt) == [0, 0, 0, 1, 0, 0, 0], list(cnt)
    g = _graph("z16")
    x = _inputs("z16", "MS")
    c = _cfg("MS", "fused", ucn=True).c_struct(False)
    fast = ctypes.c_int32(-1)
    _lib.check(L.nldpc_fast_path(g.handle(DEV), ctypes.byref(c), 4, T, 4, ctypes.byref(fast)))
    assert fast.value == 0
    with pytest.raises(NotImplementedError):
        decode_early_stop(g, _cfg("MS", "fused", ucn=True), x, T)
    # UCN on the default path: the fallback, against the same restatement
    from nldpc.decode import decode
    outs, _, _ = decode(g, _cfg("MS", ucn=True), x, T)
    bits = (outs.cpu().numpy() > 0).astype(np.int64)
    un = np.stack([unsat_numpy(bits[t], BG2, 16) for t in range(T)])
    ts = np.where((un == 0).any(0), (un == 0).argmax(0), T - 1)
    out, iters, unsat = decode_early_stop(g, _cfg("MS", ucn=True), x, T)
    assert np.array_equal(iters.cpu().numpy(), ts + 1)
    assert torch.equal(out.cpu(), outs.cpu()[torch.from_numpy(ts), torch.arange(len(ts))])
    assert np.array_equal(unsat.cpu().numpy(), un[ts, np.arange(len(ts))])


@pytest.mark.parametrize("case,kind", [("z16", "Neural"), ("z24", "Neural"), ("z16", "QMS")])
def test_codeword_alone_equals_codeword_in_batch(case, kind):
    from nldpc.decode import decode_early_stop
    x = _inputs(case, kind)
    want_out, want_it, want_un = _expected(case, kind, "fused")
    for b in range(x.shape[0]):
        out, iters, unsat = decode_early_stop(_graph(case), _cfg(kind, "fused"), x[b:b + 1], T, **_weights(case, kind))
        assert int(iters[0]) == want_it[b] and int(unsat[0]) == want_un[b], b
        assert torch.equal(out[0].cpu(), want_out[b]), b


def test_module_methods():
    import boosted_neural_ldpc_decoder as bd
    import neural_ldpc_decoder as nd
    from boosted_neural_ldpc_decoder.BoostedNeuralLDPCDecoder import BoostedNeuralLDPCDecoder
    from boosted_neural_ldpc_decoder.struct.DecoderType import DecoderType
    from boosted_neural_ldpc_decoder.struct.NodeWeightSharingConfig import NodeWeightSharingConfig as NW
    from nldpc.decode import decode_early_stop
    B = CASES["z16"][4]
    model = nd.NeuralLDPCDecoder(T, B, nd.ConnectingMatrixTorch(nd.ConnectingMatrix(16, BG2), device=DEV)).to(DEV)
    x = _inputs("z16", "Neural")
    got = model.decode_early_stop(x)
    want = decode_early_stop(_graph("z16"), _cfg("Neural"), x, T, **_weights("z16", "Neural"))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(got[0].cpu(), _expected("z16", "Neural", "fused")[0])
    for dt, kind in ((DecoderType.MS, "MS"), (DecoderType.QMS, "QMS")):
        bm = BoostedNeuralLDPCDecoder(T, B, bd.ConnectingMatrixTorch(bd.ConnectingMatrix(16, BG2), device=DEV),
                                      node_weight_sharing_config=NW(0, 0, 0), decoding_type=dt,
                                      decoder_qms_qbit=5).to(DEV)
        x = _inputs("z16", kind)
        with torch.no_grad():
            full = bm(x)
        before = [o.clone() for o in bm.outputs]
        ids = [id(o) for o in bm.outputs]
        got = bm.decode_early_stop(x)
        assert [id(o) for o in bm.outputs] == ids and all(torch.equal(a, b) for a, b in zip(bm.outputs, before))
        cfg = _cfg(kind, llr_lo=float(bm.allowed_llr_range.start), llr_hi=float(bm.allowed_llr_range.end))
        want = decode_early_stop(_graph("z16"), cfg, x, T)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        its = got[1].cpu().long() - 1
        assert torch.equal(got[0].cpu(), torch.stack(list(full)).cpu()[its, torch.arange(B)])


# ---------------------------------------------------------------- nldpc_syndrome
def _pm(bits):
    """Bits -> LLRs of magnitude 1 in the decoder's convention (bit = LLR > 0)."""
    return torch.from_numpy(np.where(np.asarray(bits) != 0, 1.0, -1.0).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("case,B", [("z16", 37), ("z24", 9), ("z384", 3)])
def test_syndrome_equals_numpy_on_random_llrs(case, B):
    from nldpc.channel import syndrome_weight
    hb, Z = CASES[case][:2]
    gen = torch.Generator().manual_seed(5)
    llr = torch.randn(B, hb.shape[1] * Z, generator=gen)
    llr[0, ::7] = 0.0  # exact zeros are bit 0
    sw = syndrome_weight(llr.to(DEV), _graph(case))
    assert sw.dtype == torch.int32 and tuple(sw.shape) == (1, B)
    assert np.array_equal(sw[0].cpu().numpy(), unsat_numpy((llr.numpy() > 0), hb, Z))
    sw1 = syndrome_weight([llr.to(DEV), (-llr).to(DEV)], _graph(case), convention=1)
    assert np.array_equal(sw1[0].cpu().numpy(), unsat_numpy((llr.numpy() < 0), hb, Z))
    assert np.array_equal(sw1[1].cpu().numpy(), unsat_numpy((llr.numpy() > 0), hb, Z))


def test_syndrome_of_codewords_and_single_flips():
    from nldpc.channel import syndrome_weight
    g = _graph("z16")
    y = _codewords("z16").copy()
    assert not syndrome_weight(_pm(y), g).cpu().numpy().any()
    deg = (BG2 != -1).sum(0)
    flipped = y.copy()
    pos = [(b * 29 + 3) % (52 * 16) for b in range(len(y))]
    for b, n in enumerate(pos):
        flipped[b, n] ^= 1
    assert np.array_equal(syndrome_weight(_pm(flipped), g)[0].cpu().numpy(), [deg[n // 16] for n in pos])
    # `>` against `>=`: a bit of value 1 whose LLR is exactly 0 reads as bit 0, i.e. as flipped
    llr = _pm(y)
    ones = [int(np.nonzero(y[b])[0][b % 5]) for b in range(len(y))]
    for b, n in enumerate(ones):
        llr[b, n] = 0.0
    assert np.array_equal(syndrome_weight(llr, g)[0].cpu().numpy(), [deg[n // 16] for n in ones])


# ---------------------------------------------------------------- C ABI
def test_capi_refusals():
    from nldpc import _lib
    from nldpc.graph import LiftedGraph
    L = _lib.lib()
    g = _graph("z16")
    x = _inputs("z16", "MS").contiguous()
    B = x.shape[0]
    out = torch.empty((B, 52 * 16), device=DEV)
    iters = torch.empty((B,), dtype=torch.int32, device=DEV)

    def call(graph, c, t=T):
        return L.nldpc_forward_early_stop(graph.handle(DEV), ctypes.byref(c), B, t, x.data_ptr(), None, None, None, None,
                                          out.data_ptr(), iters.data_ptr(), None, _lib.stream_of(DEV))

    ok = _cfg("MS").c_struct(False)
    assert call(g, ok) == _lib.NLDPC_OK
    assert np.array_equal(iters.cpu().numpy(), _expected("z16", "MS", "fused")[1])  # (unsat NULL: iters still filled)
    bad = [(_cfg("MS").c_struct(True), T, g), (_cfg("MS", first_iter=2).c_struct(False), T, g), (ok, 65, g),
           (_cfg("MS", path="stream").c_struct(False), T, g), (_cfg("MS", ucn=True).c_struct(False), T, g),
           (ok, T, LiftedGraph(BG2, 8))]  # (z=8: no compiled kernel)
    for c, t, graph in bad:
        assert call(graph, c, t) == _lib.NLDPC_EUNSUPPORTED
        assert L.nldpc_last_error().decode().startswith("nldpc_forward_early_stop:")
