"""The on-device systematic encoder (nldpc_encode, nldpc.channel.encode) on the GPU.

Expected values never come from the encoder: a codeword must carry its info bits in the first K*Z positions and have
zero syndrome (numpy restatement of test_early_stop_gen.py, and the device syndrome kernel) -- which determines it --,
at BG2 z=16 it must equal info @ GEN16 % 2 (the reference's generator matrix), and the drawn info bits must equal the
host Philox restatement (oracle/philox.py) of the stream include/nldpc.h states.

Shapes: the smallest at which the kernel can go wrong -- many codewords per workgroup with an odd remainder (z=2), a
lifting size below a wave and odd (z=13), small Z with odd B (z=16), a size no kernel is built for (z=52), the headline
graph (z=384, one codeword per workgroup), and the second base graph (WiMAX z=24).
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle.philox import philox4x32_10
from test_early_stop_gen import unsat_numpy

pytestmark = pytest.mark.gpu

RES = os.path.join(ROOT, "resources")
BG2 = np.loadtxt(os.path.join(RES, "basegraph2_set0.txt"), int, delimiter="\t")
WIMAX = np.loadtxt(os.path.join(RES, "wman_N0576_R34_z24.txt"), int, delimiter="\t")
GEN16 = np.loadtxt(os.path.join(RES, "gen_matrix_bg2_z16.txt"), int, delimiter=",")
NO_PLAN = np.array([[1, 2, 0, 1], [3, 0, 2, 0]])
GRAPHS = {"bg2": BG2, "wimax": WIMAX}
DEV = torch.device("cuda")
ENC_TAG = 0x454E4331

SHAPES = [("bg2", 2, 130), ("bg2", 13, 5), ("bg2", 16, 37), ("bg2", 52, 3), ("bg2", 384, 3), ("wimax", 24, 29)]


@functools.lru_cache(maxsize=None)
def _graph(name, Z):
    from nldpc.graph import LiftedGraph
    return LiftedGraph(GRAPHS[name], Z)


def _info(name, Z, B, seed=0):
    hb = GRAPHS[name]
    return np.random.default_rng(1000 * Z + B + seed).integers(0, 2, size=(B, (hb.shape[1] - hb.shape[0]) * Z))


def philox_info(B, KZ, seed, b_offset=0):
    """Host restatement of the info bits nldpc_encode draws with info == NULL."""
    W = -(-KZ // 128)
    idx = ((np.arange(b_offset, b_offset + B, dtype=np.uint64)[:, None] * np.uint64(W)) +
           np.arange(W, dtype=np.uint64)[None, :]).reshape(-1)
    ctr = np.zeros((len(idx), 4), dtype=np.uint32)
    ctr[:, 0] = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (idx >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = ENC_TAG
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(B, 4 * W)
    i = np.arange(KZ)
    return ((words[:, i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(np.int64)


def _check_codewords(y, info, name, Z):
    from nldpc.channel import syndrome_weight
    hb = GRAPHS[name]
    KZ = (hb.shape[1] - hb.shape[0]) * Z
    assert y.dtype == torch.uint8 and tuple(y.shape) == (info.shape[0], hb.shape[1] * Z)
    yh = y.cpu().numpy()
    assert yh.max() <= 1
    assert np.array_equal(yh[:, :KZ], info)
    assert not unsat_numpy(yh, hb, Z).any()
    assert not syndrome_weight(2.0 * y.float() - 1.0, _graph(name, Z)).cpu().numpy().any()
    if name == "bg2" and Z == 16:
        assert np.array_equal(yh, info @ GEN16 % 2)


@pytest.mark.parametrize("name,Z,B", SHAPES)
def test_given_info(name, Z, B):
    from nldpc.channel import encode
    info = _info(name, Z, B)
    info[0] = 0
    info[-1] = 1
    for dtype in (torch.uint8, torch.float32):
        y = encode(_graph(name, Z), torch.from_numpy(info).to(DEV).to(dtype))
        _check_codewords(y, info, name, Z)


@pytest.mark.parametrize("name,Z,B", SHAPES)
def test_philox_info(name, Z, B):
    from nldpc.channel import encode
    g = _graph(name, Z)
    y = encode(g, B=B, seed=77, device=DEV)
    want = philox_info(B, g.K * Z, 77)
    assert 0.3 < want.mean() < 0.7
    _check_codewords(y, want, name, Z)


def test_nonzero_info_bytes_count_as_one():
    from nldpc.channel import encode
    g = _graph("bg2", 16)
    info = _info("bg2", 16, 9)
    vals = np.array([1, 2, 255, 128, 17])
    raw = torch.from_numpy((info * vals[np.arange(info.size).reshape(info.shape) % 5]).astype(np.uint8))
    assert set(raw.unique().tolist()) == {0, 1, 2, 17, 128, 255}
    y = encode(g, raw.to(DEV))
    assert np.array_equal(y.cpu().numpy(), info @ GEN16 % 2)


@pytest.mark.parametrize("name,Z,B", [("bg2", 13, 5), ("wimax", 24, 29), ("bg2", 384, 3)])
def test_linearity(name, Z, B):
    from nldpc.channel import encode
    g = _graph(name, Z)
    a, b = _info(name, Z, B, 1), _info(name, Z, B, 2)
    enc = lambda v: encode(g, torch.from_numpy(v).to(DEV)).cpu().numpy()  # noqa: E731
    assert np.array_equal(enc(a ^ b), enc(a) ^ enc(b))


@pytest.mark.parametrize("name,Z,B", [("bg2", 2, 130), ("bg2", 13, 5), ("bg2", 16, 37), ("bg2", 384, 3)])
@pytest.mark.parametrize("shift", [0, 3])
def test_guard_row_untouched(name, Z, B, shift):
    """Nothing is written before y or after its last codeword, wherever y and info start (16-byte stores, 4-byte
    loads inside the kernel: `shift` moves both off their alignment)."""
    from nldpc.channel import encode
    g = _graph(name, Z)
    L, KZ = g.N * Z, g.K * Z
    info = _info(name, Z, B)
    buf = torch.full((shift + (B + 1) * L + 16,), 0xAA, dtype=torch.uint8, device=DEV)
    ibuf = torch.zeros((shift + B * KZ,), dtype=torch.uint8, device=DEV)
    ibuf[shift:] = torch.from_numpy(info).to(torch.uint8).reshape(-1).to(DEV)
    out = buf[shift:shift + B * L].view(B, L)
    y = encode(g, ibuf[shift:].view(B, KZ), out=out)
    assert y.data_ptr() == out.data_ptr()
    _check_codewords(y, info, name, Z)
    assert (buf[:shift] == 0xAA).all() and (buf[shift + B * L:] == 0xAA).all()
    buf.fill_(0xAA)
    encode(g, B=B, seed=5, out=out)
    _check_codewords(out, philox_info(B, KZ, 5), name, Z)
    assert (buf[:shift] == 0xAA).all() and (buf[shift + B * L:] == 0xAA).all()


@pytest.mark.parametrize("name,Z", [("bg2", 2), ("bg2", 16), ("bg2", 384)])
def test_sharded_batch_draws_the_same_words(name, Z):
    from nldpc.channel import encode
    g = _graph(name, Z)
    whole = encode(g, B=8, seed=2042, device=DEV)
    part = encode(g, B=5, seed=2042, b_offset=3, device=DEV)
    assert torch.equal(whole[3:], part)
    assert np.array_equal(part.cpu().numpy()[:, :g.K * Z], philox_info(5, g.K * Z, 2042, 3))
    other = encode(g, B=8, seed=2043, device=DEV)
    assert not torch.equal(other, whole)
    assert all(not torch.equal(other[b], whole[b]) for b in range(8))
    big = (1 << 63) + 12345  # a seed above 2^32 reaches both key words
    assert np.array_equal(encode(g, B=2, seed=big, device=DEV).cpu().numpy()[:, :g.K * Z], philox_info(2, g.K * Z, big))


def test_unsupported_graph_and_bad_arguments():
    from nldpc import _lib
    from nldpc.channel import encode
    from nldpc.graph import LiftedGraph
    g = LiftedGraph(NO_PLAN, 5)
    assert g.handle(DEV)  # creating the graph still succeeds
    with pytest.raises(_lib.NldpcUnsupported):
        encode(g, B=2, device=DEV)
    with pytest.raises(_lib.NldpcUnsupported):
        encode(g, torch.zeros((2, 10), dtype=torch.uint8, device=DEV))
    g16 = _graph("bg2", 16)
    with pytest.raises(ValueError):
        encode(g16, torch.zeros((2, 161), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        encode(g16)
    L = _lib.lib()
    y = torch.empty((1, 832), dtype=torch.uint8, device=DEV)
    assert L.nldpc_encode(g16.handle(DEV), None, 0, 1, 0, y.data_ptr(), None) == _lib.NLDPC_EINVAL
    assert L.nldpc_encode(g16.handle(DEV), None, 1, 1, 0, None, None) == _lib.NLDPC_EINVAL


def test_pipeline_z16_random_codewords_decode():
    """encode(info=None) -> awgn_llr(y=) -> decode at Eb/N0 = 12 dB (rate 0.2), Neural weights 0.5, bias 0, T=8, no
    puncturing.  On the CPU oracle with numpy noise all 64 random codewords were error-free from iteration 1 at 12 dB
    (from iteration 2 at 9 dB), so the last iteration has six iterations to spare."""
    import neural_ldpc_decoder as nd
    from nldpc.channel import awgn_llr, ber_counts, encode, sigma_for
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    g = _graph("bg2", 16)
    B, T = 64, 8
    y = encode(g, B=B, seed=2042, device=DEV)
    assert 0.4 < float(y.float().mean()) < 0.6
    xa = awgn_llr(B, g.N, 16, sigma_for(12.0, 0.2), seed=7, device=DEV, y=y)
    w, b = torch.full((T, g.E), 0.5, device=DEV), torch.zeros((T, g.E), device=DEV)
    outs, _, _ = decode(g, DecodeCfg(kind=KIND_NEURAL, keep_state=False), xa, T, w_cn=w, bias=b)
    counts = ber_counts(outs, y).cpu().numpy()
    print("bit / frame errors per iteration:", counts.tolist())
    assert counts[-1, 1] == 0 and counts[-1, 0] == 0
    want = [[int(((outs[t] > 0) != (y != 0)).sum()), int(((outs[t] > 0) != (y != 0)).any(1).sum())] for t in range(T)]
    assert counts.tolist() == want
    model = nd.NeuralLDPCDecoder(T, B, nd.ConnectingMatrixTorch(nd.ConnectingMatrix(16, BG2), device=DEV)).to(DEV)
    assert np.array_equal(model.count_errors(xa, y).cpu().numpy(), counts)
    # against the all-zero word the same posteriors are wrong in about half the positions
    assert ber_counts(outs, None).cpu().numpy()[-1, 1] == B


def test_pipeline_z384_count_errors_equals_ber_counts():
    """No absolute claim at this shape (nobody has decoded a random z=384 word before): the count-only decode and the
    counter over the written posteriors must agree on encoded codewords."""
    import neural_ldpc_decoder as nd
    from nldpc.channel import awgn_llr, ber_counts, encode, sigma_for
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    g = _graph("bg2", 384)
    B, T = 3, 8
    y = encode(g, B=B, seed=11, device=DEV)
    xa = awgn_llr(B, g.N, 384, sigma_for(3.0, 0.2), seed=7, device=DEV, y=y)
    w, b = torch.full((T, g.E), 0.5, device=DEV), torch.zeros((T, g.E), device=DEV)
    outs, _, _ = decode(g, DecodeCfg(kind=KIND_NEURAL, keep_state=False), xa, T, w_cn=w, bias=b)
    counts = ber_counts(outs, y).cpu().numpy()
    print("bit / frame errors per iteration:", counts.tolist())
    model = nd.NeuralLDPCDecoder(T, B, nd.ConnectingMatrixTorch(nd.ConnectingMatrix(384, BG2), device=DEV)).to(DEV)
    assert np.array_equal(model.count_errors(xa, y).cpu().numpy(), counts)
    assert counts[0, 0] > 0  # (3 dB: the first iteration still has bit errors, so the counts compare something)
