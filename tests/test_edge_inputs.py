"""The special-value batch of tests/edge_inputs.py really reaches the special cases (CPU, oracle only).

The GPU tests that use the batch (test_gpu_edge_values.py, test_gpu_grad_oracle.py) are only as good as
the batch: a later edit of the builder, or of its seed, could lose the ties or the zeros without any of
them failing.  Here the oracle runs on the batch at BG2 z=16, T=4 and its coverage counters
(oracle/ldpc_oracle.py, `probe`) must all be positive for every decoder kind they apply to.
"""
import os

import numpy as np
import pytest
import torch

import edge_inputs as ei
from conftest import ROOT
from oracle.ldpc_oracle import OracleGraph, boosted_forward, neural_forward, quantize

BG2 = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
Z, T, B = 16, 4, 6


def test_edge_batch_properties():
    x = ei.edge_batch(19, 52, Z)
    plain = ei.gaussian_llr(19, 52, Z, ei.SEED)
    assert not x[0].any()
    assert not x[1, :2].any() and x[1, 2:].all()
    assert torch.equal(x[2], torch.round(x[2])) and (x[2] == 0).any()
    assert torch.equal(x[3].abs(), torch.full_like(x[3], 20.0)) and torch.equal(x[3] > 0, plain[3] > 0)
    assert (x[4].abs() > 20).any() and torch.equal(x[4], 10 * plain[4])
    assert torch.signbit(x[5, :, 1::2]).all() and not x[5, :, 1::2].any() and x[5, :, 0::2].all()
    assert torch.equal(x[6:], plain[6:]) and x[6:].all()
    w = ei.edge_cn_weights(T, 197)
    n = T * 197  # (an entry that is both a 7th and an 11th is -0.0: a zero, not a negative)
    assert (w == 0).sum() >= n // 7 and (w < 0).sum() >= n // 11 - n // 77 - 2 and torch.signbit(w[w == 0]).any()
    nw, nb = ei.edge_neural_params(T, 197)
    assert (nw == 0).any() and (nw < 0).any() and (nb == -0.5).sum() >= T * 197 // 5


@pytest.mark.parametrize("kind,q", [("neural", 0), ("ms", 5), ("sp", 5), ("qms", 5), ("qms", 6), ("qms", -5),
                                    ("qms", 4), ("qms", 3)])
def test_edge_batch_reaches_the_special_cases(kind, q):
    g = OracleGraph(BG2, Z)
    x = ei.edge_batch(B, g.N, Z)
    probe = {}
    if kind == "neural":
        w, b = ei.edge_neural_params(T, g.E)
        neural_forward(g, x, list(w), list(b), probe=probe)
        want = ("cn_tied_minima", "cn_zero_inputs", "relu_killed")
    else:
        dtype = {"sp": 0, "ms": 1, "qms": 2}[kind]
        if dtype == 2:
            x = quantize(x, q)
        wc, wv = ei.edge_cn_weights(T, g.E), ei.edge_vn_weights(T, g.N)
        outs = boosted_forward(g, x, dtype=dtype, q=q, nw=(1, 0, 2), iters=list(range(T)), w_cn=lambda t: wc[t],
                               w_ucn=lambda t: None, w_vn=lambda t: wv[t], probe=probe)
        want = ("cn_zero_inputs", "relu_killed", "posterior_at_clamp") + (("sp_clipped",) if dtype == 0 else
                                                                          ("cn_tied_minima",))
        assert probe["posterior_at_clamp"] == sum(int((outs[t].abs() == 20).sum()) for t in range(T))
    for k in want:
        assert probe.get(k, 0) > 0, f"{kind} q={q}: the batch no longer reaches '{k}' ({probe})"
