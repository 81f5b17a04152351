"""Weight gradients of decode_backward against the CPU oracle's autograd: every quantiser, both paths.

The device side is decode(save=True) + decode_backward, as test_fused_backward_equals_stream drives it; the
oracle side is boosted_forward / neural_forward with requires_grad weights.  The objective is
sum_t (out_t * gy_t).sum(), so gy is the seed on both sides.  In every case the forward outputs are
bit-exact (SP: sp_check) and every gradient tensor (one iteration's weights) obeys

    |dev - ref| <= 1e-4 * |ref| + a * max|ref|

The relative part is the project's parity figure.  `a` is not the device's own error: it is 16 * s, capped
at 1e-4, where s is the oracle's own reduction noise, measured on the CPU as the largest max|delta| / max|g|
between any two of four orders of the oracle's autograd on the same case (the batch as given, reversed, and
two random orders whose lifted copies are also rotated by 5 and by Z // 2 + 1 -- a quasi-cyclic code maps
onto itself under a common rotation, so these reorder the sums over the Z copies too; each gradient seed
stays with its codeword).  The message chain is bit-identical on both sides, only the order of the sums
over the B * Z copies differs (autograd: ATen's sum; device: wave / tree / atomic order), and the factor 16
covers that.  Measured s per case (CASE_S is read from this table; a = min(16 s, 1e-4); a case whose four
orders agreed to the last bit has s = 0, and its bound is the relative part alone):

    kind      weights  Z    gauss/dense  gauss/single  edge/dense   edge/single
    qms6      edge     16      2.36e-07     1.35e-07     3.29e-07     1.23e-07
    qms6      edge     384     2.01e-07     2.37e-07     2.71e-07     2.13e-07
    qms6      tied     16      1.03e-06     0.00e+00     1.19e-05     0.00e+00
    qms6      tied     384     9.89e-07     2.32e-07     5.53e-07     3.11e-07
    qms5      edge     16      2.23e-07     1.25e-07     2.45e-07     1.48e-07
    qms5      edge     384     2.35e-07     1.47e-07     5.40e-07     2.19e-07
    qms5      tied     16      1.60e-06     0.00e+00     2.47e-06     1.70e-07
    qms5      tied     384     4.30e-07     1.03e-06     3.92e-06     1.29e-06
    qmsm5     edge     16      5.34e-07     7.65e-08     3.05e-07     1.94e-07
    qmsm5     edge     384     2.09e-07     1.82e-07     1.93e-07     1.83e-07
    qmsm5     tied     16      8.35e-07     0.00e+00     4.68e-07     0.00e+00
    qmsm5     tied     384     4.47e-07     4.78e-05     8.62e-07     6.61e-07
    qms4      edge     16      2.80e-07     1.63e-07     2.18e-07     1.76e-07
    qms4      edge     384     2.62e-07     2.09e-07     1.94e-07     2.02e-07
    qms4      tied     16      7.29e-07     0.00e+00     6.39e-07     0.00e+00
    qms4      tied     384     2.17e-06     5.23e-05     7.55e-07     4.87e-06
    qms3      edge     16      3.58e-07     1.12e-07     2.79e-07     1.42e-07
    qms3      edge     384     2.13e-07     3.09e-07     2.71e-07     2.46e-07
    qms3      tied     16      2.04e-06     1.08e-08     4.74e-06     0.00e+00
    qms3      tied     384     1.08e-06     1.14e-05     6.68e-07     2.61e-07
    ms        edge     16      2.42e-07     1.05e-07     2.46e-07     1.26e-07
    ms        edge     384     2.27e-07     2.36e-07     2.53e-07     1.76e-07
    ms        tied     16      5.35e-06     2.14e-07     1.66e-06     8.08e-08
    ms        tied     384     4.11e-07     1.82e-06     7.77e-06     7.67e-06
    sp        edge     16      2.94e-07     1.59e-07     3.61e-07     9.40e-08
    sp        edge     384     2.68e-07     2.37e-07     2.45e-07     2.26e-07
    neural    edge     16      1.95e-07     1.72e-07     2.33e-07     1.40e-07
    neural    edge     384     2.51e-07     2.23e-07     2.16e-07     2.27e-07
    ms_ucn    edge     16      2.28e-07     1.34e-07     4.31e-07     1.38e-07
    ms_ucn    edge     384     2.05e-07     2.24e-07     2.13e-07     2.19e-07
    qms6_ucn  edge     16      2.55e-07     1.42e-07     2.46e-07     1.33e-07
    qms6_ucn  edge     384     2.54e-07     2.18e-07     4.16e-07     1.96e-07

Cases.  Kinds: QMS q = 6, 5, -5, 4, 3; MS; SP; Neural; UCN (1,1,2) for MS and QMS q=6 (streaming backward only).
Weights: per-edge CN + cumulative per-column VN ("edge"), or one CN weight per iteration passed as a stride-0
expand with cn_tied=True ("tied": every iteration's row sum against the oracle's sharing-3 scalar gradient).
Sizes: BG2 z=16 B=19 T=5 (one full workgroup of 16 codewords and a partial one), BG2 z=384 B=2 T=4.
Inputs: the suite's Gaussian draw ("gauss") and the special-value batch of tests/edge_inputs.py ("edge":
all six special codewords at z=16; at z=384, where B=2, the integer-grid and the +-20 codewords, the two whose
ties and closed-interval boundary decide the backward routing), with the zero / negative weights of that
module (tied: [0.5, 1.5)).  Seeds: a dense gy, and gy nonzero for one codeword at the last iteration only
("single": max|ref| is then that codeword's own scale, so an edge that gets another edge's gradient shows).

Findings of this module.
  * SP: the backward evaluated 1 - t^2 of the tanh derivative with two roundings where ATen's tanh_backward
    uses one (a fused multiply-add); with t near +-1 single entries were off by up to 1e-2 relative
    (6.6e-5 of max|ref|).  Fixed in cn_backward (nldpc_node.h); all 16 SP cases hold the bound since.
  * MS with a tied CN weight on the register-resident backward ([ms-tied-16-fused-gauss-dense],
    [ms-tied-384-fused-gauss-dense]): z=16 iteration 0's row sum was -0.2673353 against the oracle's
    -0.6238457 (untied fused and streaming: -0.6238438), w_vn of iterations 0 and 1 off by 9.1e-2 and 4.4e-2
    of max|ref|; z=384: 20.4489117 against 20.4473648.  One codeword at a time (B=1 on both sides) it was
    codewords 3 and 16 of the z=16 batch and codeword 0 at z=384, and only what the check node of iteration 1
    hands back to the variable nodes (dL/dv2c).  Cause: a check copy whose smallest |input| lies in (0, 1e-4)
    -- a continuous MS input; no quantiser's code value -- gets the NEGATIVE magnitude min - 1e-4 from the
    reference's zero-fix correction, so the message's sign is opposite to the sign product; the tied check
    node (cn_bwd_ms, NLDPC_CNB_SPARSE) dropped the factor (s * sgn) = -1 that routes the gradient to the
    argmins, which is only an identity for QMS.  Fixed there; QMS keeps the short form.
"""
import functools
import os

import numpy as np
import pytest
import torch

import edge_inputs as ei
from conftest import ROOT

pytestmark = pytest.mark.gpu

BG2 = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
SP, MS, QMS, NEURAL = 0, 1, 2, 3
SIZES = {16: (19, 5), 384: (2, 4)}  # Z -> (B, T)
EDGE_ROWS = {16: None, 384: (2, 3)}  # special codewords of the "edge" input (None: all six)
SINGLE = {16: 2, 384: 0}  # the codeword of the "single" seed: the integer-grid one of the "edge" input
INPUTS = ("gauss", "edge")
SEEDS = ("dense", "single")

# kind tag -> (decoder kind, qbit, UCN)
KINDS = {"qms6": (QMS, 6, False), "qms5": (QMS, 5, False), "qmsm5": (QMS, -5, False), "qms4": (QMS, 4, False),
         "qms3": (QMS, 3, False), "ms": (MS, 5, False), "sp": (SP, 5, False), "neural": (NEURAL, 5, False),
         "ms_ucn": (MS, 5, True), "qms6_ucn": (QMS, 6, True)}
WMODES = {"qms6": ("edge", "tied"), "qms5": ("edge", "tied"), "qmsm5": ("edge", "tied"), "qms4": ("edge", "tied"),
          "qms3": ("edge", "tied"), "ms": ("edge", "tied"), "sp": ("edge",), "neural": ("edge",),
          "ms_ucn": ("edge",), "qms6_ucn": ("edge",)}
CASES = [(k, w, Z) for k in KINDS for w in WMODES[k] for Z in (16, 384)]
# (the register-resident backward does not cover UCN: those cases run on the streaming backward only)
RUNS = [(k, w, Z, p) for k, w, Z in CASES for p in ("stream", "fused") if not (KINDS[k][2] and p == "fused")]

# s per (kind tag, weights, Z) -> (gauss/dense, gauss/single, edge/dense, edge/single): the docstring's table
CASE_S = {(r[0], r[1], int(r[2])): tuple(float(v) for v in r[3:7])
          for r in (line.split() for line in __doc__.splitlines()) if len(r) == 7 and r[0] in KINDS}
assert len(CASE_S) == len(CASES)


def tolerance_a(tag, wmode, Z, inp, seed):
    s = CASE_S[tag, wmode, Z][2 * INPUTS.index(inp) + SEEDS.index(seed)]
    return min(16.0 * s, 1e-4)


def build_case(tag, wmode, Z, inp):
    """(x [B, N, Z], weights dict of [T, .] tensors, {seed: gy [T, B, N*Z]}), all on the CPU."""
    from oracle.ldpc_oracle import OracleGraph, quantize
    kind, q, ucn = KINDS[tag]
    B, T = SIZES[Z]
    og = OracleGraph(BG2, Z)
    N, E = og.N, og.E
    gen = torch.Generator().manual_seed(1000 * list(KINDS).index(tag) + 10 * Z + INPUTS.index(inp)
                                        + (5 if wmode == "tied" else 0))
    x = ei.gaussian_llr(B, N, Z, 77 + Z) if inp == "gauss" else ei.edge_batch(B, N, Z, rows=EDGE_ROWS[Z])
    if kind == QMS:
        x = quantize(x, q)
    if kind == NEURAL:
        if inp == "gauss":
            kw = dict(w_cn=torch.rand(T, E, generator=gen) * 1.2, bias=torch.randn(T, E, generator=gen) * 0.1)
        else:
            kw = dict(zip(("w_cn", "bias"), ei.edge_neural_params(T, E)))
    else:
        if wmode == "tied":
            kw = dict(w_cn=0.5 + torch.rand(T, 1, generator=gen))
        elif inp == "gauss":
            kw = dict(w_cn=0.5 + torch.rand(T, E, generator=gen))
        else:
            kw = dict(w_cn=ei.edge_cn_weights(T, E))
        if ucn:
            kw["w_ucn"] = (0.3 + torch.rand(T, E, generator=gen)) if inp == "gauss" else ei.edge_cn_weights(
                T, E, ei.SEED + 1)
        kw["w_vn"] = (0.8 + 0.4 * torch.rand(T, N, generator=gen)) if inp == "gauss" else ei.edge_vn_weights(T, N)
    dense = torch.randn(T, B, N * Z, generator=gen) * 1e-2
    single = torch.zeros(T, B, N * Z)
    single[T - 1, SINGLE[Z]] = torch.randn(N * Z, generator=gen) * 1e-2
    return x, kw, {"dense": dense, "single": single}


def oracle_grads(tag, wmode, Z, inp, perm=None, roll=0):
    """Oracle outputs [T, B, N*Z] and {seed: {weight name: gradient [T, .]}}.  perm / roll: another order of
    the same case (batch order perm, lifted copies rotated by roll; outputs are returned in the given order)."""
    from oracle.ldpc_oracle import OracleGraph, boosted_forward, neural_forward
    kind, q, ucn = KINDS[tag]
    B, T = SIZES[Z]
    og = OracleGraph(BG2, Z)
    x, kw, gys = build_case(tag, wmode, Z, inp)
    perm = torch.arange(B) if perm is None else torch.as_tensor(perm)
    xp = torch.roll(x[perm], roll, dims=2)
    P = {k: v.clone().requires_grad_(True) for k, v in kw.items()}
    if kind == NEURAL:
        outs = neural_forward(og, xp, list(P["w_cn"]), list(P["bias"]))
    else:
        r = boosted_forward(og, xp, dtype=kind, q=q, nw=(3 if wmode == "tied" else 1, 1 if ucn else 0, 2),
                            iters=list(range(T)), w_cn=lambda t: P["w_cn"][t],
                            w_ucn=lambda t: P["w_ucn"][t] if ucn else None, w_vn=lambda t: P["w_vn"][t])
        outs = [r[t] for t in range(T)]
    grads = {}
    for seed, gy in gys.items():
        gyp = torch.roll(gy[:, perm].reshape(T, B, og.N, Z), roll, dims=3).reshape(T, B, og.N * Z)
        obj = sum((outs[t] * gyp[t]).sum() for t in range(T))
        gs = torch.autograd.grad(obj, list(P.values()), retain_graph=True)
        grads[seed] = {k: g.detach() for k, g in zip(P, gs)}
    inv = torch.argsort(perm)
    o = torch.roll(torch.stack([o.detach() for o in outs]).reshape(T, B, og.N, Z), -roll, dims=3)[:, inv]
    return o.reshape(T, B, og.N * Z).numpy(), grads


def orders(Z):
    """The four orders of the reference's noise measurement: (perm, roll)."""
    B = SIZES[Z][0]
    r = np.random.default_rng(Z)
    return [(None, 0), (list(range(B - 1, -1, -1)), 0), (r.permutation(B).tolist(), 5),
            (r.permutation(B).tolist(), Z // 2 + 1)]


def per_tensor_ratio(d, g):
    """max over the iterations t of max|d_t| / max|g_t| (an iteration whose gradient is all zero: 0 or inf)."""
    d, g = d.reshape(d.shape[0], -1).abs().max(1)[0], g.reshape(g.shape[0], -1).abs().max(1)[0]
    r = torch.where(g > 0, d / g.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")),
                                                                torch.zeros_like(d)))
    return float(r.max())


@functools.lru_cache(maxsize=None)
def _reference(tag, wmode, Z, inp):
    return oracle_grads(tag, wmode, Z, inp)


@functools.lru_cache(maxsize=None)
def _graph(Z):
    from nldpc.graph import LiftedGraph
    return LiftedGraph(BG2, Z)


def _assert_grad(dev, ref, a, what, rounding=None):
    """Per iteration t: |dev_t - ref_t| <= 1e-4 |ref_t| + a max|ref_t| (+ rounding[t], see the tied case)."""
    dev, ref = dev.double().reshape(ref.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    for t in range(ref.shape[0]):
        m = float(ref[t].abs().max())
        excess = (dev[t] - ref[t]).abs() - (1e-4 * ref[t].abs() + a * m + (0.0 if rounding is None else float(rounding[t])))
        k = int(excess.argmax())
        print(f"{what} t={t}: max|d|/max|ref| = {float((dev[t] - ref[t]).abs().max()) / max(m, 1e-300):.3e} (a = {a:.2e})")
        assert float(excess[k]) <= 0, (f"{what}, iteration {t}: {int((excess > 0).sum())} of {excess.numel()} entries "
                                       f"beyond the bound; worst entry {k}: device {float(dev[t, k]):.9g}, oracle "
                                       f"{float(ref[t, k]):.9g}, max|oracle| {m:.9g}, a {a:.3g}")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("inp", INPUTS)
@pytest.mark.parametrize("tag,wmode,Z,path", RUNS)
def test_backward_matches_oracle_autograd(tag, wmode, Z, path, inp, seed):
    from nldpc.decode import DecodeCfg, decode, decode_backward
    kind, q, ucn = KINDS[tag]
    B, T = SIZES[Z]
    dev = torch.device("cuda")
    g = _graph(Z)
    x, kw, gys = build_case(tag, wmode, Z, inp)
    ref_outs, ref_grads = _reference(tag, wmode, Z, inp)
    ref = ref_grads[seed]
    tied = wmode == "tied"
    dkw = {k: v.to(dev) for k, v in kw.items()}
    if tied:
        dkw["w_cn"] = dkw["w_cn"].expand(T, g.E)  # stride 0 along the edges: what the tied flag is honoured for
    cfg = DecodeCfg(kind, qbit=q, ucn=ucn, vn_cumulative=kind != NEURAL, path=path, cn_tied=tied)
    outs, _, saved = decode(g, cfg, x.to(dev), T, save=True, **dkw)
    o = outs.cpu().numpy()
    if kind == SP:
        from test_gpu_forward import sp_check
        sp_check(o, ref_outs)
    else:
        assert np.array_equal(o, ref_outs), f"forward: per codeword {ei.per_codeword_diff(o, ref_outs)}"
    gy = [t.to(dev) for t in gys[seed]]
    need = (True, ucn, kind == NEURAL, kind != NEURAL)
    g_cn, g_ucn, g_b, g_vn, _ = decode_backward(g, cfg, x.to(dev), T, gy, list(outs.unbind(0)), saved, need=need, **dkw)
    a = tolerance_a(tag, wmode, Z, inp, seed)
    what = f"{tag} {wmode} z={Z} {path} {inp} {seed}"
    g_cn = g_cn.cpu()
    if tied:
        # the row sum is taken here, in fp64, of E entries that the device has already rounded to fp32: each carries
        # up to half an ulp, 2^-24 |entry|, which the sum cannot shed (seen: entries +-k * 0.00272 that cancel to an
        # exact 0 in the oracle's scalar gradient and to -1.2e-9 as rounded fp32 entries).  That rounding is the
        # comparison's own, so it is allowed on top: 2^-24 * sum |entry|
        _assert_grad(g_cn.double().sum(1, keepdim=True), ref["w_cn"], a, what + " w_cn (row sum)",
                     rounding=2.0 ** -24 * g_cn.double().abs().sum(1))
    else:
        _assert_grad(g_cn, ref["w_cn"], a, what + " w_cn")
    if ucn:
        _assert_grad(g_ucn.cpu(), ref["w_ucn"], a, what + " w_ucn")
    if kind == NEURAL:
        _assert_grad(g_b.cpu(), ref["bias"], a, what + " bias")
    else:
        _assert_grad(g_vn.cpu(), ref["w_vn"], a, what + " w_vn")
