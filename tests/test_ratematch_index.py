"""The rate-matching index map (nldpc_rm_index, nldpc.ratematch.index), nldpc_rm_k0 and the argument rules, without a
GPU.  The expected index is the sequential loop of TS 38.212 §5.4.2 (ratematch_model.model_index); the library computes
it with the closed-form functions its kernels use (csrc/nldpc_rm_index.h), walking and seeking as they do.

The grid crosses, for BG2 and WiMAX at Z in {2, 3, 13, 16} with punct_cols in {0, 2}:
  F     0, 1, Z + 1, (K - punct_cols) * Z - 1
  ncb   full, K*Z - P + 3, full - 5
  k0    0, f0 - 1, f0, strictly inside the filler range, f1, Ncb - 1 (those that exist and differ)
  qm    1, 2, 6
  E     qm, the largest multiple of qm below Nv, Nv (the multiple of qm at or above it), and the first multiple of qm
        above 2 * Nv that leaves a remainder
Z = 2 and 3 run the whole cross; Z = 13 and 16 run every fifth set of it (5 is coprime to the inner counts, so every
corner value still occurs with every graph, Z and punct_cols).
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from ratematch_model import model_index

RES = os.path.join(ROOT, "resources")
BG2 = np.loadtxt(os.path.join(RES, "basegraph2_set0.txt"), int, delimiter="\t")
WIMAX = np.loadtxt(os.path.join(RES, "wman_N0576_R34_z24.txt"), int, delimiter="\t")
GRAPHS = {"bg2": BG2, "wimax": WIMAX}


def _graph(name, Z):
    from nldpc.graph import LiftedGraph
    return LiftedGraph(GRAPHS[name], Z)


def grid(M, N, Z, pc):
    K = N - M
    P, full = pc * Z, N * Z - pc * Z
    for F in (0, 1, Z + 1, (K - pc) * Z - 1):
        f0, f1 = K * Z - F - P, K * Z - P
        for ncb in (0, K * Z - P + 3, full - 5):
            Ncb = ncb or full
            Nv = Ncb - F
            k0s = [0, f0 - 1, f0, f1, Ncb - 1] + ([f0 + F // 2] if F >= 2 else [])
            for k0 in sorted({k for k in k0s if 0 <= k < Ncb}):
                for qm in (1, 2, 6):
                    below = (Nv - 1) // qm * qm
                    above = (2 * Nv) // qm * qm + qm
                    while above % Nv == 0:
                        above += qm
                    for E in sorted({qm, below, -(-Nv // qm) * qm, above} - {0}):
                        yield dict(E=E, k0=k0, punct_cols=pc, n_filler=F, ncb=ncb, qm=qm)


@pytest.mark.parametrize("pc", [0, 2])
@pytest.mark.parametrize("Z", [2, 3, 13, 16])
@pytest.mark.parametrize("name", ["bg2", "wimax"])
def test_index_equals_the_sequential_loop(name, Z, pc):
    from nldpc.ratematch import RateMatch, index
    g = _graph(name, Z)
    seen = dict(F=set(), ncb=set(), qm=set(), k0=set(), E=set())
    n = 0
    for i, kw in enumerate(grid(g.M, g.N, Z, pc)):
        if Z >= 13 and i % 5:
            continue
        got = index(g, RateMatch(**kw))
        assert got.dtype == np.int32 and got.shape == (kw["E"],)
        want = model_index(g.M, g.N, Z, **kw)
        assert np.array_equal(got, want), kw
        # which corners this run met
        P, F = pc * Z, kw["n_filler"]
        Ncb = kw["ncb"] or g.N * Z - P
        f0, f1, Nv = g.K * Z - F - P, g.K * Z - P, Ncb - F
        seen["F"].add(F)
        seen["ncb"].add(kw["ncb"])
        seen["qm"].add(kw["qm"])
        seen["k0"] |= {c for c, v in (("0", 0), ("f0-1", f0 - 1), ("f0", f0), ("f1", f1), ("last", Ncb - 1))
                       if kw["k0"] == v} | ({"inside"} if f0 < kw["k0"] < f1 else set())
        seen["E"] |= {c for c, ok in (("qm", kw["E"] == kw["qm"]), ("<Nv", kw["E"] < Nv), ("=Nv", kw["E"] == Nv),
                                      (">2Nv", kw["E"] > 2 * Nv and kw["E"] % Nv)) if ok}
        n += 1
    K = g.K
    assert seen["F"] == {0, 1, Z + 1, (K - pc) * Z - 1}
    assert seen["ncb"] == {0, K * Z - pc * Z + 3, g.N * Z - pc * Z - 5}
    assert seen["qm"] == {1, 2, 6}
    assert seen["k0"] == {"0", "f0-1", "f0", "inside", "f1", "last"}
    assert seen["E"] == {"qm", "<Nv", "=Nv", ">2Nv"}
    assert n >= 100


K0_PINNED = [(2, 800, [0, 208, 400, 688]), (2, 600, [0, 144, 288, 512]), (1, 1056, [0, 272, 528, 896])]


@pytest.mark.parametrize("bg,ncb,want", K0_PINNED)
def test_rm_k0_pinned(bg, ncb, want):
    from nldpc import _lib
    for rv in range(4):
        k0 = ctypes.c_int64(-1)
        assert _lib.lib().nldpc_rm_k0(bg, rv, ncb, 16, ctypes.byref(k0)) == _lib.NLDPC_OK
        assert k0.value == want[rv]


def test_nr5g_resolves_k0():
    from nldpc.graph import LiftedGraph
    from nldpc.ratematch import RateMatch
    g2 = _graph("bg2", 16)  # full buffer: 52 * 16 - 32 = 800
    for rv, k0 in enumerate([0, 208, 400, 688]):
        rm = RateMatch.nr5g(g2, 272, rv=rv, n_filler=24, qm=2)
        assert rm == RateMatch(E=272, k0=k0, punct_cols=2, n_filler=24, ncb=0, qm=2)
    for rv, k0 in enumerate([0, 144, 288, 512]):
        assert RateMatch.nr5g(g2, 100, rv=rv, ncb=600) == RateMatch(E=100, k0=k0, punct_cols=2, ncb=600)
    g1 = LiftedGraph(np.zeros((46, 68), int), 16)  # BG1's dimensions: 68 * 16 - 32 = 1056
    for rv, k0 in enumerate([0, 272, 528, 896]):
        assert RateMatch.nr5g(g1, 100, bg=1, rv=rv).k0 == k0


def test_k0_rejects_unknown_bg_and_rv():
    from nldpc import _lib
    from nldpc.ratematch import RateMatch
    k0 = ctypes.c_int64()
    L = _lib.lib()
    assert L.nldpc_rm_k0(3, 0, 800, 16, ctypes.byref(k0)) == _lib.NLDPC_EINVAL
    assert L.nldpc_rm_k0(2, 4, 800, 16, ctypes.byref(k0)) == _lib.NLDPC_EINVAL
    assert L.nldpc_rm_k0(2, -1, 800, 16, ctypes.byref(k0)) == _lib.NLDPC_EINVAL
    assert L.nldpc_rm_k0(2, 0, 0, 16, ctypes.byref(k0)) == _lib.NLDPC_EINVAL
    assert L.nldpc_rm_k0(2, 0, 800, 16, None) == _lib.NLDPC_EINVAL
    with pytest.raises(ValueError):
        RateMatch.nr5g(_graph("bg2", 16), 272, bg=3)
    with pytest.raises(ValueError):
        RateMatch.nr5g(_graph("bg2", 16), 272, rv=4)


# BG2 z=16: K = 10, K*Z = 160, N*Z = 832; with punct_cols = 2: P = 32, full buffer 800
RULES = {
    "punct_cols_negative": dict(E=10, punct_cols=-1),
    "punct_cols_above_K": dict(E=10, punct_cols=11),
    "filler_negative": dict(E=10, punct_cols=2, n_filler=-1),
    "filler_above_info": dict(E=10, punct_cols=2, n_filler=129),
    "ncb_below_systematic": dict(E=10, punct_cols=2, ncb=127),
    "ncb_above_full": dict(E=10, punct_cols=2, ncb=801),
    "no_valid_position": dict(E=10, punct_cols=0, n_filler=160, ncb=160),
    "k0_negative": dict(E=10, punct_cols=2, k0=-1),
    "k0_at_ncb": dict(E=10, punct_cols=2, k0=800),
    "k0_at_limited_ncb": dict(E=10, punct_cols=2, ncb=600, k0=600),
    "E_zero": dict(E=0),
    "qm_zero": dict(E=10, qm=0),
    "qm_not_dividing_E": dict(E=10, qm=6),
    "E_2_31": dict(E=2 ** 31),
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_rule_raises_value_error(rule):
    from nldpc.ratematch import RateMatch, index
    with pytest.raises(ValueError):
        index(_graph("bg2", 16), RateMatch(**RULES[rule]))


def test_rules_accept_their_boundaries():
    from nldpc.ratematch import RateMatch, index
    g = _graph("bg2", 16)
    for kw in (dict(E=10, punct_cols=10), dict(E=10, punct_cols=2, n_filler=128), dict(E=10, punct_cols=2, ncb=128),
               dict(E=10, punct_cols=2, ncb=800, k0=799), dict(E=12, qm=6), dict(E=6, qm=6),
               dict(E=1, punct_cols=0, n_filler=159, ncb=160)):
        assert len(index(g, RateMatch(**kw))) == kw["E"]


def test_codeword_of_2_31_bits_is_rejected():
    from nldpc.ratematch import RateMatch, index
    with pytest.raises(ValueError):
        index(_graph("bg2", 2 ** 26), RateMatch(E=10))  # N*Z = 52 * 2^26 >= 2^31


def test_null_pointers_are_rejected():
    from nldpc import _lib
    L = _lib.lib()
    rm = _lib.NldpcRm(0, 1, 0, 0, 0, 10)
    idx = (ctypes.c_int32 * 10)()
    assert L.nldpc_rm_index(42, 52, 16, ctypes.byref(rm), idx) == _lib.NLDPC_OK
    assert L.nldpc_rm_index(42, 52, 16, None, idx) == _lib.NLDPC_EINVAL
    assert L.nldpc_rm_index(42, 52, 16, ctypes.byref(rm), None) == _lib.NLDPC_EINVAL
    assert L.nldpc_rate_match(None, ctypes.byref(rm), None, 1, None, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_rate_recover(None, ctypes.byref(rm), None, 1, 0.0, -20.0, 0.0, 0, None, None) == _lib.NLDPC_EINVAL


def test_rm_struct_layout_matches_header():
    import re
    from nldpc import _lib
    src = open(os.path.join(ROOT, "include", "nldpc.h")).read()
    body = re.search(r"typedef struct nldpc_rm \{(.*?)\} nldpc_rm;", src, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|int64_t)\s+(\w+);", body, re.M)
    assert [f for _, f in fields] == [f for f, _ in _lib.NldpcRm._fields_]
    assert ctypes.sizeof(_lib.NldpcRm) == sum(4 if t == "int32_t" else 8 for t, _ in fields) == 40


def test_code_rate():
    from nldpc.ratematch import RateMatch, code_rate
    assert code_rate(_graph("bg2", 16), RateMatch(E=272, punct_cols=2, n_filler=24)) == 0.5
