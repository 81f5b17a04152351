"""The systematic encoder's plan (nldpc_encode_plan, LiftedGraph.encode_plan) without a GPU.

The returned plan is executed in numpy, straight from the step semantics include/nldpc.h states, on random info bits.
Expected values never come from the encoder: the word must be systematic with zero syndrome (test_early_stop_gen's
unsat_numpy) -- which, the parity part being invertible wherever a plan exists, determines it uniquely -- and at BG2
z=16 it must equal info @ GEN16 % 2, the reference's generator matrix.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from test_early_stop_gen import unsat_numpy

RES = os.path.join(ROOT, "resources")
BG2 = np.loadtxt(os.path.join(RES, "basegraph2_set0.txt"), int, delimiter="\t")
WIMAX = np.loadtxt(os.path.join(RES, "wman_N0576_R34_z24.txt"), int, delimiter="\t")
GEN16 = np.loadtxt(os.path.join(RES, "gen_matrix_bg2_z16.txt"), int, delimiter=",")
NO_PLAN = np.array([[1, 2, 0, 1], [3, 0, 2, 0]])

CASES = [("bg2", Z) for Z in (2, 3, 13, 16, 52, 96, 384)] + [("wimax", Z) for Z in (5, 24, 96)]
GRAPHS = {"bg2": BG2, "wimax": WIMAX}


def run_plan(plan, info, hb, Z):
    """Codewords [B, N*Z] from info [B, K*Z]: the plan's steps in order, each for every check copy h."""
    M, N = hb.shape
    K = N - M
    y = np.zeros((info.shape[0], N, Z), dtype=np.int64)
    y[:, :K, :] = info.reshape(-1, K, Z)
    h = np.arange(Z)
    for s in range(M):
        acc = np.zeros((info.shape[0], Z), dtype=np.int64)
        for k in range(plan["step_ptr"][s], plan["step_ptr"][s + 1]):
            acc ^= y[:, plan["term_col"][k], (h + plan["term_shift"][k]) % Z]
        y[:, plan["step_col"][s], (h + plan["step_shift"][s]) % Z] = acc
    return y.reshape(info.shape[0], N * Z)


@pytest.mark.parametrize("name,Z", CASES)
def test_plan_gives_systematic_codewords(name, Z):
    from nldpc.graph import LiftedGraph
    hb = GRAPHS[name]
    M, N = hb.shape
    g = LiftedGraph(hb, Z)
    assert g.K == N - M
    plan = g.encode_plan()
    for key in ("step_col", "step_shift", "step_level", "step_ptr", "term_col", "term_shift"):
        assert isinstance(plan[key], np.ndarray) and plan[key].dtype == np.int32, key
    assert len(plan["step_col"]) == len(plan["step_shift"]) == len(plan["step_level"]) == M
    assert len(plan["step_ptr"]) == M + 1 and plan["step_ptr"][0] == 0
    assert len(plan["term_col"]) == len(plan["term_shift"]) == plan["step_ptr"][-1]
    assert (np.diff(plan["step_ptr"]) >= 0).all()
    # every parity column is the target of exactly one step; shifts are taken mod Z
    assert sorted(plan["step_col"].tolist()) == list(range(N - M, N))
    assert ((plan["step_shift"] >= 0) & (plan["step_shift"] < Z)).all()
    assert ((plan["term_shift"] >= 0) & (plan["term_shift"] < Z)).all()
    # levels: sorted, from 0, and every term is an info column or the target of a lower level
    lv = plan["step_level"]
    assert (np.diff(lv) >= 0).all() and lv[0] == 0 and plan["n_levels"] == lv[-1] + 1
    level_of = {int(c): int(l) for c, l in zip(plan["step_col"], lv)}
    for s in range(M):
        for k in range(plan["step_ptr"][s], plan["step_ptr"][s + 1]):
            c = int(plan["term_col"][k])
            assert 0 <= c < N
            assert c < N - M or level_of[c] < lv[s], (s, c)
    if name == "bg2":  # the 38 degree-1 columns run concurrently, after the 4 core columns
        deg1 = [j for j in range(N - M, N) if (hb[:, j] != -1).sum() == 1]
        assert len(deg1) == 38
        assert len({level_of[j] for j in deg1}) == 1
        assert all(level_of[j] < level_of[deg1[0]] for j in range(N - M, N) if j not in deg1)
    info = np.random.default_rng(100 + Z).integers(0, 2, size=(6, (N - M) * Z))
    y = run_plan(plan, info, hb, Z)
    assert np.array_equal(y[:, :(N - M) * Z], info)
    assert not unsat_numpy(y, hb, Z).any()
    assert set(np.unique(y)) <= {0, 1}


def test_bg2_z16_equals_the_generator_matrix():
    from nldpc.graph import LiftedGraph
    assert np.array_equal(GEN16[:, :160], np.eye(160, dtype=int))  # systematic, info columns first
    info = np.random.default_rng(3).integers(0, 2, size=(40, GEN16.shape[0]))
    info[0], info[1] = 0, 1
    y = run_plan(LiftedGraph(BG2, 16).encode_plan(), info, BG2, 16)
    assert np.array_equal(y, info @ GEN16 % 2)


def test_graph_without_a_plan_is_refused():
    """No row has a single unknown, and the row sum leaves two monomials in both parity columns."""
    from nldpc import _lib
    from nldpc.graph import LiftedGraph
    with pytest.raises(_lib.NldpcUnsupported):
        LiftedGraph(NO_PLAN, 5).encode_plan()
    with pytest.raises(NotImplementedError):  # (N <= M: no info columns)
        LiftedGraph(np.array([[0, 1], [1, 0]]), 5).encode_plan()


def _raw_plan(hb, Z, cap):
    from nldpc import _lib
    M, N = hb.shape
    tbl = np.ascontiguousarray(hb, dtype=np.int32)
    arr = lambda n: (ctypes.c_int32 * n)()  # noqa: E731
    out = [arr(M), arr(M), arr(M), arr(M + 1), arr(max(cap, 1)), arr(max(cap, 1))]
    nlev = ctypes.c_int32(-1)
    rc = _lib.lib().nldpc_encode_plan(M, N, Z, tbl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), *out, cap,
                                      ctypes.byref(nlev))
    return rc, out, nlev.value


def test_term_cap():
    from nldpc import _lib
    E = int((BG2 != -1).sum())
    rc, out, nlev = _raw_plan(BG2, 16, 2 * E)
    assert rc == _lib.NLDPC_OK and nlev >= 2
    n_terms = out[3][BG2.shape[0]]
    assert 0 < n_terms <= 2 * E
    assert _raw_plan(BG2, 16, n_terms)[0] == _lib.NLDPC_OK
    assert _raw_plan(BG2, 16, n_terms - 1)[0] == _lib.NLDPC_EINVAL
    assert b"term_cap" in _lib.lib().nldpc_last_error()
    assert _raw_plan(NO_PLAN, 5, 64)[0] == _lib.NLDPC_EUNSUPPORTED
    assert _lib.lib().nldpc_encode_plan(0, 4, 5, None, None, None, None, None, None, None, 0, None) == _lib.NLDPC_EINVAL
