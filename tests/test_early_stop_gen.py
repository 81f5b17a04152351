"""The early-stopping decode's generated unit (csrc/gen_fused.py, MODE 7, fused_<tag>_s7.hip) and the parity-check
arithmetic its tests rely on, without a GPU:

* --list names the unit for every built-in graph, and it cross-compiles for gfx950 (BG2 z=16: 16 codewords per
  workgroup, degree-1 columns; WiMAX z=24: 8 codewords, no degree-1 column);
* adding the MODE left every other generated unit of BG2 z=16 as it was (hashes of the generator's output before
  the MODE existed; fused_table.hip is not listed: the FusedSpec table gained the new kernels' entries);
* the edge-table form of the syndrome weight (check copy h of edge (i, j, s) reads variable copy (h + s) mod Z)
  equals the dense H . bits mod 2.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

CS = os.path.join(ROOT, "neural-ldpc-decoder-torch_amd", "csrc")
RES = os.path.join(ROOT, "resources")
HIPCC = "/opt/rocm/bin/hipcc"
TAGS = ("bg2_z384", "bg2_z16", "wimax_z24", "bg2_z96")

# sha256 of the BG2 z=16 units as the generator emitted them before the early-stop MODE was added
PARENT_SHA256 = {
    "fused_bg2_z16_s0.hip": "13cf8a5bf1007108022a5a0439d7a8352d1193413757f4611d963aab5ede7998",
    "fused_bg2_z16_s1.hip": "a8dce62afcdca89ea92867690038c22bae6b845efbcb862cc420b39f2078d72b",
    "fused_bg2_z16_s2.hip": "4247e852333a501df1142e2028866c9481baa374e3062a868ef7f5c8d81ac7b1",
    "fused_bg2_z16_s3.hip": "43a2e6b903726599764c22790ba154f4a4960fe6791ad9bd238241ec2e592a4c",
    "fused_bg2_z16_s0u.hip": "5d17bd2c4059fdd0a4e5ea68c39c31ede77c4d9ab99a4909ee41bcbc7f0aac57",
    "fused_bg2_z16_bwd.hip": "ccd26508edca1b127bf35ebc5d06da03505f7d4a2910557abf41f28f58f4920c",
}


def _clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith(("NLDPC_GEN_", "NLDPC_FUSED_"))}


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gen"))
    subprocess.run([sys.executable, os.path.join(CS, "gen_fused.py"), out, RES], env=_clean_env(), check=True,
                   capture_output=True)
    return out


def test_list_names_the_early_stop_unit():
    r = subprocess.run([sys.executable, os.path.join(CS, "gen_fused.py"), "--list"], env=_clean_env(), check=True,
                       capture_output=True, text=True)
    names = r.stdout.split()
    for tag in TAGS:
        assert f"fused_{tag}_s7.hip" in names, (tag, names)


def test_existing_units_unchanged(generated):
    for name, want in PARENT_SHA256.items():
        got = hashlib.sha256(open(os.path.join(generated, name), "rb").read()).hexdigest()
        assert got == want, name


def test_early_stop_unit_has_its_own_text(generated):
    """The unit instantiates MODE 7 of every kind, carries its own signature entry, and the table knows it."""
    for tag in TAGS:
        src = open(os.path.join(generated, f"fused_{tag}_s7.hip")).read()
        for k in range(4):
            assert f"fused_{tag}::kernel<{k}, 7>" in src
        assert f"fused_{tag}_sig_s7()" in src
        assert "es_stop == es_live" in src
    tab = open(os.path.join(generated, "fused_table.hip")).read()
    for tag in TAGS:
        assert f"fused_{tag}_kernel_s7(3)" in tab and f"fused_{tag}_sig_s7()" in tab


@pytest.mark.parametrize("tag", ["bg2_z16", "wimax_z24"])
def test_early_stop_unit_compiles(generated, tag, tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    unit = os.path.join(generated, f"fused_{tag}_s7.hip")
    co = str(tmp_path / (tag + ".co"))
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--genco", "-O1", "-std=c++17", "-ffp-contract=off",
                        "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"), "-I" + CS, "-x", "hip", unit, "-o", co],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.getsize(co) > 1000


def edge_tables(hb, Z):
    """C-order edges of a base graph: check row, variable column, shift mod Z (what nldpc_graph_edges returns)."""
    rows, cols = np.nonzero(hb != -1)
    return rows, cols, hb[rows, cols] % Z


def unsat_numpy(bits, hb, Z):
    """Syndrome weight of hard decisions bits [B, N*Z] from the edge tables."""
    M, N = hb.shape
    chk, var, shift = edge_tables(hb, Z)
    b3 = np.asarray(bits).reshape(-1, N, Z).astype(np.int64)
    par = np.zeros((b3.shape[0], M, Z), dtype=np.int64)
    h = np.arange(Z)
    for i, j, s in zip(chk, var, shift):
        par[:, i, :] ^= b3[:, j, (h + s) % Z]
    return par.reshape(b3.shape[0], -1).sum(1)


def dense_H(hb, Z):
    M, N = hb.shape
    H = np.zeros((M * Z, N * Z), dtype=np.int64)
    h = np.arange(Z)
    for i, j, s in zip(*edge_tables(hb, Z)):
        H[i * Z + h, j * Z + (h + s) % Z] = 1
    return H


def test_edge_table_syndrome_equals_dense_H():
    hb = np.loadtxt(os.path.join(RES, "basegraph2_set0.txt"), int, delimiter="\t")
    Z = 16
    H = dense_H(hb, Z)
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, size=(9, hb.shape[1] * Z))
    assert np.array_equal(unsat_numpy(bits, hb, Z), ((bits @ H.T) % 2).sum(1))
    # generated codewords have syndrome 0; one flipped bit leaves its column's degree unsatisfied
    G = np.loadtxt(os.path.join(RES, "gen_matrix_bg2_z16.txt"), int, delimiter=",")
    info = rng.integers(0, 2, size=(5, G.shape[0]))
    cw = info @ G % 2
    assert not unsat_numpy(cw, hb, Z).any()
    cw[0, 3 * Z + 5] ^= 1
    assert unsat_numpy(cw, hb, Z)[0] == (hb[:, 3] != -1).sum()
