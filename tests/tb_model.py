"""The transport-block steps of 3GPP TS 38.212 restated in numpy, literally and sequentially: §5.2.2 (code-block
segmentation and the code-block CRC), the E_r rule of §5.4.2.1, §5.5 (code-block concatenation), their inverses and the
verdicts of a received TB -- the expected values of test_transport_host.py and test_gpu_transport.py.  CRCs are
crc_model.py's long division; nothing here is shared with csrc/nldpc_tb.h (no combination of remainders: the TB is
reassembled and divided as a whole).

Batches are block-major, as in the library: code block r of transport block t is row r * Btb + t.
"""
import collections

import numpy as np

import crc_model as cm

Plan = collections.namedtuple("Plan", "A tb_crc W C L Kp F")
LIFTING_SIZES = sorted(a * 2 ** j for a in (2, 3, 5, 7, 9, 11, 13, 15) for j in range(8) if a * 2 ** j <= 384)


def plan(A, tb_crc, W, kcb=0):
    """§5.2.2 with B = A + L_tb input bits, rows of W bits and the largest code block kcb (0: W); ValueError when the
    sizes do not fit"""
    Bp = A + cm.length(tb_crc)
    kcb = kcb or W
    if kcb > W:
        raise ValueError("kcb > W")
    if Bp <= kcb:
        L, C, Bpp = 0, 1, Bp
    else:
        if kcb <= 24:
            raise ValueError("kcb <= 24")
        L = 24
        C = -(-Bp // (kcb - L))
        Bpp = Bp + C * L
    if Bpp % C:
        raise ValueError("C does not divide B''")
    Kp = Bpp // C
    if Kp > W:
        raise ValueError("K' > W")
    return Plan(A, tb_crc, W, C, L, Kp, W - Kp)


def lifting_size(bg, Bp):
    """(Kb, Zc): the search of §5.2.2 over all 51 lifting sizes, K' = ceil(B'' / C) under the base graph's Kcb"""
    kcb = 8448 if bg == 1 else 3840
    C, L = (1, 0) if Bp <= kcb else (-(-Bp // (kcb - 24)), 24)
    Kp = -(-(Bp + C * L) // C)
    if bg == 1:
        Kb = 22
    elif Bp > 640:
        Kb = 10
    elif Bp > 560:
        Kb = 9
    elif Bp > 192:
        Kb = 8
    else:
        Kb = 6
    return Kb, min(Z for Z in LIFTING_SIZES if Kb * Z >= Kp)


def segment(tb, p):
    """tb [Btb, B'] of 0/1 -> info [C * Btb, W]: the spec's loop over r and k with s running through the TB's bits"""
    tb = np.asarray(tb, dtype=np.uint8)
    Btb = tb.shape[0]
    assert tb.shape[1] == p.A + cm.length(p.tb_crc) == p.C * (p.Kp - p.L)
    info = np.zeros((p.C * Btb, p.W), dtype=np.uint8)
    s = 0
    for r in range(p.C):
        rows = info[r * Btb:(r + 1) * Btb]
        for k in range(p.Kp - p.L):
            rows[:, k] = tb[:, s]
            s += 1
        if p.C > 1:
            rows[:, p.Kp - p.L:p.Kp] = cm.parity_bits(rows[:, :p.Kp - p.L], "24B")
        # (k = K' .. W - 1: filler bits, zero)
    return info


def desegment(rows, p):
    """rows [C * Btb, >= K'] -> tb [Btb, B']: the inverse loop"""
    rows = np.asarray(rows)
    Btb = rows.shape[0] // p.C
    tb = np.zeros((Btb, p.C * (p.Kp - p.L)), dtype=np.uint8)
    s = 0
    for r in range(p.C):
        for k in range(p.Kp - p.L):
            tb[:, s] = rows[r * Btb:(r + 1) * Btb, k]
            s += 1
    return tb


def split_E(G, qm, C, n_layers=1):
    """[E_0 .. E_{C-1}] of §5.4.2.1 (every code block is scheduled: C' = C)"""
    q = n_layers * qm
    if G % q or G // q < C:
        raise ValueError("G")
    E = []
    for r in range(C):
        if r <= C - (G // q) % C - 1:
            E.append(q * ((G // q) // C))
        else:
            E.append(q * -(-(G // q) // C))
    return E


def concat(f, Btb):
    """f: list of C arrays [Btb, E_r] -> g [Btb, G]: the loop of §5.5"""
    g = np.zeros((Btb, sum(x.shape[1] for x in f)), dtype=f[0].dtype)
    k = 0
    for r in range(len(f)):
        for j in range(f[r].shape[1]):
            g[:, k] = f[r][:, j]
            k += 1
    return g


def deconcat(g, E):
    out, k = [], 0
    for r in range(len(E)):
        out.append(g[:, k:k + E[r]].copy())
        k += E[r]
    return out


def check(hard, p, ref_tb=None):
    """hard [C * Btb, >= K'] of 0/1 -> (cb_ok bool [C * Btb], tb_ok bool [Btb], tb [Btb, B'], counts int64 [4]: TB CRC
    failures, undetected TB errors, TB errors, code-block CRC failures)"""
    hard = np.asarray(hard).astype(np.uint8)
    tb = desegment(hard, p)
    tb_ok = cm.passes(tb, p.tb_crc, p.A)
    Btb = tb.shape[0]
    cb_ok = cm.passes(hard, "24B", p.Kp - 24) if p.C > 1 else tb_ok.copy()
    if ref_tb is None:
        err = np.zeros(Btb, dtype=bool)
    else:
        err = (tb != (np.asarray(ref_tb) != 0)).any(axis=1)
    counts = np.array([(~tb_ok).sum(), (tb_ok & err).sum(), err.sum(), (~cb_ok).sum()], dtype=np.int64)
    return cb_ok, tb_ok, tb, counts
