"""Sequential models of circular-buffer rate matching (3GPP TS 38.212 §5.4.2) for the tests: the spec's selection
loop and interleaver loops as written, and rate recovery as sequential fp32 sums.  Nothing here uses the closed-form
maps of csrc/nldpc_rm_index.h."""
import numpy as np


def model_index(M, N, Z, E, k0=0, punct_cols=0, n_filler=0, ncb=0, qm=1):
    """idx[m] = the codeword bit that output bit m carries."""
    K = N - M
    P = punct_cols * Z
    Ncb = ncb if ncb else N * Z - P
    f0, f1 = K * Z - n_filler - P, K * Z - P
    e = np.zeros(E, dtype=np.int64)
    k = j = 0
    while k < E:
        p = (k0 + j) % Ncb
        if not (f0 <= p < f1):
            e[k] = P + p  # d[p] = y[P + p]
            k += 1
        j += 1
    f = np.zeros(E, dtype=np.int64)
    for i in range(qm):
        for jj in range(E // qm):
            f[i + jj * qm] = e[i * (E // qm) + jj]
    return f


def model_sel_order(E, qm):
    """k[m]: the selection index of output bit m (f[m] = e[k[m]]), from the interleaver loops."""
    k = np.zeros(E, dtype=np.int64)
    for i in range(qm):
        for jj in range(E // qm):
            k[i + jj * qm] = i * (E // qm) + jj
    return k


def model_recover(M, N, Z, rm, llr, prev=None, erasure=0.0, filler=-20.0, clip=0.0):
    """fp32 [B, N*Z].  rm: dict of model_index's keyword arguments.  prev None: sums start at +0 and positions that
    received nothing hold `erasure`; prev [B, N*Z]: sums start there and such positions keep it."""
    E = rm["E"]
    idx = model_index(M, N, Z, **rm)
    sel = model_sel_order(E, rm.get("qm", 1))
    B = llr.shape[0]
    K, F = N - M, rm.get("n_filler", 0)
    acc = np.zeros((B, N * Z), dtype=np.float32) if prev is None else prev.astype(np.float32).copy()
    got = np.zeros(N * Z, dtype=bool)
    for m in np.argsort(sel, kind="stable"):  # ascending selection index k
        acc[:, idx[m]] = acc[:, idx[m]] + llr[:, m].astype(np.float32)  # one fp32 rounding per add
        got[idx[m]] = True
    if clip > 0:
        c = np.float32(clip)
        lo = np.where(acc < -c, -c, acc)  # clampf: a NaN fails both comparisons and stays
        acc[:, got] = np.where(lo > c, c, lo)[:, got]
    if prev is None:
        acc[:, ~got] = np.float32(erasure)
    acc[:, K * Z - F:K * Z] = np.float32(filler)
    return acc, got
