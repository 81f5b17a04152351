"""numpy model of QAM modulation, soft demapping and the fused QAM/AWGN channel for the tests, written from the
definitions of include/nldpc.h (3GPP TS 38.211 §5.1.3-5.1.6), never from the library:

  amplitudes / modulate / constellation   the 38.211 formulas, written out per order
  maxlog                                   the fp32 max-log demapper with the stated roundings (numpy float32 operations)
  logmap64 / logmap_bound                  the fp64 log-MAP demapper and the bound on the fp32 one's distance from it
  normals / noisy_symbols                  the noise of nldpc_qam_channel_llr from oracle.philox.philox4x32_10

The log-MAP bound, derived from how the fp32 demapper computes (u = 2^-24 the unit roundoff, one ulp <= 2u relative):
for one real dimension let D = max over the 2^h levels of |d w| (fp64) and n = 2^(h-1) the levels per bit value.
  1. t = fl(x - l), d = fl(t t), m = -fl(d w): m^ = m (1 + theta), |theta| <= g = (1 + u)^4 - 1, so every exponent is off
     by at most e1 = g D, and so is a log-sum-exp of them (lse is 1-Lipschitz in the maximum norm).  D^ = D (1 + g).
  2. From the m^: the maximum M^ is exact; a = fl(m^ - M^) is off by at most u D^; expf is within KE ulp, so a term has
     relative error rho = exp(u D^) (1 + 2 KE u) - 1 (a term so small that it is subnormal adds at most 2^-120 to a sum
     that is at least 1); n positive terms added one by one from +0: the sum has relative error
     rs = (1 + rho) (1 + u)^(n-1) - 1 + 2^-120 n.  |log s^ - log s| <= e2 = min(-log(1 - rs), log n) -- both sums lie in
     [1, n] whatever the errors: the largest term is exp(0) = 1 exactly and no term exceeds it; log n alone is used once
     rs >= 1/2 (a symbol far outside the constellation at a small sigma) --; logf is within KL ulp of a value of at most
     log n + e2: e3 = e2 + 2 KL u (log n + e2).  lse^ = fl(M^ + L^) adds e4 = u (D^ + log n + e3).
     Each log-sum-exp is therefore within e = e1 + e3 + e4 of the fp64 one.
  3. The final fl(lse1^ - lse0^) adds u (|LLR| + 2 e).
  bound = 2 e + u (|LLR| + 2 e) + 2^-40 (1 + D)   (the last term covers the fp64 model's own rounding)
KE = KL = 2 ulp for both functions: glibc's expf / logf are within 1 ulp, and 2 is the largest maximum error the GPU
vendors' math-library tables give for either (expf 2, logf 1 in the CUDA programming guide, which the HIP device
functions follow or better).  The bound grows linearly with D and is about 14 u D + 50 u for moderate D.
"""
import numpy as np

from oracle.philox import philox4x32_10

ORDERS = (2, 4, 6, 8)
TAG = 0x51414D31  # counter word 2 of the QAM noise stream
U = 2.0 ** -24
KE = KL = 2


def scale(qm):
    """A: the fp32 nearest to 1/sqrt(2), 1/sqrt(10), 1/sqrt(42), 1/sqrt(170), computed in double and rounded once"""
    return np.float32(1.0 / np.sqrt(np.float64({2: 2, 4: 10, 6: 42, 8: 170}[qm])))


def amplitudes(bits, qm):
    """bits [..., qm] of 0 / 1 -> the integer amplitudes (I, Q) of TS 38.211 §5.1.3 (QPSK), §5.1.4 (16QAM), §5.1.5
    (64QAM), §5.1.6 (256QAM), each formula as the specification prints it"""
    b = [bits[..., i].astype(np.int64) for i in range(qm)]
    if qm == 2:
        return (1 - 2 * b[0]), (1 - 2 * b[1])
    if qm == 4:
        return (1 - 2 * b[0]) * (2 - (1 - 2 * b[2])), (1 - 2 * b[1]) * (2 - (1 - 2 * b[3]))
    if qm == 6:
        return ((1 - 2 * b[0]) * (4 - (1 - 2 * b[2]) * (2 - (1 - 2 * b[4]))),
                (1 - 2 * b[1]) * (4 - (1 - 2 * b[3]) * (2 - (1 - 2 * b[5]))))
    if qm == 8:
        return ((1 - 2 * b[0]) * (8 - (1 - 2 * b[2]) * (4 - (1 - 2 * b[4]) * (2 - (1 - 2 * b[6])))),
                (1 - 2 * b[1]) * (8 - (1 - 2 * b[3]) * (4 - (1 - 2 * b[5]) * (2 - (1 - 2 * b[7])))))
    raise ValueError(qm)


def modulate(f, qm):
    """f [B, E] bytes (non-zero = 1) -> fp32 [B, E/qm, 2]: level = (float)a * A, one fp32 rounding"""
    B, E = f.shape
    ai, aq = amplitudes((f != 0).reshape(B, E // qm, qm), qm)
    return np.stack([ai.astype(np.float32) * scale(qm), aq.astype(np.float32) * scale(qm)], axis=-1)


def constellation(qm):
    """fp32 [2^qm, 2]: point v is the symbol of the bits b_i = (v >> (qm-1-i)) & 1"""
    v = np.arange(2 ** qm)
    bits = np.stack([(v >> (qm - 1 - i)) & 1 for i in range(qm)], axis=1).astype(np.uint8)
    return modulate(bits.reshape(1, -1), qm)[0]


def dim_levels(qm):
    """(levels fp32 [2^h], labels [2^h, h]) of one real dimension: the level of every choice of c_0 .. c_{h-1}"""
    h = qm // 2
    c = np.arange(2 ** h)
    labels = np.stack([(c >> (h - 1 - k)) & 1 for k in range(h)], axis=1)
    bits = np.zeros((2 ** h, qm), dtype=np.uint8)
    bits[:, 0::2] = labels  # the I dimension takes b_0, b_2, ...
    return modulate(bits.reshape(1, -1), qm)[0, :, 0], labels


def weight(sigma):
    """w = (float)(1 / (2 sigma^2)) with sigma the fp32 the ABI takes, computed in double"""
    s = np.float64(np.float32(sigma))
    return np.float32(1.0 / (2.0 * s * s))


def maxlog(sym, qm, sigma):
    """fp32 [..., S, 2] -> fp32 [..., S*qm]: t = x - l, d = t * t, (min_{c_k=0} d - min_{c_k=1} d) * w, all fp32"""
    lv, lab = dim_levels(qm)
    h, w = qm // 2, weight(sigma)
    x = np.asarray(sym, dtype=np.float32)
    t = x[..., None] - lv  # [..., S, 2, 2^h], float32 - float32
    d = t * t
    assert d.dtype == np.float32
    out = np.zeros(x.shape[:-1] + (qm,), dtype=np.float32)
    for k in range(h):
        m0 = d[..., lab[:, k] == 0].min(axis=-1)
        m1 = d[..., lab[:, k] == 1].min(axis=-1)
        llr = (m0 - m1) * w
        out[..., 2 * k] = llr[..., 0]      # I: b_{2k}
        out[..., 2 * k + 1] = llr[..., 1]  # Q: b_{2k+1}
    assert out.dtype == np.float32
    return out.reshape(x.shape[:-2] + (x.shape[-2] * qm,))


def logmap64(sym, qm, sigma):
    """fp64 log-MAP LLRs [..., S*qm] of fp32 symbols, and D = max |d w| of each LLR's dimension (same shape)"""
    lv, lab = dim_levels(qm)
    h, w = qm // 2, np.float64(weight(sigma))
    x = np.asarray(sym, dtype=np.float32).astype(np.float64)
    d = (x[..., None] - lv.astype(np.float64)) ** 2
    m = -d * w

    def lse(a):
        mx = a.max(axis=-1)
        return mx + np.log(np.exp(a - mx[..., None]).sum(axis=-1))

    out = np.zeros(x.shape[:-1] + (qm,))
    dmax = np.zeros_like(out)
    D = (d * w).max(axis=-1)
    for k in range(h):
        llr = lse(m[..., lab[:, k] == 1]) - lse(m[..., lab[:, k] == 0])
        for dim in (0, 1):
            out[..., 2 * k + dim] = llr[..., dim]
            dmax[..., 2 * k + dim] = D[..., dim]
    shape = x.shape[:-2] + (x.shape[-2] * qm,)
    return out.reshape(shape), dmax.reshape(shape)


def logmap_bound(qm, llr64, dmax):
    """the bound of the module docstring, per LLR"""
    n = 2 ** (qm // 2 - 1)
    g = (1 + U) ** 4 - 1
    D = np.asarray(dmax, dtype=np.float64)
    Dh = D * (1 + g)
    e1 = g * D
    rho = np.exp(U * Dh) * (1 + 2 * KE * U) - 1
    rs = (1 + rho) * (1 + U) ** (n - 1) - 1 + 2.0 ** -120 * n
    e2 = np.where(rs < 0.5, np.minimum(-np.log1p(-np.minimum(rs, 0.5)), np.log(n)), np.log(n))
    e3 = e2 + 2 * KL * U * (np.log(n) + e2)
    e4 = U * (Dh + np.log(n) + e3)
    e = e1 + e3 + e4
    return 2 * e + U * (np.abs(llr64) + 2 * e) + 2.0 ** -40 * (1 + D)


def normals(B, S, seed, b_offset=0, tag=TAG):
    """fp64 [B, S, 2]: the noise of nldpc_qam_channel_llr.  Global symbol G = (b_offset + b) * S + s; counter
    (lo32(G >> 1), hi32(G >> 1), tag, 0); Box-Muller of (u0, u1) is (I, Q) of the even symbol, of (u2, u3) the odd one's"""
    G = np.arange(b_offset * S, (b_offset + B) * S, dtype=np.int64)
    pairs = np.unique(G >> 1)
    ctr = np.zeros((len(pairs), 4), dtype=np.uint32)
    ctr[:, 0] = (pairs & 0xFFFFFFFF).astype(np.uint32)
    ctr[:, 1] = (pairs >> 32).astype(np.uint32)
    ctr[:, 2] = tag
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).astype(np.float64)
    u = (r + 1.0) * (1.0 / 4294967296.0)
    rad0, th0 = np.sqrt(-2.0 * np.log(u[:, 0])), 6.283185307179586 * u[:, 1]
    rad1, th1 = np.sqrt(-2.0 * np.log(u[:, 2])), 6.283185307179586 * u[:, 3]
    n = np.stack([rad0 * np.cos(th0), rad0 * np.sin(th0), rad1 * np.cos(th1), rad1 * np.sin(th1)], axis=1)
    n = n.reshape(-1, 2)  # [2 * pairs, (I, Q)] by global symbol, from symbol 2 * pairs[0] on
    return n[G - 2 * pairs[0]].reshape(B, S, 2)


def noisy_symbols(f, qm, sigma, seed, b_offset=0):
    """fp32 [B, S, 2]: r = (float)((double)level + (double)sigma * n), one rounding per dimension"""
    lv = modulate(f, qm).astype(np.float64)
    B, S = lv.shape[:2]
    return (lv + np.float64(np.float32(sigma)) * normals(B, S, seed, b_offset)).astype(np.float32)
