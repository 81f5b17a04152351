"""numpy model of MIMO spatial multiplexing with LMMSE soft detection for the tests, written from the definitions of
include/nldpc.h, never from the library, on oracle.philox and qam_model.  Two parts:

(a) a restatement in the stated order of operations, every array operation one IEEE operation per element (numpy adds,
    multiplies, divides and takes square roots element by element and fuses nothing), float64 for the filter and float32
    for the channel product, the equaliser and the demapper.  Everything without log / cos / sin is expected to equal
    the library bit for bit:
      n_blocks / block_index        the fading blocks of a row of R resource elements
      entry_of_words / channels     a drawn entry from its Philox words, and the table [B, n_blk, nr, nt, 2]
      normals / received            the noise [B, R, nr, 2] and y = H x + sigma n
      filter_ordered                W, mu, w from the Cholesky factor of I + H^H H / n0
      equalise / maxlog / logmap64  x^ = W y, and the demappers on the levels fl32(mu l) with weight w per symbol
      detect_maxlog / detect_logmap64   the whole receiver from y and the table
(b) an independent LMMSE in complex128 on numpy.linalg: filter_linalg (solve(G, H^H), diag(W H)).

The log-MAP bound is qam_model.logmap_bound unchanged, as for the fading channel (fading_model's docstring): the
derivation takes the fp32 levels, the fp32 received value and the fp32 weight as inputs of both the fp32 demapper and
the fp64 model and uses nothing about where they come from.  Here the levels are fl32(mu_k l), the value is x^_k and
the weight is w_k.

siso_bound: for nt = nr = 1 and a real channel h = g the detector is analytically the CSI demapper of the fading
section, (x^ - mu l)^2 w = (y - g l)^2 / n0 with x^ = W y, W = g / (g^2 + n0), mu = W g, w = 1 / (mu (1 - mu)) and
W^2 w = 1 / n0.  Both fp32 max-log chains are compared with the exact max-log LLR* of the fp32 y and g, per real
dimension, in the units of the fading chain (the MIMO chain's lengths divided by W).  u = 2^-24, u' = u + 2^-47 (a
value computed by a few dozen double operations and rounded to fp32 once), A = g max|l|, Y = |y|,
T = max over the levels of |y - g l|, n0 = 2 sigma^2 with the fp32 sigma.
  fading chain:  gl^ = fl(g l) is off by u A; t^ = fl(y - gl^) by dt_F = u A + u (T + u A); d^ = fl(t^ t^) by
                 dd_F = 2 T dt_F + dt_F^2 + u (T + dt_F)^2.
  MIMO chain:    W = W* (1 + d1), |d1| <= u'; x^ = fl(W y) exactly (the imaginary part of W is +-0, whose products
                 vanish), so x^ / W* is off from y by ((1 + u')(1 + u) - 1) Y; mu = mu* (1 + d3), |d3| <= u', and
                 fl(mu l) / W* is off from g l by ((1 + u')(1 + u) - 1) A; their sum is s = ((1 + u')(1 + u) - 1)(Y + A);
                 t' = fl(x^ - mu l) is off by dt_M = s + u (T + s); d' by dd_M = 2 T dt_M + dt_M^2 + u (T + dt_M)^2.
  LLR:           min is 1-Lipschitz in the maximum norm, so each of the two minima moves by at most dd; the difference,
                 the product with the weight and the weight's own rounding (fl32(1 / n0) in the fading chain; W^2 w =
                 (1 + u')^3 / n0 at worst in the MIMO chain) multiply by at most (1 + u')^5:
                 |LLR^ - LLR*| <= (2 dd / n0) (1 + u')^5 + |LLR*| ((1 + u')^5 - 1)   for either chain.
  bound = that for the fading chain + that for the MIMO chain (no underflow: g is 0 or of ordinary size).
"""
import numpy as np

import qam_model as qm_
from oracle.philox import philox4x32_10

TAG_NOISE = 0x4D494E31  # "MIN1"
TAG_CHAN = 0x4D494831   # "MIH1"
DIMS = ((1, 1), (1, 2), (1, 4), (2, 2), (2, 4), (4, 4))
F32, F64 = np.float32, np.float64


def n_blocks(R, L):
    return 1 if L >= R else -(-R // L)


def block_index(R, L):
    """int64 [R]: the in-row fading block of every resource element of a row"""
    return np.arange(R, dtype=np.int64) // min(L, R)


def _philox(G, tag, q, seed):
    """uint32 [len(G), 4]: the words of counter (lo32(G), hi32(G), tag, q)"""
    G = np.asarray(G, dtype=np.int64)
    ctr = np.zeros((len(G), 4), dtype=np.uint32)
    ctr[:, 0] = (G & 0xFFFFFFFF).astype(np.uint32)
    ctr[:, 1] = (G >> 32).astype(np.uint32)
    ctr[:, 2] = tag
    ctr[:, 3] = q
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def _box_muller(r0, r1):
    u0 = (r0.astype(F64) + 1.0) * (1.0 / 4294967296.0)
    u1 = (r1.astype(F64) + 1.0) * (1.0 / 4294967296.0)
    rad, th = np.sqrt(-2.0 * np.log(u0)), 6.283185307179586 * u1
    return rad * np.cos(th), rad * np.sin(th)


def entry_of_words(nt, r0, r1):
    """fp32 [..., 2]: the CN(0, 1/nt) entry of the Philox words (r0, r1), in double, each component rounded once"""
    s = np.sqrt(1.0 / (2.0 * F64(nt)))
    a, b = _box_muller(r0, r1)
    return np.stack([(s * a).astype(F32), (s * b).astype(F32)], axis=-1)


def block_words(G, nt, nr, seed):
    """uint32 [len(G), nr*nt, 2]: entry e of global block Gf takes words (x, y) of counter e >> 1 when even, (z, w)
    when odd"""
    ne = nr * nt
    w = np.stack([_philox(G, TAG_CHAN, c, seed) for c in range((ne + 1) // 2)], axis=1)  # [n, ceil(ne/2), 4]
    return w.reshape(len(G), -1, 2)[:, :ne]


def channels(B, R, L, nt, nr, seed, b_offset=0):
    """fp32 [B, n_blk, nr, nt, 2]: global block Gf = (b_offset + b) * n_blk + k"""
    nb = n_blocks(R, L)
    G = np.arange(b_offset * nb, (b_offset + B) * nb, dtype=np.int64)
    w = block_words(G, nt, nr, seed)
    return entry_of_words(nt, w[..., 0], w[..., 1]).reshape(B, nb, nr, nt, 2)


def normals(B, R, nr, seed, b_offset=0):
    """fp64 [B, R, nr, 2]: global RE index Gre = (b_offset + b) * R + i, counter word 3 = the antenna pair q; words
    (x, y) give antenna 2q, (z, w) antenna 2q + 1"""
    G = np.arange(b_offset * R, (b_offset + B) * R, dtype=np.int64)
    out = np.zeros((len(G), nr, 2))
    for q in range((nr + 1) // 2):
        w = _philox(G, TAG_NOISE, q, seed)
        out[:, 2 * q, 0], out[:, 2 * q, 1] = _box_muller(w[:, 0], w[:, 1])
        if 2 * q + 1 < nr:
            out[:, 2 * q + 1, 0], out[:, 2 * q + 1, 1] = _box_muller(w[:, 2], w[:, 3])
    return out.reshape(B, R, nr, 2)


def per_re(table, R, L):
    """a table [B, n_blk, ...] spread over the resource elements: [B, R, ...]"""
    return np.asarray(table)[:, block_index(R, L)]


# ---- complex arithmetic on (re, im) pairs of arrays: four products, one difference, one sum
def _mul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _conj_mul(a, b):  # conj(a) b
    return a[0] * b[0] + a[1] * b[1], a[0] * b[1] - a[1] * b[0]


def _mul_conj(a, b):  # a conj(b)
    return a[0] * b[0] + a[1] * b[1], a[1] * b[0] - a[0] * b[1]


def _sum(terms):
    """the first term, then the others added in order, real and imaginary parts separately"""
    re, im = terms[0]
    for t in terms[1:]:
        re, im = re + t[0], im + t[1]
    return re, im


def _abs2(a):
    return a[0] * a[0] + a[1] * a[1]


def apply_matrix(mat, vec):
    """fp32: out(r) = sum_t mat(r, t) vec(t), t ascending.  mat [..., n_out, n_in, 2], vec [..., n_in, 2]"""
    mat, vec = np.asarray(mat, dtype=F32), np.asarray(vec, dtype=F32)
    n_out, n_in = mat.shape[-3], mat.shape[-2]
    out = np.zeros(mat.shape[:-3] + (n_out, 2), dtype=F32)
    for r in range(n_out):
        re, im = _sum([_mul((mat[..., r, t, 0], mat[..., r, t, 1]), (vec[..., t, 0], vec[..., t, 1]))
                       for t in range(n_in)])
        assert re.dtype == F32
        out[..., r, 0], out[..., r, 1] = re, im
    return out


def received(f, qm, sigma, table, L, nt, nr, seed, b_offset=0):
    """fp32 [B, R, nr, 2]: s = H x in fp32, then one rounding of the double sum s + sigma n per component"""
    x = qm_.modulate(f, qm)
    B, S = x.shape[:2]
    R = S // nt
    s = apply_matrix(per_re(table, R, L), x.reshape(B, R, nt, 2))
    return (s.astype(F64) + F64(F32(sigma)) * normals(B, R, nr, seed, b_offset)).astype(F32)


def filter_ordered(h, sigma):
    """(a): h fp32 [..., nr, nt, 2] -> W fp32 [..., nt, nr, 2], mu fp32 [..., nt], w fp32 [..., nt], float64 in the order
    include/nldpc.h states"""
    h = np.asarray(h, dtype=F32)
    nr, nt = h.shape[-3], h.shape[-2]
    lead = h.shape[:-3]
    H = [[(h[..., r, t, 0].astype(F64), h[..., r, t, 1].astype(F64)) for t in range(nt)] for r in range(nr)]
    s = F64(F32(sigma))
    n0 = 2.0 * (s * s)
    q = 1.0 / n0
    zero = np.zeros(lead)
    Gn = {}
    for j in range(nt):
        for k in range(j + 1):
            if k == j:
                d = _abs2(H[0][k])
                for r in range(1, nr):
                    d = d + _abs2(H[r][k])
                Gn[j, k] = (d * q + 1.0, zero)
            else:
                a = _sum([_conj_mul(H[r][j], H[r][k]) for r in range(nr)])
                Gn[j, k] = (a[0] * q, a[1] * q)
    C, c = {}, {}
    for j in range(nt):
        d = Gn[j, j][0]
        for k in range(j):
            d = d - _abs2(C[j, k])
        C[j, j] = (np.sqrt(d), zero)
        c[j] = 1.0 / C[j, j][0]
        for i in range(j + 1, nt):
            zr, zi = Gn[i, j]
            for k in range(j):
                p = _mul_conj(C[i, k], C[j, k])
                zr, zi = zr - p[0], zi - p[1]
            C[i, j] = (zr * c[j], zi * c[j])
    M = {}
    for j in range(nt):
        M[j, j] = (c[j], zero)
        for i in range(j + 1, nt):
            a = _sum([_mul(C[i, k], M[k, j]) for k in range(j, i)])
            M[i, j] = (-a[0] * c[i], -a[1] * c[i])
    mu = np.zeros(lead + (nt,), dtype=F32)
    w = np.zeros(lead + (nt,), dtype=F32)
    for k in range(nt):
        e = M[k, k][0] * M[k, k][0]
        for i in range(k + 1, nt):
            e = e + _abs2(M[i, k])
        m = 1.0 - e
        p = m * e
        ok = (p > 0.0) & np.isfinite(p)
        mu[..., k] = m.astype(F32)
        w[..., k] = np.where(ok, 1.0 / np.where(ok, p, 1.0), 0.0).astype(F32)
    W = np.zeros(lead + (nt, nr, 2), dtype=F32)
    T = {(i, r): _sum([_mul_conj(M[i, k], H[r][k]) for k in range(i + 1)]) for i in range(nt) for r in range(nr)}
    for k in range(nt):
        for r in range(nr):
            a = _sum([_conj_mul(M[i, k], T[i, r]) for i in range(k, nt)])
            W[..., k, r, 0], W[..., k, r, 1] = (a[0] * q).astype(F32), (a[1] * q).astype(F32)
    return W, mu, w


def filter_linalg(h, sigma):
    """(b): the same three tables from numpy.linalg in complex128: G = H^H H + n0 I, W = solve(G, H^H), mu = diag(W H),
    w = 1 / (mu (1 - mu))"""
    h = np.asarray(h, dtype=F32).astype(F64)
    H = h[..., 0] + 1j * h[..., 1]  # [..., nr, nt]
    nt = H.shape[-1]
    s = F64(F32(sigma))
    Hh = np.conj(np.swapaxes(H, -1, -2))
    G = Hh @ H + 2.0 * s * s * np.eye(nt)
    W = np.linalg.solve(G, Hh)
    mu = np.real(np.einsum("...kr,...rk->...k", W, H))
    p = mu * (1.0 - mu)
    with np.errstate(divide="ignore"):
        w = np.where(p > 0, 1.0 / p, 0.0)
    return np.stack([W.real, W.imag], axis=-1).astype(F32), mu.astype(F32), w.astype(F32)


def equalise(W, y):
    """fp32 [..., nt, 2]: x^_k = sum_r W(k, r) y(r), r ascending"""
    return apply_matrix(W, y)


def _levels(qm, mu):
    lv, lab = qm_.dim_levels(qm)
    glv = np.asarray(mu, dtype=F32)[..., None, None] * lv
    assert glv.dtype == F32
    return glv, lab


def maxlog(xh, qm, mu, w):
    """fp32 symbols xh [B, S, 2], mu and w per symbol [B, S] -> fp32 [B, S*qm]: qam_model.maxlog on the levels fl32(mu l)
    with the weight w"""
    glv, lab = _levels(qm, mu)
    x = np.asarray(xh, dtype=F32)
    wt = np.asarray(w, dtype=F32)[..., None]
    t = x[..., None] - glv
    d = t * t
    assert d.dtype == F32
    out = np.zeros(x.shape[:-1] + (qm,), dtype=F32)
    for k in range(qm // 2):
        llr = (d[..., lab[:, k] == 0].min(axis=-1) - d[..., lab[:, k] == 1].min(axis=-1)) * wt
        out[..., 2 * k], out[..., 2 * k + 1] = llr[..., 0], llr[..., 1]
    assert out.dtype == F32
    return out.reshape(x.shape[0], -1)


def logmap64(xh, qm, mu, w):
    """fp64 log-MAP LLRs [B, S*qm] of the fp32 symbols on the fp32 levels fl32(mu l) with the fp32 weight w, and
    D = max |d w| of each LLR's dimension"""
    glv, lab = _levels(qm, mu)
    x = np.asarray(xh, dtype=F32).astype(F64)
    wt = np.asarray(w, dtype=F32).astype(F64)[..., None, None]
    d = (x[..., None] - glv.astype(F64)) ** 2
    m = -d * wt

    def lse(a):
        mx = a.max(axis=-1)
        return mx + np.log(np.exp(a - mx[..., None]).sum(axis=-1))

    out = np.zeros(x.shape[:-1] + (qm,))
    dmax = np.zeros_like(out)
    D = (d * wt).max(axis=-1)
    for k in range(qm // 2):
        llr = lse(m[..., lab[:, k] == 1]) - lse(m[..., lab[:, k] == 0])
        for dim in (0, 1):
            out[..., 2 * k + dim] = llr[..., dim]
            dmax[..., 2 * k + dim] = D[..., dim]
    return out.reshape(x.shape[0], -1), dmax.reshape(x.shape[0], -1)


def _front(y, table, sigma, L, filt):
    """the equalised symbols [B, S, 2] and mu, w per symbol [B, S] of the samples y [B, R, nr, 2]"""
    y = np.asarray(y, dtype=F32)
    B, R = y.shape[:2]
    W, mu, w = filt(table, sigma)
    nt = mu.shape[-1]
    xh = equalise(per_re(W, R, L), y)
    return xh.reshape(B, R * nt, 2), per_re(mu, R, L).reshape(B, R * nt), per_re(w, R, L).reshape(B, R * nt)


def detect_maxlog(y, table, qm, sigma, L, filt=filter_ordered):
    xh, mu, w = _front(y, table, sigma, L, filt)
    return maxlog(xh, qm, mu, w)


def detect_logmap64(y, table, qm, sigma, L, filt=filter_ordered):
    xh, mu, w = _front(y, table, sigma, L, filt)
    return logmap64(xh, qm, mu, w)


def siso_bound(sym, qm, sigma, g):
    """the bound of the module docstring on |MIMO max-log - fading max-log| for nt = nr = 1 and h = g real: sym fp32
    [B, S, 2], g per symbol [B, S] -> [B, S*qm]"""
    u = 2.0 ** -24
    u1 = u + 2.0 ** -47
    lv, lab = qm_.dim_levels(qm)
    s = F64(F32(sigma))
    n0 = 2.0 * s * s
    y = np.asarray(sym, dtype=F32).astype(F64)
    gg = np.asarray(g, dtype=F32).astype(F64)[..., None]
    d = (y[..., None] - gg[..., None] * lv.astype(F64)) ** 2  # [B, S, 2, 2^h]
    T = np.sqrt(d.max(axis=-1))
    A = gg * np.abs(lv).max()
    Y = np.abs(y)
    dt_f = u * A + u * (T + u * A)
    dd_f = 2 * T * dt_f + dt_f ** 2 + u * (T + dt_f) ** 2
    sm = ((1 + u1) * (1 + u) - 1) * (Y + A)
    dt_m = sm + u * (T + sm)
    dd_m = 2 * T * dt_m + dt_m ** 2 + u * (T + dt_m) ** 2
    k5 = (1 + u1) ** 5
    out = np.zeros(y.shape[:-1] + (qm,))
    for k in range(qm // 2):
        llr = (d[..., lab[:, k] == 0].min(axis=-1) - d[..., lab[:, k] == 1].min(axis=-1)) / n0
        b = (2 * (dd_f + dd_m) / n0) * k5 + 2 * np.abs(llr) * (k5 - 1)
        out[..., 2 * k], out[..., 2 * k + 1] = b[..., 0], b[..., 1]
    return out.reshape(y.shape[0], -1)
