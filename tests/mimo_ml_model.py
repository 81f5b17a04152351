"""numpy model of the exact max-log ML (joint) MIMO detector for the tests, written from the definitions of
include/nldpc.h (F14), never from the library, on mimo_model and qam_model.  Two parts:

(a) detect_ml: the sliced two-pass detector in the stated order of operations, float32, every array operation one IEEE
    operation per element.  The candidates of a pass are an array axis; a minimum is exact, so the order in which the
    library walks them does not show.  Expected to equal the library bit for bit.
(b) detect_exhaustive64: an independent float64 search over all M^nt symbol vectors of every resource element,
    d(x) = sum_r |y_r - sum_t h_rt x_t|^2 with numpy's complex arithmetic, LLR = (min_{b=0} d - min_{b=1} d) / n0.

ml_bound: |(a) - (b)| per LLR, derived from the arithmetic.  u = 2^-24, xm = the largest level, per antenna
S_r = max(|Re y_r|, |Im y_r|) + sum_t (|Re h_rt| + |Im h_rt|) xm (no partial residual component exceeds it).
  residual:  a component is y_r minus up to nt complex products subtracted one by one; a term carries at most nt + 2
             roundings, so the component is off by at most dl_r = ((1 + u)^(nt+2) - 1) S_r.
  metric:    a square moves by 2 S_r dl_r + dl_r^2; the sum of the 2 nr rounded squares adds at most
             ((1 + u)^(2 nr + 1) - 1) of the sum:  dd = sum_r 2 (2 S_r dl_r + dl_r^2) + ((1 + u)^(2 nr + 1) - 1) sum_r 2 (S_r + dl_r)^2.
  slice:     with g = |h_s|^2 the metric of (x_enum, x_s) is g |z - x_s|^2 + const, z = h_s^H r / g, separable in Re / Im.
             The numerator's component is a sum of 2 nr products of a channel component and a residual component:
             dnum = sum_r (|Re h_rs| + |Im h_rs|) dl_r + ((1 + u)^(nr+2) - 1) sum_r (|Re h_rs| + |Im h_rs|) (S_r + dl_r).
             fl(g), fl(1 / g) and the product with it are a relative rho = (1 + u)^(nr+4) - 1.  The slice can pick a point
             other than the nearest one only when z is within dz of a threshold between two levels, hence where
             |z| <= (2^h + 1) A (dz <= A is checked): dz = (dnum / g)(1 + rho) + (2^h + 1) A rho + 2 A 5 u (2^h + 2), the
             last term for u = fl(fl(z K) + 2^(h-1)) with K = fl32(1 / (2 A)) taken back to the units of z.  At distance
             eps <= dz from a threshold the neighbouring point's squared distance exceeds the nearest one's by
             (A + eps)^2 - (A - eps)^2 = 4 A eps, per dimension: the candidate's true metric exceeds the minimum over x_s
             by at most ex_s = g 2 (4 A dz): first order in dz, times a level spacing.  g = 0: the metric does not
             depend on x_s, ex_s = 0.  (g is 0 or of ordinary size; 1 / g does not overflow.)
  LLR:       every candidate the library evaluates is a true candidate whose computed metric is within
             E = dd + max_s ex_s of the exact minimum over x_s; min is 1-Lipschitz in the maximum norm, so each of the
             two minima moves by at most E; the difference, the weight's rounding and the product are three more
             roundings:  |LLR^ - LLR*| <= 2 E / n0 (1 + u)^3 + |LLR*| ((1 + u)^3 - 1).

lmmse_orthogonal_bound: the LMMSE max-log chain of mimo_model against the same exact LLR* when the columns of H are
exactly orthogonal in real arithmetic (one column, or entries 0 / +-c / +-i c arranged as a scaled unitary matrix), where
the layers decouple and LMMSE max-log is analytically max-log ML: G is diagonal, the double-precision factorisation
meets no off-diagonal term, W = H^H / (g_k + n0), mu_k = g_k / (g_k + n0), w_k = (g_k + n0)^2 / (g_k n0), each fp32
table entry off by at most u' = u + 2^-47.  Per layer and real dimension, with x* = sum_r W_kr y_r exact,
Sx = sum_r (|Re W| + |Im W|)(|Re y| + |Im y|), T = max_l |x* - mu l|:  x^ is off by dx = ((1 + u')(1 + u)^(nr+1) - 1) Sx,
fl32(mu l) by dl = ((1 + u')(1 + u) - 1) mu xm, t by dt = dx + dl + u (T + dx + dl), t^2 by dd = 2 T dt + dt^2 +
u (T + dt)^2, and as in mimo_model.siso_bound  |LLR^ - LLR*| <= 2 dd w (1 + u')^5 + |LLR*| ((1 + u')^5 - 1).
"""
import numpy as np

import mimo_model as mm
import qam_model as qm_

F32, F64 = np.float32, np.float64
FLT_MAX = F32(3.402823466e38)
U = 2.0 ** -24


def supported(qm, nt):
    return nt < 4 or qm <= 4


def candidates(qm, nt):
    """candidate metrics per resource element"""
    return 2 ** qm if nt == 1 else 2 * (2 ** qm) ** (nt - 1)


def step(qm):
    """K = 1 / (2 A): the 17-digit literals of include/nldpc.h rounded to fp32 once"""
    return F32({2: 0.70710678118654752, 4: 1.5811388300841897, 6: 3.2403703492039302, 8: 6.5192024052026492}[qm])


def slice_level(z, qm):
    """fp32: the level nearest to z by u = fl(fl(z K) + 2^(h-1)), j = floor(u) clamped to 0 .. 2^h - 1 (NaN -> 0)"""
    h = qm // 2
    half, top = F32(2 ** (h - 1)), F32(2 ** h - 1)
    u = z * step(qm) + half
    j = np.floor(u)
    j = np.where(j > 0, j, F32(0))
    j = np.where(j < top, j, top)
    out = (F32(2) * j - top) * qm_.scale(qm)
    assert out.dtype == F32
    return out


def _pass(y, h, qm, enum, s):
    """one pass over the resource elements y [n, nr, 2], h [n, nr, nt, 2]: the layers `enum` (ascending) enumerated, layer
    s sliced (None: no slicing) -> (metric fp32 [n, M^len(enum)], labels {layer: (ci, cq)} per candidate)"""
    lv, _ = qm_.dim_levels(qm)
    ld, nr = len(lv), y.shape[1]
    grid = np.meshgrid(*([np.arange(ld)] * (2 * len(enum))), indexing="ij")
    lab = {e: (grid[2 * i].reshape(-1), grid[2 * i + 1].reshape(-1)) for i, e in enumerate(enum)}
    res = [(y[:, r, 0][:, None], y[:, r, 1][:, None]) for r in range(nr)]
    col = lambda r, t: (h[:, r, t, 0][:, None], h[:, r, t, 1][:, None])  # noqa: E731
    for e in enum:
        li, lq = lv[lab[e][0]][None, :], lv[lab[e][1]][None, :]
        for r in range(nr):
            a, b = col(r, e)
            res[r] = (res[r][0] - (a * li - b * lq), res[r][1] - (a * lq + b * li))
    if s is not None:
        g = None
        for r in range(nr):
            a, b = col(r, s)
            p = a * a + b * b
            g = p if g is None else g + p
        with np.errstate(divide="ignore"):
            q = F32(1) / g
        inv = np.where((g > 0) & (q <= FLT_MAX), q, F32(0))
        zr = zi = None
        for r in range(nr):
            a, b = col(r, s)
            c, d = res[r]
            pr, pi = a * c + b * d, a * d - b * c
            zr, zi = (pr, pi) if zr is None else (zr + pr, zi + pi)
        xr, xi = slice_level(zr * inv, qm), slice_level(zi * inv, qm)
        for r in range(nr):
            a, b = col(r, s)
            res[r] = (res[r][0] - (a * xr - b * xi), res[r][1] - (a * xi + b * xr))
    m = None
    for r in range(nr):
        p = res[r][0] * res[r][0] + res[r][1] * res[r][1]
        m = p if m is None else m + p
    assert m.dtype == F32
    return m, lab


def _finish(m, lab_e, qm, w):
    """the qm LLRs [n, qm] of one enumerated layer from the metrics m [n, ncand] and its labels per candidate"""
    _, bits = qm_.dim_levels(qm)
    ld = bits.shape[0]
    out = np.zeros((m.shape[0], qm), dtype=F32)
    for dim in (0, 1):
        mn = np.stack([m[:, lab_e[dim] == c].min(axis=1) for c in range(ld)], axis=1)  # per-label minima [n, ld]
        for k in range(qm // 2):
            out[:, 2 * k + dim] = (mn[:, bits[:, k] == 0].min(axis=1) - mn[:, bits[:, k] == 1].min(axis=1)) * w
    return out


def detect_ml(y, table, qm, sigma, L):
    """(a): y fp32 [B, R, nr, 2], table fp32 [B, n_blk, nr, nt, 2] -> fp32 [B, R*nt*qm]"""
    y = np.asarray(y, dtype=F32)
    B, R, nr = y.shape[:3]
    h = mm.per_re(np.asarray(table, dtype=F32), R, L).reshape(B * R, nr, -1, 2)
    nt = h.shape[2]
    assert supported(qm, nt)
    yy = y.reshape(B * R, nr, 2)
    w = qm_.weight(sigma)
    out = np.zeros((B * R, nt, qm), dtype=F32)
    if nt == 1:
        m, lab = _pass(yy, h, qm, [0], None)
        out[:, 0] = _finish(m, lab[0], qm, w)
    else:
        m, lab = _pass(yy, h, qm, list(range(nt - 1)), nt - 1)
        for k in range(nt - 1):
            out[:, k] = _finish(m, lab[k], qm, w)
        m, lab = _pass(yy, h, qm, list(range(1, nt)), 0)
        out[:, nt - 1] = _finish(m, lab[nt - 1], qm, w)
    return out.reshape(B, R * nt * qm)


def detect_exhaustive64(y, table, qm, sigma, L):
    """(b): fp64 [B, R*nt*qm], every one of the M^nt symbol vectors of every resource element"""
    y = np.asarray(y, dtype=F32).astype(F64)
    B, R, nr = y.shape[:3]
    h = mm.per_re(np.asarray(table, dtype=F32), R, L).astype(F64).reshape(B * R, nr, -1, 2)
    nt = h.shape[2]
    H = h[..., 0] + 1j * h[..., 1]
    Y = (y[..., 0] + 1j * y[..., 1]).reshape(B * R, nr)
    c = qm_.constellation(qm).astype(F64)
    pts = c[:, 0] + 1j * c[:, 1]
    M = len(pts)
    bit = np.stack([(np.arange(M) >> (qm - 1 - i)) & 1 for i in range(qm)], axis=1)
    X = np.stack([g.reshape(-1) for g in np.meshgrid(*([pts] * nt), indexing="ij")], axis=1)  # [M^nt, nt]
    s = F64(F32(sigma))
    n0 = 2.0 * s * s
    out = np.zeros((B * R, nt, qm))
    chunk = max(1, (1 << 21) // (len(X) * nr))
    for i in range(0, B * R, chunk):
        e = Y[i:i + chunk, None, :] - np.einsum("nrt,ct->ncr", H[i:i + chunk], X)
        d = (e.real ** 2 + e.imag ** 2).sum(axis=2).reshape((-1,) + (M,) * nt)
        for k in range(nt):
            pk = d.min(axis=tuple(a + 1 for a in range(nt) if a != k))  # [n, M]: the minimum for each point of layer k
            for b in range(qm):
                out[i:i + chunk, k, b] = (pk[:, bit[:, b] == 0].min(axis=1) - pk[:, bit[:, b] == 1].min(axis=1)) / n0
    return out.reshape(B, R * nt * qm)


def ml_bound(y, table, qm, sigma, L, llr64):
    """the bound of the module docstring on |detect_ml - detect_exhaustive64|, [B, R*nt*qm] (inf where dz > A)"""
    y = np.abs(np.asarray(y, dtype=F32).astype(F64))
    B, R, nr = y.shape[:3]
    h = np.abs(mm.per_re(np.asarray(table, dtype=F32), R, L).astype(F64))  # [B, R, nr, nt, 2]
    nt, hh = h.shape[3], qm // 2
    A = F64(qm_.scale(qm))
    xm = (2 ** hh - 1) * A
    h1 = h[..., 0] + h[..., 1]  # |Re| + |Im|, [B, R, nr, nt]
    S = y.max(axis=-1) + h1.sum(axis=-1) * xm  # [B, R, nr]
    dl = ((1 + U) ** (nt + 2) - 1) * S
    dd = (2 * (2 * S * dl + dl ** 2)).sum(axis=-1) + ((1 + U) ** (2 * nr + 1) - 1) * (2 * (S + dl) ** 2).sum(axis=-1)
    ex = np.zeros_like(dd)
    if nt > 1:
        rho = (1 + U) ** (nr + 4) - 1
        for s in (nt - 1, 0):
            g = (h[..., s, :] ** 2).sum(axis=(-1, -2))
            hs = h1[..., s]
            dnum = (hs * dl).sum(axis=-1) + ((1 + U) ** (nr + 2) - 1) * (hs * (S + dl)).sum(axis=-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                dz = np.where(g > 0, dnum / g * (1 + rho), 0.0) + (2 ** hh + 1) * A * rho + 2 * A * 5 * U * (2 ** hh + 2)
            e = np.where(g > 0, np.where(dz <= A, g * 2 * (4 * A * dz), np.inf), 0.0)
            ex = np.maximum(ex, e)
    s = F64(F32(sigma))
    E = np.repeat(dd + ex, nt * qm, axis=-1).reshape(B, R * nt * qm)
    k3 = (1 + U) ** 3
    return 2 * E / (2.0 * s * s) * k3 + np.abs(llr64) * (k3 - 1)


def lmmse_orthogonal_bound(y, table, qm, sigma, L, llr64):
    """the bound of the module docstring on |mimo_model.detect_maxlog - LLR*| for channels with exactly orthogonal columns,
    [B, R*nt*qm]"""
    y = np.asarray(y, dtype=F32).astype(F64)
    B, R, nr = y.shape[:3]
    h = mm.per_re(np.asarray(table, dtype=F32), R, L).astype(F64)
    nt, hh = h.shape[3], qm // 2
    u1 = U + 2.0 ** -47
    lv = qm_.dim_levels(qm)[0].astype(F64)
    xm = np.abs(lv).max()
    s = F64(F32(sigma))
    n0 = 2.0 * s * s
    Hc = h[..., 0] + 1j * h[..., 1]  # [B, R, nr, nt]
    Yc = y[..., 0] + 1j * y[..., 1]  # [B, R, nr]
    gram = np.einsum("...rj,...rk->...jk", np.conj(Hc), Hc)
    assert not (gram * (1 - np.eye(nt))).any(), "the columns are not exactly orthogonal"
    g = np.real(np.einsum("...kk->...k", gram))  # [B, R, nt]
    W = np.conj(np.swapaxes(Hc, -1, -2)) / (g + n0)[..., None]  # [B, R, nt, nr]
    mu = g / (g + n0)
    with np.errstate(divide="ignore"):
        w = np.where(g > 0, (g + n0) ** 2 / np.where(g > 0, g * n0, 1.0), 0.0)
    x = np.einsum("...kr,...r->...k", W, Yc)
    Sx = np.einsum("...kr,...r->...k", np.abs(W.real) + np.abs(W.imag), np.abs(Yc.real) + np.abs(Yc.imag))
    dx = ((1 + u1) * (1 + U) ** (nr + 1) - 1) * Sx
    dlv = ((1 + u1) * (1 + U) - 1) * mu * xm
    out = np.zeros((B, R, nt, qm))
    k5 = (1 + u1) ** 5
    ref = np.abs(llr64).reshape(B, R, nt, qm)
    for dim, xc in enumerate((x.real, x.imag)):
        T = np.abs(xc[..., None] - mu[..., None] * lv).max(axis=-1)
        dt = dx + dlv + U * (T + dx + dlv)
        dd = 2 * T * dt + dt ** 2 + U * (T + dt) ** 2
        out[..., dim::2] = (2 * dd * w * k5)[..., None] + ref[..., dim::2] * (k5 - 1)
    return out.reshape(B, R * nt * qm)


def unitary(nt, nr):
    """complex [nr, nt]: nt exactly orthogonal columns with entries 1, i, -1: (the first nt columns of) the Kronecker
    powers of [[1, i], [i, 1]]"""
    u = np.array([[1, 1j], [1j, 1]])
    m = {1: np.ones((1, 1), dtype=complex), 2: u, 4: np.kron(u, u)}[nr]
    return m[:, :nt]
