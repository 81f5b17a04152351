"""numpy model of the flat block-fading QAM channel with perfect CSI for the tests, written from the definitions of
include/nldpc.h, never from the library, on oracle.philox and qam_model:

  n_blocks / block_index        the fading blocks of a row and each symbol's block
  gain_of_words / gains         the Rician gain of a pair of Philox words, and the drawn table [B, n_blk]
  symbol_gains                  a table [B, n_blk] spread over the symbols [B, S]
  faded_symbols                 r = (float)((double)fl32(g * level) + (double)sigma * n), n the AWGN channel's normals
  maxlog_csi                    the fp32 max-log demapper on the levels fl32(g * l), with the stated roundings
  logmap64_csi                  the fp64 log-MAP demapper on the same fp32 levels, and D = max |d w| per LLR

The log-MAP bound is qam_model.logmap_bound unchanged: its derivation starts from fp32 levels l and an fp32 received x
that are INPUTS of both the fp32 demapper and the fp64 model (step 1 there is t = fl(x - l)), and nothing in it uses
what the levels are.  Here the scaled levels fl32(g * l) are computed once in fp32 -- that multiply is part of the
definition, not an error of the demapper -- and handed to the fp64 model as they are, so every step of the derivation
holds with D taken over the scaled levels.
"""
import numpy as np

import qam_model as qm_
from oracle.philox import philox4x32_10

TAG = 0x46414431  # counter word 2 of the gain stream ("FAD1")


def n_blocks(S, L):
    return -(-S // L)


def block_index(S, L):
    """int64 [S]: the in-row fading block of every symbol of a row"""
    return np.arange(S, dtype=np.int64) // L


def gain_of_words(K, r0, r1):
    """fp32: the gain of the Philox words (r0, r1) (uint32 arrays), everything in double, one rounding to fp32"""
    K = np.float64(K)
    u0 = (r0.astype(np.float64) + 1.0) * (1.0 / 4294967296.0)
    u1 = (r1.astype(np.float64) + 1.0) * (1.0 / 4294967296.0)
    rad, th = np.sqrt(-2.0 * np.log(u0)), 6.283185307179586 * u1
    a, b = rad * np.cos(th), rad * np.sin(th)
    mu, s = np.sqrt(K / (K + 1.0)), np.sqrt(1.0 / (2.0 * (K + 1.0)))
    x, y = mu + s * a, s * b
    return np.sqrt(x * x + y * y).astype(np.float32)


def block_words(n, seed, first=0):
    """uint32 [n, 2]: the word pairs of the global blocks first .. first + n - 1: counter (lo32(Gf >> 1), hi32(Gf >> 1),
    TAG, 0), words (x, y) for an even Gf and (z, w) for an odd one"""
    G = np.arange(first, first + n, dtype=np.int64)
    pairs = np.unique(G >> 1)
    ctr = np.zeros((len(pairs), 4), dtype=np.uint32)
    ctr[:, 0] = (pairs & 0xFFFFFFFF).astype(np.uint32)
    ctr[:, 1] = (pairs >> 32).astype(np.uint32)
    ctr[:, 2] = TAG
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1, 2)  # by block from 2 * pairs[0]
    return r[G - 2 * pairs[0]]


def gains(B, S, L, K, seed, b_offset=0):
    """fp32 [B, n_blk]: global block Gf = (b_offset + b) * n_blk + k"""
    nb = n_blocks(S, L)
    w = block_words(B * nb, seed, b_offset * nb)
    return gain_of_words(K, w[:, 0], w[:, 1]).reshape(B, nb)


def symbol_gains(table, S, L):
    """fp32 [B, S] from a table [B, n_blk]"""
    return np.asarray(table, dtype=np.float32)[:, block_index(S, L)]


def faded_symbols(f, qm, sigma, table, L, seed, b_offset=0):
    """fp32 [B, S, 2]: one fp32 rounding of g * level, then one rounding of the double sum"""
    lv = qm_.modulate(f, qm)
    B, S = lv.shape[:2]
    gl = symbol_gains(table, S, L)[..., None] * lv
    assert gl.dtype == np.float32
    return (gl.astype(np.float64) + np.float64(np.float32(sigma)) * qm_.normals(B, S, seed, b_offset)).astype(np.float32)


def _levels(qm, g):
    """fp32 [B, S, 1, 2^h]: fl32(g * l) of every symbol, and the labels"""
    lv, lab = qm_.dim_levels(qm)
    glv = np.asarray(g, dtype=np.float32)[..., None, None] * lv
    assert glv.dtype == np.float32
    return glv, lab


def maxlog_csi(sym, qm, sigma, g):
    """fp32 [B, S, 2] and gains per symbol [B, S] -> fp32 [B, S*qm]: qam_model.maxlog on the scaled levels"""
    glv, lab = _levels(qm, g)
    h, w = qm // 2, qm_.weight(sigma)
    x = np.asarray(sym, dtype=np.float32)
    t = x[..., None] - glv  # [B, S, 2, 2^h], float32 - float32
    d = t * t
    assert d.dtype == np.float32
    out = np.zeros(x.shape[:-1] + (qm,), dtype=np.float32)
    for k in range(h):
        llr = (d[..., lab[:, k] == 0].min(axis=-1) - d[..., lab[:, k] == 1].min(axis=-1)) * w
        out[..., 2 * k] = llr[..., 0]
        out[..., 2 * k + 1] = llr[..., 1]
    assert out.dtype == np.float32
    return out.reshape(x.shape[0], -1)


def logmap64_csi(sym, qm, sigma, g):
    """fp64 log-MAP LLRs [B, S*qm] of fp32 symbols on the fp32 levels fl32(g * l), and D = max |d w| of each LLR's
    dimension (same shape)"""
    glv, lab = _levels(qm, g)
    h, w = qm // 2, np.float64(qm_.weight(sigma))
    x = np.asarray(sym, dtype=np.float32).astype(np.float64)
    d = (x[..., None] - glv.astype(np.float64)) ** 2
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
    return out.reshape(x.shape[0], -1), dmax.reshape(x.shape[0], -1)
