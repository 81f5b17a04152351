"""Special-value inputs for the decoder tests (a plain helper module, no tests in it).

The suite's usual inputs are continuous Gaussian LLR draws with weights in [0.5, 1.5): they never hold
an exact zero, a tie, a value at or beyond the +-20 clamp, a -0.0, or a weight that kills a message.
`edge_batch` builds one batch in which each of the first six codewords carries one such property, and
`edge_cn_weights` / `edge_neural_params` build weights with exact zeros, negatives and clearly negative
biases.  tests/test_edge_inputs.py asserts on the CPU oracle that the batch really reaches the cases
(ties, zeros before the zero fix, posteriors at the clamp, ReLU-killed messages, clipped SP products).

Codeword 0   all zeros (an erased word; in the Neural check node every min is the 10000 mask value)
Codeword 1   the first two columns exactly 0 (the NR puncturing)
Codeword 2   rounded to integers (ties and exact zeros on a continuous-kind decoder)
Codeword 3   sign(x) * 20 (on the clamp and on the closed-interval STE boundary)
Codeword 4   10 * x (far beyond the clamp; saturates SP)
Codeword 5   every second lifted copy is -0.0
Codeword 6+  the plain Gaussian draw
"""
import torch

SEED = 5  # the seed the suite uses: every coverage count of tests/test_edge_inputs.py is positive with it
N_SPECIAL = 6


def gaussian_llr(B, N, Z, seed):
    """The suite's usual channel: all-zero codeword (bit 0 -> -1), sigma 0.9, LLR = 2 y / sigma^2."""
    gen = torch.Generator().manual_seed(seed)
    return (2 * (-1 + 0.9 * torch.randn(B, N, Z, generator=gen)) / 0.81).float()


def edge_batch(B, N, Z, seed=SEED, rows=None):
    """xa [B, N, Z] fp32: codeword b carries property rows[b] of the module docstring (rows = 0, 1, 2, ... when
    not given; a batch too small for all six names the ones it wants), the others stay Gaussian."""
    x = gaussian_llr(B, N, Z, seed)
    rows = list(range(N_SPECIAL)) if rows is None else list(rows)
    for b, p in enumerate(rows[:B]):
        if p == 0:
            x[b] = 0.0
        elif p == 1:
            x[b, :2] = 0.0
        elif p == 2:
            x[b] = torch.round(x[b])
        elif p == 3:
            x[b] = torch.where(x[b] < 0, torch.full_like(x[b], -20.0), torch.full_like(x[b], 20.0))
        elif p == 4:
            x[b] = 10.0 * x[b]
        elif p == 5:
            x[b, :, 1::2] = -0.0
    return x


def _kill(w):
    """Every 7th entry (flat order) exactly 0, every 11th starting at 3 negated."""
    f = w.reshape(-1)
    f[0::7] = 0.0
    f[3::11] = -f[3::11]
    return w


def edge_cn_weights(T, E, seed=SEED):
    """[T, E] check-node weights drawn as the suite draws them, [0.5, 1.5), with zeros and negatives."""
    gen = torch.Generator().manual_seed(1000 + seed)
    return _kill(0.5 + torch.rand(T, E, generator=gen))


def edge_vn_weights(T, N, seed=SEED):
    """[T, N] per-column VN weights as the suite draws them, [0.8, 1.2)."""
    gen = torch.Generator().manual_seed(2000 + seed)
    return 0.8 + 0.4 * torch.rand(T, N, generator=gen)


def edge_neural_params(T, E, seed=SEED):
    """Neural (weights, biases), each [T, E]: weights in [0, 1.2) with zeros and negatives, biases
    N(0, 0.1) with every 5th entry -0.5 so that the ReLU mask kills messages."""
    gen = torch.Generator().manual_seed(3000 + seed)
    w = _kill(torch.rand(T, E, generator=gen) * 1.2)
    b = torch.randn(T, E, generator=gen) * 0.1
    b.reshape(-1)[0::5] = -0.5
    return w, b


def per_codeword_diff(o, ref):
    """'codeword b: n' for every codeword of [T, B, ...] arrays in which values differ (bitwise compare
    through ==; a failure message that names the failing property)."""
    import numpy as np
    o, ref = np.asarray(o), np.asarray(ref)
    bad = (o != ref).reshape(o.shape[0], o.shape[1], -1).sum(axis=(0, 2))
    return ", ".join(f"codeword {b}: {int(n)}" for b, n in enumerate(bad) if n) or "none"
