"""The two MLPs of a dense probe model (tests/dense_model.py) restated in float64, with the certificate that makes the
restatement exact (helper of test_dense_cpu.py and test_dense_gpu.py; numpy only, no test in it).

The arithmetic contract (oracle/nerf_oracle.cpp mlp_one, shared with the HIP path): per layer the dot products of fp16
inputs with the weights accumulated in fp32, the activation on the sum, one fp16 store (round to nearest even); the density
network's 16 outputs g, stored as fp16, are columns 0..15 of the rgb network's input, the direction encoding follows.

CERTIFICATE, per sample and neuron.  The weights are integers (+-1, and the 11 of the sigma route), so every product is an
integer multiple of an input.  Let q be the largest power of two that divides every input with a non-zero weight and
S = sum |w| |x|.  If S < 2^24 q, every partial sum of the products, in any order and grouping, is a multiple of q of magnitude
below 2^24 q: exactly representable in fp32 (24 significant bits).  So ANY fp32 accumulation -- the oracle's ascending k, an
MFMA's internal one -- returns the exact sum, and the fp16 store that follows is determined.  A sample is certified when every
neuron of every layer of both networks passes; there kernel, oracle and `chain` below must agree bit for bit.  (float64
holds such a sum exactly as well: 53 bits.)

Mutated chains (`store`, `acc_block`, changed matrices or inputs) give what a wrong MLP would show; test_dense_cpu.py proves
that each differs from the right one on at least half of the certified pixels of every frame."""
from __future__ import annotations

import numpy as np

STORE_RNE, STORE_SKIP, STORE_RTZ = "rne", "skip", "rtz"


def _to_f16(x, rounding):
    """x rounded to a multiple of its fp16 ulp, 2^(max(e, -14) - 10) for 2^e <= |x| < 2^(e + 1): scaling by a power of two is
    exact, `rounding` (np.rint: ties to even; np.trunc: toward zero) does the one rounding.  (numpy's own float64 -> float16
    cast gives the same values -- test_dense_cpu.py compares them -- at fifty times the cost.)"""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)  # |x| = m 2^e, m in [0.5, 1)
    ulp = np.maximum(e - 1, -14) - 10
    r = np.ldexp(rounding(np.ldexp(x, -ulp)), ulp)
    big = np.abs(r) >= 65520.0  # past the largest fp16 value by half an ulp or more
    if big.any():
        r = np.where(big, np.copysign(np.inf if rounding is np.rint else 65504.0, x), r)
    return r


def f16(x):
    """float64 -> the nearest fp16 value (ties to even), as float64: one rounding."""
    return _to_f16(x, np.rint)


def f16_toward_zero(x):
    """float64 -> the fp16 value next to it toward zero (a truncating conversion)."""
    return _to_f16(x, np.trunc)


def quantum(x):
    """The largest power of two that divides each fp16 value of x (float64 holding fp16 values); +inf for 0."""
    x = np.abs(np.asarray(x, np.float64))
    m, e = np.frexp(x)  # x = m 2^e, m in [0.5, 1): an fp16 value's m has at most 11 bits
    M = (m * 2048.0).astype(np.int64)
    assert np.array_equal(M.astype(np.float64), m * 2048.0), "not fp16 values"
    low = (M & -M).astype(np.float64)
    return np.where(x == 0.0, np.inf, np.ldexp(low, e - 11))


def layer_certificate(w, x):
    """[n][n_out] bool: S < 2^24 q for the neuron's sum (module docstring).  w [n_out][n_in] integers, x [n][n_in] fp16 values."""
    assert np.array_equal(w, np.rint(w))
    q, S = quantum(x), np.abs(x) @ np.abs(w).T
    ok = np.empty(S.shape, bool)
    for o in range(w.shape[0]):
        cols = np.flatnonzero(w[o])
        qo = q[:, cols].min(axis=1) if len(cols) else np.full(len(x), np.inf)
        ok[:, o] = S[:, o] < 2.0 ** 24 * qo
    return ok


def _dot(w, x, acc_block):
    """The exact dot products (float64; exact on certified samples), or with an fp16 accumulator that is rounded after every
    `acc_block` products (the oracle's set_mlp_accumulate arithmetic: the block's products and the accumulator summed, one
    fp16 rounding)."""
    if not acc_block:
        return x @ w.T
    acc = np.zeros((len(x), w.shape[0]))
    for k in range(0, w.shape[1], acc_block):
        acc = f16(acc + x[:, k:k + acc_block] @ w[:, k:k + acc_block].T)
    return acc


def _mlp(mats, x, act, store, acc_block, certify, hidden):
    ok = np.ones(len(x), bool)
    for i, w in enumerate(mats):
        w = w.astype(np.float64)
        last = i == len(mats) - 1
        if certify:
            ok &= layer_certificate(w, x).all(axis=1)
        y = _dot(w, x, acc_block)
        if act == "ReLU" and not last:
            y = np.maximum(y, 0.0)
        # the outputs of a network are stored as fp16 in every variant: the mutations are of the HIDDEN store
        x = f16(y) if last or store == STORE_RNE else (y if store == STORE_SKIP else f16_toward_zero(y))
        if not last:
            hidden.append(x)
    return x, ok


def chain(D, R, act, feat, dirf, store=STORE_RNE, acc_block=0, certify=True):
    """feat [n][feat_w], dirf [n][dir_w]: fp16 values.  Returns dict(rgb float32 [n][3], g [n][16], certified [n],
    hidden: every hidden layer's stored activations, density network first).  Column order of the rgb input: g, then the
    direction encoding as the oracle lays it out (padding ones of SphericalHarmonics first, any other encoding's last)."""
    feat, dirf = np.asarray(feat, np.float64), np.asarray(dirf, np.float64)
    hidden = []
    g, ok_d = _mlp(D, feat, act, store, acc_block, certify, hidden)
    out, ok_r = _mlp(R, np.concatenate([g, dirf], axis=1), act, store, acc_block, certify, hidden)
    return dict(rgb=out[:, :3].astype(np.float32), g=g, certified=ok_d & ok_r, hidden=hidden, n_density_hidden=len(D) - 1)


def move_weight(mats, index, row, col, to):
    """A copy of `mats` with the weight at [row][col] of matrix `index` moved to column `to` of the same row."""
    out = [m.copy() for m in mats]
    m = out[index]
    assert m[row, col] != 0 and m[row, to] == 0
    m[row, to], m[row, col] = m[row, col], 0.0
    return out


def neighbour(m, row, col, avoid=()):
    """The nearest column to `col` that holds no weight in `row` and is not in `avoid`, or None."""
    for d in sorted(range(-m.shape[1], m.shape[1]), key=abs):
        if d and 0 <= col + d < m.shape[1] and m[row, col + d] == 0 and col + d not in avoid:
            return col + d
    return None
