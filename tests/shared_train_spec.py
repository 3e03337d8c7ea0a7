"""Exact restatement of es_rows_scatter_sum (csrc/transformer.hip): per scene row the gradients of the prompts that selected it, added in
f32 from +0 in ascending prompt order; with `accumulate` that sum is then added to what the row held.  numpy f32 additions are IEEE
round-to-nearest single additions, so the comparison with the kernel is BIT FOR BIT (signs of zero included)."""
import numpy as np


def scatter_sum_ref(dy, idx, L, accumulate=0, dx0=None):
    """dy (P*Q, C) f32, idx (P, Q) int (distinct within a row; entries outside [0, L) select nothing) -> dx (L, C) f32"""
    dy = np.asarray(dy, np.float32)
    idx = np.asarray(idx, np.int64)
    P, Q = idx.shape
    C = dy.shape[1]
    assert dy.shape[0] == P * Q
    out = np.zeros((L, C), np.float32)                       # +0
    for p in range(P):                                       # ascending p: the order IS the specification
        for q in range(Q):
            l = int(idx[p, q])
            if 0 <= l < L:
                out[l] = out[l] + dy[p * Q + q]
    if accumulate:
        out = np.asarray(dx0, np.float32) + out              # after the prompt sum is formed
    return out


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)
