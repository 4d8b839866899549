"""fp64 model of the three edge passes of include/ampconv.h, one pass at a time.

TEST INFRASTRUCTURE.  Plain numpy on LOGICAL arrays [N, L, H, dh]; a loop over destination rows, edges and heads with
2-D matrix products, so that it shares no code (and no einsum formulation) with oracle/ampconv_numpy.py, with torch
autograd or with the kernels.  tests/test_edge_reference_cpu.py pins it against the first two at fp64 round-off.

    fwd   O[r]  = (1 / deg_r) sum_{p in row r} softmax_rows(Q[d] K[s_p]^T / sqrt(dh)) V[s_p],  d = qidx[r] or r; 0 if deg_r = 0
    bwd   with g = dObar[d] / deg_d (dObar is the gradient of the MEAN), P the softmax above, per edge (s -> d), head:
              dV[s] += P^T g;   dP = g V[s]^T;   delta_i = sum_j P_ij dP_ij;   dS = P (dP - delta)
              dQ[d] += dS K[s] / sqrt(dh);   dK[s] += dS^T Q[d] / sqrt(dh)
    stats per (edge, head, destination token i): log2 sum_j exp(S_ij) and delta_i (of the UNSCALED dP above)
"""
import numpy as np


def _rows(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return rowptr, len(rowptr) - 1


def _softmax(s):
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def csr_of(src, dst, n):
    """Destination-sorted CSR (stable) of an edge list: rowptr [n + 1], col [E] = source of each sorted edge."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.argsort(dst, kind='stable')
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=rowptr[1:])
    return rowptr, src[order]


def fwd(Q, K, V, rowptr, col, qidx=None):
    """O [R, L, H, dh] for the R = len(rowptr) - 1 rows."""
    Q, K, V = (np.asarray(t, dtype=np.float64) for t in (Q, K, V))
    rowptr, R = _rows(rowptr)
    _, L, H, dh = Q.shape
    O = np.zeros((R, L, H, dh))
    for r in range(R):
        d = r if qidx is None else int(qidx[r])
        deg = rowptr[r + 1] - rowptr[r]
        for p in range(rowptr[r], rowptr[r + 1]):
            s = int(col[p])
            for h in range(H):
                P = _softmax(Q[d, :, h] @ K[s, :, h].T / np.sqrt(dh))
                O[r, :, h] += P @ V[s, :, h] / deg
    return O


def bwd(Q, K, V, dObar, rowptr, col):
    """dQ, dK, dV [N, L, H, dh]; rows of dObar without in-edges reach nothing."""
    Q, K, V, dObar = (np.asarray(t, dtype=np.float64) for t in (Q, K, V, dObar))
    rowptr, R = _rows(rowptr)
    _, L, H, dh = Q.shape
    dQ, dK, dV = np.zeros_like(Q), np.zeros_like(K), np.zeros_like(V)
    c = 1.0 / np.sqrt(dh)
    for d in range(R):
        deg = rowptr[d + 1] - rowptr[d]
        for p in range(rowptr[d], rowptr[d + 1]):
            s = int(col[p])
            for h in range(H):
                q, k, v, g = Q[d, :, h], K[s, :, h], V[s, :, h], dObar[d, :, h] / deg
                P = _softmax(q @ k.T * c)
                dP = g @ v.T
                dS = P * (dP - (P * dP).sum(axis=1, keepdims=True))
                dV[s, :, h] += P.T @ g
                dQ[d, :, h] += dS @ k * c
                dK[s, :, h] += dS.T @ q * c
    return dQ, dK, dV


def stats(Q, K, V, dObar, rowptr, col):
    """(lse2, delta), each [E, H, L] in CSR edge order: log2-sum-exp of the scaled scores and delta_i of every
    (edge, head, destination token)."""
    Q, K, V, dObar = (np.asarray(t, dtype=np.float64) for t in (Q, K, V, dObar))
    rowptr, R = _rows(rowptr)
    _, L, H, dh = Q.shape
    E = int(rowptr[-1])
    lse2, delta = np.zeros((E, H, L)), np.zeros((E, H, L))
    for d in range(R):
        deg = rowptr[d + 1] - rowptr[d]
        for p in range(rowptr[d], rowptr[d + 1]):
            s = int(col[p])
            for h in range(H):
                S = Q[d, :, h] @ K[s, :, h].T / np.sqrt(dh)
                m = S.max(axis=1)
                lse2[p, h] = (m + np.log(np.exp(S - m[:, None]).sum(axis=1))) / np.log(2.0)
                P = _softmax(S)
                delta[p, h] = (P * ((dObar[d, :, h] / deg) @ V[s, :, h].T)).sum(axis=1)
    return lse2, delta
