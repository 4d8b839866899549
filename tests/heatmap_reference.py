"""fp64 model of ampconv_attn_heatmap and the bar its GPU tests hold the kernels to (tests/test_gpu_heatmap_kernel.py),
written from the wording of include/ampconv.h ("attn_heatmap").

TEST INFRASTRUCTURE.  Plain numpy on LOGICAL arrays; the per-edge weights are linear_reference.attn_weights, not restated
here.  For every edge e = (s -> d) that is not masked (mask given and mask[e] == 0) and whose ids both lie in [0, N),
destination token i and source token j with r = rowpos[s, j] in [0, rows) and c = colpos[d, i] in [0, cols):
    S[r, c] += W[e, i, j];   cnt[r, c] += 1
ROW = position of the SOURCE token, COLUMN = position of the DESTINATION token.  The kernels add rint(W 2^SHIFT) as
integers; `share` is the project's flat bar for one weight (linear_reference.ATOL, RTOL: what attn_weights' own kernels
are held to) summed over the terms of a cell, plus the fixed point's half quantum per term.  It is not tuned to what
the kernels give.  tests/test_heatmap_reference_cpu.py pins the model to the reference's fixtures and shows what the
bar rejects.
"""
import numpy as np

import linear_reference as lr

SHIFT = 28                      # AMPCONV_HEATMAP_SHIFT (the GPU tests hold the loaded build to it)
ATOL, RTOL = lr.ATOL, lr.RTOL


def live_edges(src, dst, N, mask=None):
    """Indices of the edges the call does not ignore."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    ok = (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return np.flatnonzero(ok)


def accumulate(W, src, dst, rowpos, colpos, rows, cols, dtype=np.float64):
    """The tables of the edges (src[e] -> dst[e]), all of them live, from their weights W [E, L, L] (W[e, i, j]:
    destination token i, source token j): (sum [rows, cols] of `dtype`, cnt int64).  Vectorised over (i, j)."""
    rowpos, colpos = np.asarray(rowpos, np.int64), np.asarray(colpos, np.int64)
    S, cnt = np.zeros(rows * cols, dtype), np.zeros(rows * cols, np.int64)
    for e in range(len(src)):
        r, c = np.broadcast_arrays(rowpos[src[e]][None, :], colpos[dst[e]][:, None])          # [i, j]
        ok = (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
        flat = (r * cols + c)[ok]
        np.add.at(S, flat, W[e][ok])
        np.add.at(cnt, flat, 1)
    return S.reshape(rows, cols), cnt.reshape(rows, cols)


def heat_tables(Q, K, src, dst, N, mask, rowpos, colpos, rows, cols, weights=None):
    """(S float64, cnt int64) [rows, cols] of one call on zeroed tables.  Q, K [N', L, H, dh] (N' >= N); mask [E] or None;
    rowpos, colpos [N', L].  weights: a dict {(s, d): W of an edge s -> d} the caller keeps between calls on the SAME
    Q and K (an edge's weights depend on neither the maps nor the edge list around it)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    live = live_edges(src, dst, N, mask)
    if weights is None:
        W = lr.attn_weights(Q, K, src[live], dst[live])[0]
    else:
        pairs = list(zip(src[live].tolist(), dst[live].tolist()))
        new = sorted(set(pairs) - weights.keys())
        if new:
            s, d = np.array(new, np.int64).T
            weights.update(zip(new, lr.attn_weights(Q, K, s, d)[0]))
        L = np.asarray(Q).shape[1]
        W = np.stack([weights[p] for p in pairs]) if pairs else np.zeros((0, L, L))
    return accumulate(W, src[live], dst[live], rowpos, colpos, rows, cols)


def quantised(W):
    """rint(W 2^SHIFT) as int64: what the kernels add for a weight W they hold exactly."""
    return np.rint(np.asarray(W, np.float64) * 2.0 ** SHIFT).astype(np.int64)


def share(sum_, cnt, S, cnt_ref):
    """The bar: inf unless cnt == cnt_ref exactly and every cell without a term holds sum == 0; otherwise the maximum
    over the cells of |sum / 2^SHIFT - S| / (cnt (ATOL + 2^-(SHIFT + 1)) + RTOL S).  At most 1 passes."""
    sum_, cnt, cnt_ref = np.asarray(sum_, np.int64), np.asarray(cnt, np.int64), np.asarray(cnt_ref, np.int64)
    S = np.asarray(S, np.float64)
    assert sum_.shape == cnt.shape == S.shape == cnt_ref.shape, (sum_.shape, cnt.shape, S.shape, cnt_ref.shape)
    if not np.array_equal(cnt, cnt_ref) or sum_[cnt_ref == 0].any():
        return np.inf
    has = cnt_ref > 0
    if not has.any():
        return 0.0
    err = np.abs(sum_[has] / 2.0 ** SHIFT - S[has])
    return float((err / (cnt_ref[has] * (ATOL + 2.0 ** -(SHIFT + 1)) + RTOL * S[has])).max())


def coverage(cnt):
    """Share of the cells with at least one term: a test of (nearly) empty tables proves nothing."""
    return float((np.asarray(cnt) != 0).mean())


# ---------------------------------------------------------------------------------------------------- position maps
def unique_maps(N, L):
    """rowpos[n, j] = colpos[n, j] = n L + j, rows = cols = N L: the table is a full read-out of every W[e, i, j], and
    only multi-edges share a cell."""
    pos = np.arange(N * L, dtype=np.int32).reshape(N, L)
    return pos, pos.copy(), N * L, N * L


def token_maps(N, L):
    """rows = cols = L, rowpos[n, j] = (j + n) % L, colpos[n, i] = (i + 3 n) % L: every token selected, ONE edge already
    fills every cell -- the map for the shortest edge lists."""
    n, t = np.arange(N)[:, None], np.arange(L)[None, :]
    return ((t + n) % L).astype(np.int32), ((t + 3 * n) % L).astype(np.int32), L, L


def selected_maps(N, L, rows=48, cols=64, seed=0, vocab=None):
    """Seeded token features from a vocabulary with repeats inside nodes and two different seeded feature lists of `rows`
    source and `cols` destination features: (rowpos, colpos, rows, cols, tok).  Tokens whose feature is in neither list
    get -1."""
    vocab = max(rows, cols) * 5 // 4 if vocab is None else vocab
    rng = np.random.default_rng(4001 + 97 * L + N + 7919 * seed)
    tok = rng.integers(0, vocab, (N, L))
    pos_r, pos_c = np.full(vocab, -1, np.int32), np.full(vocab, -1, np.int32)
    pos_r[rng.permutation(vocab)[:rows]] = np.arange(rows)
    pos_c[rng.permutation(vocab)[:cols]] = np.arange(cols)
    return pos_r[tok], pos_c[tok], rows, cols, tok
