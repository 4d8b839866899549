"""fp64 models of the eight C calls around the softmax-free edge phase, one call each, written from the wording of
include/ampconv.h: ampconv_linear_outer, ampconv_linear_apply, ampconv_gather_segment_sum, ampconv_segment_mean,
ampconv_mask_rows, ampconv_masked_colsum, ampconv_attn_scores, ampconv_attn_weights.

TEST INFRASTRUCTURE.  Plain numpy on LOGICAL arrays (tiles [N, L, H, dh], matrices M [N, H, dh, dh], rows [R, F]);
loops over nodes, heads and edges with 2-D products.  Nothing here imports the library, torch or the oracle:
tests/test_linear_reference_cpu.py composes the models into the layer and pins that to oracle/ampconv_numpy.py.

Every model that sums returns (value, S): S is the sum of the ABSOLUTE values of the terms of each output element,
after every scale the definition applies -- what the forward-error bound of a floating-point sum is stated in.

The second half holds what the GPU tests of these calls share and the CPU mutant test holds to account: the two kinds
of input (exact: small integers and powers of two, every product and partial sum exact in fp32 in any order; random:
N(0, 1)) and the bars
    exact    bit-equal to the model cast to fp32; where a mean divides by a degree that is no power of two, within
             2 ulp of fl32(sum / deg) (one rounding of the reciprocal, one of the product)
    random   |got - ref| <= (n + 4) 2^-24 S, n = the longest chain of additions the definition implies (the forward
             error of an fp32 dot product; the 4: scale, reciprocal, final add)
    colsum   |got - ref| <= 1e-6 max_c sum |x| + 1e-6 (tests/test_gpu_proj.py's column-sum bar)
    weights  conftest.ATOL / RTOL flat and rows that sum to 1 within 1e-5 (tests/test_gpu_planes.py)
None of them is tuned to what the kernels give.
"""
import numpy as np

U = 2.0 ** -24                  # unit round-off of fp32
ATOL, RTOL = 1e-5, 1e-4         # = conftest.ATOL, RTOL (tests/test_linear_reference_cpu.py holds them equal)


# ------------------------------------------------------------------------------------------------------ the models
def linear_outer(A, B, scale):
    """M[n, h] = scale * A[n, :, h]^T B[n, :, h]  ->  (M, S) [N, H, dh, dh]."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    N, L, H, dh = A.shape
    M, S = np.zeros((N, H, dh, dh)), np.zeros((N, H, dh, dh))
    for n in range(N):
        for h in range(H):
            M[n, h] = scale * (A[n, :, h].T @ B[n, :, h])
            S[n, h] = abs(scale) * (np.abs(A[n, :, h]).T @ np.abs(B[n, :, h]))
    return M, S


def linear_apply(A, M, transpose, scale):
    """Out[n, :, h] = scale * A[n, :, h] M[n, h]  (transpose: ... M[n, h]^T)  ->  (Out, S) [N, L, H, dh]."""
    A, M = np.asarray(A, np.float64), np.asarray(M, np.float64)
    N, L, H, dh = A.shape
    out, S = np.zeros((N, L, H, dh)), np.zeros((N, L, H, dh))
    for n in range(N):
        for h in range(H):
            m = M[n, h].T if transpose else M[n, h]
            out[n, :, h] = scale * (A[n, :, h] @ m)
            S[n, :, h] = abs(scale) * (np.abs(A[n, :, h]) @ np.abs(m))
    return out, S


def gather_segment_sum(rows, ptr, idx, w, mean):
    """out[r] = scale_r * sum_{p in [ptr[r], ptr[r + 1])} (w ? w[p] : 1) * rows[idx[p]], scale_r = 1 / segment length if
    `mean` else 1, 0 for empty segments  ->  (out, S) [R, F]."""
    rows = np.asarray(rows, np.float64)
    ptr = np.asarray(ptr, np.int64)
    R = len(ptr) - 1
    out, S = np.zeros((R, rows.shape[1])), np.zeros((R, rows.shape[1]))
    for r in range(R):
        n = ptr[r + 1] - ptr[r]
        if n == 0:
            continue
        sc = 1.0 / n if mean else 1.0
        for p in range(ptr[r], ptr[r + 1]):
            t = rows[idx[p]] * (1.0 if w is None else float(w[p]))
            out[r] += t
            S[r] += np.abs(t)
        out[r] *= sc
        S[r] *= sc
    return out, S


def segment_mean(msg, rowptr, eperm, F):
    """out[n] = mean of msg[eperm[p]] over the CSR segment of n, 0 for empty segments  ->  (out, S) [N, F]."""
    rowptr = np.asarray(rowptr, np.int64)
    N = len(rowptr) - 1
    out, S = np.zeros((N, F)), np.zeros((N, F))
    for n in range(N):
        seg = np.asarray(eperm[rowptr[n]:rowptr[n + 1]], np.int64)
        if len(seg):
            m = np.asarray(msg)[seg].astype(np.float64)
            out[n], S[n] = m.sum(axis=0) / len(seg), np.abs(m).sum(axis=0) / len(seg)
    return out, S


def mask_rows(Y, rowptr):
    """Y [N, F] with the rows whose segment is empty set to +0 (whatever they held); the others as they are."""
    rowptr = np.asarray(rowptr, np.int64)
    out = np.array(Y, copy=True)
    out[rowptr[1:] == rowptr[:-1]] = 0
    return out


def masked_colsum(dY, rowptr):
    """out[c] = sum over the nodes n with a non-empty segment and the tokens l of dY[n, l, c]  ->  (out, S) [D]; the
    rows of the other nodes are not read (they may hold anything)."""
    rowptr = np.asarray(rowptr, np.int64)
    keep = rowptr[1:] != rowptr[:-1]
    x = np.asarray(dY)[keep].astype(np.float64)
    return x.sum(axis=(0, 1)), np.abs(x).sum(axis=(0, 1))


def _scores(Q, K, src, dst):
    Q, K = np.asarray(Q, np.float64), np.asarray(K, np.float64)
    _, L, H, dh = Q.shape
    for e in range(len(src)):
        yield e, [(Q[dst[e], :, h], K[src[e], :, h]) for h in range(H)], 1.0 / np.sqrt(dh), H


def attn_scores(Q, K, src, dst):
    """W[e] = mean_h Q[dst e, :, h] K[src e, :, h]^T / sqrt(dh), original edge order  ->  (W, S) [E, L, L]."""
    L = np.asarray(Q).shape[1]
    W, S = np.zeros((len(src), L, L)), np.zeros((len(src), L, L))
    for e, tiles, c, H in _scores(Q, K, src, dst):
        for q, k in tiles:
            W[e] += q @ k.T * c / H
            S[e] += np.abs(q) @ np.abs(k).T * c / H
    return W, S


def attn_weights(Q, K, src, dst):
    """W[e] = mean_h softmax_rows(Q[dst e, :, h] K[src e, :, h]^T / sqrt(dh))  ->  (W, S) [E, L, L]; the terms of the
    head mean are positive, so S = W."""
    L = np.asarray(Q).shape[1]
    W = np.zeros((len(src), L, L))
    for e, tiles, c, H in _scores(Q, K, src, dst):
        for q, k in tiles:
            s = q @ k.T * c
            p = np.exp(s - s.max(axis=1, keepdims=True))
            W[e] += p / p.sum(axis=1, keepdims=True) / H
    return W, W.copy()


# ------------------------------------------------------------------------------------------------------ the inputs
def tiles(kind, shape, N, seed=0):
    """[N, L, H, dh] float32: 'exact' integers in -3..3, 'random' N(0, 1)."""
    L, dh, H = shape
    rng = np.random.default_rng(1000 * L + 10 * dh + H + 7919 * seed)
    if kind == 'exact':
        return rng.integers(-3, 4, (N, L, H, dh)).astype(np.float32)
    return rng.standard_normal((N, L, H, dh), dtype=np.float32)


def matrices(kind, shape, N, seed=0):
    """M [N, H, dh, dh] float32: 'exact' integers in -7..7, 'random' N(0, 1)."""
    L, dh, H = shape
    rng = np.random.default_rng(31 * L + 10 * dh + H + 104729 * (seed + 1))
    if kind == 'exact':
        return rng.integers(-7, 8, (N, H, dh, dh)).astype(np.float32)
    return rng.standard_normal((N, H, dh, dh), dtype=np.float32)


def rows(kind, R, F, seed=0, lo=-3, hi=3):
    """[R, F] float32 rows: 'exact' integers in lo..hi, 'random' N(0, 1)."""
    rng = np.random.default_rng(R * 65537 + F + 15485863 * (seed + 1))
    if kind == 'exact':
        return rng.integers(lo, hi + 1, (R, F)).astype(np.float32)
    return rng.standard_normal((R, F), dtype=np.float32)


def pow2_weights(E, seed=0):
    """E float32 weights out of {1, 1/2, 1/4, 1/8}: every product with a small integer is exact."""
    return (2.0 ** -np.random.default_rng(977 + seed).integers(0, 4, E)).astype(np.float32)


def poison(a, which, seed=0):
    """`a` with the rows `which` (a boolean mask over the first axis) filled with NaN, +inf and -inf in turn: what a
    masked path must neither read into a result nor multiply by 0."""
    a = np.array(a, copy=True)
    bad = np.array([np.nan, np.inf, -np.inf], dtype=a.dtype)
    flat = a.reshape(len(a), -1)
    flat[which] = bad[(np.arange(flat.shape[1]) + seed) % 3]
    return a


def to_bf16(x):
    """float32 -> the nearest bf16 value (ties to even), as float32.  Finite inputs."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


# -------------------------------------------------------------------------------------------------------- the bars
def _ordered(x32):
    """float32 -> int64 that grows with the value, one step per representable number (+0 and -0 coincide)."""
    b = np.ascontiguousarray(x32, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def ulp_distance(got, want):
    """Representable fp32 numbers between got and want, elementwise; a non-finite value on either side that the other
    does not hold bit for bit counts as infinitely far."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    d = np.abs(_ordered(got) - _ordered(want)).astype(np.float64)
    odd = ~(np.isfinite(got) & np.isfinite(want)) & (got.view(np.int32) != want.view(np.int32))
    d[odd] = np.inf
    return d


def exact_problems(got, ref, loose=None):
    """The exact bar: got (float32) against the fp64 model `ref`.  Bit-equal to fl32(ref) (a zero of the model is +0,
    what a sum that starts at +0 gives) except where `loose` (a boolean array that broadcasts against got: the
    elements whose mean divides by a degree that is no power of two) allows 2 ulp.  -> the number of elements that
    miss it."""
    got = np.ascontiguousarray(got, np.float32)
    want = (np.asarray(ref, np.float64) + 0.0).astype(np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    same = got.view(np.int32) == want.view(np.int32)
    if loose is not None:
        same = same | (np.broadcast_to(loose, got.shape) & (ulp_distance(got, want) <= 2))
    return int((~same).sum())


def random_share(got, ref, S, n):
    """The random bar: max over the elements of |got - ref| / ((n + 4) 2^-24 S) -- at most 1 passes; n a number or an
    array that broadcasts against got.  An element whose bound is 0 (no terms) must be exactly 0; NaN or infinity in
    got: inf."""
    got, ref, S = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    if not got.size:
        return 0.0
    if not np.isfinite(got).all():
        return np.inf
    bound = (np.broadcast_to(np.asarray(n, np.float64), got.shape) + 4) * U * S
    err = np.abs(got - ref)
    share = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(share.max())


def colsum_share(got, ref, S):
    """The column-sum bar of tests/test_gpu_proj.py: max |got - ref| / (1e-6 max_c S + 1e-6); at most 1 passes."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return np.inf
    return float(np.abs(got - ref).max() / (1e-6 * float(np.max(S)) + 1e-6)) if got.size else 0.0


def weights_share(got, ref):
    """attn_weights' bar: max of |got - ref| / (ATOL + RTOL |ref|) and of |row sum - 1| / 1e-5; at most 1 passes."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return np.inf
    if not got.size:
        return 0.0
    return float(max((np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))).max(), np.abs(got.sum(-1) - 1.0).max() / 1e-5))


def pow2(deg):
    """Which of the degrees are powers of two (a mean over them is exact in fp32 on exact data); 0: True."""
    deg = np.asarray(deg, np.int64)
    return (deg & (deg - 1)) == 0
