"""numpy models of the input side of a batch -- the featuriser (csrc/featurizer.hip) and the GraphSAINT sampler
(csrc/sampler.hip) -- written from the wording of include/ampconv.h, the inputs the GPU tests of those kernels run on,
and the bars they are held to.

TEST INFRASTRUCTURE.  Plain numpy: no torch, no GPU, no call into the library.  tests/test_pipeline_reference_cpu.py
holds the models to the two restatements under oracle/ and to their statistical bar, and shows that every input set
below tells the model from each of its mutants; tests/test_gpu_featurizer_kernels.py and tests/test_gpu_sampler_kernels.py
then hold the kernels to the models.

THE STREAMS (a contract, like the dropout mask): draw(seed, a, b) = splitmix64(seed ^ splitmix64(a * 0x100000001B3 + b)) in
wrapping uint64 arithmetic.  Token l of node n is the (draw(seed, n, l) % count)-th PRESENT column of row n in ascending
order; step t of walk b moves to crow[cscptr[cur] + draw(seed, b, t) % deg] (stays where it is if deg == 0).
PRESENT means x != 0 as numpy decides it for finite values: -0.0 is absent, denormals and negatives are present.  The
library is built with -fno-honor-nans, under which a NaN feature has no defined presence: every input here is finite.

THE BARS, derived, none measured:
    every integer output                equal element for element
    build_tokens fp32                   bit-equal to build_tokens_f32 (a copy and two fp32 operations, one rounding each)
    build_tokens bf16                   bit-equal to the round-to-nearest-even of the fp32 result
    mean, inv_std                       within 1 float32 ulp of the rounded fp64 value (the kernel accumulates in double:
                                        its own error is about N 2^-53, far below half an ulp, so 1 ulp allows for a
                                        rounding boundary between the two fp64 values)
    constant verdict                    equal (the inputs keep every column away from the rule's threshold: zscore_margin)
    z assembled from fp32 mean/inv_std  |z - z64| <= 2^-24 (2 |mean| inv_std + 4 |z|): one ulp on the fp32 mean (half an ulp
                                        of rounding, half of accumulation slack) times inv_std, three roundings on z
                                        (inv_std, the subtraction, the product) and one more for the second-order terms
    table_grad, exact data              bit-equal (small integers times powers of two: every partial sum is exact in
                                        any order)
    table_grad, random data             |got - ref| <= (n + 4) 2^-24 S, n the number of terms, S the sum of their absolute
                                        values (tests/linear_reference.py: the bar for atomics and ordered sums)
    norms                               the branch constants 0.1 and 1e4 bit-exact; edge_norm within 1 ulp (one correctly
                                        rounded division), node_norm within 2 ulp (two) of the float32 model
"""
import math

import numpy as np

from glue_reference import splitmix64
from linear_reference import U, random_share, to_bf16, ulp_distance      # noqa: F401  (the GPU tests take them from here)

_U = np.uint64
MULT = 0x100000001B3
SEEDS = (0, 3, 2 ** 63 + 5)
EPS64 = 2.220446049250313e-16


# ------------------------------------------------------------------------------------------------------ the streams
def draw(seed, a, b):
    """splitmix64(seed ^ splitmix64(a * 0x100000001B3 + b)), uint64, wrapping; a and b broadcast."""
    a, b = np.asarray(a).astype(np.uint64), np.asarray(b).astype(np.uint64)
    with np.errstate(over='ignore'):
        return splitmix64(_U(int(seed) & (2 ** 64 - 1)) ^ splitmix64(a * _U(MULT) + b))


def sample_present(x, L, seed):
    """(idx int32 [N, L], empty flag): idx[n, l] = the (draw(seed, n, l) % count)-th present column of row n, ascending;
    a row without a present column holds -1 throughout and raises the flag."""
    x = np.asarray(x)
    N = x.shape[0]
    idx = np.full((N, L), -1, dtype=np.int32)
    empty = 0
    for n in range(N):
        present = np.nonzero(x[n] != 0)[0]
        if present.size == 0:
            empty = 1
            continue
        idx[n] = present[(draw(seed, n, np.arange(L)) % _U(present.size)).astype(np.int64)]
    return idx, empty


def random_walk(cscptr, crow, start, walk_length, seed):
    """walks int64 [B, walk_length + 1]: walks[b, 0] = start[b]; step t moves along the (draw(seed, b, t) % deg)-th
    out-edge of the current node in CSC order, or stays if the node has none."""
    cscptr, crow = np.asarray(cscptr, np.int64), np.asarray(crow, np.int64)
    B = len(start)
    walks = np.empty((B, walk_length + 1), dtype=np.int64)
    walks[:, 0] = cur = np.asarray(start, np.int64)
    b = np.arange(B)
    for t in range(walk_length):
        beg, deg = cscptr[cur], cscptr[cur + 1] - cscptr[cur]
        r = (draw(seed, b, t) % np.maximum(deg, 1).astype(np.uint64)).astype(np.int64)
        pos = np.where(deg > 0, beg + r, 0)
        cur = np.where(deg > 0, crow[pos] if crow.size else cur, cur)
        walks[:, t + 1] = cur
    return walks


# ---------------------------------------------------------------------------------------------------- the sub-graph
def csc_of(edge_index, N):
    """(cscptr, crow, cperm) of ampconv_graph_build: the edges in the STABLE order of their source
    (tests/test_gpu_parity.py: test_csr_build_is_a_stable_sort pins the library's arrays to exactly this)."""
    src, dst = np.asarray(edge_index, np.int64)
    cperm = np.argsort(src, kind='stable')
    cscptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))])
    return cscptr.astype(np.int32), dst[cperm].astype(np.int32), cperm.astype(np.int32)


def saint_nodes(nodes, N):
    """(mark int32 [N], relabel int32 [N] = exclusive scan of mark, node_idx int64 = the sorted unique nodes, n_sub)."""
    mark = np.zeros(N, dtype=np.int32)
    mark[np.asarray(nodes, np.int64)] = 1
    relabel = (np.cumsum(mark) - mark).astype(np.int32)
    node_idx = np.nonzero(mark)[0].astype(np.int64)
    return mark, relabel, node_idx, int(node_idx.size)


def count_edges(node_idx, n_sub, cscptr, crow, mark, n_bound=None):
    """(cnt, off, e_sub): cnt[k] = out-edges of the k-th sampled node whose destination is sampled, off = its exclusive
    scan.  Both have n_sub + 1 entries (the last count 0, so off[n_sub] = e_sub), or n_bound + 1 with n_bound >= n_sub:
    the entries from n_sub on count 0."""
    n = n_sub if n_bound is None else n_bound
    cnt = np.zeros(n + 1, dtype=np.int32)
    for k in range(n_sub):
        u = node_idx[k]
        cnt[k] = int(np.asarray(mark)[crow[cscptr[u]:cscptr[u + 1]]].sum())
    off = (np.cumsum(cnt) - cnt).astype(np.int32)
    return cnt, off, int(off[n])


def fill_edges(node_idx, n_sub, cscptr, crow, cperm, mark, relabel):
    """(edge_index int64 [2, e_sub], edge_id int64 [e_sub]) at EXACT positions: for the k-th sampled node in ascending k
    its kept CSC entries in CSC order, each as (k, relabel[destination]) with the original edge id cperm[p]."""
    s, d, e = [], [], []
    for k in range(n_sub):
        u = node_idx[k]
        for p in range(cscptr[u], cscptr[u + 1]):
            if mark[crow[p]]:
                s.append(k), d.append(relabel[crow[p]]), e.append(cperm[p])
    return np.array([s, d], dtype=np.int64).reshape(2, -1), np.array(e, dtype=np.int64)


def add_counts(idx, count):
    """count (float32) with 1 added per occurrence in idx: integer-valued below 2^24, hence exact in any order."""
    out = np.asarray(count, np.float64) + np.bincount(np.asarray(idx, np.int64), minlength=len(count))
    assert out.max(initial=0) < 2 ** 24
    return out.astype(np.float32)


def norms(node_count, edge_count, edge_src, N, num_samples):
    """(node_norm, edge_norm) float32: oracle/graphsaint_numpy.norms operation by operation in float32 -- the quotient
    node_count[src] / edge_count, clipped into [0, 1e4], NaN (0 / 0) replaced by 0.1; node counts of 0 replaced by 0.1,
    then num_samples / count / N, two divisions."""
    nc = np.asarray(node_count, np.float32).copy()
    ec = np.asarray(edge_count, np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = nc[np.asarray(edge_src, np.int64)] / ec
    edge_norm = np.minimum(np.maximum(q, np.float32(0)), np.float32(1e4)).astype(np.float32)
    edge_norm[np.isnan(q)] = np.float32(0.1)
    nc[nc == 0] = np.float32(0.1)
    node_norm = (np.float32(num_samples) / nc) / np.float32(N)
    return node_norm.astype(np.float32), edge_norm


# --------------------------------------------------------------------------------------------------- the featuriser
def _column_moments(x):
    """Exactly rounded fp64 mean and population variance of every column (math.fsum)."""
    x = np.asarray(x, np.float64)
    N = x.shape[0]
    mean = np.array([math.fsum(c) / N for c in x.T])
    var = np.array([math.fsum((c - m) ** 2) / N for c, m in zip(x.T, mean)])
    return mean, var


def zscore_bound(mean, var, N):
    """sklearn's constant-feature threshold: a variance at or below it means a constant column (scale 1)."""
    return N * EPS64 * var + (N * mean * EPS64) ** 2


def zscore_stats(x):
    """(mean64, inv_std64, constant): fp64 mean, 1 / sqrt(population variance), and sklearn's verdict
    var <= N eps var + (N mean eps)^2, under which the scale is 1."""
    mean, var = _column_moments(x)
    constant = var <= zscore_bound(mean, var, np.asarray(x).shape[0])
    with np.errstate(divide='ignore'):
        inv_std = np.where(constant, 1.0, 1.0 / np.sqrt(np.where(constant, 1.0, var)))
    return mean, inv_std, constant


def zscore_margin(x):
    """min over the non-constant columns of var / threshold (inf if there is none), and whether every constant column has
    a variance of exactly 0: the distance of the verdicts from the rule's border."""
    mean, var = _column_moments(x)
    bound = zscore_bound(mean, var, np.asarray(x).shape[0])
    const = var <= bound
    return float((var[~const] / bound[~const]).min()) if (~const).any() else np.inf, bool((var[const] == 0).all())


def z_bar(mean64, inv_std64, z64):
    """The bound on |z - z64| for a z assembled in fp32 from the fp32 mean and inv_std."""
    return U * (2 * np.abs(mean64) * inv_std64 + 4 * np.abs(z64))


def build_tokens_f32(x, mean, inv_std, idx, table):
    """float32 [N, L, De + 1], the kernel's expression in numpy float32: the table row copied, the last channel
    (x - mean) * inv_std with one rounding per operation; a token with idx -1 is all +0."""
    x, mean, inv_std = (np.asarray(a, np.float32) for a in (x, mean, inv_std))
    table, idx = np.asarray(table, np.float32), np.asarray(idx, np.int64)
    N, L = idx.shape
    De = table.shape[1]
    out = np.zeros((N, L, De + 1), dtype=np.float32)
    ok = idx >= 0
    f = np.where(ok, idx, 0)
    rows = np.arange(N)[:, None]
    out[..., :De] = table[f]
    out[..., De] = ((x[rows, f] - mean[f]).astype(np.float32) * inv_std[f]).astype(np.float32)
    out[~ok] = 0
    return out


def table_grad(dout, idx, F):
    """(dtable, S, n) [F, De]: fp64 index_add of dout[n, l, :De] into row idx[n, l] (tokens with idx -1 add nothing),
    the sum of the absolute values of the terms, and the number of terms of each row (as [F, 1])."""
    dout, idx = np.asarray(dout, np.float64), np.asarray(idx, np.int64).reshape(-1)
    De = dout.shape[-1] - 1
    g = dout.reshape(-1, De + 1)[idx >= 0][:, :De]
    f = idx[idx >= 0]
    dtable, S = np.zeros((F, De)), np.zeros((F, De))
    np.add.at(dtable, f, g)
    np.add.at(S, f, np.abs(g))
    return dtable, S, np.bincount(f, minlength=F).astype(np.float64)[:, None]


# ========================================================================================================= the inputs
# Everything below builds the inputs of the GPU tests; the CPU mutant test runs models and mutants on the same ones.

# (F, L): every F and every L at least twice; the seeds cycle over SEEDS
SAMPLE_CASES = ((1, 1), (1, 40), (63, 64), (63, 200), (64, 1), (64, 65), (65, 40), (65, 64), (200, 65), (200, 200),
                (200, 40), (1433, 40), (1433, 1), (1433, 200), (1433, 64), (1433, 65))
EMPTY_ROW = 7
N_CONSTRUCTED = 12


def sample_cases():
    return [(F, L, SEEDS[i % 3]) for i, (F, L) in enumerate(SAMPLE_CASES)]


def sample_rows(F):
    """x float32 [72, F], finite: 12 constructed rows, then 60 random sparse ones with at least one present column.
      0 only column 0              1 only column F - 1           2 every column
      3 only columns 63 and 64 (clipped to F - 1)                4 every column but those of chunk 1 (64..127)
      5 negatives only             6 -0.0 (absent) beside denormals (present)
      7 ALL ZERO (-1 and the flag) 8 the first and the last column of every 64-column chunk
      9 every column but column 0  10 columns 0 and F - 1        11 every other column, from column 1 on
    A constructed row that would come out empty at a small F (rows 9 and 11 at F = 1) gets column 0."""
    rng = np.random.default_rng(4000 + F)
    x = np.zeros((N_CONSTRUCTED + 60, F), dtype=np.float32)
    cols = np.arange(F)
    x[0, 0] = 1.5
    x[1, F - 1] = 2.5
    x[2] = rng.random(F) + 0.5
    x[3, [min(63, F - 1), min(64, F - 1)]] = 1.0
    x[4] = np.where((cols >= 64) & (cols < 128), 0.0, rng.random(F) + 0.5)
    x[5, rng.random(F) < 0.3] = -1.25
    x[5, F // 2] = -3.0
    x[6] = -0.0
    denormal = np.array([1e-45, -1e-42, 1e-40, 1.1754942e-38], dtype=np.float32)      # the last one: the largest denormal
    assert (denormal != 0).all() and (np.abs(denormal) < np.finfo(np.float32).tiny).all()
    pick = np.unique(np.concatenate([[0, F - 1, F // 3], rng.integers(0, F, 5)]))
    x[6, pick] = denormal[np.arange(len(pick)) % 4]
    x[8, np.concatenate([cols[::64], cols[63::64]])] = 0.75
    x[9, 1:] = 1.0
    x[10, [0, F - 1]] = -2.0
    x[11, 1::2] = 3.0
    r = x[N_CONSTRUCTED:]
    r[rng.random(r.shape) < max(0.013, min(0.5, 3.0 / F))] = 1.0
    r[np.arange(60), rng.integers(0, F, 60)] = 1.0
    r *= (rng.random(r.shape).astype(np.float32) + 0.5) * rng.choice(np.float32([-1, 1]), r.shape)
    for n in range(len(x)):
        if n != EMPTY_ROW and not (x[n] != 0).any():
            x[n, 0] = 2.0
    assert np.isfinite(x).all() and not (x[EMPTY_ROW] != 0).any() and np.signbit(x[6][x[6] == 0]).all()
    return x


# ---- z-score
ZSCORE_N, ZSCORE_F = (1, 2, 500), (1, 63, 64, 65, 130)
FAMILIES = ('zero', 'const 0.1f', 'const 3e7', 'two-valued', 'uniform', '1000 +- 0.01', 'scale 1e-20', 'scale 1e19')


def zscore_columns(N, F, shift=0):
    """x float32 [N, F]: column f is of family (f + shift) % 8 (FAMILIES)."""
    rng = np.random.default_rng(77 * N + F)
    x = np.empty((N, F), dtype=np.float32)
    for f in range(F):
        k = (f + shift) % 8
        x[:, f] = (np.zeros(N), np.full(N, np.float32(0.1)), np.full(N, 3e7),
                   np.where(rng.random(N) < 0.3, 2.0, -0.5) if N > 1 else np.full(N, 2.0),
                   rng.random(N), 1000.0 + 0.01 * rng.standard_normal(N),
                   1e-20 * rng.standard_normal(N), 1e19 * rng.standard_normal(N))[k]
        if k == 3 and N > 1:
            x[0, f], x[1, f] = 2.0, -0.5                      # both values present at every N
    return x


def zscore_cases():
    """(N, F, shift): the product of ZSCORE_N and ZSCORE_F; F = 1 runs once per family."""
    return [(N, F, s) for N in ZSCORE_N for F in ZSCORE_F for s in (range(8) if F == 1 else (0,))]


# ---- tokens and the table gradient
DE = (0, 1, 3, 99, 127)
TOKEN_N, TOKEN_F, TOKEN_L = 37, 70, 8


def token_inputs(De, seed=0):
    """(x [N, F], mean [F], inv_std [F], idx [N, L] with some -1, table [F, De]) float32 / int32: random, mean and
    inv_std are test inputs, not statistics of x."""
    rng = np.random.default_rng(900 + De + seed)
    N, F, L = TOKEN_N, TOKEN_F, TOKEN_L
    x = rng.standard_normal((N, F)).astype(np.float32)
    mean = rng.standard_normal(F).astype(np.float32)
    inv_std = (rng.random(F) * 3 + 0.1).astype(np.float32)
    idx = rng.integers(0, F, (N, L)).astype(np.int32)
    idx[rng.random((N, L)) < 0.1] = -1
    idx[3] = -1                                               # a whole node without tokens
    idx[0, 0], idx[N - 1, L - 1] = F - 1, 0
    table = rng.standard_normal((F, De)).astype(np.float32)
    return x, mean, inv_std, idx, table


GRAD_N, GRAD_L, GRAD_F = 512, 8, 70
PATTERNS = ('hot', 'random', 'with -1')


def grad_inputs(De, pattern, kind, seed=0):
    """(dout float32 [N, L, De + 1], idx int32 [N, L]): 'hot' every token on feature 5 (N L = 4096 terms in one row),
    'random', 'with -1' (random, a fifth of the tokens and two whole nodes -1).  kind 'exact': small integers times
    powers of two -- |value| <= 7 * 2^3 in units of 2^-3, so any 4096 of them sum exactly in fp32 in any order (and
    every value is a bf16 number) --, 'random': N(0, 1)."""
    rng = np.random.default_rng(5000 + 10 * De + PATTERNS.index(pattern) + 100 * seed)
    N, L, F = GRAD_N, GRAD_L, GRAD_F
    if kind == 'exact':
        dout = rng.integers(-7, 8, (N, L, De + 1)) * 2.0 ** rng.integers(-3, 4, (N, L, De + 1))
    else:
        dout = rng.standard_normal((N, L, De + 1))
    if pattern == 'hot':
        idx = np.full((N, L), 5)
    else:
        idx = rng.integers(0, F - 4, (N, L))                  # rows F - 4 .. F - 1 are never sampled
        idx[0, 0] = F - 5
        if pattern == 'with -1':
            idx[rng.random((N, L)) < 0.2] = -1
            idx[[1, N - 1]] = -1
    return dout.astype(np.float32), idx.astype(np.int32)


# ---- the walk
WALK_N = 50
WALK_CASES = ((1, 0), (1, 50), (127, 1), (127, 50), (128, 0), (128, 50), (129, 1), (129, 50), (300, 0), (300, 1),
              (300, 50))                                     # (B, walk_length)
WALK_SEEDS = (0, 2 ** 64 - 1, 2 ** 63 + 5, 12345)             # (cycled: the walk_length 0 cases take seed 0)


def walk_graph():
    """edge_index int64 [2, E] on 50 nodes: 160 random edges among nodes 0..39 and node 45; nodes 40..44 isolated; node 45
    a sink (in-edges only); node 46 with its self-loop as its only edge; self-loops on 3 and 5 beside other edges; the edge
    7 -> 8 three times; node 47 -> 48 -> 47 (a two-cycle); node 49 = N - 1 with 40 out-edges (duplicates among them) and
    no in-edge."""
    rng = np.random.default_rng(21)
    src, dst = rng.integers(0, 40, 160), rng.integers(0, 40, 160)
    dst[:12] = 45
    extra = [(46, 46), (3, 3), (5, 5), (7, 8), (7, 8), (7, 8), (47, 48), (48, 47)]
    out49 = [(49, int(v)) for v in rng.integers(0, 30, 40)]
    e = np.array(list(zip(src.tolist(), dst.tolist())) + extra + out49, dtype=np.int64).T
    e = e[:, rng.permutation(e.shape[1])]
    outdeg, indeg = np.bincount(e[0], minlength=WALK_N), np.bincount(e[1], minlength=WALK_N)
    assert not outdeg[40:46].any() and not indeg[40:45].any() and indeg[45] == 12 and outdeg[49] == 40 and indeg[49] == 0
    assert len(set(e[1][e[0] == 49].tolist())) < 40
    return e


def walk_starts(B):
    """start nodes int64 [B]: random, with the sink, an isolated node, the self-loop-only node and N - 1 among them."""
    s = np.random.default_rng(300 + B).integers(0, WALK_N, B)
    s[::7] = np.array([49, 45, 42, 46, 7, 0])[np.arange(len(s[::7])) % 6]
    return s.astype(np.int64)


def walk_cases():
    return [(B, wl, WALK_SEEDS[i % 4]) for i, (B, wl) in enumerate(WALK_CASES)]


# ---- the sub-graph
SAINT_N = (1, 255, 256, 257, 1000)
NODE_SETS = ('none', 'one repeated', 'every node', 'random', 'leaving')


def saint_graph(N):
    """edge_index int64 [2, E] on N nodes: 4 N random edges (duplicates and self-loops among them); node N - 1 sends to
    node 0 only (never to itself) unless N == 1, where the graph is two self-loops."""
    if N == 1:
        return np.zeros((2, 2), dtype=np.int64)
    rng = np.random.default_rng(600 + N)
    e = rng.integers(0, N, (2, 4 * N))
    e[1][e[0] == N - 1] = 0
    e[:, :3] = [[N - 1, 5, 5], [0, 5, 6]]
    return e.astype(np.int64)


def saint_node_input(N, kind):
    """The walked nodes (with repeats) int64: 'none' n = 0; 'one repeated'; 'every node' (shuffled, some twice);
    'random' about N / 3 draws; 'leaving' node N - 1 alone, all of whose out-edges leave the sample (e_sub = 0)."""
    rng = np.random.default_rng(700 + N + NODE_SETS.index(kind))
    if kind == 'none':
        return np.zeros(0, dtype=np.int64)
    if kind == 'one repeated':
        return np.full(300, N // 2, dtype=np.int64)
    if kind == 'every node':
        return rng.permutation(np.concatenate([np.arange(N), rng.integers(0, N, N // 2)])).astype(np.int64)
    if kind == 'random':
        return rng.integers(0, N, max(1, N // 3)).astype(np.int64)
    return np.full(2, N - 1, dtype=np.int64)


def saint_cases():
    """(N, kind); 'leaving' needs a node that does not send to itself: not at N = 1."""
    return [(N, k) for N in SAINT_N for k in NODE_SETS if not (N == 1 and k == 'leaving')]


def n_bounds(n_sub, N):
    """The n_bound values of count_edges_bounded: n_sub, n_sub + 1, the next value from n_sub on that makes n_bound + 1 a
    multiple of 128 (one full workgroup more, no partial one), and N."""
    return sorted({n_sub, n_sub + 1, -(-(n_sub + 1) // 128) * 128 - 1, max(N, n_sub)})


# ---- the norms
def norm_inputs(shape):
    """(node_count [N], edge_count [E], edge_src [E], num_samples) for shape 'N > E', 'E > N', 'E = 0': integer-valued
    float32 counts that reach every branch -- 0 / 0, x / 0, a quotient just above and just below 1e4 with edge counts 1,
    2 and 3, the clamp far above, ordinary quotients that are no float32 number -- and node counts of 0."""
    N, E = {'N > E': (300, 40), 'E > N': (40, 700), 'E = 0': (300, 0)}[shape]
    rng = np.random.default_rng(800 + N + E)
    nc = rng.integers(1, 200, N).astype(np.float32)
    nc[[0, 7, N - 1]] = 0
    nc[[1, 2, 3, 4, 5, 6]] = [10001, 9999, 20001, 19999, 30001, 29999]
    if E == 0:
        return nc, np.zeros(0, np.float32), np.zeros(0, np.int64), 17
    src = rng.integers(8, N - 1, E).astype(np.int64)
    ec = rng.integers(1, 60, E).astype(np.float32)
    head = [(0, 0), (8, 0), (1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (6, 3), (3, 1), (N - 1, 0), (N - 1, 5), (9, 10000)]
    for i, (s, c) in enumerate(head):
        src[i], ec[i] = s, c
    src[E - 1], ec[E - 1] = 1, 1                             # the clamp in the last element too
    return nc, ec, src, 17
