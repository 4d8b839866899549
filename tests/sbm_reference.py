"""numpy model of the stochastic block model generator (csrc/sbm.hip, ampnet_amd/random_graphs.py), written from the
wording of include/ampconv.h, "THE BLOCK MODEL", the case ladder both test files run on, and the bars.

TEST INFRASTRUCTURE.  Plain numpy: no torch, no GPU, no call into the library.  tests/test_sbm_cpu.py holds the model to
its invariants, to its statistical bar and to networkx, and shows that the ladder tells it from each of its mutants;
tests/test_gpu_sbm.py then holds the kernels to the model, element for element.

THE MODEL is vectorised over the units (u, b), with one Python loop over the draw number t.

THE MARGIN.  The kernel and the model share every bit of their inputs (lq = log1p(-p) is a host table), integer
arithmetic and an IEEE division; they differ in the fp64 log(U) alone -- a few ulp, about 1e-15 relative on q (ROCm
documents at most 1 ulp; nobody has measured it here).  A draw decides two things: whether q < m - 1 - j, an integer,
and, if so, floor(q).  Both are safe if q is far from the integers around it, so the margin of a run is the minimum
over ALL its draws of
    min(q - floor(q), floor(q) + 1 - q) / max(1, q)
and a (case, seed) pair is compared exactly only if its margin is at least MARGIN_MIN = 1e-9: a condition on the
inputs, six decades above the error it guards against, not a measurement.  One amendment to that formula, needed for
the entries p = 1e-12 and 1e-300 of the mixed matrix: there q is 1e9 .. 1e302, the formula divides a fraction below 1
by it -- or fp64 has no fractional bits left -- and gives less than 1e-9 whatever the seed, although such a draw decides
nothing but a stop, and by a wide berth.  So a draw that STOPS its chain with q >= (m - 1 - j) + 1, the bound it is
compared to plus one, counts with (q - (m - 1 - j)) / max(1, q), its relative distance from that bound (an infinite q
with 1); a stop within one unit of the bound, and every draw that goes on, counts with the formula as it stands.
No pair of the ladder falls below the bar with the seeds of pipeline_reference.SEEDS (the ladder's smallest margin is
8e-8, the larger case's 1.6e-9; test_sbm_cpu.py asserts the bar for every pair, the GPU test again for each pair it
compares): no seed was replaced and no pair is dropped.

THE BARS, derived: every integer output equal element for element, E included; per block pair the number of edges
within 5 standard deviations of n_pairs p (sd = sqrt(n p (1 - p))): a two-sided 5.7e-7 event per block pair, about
1e-3 over the roughly 2000 block pairs with 0 < p < 1 of the ladder.
"""
import functools
import itertools

import numpy as np

from pipeline_reference import SEEDS, draw

MARGIN_MIN = 1e-9
MAX_K = 256
MUTANTS = ('u_without_plus_one', 'u_stays_a_candidate', 'counter_b_major', 'stop_after_the_cast')
_I64_MIN = np.iinfo(np.int64).min


def starts_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def blocks_of(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.int64), np.asarray(sizes, np.int64))


def log1p_table(P):
    """lq = log1p(-p) in fp64, the table the C calls take (entries with p >= 1 are -inf and never read)."""
    with np.errstate(divide='ignore'):
        return np.log1p(-np.asarray(P, np.float64))


class Result:
    """edge_index int64 [2, E], block int64 [N], count / mcount int64 [N K] (edges / mirrors per unit), off / moff their
    exclusive prefix sums, e_upper = sum(count), margin (see the module's text), draws (how many the run took)."""


def block_model(sizes, P, directed, selfloops, seed, mutant=None, stream=draw):
    """The model.  mutant: one of MUTANTS (tests/test_sbm_cpu.py); stream: the draw function, the library's unless a test
    plants a chosen value in it."""
    sizes = np.asarray(sizes, np.int64)
    K = len(sizes)
    P = np.asarray(P, np.float64).reshape(K, K)
    start, block = starts_of(sizes), blocks_of(sizes)
    N = int(start[-1])
    lq_table = log1p_table(P)
    u = np.repeat(np.arange(N, dtype=np.int64), K)
    b = np.tile(np.arange(K, dtype=np.int64), N)
    bu = block[u]
    p, lq = P[bu, b], lq_table[bu, b]
    lo, hi = start[b].copy(), start[b + 1]
    if directed:
        hole = np.full(N * K, not selfloops) & (bu == b)
        if mutant == 'u_stays_a_candidate':
            hole[:] = False
    else:
        hole = np.zeros(N * K, bool)
        first = u + (0 if selfloops or mutant == 'u_stays_a_candidate' else 1)
        lo = np.maximum(lo, first)
    m = np.maximum(hi - lo - hole, 0)
    counter = (b * N + u if mutant == 'counter_b_major' else u * K + b).astype(np.uint64)

    live = (m > 0) & (p > 0)
    full = live & (p >= 1)
    units = [np.repeat(np.nonzero(full)[0], m[full])]
    js = [np.concatenate([np.arange(k, dtype=np.int64) for k in m[full]]) if full.any() else np.zeros(0, np.int64)]
    act = np.nonzero(live & ~full)[0]
    j = np.full(act.size, -1, np.int64)
    margin, draws, t = np.inf, 0, 0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        while act.size:
            r = stream(seed, counter[act], t)
            U = ((r >> np.uint64(11)) + np.uint64(0 if mutant == 'u_without_plus_one' else 1)).astype(np.float64) * 2.0 ** -53
            q = np.log(U) / lq[act]
            bound = m[act] - 1 - j
            fl = np.floor(q)
            if mutant == 'stop_after_the_cast':                 # the conversion first, as cvttsd2si does it: out of range -> INT64_MIN
                fl_int = np.where(np.abs(fl) < 2.0 ** 63, fl, 0).astype(np.int64)
                fl_int = np.where(np.abs(fl) < 2.0 ** 63, fl_int, _I64_MIN)
                go = fl_int < bound
            else:
                go = q < bound.astype(np.float64)
                fl_int = np.where(go, fl, 0).astype(np.int64)
            draws += act.size
            near = np.minimum(q - fl, fl + 1 - q) / np.maximum(1.0, q)
            clear = ~go & (q >= bound + 1.0)                    # a stop, and not by the last unit of q: see THE MARGIN
            far = np.where(np.isfinite(q), (q - bound) / np.maximum(1.0, q), 1.0)
            margin = min(margin, float(np.where(clear, far, near).min()))
            act, j = act[go], j[go] + 1 + fl_int[go]
            units.append(act.copy())
            js.append(j.copy())
            t += 1
            if mutant and t > 4 * int(m.max()) + 8:              # a mutant's chain need not end by itself
                break
    unit, jj = np.concatenate(units), np.concatenate(js)
    order = np.lexsort((jj, unit))
    unit, jj = unit[order], jj[order]
    src = u[unit]
    dst = lo[unit] + jj
    dst = dst + (hole[unit] & (dst >= src))

    res = Result()
    res.block, res.num_nodes, res.margin, res.draws = block, N, margin, draws
    res.count = np.bincount(unit, minlength=N * K).astype(np.int64)
    res.mcount = res.count - np.bincount(unit[dst == src], minlength=N * K).astype(np.int64)
    res.off = np.concatenate([[0], np.cumsum(res.count)[:-1]]).astype(np.int64) if N * K else np.zeros(0, np.int64)
    res.moff = np.concatenate([[0], np.cumsum(res.mcount)[:-1]]).astype(np.int64) if N * K else np.zeros(0, np.int64)
    res.e_upper = int(res.count.sum())
    upper = np.stack([src, dst]).astype(np.int64)
    if directed:
        res.edge_index = upper
    else:
        keep = dst != src
        res.edge_index = np.concatenate([upper, np.stack([dst[keep], src[keep]])], axis=1).astype(np.int64)
    return res


# ------------------------------------------------------------------------------------------------------------ the ladder
SIZES = ([1], [2], [63, 1], [64], [65, 64], [0, 5, 0, 7], [257], [64, 65, 63, 1], [100] * 4)
MIXED_VALUES = (1e-12, 0.0, 1.0, 1e-300)       # entry (a, b) is value (a + b) % 4: a 0, a 1 and a 1e-12 from K = 2 on
BIG = dict(sizes=[5000] * 4, p_in=2e-3, p_out=2e-4)        # about 260 k directed edges


def uniform(K, p):
    return np.full((K, K), float(p))


def in_out(K, p_in, p_out):
    return np.where(np.eye(K, dtype=bool), float(p_in), float(p_out))


def mixed(K):
    a = np.arange(K)
    return np.asarray(MIXED_VALUES)[(a[:, None] + a[None, :]) % 4]


def asymmetric(K):
    """P[a][b] = 0.6 / (1 + a + 2 b): differs from its transpose wherever a != b; K == 1 has only the diagonal."""
    a = np.arange(K, dtype=np.float64)
    return 0.6 / (1.0 + a[:, None] + 2.0 * a[None, :])


MATRICES = {'p0': lambda K: uniform(K, 0.0), 'p1': lambda K: uniform(K, 1.0), 'p0.3': lambda K: uniform(K, 0.3),
            'in0.8_out0.05': lambda K: in_out(K, 0.8, 0.05), 'in0.05_out0.001': lambda K: in_out(K, 0.05, 0.001),
            'mixed': mixed, 'asymmetric': asymmetric}


def ladder():
    """[(sizes, matrix name, directed, selfloops)]: every size list x every matrix x the four flag pairs, the asymmetric
    matrix on the directed ones alone.  Every entry is run with every seed of SEEDS."""
    out = []
    for sizes, name in itertools.product(SIZES, MATRICES):
        for directed, selfloops in itertools.product((False, True), (False, True)):
            if name == 'asymmetric' and not directed:
                continue
            out.append((tuple(sizes), name, directed, selfloops))
    return out


def case_id(c):
    sizes, name, directed, selfloops = c
    return f"{'x'.join(map(str, sizes))}-{name}-{'dir' if directed else 'und'}-{'loops' if selfloops else 'noloops'}"


@functools.lru_cache(maxsize=None)
def reference(sizes, name, directed, selfloops, seed):
    """The model's result for a ladder entry, computed once and shared: treat it as read-only."""
    return block_model(sizes, MATRICES[name](len(sizes)), directed, selfloops, seed)


@functools.lru_cache(maxsize=None)
def big_reference(directed, seed):
    return block_model(BIG['sizes'], in_out(4, BIG['p_in'], BIG['p_out']), directed, False, seed)


def candidate_pairs(sizes, directed, selfloops):
    """n_pairs [K, K]: the number of candidate pairs (u in block a, v in block b) of the model."""
    s = np.asarray(sizes, np.int64)
    n = np.outer(s, s)
    d = s * s if selfloops else s * (s - 1)
    if directed:
        n[np.diag_indices(len(s))] = d
        return n
    n = np.triu(n)                                   # u < v: only blocks a <= b hold pairs
    n[np.diag_indices(len(s))] = (s * (s + 1) if selfloops else s * (s - 1)) // 2
    return n


def pair_counts(res, K, upper_only):
    """[K, K] edge counts by (block of row, block of column) of the first e_upper edges (all of them if directed)."""
    e = res.edge_index[:, :res.e_upper] if upper_only else res.edge_index
    return np.bincount(res.block[e[0]] * K + res.block[e[1]], minlength=K * K).reshape(K, K)
