"""numpy models of graph preparation (csrc/graph_prep.hip), of the long-segment plan (csrc/hub.hip) and of the node
lists, and the inputs tests/test_gpu_graph_prep.py runs them on.

TEST INFRASTRUCTURE.  Everything here is integer-exact but `cinv`, one correctly rounded float32 division: the GPU tests
compare element for element, nothing is sorted before comparing except the descriptors of a plan, whose SLOT order
(which long row took which slots) is arbitrary by design -- `check_plan` holds everything about a plan that is not.
tests/test_graph_reference_cpu.py shows that the inputs below tell each model from its mutants and that every plan they
ask for fits the capacity the library allots.

The two preparation paths of ampconv_graph_build: ONE launch (`csr_small_kernel`) for 0 < E <= 12 288 and N <= 16 384,
the device-wide radix sorts (`ampconv_csr_build`, then `ampconv_hub_plan` twice) for everything else -- `path_of`.
"""
import collections
import functools

import numpy as np

from edge_runner import chunks_per_row
from edge_runner import graph as runner_graph

SMALL_MAX_E, SMALL_MAX_N, SMALL_EBITS = 12288, 1 << 14, 14      # kSmallMaxE, kSmallMaxN, kSmallEbits
PAD_KEY = 0xFFFFFFFF
LIST_PAD = 8                                                     # zeros behind a node list
INT64_MIN = -2 ** 63


def path_of(N, E):
    return 'small' if 0 < E <= SMALL_MAX_E and 0 < N <= SMALL_MAX_N else 'multi'


def bits_for(N):
    b = 1
    while b < 31 and (1 << b) < N:
        b += 1
    return b


def clamp(ids, N):
    """The library's rule for ids outside [0, N): v < 0 -> 0, v >= N -> N - 1 (on the int64 value, before it is narrowed)."""
    ids = np.asarray(ids, dtype=np.int64)
    return np.where(ids < 0, 0, np.where(ids >= N, N - 1, ids))


def pointer(keys, N):
    """ptr[n] = number of keys < n (the lower bound in the sorted keys), n = 0..N."""
    return np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=N))]).astype(np.int32)


class Built(collections.namedtuple('Built', 'rowptr col eperm cscptr crow cperm cinv by_edge flag')):
    status = None               # {flag, chunks of the destination plan, chunks of the source plan, 0}, set by graph_build


ARRAYS = Built._fields[:7]      # what ampconv_csr_build writes


def graph_build(ei, N, chunk=0):
    """(rowptr, col, eperm, cscptr, crow, cperm, cinv, by_edge, flag) of ampconv_graph_build for edge_index `ei` [2, E]:
    the CLAMPED graph's destination-sorted CSR and source-sorted CSC in stable order, cinv[p] = float32 1 / float32
    in-degree of crow[p], by_edge[e] = CSC position of edge e, flag = 1 iff an id was outside [0, N).  The result's
    `status` is the call's status words for plans of `chunk` edges (0: no plans)."""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    E = ei.shape[1]
    flag = int(((ei < 0) | (ei >= N)).any())
    src, dst = clamp(ei, N)
    eperm = np.argsort(dst, kind='stable')
    cperm = np.argsort(src, kind='stable')
    crow = dst[cperm]
    indeg = np.bincount(dst, minlength=N)
    cinv = np.float32(1) / indeg[crow].astype(np.float32)
    by_edge = np.empty(E, dtype=np.int32)
    by_edge[cperm] = np.arange(E, dtype=np.int32)
    i32 = np.int32
    b = Built(pointer(dst, N), src[eperm].astype(i32), eperm.astype(i32), pointer(src, N), crow.astype(i32),
              cperm.astype(i32), cinv, by_edge, flag)
    nd, ns = (plan(p, N, chunk)[2] if chunk > 0 and E > 0 else 0 for p in (b.rowptr, b.cscptr))
    b.status = np.array([flag, nd, ns, 0], dtype=np.int32)
    return b


# ----------------------------------------------------------------------------------------------------------- plans
def max_chunks(E, chunk):
    return 2 * (E // chunk) + 2


def plan_words_total(E, chunk):
    """int32 words of a plan: ampconv_hub_plan_bytes / 4."""
    mc = max_chunks(E, chunk)
    return 4 + 4 * mc + mc // 2 + 2


def plan(ptr, n_rows, chunk):
    """({(row, beg, end, nfirst)}, long rows, chunks) of a plan over the first n_rows rows of `ptr`: every row LONGER than
    `chunk` edges is cut into ceil(deg / chunk) chunks of `chunk` edges, the last one ending at the segment's end;
    nfirst = the row's chunk count in its first chunk, 0 in the others."""
    ptr = np.asarray(ptr, dtype=np.int64)[:n_rows + 1]
    deg = np.diff(ptr)
    rows = np.nonzero(deg > chunk)[0]
    descs = set()
    for r, nc in zip(rows, chunks_per_row(deg, chunk)):
        b, e = int(ptr[r]), int(ptr[r + 1])
        descs |= {(int(r), b + k * chunk, min(e, b + (k + 1) * chunk), int(nc) if k == 0 else 0) for k in range(int(nc))}
    return descs, len(rows), len(descs)


def plan_words(ptr, n_rows, E, chunk, sentinel, order=None):
    """The words a plan buffer full of `sentinel` holds after the library wrote ONE legal plan into it: the long rows take
    their slots in ascending row order (or in `order`, a permutation of them)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    mc = max_chunks(E, chunk)
    w = np.full(plan_words_total(E, chunk), sentinel, dtype=np.int32)
    rows = np.nonzero(np.diff(ptr[:n_rows + 1]) > chunk)[0]
    rows = rows if order is None else rows[np.asarray(order)]
    slot = 0
    for i, r in enumerate(rows):
        b, e = int(ptr[r]), int(ptr[r + 1])
        nc = -(-(e - b) // chunk)
        for k in range(nc):
            w[4 + 4 * (slot + k):8 + 4 * (slot + k)] = (r, b + k * chunk, min(e, b + (k + 1) * chunk), nc if k == 0 else 0)
        w[4 + 4 * mc + i] = slot
        slot += nc
    w[:4] = (slot, chunk, len(rows), 4 + 4 * mc)
    return w


def check_plan(words, ptr, n_rows, E, chunk, sentinel=None, origin=0):
    """Asserts that `words` -- the int32 words of a plan buffer, the plan beginning at word `origin` -- hold a plan of
    the first n_rows rows of `ptr`: the header {chunks, chunk, long rows, 4 + 4 * max_chunks}; the descriptors as a set;
    every row's chunks in CONSECUTIVE slots from its first, in order k = 0, 1, ... (the combine pass reads the partial
    tiles P + (c + k) * L * D of the row whose first chunk is c); the list = exactly the slots with nfirst != 0, each once;
    and, with `sentinel`, every other word of `words` -- unused slots, unused list entries, what lies around the plan --
    still the sentinel.  Returns the slots of the list in list order."""
    words = np.asarray(words, dtype=np.int32)
    want, n_long, n_chunks = plan(ptr, n_rows, chunk)
    mc = max_chunks(E, chunk)
    off = 4 + 4 * mc
    assert n_chunks <= mc and n_long <= mc // 2 + 2, f'the plan ({n_chunks} chunks, {n_long} rows) exceeds its capacity ({mc})'
    w = words[origin:origin + plan_words_total(E, chunk)]
    assert len(w) == plan_words_total(E, chunk), 'the buffer is shorter than the plan'
    assert w[:4].tolist() == [n_chunks, chunk, n_long, off], f'header {w[:4].tolist()}, want {[n_chunks, chunk, n_long, off]}'
    descs = w[4:4 + 4 * n_chunks].reshape(n_chunks, 4)
    got = {tuple(int(v) for v in d) for d in descs}
    assert len(got) == n_chunks and got == want, (f'descriptors differ from the model: {len(got ^ want)} in one set only, '
                                                  f'e.g. {sorted(got ^ want)[:4]}')
    firsts = np.nonzero(descs[:, 3])[0] if n_chunks else np.zeros(0, dtype=np.int64)
    for s in firsts:
        r, b, e, nc = (int(v) for v in descs[s])
        end = int(ptr[r + 1])
        assert s + nc <= n_chunks, f'row {r}: {nc} chunks from slot {s} run past the {n_chunks} used slots'
        for k in range(nc):
            exp = (r, b + k * chunk, min(end, b + (k + 1) * chunk), nc if k == 0 else 0)
            assert tuple(int(v) for v in descs[s + k]) == exp, (f'row {r}: slot {s} + {k} holds {descs[s + k].tolist()}, not '
                                                                f'chunk {k} {exp}: a row\'s chunks must be consecutive and in order')
    lst = w[off:off + n_long]
    assert sorted(lst.tolist()) == firsts.tolist(), f'the list {sorted(lst.tolist())[:8]}... is not the first-chunk slots {firsts.tolist()[:8]}...'
    if sentinel is not None:
        used = np.zeros(len(words), dtype=bool)
        used[origin:origin + 4 + 4 * n_chunks] = True
        used[origin + off:origin + off + n_long] = True
        stray = np.nonzero(~used & (words != np.int32(sentinel)))[0]
        assert stray.size == 0, (f'{stray.size} words outside the header, the {n_chunks} descriptors and the {n_long} list entries '
                                 f'were written, first at word {stray[:4] - origin} of the plan')
    return lst.copy()


# -------------------------------------------------------------------------------------------- positions, node lists
def spos(eperm, cperm):
    """spos[p] = CSC position of the edge at CSR position p: cperm[spos[p]] == eperm[p]."""
    by_edge = np.empty(len(cperm), dtype=np.int32)
    by_edge[np.asarray(cperm)] = np.arange(len(cperm), dtype=np.int32)
    return by_edge[np.asarray(eperm)]


def active(rowptr, cscptr, N, which):
    """(list, ptr, count) of ampconv_active_nodes: the ascending ids of the nodes with an in-edge (which & 1) or an
    out-edge (which & 2), then LIST_PAD zeros; ptr [N + 1] = exclusive count of listed nodes in front of n."""
    on = np.zeros(N, dtype=bool)
    if which & 1:
        on |= np.diff(np.asarray(rowptr)[:N + 1]) != 0
    if which & 2:
        on |= np.diff(np.asarray(cscptr)[:N + 1]) != 0
    ids = np.nonzero(on)[0].astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(on)]).astype(np.int32)
    return np.concatenate([ids, np.zeros(LIST_PAD, dtype=np.int32)]), ptr, len(ids)


# ------------------------------------------------------------------------------------- the one-launch kernel as data
def lower_bound(sorted_keys, E, wants):
    """The kernel's search, step for step: the first position in [0, E) whose key is >= want, for every want."""
    wants = np.asarray(wants, dtype=np.uint32)
    lo, hi = np.zeros(len(wants), dtype=np.int64), np.full(len(wants), E, dtype=np.int64)
    while (lo < hi).any():
        live = lo < hi
        mid = (lo + hi) >> 1
        less = sorted_keys[np.minimum(mid, max(E - 1, 0))] < wants
        lo = np.where(live & less, mid + 1, lo)
        hi = np.where(live & ~less, mid, hi)
    return lo.astype(np.int32)


def small_keys_sorted(ids, N, order_of=None):
    """The 12 288 key slots of one workgroup of csr_small_kernel after its sort: (clamped id << 14) | edge id for the E
    edges in blocked order, PAD_KEY behind them, stably sorted on bits [14, 14 + bits_for(N)) ONLY -- the padding's
    sorted bits are all ones, which at a power-of-two N are those of node N - 1: stability alone (the padding stands
    behind every real key in the input) keeps it out of the first E slots."""
    ids = clamp(ids, N)
    E = len(ids)
    assert 0 < E <= SMALL_MAX_E and 0 < N <= SMALL_MAX_N
    keys = np.full(SMALL_MAX_E, PAD_KEY, dtype=np.uint32)
    keys[:E] = (ids.astype(np.uint32) << SMALL_EBITS) | np.arange(E, dtype=np.uint32)
    digit = (keys >> SMALL_EBITS) & np.uint32((1 << bits_for(N)) - 1)
    order = np.argsort(digit, kind='stable') if order_of is None else order_of(digit, keys)
    return keys[order]


def small_kernel_keys(ei, N, order_of=None):
    """((sorted keys, eperm, rowptr), (sorted keys, cperm, cscptr)) as workgroups 0 and 1 of csr_small_kernel read them
    off their sorted key slots: perm[p] = the low 14 bits of slot p < E, ptr[n] = lower_bound of n << 14 over the first
    E slots (full 32-bit compare)."""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    E = ei.shape[1]
    out = []
    for ids in (ei[1], ei[0]):
        s = small_keys_sorted(ids, N, order_of)
        perm = (s[:E] & np.uint32((1 << SMALL_EBITS) - 1)).astype(np.int32)
        out.append((s, perm, lower_bound(s, E, np.arange(N + 1, dtype=np.uint32) << SMALL_EBITS)))
    return tuple(out)


# ======================================================================================================== the inputs
Case = collections.namedtuple('Case', 'name path N chunk ei')


def _shuffled(src, dst, seed):
    p = np.random.default_rng(seed).permutation(len(src))
    return np.stack([np.asarray(src, np.int64)[p], np.asarray(dst, np.int64)[p]])


def _corner_graph(N, E, seed):
    """Random edges; more than a quarter of them END at node N - 1 and more than a quarter START there (independently drawn
    positions, so some do both), node 0 sends and receives too.  E = 1: the one edge is the self-loop of node N - 1."""
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, N, size=(2, E)).astype(np.int64)
    q = E // 4 + 1
    for side in (0, 1):
        pos = rng.permutation(E)
        ei[side, pos[q:q + max(1, E // 16)]] = 0
        ei[side, pos[:q]] = N - 1
    return ei


def _hub_graph(N, E, hub, seed=3):
    """test_csr_build_is_a_stable_sort's graph: random, `hub` edges into node 7 and hub // 2 out of node 11."""
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, N, size=(2, E)).astype(np.int64)
    ei[1, :hub] = 7
    ei[0, hub:hub + hub // 2] = min(11, N - 1)
    return ei


def _two_chunk_rows(n, chunk, seed):
    """n rows of chunk + 1 edges on BOTH sides (dst = e // (chunk + 1), src = e % n), shuffled: every row long with two
    chunks, the most chunks and the most list entries a plan of that many edges can be asked to hold."""
    e = np.arange(n * (chunk + 1))
    return _shuffled(e % n, e // (chunk + 1), seed)


BUILD_CASES = ('s-N1-E1', 's-N1-E70-loops', 's-N2-E1', 's-N2-E1025', 's-N64-E1023', 's-N1024-E12287', 's-N16384-E1025',
               's-N16384-E12288', 's-N300-E12288-one-row', 's-N189-E12285-two-chunk-rows', 's-N63-E4095-full-plan',
               's-ladder', 'm-N16385-E1', 'm-N16385-E5', 'm-N16385-E1000-hub', 'm-N40000-E12288', 'm-N500-E12289',
               'm-N190-E12350-two-chunk-rows', 'm-N16385-E4095-full-plan', 'm-N1000-E20000-chunk128')
# the plans of these reach max_chunks - 2 = 2 * (E // chunk) chunks, the most a graph of E edges can need
FULL_PLAN_CASES = ('s-N63-E4095-full-plan', 'm-N16385-E4095-full-plan')


@functools.lru_cache(maxsize=None)
def build_case(name):
    chunk = 64
    if name == 's-N1-E1':
        N, ei = 1, np.zeros((2, 1), np.int64)
    elif name == 's-N1-E70-loops':                      # bits_for(1) = 1; one long row on both sides
        N, ei = 1, np.zeros((2, 70), np.int64)
    elif name.startswith(('s-N2-', 's-N64-', 's-N1024-', 's-N16384-')):
        N, E = (int(t[1:]) for t in name.split('-')[1:3])
        ei = _corner_graph(N, E, seed=N + E)
    elif name == 's-N300-E12288-one-row':               # one destination row of 192 chunks
        e = np.arange(12288)
        N, ei = 300, np.stack([e % 300, np.full(12288, 7)])
    elif name == 's-N189-E12285-two-chunk-rows':
        N, ei = 189, _two_chunk_rows(189, 64, 21)
    elif name == 's-N63-E4095-full-plan':
        N, ei = 63, _two_chunk_rows(63, 64, 22)
    elif name == 's-ladder':                            # segment lengths 0..20, 63..65, 127..129, 191..193, 257, ..., 1025
        g = runner_graph('L', 64)
        N, ei = g.N, _shuffled(g.src, g.dst, 23)
    elif name == 'm-N16385-E1':
        N, ei = 16385, np.array([[0], [16384]], np.int64)
    elif name == 'm-N16385-E5':
        N, ei = 16385, np.array([[16384, 0, 16384, 3, 0], [0, 16384, 16384, 3, 16384]], np.int64)
    elif name == 'm-N16385-E1000-hub':                  # a sparse batch over many nodes: 70 edges into node 7, 70 out of 16384
        N, ei = 16385, _hub_graph(16385, 1000, 70, seed=4)
        ei[0, 500:570] = 16384
    elif name == 'm-N40000-E12288':
        N, ei = 40000, _corner_graph(40000, 12288, seed=5)
    elif name == 'm-N500-E12289':
        N, ei = 500, _hub_graph(500, 12289, 70)
    elif name == 'm-N190-E12350-two-chunk-rows':
        N, ei = 190, _two_chunk_rows(190, 64, 24)
    elif name == 'm-N16385-E4095-full-plan':            # 63 two-chunk rows among 16 385 nodes
        N, ei = 16385, _two_chunk_rows(63, 64, 25)
        ei = np.where(ei == 62, 16384, ei)
    elif name == 'm-N1000-E20000-chunk128':
        N, ei, chunk = 1000, _hub_graph(1000, 20000, 4000), 128
    else:
        raise ValueError(name)
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    path = path_of(N, ei.shape[1])
    assert path == {'s': 'small', 'm': 'multi'}[name[0]], name
    ei.setflags(write=False)
    return Case(name, path, N, chunk, ei)


# ---- ids out of range: each of these on the source side, the destination side and both
BAD_IDS = (-1, 'N', 'N+7', 2 ** 31, 2 ** 40, -2 ** 40, INT64_MIN)
OOB_SHAPES = ((5, 4), (1024, 3000), (20000, 3000))
OOB_CASES = tuple((N, E, side, part) for N, E in OOB_SHAPES for side in ('src', 'dst', 'both')
                  for part in ((0, 1) if E < len(BAD_IDS) else (0,)))


def bad_ids(N):
    return np.array([{'N': N, 'N+7': N + 7}.get(v, v) for v in BAD_IDS], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def oob_case(N, E, side, part):
    """(edge_index with ids out of range, the same graph before they were put in).  E >= 7: all seven bad ids on each
    side named, at random positions; E = 4: ids 0..3 of BAD_IDS (part 0) or 3..6 (part 1)."""
    rng = np.random.default_rng(N + E)
    clean = rng.integers(0, N, size=(2, E)).astype(np.int64)
    ids = bad_ids(N)
    if E < len(ids):
        ids = ids[:4] if part == 0 else ids[3:]
    ei = clean.copy()
    for s in {'src': (0,), 'dst': (1,), 'both': (0, 1)}[side]:
        ei[s, rng.permutation(E)[:len(ids)]] = rng.permutation(ids)
    for a in (ei, clean):
        a.setflags(write=False)
    return ei, clean


# ---- ampconv_hub_plan alone: (name, ptr, rows of the call, E, chunk)
@functools.lru_cache(maxsize=None)
def plan_cases():
    g = runner_graph('L', 64)
    ladder = np.asarray(g.rowptr, dtype=np.int32)
    cases = [(f'ladder-rows{n}-chunk{c}', ladder, n, g.E, c) for c in (1, 64, 128) for n in (g.N, 31)]
    cases.append(('ladder-rows21-no-long-row', ladder, 21, g.E, 64))
    # 70 000 rows, a third of them with one edge, 40 long ones (65, 72, ... edges) spread over the 274 blocks of the launch
    deg = (np.arange(70000) % 3 == 0).astype(np.int64)
    deg[np.arange(40) * 1750 + 3] = 65 + 7 * np.arange(40)
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    cases.append(('N70000-40-long-rows', ptr, 70000, int(ptr[-1]), 64))
    return tuple(cases)


# ---- ampconv_active_nodes directly: the pointers alone are its input
ACTIVE_N = (1, 2, 255, 256, 257, 70000)
ACTIVE_KINDS = ('all', 'first', 'last', 'no-in-edge', 'sparse')


@functools.lru_cache(maxsize=None)
def active_case(N, kind):
    """(rowptr, cscptr) int32 [N + 1]."""
    one = lambda on: np.concatenate([[0], np.cumsum(on)]).astype(np.int32)
    ar = np.arange(N)
    if kind == 'all':                                    # count == N: the list needs all N + 8 words
        return one(np.ones(N, int)), one(np.full(N, 2))
    if kind == 'first':
        return one(ar == 0), one(ar == 0)
    if kind == 'last':
        return one(ar == N - 1), one(3 * (ar == N - 1))
    if kind == 'no-in-edge':                             # which = 1 lists nothing; the out-edges are there
        return np.zeros(N + 1, np.int32), one(ar % 2 == 0)
    if kind == 'sparse':                                 # tests/test_gpu_proj.py: _sparse_graph, a third of the nodes silent
        rng = np.random.default_rng(N)
        act = N - N // 3
        src = rng.integers(0, max(act // 2, 1), size=2 * N)
        dst = rng.integers(act // 4, max(act, act // 4 + 1), size=2 * N)
        return pointer(dst, N), pointer(src, N)
    raise ValueError(kind)
