"""CPU checks of tests/graph_reference.py, the numpy models tests/test_gpu_graph_prep.py holds graph preparation, the
long-segment plans and the node lists to by exact equality: the one-launch kernel's sort restated as data agrees with
the plain model on every small-path input (at a power-of-two N only because the sort is stable); the model agrees with
tests/pipeline_reference.py, tests/edge_reference.py and the oracle's segment mean; every listed MUTANT of a model
differs from it on at least one input of the GPU file -- a mutant those inputs cannot tell from the model would mean a
kernel with that defect passes --; and every plan the GPU file asks for fits the capacity the library allots, so that
the inputs are known to be legal before they reach a GPU.  The mutants are variants of the MODELS, never of the library."""
import numpy as np
import pytest

import edge_reference as er
import graph_reference as gr
import pipeline_reference as pr
from oracle.ampconv_numpy import segment_mean

SENT = 0x5A5A5A5A


def small_inputs():
    """(name, edge_index, N) of everything the GPU file sends down the one-launch path."""
    for name in gr.BUILD_CASES:
        c = gr.build_case(name)
        if c.path == 'small':
            yield name, c.ei, c.N
    for N, E, side, part in gr.OOB_CASES:
        if gr.path_of(N, E) == 'small':
            ei, clean = gr.oob_case(N, E, side, part)
            yield f'oob-N{N}-E{E}-{side}-{part}', ei, N
            yield f'oob-N{N}-E{E}-clean', clean, N


def all_inputs():
    for name in gr.BUILD_CASES:
        c = gr.build_case(name)
        yield name, c.ei, c.N, c.chunk
    for N, E, side, part in gr.OOB_CASES:
        yield f'oob-N{N}-E{E}-{side}-{part}', gr.oob_case(N, E, side, part)[0], N, 64


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_cases_are_what_their_names_say():
    paths = [gr.build_case(n).path for n in gr.BUILD_CASES]
    assert paths.count('small') == 12 and paths.count('multi') == 8
    for name in gr.BUILD_CASES:
        c = gr.build_case(name)
        N, E = c.N, c.ei.shape[1]
        if '-N' in name:
            assert f'-N{N}-' in name + '-' and (f'-E{E}' in name), name
        if name.startswith(('s-N2-', 's-N64-', 's-N1024-', 's-N16384-')):
            # more than a quarter of the edges end at node N - 1, more than a quarter start there; node 0 takes part
            assert 4 * (c.ei[1] == N - 1).sum() > E and 4 * (c.ei[0] == N - 1).sum() > E, name
            assert E == 1 or ((c.ei[0] == 0).any() and (c.ei[1] == 0).any()), name
    c = gr.build_case('s-N300-E12288-one-row')
    assert gr.plan(gr.graph_build(c.ei, c.N).rowptr, c.N, 64)[1:] == (1, 192)
    for name in ('s-N189-E12285-two-chunk-rows', 'm-N190-E12350-two-chunk-rows'):
        c = gr.build_case(name)
        b = gr.graph_build(c.ei, c.N)
        assert (np.diff(b.rowptr) == 65).all() and (np.diff(b.cscptr) == 65).all(), name
    deg = np.diff(gr.graph_build(gr.build_case('s-ladder').ei, gr.build_case('s-ladder').N).rowptr)
    assert {0, 63, 64, 65, 127, 128, 129} <= set(deg.tolist())
    b = gr.graph_build(gr.build_case('m-N16385-E1000-hub').ei, 16385)
    assert np.diff(b.rowptr).max() >= 70 and np.diff(b.cscptr)[16384] == 70


def test_small_kernel_keys_agree_with_the_model():
    """Every small-path input: eperm, rowptr, cperm, cscptr read off the sorted key slots equal the stable argsort's.
    At a power-of-two N with E < 12 288 the padding TIES with node N - 1 in the sorted bits: it stands behind that node's
    edges only because it stood behind them in the input and the sort is stable."""
    ties = []
    for name, ei, N in small_inputs():
        b = gr.graph_build(ei, N)
        (kd, eperm, rowptr), (ks, cperm, cscptr) = gr.small_kernel_keys(ei, N)
        assert same((eperm, rowptr, cperm, cscptr), (b.eperm, b.rowptr, b.cperm, b.cscptr)), name
        E = ei.shape[1]
        assert (kd[E:] == gr.PAD_KEY).all() and (ks[E:] == gr.PAD_KEY).all(), name
        mask = (1 << gr.bits_for(N)) - 1
        if E < gr.SMALL_MAX_E and (gr.PAD_KEY >> gr.SMALL_EBITS) & mask == N - 1 and (gr.clamp(ei, N) == N - 1).any():
            ties.append(name)
    print('[ties] small-path inputs whose padding ties with node N - 1:', ties)
    assert {'s-N2-E1', 's-N2-E1025', 's-N64-E1023', 's-N1024-E12287', 's-N16384-E1025'} <= set(ties)


def test_model_agrees_with_the_other_restatements():
    """pipeline_reference.csc_of and edge_reference.csr_of on every in-range input; the oracle's segment mean (PyG
    aggr='mean' over the unsorted edge list) against the mean over the model's CSR segments and against cinv."""
    for name, ei, N, chunk in all_inputs():
        if not name.startswith('oob'):
            b = gr.graph_build(ei, N)
            assert b.flag == 0
            assert same(pr.csc_of(ei, N), (b.cscptr, b.crow, b.cperm)), name
            rowptr, col = er.csr_of(ei[0], ei[1], N)
            assert same((rowptr, col), (b.rowptr, b.col)), name
            assert np.array_equal(b.cperm[gr.spos(b.eperm, b.cperm)], b.eperm) and np.array_equal(b.cperm[b.by_edge], np.arange(ei.shape[1]))
            x = np.random.default_rng(1).integers(-50, 50, ei.shape[1]).astype(np.float64)       # exact sums
            want = segment_mean(x, ei[1], N)
            deg = np.diff(b.rowptr)
            got = np.array([x[b.eperm[b.rowptr[r]:b.rowptr[r + 1]]].sum() for r in range(N)]) / np.maximum(deg, 1)
            assert np.array_equal(got, want), name
            w = np.zeros(N, dtype=np.float64)
            np.add.at(w, b.crow, b.cinv.astype(np.float64))                                        # the weights of a mean
            assert np.allclose(w[deg > 0], 1.0, rtol=0, atol=1e-4) and not w[deg == 0].any(), name
            assert b.cinv.dtype == np.float32


# ---------------------------------------------------------------------------------------------------------- mutants
def build_mutant(ei, N, kind):
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    E = ei.shape[1]
    src, dst = gr.clamp(ei, N)
    if kind == 'negative ids clamped to N - 1':
        src, dst = np.where((ei < 0) | (ei >= N), N - 1, ei)
    if kind == 'unstable sort':                                   # segments in descending edge id
        eperm, cperm = np.lexsort((-np.arange(E), dst)), np.lexsort((-np.arange(E), src))
    else:
        eperm, cperm = np.argsort(dst, kind='stable'), np.argsort(src, kind='stable')
    ptr = gr.pointer
    if kind == 'pointer as an upper bound':
        ptr = lambda k, n: np.searchsorted(np.sort(k), np.arange(n + 1), side='right').astype(np.int32)
    crow = dst[cperm]
    deg = np.bincount(src if kind == 'cinv from out-degrees' else dst, minlength=N)
    with np.errstate(divide='ignore'):
        cinv = np.float32(1) / deg[crow].astype(np.float32)
    return ptr(dst, N), src[eperm], eperm, ptr(src, N), crow, cperm, cinv


BUILD_MUTANTS = ('unstable sort', 'pointer as an upper bound', 'negative ids clamped to N - 1', 'cinv from out-degrees')


def test_build_inputs_tell_the_mutants_apart():
    told = {k: [] for k in BUILD_MUTANTS}
    for name, ei, N, chunk in all_inputs():
        b = gr.graph_build(ei, N)
        assert same(build_mutant(ei, N, None), b[:7]), name
        for k in BUILD_MUTANTS:
            if not same(build_mutant(ei, N, k), b[:7]):
                told[k].append(name)
    print('[mutants] graph_build:', {k: len(v) for k, v in told.items()}, 'of', len(list(all_inputs())))
    for k, names in told.items():
        assert names, f'no input of the GPU file tells the mutant "{k}" from the model'
    assert all(n.startswith('oob') for n in told['negative ids clamped to N - 1'])


def test_small_path_inputs_tell_the_padding_mutant_apart():
    """Padding sorted IN FRONT of node N - 1's keys (a sort that is stable on the node ids but not on ties with the
    padding): wrong at a power-of-two N, right at every other."""
    pad_first = lambda digit, keys: np.lexsort((keys != gr.PAD_KEY, digit))
    told = []
    for name, ei, N in small_inputs():
        want = gr.small_kernel_keys(ei, N)
        got = gr.small_kernel_keys(ei, N, order_of=pad_first)
        if not all(same(g[1:], w[1:]) for g, w in zip(got, want)):
            told.append(name)
            assert N & (N - 1) == 0 and N > 1, name
    print('[mutants] padding in front of node N - 1:', told)
    assert told, 'no small-path input of the GPU file tells the mutant "padding in front of node N - 1" from the model'


def plan_inputs():
    """(name, ptr, rows, E, chunk) of every plan the GPU file builds or checks."""
    for name, ei, N, chunk in all_inputs():
        b = gr.graph_build(ei, N)
        yield name + '/dst', b.rowptr, N, ei.shape[1], chunk
        yield name + '/src', b.cscptr, N, ei.shape[1], chunk
    yield from gr.plan_cases()
    g = gr.runner_graph('L', 64)
    yield 'slot-order/dst', np.asarray(g.rowptr), g.N, g.E, 64


def plan_mutant(ptr, n_rows, chunk, kind):
    ptr = np.asarray(ptr, dtype=np.int64)[:n_rows + 1]
    descs = set()
    for r in range(n_rows):
        b, e = int(ptr[r]), int(ptr[r + 1])
        if e - b > chunk or (kind == 'row cut at deg >= chunk' and e - b == chunk):
            nc = -(-(e - b) // chunk)
            for k in range(nc):
                end = b + (k + 1) * chunk
                descs.add((r, b + k * chunk, end if kind == 'last end not cut' else min(e, end), nc if k == 0 else 0))
    return descs


def test_plan_inputs_tell_the_mutants_apart():
    told = {'row cut at deg >= chunk': [], 'last end not cut': [], 'chunks in reversed slot order': []}
    for name, ptr, n, E, chunk in plan_inputs():
        want, n_long, n_chunks = gr.plan(ptr, n, chunk)
        assert plan_mutant(ptr, n, chunk, None) == want, name
        for k in ('row cut at deg >= chunk', 'last end not cut'):
            if plan_mutant(ptr, n, chunk, k) != want:
                told[k].append(name)
        if n_chunks == 0 or n_chunks > 2000:
            continue
        w = gr.plan_words(ptr, n, E, chunk, SENT)
        firsts = gr.check_plan(w, ptr, n, E, chunk, SENT)
        descs = w[4:4 + 4 * n_chunks].reshape(n_chunks, 4)
        for s in firsts:                                        # every row's chunks k = nc - 1, ..., 0 in its slots
            descs[s:s + descs[s, 3]] = descs[s:s + descs[s, 3]][::-1].copy()
        with pytest.raises(AssertionError):
            gr.check_plan(w, ptr, n, E, chunk, SENT)
        told['chunks in reversed slot order'].append(name)
    print('[mutants] plans:', {k: len(v) for k, v in told.items()})
    for k, names in told.items():
        assert names, f'no input of the GPU file tells the mutant "{k}" from the model'
    assert any(n.startswith(('s-ladder', 'ladder')) for n in told['row cut at deg >= chunk'])


def test_check_plan_takes_any_row_order_and_nothing_else():
    g = gr.runner_graph('L', 64)
    ptr, n, E = np.asarray(g.rowptr), g.N, g.E
    n_long = gr.plan(ptr, n, 64)[1]
    for order in (None, np.arange(n_long)[::-1], np.random.default_rng(0).permutation(n_long)):
        w = np.concatenate([np.full(7, SENT, np.int32), gr.plan_words(ptr, n, E, 64, SENT, order), np.full(5, SENT, np.int32)])
        gr.check_plan(w, ptr, n, E, 64, SENT, origin=7)
    good = gr.plan_words(ptr, n, E, 64, SENT)
    n_chunks, off = int(good[0]), int(good[3])
    for word, what in ((4 + 4 * n_chunks, 'an unused descriptor slot'), (off + n_long, 'an unused list entry'),
                       (len(good) - 1, 'the last list entry'), (2, 'the row count'), (3, 'the list offset'),
                       (off, 'a list entry'), (5, 'a descriptor')):
        w = good.copy()
        w[word] = w[word] + 1 if w[word] != SENT else 0
        with pytest.raises(AssertionError):
            gr.check_plan(w, ptr, n, E, 64, SENT)
            pytest.fail(f'check_plan accepts a plan with {what} changed')
    w = np.concatenate([good, np.array([0], np.int32)])
    with pytest.raises(AssertionError):
        gr.check_plan(w, ptr, n, E, 64, SENT)
    dup = good.copy()
    dup[off + 1] = dup[off]                                     # one first chunk listed twice
    with pytest.raises(AssertionError):
        gr.check_plan(dup, ptr, n, E, 64, SENT)


def test_spos_inputs_tell_the_mutant_apart():
    told = []
    for name, ei, N, chunk in all_inputs():
        b = gr.graph_build(ei, N)
        want = gr.spos(b.eperm, b.cperm)
        assert np.array_equal(b.cperm[want], b.eperm) and np.array_equal(want, b.by_edge[b.eperm]), name
        if not np.array_equal(gr.spos(b.cperm, b.eperm), want):             # CSC position -> CSR position
            told.append(name)
    print('[mutants] spos inverted:', len(told))
    assert told, 'no input of the GPU file tells the mutant "spos inverted" from the model'


def active_mutant(rowptr, cscptr, N, which, kind):
    if kind == 'which bits swapped':
        which = {1: 2, 2: 1, 3: 3}[which]
    lst, ptr, count = gr.active(rowptr, cscptr, N, which)
    return (lst[:-1] if kind == '7 padding entries' else lst), ptr, count


def test_active_inputs_tell_the_mutants_apart():
    told = {'which bits swapped': [], '7 padding entries': []}
    for N in gr.ACTIVE_N:
        for kind in gr.ACTIVE_KINDS:
            rowptr, cscptr = gr.active_case(N, kind)
            assert len(rowptr) == len(cscptr) == N + 1 and rowptr[0] == cscptr[0] == 0
            for which in (1, 2, 3):
                want = gr.active(rowptr, cscptr, N, which)
                assert len(want[0]) == want[2] + 8 <= N + 8 and want[1][N] == want[2]
                for k in told:
                    got = active_mutant(rowptr, cscptr, N, which, k)
                    if not (len(got[0]) == len(want[0]) and same(got[:2], want[:2]) and got[2] == want[2]):
                        told[k].append((N, kind, which))
            if kind == 'all':
                assert gr.active(rowptr, cscptr, N, 1)[2] == N
            if kind == 'no-in-edge':
                assert gr.active(rowptr, cscptr, N, 1)[2] == 0 and gr.active(rowptr, cscptr, N, 2)[2] > 0
    print('[mutants] active:', {k: len(v) for k, v in told.items()})
    for k, cases in told.items():
        assert cases, f'no input of the GPU file tells the mutant "{k}" from the model'


# --------------------------------------------------------------------------------------------------------- capacity
def test_every_plan_fits_its_capacity():
    """chunks <= 2 * (E // chunk) + 2 and long rows <= max_chunks // 2 + 2 for every plan the GPU file builds; the
    full-plan graphs (E // chunk rows of chunk + 1 edges) reach max_chunks - 2, the most any graph of E edges can need:
    n long rows of c_i chunks hold more than sum (c_i - 1) * chunk edges, and c_i <= 2 (c_i - 1)."""
    most = {}
    for name, ptr, n, E, chunk in plan_inputs():
        _, n_long, n_chunks = gr.plan(ptr, n, chunk)
        mc = gr.max_chunks(E, chunk)
        assert n_chunks <= mc and n_long <= mc // 2 + 2, (name, n_chunks, n_long, mc)
        assert gr.plan_words_total(E, chunk) * 4 == 16 + 16 * mc + 4 * (mc // 2 + 2)
        most[name] = mc - n_chunks
    print('[capacity] slots left, tightest five:', sorted(most.items(), key=lambda kv: kv[1])[:5])
    for name in gr.FULL_PLAN_CASES:
        assert most[name + '/dst'] == 2 and most[name + '/src'] == 2, name
    # the 189- and 190-row graphs of 65-edge rows: 378 of 384 and 380 of 386 slots (E // 65 rows, three short of E // 64)
    assert most['s-N189-E12285-two-chunk-rows/dst'] == 6 and most['m-N190-E12350-two-chunk-rows/src'] == 6
