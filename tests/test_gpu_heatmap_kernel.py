"""ampconv_attn_heatmap (csrc/attn_heatmap.hip: heat_mfma, heat_generic, each with its LDS and its global accumulation
target) ONE C CALL AT A TIME through ctypes, against the fp64 model of tests/heatmap_reference.py.

Q and K lie in NaN margins and gaps (edge_layouts.place), edge_index and both position maps in -1 margins, the int64
tables inside sentinel-filled allocations whose inner part the test sets (edge_layouts.place_flat_int): after every call
nothing outside the tables may have changed.  The counts must equal the model's exactly, the sums lie within
heatmap_reference.share (the project's flat bar per weight, summed over a cell's terms, plus the fixed point's half
quantum; tests/test_heatmap_reference_cpu.py shows what it rejects), and wherever two calls add the same integers --
the two targets, layouts under one kernel, another prior_triples, a table cut out of a larger one, an edge list tiled
k times -- the tables are compared bit for bit.  Every case first asserts ON THE MODEL that at least a third of its
cells hold a term.  Every sweep names all its failing cases in one assertion.

Position maps (heatmap_reference): `unique` (a full read-out of every W[e, i, j]), `selected` (seeded features with
repeats inside nodes, 48 x 64 from two feature lists; on the 6-node graph S at L < 16 the lists shrink to 3 L x 4 L of
5 L features (4 at L = 1), because 6 L tokens cannot reach a third of 3072 cells), and `token` (rows = cols = L, every token
selected) for the edge lists of a few edges or of one destination, which fill a third of no larger table.
"""
import numpy as np
import pytest
import torch

import heatmap_reference as hr
import linear_reference as lr
from edge_layouts import LAYOUTS, alignment_bytes, place, place_flat_int
from edge_runner import graph, stream

from ampnet_amd import _lib, heatmap

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
BADARG = -1
INT32_MAX = 2 ** 31 - 1
SHARE = {}          # kernel -> the largest share of the bar used, printed whenever it rises


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    lib = _lib.load()
    assert lib.ampconv_attn_heatmap_shift() == hr.SHIFT == heatmap.SHIFT
    return lib


def sid(shape):
    return 'L{}dh{}H{}'.format(*shape)


class GraphS:
    """6 nodes, 70 edges (one window of 64 and six more), seeded, with multi-edges and self-loops."""
    N = 6
    rng = np.random.default_rng(31)
    src, dst = rng.integers(0, 6, 70), rng.integers(0, 6, 70)
    src[:4], dst[:4] = [2, 2, 4, 0], [5, 5, 4, 0]
    E = 70
    assert len(set(zip(src.tolist(), dst.tolist()))) < 70 and (src == dst).any()
    del rng


def selected(N, L):
    Lp = min(L, 16) if N < 16 else 16
    return hr.selected_maps(N, L, rows=3 * Lp, cols=4 * Lp, vocab=5 * Lp if Lp > 1 else 4)[:4]


class Operands:
    """Q, K of one (shape, node count, scale): the float32 tiles, their placements per layout, and the model's weights
    per (source, destination) pair."""

    def __init__(self, shape, N, scale=1):
        self.shape, self.N = shape, N
        self.Q = lr.tiles('random', shape, N) * np.float32(scale)
        self.K = lr.tiles('random', shape, N, seed=1) * np.float32(scale)
        self.placed, self.weights = {}, {}

    def views(self, layout):
        if layout not in self.placed:
            self.placed[layout] = place(self.Q, layout, F32, 'Q'), place(self.K, layout, F32, 'K')
        return self.placed[layout]

    def kernel(self, layout):
        L, dh, H = self.shape
        pq, pk = self.views(layout)
        if L <= 20 and dh in (16, 32) and alignment_bytes([pq.view, pk.view], 4) == 16:
            return f'heat_mfma dh{dh}'
        return 'heat_generic'

    def model(self, src, dst, maps, mask=None, N=None):
        S, cnt = hr.heat_tables(self.Q, self.K, src, dst, self.N if N is None else N, mask, *maps, weights=self.weights)
        assert hr.coverage(cnt) >= 1 / 3, f'{sid(self.shape)}: only {hr.coverage(cnt):.2f} of the cells hold a term'
        return S, cnt


def call(lib, ops, layout, src, dst, maps, *, mask=None, pre=None, prior=0, N=None, ei_skew=0, pos_skew=0):
    """One call -> (return code, sum, cnt as numpy int64 [rows, cols], problems).  pre: (sum, cnt) the tables hold
    before the call (default: zeros).  ei_skew / pos_skew: elements the index buffers begin behind a 256-byte boundary;
    a mask begins one byte behind one."""
    L, dh, H = ops.shape
    rowpos, colpos, rows, cols = maps
    E = len(src)
    pq, pk = ops.views(layout)
    pei = place_flat_int(np.stack([src, dst]).astype(np.int64), I64, skew=ei_skew)
    pr, pc = place_flat_int(rowpos, I32, skew=pos_skew), place_flat_int(colpos, I32, skew=pos_skew)
    tables = place_flat_int((rows, cols), I64), place_flat_int((rows, cols), I64)
    for p, v in zip(tables, pre if pre is not None else (np.zeros((rows, cols), np.int64),) * 2):
        p.backing[p.index.reshape(-1)] = torch.from_numpy(np.ascontiguousarray(v)).cuda().reshape(-1)
    mptr = None
    if mask is not None:
        mbuf = torch.full((E + 65,), 0xA5, dtype=torch.uint8, device='cuda:0')
        mbuf[1:1 + E] = torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
        mptr = mbuf.data_ptr() + 1
        assert mptr % 2 == 1
    rc = lib.ampconv_attn_heatmap(pq.view, pk.view, pei.ptr, E, ops.N if N is None else N, mptr, pr.ptr, pc.ptr, L, dh * H, H,
                                  rows, cols, tables[0].ptr, tables[1].ptr, prior, _lib.AMPCONV_F32, stream())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a faulted context tells nothing about any later call
        pytest.exit(f'the device reported {e} after ampconv_attn_heatmap at {sid(ops.shape)} {layout} E={E}', returncode=3)
    got = [p.backing[p.index.reshape(-1)].reshape(rows, cols).cpu().numpy() for p in tables]
    bad = [] if all(p.outside_intact() for p in tables) else ['memory around the tables was written']
    return rc, got[0], got[1], bad


def judge(kernel, name, got, ref, pre=None):
    """The bar -> a list of problems; keeps and prints the largest share per kernel."""
    rc, s, n, bad = got
    if rc != 0:
        return [f'{name}: returned {rc}'] + [f'{name}: {b}' for b in bad]
    if pre is not None:
        s, n = s - pre[0], n - pre[1]
    used = hr.share(s, n, *ref)
    if np.isfinite(used) and used > SHARE.get(kernel, 0.0):
        SHARE[kernel] = used
        print(f'[bar] {kernel}: {100 * used:.2f} % of the bar at {name}')
    if used == np.inf:
        bad = bad + [f'counts differ from the model in {int((n != ref[1]).sum())} cells, or a cell without a term holds a sum']
    elif used > 1:
        bad = bad + [f'{used:.3g} times the bar']
    return [f'{name}: {b}' for b in bad]


def same_bits(name, a, b):
    return [] if a[0] == b[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) else [f'{name}: tables differ']


def both_targets(lib, monkeypatch, ops, layout, src, dst, maps, name, ref, **kw):
    """The call as it ships and with the global target pinned: each against the model, the two bit for bit."""
    a = call(lib, ops, layout, src, dst, maps, **kw)
    monkeypatch.setenv('AMPCONV_HEATMAP_GLOBAL', '1')
    b = call(lib, ops, layout, src, dst, maps, **kw)
    monkeypatch.delenv('AMPCONV_HEATMAP_GLOBAL')
    k = ops.kernel(layout)
    return a, (judge(k, name, a, ref, kw.get('pre')) + judge(k, name + ' global', b, ref, kw.get('pre')) +
               same_bits(name + ': LDS target against global target', a, b))


def sweep_graph_s(lib, monkeypatch, shape, layout='nld'):
    """Graph S under the unique map and, on both targets, under the selected one -> (results, problems)."""
    L = shape[0]
    ops = Operands(shape, GraphS.N)
    name = f'{sid(shape)} {layout}'
    uni, sel = hr.unique_maps(GraphS.N, L), selected(GraphS.N, L)
    a = call(lib, ops, layout, GraphS.src, GraphS.dst, uni)
    failed = judge(ops.kernel(layout), name + ' unique', a, ops.model(GraphS.src, GraphS.dst, uni))
    b, bad = both_targets(lib, monkeypatch, ops, layout, GraphS.src, GraphS.dst, sel, name + ' selected',
                          ops.model(GraphS.src, GraphS.dst, sel))
    return ops, (a, b), failed + bad


# ---------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize('dh,H', [(32, 1), (32, 4), (16, 3)])
def test_every_token_count_mfma(dh, H, lib, monkeypatch):
    """L = 1..20: column_softmax's masks of the source tokens >= L (L <= 16: the whole second row tile) and table_pos'
    drop of the destination tokens >= L, at one head, several, and half-filled k-steps."""
    failed = []
    for L in range(1, 21):
        ops, _, bad = sweep_graph_s(lib, monkeypatch, (L, dh, H))
        assert ops.kernel('nld') == f'heat_mfma dh{dh}'
        failed += bad
    assert not failed, failed


@pytest.mark.parametrize('dh,H', [(1, 2), (3, 2), (50, 2), (64, 1)])
def test_every_token_count_generic(dh, H, lib, monkeypatch):
    """dh = 1, odd dh (dhp = dh | 1 = dh: no padding column), even dh; L past one wavefront (63, 64, 65, 70): the lane
    loops `j += 64` take a second turn.  At L = 70, dh = 64 the LDS request passes 48 KiB."""
    failed = []
    for L in list(range(1, 25)) + [63, 64, 65, 70]:
        ops, _, bad = sweep_graph_s(lib, monkeypatch, (L, dh, H))
        assert ops.kernel('nld') == 'heat_generic'
        failed += bad
    assert not failed, failed


@pytest.mark.parametrize('shape', [(20, 32, 4), (17, 16, 3)], ids=sid)
def test_unaligned_views_take_the_generic_kernel(shape, lib, monkeypatch):
    """The MFMA shapes on views that rule the MFMA kernel out (8- and 4-byte alignment): against the model, and
    against the MFMA kernel's tables of the same operands -- counts equal, sums through the bar only (two kernels)."""
    ops, (uni, sel), failed = sweep_graph_s(lib, monkeypatch, shape)
    assert ops.kernel('nld').startswith('heat_mfma')
    for layout in ('pad8', 'pad4'):
        other, (u2, s2), bad = sweep_graph_s(lib, monkeypatch, shape, layout)
        assert other.kernel(layout) == 'heat_generic'
        failed += bad
        for tag, m, g in (('unique', uni, u2), ('selected', sel, s2)):
            if not np.array_equal(m[2], g[2]):
                failed.append(f'{sid(shape)} {layout} {tag}: counts differ from the MFMA kernel\'s')
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('shape', [(20, 32, 4), (13, 16, 3), (40, 50, 2)], ids=sid)
def test_every_layout(shape, lib):
    g = graph('A')
    ops = Operands(shape, g.N)
    maps = selected(g.N, shape[0])
    ref = ops.model(g.src, g.dst, maps)
    failed, first = [], {}
    for layout in LAYOUTS + ('mixed',):
        got = call(lib, ops, layout, g.src, g.dst, maps)
        k = ops.kernel(layout)
        failed += judge(k, f'{sid(shape)} {layout}', got, ref)
        if k in first:
            failed += same_bits(f'{sid(shape)}: {layout} against {first[k][0]} (both {k})', got, first[k][1])
        else:
            first[k] = layout, got
    assert len(first) == (2 if shape[0] <= 20 else 1), list(first)
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------------- 4
def bad_edges(n, N):
    """n edges with one id outside [0, N): source -1, source N, destination N, destination 2^40 in turn."""
    src, dst = np.arange(n) % N, (np.arange(n) * 7 + 1) % N
    kind = np.arange(n) % 4
    src = np.where(kind == 0, -1, np.where(kind == 1, N, src))
    dst = np.where(kind == 2, N, np.where(kind == 3, 2 ** 40, dst))
    return src.astype(np.int64), dst.astype(np.int64)


@pytest.mark.parametrize('shape', [(20, 32, 4), (5, 6, 3)], ids=sid)
def test_window_edges_and_ignored_edges(shape, lib, monkeypatch):
    """window_scan's windows of 64: one edge, one short of a window, a window, one more, two, two and one.  Then edges
    the header says are ignored (a node id outside [0, N) -- window_scan tests the ids before anything is read through
    them) in the first and the last lane of a window and as a whole window; then N = 0, under which every edge is."""
    g = graph('A')
    ops = Operands(shape, g.N)
    k = ops.kernel('nld')
    tok = hr.token_maps(g.N, shape[0])
    failed = []
    for E in (1, 63, 64, 65, 128, 129):
        src, dst = g.src[:E], g.dst[:E]
        _, bad = both_targets(lib, monkeypatch, ops, 'nld', src, dst, tok, f'{sid(shape)} E={E}', ops.model(src, dst, tok))
        failed += bad
    maps = selected(g.N, shape[0])
    clean = call(lib, ops, 'nld', g.src, g.dst, maps)
    failed += judge(k, f'{sid(shape)} graph A', clean, ops.model(g.src, g.dst, maps))
    bs, bd = bad_edges(66, g.N)
    at = [64, 127 - 1, 192 - 2] + [192 - 2] * 63           # np.insert counts positions in the ORIGINAL list
    src, dst = np.insert(g.src, at, bs[[0, 1] + list(range(2, 66))]), np.insert(g.dst, at, bd[[0, 1] + list(range(2, 66))])
    live = hr.live_edges(src, dst, g.N)
    assert len(src) == g.E + 66 and len(live) == g.E and np.array_equal(src[live], g.src)
    dead = np.setdiff1d(np.arange(len(src)), live)
    assert dead.tolist() == [64, 127] + list(range(192, 256)), dead           # lanes 0 and 63 of window 1, all of window 3
    spliced, bad = both_targets(lib, monkeypatch, ops, 'nld', src, dst, maps, f'{sid(shape)} graph A + 66 ignored edges',
                                ops.model(src, dst, maps))
    failed += bad + same_bits(f'{sid(shape)}: with ignored edges against without', spliced, clean)
    rng = np.random.default_rng(3)
    pre = rng.integers(0, 2 ** 40, (2,) + clean[1].shape)
    rc, s, n, bad = call(lib, ops, 'nld', g.src, g.dst, maps, N=0, pre=pre)
    failed += bad + ([] if rc == 0 and np.array_equal(s, pre[0]) and np.array_equal(n, pre[1]) else
                     [f'{sid(shape)} N = 0: returned {rc} or changed the tables'])
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------------- 5
def wild_maps(N, L, rng):
    """The selected maps with positions outside the table mixed in: -7, rows (= 48, a valid COLUMN), cols, INT32_MAX and,
    as rows, 48..63, which only a comparison against the wrong extent would take; node 7 (graph A's hub source) with no
    selected source token, node 21 with no selected destination token."""
    rowpos, colpos, rows, cols = selected(N, L)
    assert (rows, cols) == (48, 64)
    rowpos, colpos = rowpos.copy(), colpos.copy()
    for pos, values in ((rowpos, [-7, rows, cols, INT32_MAX, 55, 63]), (colpos, [-7, cols, INT32_MAX, -2 ** 31, 48, 63])):
        where = rng.random(pos.shape) < 0.3
        pos[where] = rng.choice(values, int(where.sum()))
    rowpos[7], colpos[21] = [-1, rows] * (L // 2), [cols, -7] * (L // 2)
    assert (colpos >= rows).any() and (rowpos == rows).any()
    return rowpos, colpos, rows, cols


@pytest.mark.parametrize('shape', [(20, 32, 4), (40, 50, 2)], ids=sid)
def test_selection_rules(shape, lib, monkeypatch):
    """Any non-zero mask byte selects, at an odd address; edge_index 8 bytes and the maps 4 bytes off a 16-byte
    boundary; positions outside [0, rows) / [0, cols) with rows < cols; nodes without a selected token on one side;
    tables that already hold values; prior_triples at its largest."""
    g = graph('A')
    L = shape[0]
    ops = Operands(shape, g.N)
    rng = np.random.default_rng(77)
    maps = wild_maps(g.N, L, rng)
    mask = rng.choice(np.array([0, 1, 2, 255], np.uint8), g.E)
    ref = ops.model(g.src, g.dst, maps, mask)
    assert g.outdeg[7] > 128 and g.indeg[21] > 0
    quiet = np.where((g.src == 7) | (g.dst == 21), 0, mask)
    assert np.array_equal(hr.heat_tables(ops.Q, ops.K, g.src, g.dst, g.N, quiet, *maps, weights=ops.weights)[1], ref[1])
    pre = rng.integers(0, 2 ** 40, (2,) + ref[0].shape)
    kw = dict(mask=mask, pre=pre, ei_skew=1, pos_skew=1)
    name = f'{sid(shape)} selection'
    first, failed = both_targets(lib, monkeypatch, ops, 'nld', g.src, g.dst, maps, name, ref, **kw)
    top = heatmap.MAX_TRIPLES - g.E * L * L
    failed += same_bits(name + ': prior_triples at its largest against 0', first,
                        call(lib, ops, 'nld', g.src, g.dst, maps, prior=top, **kw))
    rc, s, n, bad = call(lib, ops, 'nld', g.src, g.dst, maps, prior=top + 1, **kw)
    failed += bad + ([] if rc == BADARG and np.array_equal(s, pre[0]) and np.array_equal(n, pre[1]) else
                     [name + f': one triple too many returned {rc} or changed the tables'])
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------------- 6
def test_the_4096_cell_boundary(lib):
    """64 x 64 = kLdsCells cells take the LDS target, 64 x 65 the global one; columns 0..63 hold the same bits."""
    g = graph('A')
    shape = (20, 32, 4)
    ops = Operands(shape, g.N)
    rowpos, colpos, rows, cols, _ = hr.selected_maps(g.N, shape[0], rows=64, cols=65, vocab=80)
    assert (colpos == 64).any()
    large, small = (rowpos, colpos, 64, 65), (rowpos, np.where(colpos == 64, -1, colpos).astype(np.int32), 64, 64)
    ref = ops.model(g.src, g.dst, large)
    assert ref[1][:, 64].sum() > 0
    a, b = call(lib, ops, 'nld', g.src, g.dst, small), call(lib, ops, 'nld', g.src, g.dst, large)
    k = ops.kernel('nld')
    failed = judge(k, '64 x 64', a, ops.model(g.src, g.dst, small)) + judge(k, '64 x 65', b, ref)
    failed += same_bits('columns 0..63 of 64 x 65 against 64 x 64', a, (b[0], b[1][:, :64], b[2][:, :64]))
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------------- 7
# Edges past which a wave takes a second window: the grid is capped at `max_blocks = mfma ? 1024 : 4096` workgroups
# (csrc/attn_heatmap.hip:346) of kHeatWaves = 8 waves (:34) or of one wave, a window is 64 edges.
CAP = {(2, 16, 1): 1024 * 8 * 64, (2, 3, 2): 4096 * 64}


@pytest.mark.parametrize('shape', list(CAP), ids=sid)
def test_a_second_window_per_wave(shape, lib, monkeypatch):
    """The integer tables are exactly additive: the 129-edge list of the window test (tables T, held to the model
    there and here) tiled k times, then its first 65 edges (tables R), just past TWICE the grid's capacity -- every wave
    takes a second window, the first a third -- gives k T + R bit for bit on either target."""
    g = graph('A')
    ops = Operands(shape, g.N)
    maps = hr.token_maps(g.N, shape[0])
    src, dst = g.src[:129], g.dst[:129]
    k = -(-(2 * CAP[shape] + 1 - 65) // 129)
    long_src, long_dst = np.concatenate([np.tile(src, k), src[:65]]), np.concatenate([np.tile(dst, k), dst[:65]])
    assert 2 * CAP[shape] < len(long_src) <= 2 * CAP[shape] + 129
    assert ops.kernel('nld') == ('heat_mfma dh16' if shape[1] == 16 else 'heat_generic')
    T = call(lib, ops, 'nld', src, dst, maps)
    R = call(lib, ops, 'nld', src[:65], dst[:65], maps)
    failed = (judge(ops.kernel('nld'), f'{sid(shape)} E=129', T, ops.model(src, dst, maps)) +
              judge(ops.kernel('nld'), f'{sid(shape)} E=65', R, ops.model(src[:65], dst[:65], maps)))
    want = (0, k * T[1] + R[1], k * T[2] + R[2])
    for target in ('LDS', 'global'):
        if target == 'global':
            monkeypatch.setenv('AMPCONV_HEATMAP_GLOBAL', '1')
        got = call(lib, ops, 'nld', long_src, long_dst, maps)
        failed += got[3] + same_bits(f'{sid(shape)} E={len(long_src)} {target} against k T + R', got, want)
    monkeypatch.delenv('AMPCONV_HEATMAP_GLOBAL')
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize('shape,scale', [((20, 32, 4), 8), ((13, 16, 3), 8), ((40, 50, 2), 3)], ids=lambda v: str(v))
def test_large_scores(shape, scale, lib, monkeypatch):
    """Both operands times `scale`: a fifth to two thirds of the weights quantise to 0 and single ones pass 0.7 (a head
    mean: 1 only where every head agrees); no sum passes cnt 2^SHIFT."""
    g = graph('A')
    failed = []
    for gname, src, dst, N, maps in (('A', g.src, g.dst, g.N, selected(g.N, shape[0])),
                                     ('S', GraphS.src, GraphS.dst, GraphS.N, hr.unique_maps(GraphS.N, shape[0]))):
        ops = Operands(shape, N, scale)
        ref = ops.model(src, dst, maps)
        W = np.stack(list(ops.weights.values()))
        assert (W < 2.0 ** -(hr.SHIFT + 1)).mean() > 0.2 and W.max() > 0.7
        got, bad = both_targets(lib, monkeypatch, ops, 'nld', src, dst, maps, f'{sid(shape)} x{scale} graph {gname}', ref)
        failed += bad
        if (got[1] > got[2] * 2 ** hr.SHIFT).any():
            failed.append(f'{sid(shape)} x{scale} graph {gname}: a sum exceeds cnt 2^SHIFT')
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------------- 9
def test_lds_limits_of_the_generic_kernel(lib):
    """dh = 1, H = 2: the tiles take (L^2 + 5 L) 4 bytes, 162 384 at L = 199 -- the largest L under the 160 KiB cap of
    set_dynamic_lds.  There a 2 x 2 table (48 bytes) still fits behind the tiles (LDS target), a 64 x 64 one (48 KiB)
    does not (global target); at L = 200 the tiles alone pass the cap: AMPCONV_E_BADARG, nothing written."""
    N, src, dst = 3, np.array([0, 1, 2, 1]), np.array([1, 2, 0, 1])
    L = 199
    assert (L * L + 5 * L) * 4 <= 160 * 1024 < ((L + 1) ** 2 + 5 * (L + 1)) * 4
    assert (L * L + 5 * L) * 4 + 4 * 12 <= 160 * 1024 < (L * L + 5 * L) * 4 + 4096 * 12
    ops = Operands((L, 1, 2), N)
    rowpos, colpos, rows, cols, _ = hr.selected_maps(N, L, rows=64, cols=64, vocab=80)
    large = rowpos, colpos, 64, 64
    small = np.where(rowpos < 2, rowpos, -1).astype(np.int32), np.where(colpos < 2, colpos, -1).astype(np.int32), 2, 2
    a, b = call(lib, ops, 'nld', src, dst, small), call(lib, ops, 'nld', src, dst, large)
    failed = (judge('heat_generic', 'L199 2 x 2', a, ops.model(src, dst, small)) +
              judge('heat_generic', 'L199 64 x 64', b, ops.model(src, dst, large)))
    failed += same_bits('L199: the 2 x 2 table against the corner of the 64 x 64 one', a, (b[0], b[1][:2, :2], b[2][:2, :2]))
    ops = Operands((L + 1, 1, 2), N)
    rowpos, colpos, rows, cols, _ = hr.selected_maps(N, L + 1, rows=2, cols=2, vocab=3)
    pre = np.random.default_rng(9).integers(0, 2 ** 40, (2, 2, 2))
    rc, s, n, bad = call(lib, ops, 'nld', src, dst, (rowpos, colpos, 2, 2), pre=pre)
    failed += bad + ([] if rc == BADARG and np.array_equal(s, pre[0]) and np.array_equal(n, pre[1]) else
                     [f'L200: returned {rc} or changed the tables'])
    assert not failed, failed
