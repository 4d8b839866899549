"""The three edge passes of the C ABI (include/ampconv.h: ampconv_fwd_edge, ampconv_bwd_edge_dst, ampconv_bwd_edge_src
and their _planes / _scaled siblings), ONE PASS AT A TIME, through ctypes, on strided and offset views.

Every other GPU test reaches these kernels through the layer with the one stride pattern conv/functional.py builds.
Here each pass gets independent N(0, 1) operands placed under the layouts of tests/edge_layouts.py (NaN around every
input, a sentinel around and inside every output) and is held against the per-pass fp64 model of tests/edge_reference.py;
ampconv_edge_family says which kernel family a call took, so "the misaligned view fell back to the next family" is
asserted, not hoped for.

Tolerances (the project's own bars, SURVEY.md 8c, against fp64):
  fp32 storage   O, dQ (means over a row's edges) and dK, dV of sources with at most 12 out-edges: FLAT atol 1e-5,
                 rtol 1e-4; dK, dV of the hub source (sums over ~160 edges): atol scaled by max |want|
                 (assert_close_scaled(scaled=True), as test_random_shapes_mfma_vs_generic kind 2 does for such sums)
  bf16 storage   atol 2e-2, rtol 2e-2 (test_bf16_storage), the reference computed from the bf16-rounded operands
  _planes, _scaled: the fp32 bars.
"""
import functools
import math

import numpy as np
import pytest
import torch

import edge_reference as er
from conftest import assert_close_scaled
from edge_layouts import alignment_bytes, place, read

from ampnet_amd import _lib

gpu = pytest.mark.gpu

F32, BF16 = 'f32', 'bf16'
B16, SMALL, MFMA, BLOCK, GEN = (_lib.FAMILY_BF16_MFMA, _lib.FAMILY_SMALL, _lib.FAMILY_MFMA, _lib.FAMILY_BLOCK,
                                _lib.FAMILY_GENERIC)
BADARG, EDTYPE = -1, -2
FAMILY_NAME = {B16: 'bf16-mfma', SMALL: 'small', MFMA: 'mfma', BLOCK: 'block', GEN: 'generic', BADARG: 'E_BADARG',
               EDTYPE: 'E_DTYPE'}
# the five kinds of call: (pass, statistics hand-off)
FWD, DST, DST_S, SRC, SRC_S = range(5)
CALLS = ((_lib.PASS_FWD, 0), (_lib.PASS_DST, 0), (_lib.PASS_DST, 1), (_lib.PASS_SRC, 0), (_lib.PASS_SRC, 1))
CALL_NAME = ('fwd', 'dst', 'dst+stats', 'src', 'src+stats')

# ---- the family table: written from the wording of include/ampconv.h ("which kernels serve a call"), per
# (storage, shape (L, dh, H)) and per alignment class of the call's views in bytes -> the family (or error code) of
# (fwd, dst, dst + stats, src, src + stats).  Read against the predicates of csrc/edge_api.hip: they agree; what the
# header did not say before this table was written, and says now: a statistics buffer is taken only by the family
# ampconv_softmax_stats_bytes sized it for (E_BADARG at every short-sequence shape, at the bf16 MFMA shapes, and at the
# fp32 MFMA shapes on views that family cannot take); the workgroup-per-unit source pass exists only with statistics
# (fp32: generic without; bf16: E_DTYPE without).
_ONE_WAVE = {16: (MFMA,) * 5, 8: (BLOCK, BLOCK, BADARG, GEN, BADARG), 4: (GEN, GEN, BADARG, GEN, BADARG)}
_SMALL_V2 = {16: (SMALL, SMALL, BADARG, SMALL, BADARG), 8: (SMALL, SMALL, BADARG, SMALL, BADARG),
             4: (GEN, GEN, BADARG, GEN, BADARG)}
_SMALL_V1 = {a: (SMALL, SMALL, BADARG, SMALL, BADARG) for a in (16, 8, 4)}
_SMALL_V4 = {16: (SMALL, SMALL, BADARG, SMALL, BADARG), 8: (BLOCK, BLOCK, BADARG, GEN, BADARG),
             4: (GEN, GEN, BADARG, GEN, BADARG)}
_PER_UNIT = {16: (BLOCK, BLOCK, BLOCK, GEN, BLOCK), 8: (BLOCK, BLOCK, BLOCK, GEN, BLOCK),
             4: (GEN, GEN, BADARG, GEN, BADARG)}
_GENERIC = {a: (GEN, GEN, BADARG, GEN, BADARG) for a in (16, 8, 4)}
_BF_ONE_WAVE = {16: (B16, B16, BADARG, B16, BADARG), 8: (BLOCK, BLOCK, BADARG, EDTYPE, BADARG),
                4: (BLOCK, BLOCK, BADARG, EDTYPE, BADARG)}
_BF_PER_UNIT = {a: (BLOCK, BLOCK, BLOCK, EDTYPE, BLOCK) for a in (16, 8, 4)}
TABLE = {
    # one wave per (row, head), fp32 MFMA: full tile / batched tails / no tail / a quarter tile
    (F32, (20, 32, 2)): _ONE_WAVE, (F32, (17, 16, 3)): _ONE_WAVE, (F32, (13, 32, 1)): _ONE_WAVE,
    (F32, (5, 16, 2)): _ONE_WAVE,
    # short sequences: 2, 1, 2 and 4 channels per lane
    (F32, (1, 16, 8)): _SMALL_V2, (F32, (2, 16, 2)): _SMALL_V1, (F32, (4, 32, 4)): _SMALL_V2,
    (F32, (2, 32, 8)): _SMALL_V4,
    # workgroup per unit: dh % 4 == 2 / 3 token tiles, dh = 12 / 4 token tiles, two k-steps / 2 token tiles
    (F32, (40, 50, 2)): _PER_UNIT, (F32, (33, 12, 2)): _PER_UNIT, (F32, (64, 64, 1)): _PER_UNIT,
    (F32, (24, 64, 2)): _PER_UNIT,
    # odd dh; dh > 64
    (F32, (7, 5, 3)): _GENERIC, (F32, (3, 96, 1)): _GENERIC,
    (BF16, (20, 32, 2)): _BF_ONE_WAVE, (BF16, (13, 16, 2)): _BF_ONE_WAVE,
    (BF16, (40, 50, 2)): _BF_PER_UNIT,
}
LAYOUT_IDS = ('nld', 'packed3', 'nhld', 'hnld', 'lnd', 'pad16', 'pad8', 'pad4', 'mixed')


def layouts_of(dtype):
    return tuple(l for l in LAYOUT_IDS if not (dtype == BF16 and l == 'pad4'))


ALL_CASES = [(dt, shape, lay) for (dt, shape) in TABLE for lay in layouts_of(dt)]


def case_id(c):
    dt, (L, dh, H), lay = c[:3]
    return '-'.join([dt, f'L{L}dh{dh}H{H}', lay] + [str(x) for x in c[3:]])


TDT = {F32: torch.float32, BF16: torch.bfloat16}
CODE = {F32: _lib.AMPCONV_F32, BF16: _lib.AMPCONV_BF16}
TOL = {F32: dict(atol=1e-5, rtol=1e-4), BF16: dict(atol=2e-2, rtol=2e-2)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda:0')


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------- graphs
class Graph:
    def __init__(self, name, src, dst, N, n_rows):
        self.name, self.N, self.n_rows = name, N, n_rows
        self.src, self.dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        self.E = len(self.src)
        self.rowptr, self.col = er.csr_of(self.src, self.dst, N)
        self.indeg = np.bincount(self.dst, minlength=N)
        self.outdeg = np.bincount(self.src, minlength=N)
        self._csr = None

    def csr(self):
        """ampconv_graph_build with the chunk that ships below a million edges (64), plans included."""
        if self._csr is None:
            from ampnet_amd import EdgeCSR
            assert _lib.hub_chunk(self.E) == 64
            self._csr = EdgeCSR(torch.from_numpy(np.stack([self.src, self.dst])).cuda(), self.N)
        return self._csr


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == 'A':
        # 64 nodes, 703 edges.  Nodes 0..49 send: 8 random edges each, 3 to node 3 (multi-edges: in-degree ~160, a long
        # CSR segment) and receive 3 from node 7 (out-degree ~160, a long CSC segment); self-loops on 3, 5, 7.  Node 50
        # receives nothing, 50..57 send nothing, 58..63 are isolated.  Every source but node 7 has at most 12 out-edges.
        rng = np.random.default_rng(11)
        src = [np.arange(150) % 50, np.full(150, 7), rng.permutation(np.tile(np.arange(50), 8)), [3, 5, 7]]
        d = rng.integers(0, 57, 400)
        dst = [np.full(150, 3), np.arange(150) % 50, d + (d >= 50), [3, 5, 7]]
        g = Graph('A', np.concatenate(src), np.concatenate(dst), 64, 64)
        assert g.E == 703 and g.indeg[3] > 128 and g.outdeg[7] > 128 and g.indeg[50] == 0
        assert (np.delete(g.outdeg, 7) <= 12).all() and not g.indeg[58:].any() and not g.outdeg[50:].any()
        return g
    if name == 'B':
        # 40 nodes, 160 edges, every degree <= 12 (no long segment: no plan); the passes get n_rows = 33, and rows
        # 33..35 HAVE edges: what stays untouched there is the row count's doing, not an empty row's
        rng = np.random.default_rng(12)
        src = rng.permutation(np.repeat(np.arange(40), np.arange(40) % 10))[:160]          # out-degrees 0..9
        dst = rng.permutation(np.repeat(np.arange(36), np.arange(36) % 9 + 1))[:160]       # in-degrees up to 9, 36..39: 0
        src[:4], dst[:4] = [1, 1, 9, 34], [2, 2, 9, 35]
        g = Graph('B', src, dst, 40, 33)
        assert g.indeg.max() <= 12 and g.outdeg.max() <= 12 and g.indeg[33:36].all() and g.outdeg[33:].any()
        return g
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def qidx_rows():
    """Graph C: 50 rows of 0..5 edges over 40 nodes, queries from random nodes (repeats, not the identity)."""
    rng = np.random.default_rng(13)
    deg = rng.integers(0, 6, 50)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col, qidx = rng.integers(0, 40, rowptr[-1]), rng.integers(0, 40, 50)
    assert (deg == 0).any() and len(set(qidx)) < 50 and (qidx != np.arange(50)).any()
    return rowptr, col, qidx


# ---------------------------------------------------------------------------------------- operands and references
@functools.lru_cache(maxsize=None)
def operands(dtype, shape, N, scale=1.0):
    """Q, K, V, dObar [N, L, H, dh], independent N(0, 1) (float64; bf16 storage: rounded to bf16 first)."""
    L, dh, H = shape
    rng = np.random.default_rng(1000 * L + 10 * dh + H)
    ops = [rng.standard_normal((N, L, H, dh)).astype(np.float32) * np.float32(scale) for _ in range(4)]
    if dtype == BF16:
        ops = [torch.from_numpy(t).bfloat16().float().numpy() for t in ops]
    return tuple(t.astype(np.float64) for t in ops)


@functools.lru_cache(maxsize=None)
def reference(dtype, shape, gname):
    """O, dQ, dK, dV of the whole graph (the passes' row counts select from them)."""
    g = graph(gname)
    Q, K, V, dO = operands(dtype, shape, g.N)
    return (er.fwd(Q, K, V, g.rowptr, g.col),) + er.bwd(Q, K, V, dO, g.rowptr, g.col)


# ------------------------------------------------------------------------------------------------------ the calls
def family(call, dtype, shape, views):
    L, dh, H = shape
    arr = (_lib.View * len(views))(*views)
    return _lib.load().ampconv_edge_family(CALLS[call][0], CODE[dtype], L, dh * H, H, CALLS[call][1], arr, len(views))


def expected_family(call, dtype, shape, views):
    return TABLE[dtype, shape][alignment_bytes(views, 2 if dtype == BF16 else 4)][call]


def hub(csr, side, L, D, tiles, keep):
    plan, n, ws = csr.hub_args(side, L, D, tiles)
    keep.append(ws)
    return plan, n, (ws.data_ptr() if ws is not None else None)


class Run:
    """One (storage, shape, layout, graph): the placed operands and what each call returned."""

    def __init__(self, dtype, shape, layout, gname):
        self.dtype, self.shape, self.layout, self.g = dtype, shape, layout, graph(gname)
        L, dh, H = shape
        self.ops = operands(dtype, shape, self.g.N)
        self.inp = {r: place(t, layout, TDT[dtype], r) for r, t in zip(('Q', 'K', 'V', 'dO'), self.ops)}
        self.out, self.fam, self.want, self.rc, self.problems, self.keep = {}, {}, {}, {}, [], []

    def views(self, *roles):
        return [self.inp[r].view for r in roles]

    def output(self, role):
        L, dh, H = self.shape
        return place((self.g.N, L, H, dh), self.layout, TDT[self.dtype], role)

    def check_written(self, label, p, n_rows, deg):
        """Sentinel intact outside the first n_rows nodes of the view, every element of them written, rows without
        edges exact zeros; files the logical result."""
        rows = slice(0, n_rows)
        if not p.outside_intact(rows):
            self.problems.append(f'{label}: bytes outside the output view (or behind row {n_rows}) were written')
        if p.unwritten(rows):
            self.problems.append(f'{label}: {p.unwritten(rows)} elements of the view were not written')
        got = read(p.backing, p.index)[:n_rows]
        if got[deg[:n_rows] == 0].any():
            self.problems.append(f'{label}: rows without edges are not exact zeros')
        self.out[label] = got

    def check_untouched(self, label, *placed):
        for p in placed:
            if p.unwritten() != p.index.numel() or not p.outside_intact():
                self.problems.append(f'{label}: an error code was returned but the output buffer was written')

    def query(self, call, views):
        self.fam[call] = family(call, self.dtype, self.shape, views)
        self.want[call] = expected_family(call, self.dtype, self.shape, views)
        return self.fam[call]

    def stats_buffer(self):
        """Sized by ampconv_softmax_stats_bytes; where that is 0 the passes must REFUSE a buffer -- the one handed over
        to see that is still as large as any family could want (40 or 32 ceil(L / 16) floats per (edge, head)), so that
        a pass that wrongly took it would stay inside it."""
        L, dh, H = self.shape
        nb = _lib.load().ampconv_softmax_stats_bytes(self.g.E, L, dh * H, H, CODE[self.dtype])
        return torch.empty(max(nb // 4, self.g.E * H * max(40, 32 * ((L + 15) // 16))), device='cuda:0')

    def forward(self):
        lib, g, (L, dh, H) = _lib.load(), self.g, self.shape
        csr, O = g.csr(), self.output('out0')
        views = self.views('Q', 'K', 'V') + [O.view]
        f = self.query(FWD, views)
        rc = lib.ampconv_fwd_edge(*views[:3], csr.rowptr.data_ptr(), csr.col.data_ptr(), None, g.n_rows, L, dh * H, H,
                                  O.view, *hub(csr, 'dst', L, dh * H, 1, self.keep), CODE[self.dtype], stream())
        self.rc[FWD] = rc
        if f < 0 or rc != 0:
            self.check_untouched('O', O)
        else:
            self.check_written('O', O, g.n_rows, g.indeg)

    def backward(self, with_stats):
        """The destination pass, then the source pass (which reads the statistics the destination pass left)."""
        lib, g, (L, dh, H) = _lib.load(), self.g, self.shape
        D, csr, code, tag = dh * H, g.csr(), CODE[self.dtype], '/stats' if with_stats else ''
        stats = self.stats_buffer() if with_stats else None
        sp = (csr.csc_positions().data_ptr(), stats.data_ptr()) if with_stats else (None, None)
        cd, cs = (DST_S, SRC_S) if with_stats else (DST, SRC)
        dQ = self.output('out0')
        views = self.views('Q', 'K', 'V', 'dO') + [dQ.view]
        fd = self.query(cd, views)
        rc = lib.ampconv_bwd_edge_dst(*views[:4], csr.rowptr.data_ptr(), csr.col.data_ptr(), g.n_rows, L, D, H, dQ.view,
                                      *hub(csr, 'dst', L, D, 1, self.keep), *sp, None, code, stream())
        self.rc[cd] = rc
        if fd < 0 or rc != 0:
            self.check_untouched('dQ' + tag, dQ)
        else:
            self.check_written('dQ' + tag, dQ, g.n_rows, g.indeg)
        dK, dV = self.output('out0'), self.output('out1')
        views = self.views('Q', 'K', 'V', 'dO') + [dK.view, dV.view]
        fs = self.query(cs, views)
        if with_stats and fs >= 0:
            if fd < 0:
                return                                            # no statistics were written: nothing to hand over
            if g.n_rows < g.N:
                # the source pass reads the statistics of EVERY in-edge of its sources: fill them for all rows first
                scratch = self.output('out0')
                _lib.check(lib.ampconv_bwd_edge_dst(*views[:4], csr.rowptr.data_ptr(), csr.col.data_ptr(), g.N, L, D, H,
                                                    scratch.view, None, 0, None, *sp, None, code, stream()),
                           'dst, all rows')
        rc = lib.ampconv_bwd_edge_src(*views[:4], csr.cscptr.data_ptr(), csr.crow.data_ptr(), csr.cinv.data_ptr(),
                                      g.n_rows, L, D, H, dK.view, dV.view, *hub(csr, 'src', L, D, 2, self.keep), sp[1],
                                      None, code, stream())
        self.rc[cs] = rc
        if fs < 0 or rc != 0:
            self.check_untouched('dK' + tag, dK, dV)
        else:
            self.check_written('dK' + tag, dK, g.n_rows, g.outdeg)
            self.check_written('dV' + tag, dV, g.n_rows, g.outdeg)


LABEL_CALL = {'O': FWD, 'dQ': DST, 'dQ/stats': DST_S, 'dK': SRC, 'dV': SRC, 'dK/stats': SRC_S, 'dV/stats': SRC_S}


@functools.lru_cache(maxsize=None)
def run(dtype, shape, layout, gname):
    """All five calls of one (storage, shape, layout, graph), once: compared with the fp64 model and with the `nld` run
    right away, so that what stays cached is the verdicts (and, for `nld`, the outputs the other layouts are compared
    with), not a few hundred megabytes of outputs."""
    r = Run(dtype, shape, layout, gname)
    r.forward()
    r.backward(False)
    r.backward(True)
    torch.cuda.synchronize()
    r.inp = r.keep = None
    g = r.g
    want = dict(zip(('O', 'dQ', 'dK', 'dV'), (t[:g.n_rows] for t in reference(dtype, shape, gname))))
    r.failures, r.vs_nld = [], {}
    base = r if layout == 'nld' else run(dtype, shape, 'nld', gname)
    for label, got in r.out.items():
        kind = label.split('/')[0]
        try:
            compare(r, label, want[kind], g.outdeg[:g.n_rows] if kind in ('dK', 'dV') else None)
        except AssertionError as e:
            r.failures.append(str(e))
        call = LABEL_CALL[label]
        if label in base.out and base.fam[call] == r.fam[call]:
            r.vs_nld[label] = (r.fam[call], float(np.abs(got - base.out[label]).max()), np.array_equal(got, base.out[label]))
    r.labels = set(r.out)
    if layout != 'nld':
        r.out = None
    return r


def compare(r, label, want, outdeg=None):
    """One output tensor of a run against the fp64 model at the module's bars."""
    got, tol = r.out[label], TOL[r.dtype]
    name = f'{case_id((r.dtype, r.shape, r.layout, r.g.name))} {label} [{FAMILY_NAME[r.fam[LABEL_CALL[label]]]}]'
    assert np.isfinite(got).all(), f'{name}: non-finite values (NaN from a gap or a margin?)'
    if outdeg is None or (outdeg <= 12).all():
        assert_close_scaled(got, want, name, scaled=False, **tol)
        return
    few = outdeg <= 12
    assert_close_scaled(got[few], want[few], name + ' (<= 12 out-edges)', scaled=False, **tol)
    # a hub source's rows are sums over ~160 edges of O(1) terms: the absolute bar scales with their magnitude
    assert_close_scaled(got[~few], want[~few], name + ' (hub source)', scaled=True, **tol)


# ----------------------------------------------------------------------------------------------------------- tests
def test_family_follows_the_views():
    """ampconv_edge_family against TABLE for every (shape, layout, pass, statistics on / off): the views are real
    placements (their base addresses included).  The call launches nothing and reads no device memory, so this test runs
    on host buffers, without a GPU."""
    seen = set()
    for dtype, shape, layout in ALL_CASES:
        L, dh, H = shape
        keep = {r: place((8, L, H, dh), layout, TDT[dtype], r, device='cpu') for r in ('Q', 'K', 'V', 'dO', 'out0', 'out1')}
        ph = {r: p.view for r, p in keep.items()}
        for call in range(5):
            roles = (('Q', 'K', 'V', 'out0'), ('Q', 'K', 'V', 'dO', 'out0'), ('Q', 'K', 'V', 'dO', 'out0'),
                     ('Q', 'K', 'V', 'dO', 'out0', 'out1'), ('Q', 'K', 'V', 'dO', 'out0', 'out1'))[call]
            views = [ph[r] for r in roles]
            got, want = family(call, dtype, shape, views), expected_family(call, dtype, shape, views)
            assert got == want, (f'{case_id((dtype, shape, layout))} {CALL_NAME[call]}: {FAMILY_NAME.get(got, got)}, '
                                 f'the header says {FAMILY_NAME[want]}')
            seen.add((dtype, want))
    # the cases reach every family (and both refusals) of both storages
    assert {(F32, f) for f in (SMALL, MFMA, BLOCK, GEN, BADARG)} | {(BF16, f) for f in (B16, BLOCK, EDTYPE, BADARG)} <= seen
    lib = _lib.load()
    held = place((8, 20, 2, 32), 'nld', torch.float32, 'out0', device='cpu')
    v = held.view
    arr = (_lib.View * 4)(v, v, v, v)
    assert lib.ampconv_edge_family(3, 0, 20, 64, 2, 0, arr, 4) == BADARG          # no such pass
    assert lib.ampconv_edge_family(0, 0, 20, 64, 2, 1, arr, 4) == BADARG          # the forward pass has no statistics
    assert lib.ampconv_edge_family(0, 0, 20, 64, 3, 0, arr, 4) == BADARG          # D % H
    assert lib.ampconv_edge_family(0, 7, 20, 64, 2, 0, arr, 4) == EDTYPE
    assert lib.ampconv_edge_family(0, 0, 20, 64, 2, 0, None, 0) == MFMA           # the shape alone


@gpu
@pytest.mark.parametrize('case', [c + (g,) for c in ALL_CASES for g in 'AB'], ids=case_id)
def test_pass_on_layout_vs_fp64(case, dev):
    """Forward, destination and source pass, without and with the statistics hand-off, on graph A (long-segment plans
    on both sides) and graph B (no plan, n_rows = 33 of 40), against the fp64 model; the family each call took is the
    table's; an error code leaves every output byte alone."""
    dtype, shape, layout, gname = case
    r = run(dtype, shape, layout, gname)
    print('families:', ', '.join(f'{CALL_NAME[c]}={FAMILY_NAME.get(f, f)}' for c, f in sorted(r.fam.items())))
    assert not r.problems, r.problems
    for call, f in r.fam.items():
        want = r.want[call]
        assert f == want, f'{CALL_NAME[call]}: family {FAMILY_NAME.get(f, f)}, expected {FAMILY_NAME[want]}'
        if call in r.rc:
            assert r.rc[call] == (f if f < 0 else 0), f'{CALL_NAME[call]}: returned {r.rc[call]}, family query {f}'
    # every pass ran: fp32 always has a source pass without statistics, bf16 one with or without them
    assert {'O', 'dQ'} <= r.labels and r.labels & {'dK', 'dK/stats'} and r.labels & {'dV', 'dV/stats'} or \
        TABLE[dtype, shape] is _BF_ONE_WAVE and {'O', 'dQ'} <= r.labels
    assert not r.failures, r.failures


@gpu
@pytest.mark.parametrize('dtype,shape', list(TABLE), ids=lambda x: x if isinstance(x, str) else 'L%ddh%dH%d' % x)
def test_layouts_agree_with_the_canonical_layout(dtype, shape, dev):
    """Every layout against the `nld` run of the same call, where both took the same family.

    BITWISE for the generic, short-sequence, fp32 MFMA and bf16 MFMA families: their kernel variant follows from the
    shape (and the environment) alone, every lane loads the same elements into the same registers / LDS slots under any
    strides (edge_generic.hip: element-wise tile loads; edge_small.hip: the lane's vector width comes from
    small_shape(L, D, H), never from the views; edge_mfma.hip / edge_mfma_bf16.hip: always 16-byte loads), and the
    long-segment combine adds a row's partial tiles in the same fixed tree whether it stores vectors or scalars
    (hub.hip).  The workgroup-per-unit family picks its staging vector (4 or 2 elements) from the views: its cases are
    printed, and held to the fp64 bars of test_pass_on_layout_vs_fp64 only."""
    compared = 0
    for gname in 'AB':
        for layout in layouts_of(dtype)[1:]:
            r = run(dtype, shape, layout, gname)
            for label, (fam, diff, equal) in sorted(r.vs_nld.items()):
                print(f'{gname} {layout:8s} {label:9s} {FAMILY_NAME[fam]:9s} max |diff| vs nld {diff:.3e}')
                compared += 1
                if fam != BLOCK:
                    assert equal, (gname, layout, label, FAMILY_NAME[fam], diff)
    assert compared


@gpu
@pytest.mark.parametrize('dtype,shape', list(TABLE), ids=lambda x: x if isinstance(x, str) else 'L%ddh%dH%d' % x)
def test_forward_with_qidx(dtype, shape, dev):
    """Graph C: 50 rows whose queries come from qidx[r] (random nodes with repeats), on `nld`, `nhld` and `pad8`: every
    family that takes a query index."""
    lib = _lib.load()
    L, dh, H = shape
    rowptr, col, qidx = qidx_rows()
    Q, K, V, _ = operands(dtype, shape, 40)
    want = er.fwd(Q, K, V, rowptr, col, qidx)
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).cuda()
    rp, cl, qi = i32(rowptr), i32(col), i32(qidx)
    for layout in ('nld', 'nhld', 'pad8'):
        q, k, v = (place(t, layout, TDT[dtype], r) for t, r in zip((Q, K, V), 'QKV'))
        O = place((50, L, H, dh), layout, TDT[dtype], 'out0')
        views = [q.view, k.view, v.view, O.view]
        f = family(FWD, dtype, shape, views)
        assert f == expected_family(FWD, dtype, shape, views) and f >= 0
        _lib.check(lib.ampconv_fwd_edge(q.view, k.view, v.view, rp.data_ptr(), cl.data_ptr(), qi.data_ptr(), 50, L,
                                        dh * H, H, O.view, None, 0, None, CODE[dtype], stream()), 'fwd with qidx')
        torch.cuda.synchronize()
        assert O.outside_intact() and O.unwritten() == 0
        got = read(O.backing, O.index)
        assert not got[np.diff(rowptr) == 0].any()
        assert_close_scaled(got, want, f'{case_id((dtype, shape, layout))} qidx O [{FAMILY_NAME[f]}]', scaled=False,
                            **TOL[dtype])


def to_planes(x, bound):
    """[N, L, H, dh] float64 -> the plane format of include/ampconv.h as float32 BIT PATTERNS [N, L, H, dh]: the 4 dh bytes
    of a (token row, head) slot hold dh fp16 `hi` then dh fp16 `lo` of x * 2^(14 - floor(log2 bound)) (what
    tools/bench_kernels.py: to_planes builds for dh = 32)."""
    xs = torch.from_numpy(x * 2.0 ** (14 - math.floor(math.log2(bound)))).float()
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return torch.cat([hi, lo], dim=-1).contiguous().view(torch.float32).numpy()


def _finish(label, p, n, deg, want, name, outdeg=None):
    assert p.outside_intact(slice(0, n)), f'{name} {label}: bytes outside the output view were written'
    assert p.unwritten(slice(0, n)) == 0, f'{name} {label}: elements of the view were not written'
    got = read(p.backing, p.index)[:n]
    assert np.isfinite(got).all() and not got[deg[:n] == 0].any(), f'{name} {label}'
    few = np.ones(n, bool) if outdeg is None else outdeg[:n] <= 12
    assert_close_scaled(got[few], want[:n][few], f'{name} {label}', scaled=False, **TOL[F32])
    if not few.all():     # the hub source's sums over ~160 edges: the absolute bar scales with their magnitude
        assert_close_scaled(got[~few], want[:n][~few], f'{name} {label} (hub source)', scaled=True, **TOL[F32])


@gpu
@pytest.mark.parametrize('shape', [(20, 32, 2), (17, 16, 3)], ids=lambda s: 'L%ddh%dH%d' % s)
def test_planes_entry_points_on_layouts(shape, dev):
    """ampconv_*_edge_planes: operands in the plane format under `packed3` and `pad16` (head_stride must be dh), the
    fp32 outputs under `nld`, `nhld`, `pad16`; graph A with its plans.  An operand view with head_stride != dh is
    refused with every output byte intact."""
    lib, g = _lib.load(), graph('A')
    L, dh, H = shape
    D, csr, keep = dh * H, g.csr(), []
    assert lib.ampconv_planes_supported(L, D, H) == 1
    Q, K, V, dO = operands(F32, shape, g.N)
    O_, dQ_, dK_, dV_ = reference(F32, shape, 'A')
    gbar = dO / np.maximum(g.indeg, 1)[:, None, None, None]       # the plane passes carry no per-edge weight
    mq, mg = max(np.abs(t).max() for t in (Q, K, V)), np.abs(gbar).max()
    bounds = torch.tensor([2 * mq, 2 * mg, np.abs(V).max(), mg], dtype=torch.float32, device=dev)
    planes = [to_planes(t, 2 * mq) for t in (Q, K, V)] + [to_planes(gbar, 2 * mg)]
    stats = torch.empty(g.E * H * 40, device=dev)
    spos = csr.csc_positions()
    rp, cl, cp, cr = (t.data_ptr() for t in (csr.rowptr, csr.col, csr.cscptr, csr.crow))
    for lin in ('packed3', 'pad16'):
        q, k, v, go = (place(t, lin, torch.float32, r) for t, r in zip(planes, ('Q', 'K', 'V', 'dO')))
        for lout in ('nld', 'nhld', 'pad16'):
            for with_stats in (False, True):
                name = f'planes L{L}dh{dh}H{H} {lin}->{lout}' + ('/stats' if with_stats else '')
                sp = (spos.data_ptr(), stats.data_ptr()) if with_stats else (None, None)
                O, dQ, dK, dV = (place((g.N, L, H, dh), lout, torch.float32, 'out0') for _ in range(4))
                if not with_stats:
                    _lib.check(lib.ampconv_fwd_edge_planes(q.view, k.view, v.view, rp, cl, g.N, L, D, H, O.view,
                                                           *hub(csr, 'dst', L, D, 1, keep), bounds.data_ptr(), stream()), name)
                    _finish('O', O, g.N, g.indeg, O_, name)
                _lib.check(lib.ampconv_bwd_edge_dst_planes(q.view, k.view, v.view, go.view, rp, cl, g.N, L, D, H, dQ.view,
                                                           *hub(csr, 'dst', L, D, 1, keep), bounds.data_ptr(), *sp, None,
                                                           stream()), name)
                _lib.check(lib.ampconv_bwd_edge_src_planes(q.view, k.view, v.view, go.view, cp, cr, g.N, L, D, H, dK.view,
                                                           dV.view, *hub(csr, 'src', L, D, 2, keep), bounds.data_ptr(), sp[1],
                                                           None, stream()), name)
                torch.cuda.synchronize()
                _finish('dQ', dQ, g.N, g.indeg, dQ_, name)
                _finish('dK', dK, g.N, g.outdeg, dK_, name, g.outdeg)
                _finish('dV', dV, g.N, g.outdeg, dV_, name, g.outdeg)
    # operands whose heads are not dh apart: refused, nothing written
    bad = [place(t, 'nhld', torch.float32, r) for t, r in zip(planes, ('Q', 'K', 'V', 'dO'))]
    O, dK, dV = (place((g.N, L, H, dh), 'nld', torch.float32, 'out0') for _ in range(3))
    bv = [p.view for p in bad]
    assert lib.ampconv_fwd_edge_planes(*bv[:3], rp, cl, g.N, L, D, H, O.view, None, 0, None, bounds.data_ptr(),
                                       stream()) == BADARG
    assert lib.ampconv_bwd_edge_dst_planes(*bv, rp, cl, g.N, L, D, H, O.view, None, 0, None, bounds.data_ptr(), None,
                                           None, None, stream()) == BADARG
    assert lib.ampconv_bwd_edge_src_planes(*bv, cp, cr, g.N, L, D, H, dK.view, dV.view, None, 0, None,
                                           bounds.data_ptr(), None, None, stream()) == BADARG
    torch.cuda.synchronize()
    for p in (O, dK, dV):
        assert p.outside_intact() and p.unwritten() == p.index.numel()


@gpu
def test_scaled_entry_points_on_layouts(dev):
    """ampconv_*_edge_scaled at the reference's class default (40, 50, 2) under `nld`, `nhld`, `pad8`, graph A with its
    plans; 4-byte aligned views (`pad4`) are refused with every output byte intact."""
    lib, g, shape = _lib.load(), graph('A'), (40, 50, 2)
    L, dh, H = shape
    D, csr, keep = dh * H, g.csr(), []
    assert lib.ampconv_scaled_supported(L, D, H) == 1
    ops = operands(F32, shape, g.N)
    O_, dQ_, dK_, dV_ = reference(F32, shape, 'A')
    mq, mg = max(np.abs(t).max() for t in ops[:3]), np.abs(ops[3]).max()
    bounds = torch.tensor([mq, mg, np.abs(ops[2]).max(), mg], dtype=torch.float32, device=dev)
    stats = torch.empty(lib.ampconv_softmax_stats_bytes(g.E, L, D, H, _lib.AMPCONV_F32) // 4, device=dev)
    spos = csr.csc_positions()
    rp, cl, cp, cr, ci = (t.data_ptr() for t in (csr.rowptr, csr.col, csr.cscptr, csr.crow, csr.cinv))
    for layout in ('nld', 'nhld', 'pad8', 'pad4'):
        name = f'scaled L{L}dh{dh}H{H} {layout}'
        q, k, v, go = (place(t, layout, torch.float32, r) for t, r in zip(ops, ('Q', 'K', 'V', 'dO')))
        O, dQ, dK, dV = (place((g.N, L, H, dh), layout, torch.float32, 'out0') for _ in range(4))
        rcs = [lib.ampconv_fwd_edge_scaled(q.view, k.view, v.view, rp, cl, g.N, L, D, H, O.view,
                                           *hub(csr, 'dst', L, D, 1, keep), bounds.data_ptr(), stream()),
               lib.ampconv_bwd_edge_dst_scaled(q.view, k.view, v.view, go.view, rp, cl, g.N, L, D, H, dQ.view,
                                               *hub(csr, 'dst', L, D, 1, keep), bounds.data_ptr(), spos.data_ptr(),
                                               stats.data_ptr(), None, stream())]
        if layout == 'pad4':
            rcs.append(lib.ampconv_bwd_edge_src_scaled(q.view, k.view, v.view, go.view, cp, cr, ci, g.N, L, D, H, dK.view,
                                                       dV.view, None, 0, None, bounds.data_ptr(), stats.data_ptr(), None,
                                                       stream()))
            torch.cuda.synchronize()
            assert rcs == [BADARG] * 3, rcs
            for p in (O, dQ, dK, dV):
                assert p.outside_intact() and p.unwritten() == p.index.numel()
            continue
        rcs.append(lib.ampconv_bwd_edge_src_scaled(q.view, k.view, v.view, go.view, cp, cr, ci, g.N, L, D, H, dK.view,
                                                   dV.view, *hub(csr, 'src', L, D, 2, keep), bounds.data_ptr(),
                                                   stats.data_ptr(), None, stream()))
        torch.cuda.synchronize()
        assert rcs == [0, 0, 0], rcs
        _finish('O', O, g.N, g.indeg, O_, name)
        _finish('dQ', dQ, g.N, g.indeg, dQ_, name)
        _finish('dK', dK, g.N, g.outdeg, dK_, name, g.outdeg)
        _finish('dV', dV, g.N, g.outdeg, dV_, name, g.outdeg)


@gpu
@pytest.mark.parametrize('shape', [(20, 32, 2), (4, 32, 4), (40, 50, 2), (3, 96, 1)], ids=lambda s: 'L%ddh%dH%d' % s)
def test_out_absmax_on_layouts(shape, dev):
    """out_absmax of the fp32 backward passes (one shape per family).  Row-major outputs that ampconv_absmax can walk
    (`nld`, `packed3`, and `padrow`: 16-byte gaps behind every row): exactly the largest finite magnitude of what was
    written -- the sentinel in the gaps is a NaN and is not counted.  Any other output view (head-major, token-major,
    gaps BETWEEN nodes as in `pad16`, 8-byte alignment): AMPCONV_E_BADARG and not one byte written.  The destination
    pass of the one-wave-per-unit family records the maximum in its kernels and takes every layout it runs on."""
    lib, g = _lib.load(), graph('A')
    L, dh, H = shape
    D, csr, keep = dh * H, g.csr(), []
    ops = operands(F32, shape, g.N)
    q, k, v, go = (place(t, 'nld', torch.float32, r) for t, r in zip(ops, ('Q', 'K', 'V', 'dO')))
    rp, cl, cp, cr, ci = (t.data_ptr() for t in (csr.rowptr, csr.col, csr.cscptr, csr.crow, csr.cinv))
    nb = lib.ampconv_softmax_stats_bytes(g.E, L, D, H, _lib.AMPCONV_F32)
    stats = torch.empty(nb // 4, device=dev) if nb else None
    sp = (csr.csc_positions().data_ptr(), stats.data_ptr()) if nb else (None, None)
    for layout in ('nld', 'packed3', 'padrow', 'nhld', 'hnld', 'lnd', 'pad16', 'pad8'):
        served = layout in ('nld', 'packed3', 'padrow')
        dQ, dK, dV = (place((g.N, L, H, dh), layout, torch.float32, 'out0') for _ in range(3))
        amax = torch.zeros(2, device=dev)
        fd = family(DST_S if nb else DST, F32, shape, [q.view, k.view, v.view, go.view, dQ.view])
        fs = family(SRC_S if nb else SRC, F32, shape, [q.view, k.view, v.view, go.view, dK.view, dV.view])
        rd = lib.ampconv_bwd_edge_dst(q.view, k.view, v.view, go.view, rp, cl, g.N, L, D, H, dQ.view,
                                      *hub(csr, 'dst', L, D, 1, keep), *sp, amax[0:].data_ptr(), _lib.AMPCONV_F32, stream())
        if nb and rd != 0 and fs >= 0:
            # the refused destination pass left no statistics: fill them through a layout it takes
            tmp = place((g.N, L, H, dh), 'nld', torch.float32, 'out0')
            _lib.check(lib.ampconv_bwd_edge_dst(q.view, k.view, v.view, go.view, rp, cl, g.N, L, D, H, tmp.view, None, 0,
                                                None, *sp, None, _lib.AMPCONV_F32, stream()), 'dst for the statistics')
        rs = lib.ampconv_bwd_edge_src(q.view, k.view, v.view, go.view, cp, cr, ci, g.N, L, D, H, dK.view, dV.view,
                                      *hub(csr, 'src', L, D, 2, keep), sp[1], amax[1:].data_ptr(), _lib.AMPCONV_F32,
                                      stream()) if fs >= 0 else fs
        torch.cuda.synchronize()
        name = f'absmax L{L}dh{dh}H{H} {layout}'
        print(f'{name}: dst {FAMILY_NAME.get(fd, fd)} rc {rd}, src {FAMILY_NAME.get(fs, fs)} rc {rs}')
        if fd >= 0 and (served or fd == MFMA):
            assert rd == 0, name
            got = read(dQ.backing, dQ.index)
            assert dQ.outside_intact() and dQ.unwritten() == 0 and np.isfinite(got).all(), name
            assert float(amax[0]) == np.abs(got).max(), f'{name}: dQ absmax {float(amax[0])} vs {np.abs(got).max()}'
        else:
            assert rd == BADARG, name
            assert dQ.outside_intact() and dQ.unwritten() == dQ.index.numel(), f'{name}: refused, but dQ was written'
            assert float(amax[0]) == 0.0
        if fs >= 0 and served:
            assert rs == 0, name
            gk, gv = read(dK.backing, dK.index), read(dV.backing, dV.index)
            assert all(p.outside_intact() and p.unwritten() == 0 for p in (dK, dV)), name
            want = max(np.abs(gk).max(), np.abs(gv).max())
            assert float(amax[1]) == want, f'{name}: dK | dV absmax {float(amax[1])} vs {want}'
        else:
            assert rs == BADARG, name
            for p in (dK, dV):
                assert p.outside_intact() and p.unwritten() == p.index.numel(), f'{name}: refused, but dK / dV written'
            assert float(amax[1]) == 0.0
