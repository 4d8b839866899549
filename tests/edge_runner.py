"""What the GPU tests of the edge C ABI share (tests/test_gpu_edge_views.py, tests/test_gpu_edge_ladder.py): the family
table written from include/ampconv.h, the test graphs, operands and fp64 references, and the runner that places one
(storage, shape, layout, graph), makes the five calls through ctypes and checks what they wrote.

TEST INFRASTRUCTURE.  Tolerances (the project's own bars, SURVEY.md 8c, against fp64):
  fp32 storage   O, dQ (means over a row's edges) and dK, dV of sources with at most 12 out-edges: FLAT atol 1e-5,
                 rtol 1e-4; dK, dV of sources with more out-edges (sums over many edges): atol scaled by max |want|
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


def header_rule(dtype, shape, small=True):
    """The rule tuple of ANY (storage, shape), from the same wording of include/ampconv.h the table was written from
    (`small=False`: AMPCONV_SMALL=0 in the environment): what the token-count sweep holds ampconv_edge_family to at
    the shapes the table does not list.  tests/test_edge_reference_cpu.py holds it to the table."""
    L, dh, H = shape
    one_wave = L <= 20 and dh in (16, 32)
    per_unit = L <= 64 and dh <= 64 and dh % 2 == 0
    if dtype == BF16:
        return _BF_ONE_WAVE if one_wave else _BF_PER_UNIT if per_unit else None
    if small and L <= 4:
        # the smallest v with D / v <= 64 lanes and a head of dh / v = 4, 8, 16 or 32 lanes
        for v, rule in ((1, _SMALL_V1), (2, _SMALL_V2), (4, _SMALL_V4)):
            if dh % v == 0 and H * dh // v <= 64 and dh // v in (4, 8, 16, 32):
                return rule
    return _ONE_WAVE if one_wave else _PER_UNIT if per_unit else _GENERIC


def case_id(c):
    dt, (L, dh, H), lay = c[:3]
    return '-'.join([dt, f'L{L}dh{dh}H{H}', lay] + [str(x) for x in c[3:]])


TDT = {F32: torch.float32, BF16: torch.bfloat16}
CODE = {F32: _lib.AMPCONV_F32, BF16: _lib.AMPCONV_BF16}
TOL = {F32: dict(atol=1e-5, rtol=1e-4), BF16: dict(atol=2e-2, rtol=2e-2)}
FEW = 12          # dK, dV of a source with more out-edges than this are sums the absolute bar scales with
SCALED_CAP = 8.0  # ... and max |want| over those rows may not exceed this (compare_rows): the scaled bar stays near the flat one


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
        self._csr = {}

    def csr(self, chunk=64):
        """ampconv_graph_build, plans included, with the chunk that ships below a million edges (64) or, for any other
        value, with _lib.HUB_CHUNK set to it around the build (128: what ships from a million edges up)."""
        if chunk not in self._csr:
            from ampnet_amd import EdgeCSR
            ei = torch.from_numpy(np.stack([self.src, self.dst])).cuda()
            if chunk == 64:
                assert _lib.hub_chunk(self.E) == 64
                self._csr[chunk] = EdgeCSR(ei, self.N)
            else:
                with pytest.MonkeyPatch.context() as mp:
                    mp.setattr(_lib, 'HUB_CHUNK', chunk)
                    self._csr[chunk] = EdgeCSR(ei, self.N)
            assert self._csr[chunk].hub_chunk == chunk
        return self._csr[chunk]


def ladder_degrees(chunk):
    """The segment lengths of graph 'L': every length 0..20 (the batches of four edges and their tails, the prefetch
    distances); one below, at and one above 1, 2 and 3 chunks (an uncut row of exactly `chunk` edges, one-edge last
    chunks, full last chunks, rows of 2 and 3 chunks, whose later combine phases add nothing); 4, 8, 12 and 16 chunks
    and one edge (5, 9, 13, 17 chunks: the combine's paired loop once and twice, without and with its single
    remainder); three isolated nodes."""
    c = chunk
    return np.array(list(range(21)) + [k * c + d for k in (1, 2, 3) for d in (-1, 0, 1)] +
                    [k * c + 1 for k in (4, 8, 12, 16)] + [0, 0, 0])


LADDER_CHUNKS = 63          # chunks of the ladder's plan on either side, for any chunk length


@functools.lru_cache(maxsize=None)
def graph(name, chunk=64):
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
    if name == 'L':
        # the ladder for plans of `chunk` edges: node i has in-degree ladder_degrees(chunk)[i]; the out-degrees are the
        # same multiset on a seeded permutation of the nodes (the three isolated ones stay where they are); edges pair a
        # destination slot with a randomly drawn source slot, so multi-edges and self-loops stay in.  tests/
        # test_edge_reference_cpu.py holds the construction to its figures.
        indeg = ladder_degrees(chunk)
        n = len(indeg)
        rng = np.random.default_rng(14)
        outdeg = indeg.copy()
        outdeg[:n - 3] = indeg[:n - 3][rng.permutation(n - 3)]
        dst = np.repeat(np.arange(n), indeg)
        src = rng.permutation(np.repeat(np.arange(n), outdeg))
        g = Graph('L', src, dst, n, n)
        assert np.array_equal(g.indeg, indeg) and np.array_equal(g.outdeg, outdeg)
        return g
    raise ValueError(name)


def chunks_per_row(deg, chunk):
    """Chunks of every row a plan of `chunk` edges cuts (rows LONGER than a chunk), in row order."""
    deg = np.asarray(deg)
    return -(-deg[deg > chunk] // chunk)


# ---------------------------------------------------------------------------------------- operands and references
def make_operands(dtype, shape, N, scale=1.0):
    """Q, K, V, dObar [N, L, H, dh], independent N(0, 1) (float64; bf16 storage: rounded to bf16 first)."""
    L, dh, H = shape
    rng = np.random.default_rng(1000 * L + 10 * dh + H)
    ops = [rng.standard_normal((N, L, H, dh)).astype(np.float32) * np.float32(scale) for _ in range(4)]
    if dtype == BF16:
        ops = [torch.from_numpy(t).bfloat16().float().numpy() for t in ops]
    return tuple(t.astype(np.float64) for t in ops)


def make_reference(dtype, shape, gname, chunk=64, scale=1.0):
    """O, dQ, dK, dV of the whole graph (the passes' row counts select from them)."""
    g = graph(gname, chunk)
    Q, K, V, dO = operands(dtype, shape, g.N, scale)
    return (er.fwd(Q, K, V, g.rowptr, g.col),) + er.bwd(Q, K, V, dO, g.rowptr, g.col)


# cached: the shapes of TABLE on the fixed graphs (the sweeps over many shapes call make_* and keep nothing)
operands = functools.lru_cache(maxsize=None)(make_operands)
reference = functools.lru_cache(maxsize=None)(make_reference)


# ------------------------------------------------------------------------------------------------------ the calls
def family(call, dtype, shape, views):
    L, dh, H = shape
    arr = (_lib.View * len(views))(*views)
    return _lib.load().ampconv_edge_family(CALLS[call][0], CODE[dtype], L, dh * H, H, CALLS[call][1], arr, len(views))


def expected_family(call, dtype, shape, views, rule=None):
    rule = TABLE[dtype, shape] if rule is None else rule
    return rule[alignment_bytes(views, 2 if dtype == BF16 else 4)][call]


def hub(csr, side, L, D, tiles, keep):
    plan, n, ws = csr.hub_args(side, L, D, tiles)
    keep.append(ws)
    return plan, n, (ws.data_ptr() if ws is not None else None)


def nan_buffer(floats, device='cuda:0'):
    """A statistics buffer as the passes may find it: uninitialised memory, here NaN throughout."""
    return torch.full((floats,), float('nan'), device=device)


class Run:
    """One (storage, shape, layout, graph): the placed operands and what each call returned.  chunk: of the graph's
    plans; ops: the operands (default: the cached N(0, 1) ones of the shape, times `scale`); rule: the family rule to
    expect (default: the table's)."""

    def __init__(self, dtype, shape, layout, gname, chunk=64, ops=None, rule=None, scale=1.0):
        self.dtype, self.shape, self.layout, self.g, self.chunk = dtype, shape, layout, graph(gname, chunk), chunk
        L, dh, H = shape
        self.rule = TABLE[dtype, shape] if rule is None else rule
        self.ops = operands(dtype, shape, self.g.N, scale) if ops is None else ops
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
        self.want[call] = expected_family(call, self.dtype, self.shape, views, self.rule)
        return self.fam[call]

    def stats_buffer(self):
        """Sized by ampconv_softmax_stats_bytes; where that is 0 the passes must REFUSE a buffer -- the one handed over
        to see that is still as large as any family could want (40 or 32 ceil(L / 16) floats per (edge, head)), so that
        a pass that wrongly took it would stay inside it.  It arrives full of NaN, as the inputs' margins do: the slots
        of tokens >= L are never written, and nothing read from them may reach a result."""
        L, dh, H = self.shape
        nb = _lib.load().ampconv_softmax_stats_bytes(self.g.E, L, dh * H, H, CODE[self.dtype])
        return nan_buffer(max(nb // 4, self.g.E * H * max(40, 32 * ((L + 15) // 16))))

    def forward(self):
        lib, g, (L, dh, H) = _lib.load(), self.g, self.shape
        csr, O = g.csr(self.chunk), self.output('out0')
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
        D, csr, code, tag = dh * H, g.csr(self.chunk), CODE[self.dtype], '/stats' if with_stats else ''
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


def compare(r, label, want, outdeg=None):
    """One output tensor of a run against the fp64 model at the module's bars."""
    got, tol = r.out[label], TOL[r.dtype]
    name = f'{case_id((r.dtype, r.shape, r.layout, r.g.name))} {label} [{FAMILY_NAME[r.fam[LABEL_CALL[label]]]}]'
    assert np.isfinite(got).all(), f'{name}: non-finite values (NaN from a gap or a margin?)'
    if outdeg is None or (outdeg <= FEW).all():
        assert_close_scaled(got, want, name, scaled=False, **tol)
        return
    few = outdeg <= FEW
    assert_close_scaled(got[few], want[few], name + ' (<= 12 out-edges)', scaled=False, **tol)
    # a hub source's rows are sums over ~160 edges of O(1) terms: the absolute bar scales with their magnitude
    assert_close_scaled(got[~few], want[~few], name + ' (hub source)', scaled=True, **tol)


def compare_rows(got, want, name, tol, deg, by_source):
    """The bars of `compare` with a verdict per ROW: got, want [n, L, H, dh] and the n rows' segment lengths `deg` --
    in-degrees for O and dQ (by_source False: means over a row, flat), out-degrees for dK and dV (by_source True: flat
    up to 12 out-edges, above that assert_close_scaled(scaled=True) over those rows together, whose max |want| may not
    exceed SCALED_CAP, so that the scaled bar cannot grow unnoticed).  A failure lists the segment length of every row
    out of tolerance."""
    assert np.isfinite(got).all(), (f'{name}: non-finite values in the rows of '
                                    f'{"out" if by_source else "in"}-degree {_degrees(deg, ~np.isfinite(got))}')
    few = deg <= FEW if by_source else np.ones(len(deg), bool)
    groups = [(few, False, ' (<= 12 out-edges)' if by_source else '')]
    if not few.all():
        top = float(np.abs(want[~few]).max())
        assert top <= SCALED_CAP, f'{name}: max |want| {top:.2f} over the scaled rows exceeds {SCALED_CAP}: lower the operand scale'
        groups.append((~few, True, ' (> 12 out-edges)'))
    failed = []
    for rows, scaled, suffix in groups:
        if not rows.any():
            continue
        try:
            assert_close_scaled(got[rows], want[rows], name + suffix, scaled=scaled, **tol)
        except AssertionError as e:
            scale = max(1.0, float(np.abs(want[rows]).max())) if scaled else 1.0
            bad = np.abs(got[rows] - want[rows]) > tol['atol'] * scale + tol['rtol'] * np.abs(want[rows])
            failed.append(f'{str(e).splitlines()[0]}; {"out" if by_source else "in"}-degrees of the rows out of tolerance: '
                          f'{_degrees(deg[rows], bad)}')
    assert not failed, ' | '.join(failed)


def _degrees(deg, bad):
    return sorted(int(d) for d in deg[bad.reshape(len(deg), -1).any(axis=1)])


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
    few = np.ones(n, bool) if outdeg is None else outdeg[:n] <= FEW
    assert_close_scaled(got[few], want[:n][few], f'{name} {label}', scaled=False, **TOL[F32])
    if not few.all():     # the hub source's sums over ~160 edges: the absolute bar scales with their magnitude
        assert_close_scaled(got[~few], want[:n][~few], f'{name} {label} (hub source)', scaled=True, **TOL[F32])


def finish_rows(label, p, n, deg, want, name, by_source):
    """_finish with compare_rows' verdict per row (deg: the in- or out-degrees the output's rows follow)."""
    assert p.outside_intact(slice(0, n)), f'{name} {label}: bytes outside the output view (or behind row {n}) were written'
    assert p.unwritten(slice(0, n)) == 0, f'{name} {label}: elements of the view were not written'
    got = read(p.backing, p.index)[:n]
    assert not got[deg[:n] == 0].any(), f'{name} {label}: rows without edges are not exact zeros'
    compare_rows(got, want[:n], f'{name} {label}', TOL[F32], deg[:n], by_source)


# ------------------------------------------------------------- the plane and the scaled entry points (fp32 outputs)
def plane_operands(ops, indeg, dev):
    """(the four operands in the plane format, bounds) for ampconv_*_edge_planes from Q, K, V, dObar float64."""
    Q, K, V, dO = ops
    gbar = dO / np.maximum(indeg, 1)[:, None, None, None]         # the plane passes carry no per-edge weight
    mq, mg = max(np.abs(t).max() for t in (Q, K, V)), np.abs(gbar).max()
    bounds = torch.tensor([2 * mq, 2 * mg, np.abs(V).max(), mg], dtype=torch.float32, device=dev)
    return [to_planes(t, 2 * mq) for t in (Q, K, V)] + [to_planes(gbar, 2 * mg)], bounds


def planes_calls(csr, n, shape, inp, lout, with_stats, bounds, stats, spos, keep, name, n_all=None):
    """The plane entry points over the first n rows: forward (without statistics only), destination and source pass
    with the graph's plans, from placed plane operands `inp` into fresh `lout` outputs.  n_all: the graph's node count
    where n is less (the outputs then have n_all nodes, and with statistics a destination pass over all rows goes
    first: the source pass reads the statistics of EVERY in-edge of its sources).
    {'O' (without statistics), 'dQ', 'dK', 'dV'} -> the placed output, after a synchronize."""
    lib, (L, dh, H) = _lib.load(), shape
    D = dh * H
    q, k, v, go = inp
    rp, cl, cp, cr = (t.data_ptr() for t in (csr.rowptr, csr.col, csr.cscptr, csr.crow))
    sp = (spos.data_ptr(), stats.data_ptr()) if with_stats else (None, None)
    n_all = n if n_all is None else n_all
    out = {r: place((n_all, L, H, dh), lout, torch.float32, 'out0')
           for r in (('dQ', 'dK', 'dV') if with_stats else ('O', 'dQ', 'dK', 'dV'))}
    if with_stats and n < n_all:
        scratch = place((n_all, L, H, dh), lout, torch.float32, 'out0')
        _lib.check(lib.ampconv_bwd_edge_dst_planes(q.view, k.view, v.view, go.view, rp, cl, n_all, L, D, H, scratch.view,
                                                   None, 0, None, bounds.data_ptr(), *sp, None, stream()), name)
    if not with_stats:
        _lib.check(lib.ampconv_fwd_edge_planes(q.view, k.view, v.view, rp, cl, n, L, D, H, out['O'].view,
                                               *hub(csr, 'dst', L, D, 1, keep), bounds.data_ptr(), stream()), name)
    _lib.check(lib.ampconv_bwd_edge_dst_planes(q.view, k.view, v.view, go.view, rp, cl, n, L, D, H, out['dQ'].view,
                                               *hub(csr, 'dst', L, D, 1, keep), bounds.data_ptr(), *sp, None,
                                               stream()), name)
    _lib.check(lib.ampconv_bwd_edge_src_planes(q.view, k.view, v.view, go.view, cp, cr, n, L, D, H, out['dK'].view,
                                               out['dV'].view, *hub(csr, 'src', L, D, 2, keep), bounds.data_ptr(), sp[1],
                                               None, stream()), name)
    torch.cuda.synchronize()
    return out


def scaled_bounds(ops, dev):
    mq, mg = max(np.abs(t).max() for t in ops[:3]), np.abs(ops[3]).max()
    return torch.tensor([mq, mg, np.abs(ops[2]).max(), mg], dtype=torch.float32, device=dev)


def scaled_calls(csr, n, shape, inp, out, bounds, stats, spos, keep, src_plan=True, n_all=None):
    """ampconv_*_edge_scaled over the first n rows (forward, destination pass with statistics, source pass) from the
    placed fp32 operands `inp` into the placed outputs `out` = (O, dQ, dK, dV); src_plan False: the source pass
    without its plan; n_all: the graph's node count where n is less (a destination pass over all rows then fills the
    statistics first, as in planes_calls).  The three return codes, after a synchronize."""
    lib, (L, dh, H) = _lib.load(), shape
    D = dh * H
    q, k, v, go = inp
    O, dQ, dK, dV = out
    rp, cl, cp, cr, ci = (t.data_ptr() for t in (csr.rowptr, csr.col, csr.cscptr, csr.crow, csr.cinv))
    if n_all is not None and n < n_all:
        scratch = place((n_all, L, H, dh), 'nld', torch.float32, 'out0')
        _lib.check(lib.ampconv_bwd_edge_dst_scaled(q.view, k.view, v.view, go.view, rp, cl, n_all, L, D, H, scratch.view,
                                                   None, 0, None, bounds.data_ptr(), spos.data_ptr(), stats.data_ptr(),
                                                   None, stream()), 'dst, all rows')
    rcs = [lib.ampconv_fwd_edge_scaled(q.view, k.view, v.view, rp, cl, n, L, D, H, O.view,
                                       *hub(csr, 'dst', L, D, 1, keep), bounds.data_ptr(), stream()),
           lib.ampconv_bwd_edge_dst_scaled(q.view, k.view, v.view, go.view, rp, cl, n, L, D, H, dQ.view,
                                           *hub(csr, 'dst', L, D, 1, keep), bounds.data_ptr(), spos.data_ptr(),
                                           stats.data_ptr(), None, stream()),
           lib.ampconv_bwd_edge_src_scaled(q.view, k.view, v.view, go.view, cp, cr, ci, n, L, D, H, dK.view,
                                           dV.view, *(hub(csr, 'src', L, D, 2, keep) if src_plan else (None, 0, None)),
                                           bounds.data_ptr(), stats.data_ptr(), None, stream())]
    torch.cuda.synchronize()
    return rcs
