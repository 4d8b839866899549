"""The one-query-token edge family (include/ampconv.h, "edge phase, ONE query token"; csrc/edge_token.hip) through the C
ABI, one call at a time, against the fp64 model of tests/edge_reference.py fed ONE query row (tests/
test_token_query_cpu.py pins that this is the full model's token t).

Operands sit inside NaN margins, outputs are sentinel-filled (tests/edge_layouts.py).  The query tensors Q and dObar are
placed as whole [N, L, H, dh] tensors that hold NaN at every token but t, and the call selects token t by offsetting the
view's pointer: a kernel that touched another query row would return NaN.  Bars: edge_runner.TOL through
edge_runner.compare_rows -- no number of this file's own."""
import functools

import numpy as np
import pytest
import torch

import edge_reference as er
import edge_runner as R
from edge_layouts import Placed, _INT, _sentinel, place, read
from edge_runner import BF16, F32

from ampnet_amd import _lib

pytestmark = pytest.mark.gpu

F32_SHAPES = [(2, 3, 1), (5, 6, 3), (17, 16, 3), (20, 32, 4), (20, 32, 8), (40, 50, 2), (64, 64, 1)]
BF16_SHAPES = [(17, 16, 3), (20, 32, 8), (40, 50, 2), (64, 64, 1)]
CASES = [(F32, s) for s in F32_SHAPES] + [(BF16, s) for s in BF16_SHAPES]
GRAPHS = [('B', 64), ('A', 64), ('L', 64), ('L', 128)]


def _id(c):
    return f'{c[0]}-L{c[1][0]}dh{c[1][1]}H{c[1][2]}'


def place_off(logical, dtype, role=None, device='cuda:0'):
    """edge_layouts.place for the layout 'off': rows padded by one fp32 element (two bf16 elements) and the base that
    much behind a 256-byte boundary -- every base and stride is 4-byte aligned and no better."""
    is_output = isinstance(logical, tuple)
    N, L, H, dh = logical if is_output else logical.shape
    e = 2 if dtype == torch.bfloat16 else 1
    D = H * dh
    ns, rs, hs, off = L * (D + e), D + e, dh, e
    span = (N - 1) * ns + (L - 1) * rs + (H - 1) * hs + dh
    margin = -(-(ns + L * D) // 64) * 64
    n, l, h, c = np.ix_(np.arange(N) * ns, np.arange(L) * rs, np.arange(H) * hs, np.arange(dh))
    index = torch.from_numpy(margin + off + n + l + h + c).to(device)
    total = margin + off + span + margin
    if is_output:
        backing = torch.full((total,), _sentinel(dtype), dtype=_INT[dtype], device=device).view(dtype)
    else:
        backing = torch.full((total,), float('nan'), dtype=dtype, device=device)
        backing[index.reshape(-1)] = torch.from_numpy(np.ascontiguousarray(logical)).to(dtype).to(device).reshape(-1)
    view = _lib.View(backing.data_ptr() + (margin + off) * backing.element_size(), ns, rs, hs)
    return Placed(backing, view, index)


def put(logical, layout, dtype, role):
    return place_off(logical, dtype) if layout == 'off' else place(logical, layout, dtype, role)


def token_view(p, t):
    """The one-token view of a placed [N, L, H, dh] tensor: its pointer moved to token t."""
    v = p.view
    return _lib.View(v.ptr + t * v.row_stride * p.backing.element_size(), v.node_stride, v.row_stride, v.head_stride)


def only_token(x, t):
    """x [N, L, H, dh] with NaN at every token but t."""
    out = np.full_like(x, np.nan)
    out[:, t] = x[:, t]
    return out


@functools.lru_cache(maxsize=None)
def token_reference(dtype, shape, gname, chunk, t):
    """O, dQ [N, 1, H, dh] and dK, dV [N, L, H, dh] of the whole graph for query token t (fp64)."""
    g = R.graph(gname, chunk)
    Q, K, V, dO = R.operands(dtype, shape, g.N)
    sl = slice(t, t + 1)
    return (er.fwd(Q[:, sl], K, V, g.rowptr, g.col),) + er.bwd(Q[:, sl], K, V, dO[:, sl], g.rowptr, g.col)


class TokenRun:
    """One (storage, shape, layout, graph, token): the placed operands and the three calls."""

    def __init__(self, dtype, shape, layout, gname, chunk, t):
        self.dtype, self.shape, self.layout, self.t = dtype, shape, layout, t
        self.g, self.chunk = R.graph(gname, chunk), chunk
        self.csr = self.g.csr(chunk)
        self.td, self.code = R.TDT[dtype], R.CODE[dtype]
        Q, K, V, dO = R.operands(dtype, shape, self.g.N)
        self.q = put(only_token(Q, t), layout, self.td, 'Q')
        self.go = put(only_token(dO, t), layout, self.td, 'dO')
        self.k, self.v = put(K, layout, self.td, 'K'), put(V, layout, self.td, 'V')
        self.keep = []

    def out(self, L, role='out0'):
        _, dh, H = self.shape
        return put((self.g.N, L, H, dh), self.layout, self.td, role)

    def hub(self, side, L, tiles):
        return R.hub(self.csr, side, L, self.shape[1] * self.shape[2], tiles, self.keep)

    def forward(self, n=None):
        L, dh, H = self.shape
        csr, O = self.csr, self.out(1)
        rc = _lib.load().ampconv_fwd_edge_token(token_view(self.q, self.t), self.k.view, self.v.view,
                                                csr.rowptr.data_ptr(), csr.col.data_ptr(), self.g.n_rows if n is None else n,
                                                L, dh * H, H, O.view, *self.hub('dst', 1, 1), self.code, R.stream())
        return rc, O

    def dst(self):
        L, dh, H = self.shape
        csr, dQ = self.csr, self.out(1)
        rc = _lib.load().ampconv_bwd_edge_dst_token(token_view(self.q, self.t), self.k.view, self.v.view,
                                                    token_view(self.go, self.t), csr.rowptr.data_ptr(), csr.col.data_ptr(),
                                                    self.g.n_rows, L, dh * H, H, dQ.view, *self.hub('dst', 1, 1), self.code,
                                                    R.stream())
        return rc, dQ

    def src(self):
        L, dh, H = self.shape
        csr, dK, dV = self.csr, self.out(L, 'out0'), self.out(L, 'out1')
        rc = _lib.load().ampconv_bwd_edge_src_token(token_view(self.q, self.t), self.k.view, self.v.view,
                                                    token_view(self.go, self.t), csr.cscptr.data_ptr(), csr.crow.data_ptr(),
                                                    csr.cinv.data_ptr(), self.g.n_rows, L, dh * H, H, dK.view, dV.view,
                                                    *self.hub('src', L, 2), self.code, R.stream())
        return rc, dK, dV

    def check(self, label, p, want, deg, by_source):
        """Sentinel intact outside the first n_rows nodes, every element of them written, rows without edges exact
        zeros, values at the module's bars."""
        n = self.g.n_rows
        name = f'{R.case_id((self.dtype, self.shape, self.layout, self.g.name))}-c{self.chunk}-t{self.t} {label}'
        assert p.outside_intact(slice(0, n)), f'{name}: bytes outside the output view (or behind row {n}) were written'
        assert p.unwritten(slice(0, n)) == 0, f'{name}: elements of the view were not written'
        got = read(p.backing, p.index)[:n]
        assert not got[deg[:n] == 0].any(), f'{name}: rows without edges are not exact zeros'
        R.compare_rows(got, want[:n], name, R.TOL[self.dtype], deg[:n], by_source)

    def run_and_check(self):
        g = self.g
        O, dQ, dK, dV = token_reference(self.dtype, self.shape, g.name, self.chunk, self.t)
        rc, p = self.forward()
        assert rc == 0, rc
        rc2, pq = self.dst()
        assert rc2 == 0, rc2
        rc3, pk, pv = self.src()
        assert rc3 == 0, rc3
        torch.cuda.synchronize()
        self.check('O', p, O, g.indeg, False)
        self.check('dQ', pq, dQ, g.indeg, False)
        self.check('dK', pk, dK, g.outdeg, True)
        self.check('dV', pv, dV, g.outdeg, True)
        return p, pq, pk, pv


def test_supported_answers_for_every_listed_shape():
    lib = _lib.load()
    for dtype, (L, dh, H) in CASES + [(F32, (1, 32, 2))]:
        assert lib.ampconv_token_supported(L, dh * H, H, R.CODE[dtype]) == 1, (dtype, L, dh, H)
    assert lib.ampconv_token_supported(20, 130, 4, _lib.AMPCONV_F32) == 0          # D % H != 0
    assert lib.ampconv_token_supported(20, 128, 4, 7) == 0                         # no such dtype


@pytest.mark.parametrize('gname,chunk', GRAPHS, ids=[f'{g}{c}' for g, c in GRAPHS])
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_three_calls(case, gname, chunk):
    dtype, shape = case
    g = R.graph(gname, chunk)
    if gname == 'L':        # the plan path really runs: both sides are cut
        csr = g.csr(chunk)
        assert csr.hub_dst_chunks == csr.hub_src_chunks == R.LADDER_CHUNKS
    elif gname == 'A':
        csr = g.csr(chunk)
        assert csr.hub_dst_chunks > 0 and csr.hub_src_chunks > 0
    else:
        assert g.n_rows == 33 < g.N and g.csr(chunk).hub_dst is None
    for t in (0, shape[0] - 1):
        TokenRun(dtype, shape, 'nld', gname, chunk, t).run_and_check()


def test_single_token_sequence_on_graph_b():
    """L = 1: the softmax is the constant 1 (its gradient to q and K is exactly 0).  Graph B only: on the ladder the
    fp64 model's dV of a hub source exceeds edge_runner.SCALED_CAP at this shape."""
    p, pq, pk, pv = TokenRun(F32, (1, 32, 2), 'nld', 'B', 64, 0).run_and_check()
    assert not read(pq.backing, pq.index)[:33].any()


@pytest.mark.parametrize('layout', ['off', 'packed3'])
@pytest.mark.parametrize('case', [(F32, (40, 50, 2)), (F32, (20, 32, 4)), (F32, (5, 6, 3)), (BF16, (40, 50, 2)),
                                  (BF16, (20, 32, 8))], ids=_id)
def test_view_alignment(case, layout):
    """'off': every view 4-byte (fp32) / 2-element (bf16) aligned and no better -- the narrow load pieces; 'packed3': the
    column thirds of a packed [N * L, 3D] projection buffer, what the layer passes."""
    dtype, shape = case
    r = TokenRun(dtype, shape, layout, 'A', 64, shape[0] - 1)
    esize = 2 if dtype == BF16 else 4
    if layout == 'off':
        assert all(v.ptr % 8 == 4 and (v.row_stride * esize) % 8 == 4 for v in (r.k.view, r.v.view))
    r.run_and_check()


@pytest.mark.parametrize('case', [(F32, (40, 50, 2)), (BF16, (20, 32, 8))], ids=_id)
def test_two_runs_are_bitwise_equal(case):
    dtype, shape = case
    a = TokenRun(dtype, shape, 'nld', 'L', 64, 0)
    first = a.run_and_check()
    second = [a.forward()[1], a.dst()[1], *a.src()[1:]]
    torch.cuda.synchronize()
    for x, y in zip(first, second):
        assert torch.equal(x.bits(), y.bits())


def test_empty_graph_reads_no_edge():
    """E = 0: zeros everywhere, and nothing dereferences col / crow (passed as NULL here)."""
    import types
    L, dh, H, N = 5, 6, 3, 9
    zeros = torch.zeros(N + 1, dtype=torch.int32, device='cuda:0')
    csr = types.SimpleNamespace(rowptr=zeros, cscptr=zeros, cinv=torch.ones(1, device='cuda:0'))
    Q, K, V, dO = R.make_operands(F32, (L, dh, H), N)
    q, go = place(only_token(Q, 1), 'nld', torch.float32, 'Q'), place(only_token(dO, 1), 'nld', torch.float32, 'dO')
    k, v = place(K, 'nld', torch.float32, 'K'), place(V, 'nld', torch.float32, 'V')
    O, dQ = place((N, 1, H, dh), 'nld', torch.float32, 'out0'), place((N, 1, H, dh), 'nld', torch.float32, 'out0')
    dK, dV = place((N, L, H, dh), 'nld', torch.float32, 'out0'), place((N, L, H, dh), 'nld', torch.float32, 'out1')
    lib, D = _lib.load(), dh * H
    qv, gv = token_view(q, 1), token_view(go, 1)
    assert lib.ampconv_fwd_edge_token(qv, k.view, v.view, csr.rowptr.data_ptr(), None, N, L, D, H, O.view, None, 0, None,
                                      _lib.AMPCONV_F32, R.stream()) == 0
    assert lib.ampconv_bwd_edge_dst_token(qv, k.view, v.view, gv, csr.rowptr.data_ptr(), None, N, L, D, H, dQ.view, None, 0,
                                          None, _lib.AMPCONV_F32, R.stream()) == 0
    assert lib.ampconv_bwd_edge_src_token(qv, k.view, v.view, gv, csr.cscptr.data_ptr(), None, csr.cinv.data_ptr(), N, L, D,
                                          H, dK.view, dV.view, None, 0, None, _lib.AMPCONV_F32, R.stream()) == 0
    torch.cuda.synchronize()
    for p in (O, dQ, dK, dV):
        assert p.outside_intact() and p.unwritten() == 0 and not read(p.backing, p.index).any()


def test_refusals_leave_the_outputs_untouched():
    r = TokenRun(F32, (5, 6, 3), 'nld', 'B', 64, 0)
    lib, csr, g = _lib.load(), r.csr, r.g
    L, dh, H = r.shape
    D = dh * H
    null = _lib.View(None, D, D, dh)
    qv, gv = token_view(r.q, 0), token_view(r.go, 0)
    rp, cl, cp, cr, ci = (t.data_ptr() for t in (csr.rowptr, csr.col, csr.cscptr, csr.crow, csr.cinv))
    ws = torch.empty(1024, device='cuda:0')
    # (what is wrong, L, D, H, dtype, Q view, hub workspace)
    bad = [('null view', L, D, H, r.code, null, None), ('D % H != 0', L, D + 1, H, r.code, qv, None),
           ('L > 64', 65, D, H, r.code, qv, None), ('dh > 64', L, 3 * 65, 3, r.code, qv, None),
           ('dtype', L, D, H, 7, qv, None), ('bf16, odd dh', L, 15, 3, _lib.AMPCONV_BF16, qv, None),
           ('workspace without a plan', L, D, H, r.code, qv, ws.data_ptr())]
    for what, Lx, Dx, Hx, code, q, w in bad:
        O, dQ, dK, dV = r.out(1), r.out(1), r.out(L, 'out0'), r.out(L, 'out1')
        rcs = [lib.ampconv_fwd_edge_token(q, r.k.view, r.v.view, rp, cl, g.n_rows, Lx, Dx, Hx, O.view, None, 0, w, code,
                                          R.stream()),
               lib.ampconv_bwd_edge_dst_token(q, r.k.view, r.v.view, gv, rp, cl, g.n_rows, Lx, Dx, Hx, dQ.view, None, 0, w,
                                              code, R.stream()),
               lib.ampconv_bwd_edge_src_token(q, r.k.view, r.v.view, gv, cp, cr, ci, g.n_rows, Lx, Dx, Hx, dK.view, dV.view,
                                              None, 0, w, code, R.stream())]
        torch.cuda.synchronize()
        assert all(rc in (R.BADARG, R.EDTYPE) for rc in rcs), (what, rcs)
        for p in (O, dQ, dK, dV):
            assert p.unwritten() == p.index.numel() and p.outside_intact(), what
    assert lib.ampconv_token_supported(65, D, H, r.code) == 0 and lib.ampconv_token_supported(L, 3 * 65, 3, r.code) == 0
