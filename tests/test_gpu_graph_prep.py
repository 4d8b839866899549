"""Graph preparation, the long-segment plans and the node lists, ONE CALL AT A TIME through ctypes: ampconv_graph_build,
ampconv_csr_build, ampconv_csc_positions, ampconv_csc_positions_from, ampconv_active_nodes (csrc/graph_prep.hip) and
ampconv_hub_plan (csrc/hub.hip), each against its numpy model of tests/graph_reference.py on the inputs that module builds
(tests/test_graph_reference_cpu.py shows that those inputs tell the models from their mutants and that every plan fits
its capacity: the inputs are known to be legal before they get here).

Every buffer lies inside a larger allocation (edge_layouts.place_flat_int / place_flat): edge_index and every other
integer input between margins of -1, every output, both plans, the status words, by_edge and the workspace in an
allocation full of the sentinel; after every call nothing outside an output may have changed and everything inside it
that the call owns must have been written.  Bars: every array equal element for element, cinv BIT-equal to float32
1 / float32 degree; a plan's descriptors as a set, everything else about it exact (graph_reference.check_plan).  One
synchronize per group of calls whose inputs are known to be good: what a call reads as positions or pointers has been
compared with the model before the call is made.  Cases with an odd index run on a side stream."""
import numpy as np
import pytest
import torch

import graph_reference as gr
from edge_layouts import INT_POISON, SENTINEL, place, place_flat, place_flat_int
from edge_runner import CODE, F32 as F32_, graph, operands, stream

from ampnet_amd import _lib

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
BADARG, EWORKSPACE = -1, -3
SENT = SENTINEL[I32]
INT_ARRAYS = ('rowptr', 'col', 'eperm', 'cscptr', 'crow', 'cperm')


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def vals(p):
    return p.backing[p.index.reshape(-1)].reshape(p.index.shape).cpu().numpy()


def written(p, name, rows=None):
    bad = []
    if not p.outside_intact(rows):
        bad.append(f'{name}: bytes outside the output were written')
    if p.unwritten(rows):
        bad.append(f'{name}: {p.unwritten(rows)} elements of the output were not written')
    return bad


def untouched(*placed):
    return all(p.outside_intact() and p.unwritten() == p.index.numel() for p in placed)


def differs(got, want, name):
    want = np.asarray(want)
    if got.dtype == np.float32:                          # bit for bit
        got, want = got.view(np.int32), want.astype(np.float32).view(np.int32)
    if got.shape == want.shape and np.array_equal(got, want):
        return []
    where = np.nonzero(np.asarray(got != want).reshape(-1))[0][:6].tolist() if got.shape == want.shape else 'shape'
    return [f'{name}: differs from the model at flat positions {where}']


class Streams:
    """The stream of a case: torch's current one, or (side) a fresh stream.  `raw`, read for every group of calls, makes
    the side stream wait for what torch's stream was given so far: the fills of the buffers placed for those calls."""

    def __init__(self, side):
        self.side = torch.cuda.Stream() if side else None

    @property
    def raw(self):
        if self.side is None:
            return stream()
        self.side.wait_stream(torch.cuda.current_stream())
        return self.side.cuda_stream


@pytest.fixture(scope='module')
def model():
    cache = {}

    def get(name):
        if name not in cache:
            c = gr.build_case(name)
            cache[name] = gr.graph_build(c.ei, c.N, c.chunk)
        return cache[name]
    return get


class Build:
    """The placed arguments of one ampconv_graph_build / ampconv_csr_build call.  plan_chunk: what the plan buffers are
    sized for (default: chunk); slots: elements of the per-edge outputs (default: E)."""

    def __init__(self, lib, ei, N, chunk, plan_chunk=None, slots=None, ws_skew=0):
        self.lib, self.N, self.chunk = lib, N, chunk
        self.ei = np.array(ei, dtype=np.int64).reshape(2, -1)          # (a writable copy: the cases are read-only)
        self.E = E = self.ei.shape[1]
        n = E if slots is None else slots
        self.pchunk = chunk if plan_chunk is None else plan_chunk
        self.pei = place_flat_int(self.ei, I64)
        self.out = {k: place_flat_int((N + 1 if k.endswith('ptr') else n,), I32) for k in INT_ARRAYS}
        self.out['cinv'] = place_flat((n,), F32)
        self.by_edge = place_flat_int((n,), I32)
        self.status = place_flat_int((4,), I32)
        self.plans = [place_flat_int((gr.plan_words_total(E, self.pchunk),), I32) for _ in range(2)]
        self.ws_bytes = lib.ampconv_csr_workspace_bytes(max(N, 1), E)
        assert self.ws_bytes % 4 == 0
        self.ws = place_flat_int((self.ws_bytes // 4,), I32, skew=ws_skew)

    def everything(self):
        return list(self.out.values()) + [self.by_edge, self.status, self.ws] + self.plans

    def graph_build(self, s, cinv=True, by_edge=True, plans=True, **over):
        a = dict(ei=self.pei.ptr, E=self.E, N=self.N, status=self.status.ptr, ws=self.ws.ptr, ws_bytes=self.ws_bytes,
                 **{k: p.ptr for k, p in self.out.items()})
        a.update(over)
        return self.lib.ampconv_graph_build(a['ei'], a['E'], a['N'], a['rowptr'], a['col'], a['eperm'], a['cscptr'], a['crow'],
                                            a['cperm'], a['cinv'] if cinv else None, a['status'], self.chunk,
                                            self.plans[0].ptr if plans else None, self.plans[1].ptr if plans else None,
                                            self.by_edge.ptr if by_edge else None, a['ws'], a['ws_bytes'], s)

    def csr_build(self, s, **over):
        a = dict(ei=self.pei.ptr, E=self.E, N=self.N, status=self.status.ptr, ws=self.ws.ptr, ws_bytes=self.ws_bytes,
                 **{k: p.ptr for k, p in self.out.items()})
        a.update(over)
        return self.lib.ampconv_csr_build(a['ei'], a['E'], a['N'], a['rowptr'], a['col'], a['eperm'], a['cscptr'], a['crow'],
                                          a['cperm'], a['cinv'], a['status'], a['ws'], a['ws_bytes'], s)

    def check_arrays(self, m, cinv=True):
        failed = [] if self.pei.margins_hold(INT_POISON) else ['edge_index: its margins were written']
        failed += [] if self.ws.outside_intact() else ['workspace: bytes around it were written']
        for k, p in self.out.items():
            if k == 'cinv' and not cinv:
                failed += [] if untouched(p) else ['cinv: written although NULL was passed']
                continue
            failed += written(p, k) + differs(vals(p), getattr(m, k), k)
        return failed

    def check_plans(self, m, built=True):
        """built: both plans against check_plan (sentinel everywhere else in their allocations), else untouched."""
        failed = []
        for p, ptr, side in zip(self.plans, (m.rowptr, m.cscptr), ('dst', 'src')):
            if not built:
                failed += [] if untouched(p) else [f'plan_{side}: written although no plan was asked for']
                continue
            try:
                gr.check_plan(p.backing.cpu().numpy(), ptr, self.N, self.E, self.chunk, SENT, origin=int(p.index[0]))
            except AssertionError as e:
                failed.append(f'plan_{side}: {e}')
        return failed

    def check_graph_build(self, m, cinv=True, by_edge=True, plans=True):
        failed = self.check_arrays(m, cinv)
        status = m.status if plans else np.array([m.flag, 0, 0, 0], np.int32)
        failed += written(self.status, 'status') + differs(vals(self.status), status, 'status')
        if by_edge:
            failed += written(self.by_edge, 'by_edge') + differs(vals(self.by_edge), m.by_edge, 'by_edge')
        else:
            failed += [] if untouched(self.by_edge) else ['by_edge: written although NULL was passed']
        return failed + self.check_plans(m, plans)


def whole_storage(t):
    """Every int32 word of the storage behind an int32 view."""
    st = t.untyped_storage()
    return torch.empty(0, dtype=I32, device=t.device).set_(st, 0, (st.nbytes() // 4,), (1,)).cpu().numpy()


def check_positions(lib, bd, m, st):
    """ampconv_csc_positions and ampconv_csc_positions_from on the arrays a build left on the device (compared with
    the model before this is called)."""
    E = bd.E
    scratch, sa, sb = (place_flat_int((E,), I32) for _ in range(3))
    s = st.raw
    rc = [lib.ampconv_csc_positions(bd.out['eperm'].ptr, bd.out['cperm'].ptr, E, scratch.ptr, sa.ptr, s),
          lib.ampconv_csc_positions_from(bd.out['eperm'].ptr, bd.by_edge.ptr, E, sb.ptr, s)]
    torch.cuda.synchronize()
    assert rc == [0, 0], rc
    want = gr.spos(m.eperm, m.cperm)
    failed = written(scratch, 'scratch') + written(sa, 'spos') + written(sb, 'spos from by_edge')
    failed += differs(vals(sa), want, 'spos') + differs(vals(sb), vals(sa), 'spos from by_edge against spos')
    failed += differs(vals(scratch), m.by_edge, 'scratch (CSC position of every edge id)')
    failed += differs(m.cperm[vals(sa)], m.eperm, 'cperm[spos[p]] == eperm[p]')
    return failed


# ------------------------------------------------------------------------------------------- a. both paths, the model
@pytest.mark.parametrize('name', gr.BUILD_CASES)
def test_graph_build_matches_the_model(name, lib, model):
    """The seven arrays, by_edge, status = {flag, dst chunks, src chunks, 0} and both plans of either path; then (c)
    both position calls on what the build left."""
    c, m = gr.build_case(name), model(name)
    bd = Build(lib, c.ei, c.N, c.chunk)
    st = Streams(gr.BUILD_CASES.index(name) % 2)
    rc = bd.graph_build(st.raw)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert m.flag == 0
    failed = bd.check_graph_build(m)
    assert not failed, failed
    print(f'[plans] {name}: {m.status[1]} + {m.status[2]} chunks of {gr.max_chunks(bd.E, c.chunk)} slots')
    failed = check_positions(lib, bd, m, st)
    assert not failed, failed


@pytest.mark.parametrize('N', [1, 257])
def test_no_edges(N, lib):
    """E = 0 through both entry points: the pointers all zero, the flag word(s) zeroed, nothing else touched."""
    ei = np.zeros((2, 0), np.int64)
    zeros = np.zeros(N + 1, np.int32)
    for call in ('graph_build', 'csr_build'):
        bd = Build(lib, ei, N, 64, slots=4)
        st = Streams(N > 1)
        rc = getattr(bd, call)(st.raw)
        torch.cuda.synchronize()
        assert rc == 0, (call, rc)
        failed = []
        for k in ('rowptr', 'cscptr'):
            failed += written(bd.out[k], k) + differs(vals(bd.out[k]), zeros, k)
        words = slice(0, 4 if call == 'graph_build' else 1)
        failed += written(bd.status, 'status', words) + differs(vals(bd.status)[words], np.zeros(4, np.int32)[words], 'status')
        rest = [bd.out[k] for k in ('col', 'eperm', 'crow', 'cperm', 'cinv')] + [bd.by_edge, bd.ws] + bd.plans
        failed += [] if untouched(*rest) else [f'{call}: E = 0 wrote more than the pointers and the flag']
        assert not failed, (call, failed)


OPTIONAL = ('no-cinv', 'no-by_edge', 'no-plans', 'chunk-0')


@pytest.mark.parametrize('variant', OPTIONAL)
@pytest.mark.parametrize('name', ['s-N64-E1023', 'm-N16385-E1000-hub'])
def test_optional_outputs(name, variant, lib, model):
    """cinv = NULL, by_edge = NULL, the plans NULL with chunk > 0, chunk = 0 with the plans given: everything else as
    the model, what was not asked for untouched, status[1:3] == 0 without plans."""
    c, m = gr.build_case(name), model(name)
    assert m.status[1] > 0 and m.status[2] > 0
    bd = Build(lib, c.ei, c.N, 0 if variant == 'chunk-0' else c.chunk, plan_chunk=c.chunk)
    st = Streams(OPTIONAL.index(variant) % 2)
    want = dict(cinv=variant != 'no-cinv', by_edge=variant != 'no-by_edge', plans=variant not in ('no-plans', 'chunk-0'))
    rc = bd.graph_build(st.raw, cinv=want['cinv'], by_edge=want['by_edge'], plans=variant != 'no-plans')
    torch.cuda.synchronize()
    assert rc == 0, rc
    failed = bd.check_graph_build(m, **want)
    assert not failed, failed


@pytest.mark.parametrize('name', ['s-N64-E1023', 'm-N16385-E5', 'm-N500-E12289'])
def test_csr_build_directly(name, lib, model):
    """ampconv_csr_build (the multi-launch path at any size) with its workspace 4 bytes behind a 256-byte boundary and
    exactly ampconv_csr_workspace_bytes long: the model's arrays, nothing behind the workspace written.  One byte less:
    AMPCONV_E_WORKSPACE and nothing written at all."""
    c, m = gr.build_case(name), model(name)
    bd = Build(lib, c.ei, c.N, c.chunk, ws_skew=1)
    assert bd.ws.ptr % 256 == 4
    st = Streams(True)
    rc = bd.csr_build(st.raw)
    torch.cuda.synchronize()
    assert rc == 0, rc
    failed = bd.check_arrays(m)
    failed += written(bd.status, 'oob', slice(0, 1)) + differs(vals(bd.status)[:1], [0], 'oob')
    failed += [] if untouched(bd.by_edge, *bd.plans) else ['csr_build wrote by_edge or a plan']
    assert not failed, failed
    short = Build(lib, c.ei, c.N, c.chunk, ws_skew=1)
    rc = short.csr_build(st.raw, ws_bytes=short.ws_bytes - 1)
    torch.cuda.synchronize()
    assert rc == EWORKSPACE, rc
    assert untouched(*short.everything())
    if c.path == 'multi':                                               # (the one-launch path needs no workspace)
        rc = short.graph_build(st.raw, ws_bytes=short.ws_bytes - 1)
        torch.cuda.synchronize()
        assert rc == EWORKSPACE, rc
        assert untouched(*short.everything())


# -------------------------------------------------------------------------------------------------- b. ids out of range
@pytest.mark.parametrize('N,E,side,part', gr.OOB_CASES, ids=lambda v: str(v))
def test_ids_out_of_range_are_clamped(N, E, side, part, lib):
    """-1, N, N + 7, 2^31, 2^40, -2^40 and INT64_MIN on either side or both: status[0] != 0 and every array that of the
    CLAMPED graph (v < 0 -> 0, v >= N -> N - 1) -- a consistent graph, which EdgeCSR(validate=False) hands on."""
    ei, clean = gr.oob_case(N, E, side, part)
    for which, e in (('bad', ei), ('clean', clean)):
        m = gr.graph_build(e, N, 64)
        assert m.flag == (which == 'bad')
        bd = Build(lib, e, N, 64)
        st = Streams(gr.OOB_CASES.index((N, E, side, part)) % 2)
        rc = bd.graph_build(st.raw)
        torch.cuda.synchronize()
        assert rc == 0, rc
        flag = int(vals(bd.status)[0])
        assert (flag != 0) == (which == 'bad'), (which, flag)
        got = vals(bd.status)
        got[0] = got[0] != 0
        failed = bd.check_arrays(m) + differs(got, m.status, 'status') + written(bd.status, 'status')
        failed += written(bd.by_edge, 'by_edge') + differs(vals(bd.by_edge), m.by_edge, 'by_edge') + bd.check_plans(m)
        assert not failed, (which, failed)
        a = {k: vals(bd.out[k]) for k in INT_ARRAYS}
        assert a['col'].min() >= 0 and a['col'].max() < N and a['crow'].min() >= 0 and a['crow'].max() < N
        assert np.array_equal(np.sort(a['eperm']), np.arange(E)) and np.array_equal(np.sort(a['cperm']), np.arange(E))
        assert a['rowptr'][0] == a['cscptr'][0] == 0 and a['rowptr'][N] == a['cscptr'][N] == E
        assert (np.diff(a['rowptr']) >= 0).all() and (np.diff(a['cscptr']) >= 0).all()


# ----------------------------------------------------------------------------------------------- c. the position calls
def test_positions_edge_cases(lib):
    """E = 0: OK and nothing touched; a NULL argument: AMPCONV_E_BADARG and nothing touched; the identity graph."""
    from ampnet_amd import EdgeCSR
    perm = np.array([2, 0, 1, 3], np.int32)
    pe, pc, pb = (place_flat_int(perm, I32) for _ in range(3))
    scratch, spos = place_flat_int((4,), I32), place_flat_int((4,), I32)
    s = stream()
    assert lib.ampconv_csc_positions(pe.ptr, pc.ptr, 0, scratch.ptr, spos.ptr, s) == 0
    assert lib.ampconv_csc_positions_from(pe.ptr, pb.ptr, 0, spos.ptr, s) == 0
    for args in ((None, pc.ptr, 4, scratch.ptr, spos.ptr), (pe.ptr, None, 4, scratch.ptr, spos.ptr),
                 (pe.ptr, pc.ptr, 4, None, spos.ptr), (pe.ptr, pc.ptr, 4, scratch.ptr, None),
                 (pe.ptr, pc.ptr, -1, scratch.ptr, spos.ptr)):
        assert lib.ampconv_csc_positions(*args, s) == BADARG, args
    for args in ((None, pb.ptr, 4, spos.ptr), (pe.ptr, None, 4, spos.ptr), (pe.ptr, pb.ptr, 4, None), (pe.ptr, pb.ptr, -1, spos.ptr)):
        assert lib.ampconv_csc_positions_from(*args, s) == BADARG, args
    torch.cuda.synchronize()
    assert untouched(scratch, spos) and all(p.margins_hold(INT_POISON) for p in (pe, pc, pb))
    for n in (1, 300):
        assert torch.equal(EdgeCSR.identity(n, torch.device('cuda:0')).csc_positions().cpu(), torch.arange(n, dtype=torch.int32))


# ------------------------------------------------------------------------------------------- d. ampconv_hub_plan alone
@pytest.mark.parametrize('i', range(len(gr.plan_cases())), ids=[c[0] for c in gr.plan_cases()])
def test_hub_plan_alone(i, lib):
    """A plan over n_rows <= N rows names exactly the long rows among them; chunk 1, 64, 128; no long row: the header
    {0, chunk, 0, offset} and nothing else; 40 long rows claimed from many workgroups at once."""
    name, ptr, n_rows, E, chunk = gr.plan_cases()[i]
    pp = place_flat_int(ptr, I32)
    plan = place_flat_int((gr.plan_words_total(E, chunk),), I32)
    assert plan.index.numel() * 4 == lib.ampconv_hub_plan_bytes(E, chunk)
    st = Streams(i % 2)
    rc = lib.ampconv_hub_plan(pp.ptr, n_rows, E, chunk, plan.ptr, st.raw)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert pp.margins_hold(INT_POISON)
    lst = gr.check_plan(plan.backing.cpu().numpy(), ptr, n_rows, E, chunk, SENT, origin=int(plan.index[0]))
    _, n_long, n_chunks = gr.plan(ptr, n_rows, chunk)
    print(f'[plan] {name}: {n_long} long rows, {n_chunks} chunks; list in ascending slot order: {bool((np.diff(lst) > 0).all())}')
    if 'no-long-row' in name:
        assert n_chunks == 0 and plan.unwritten() == plan.index.numel() - 4


def test_plan_sizes_and_refusals(lib):
    for E, chunk in ((0, 64), (1, 64), (63, 64), (64, 64), (12285, 64), (12350, 64), (20000, 128), (3926, 1), (1 << 33, 128)):
        mc = 2 * (E // chunk) + 2
        assert lib.ampconv_hub_plan_bytes(E, chunk) == 16 + 16 * mc + 4 * (mc // 2 + 2) == 4 * gr.plan_words_total(E, chunk)
    assert lib.ampconv_hub_plan_bytes(100, 0) == 0 and lib.ampconv_hub_plan_bytes(100, -64) == 0
    assert lib.ampconv_hub_plan_bytes(-1, 64) == 0
    assert lib.ampconv_hub_workspace_bytes(63, 20, 64, 2) == 63 * 20 * 64 * 4 * 2
    assert lib.ampconv_hub_workspace_bytes(1 << 20, 64, 512, 2) == (1 << 20) * 64 * 512 * 4 * 2
    for args in ((0, 20, 64, 1), (-1, 20, 64, 1), (5, 0, 64, 1), (5, 20, -64, 1), (5, 20, 64, 0)):
        assert lib.ampconv_hub_workspace_bytes(*args) == 0, args
    ptr = place_flat_int(np.array([0, 70, 140], np.int32), I32)
    plan = place_flat_int((gr.plan_words_total(140, 64),), I32)
    s = stream()
    for args in ((None, 2, 140, 64, plan.ptr), (ptr.ptr, 2, 140, 64, None), (ptr.ptr, 0, 140, 64, plan.ptr),
                 (ptr.ptr, 2, -1, 64, plan.ptr), (ptr.ptr, 2, 140, 0, plan.ptr)):
        assert lib.ampconv_hub_plan(*args, s) == BADARG, args
    torch.cuda.synchronize()
    assert untouched(plan)


# ------------------------------------------------------------------------------- e. slot order does not reach the result
def test_slot_order_does_not_reach_the_result(lib):
    """The ladder graph at (L, dh, H) = (20, 32, 2), fp32: forward, destination and source pass once with the plans
    ampconv_graph_build made and once with plans ampconv_hub_plan made over the same pointers -- bit-equal outputs,
    whichever slots the long rows took in either."""
    g, shape = graph('L', 64), (20, 32, 2)
    L, dh, H = shape
    D, code, s = dh * H, CODE[F32_], stream()
    csr = g.csr(64)
    m = gr.graph_build(np.stack([g.src, g.dst]), g.N, 64)
    for k in INT_ARRAYS + ('cinv',):
        assert not differs(getattr(csr, k).cpu().numpy(), getattr(m, k), k)
    assert [csr.hub_dst_chunks, csr.hub_src_chunks] == m.status[1:3].tolist()
    mine = [place_flat_int((gr.plan_words_total(g.E, 64),), I32) for _ in range(2)]
    for p, ptr in zip(mine, (csr.rowptr, csr.cscptr)):
        assert lib.ampconv_hub_plan(ptr.data_ptr(), g.N, g.E, 64, p.ptr, s) == 0
    torch.cuda.synchronize()
    orders = []
    for p, theirs, ptr, n in zip(mine, (csr.hub_dst, csr.hub_src), (m.rowptr, m.cscptr), m.status[1:3].tolist()):
        a = gr.check_plan(p.backing.cpu().numpy(), ptr, g.N, g.E, 64, SENT, origin=int(p.index[0]))
        whole = whole_storage(theirs)
        b = gr.check_plan(whole, ptr, g.N, g.E, 64)
        da, db = vals(p)[4:4 + 4 * n], whole[4:4 + 4 * n]
        orders.append((bool(np.array_equal(da, db)), bool(np.array_equal(a, b))))
    print(f'[slot order] graph_build against hub_plan, (descriptor slots equal, list order equal) for dst, src: {orders}')

    inp = {r: place(t, 'nld', F32, r) for r, t in zip(('Q', 'K', 'V', 'dO'), operands(F32_, shape, g.N))}
    q, k, v, go = (inp[r].view for r in ('Q', 'K', 'V', 'dO'))
    keep = []

    def passes(pd, ps):
        nd, ns = csr.hub_dst_chunks, csr.hub_src_chunks
        out = {r: place((g.N, L, H, dh), 'nld', F32, 'out0') for r in ('O', 'dQ', 'dK', 'dV')}
        ws = [torch.empty(lib.ampconv_hub_workspace_bytes(n, L, D, t) // 4, device='cuda:0') for n, t in ((nd, 1), (nd, 1), (ns, 2))]
        keep.append(ws)
        rp, cl, cp, cr, ci = (t.data_ptr() for t in (csr.rowptr, csr.col, csr.cscptr, csr.crow, csr.cinv))
        rcs = [lib.ampconv_fwd_edge(q, k, v, rp, cl, None, g.N, L, D, H, out['O'].view, pd, nd, ws[0].data_ptr(), code, s),
               lib.ampconv_bwd_edge_dst(q, k, v, go, rp, cl, g.N, L, D, H, out['dQ'].view, pd, nd, ws[1].data_ptr(), None, None,
                                        None, code, s),
               lib.ampconv_bwd_edge_src(q, k, v, go, cp, cr, ci, g.N, L, D, H, out['dK'].view, out['dV'].view, ps, ns,
                                        ws[2].data_ptr(), None, None, code, s)]
        assert rcs == [0, 0, 0], rcs
        return out

    first = passes(csr.hub_dst.data_ptr(), csr.hub_src.data_ptr())
    second = passes(mine[0].ptr, mine[1].ptr)
    torch.cuda.synchronize()
    for r in first:
        assert first[r].outside_intact() and first[r].unwritten() == 0, r
        assert torch.equal(first[r].bits(), second[r].bits()), f'{r}: the two plans give different bits'
        assert bool(torch.isfinite(first[r].backing[first[r].index.reshape(-1)]).all()), r


# --------------------------------------------------------------------------------------- f. ampconv_active_nodes directly
@pytest.mark.parametrize('kind', gr.ACTIVE_KINDS)
@pytest.mark.parametrize('N', gr.ACTIVE_N)
def test_active_nodes_directly(N, kind, lib):
    """which = 1, 2, 3: the ascending ids, exactly 8 zeros behind them, the rest of the N + 8 words and everything around
    them untouched; ptr as the model, ptr[N] == count; nothing written around the workspace."""
    rowptr, cscptr = gr.active_case(N, kind)
    pr_, pc = place_flat_int(rowptr, I32), place_flat_int(cscptr, I32)
    nws = lib.ampconv_active_nodes_workspace_bytes(N)
    assert nws > 0 and nws % 4 == 0
    st = Streams((gr.ACTIVE_N.index(N) + gr.ACTIVE_KINDS.index(kind)) % 2)
    runs = []
    for which in (1, 2, 3):
        lst, ptr, cnt = place_flat_int((N + 8,), I32), place_flat_int((N + 1,), I32), place_flat_int((1,), I32)
        ws = place_flat_int((nws // 4,), I32, skew=which % 2)
        rc = lib.ampconv_active_nodes(pr_.ptr if which & 1 else None, pc.ptr if which & 2 else None, N, which, lst.ptr, ptr.ptr,
                                      cnt.ptr, ws.ptr, nws, st.raw)
        assert rc == 0, (which, rc)
        runs.append((which, lst, ptr, cnt, ws))
    torch.cuda.synchronize()
    failed = [] if pr_.margins_hold(INT_POISON) and pc.margins_hold(INT_POISON) else ['an input pointer array was written']
    for which, lst, ptr, cnt, ws in runs:
        want_list, want_ptr, count = gr.active(rowptr, cscptr, N, which)
        t = f'which={which} '
        failed += written(lst, t + 'list', slice(0, count + 8)) + differs(vals(lst)[:count + 8], want_list, t + 'list')
        failed += written(ptr, t + 'ptr') + differs(vals(ptr), want_ptr, t + 'ptr')
        failed += written(cnt, t + 'count') + differs(vals(cnt), [count], t + 'count')
        failed += differs(vals(ptr)[N:], [count], t + 'ptr[N]')
        failed += [] if ws.outside_intact() else [t + 'bytes around the workspace were written']
    assert not failed, failed


def test_active_nodes_refusals(lib):
    N = 257
    rowptr, cscptr = gr.active_case(N, 'sparse')
    pr_, pc = place_flat_int(rowptr, I32), place_flat_int(cscptr, I32)
    lst, ptr, cnt = place_flat_int((N + 8,), I32), place_flat_int((N + 1,), I32), place_flat_int((1,), I32)
    nws = lib.ampconv_active_nodes_workspace_bytes(N)
    ws = place_flat_int((nws // 4,), I32)
    s = stream()
    ok = dict(rowptr=pr_.ptr, cscptr=pc.ptr, N=N, which=3, list=lst.ptr, ptr=ptr.ptr, count=cnt.ptr, ws=ws.ptr, nws=nws)
    refused = [(dict(which=0), BADARG), (dict(which=4), BADARG), (dict(nws=nws - 1), EWORKSPACE), (dict(N=0), BADARG),
               (dict(which=1, rowptr=None), BADARG), (dict(which=2, cscptr=None), BADARG), (dict(rowptr=None), BADARG),
               (dict(cscptr=None), BADARG), (dict(list=None), BADARG), (dict(ptr=None), BADARG), (dict(count=None), BADARG),
               (dict(ws=None), BADARG)]
    for over, code in refused:
        a = dict(ok, **over)
        assert lib.ampconv_active_nodes(*a.values(), s) == code, over
    torch.cuda.synchronize()
    assert untouched(lst, ptr, cnt, ws)
    assert lib.ampconv_active_nodes_workspace_bytes(0) == 0 and lib.ampconv_active_nodes_workspace_bytes(-5) == 0
    # the pointer `which` does not need may be NULL
    assert lib.ampconv_active_nodes(pr_.ptr, None, N, 1, lst.ptr, ptr.ptr, cnt.ptr, ws.ptr, nws, s) == 0
    torch.cuda.synchronize()
    assert int(vals(cnt)[0]) == gr.active(rowptr, cscptr, N, 1)[2]


# ---------------------------------------------------------------------------- g. argument checks that launch nothing
@pytest.mark.parametrize('name', ['s-N64-E1023', 'm-N16385-E5'])
def test_refused_builds_write_nothing(name, lib):
    """status NULL, N = 0, E < 0, a NULL array (either path), a missing or short workspace (multi-launch): the error code
    and every output, the status words included, still the sentinel."""
    c = gr.build_case(name)
    bd = Build(lib, c.ei, c.N, c.chunk)
    s = stream()
    refused = [dict(status=None), dict(N=0), dict(N=-3), dict(E=-1), dict(ei=None)] + [{k: None} for k in INT_ARRAYS]
    for over in refused:
        assert bd.graph_build(s, **over) == BADARG, ('graph_build', over)
        assert bd.csr_build(s, **over) == BADARG, ('csr_build', over)
    assert bd.csr_build(s, ws=None) == BADARG
    assert bd.csr_build(s, ws_bytes=0) == EWORKSPACE
    if c.path == 'multi':
        assert bd.graph_build(s, ws=None) == BADARG
        assert bd.graph_build(s, ws_bytes=0) == EWORKSPACE
    torch.cuda.synchronize()
    assert untouched(*bd.everything()) and bd.pei.margins_hold(INT_POISON)


# ------------------------------------------------------------------------------------------------------- h. EdgeCSR
def test_edge_csr_over_the_models(lib):
    from ampnet_amd import EdgeCSR
    from ampnet_amd.graph import graph_cache
    dev = torch.device('cuda:0')
    # validate=False on ids out of range: the clamped graph, no exception
    ei, _ = gr.oob_case(1024, 3000, 'both', 0)
    with pytest.raises(ValueError, match='outside'):
        EdgeCSR(torch.from_numpy(ei.copy()).to(dev), 1024)
    csr = EdgeCSR(torch.from_numpy(ei.copy()).to(dev), 1024, validate=False)
    m = gr.graph_build(ei, 1024, 64)
    failed = [f for k in INT_ARRAYS + ('cinv',) for f in differs(getattr(csr, k).cpu().numpy(), getattr(m, k), k)]
    failed += differs(csr.csc_positions().cpu().numpy(), gr.spos(m.eperm, m.cperm), 'spos')
    assert not failed, failed
    # graph_cache: one build per tensor ...
    graph_cache.clear()
    c = gr.build_case('s-N64-E1023')
    t = torch.from_numpy(c.ei.copy()).to(dev)
    first = graph_cache.get(t, c.N)
    assert graph_cache.get(t, c.N) is first
    # hub_dst / hub_src are views of the header and the descriptors; the row list the combine pass reads lies behind them in
    # the same storage
    m = gr.graph_build(c.ei, c.N, 64)
    E = c.ei.shape[1]
    assert [first.hub_dst_chunks, first.hub_src_chunks] == m.status[1:3].tolist() and first.hub_dst_chunks > 0 < first.hub_src_chunks
    for plan, n, ptr in ((first.hub_dst, first.hub_dst_chunks, m.rowptr), (first.hub_src, first.hub_src_chunks, m.cscptr)):
        assert plan.numel() == 4 + 4 * n and plan.storage_offset() == 0
        nbytes = plan.untyped_storage().nbytes()
        assert nbytes == lib.ampconv_hub_plan_bytes(E, 64) >= 4 * (int(plan[3]) + int(plan[2])) > 4 * plan.numel()
        gr.check_plan(whole_storage(plan), ptr, c.N, E, 64)
    # ... and the same tensor written in place is another graph
    changed = c.ei.copy()
    changed[:, 5] = (changed[:, 5] + 1) % c.N
    t[:, 5] = torch.from_numpy(changed[:, 5]).to(dev)
    second = graph_cache.get(t, c.N)
    assert second is not first
    m2 = gr.graph_build(changed, c.N, 64)
    assert not m2.flag and not same_arrays(m2, gr.graph_build(c.ei, c.N, 64))
    failed = [f for k in INT_ARRAYS + ('cinv',) for f in differs(getattr(second, k).cpu().numpy(), getattr(m2, k), k)]
    assert not failed, failed
    graph_cache.clear()


def same_arrays(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in INT_ARRAYS)
