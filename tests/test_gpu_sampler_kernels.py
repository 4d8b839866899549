"""The GraphSAINT sampler's C calls, ONE AT A TIME through ctypes: ampconv_saint_random_walk, _nodes, _count_edges,
_count_edges_bounded, _fill_edges, _add_counts, _norms (csrc/sampler.hip), each against its numpy model of
tests/pipeline_reference.py on the inputs that module builds (tests/test_pipeline_reference_cpu.py shows that those inputs
tell the models from their mutants and holds the walk stream to its chi-square bar: nothing here is statistical).

Every buffer lies inside a larger allocation (edge_layouts.place_flat / place_flat_int): integer inputs between margins
of -1, float inputs between NaN margins, outputs in an allocation full of the sentinel; after every call nothing
outside the output may have changed and everything inside it that the call owns must have been written.  Bars: every
integer output equal element for element -- the walks are THE stream, the edges of a sub-graph stand at their exact
positions (grouped by source in ascending order, CSC order within a source: nothing is sorted before comparing) --,
the counts exact, the norms' branch constants bit-exact, edge_norm within 1 ulp and node_norm within 2 ulp of the
float32 model."""
import numpy as np
import pytest
import torch

import pipeline_reference as pr
from edge_layouts import INT_POISON, place_flat, place_flat_int
from edge_runner import stream

from ampnet_amd import _lib

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
BADARG, EWORKSPACE = -1, -3


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
    if got.shape == want.shape and np.array_equal(got, want):
        return []
    where = np.nonzero(np.asarray(got != want).reshape(-1))[0][:6].tolist() if got.shape == want.shape else 'shape'
    return [f'{name}: differs from the model at flat positions {where}']


def workspace(lib, *sizes):
    return torch.empty(max(lib.ampconv_saint_workspace_bytes(max(int(m), 1)) for m in sizes) + 256, dtype=torch.uint8, device='cuda:0')


# ----------------------------------------------------------------------------------------------------------- random_walk
@pytest.fixture(scope='module')
def walk_csc(lib):
    """The walk graph's CSC as the library builds it (EdgeCSR), held to numpy's stable sort, placed between -1 margins."""
    from ampnet_amd import EdgeCSR
    e = pr.walk_graph()
    csr = EdgeCSR(torch.from_numpy(e).cuda(), pr.WALK_N)
    cscptr, crow, cperm = pr.csc_of(e, pr.WALK_N)
    assert np.array_equal(csr.cscptr.cpu().numpy(), cscptr) and np.array_equal(csr.crow.cpu().numpy(), crow)
    assert np.array_equal(csr.cperm.cpu().numpy(), cperm)
    return cscptr, crow, place_flat_int(csr.cscptr.cpu().numpy(), I32), place_flat_int(csr.crow.cpu().numpy(), I32)


@pytest.mark.parametrize('B,wl,seed', pr.walk_cases())
def test_random_walk_is_the_stream(B, wl, seed, lib, walk_csc):
    """B below, at and above the 128-thread workgroup; walk_length 0 (the starts alone), 1 and 50; starts on the sink, an
    isolated node, the node whose only edge is its self-loop and node N - 1."""
    cscptr, crow, pptr, prow = walk_csc
    start = pr.walk_starts(B)
    ps, pw = place_flat_int(start, I64), place_flat_int((B, wl + 1), I64)
    rc = lib.ampconv_saint_random_walk(pptr.ptr, prow.ptr, ps.ptr, B, wl, seed, pw.ptr, stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    failed = written(pw, 'walks') + differs(vals(pw), pr.random_walk(cscptr, crow, start, wl, seed), 'walks')
    assert not failed, failed


# ----------------------------------------------------------------------------------------- nodes, count, fill: a sub-graph
@pytest.mark.parametrize('N,kind', pr.saint_cases(), ids=lambda v: str(v).replace(' ', '_'))
def test_subgraph_calls_match_the_model(N, kind, lib):
    """saint_nodes (mark, relabel, node_idx with the sentinel behind n_sub, n_sub), count_edges and count_edges_bounded
    at every n_bound (equal to each other and to the model, entries from n_sub on 0), fill_edges at exact positions."""
    e = pr.saint_graph(N)
    cscptr, crow, cperm = pr.csc_of(e, N)
    nodes = pr.saint_node_input(N, kind)
    mark, relabel, node_idx, n_sub = pr.saint_nodes(nodes, N)
    cnt, off, e_sub = pr.count_edges(node_idx, n_sub, cscptr, crow, mark)
    bounds = pr.n_bounds(n_sub, N)
    ws = workspace(lib, N, *bounds)
    pptr, prow, pperm = (place_flat_int(a, I32) for a in (cscptr, crow, cperm))
    pn = place_flat_int(nodes if len(nodes) else np.zeros(1, np.int64), I64)
    pm, pl, pi, ps = place_flat_int((N,), I32), place_flat_int((N,), I32), place_flat_int((N,), I64), place_flat_int((1,), I32)
    s = stream()
    rc = lib.ampconv_saint_nodes(pn.ptr, len(nodes), N, pm.ptr, pl.ptr, pi.ptr, ps.ptr, ws.data_ptr(), ws.numel(), s)
    torch.cuda.synchronize()
    assert rc == 0, rc
    got = slice(0, n_sub)
    failed = written(pm, 'mark') + written(pl, 'relabel') + written(ps, 'n_sub') + written(pi, 'node_idx', got)
    failed += differs(vals(pm), mark, 'mark') + differs(vals(pl), relabel, 'relabel')
    failed += differs(vals(ps), np.array([n_sub], np.int32), 'n_sub') + differs(vals(pi)[:n_sub], node_idx, 'node_idx')
    assert not failed, failed            # the calls below read what this one wrote

    pc, po, pe = place_flat_int((n_sub + 1,), I32), place_flat_int((n_sub + 1,), I32), place_flat_int((1,), I32)
    rc = lib.ampconv_saint_count_edges(pi.ptr, n_sub, pptr.ptr, prow.ptr, pm.ptr, pc.ptr, po.ptr, pe.ptr, ws.data_ptr(), ws.numel(), s)
    torch.cuda.synchronize()
    assert rc == 0, rc
    failed += written(pe, 'e_sub') + differs(vals(pe), np.array([e_sub], np.int32), 'e_sub')
    if n_sub == 0:                       # nothing to count: e_sub = 0 is all the call writes
        failed += [] if untouched(pc, po) else ['count_edges with n_sub = 0 wrote cnt or off']
    else:
        failed += written(pc, 'cnt') + written(po, 'off') + differs(vals(pc), cnt, 'cnt') + differs(vals(po), off, 'off')
    off_dev = None
    for nb in bounds:
        name = f'bounded n_bound={nb}'
        bc, bo, be = place_flat_int((nb + 1,), I32), place_flat_int((nb + 1,), I32), place_flat_int((1,), I32)
        rc = lib.ampconv_saint_count_edges_bounded(pi.ptr, nb, ps.ptr, pptr.ptr, prow.ptr, pm.ptr, bc.ptr, bo.ptr, be.ptr,
                                                   ws.data_ptr(), ws.numel(), s)
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        c2, o2, e2 = pr.count_edges(node_idx, n_sub, cscptr, crow, mark, nb)
        failed += written(bc, name + ' cnt') + written(bo, name + ' off') + written(be, name + ' e_sub')
        failed += differs(vals(bc), c2, name + ' cnt') + differs(vals(bo), o2, name + ' off')
        failed += differs(vals(be), np.array([e2], np.int32), name + ' e_sub')
        if n_sub:
            failed += differs(vals(bc)[:n_sub + 1], vals(pc), name + ' cnt against count_edges')
            failed += differs(vals(bo)[:n_sub + 1], vals(po), name + ' off against count_edges')
        if nb == n_sub:
            off_dev = bo
    assert not failed, failed            # fill_edges writes where `off` says

    ei, eid = pr.fill_edges(node_idx, n_sub, cscptr, crow, cperm, mark, relabel)
    assert ei.shape == (2, e_sub)
    pei, pid = place_flat_int((2, e_sub), I64), place_flat_int((e_sub,), I64)
    rc = lib.ampconv_saint_fill_edges(pi.ptr, n_sub, pptr.ptr, prow.ptr, pperm.ptr, pm.ptr, pl.ptr, off_dev.ptr, e_sub, pei.ptr,
                                      pid.ptr, s)
    torch.cuda.synchronize()
    assert rc == 0, rc
    failed += written(pei, 'edge_index') + written(pid, 'edge_id')
    failed += differs(vals(pei), ei, 'edge_index') + differs(vals(pid), eid, 'edge_id')          # positions are exact
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------ add_counts
def test_add_counts_is_exact(lib):
    """One index 5000 times among 3000 others, onto counts that are not zero; n = 0 touches nothing."""
    rng = np.random.default_rng(6)
    M = 100
    idx = rng.permutation(np.concatenate([np.full(5000, 37), rng.integers(0, M, 3000)])).astype(np.int64)
    count = rng.integers(0, 10, M).astype(np.float32)
    pi, pc = place_flat_int(idx, I64), place_flat(count, F32)
    assert lib.ampconv_saint_add_counts(pi.ptr, 0, pc.ptr, stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(vals(pc), count)
    assert lib.ampconv_saint_add_counts(pi.ptr, len(idx), pc.ptr, stream()) == 0
    torch.cuda.synchronize()
    want = pr.add_counts(idx, count)
    assert want[37] >= 5000 and np.array_equal(vals(pc), want) and pc.margins_hold(float('nan'))


# ----------------------------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize('shape', ['N > E', 'E > N', 'E = 0'])
def test_norms_branches(shape, lib):
    """Counts built to reach 0 / 0 -> 0.1, x / 0 -> 1e4, the clamp just above 1e4 and the plain quotient just below it, and
    node counts of 0 -> 0.1; more nodes than edges, more edges than nodes, no edge at all (NULL edge pointers)."""
    nc, ec, src, ns = pr.norm_inputs(shape)
    N, E = len(nc), len(ec)
    nn, en = pr.norms(nc, ec, src, N, ns)
    pnc, pn, pe = place_flat(nc, F32), place_flat((N,), F32), place_flat((max(E, 1),), F32)
    pec, psrc = (place_flat(ec, F32), place_flat_int(src, I64)) if E else (None, None)
    rc = lib.ampconv_saint_norms(pnc.ptr, pec.ptr if E else None, psrc.ptr if E else None, N, E, float(ns), pn.ptr,
                                 pe.ptr if E else None, stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    failed = written(pn, 'node_norm') + (written(pe, 'edge_norm') if E else [] if untouched(pe) else ['edge_norm written at E = 0'])
    gn, ge = vals(pn), vals(pe)[:E]
    un = pr.ulp_distance(gn, nn).max()
    ue = pr.ulp_distance(ge, en).max(initial=0)
    print(f'[bar] norms {shape}: node_norm {un:.0f} of 2 ulp, edge_norm {ue:.0f} of 1 ulp, '
          f'bit-equal: {bool(np.array_equal(gn.view(np.int32), nn.view(np.int32)) and np.array_equal(ge.view(np.int32), en.view(np.int32)))}')
    if un > 2 or ue > 1:
        failed.append(f'node_norm {un} ulp (bar 2), edge_norm {ue} ulp (bar 1)')
    if E:
        with np.errstate(divide='ignore', invalid='ignore'):
            q = nc[src].astype(np.float64) / ec
        branch = (ec == 0) | (q > 1e4)                       # 0.1, 1e4 and the clamp: constants, bit-exact
        assert branch.sum() >= 7 and set(en[branch].tolist()) == {np.float32(0.1), np.float32(1e4)}
        if not np.array_equal(ge[branch].view(np.int32), en[branch].view(np.int32)):
            failed.append('a branch constant (0.1, 1e4) is not bit-exact')
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------------- refusals
def test_sampler_refusals(lib):
    """Read from the entry points: a NULL pointer, a negative size, N past INT32_MAX, a short workspace -- a status code
    before anything is launched, the outputs as they were; the empty calls (B, n, n_sub or E_sub of 0) succeed and write
    nothing."""
    N = 40
    e = pr.saint_graph(N)
    cscptr, crow, cperm = (place_flat_int(a, I32) for a in pr.csc_of(e, N))
    mark_h, relabel_h, node_idx_h, n_sub = pr.saint_nodes(np.arange(0, N, 3), N)
    off_h = pr.count_edges(node_idx_h, n_sub, *pr.csc_of(e, N)[:2], mark_h)[1]
    mark, relabel, off, nsd = (place_flat_int(a, I32) for a in (mark_h, relabel_h, off_h, np.array([n_sub])))
    node_idx, nodes = place_flat_int(node_idx_h, I64), place_flat_int(np.arange(0, N, 3), I64)
    fcount = place_flat(np.ones(N, np.float32), F32)
    o32 = [place_flat_int((N + 1,), I32) for _ in range(4)]
    o64 = [place_flat_int((2 * N,), I64) for _ in range(2)]
    of = [place_flat((N,), F32) for _ in range(2)]
    ws = workspace(lib, N)
    s, w, wn = stream(), ws.data_ptr(), ws.numel()
    failed = []

    def check(label, rc, want=BADARG):
        torch.cuda.synchronize()
        clean = untouched(*o32, *o64, *of) and fcount.margins_hold(float('nan')) and mark.margins_hold(INT_POISON)
        if rc != want or not clean:
            failed.append(f'{label}: returned {rc} (expected {want}) or wrote')

    def with_null(args, k):
        return [None if i == k else a for i, a in enumerate(args)]

    # random_walk(cscptr, crow, start, B, wl, seed, walks)
    for k in (0, 2, 3):
        a = with_null([cscptr.ptr, crow.ptr, nodes.ptr, o64[0].ptr], k)
        check(f'random_walk NULL #{k}', lib.ampconv_saint_random_walk(a[0], a[1], a[2], 4, 3, 1, a[3], s))
    check('random_walk B < 0', lib.ampconv_saint_random_walk(cscptr.ptr, crow.ptr, nodes.ptr, -1, 3, 1, o64[0].ptr, s))
    check('random_walk walk_length < 0', lib.ampconv_saint_random_walk(cscptr.ptr, crow.ptr, nodes.ptr, 4, -1, 1, o64[0].ptr, s))
    check('random_walk B = 0', lib.ampconv_saint_random_walk(cscptr.ptr, crow.ptr, nodes.ptr, 0, 3, 1, o64[0].ptr, s), 0)
    # saint_nodes(nodes, n, N, mark, relabel, node_idx, n_sub, ws, bytes)
    base = [nodes.ptr, o32[0].ptr, o32[1].ptr, o64[0].ptr, o32[2].ptr, w]
    for k in range(6):
        a = with_null(base, k)
        check(f'saint_nodes NULL #{k}', lib.ampconv_saint_nodes(a[0], 5, N, a[1], a[2], a[3], a[4], a[5], wn, s))
    for n, big in ((-1, N), (5, 0), (5, -4), (5, 2 ** 31)):
        check(f'saint_nodes n={n} N={big}', lib.ampconv_saint_nodes(*base[:1], n, big, *base[1:], wn, s))
    need = lib.ampconv_saint_workspace_bytes(N)
    check('saint_nodes short workspace', lib.ampconv_saint_nodes(*base[:1], 5, N, *base[1:], need - 1, s), EWORKSPACE)
    # count_edges(node_idx, n_sub, cscptr, crow, mark, cnt, off, e_sub, ws, bytes)
    base = [node_idx.ptr, cscptr.ptr, crow.ptr, mark.ptr, o32[0].ptr, o32[1].ptr, o32[2].ptr, w]
    for k in (0, 1, 3, 4, 5, 6, 7):
        a = with_null(base, k)
        check(f'count_edges NULL #{k}', lib.ampconv_saint_count_edges(a[0], n_sub, *a[1:8], wn, s))
    check('count_edges n_sub < 0', lib.ampconv_saint_count_edges(base[0], -1, *base[1:], wn, s))
    need = lib.ampconv_saint_workspace_bytes(n_sub) - 256              # = the scan's bytes for n_sub + 1 entries
    if need > 0:
        check('count_edges short workspace', lib.ampconv_saint_count_edges(base[0], n_sub, *base[1:], need - 1, s), EWORKSPACE)
    # count_edges_bounded(node_idx, n_bound, n_sub_dev, cscptr, crow, mark, cnt, off, e_sub, ws, bytes)
    base = [node_idx.ptr, nsd.ptr, cscptr.ptr, mark.ptr, o32[0].ptr, o32[1].ptr, o32[2].ptr, w]
    for k in range(8):
        a = with_null(base, k)
        check(f'count_edges_bounded NULL #{k}',
              lib.ampconv_saint_count_edges_bounded(a[0], n_sub, a[1], a[2], crow.ptr, *a[3:8], wn, s))
    check('count_edges_bounded n_bound < 0',
          lib.ampconv_saint_count_edges_bounded(base[0], -1, base[1], base[2], crow.ptr, *base[3:], wn, s))
    if need > 0:
        check('count_edges_bounded short workspace',
              lib.ampconv_saint_count_edges_bounded(base[0], n_sub, base[1], base[2], crow.ptr, *base[3:], need - 1, s), EWORKSPACE)
    # fill_edges(node_idx, n_sub, cscptr, crow, cperm, mark, relabel, off, E_sub, edge_index, edge_id)
    base = [node_idx.ptr, cscptr.ptr, crow.ptr, cperm.ptr, mark.ptr, relabel.ptr, off.ptr, o64[0].ptr, o64[1].ptr]
    for k in range(9):
        a = with_null(base, k)
        check(f'fill_edges NULL #{k}', lib.ampconv_saint_fill_edges(a[0], n_sub, *a[1:7], 3, a[7], a[8], s))
    check('fill_edges n_sub < 0', lib.ampconv_saint_fill_edges(base[0], -1, *base[1:7], 3, *base[7:], s))
    check('fill_edges E_sub < 0', lib.ampconv_saint_fill_edges(base[0], n_sub, *base[1:7], -1, *base[7:], s))
    check('fill_edges E_sub = 0', lib.ampconv_saint_fill_edges(base[0], n_sub, *base[1:7], 0, *base[7:], s), 0)
    check('fill_edges n_sub = 0', lib.ampconv_saint_fill_edges(base[0], 0, *base[1:7], 3, *base[7:], s), 0)
    # add_counts(idx, n, count)
    check('add_counts n < 0', lib.ampconv_saint_add_counts(nodes.ptr, -1, fcount.ptr, s))
    check('add_counts NULL idx', lib.ampconv_saint_add_counts(None, 3, fcount.ptr, s))
    check('add_counts NULL count', lib.ampconv_saint_add_counts(nodes.ptr, 3, None, s))
    # norms(node_count, edge_count, edge_src, N, E, num_samples, node_norm, edge_norm)
    base = [fcount.ptr, fcount.ptr, nodes.ptr, of[0].ptr, of[1].ptr]
    for k in range(5):
        a = with_null(base, k)
        check(f'norms NULL #{k}', lib.ampconv_saint_norms(a[0], a[1], a[2], N, 5, 3.0, a[3], a[4], s))
    for n, m in ((0, 5), (-1, 5), (N, -1)):
        check(f'norms N={n} E={m}', lib.ampconv_saint_norms(*base[:3], n, m, 3.0, *base[3:], s))
    assert not failed, failed
