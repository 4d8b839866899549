"""The edge passes of the C ABI on a LADDER of segment lengths and at EVERY token count, one pass at a time, against the
per-pass fp64 model (tests/edge_reference.py), with the runner of tests/edge_runner.py in the canonical `nld` layout (NaN
margins around every input, a sentinel around and inside every output).

The graphs of the other tests have whatever degrees a random draw gives; the kernels' loops over a segment (batches of
four edges and a tail, a prefetch one or two edges ahead, the statistics of edge p + 1 requested during edge p), the
long-segment plan (rows LONGER than a chunk are cut) and the ordered combine (four chunk phases, two alternating
accumulators, a paired loop and a single remainder) each have lengths at which a bound or a mask goes wrong.  Graph 'L'
(edge_runner.ladder_degrees) holds every one of them on both sides, for the chunk of the small graphs (64) and for the one
that ships from a million edges up (128).  The token count L picks the kernel within a family (plain / batched tails /
full tile; ceil(L / 16) token tiles; the short-sequence border at 4 | 5): the sweep runs every L of every family on graph
B, and holds ampconv_edge_family to the header's rule for the shape, so that no sweep passes on another family's kernels.

Bars: the module's existing ones (edge_runner.TOL, compare_rows), no new number.  A failure names the segment lengths
(in-degrees for O and dQ, out-degrees for dK and dV) or the token counts that failed, all of them.
"""
import pytest
import torch

from edge_layouts import place
from edge_runner import (BF16, CALL_NAME, F32, FAMILY_NAME, LABEL_CALL, LADDER_CHUNKS, TABLE, Run, chunks_per_row,
                         compare_rows, finish_rows, graph, header_rule, make_operands, nan_buffer, operands,
                         plane_operands, planes_calls, reference, scaled_bounds, scaled_calls, stream, TOL, _BF_ONE_WAVE,
                         _BF_PER_UNIT, _GENERIC, _ONE_WAVE, _PER_UNIT, _SMALL_V1, _SMALL_V2, _SMALL_V4)

import edge_reference as er
from ampnet_amd import _lib

gpu = pytest.mark.gpu
CHUNKS = (64, 128)
SHORT = [(dh, H) for (dt, (L, dh, H)), _ in TABLE.items() if dt == F32 and L <= 4 and dh in (16, 32)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda:0')


def shape_id(s):
    return 'L%ddh%dH%d' % s


def verdict(r, want):
    """Everything a finished Run is held to, as a list of failures: nothing written outside the view, rows without edges
    exact zeros, every call on the family of the rule (and refused exactly where the rule refuses), every pass run, every
    output within the bars of the fp64 model `want` = (O, dQ, dK, dV) of the whole graph."""
    g, bad = r.g, list(r.problems)
    for call, f in sorted(r.fam.items()):
        if f != r.want[call]:
            bad.append(f'{CALL_NAME[call]}: family {FAMILY_NAME.get(f, f)}, the header says {FAMILY_NAME[r.want[call]]}')
        if call in r.rc and r.rc[call] != (f if f < 0 else 0):
            bad.append(f'{CALL_NAME[call]}: returned {r.rc[call]}, family query {f}')
    # every pass ran: fp32 always has a source pass without statistics, bf16 one with or without them
    if not ({'O', 'dQ'} <= set(r.out) and set(r.out) & {'dK', 'dK/stats'} and set(r.out) & {'dV', 'dV/stats'}):
        bad.append(f'not every pass ran: {sorted(r.out)}')
    want = dict(zip(('O', 'dQ', 'dK', 'dV'), want))
    for label, got in r.out.items():
        kind = label.split('/')[0]
        by_source = kind in ('dK', 'dV')
        name = f'{r.dtype} {shape_id(r.shape)} {g.name}{r.chunk} {label} [{FAMILY_NAME[r.fam[LABEL_CALL[label]]]}]'
        try:
            compare_rows(got, want[kind][:g.n_rows], name, TOL[r.dtype], (g.outdeg if by_source else g.indeg)[:g.n_rows],
                         by_source)
        except AssertionError as e:
            bad.append(str(e))
    return bad


def five_calls(dtype, shape, gname, chunk=64, **kw):
    r = Run(dtype, shape, 'nld', gname, chunk, **kw)
    r.forward()
    r.backward(False)
    r.backward(True)
    torch.cuda.synchronize()
    r.inp = r.keep = None
    return r


# ------------------------------------------------------------------------------------------------------ the ladder
@gpu
@pytest.mark.parametrize('chunk', CHUNKS)
@pytest.mark.parametrize('dtype,shape', list(TABLE), ids=lambda x: x if isinstance(x, str) else shape_id(x))
def test_every_pass_on_the_ladder_vs_fp64(dtype, shape, chunk, dev):
    """Forward, destination and source pass, without and with the statistics hand-off, of every shape of the family table
    on the ladder graph with plans of 64 and of 128 edges per chunk: 63 chunks on either side, rows of 2, 3, 4, 5, 9, 13
    and 17 chunks.  (N(0, 1) operands at every shape: the model's dK, dV of the sources above 12 out-edges stay below
    SCALED_CAP, which compare_rows asserts.)"""
    r = five_calls(dtype, shape, 'L', chunk)
    csr = r.g.csr(chunk)
    print('families:', ', '.join(f'{CALL_NAME[c]}={FAMILY_NAME.get(f, f)}' for c, f in sorted(r.fam.items())))
    assert csr.hub_chunk == chunk and csr.hub_dst_chunks == csr.hub_src_chunks == LADDER_CHUNKS, \
        (csr.hub_chunk, csr.hub_dst_chunks, csr.hub_src_chunks)
    bad = verdict(r, reference(dtype, shape, 'L', chunk))
    assert not bad, bad


@gpu
@pytest.mark.parametrize('chunk', CHUNKS)
@pytest.mark.parametrize('shape', [(20, 32, 2), (17, 16, 3), (13, 16, 2)], ids=shape_id)
def test_planes_entry_points_on_the_ladder(shape, chunk, dev):
    """ampconv_*_edge_planes on the ladder, operands and outputs under `nld`, without and with the statistics."""
    lib, g = _lib.load(), graph('L', chunk)
    L, dh, H = shape
    csr, keep = g.csr(chunk), []
    assert lib.ampconv_planes_supported(L, dh * H, H) == 1
    assert csr.hub_dst_chunks == csr.hub_src_chunks == LADDER_CHUNKS
    planes, bounds = plane_operands(operands(F32, shape, g.N), g.indeg, dev)
    want = reference(F32, shape, 'L', chunk)
    inp = [place(t, 'nld', torch.float32, r) for t, r in zip(planes, ('Q', 'K', 'V', 'dO'))]
    stats, bad = nan_buffer(g.E * H * 40), []
    for with_stats in (False, True):
        name = f'planes {shape_id(shape)} L{chunk}' + ('/stats' if with_stats else '')
        out = planes_calls(csr, g.N, shape, inp, 'nld', with_stats, bounds, stats, csr.csc_positions(), keep, name)
        bad += finish_all(out, g, g.N, want, name)
    assert not bad, bad


@gpu
@pytest.mark.parametrize('chunk', CHUNKS)
@pytest.mark.parametrize('shape', [(40, 50, 2), (33, 12, 2), (64, 64, 1)], ids=shape_id)
def test_scaled_entry_points_on_the_ladder(shape, chunk, dev):
    """ampconv_*_edge_scaled on the ladder under `nld`."""
    lib, g = _lib.load(), graph('L', chunk)
    L, dh, H = shape
    csr, keep = g.csr(chunk), []
    assert lib.ampconv_scaled_supported(L, dh * H, H) == 1
    assert csr.hub_dst_chunks == csr.hub_src_chunks == LADDER_CHUNKS
    ops = operands(F32, shape, g.N)
    name = f'scaled {shape_id(shape)} L{chunk}'
    out, rcs = scaled_run(g, csr, shape, ops, g.N, dev, keep)
    assert rcs == [0, 0, 0], rcs
    bad = finish_all(out, g, g.N, reference(F32, shape, 'L', chunk), name)
    assert not bad, bad


def scaled_run(g, csr, shape, ops, n, dev, keep):
    L, dh, H = shape
    # 32 ceil(L / 16) floats per (edge, head): what ampconv_softmax_stats_bytes says wherever the fp32 entry points
    # would take the workgroup-per-unit kernels; 0 where they take the short-sequence ones (L <= 4 at dh = 64, H = 1),
    # and the scaled entry points, which serve those shapes too, need the buffer all the same (include/ampconv.h)
    floats = g.E * H * 32 * ((L + 15) // 16)
    nb = _lib.load().ampconv_softmax_stats_bytes(g.E, L, dh * H, H, _lib.AMPCONV_F32)
    assert nb == (4 * floats if header_rule(F32, shape) is _PER_UNIT else 0), (shape, nb)
    stats = nan_buffer(floats)
    inp = [place(t, 'nld', torch.float32, r) for t, r in zip(ops, ('Q', 'K', 'V', 'dO'))]
    out = {r: place((g.N, L, H, dh), 'nld', torch.float32, 'out0') for r in ('O', 'dQ', 'dK', 'dV')}
    rcs = scaled_calls(csr, n, shape, inp, tuple(out.values()), scaled_bounds(ops, dev), stats, csr.csc_positions(),
                       keep, n_all=g.N)
    return out, rcs


def finish_all(out, g, n, want, name):
    """finish_rows over the placed outputs {'O' | 'dQ' | 'dK' | 'dV': placed}; the failures."""
    bad = []
    for (label, by_source), ref in zip((('O', False), ('dQ', False), ('dK', True), ('dV', True)), want):
        if label in out:
            try:
                finish_rows(label, out[label], n, g.outdeg if by_source else g.indeg, ref, name, by_source)
            except AssertionError as e:
                bad.append(str(e))
    return bad


# ----------------------------------------------------------------------------------------------- plans and n_rows
@gpu
@pytest.mark.parametrize('shape', [(20, 32, 2), (4, 32, 4), (40, 50, 2)], ids=shape_id)
def test_a_plan_over_the_rows_of_the_call(shape, dev):
    """include/ampconv.h, long segments: a plan passed to an edge call is built over exactly the rows the call covers.
    The ladder cut at row 28 (long rows on both sides of the cut), the plan from ampconv_hub_plan over those 28 rows:
    the forward and the destination pass of the one-wave, the short-sequence and the workgroup-per-unit family (the fp32
    families that take plans) write rows 0..27 as the model has them and leave every row behind them alone."""
    lib, g, chunk, n = _lib.load(), graph('L', 64), 64, 28
    L, dh, H = shape
    D, csr = dh * H, g.csr(chunk)
    cut = chunks_per_row(g.indeg[:n], chunk)
    assert len(cut) and len(chunks_per_row(g.indeg[n:], chunk)) and g.indeg[22] == chunk
    plan = torch.empty(lib.ampconv_hub_plan_bytes(g.E, chunk) // 4, dtype=torch.int32, device=dev)
    _lib.check(lib.ampconv_hub_plan(csr.rowptr.data_ptr(), n, g.E, chunk, plan.data_ptr(), stream()), 'hub_plan')
    header = plan[:4].tolist()
    assert header[:3] == [int(cut.sum()), chunk, len(cut)], (header, cut)     # the row of exactly `chunk` edges is not cut
    nch = header[0]
    ws = torch.empty(nch * L * D, device=dev)
    ops = operands(F32, shape, g.N)
    q, k, v, go = (place(t, 'nld', torch.float32, r) for t, r in zip(ops, ('Q', 'K', 'V', 'dO')))
    O, dQ = (place((g.N, L, H, dh), 'nld', torch.float32, 'out0') for _ in range(2))
    rp, cl = csr.rowptr.data_ptr(), csr.col.data_ptr()
    rule = TABLE[F32, shape][16]
    assert rule[0] == rule[1] and FAMILY_NAME[rule[0]] in ('mfma', 'small', 'block')
    _lib.check(lib.ampconv_fwd_edge(q.view, k.view, v.view, rp, cl, None, n, L, D, H, O.view, plan.data_ptr(), nch,
                                    ws.data_ptr(), _lib.AMPCONV_F32, stream()), 'fwd')
    _lib.check(lib.ampconv_bwd_edge_dst(q.view, k.view, v.view, go.view, rp, cl, n, L, D, H, dQ.view, plan.data_ptr(), nch,
                                        ws.data_ptr(), None, None, None, _lib.AMPCONV_F32, stream()), 'dst')
    torch.cuda.synchronize()
    want = reference(F32, shape, 'L', chunk)
    bad = finish_all({'O': O, 'dQ': dQ}, g, n, want, f'plan over {n} rows {shape_id(shape)} [{FAMILY_NAME[rule[0]]}]')
    assert not bad, bad


# ------------------------------------------------------------------------------------------- the token-count sweep
def sweep(dtype, shapes, rules, small=True):
    """five_calls on graph B (40 nodes, 160 edges, n_rows = 33, no plan) at every shape of `shapes`, each held to the
    header's rule for it -- rules(L): the rule the caller means to sweep at that token count -- and to its own fp64
    model; {shape: failures} of the shapes that failed."""
    failed = {}
    for shape in shapes:
        rule = header_rule(dtype, shape, small)
        assert rule is rules(shape[0]), f'{shape_id(shape)}: not the shape class this sweep is about'
        ops = make_operands(dtype, shape, graph('B').N)
        g = graph('B')
        want = (er.fwd(*ops[:3], g.rowptr, g.col),) + er.bwd(*ops, g.rowptr, g.col)
        bad = verdict(five_calls(dtype, shape, 'B', ops=ops, rule=rule), want)
        if bad:
            failed[shape_id(shape)] = bad
    return failed


@gpu
@pytest.mark.parametrize('dh', (16, 32))
@pytest.mark.parametrize('variant', ('f32', 'f32-small-off', 'bf16'))
def test_every_token_count_one_wave_per_unit(variant, dh, dev, monkeypatch):
    """L = 1..20 at dh = 16 and 32, H = 2.  fp32: the short-sequence kernels up to L = 4, the plain tile kernels up to
    16 (at 16: no masked row), batched tails on 17..19, the full tile at 20; with AMPCONV_SMALL=0 the tile kernels from
    L = 1; bf16 storage: its own one-wave family at every L."""
    if variant == 'f32-small-off':
        monkeypatch.setenv('AMPCONV_SMALL', '0')
    rules = {'f32': lambda L: _SMALL_V1 if L <= 4 else _ONE_WAVE, 'f32-small-off': lambda L: _ONE_WAVE,
             'bf16': lambda L: _BF_ONE_WAVE}[variant]
    failed = sweep(BF16 if variant == 'bf16' else F32, [(L, dh, 2) for L in range(1, 21)], rules, small=variant == 'f32')
    assert not failed, failed


@gpu
@pytest.mark.parametrize('dh', (16, 32))
def test_every_token_count_planes(dh, dev):
    """The plane entry points at L = 1..20, H = 2, on graph B's first 33 rows, without and with the statistics."""
    lib, g, failed = _lib.load(), graph('B'), {}
    csr = g.csr()
    for L in range(1, 21):
        shape, keep, bad = (L, dh, 2), [], []
        assert lib.ampconv_planes_supported(L, 2 * dh, 2) == 1
        ops = make_operands(F32, shape, g.N)
        want = (er.fwd(*ops[:3], g.rowptr, g.col),) + er.bwd(*ops, g.rowptr, g.col)
        planes, bounds = plane_operands(ops, g.indeg, dev)
        inp = [place(t, 'nld', torch.float32, r) for t, r in zip(planes, ('Q', 'K', 'V', 'dO'))]
        stats = nan_buffer(g.E * 2 * 40)
        for with_stats in (False, True):
            name = f'planes {shape_id(shape)} B' + ('/stats' if with_stats else '')
            out = planes_calls(csr, g.n_rows, shape, inp, 'nld', with_stats, bounds, stats, csr.csc_positions(), keep,
                               name, n_all=g.N)
            bad += finish_all(out, g, g.n_rows, want, name)
        if bad:
            failed[shape_id(shape)] = bad
    assert not failed, failed


@gpu
@pytest.mark.parametrize('dh,H', ((12, 2), (50, 2), (64, 1)), ids=lambda x: str(x))
@pytest.mark.parametrize('variant', ('f32', 'bf16', 'scaled'))
def test_every_token_count_workgroup_per_unit(variant, dh, H, dev):
    """L = 1..64 (1 to 4 token tiles, L = 16 | 17, 32 | 33, 48 | 49 at the tile borders) at dh = 12, dh = 50 (dh % 4 == 2)
    and dh = 64 (two k-steps): fp32 (at dh = 64, H = 1 the short-sequence kernels serve L <= 4: the rule says so), bf16
    storage, and the `_scaled` entry points wherever ampconv_scaled_supported says 1 -- which must be every L here."""
    shapes = [(L, dh, H) for L in range(1, 65)]
    if variant != 'scaled':
        rules = (lambda L: _BF_PER_UNIT) if variant == 'bf16' else \
            (lambda L: _SMALL_V2 if L <= 4 and (dh, H) == (64, 1) else _PER_UNIT)
        failed = sweep(BF16 if variant == 'bf16' else F32, shapes, rules)
        assert not failed, failed
        return
    lib, g, failed = _lib.load(), graph('B'), {}
    csr = g.csr()
    for shape in shapes:
        assert lib.ampconv_scaled_supported(shape[0], dh * H, H) == 1, shape
        ops = make_operands(F32, shape, g.N)
        want = (er.fwd(*ops[:3], g.rowptr, g.col),) + er.bwd(*ops, g.rowptr, g.col)
        out, rcs = scaled_run(g, csr, shape, ops, g.n_rows, dev, [])
        bad = [f'return codes {rcs}'] if rcs != [0, 0, 0] else finish_all(out, g, g.n_rows, want, f'scaled {shape_id(shape)} B')
        if bad:
            failed[shape_id(shape)] = bad
    assert not failed, failed


@gpu
@pytest.mark.parametrize('dh,H', SHORT, ids=lambda x: str(x))
def test_every_token_count_short_sequences(dh, H, dev):
    """L = 1..4 at the (dh, H) of the table's short-sequence rows: 1, 2 and 4 channels per lane."""
    assert len(SHORT) == 4
    rule = {(16, 8): _SMALL_V2, (16, 2): _SMALL_V1, (32, 4): _SMALL_V2, (32, 8): _SMALL_V4}[dh, H]
    failed = sweep(F32, [(L, dh, H) for L in range(1, 5)], lambda L: rule)
    assert not failed, failed


@gpu
def test_token_counts_generic(dev):
    """The generic kernels: one token, odd dh; L just past the one-wave kernels' 20 with odd dh; L past the workgroup
    kernels' 64; dh past 64 at L = 20."""
    failed = sweep(F32, [(1, 5, 3), (21, 7, 2), (65, 6, 2), (20, 96, 1)], lambda L: _GENERIC)
    assert not failed, failed
