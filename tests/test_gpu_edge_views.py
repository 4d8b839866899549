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

import numpy as np
import pytest
import torch

import edge_reference as er
from conftest import assert_close_scaled
from edge_layouts import place, read
from edge_runner import (B16, BADARG, BF16, BLOCK, CALL_NAME, CODE, DST, DST_S, EDTYPE, F32, FAMILY_NAME, FWD, GEN,
                         LABEL_CALL, MFMA, SMALL, SRC, SRC_S, TABLE, TDT, TOL, _BF_ONE_WAVE, Run, _finish, case_id,
                         compare, expected_family, family, graph, hub, operands, plane_operands, planes_calls,
                         reference, scaled_bounds, scaled_calls, stream)

from ampnet_amd import _lib

gpu = pytest.mark.gpu
LAYOUT_IDS = ('nld', 'packed3', 'nhld', 'hnld', 'lnd', 'pad16', 'pad8', 'pad4', 'mixed')


def layouts_of(dtype):
    return tuple(l for l in LAYOUT_IDS if not (dtype == BF16 and l == 'pad4'))


ALL_CASES = [(dt, shape, lay) for (dt, shape) in TABLE for lay in layouts_of(dt)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def qidx_rows():
    """Graph C: 50 rows of 0..5 edges over 40 nodes, queries from random nodes (repeats, not the identity)."""
    rng = np.random.default_rng(13)
    deg = rng.integers(0, 6, 50)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col, qidx = rng.integers(0, 40, rowptr[-1]), rng.integers(0, 40, 50)
    assert (deg == 0).any() and len(set(qidx)) < 50 and (qidx != np.arange(50)).any()
    return rowptr, col, qidx


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
    ops = operands(F32, shape, g.N)
    O_, dQ_, dK_, dV_ = reference(F32, shape, 'A')
    planes, bounds = plane_operands(ops, g.indeg, dev)
    stats = torch.empty(g.E * H * 40, device=dev)
    spos = csr.csc_positions()
    rp, cl, cp, cr = (t.data_ptr() for t in (csr.rowptr, csr.col, csr.cscptr, csr.crow))
    for lin in ('packed3', 'pad16'):
        inp = [place(t, lin, torch.float32, r) for t, r in zip(planes, ('Q', 'K', 'V', 'dO'))]
        for lout in ('nld', 'nhld', 'pad16'):
            for with_stats in (False, True):
                name = f'planes L{L}dh{dh}H{H} {lin}->{lout}' + ('/stats' if with_stats else '')
                out = planes_calls(csr, g.N, shape, inp, lout, with_stats, bounds, stats, spos, keep, name)
                if not with_stats:
                    _finish('O', out['O'], g.N, g.indeg, O_, name)
                _finish('dQ', out['dQ'], g.N, g.indeg, dQ_, name)
                _finish('dK', out['dK'], g.N, g.outdeg, dK_, name, g.outdeg)
                _finish('dV', out['dV'], g.N, g.outdeg, dV_, name, g.outdeg)
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
    bounds = scaled_bounds(ops, dev)
    stats = torch.empty(lib.ampconv_softmax_stats_bytes(g.E, L, D, H, _lib.AMPCONV_F32) // 4, device=dev)
    spos = csr.csc_positions()
    for layout in ('nld', 'nhld', 'pad8', 'pad4'):
        name = f'scaled L{L}dh{dh}H{H} {layout}'
        inp = [place(t, layout, torch.float32, r) for t, r in zip(ops, ('Q', 'K', 'V', 'dO'))]
        O, dQ, dK, dV = (place((g.N, L, H, dh), layout, torch.float32, 'out0') for _ in range(4))
        rcs = scaled_calls(csr, g.N, shape, inp, (O, dQ, dK, dV), bounds, stats, spos, keep, src_plan=layout != 'pad4')
        if layout == 'pad4':
            assert rcs == [BADARG] * 3, rcs
            for p in (O, dQ, dK, dV):
                assert p.outside_intact() and p.unwritten() == p.index.numel()
            continue
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
