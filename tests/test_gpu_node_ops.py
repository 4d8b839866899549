"""The node-side helpers around the edge phase, ONE C CALL AT A TIME through ctypes: ampconv_gather_segment_sum,
ampconv_segment_mean, ampconv_mask_rows, ampconv_masked_colsum (csrc/node_ops.hip), each against its fp64 model of
tests/linear_reference.py.

Every buffer lies inside a larger allocation (edge_layouts.place_flat): inputs between NaN margins, outputs in an
allocation full of the sentinel; after every call nothing outside the output may have changed and everything inside
must have been written.  The library is built with -fno-honor-nans, under which a compiler may turn "skip this row"
into a multiplication by 0: every masked path is run with NaN and infinity in the rows it must not read.  The bars are
linear_reference's (exact data: bit-equal, 2 ulp where a mean divides by a degree that is no power of two; random data:
(n + 4) 2^-24 S; masked_colsum on random data: the column-sum bar of tests/test_gpu_proj.py);
tests/test_linear_reference_cpu.py shows that they reject a dropped last edge, an ignored weight, a wrong segment
length, a skipped tail and a masked row let through.  Every sweep names all its failing cases in one assertion."""
import numpy as np
import pytest
import torch

import linear_reference as lr
from edge_layouts import SENTINEL, place_flat
from edge_runner import graph, stream

from ampnet_amd import _lib

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CODE = {F32: _lib.AMPCONV_F32, BF16: _lib.AMPCONV_BF16}
BADARG = -1
SHARE = {}          # call -> the largest share of its random-data bound used, printed by every test that raises it


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def raw(p):
    """The values of a placed buffer as float32 (fp32: bit for bit; bf16: exactly)."""
    return p.backing[p.index.reshape(-1)].reshape(p.index.shape).float().cpu().numpy()


def written(p, name, rows=None):
    bad = []
    if not p.outside_intact(rows):
        bad.append(f'{name}: bytes outside the output were written')
    if p.unwritten(rows):
        bad.append(f'{name}: {p.unwritten(rows)} elements of the output were not written')
    return bad


def untouched(p, name):
    return [] if p.outside_intact() and p.unwritten() == p.index.numel() else [f'{name}: the output was written']


def note(call, share, name, what):
    if share > SHARE.get(call, 0.0):
        SHARE[call] = share
        print(f'[bar] {call}: {100 * share:.1f} % of {what} at {name}')


def judge_segments(call, name, kind, got, ref, S, deg, mean):
    """Exact data: bit-equal, 2 ulp in the rows whose mean divides by no power of two; random data: (deg + 4) 2^-24 S.
    Rows of empty segments: +0 bits either way."""
    bad = []
    if got[deg == 0].view(np.int32).any():
        bad.append(f'{name}: rows of empty segments are not exact zeros')
    if kind == 'exact':
        miss = lr.exact_problems(got, ref, ~lr.pow2(deg)[:, None] if mean else None)
        return bad + ([f'{name}: {miss}/{got.size} elements miss the exact bar'] if miss else [])
    share = lr.random_share(got, ref, S, deg[:, None])
    note(call, share, name, '(n + 4) 2^-24 S')
    return bad + ([f'{name}: {share:.3g} times the bound (n + 4) 2^-24 S'] if share > 1 else [])


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


# --------------------------------------------------------------------------------------------------- gather_segment_sum
def ladder_sides():
    """{side: (ptr, idx, the library's arrays as numpy, segment lengths, which rows no segment names)} of the ladder:
    the dst-sorted CSR and the src-sorted CSC of ampconv_graph_build, with its cinv."""
    g = graph('L')
    csr = g.csr()
    cinv = csr.cinv.cpu().numpy()
    return g, {'csr': (csr.rowptr, csr.col, csr.rowptr.cpu().numpy(), csr.col.cpu().numpy(), g.indeg, g.outdeg == 0),
               'csc': (csr.cscptr, csr.crow, csr.cscptr.cpu().numpy(), csr.crow.cpu().numpy(), g.outdeg, g.indeg == 0)}, cinv


def run_gather(lib, side, F, kind, weights, mean, sides):
    g, table, cinv = sides
    ptr, idx, ptr_h, idx_h, deg, unnamed = table[side]
    name = f'gather_segment_sum {side} F={F} {kind} w={weights} mean={mean}'
    rows = lr.poison(lr.rows(kind, g.N, F, lo=-7, hi=7), unnamed)          # NaN in the rows no segment names
    w = {'none': None, 'pow2': lr.pow2_weights(g.E), 'cinv': cinv[:g.E]}[weights]
    pr, po = place_flat(rows, F32), place_flat((g.N, F), F32)
    pw = None if w is None else place_flat(w, F32)
    rc = lib.ampconv_gather_segment_sum(pr.ptr, ptr.data_ptr(), idx.data_ptr(), None if w is None else pw.ptr, mean, g.N, F,
                                        po.ptr, stream())
    torch.cuda.synchronize()
    if rc != 0:
        return [f'{name}: returned {rc}'] + untouched(po, name)
    ref, S = lr.gather_segment_sum(rows, ptr_h, idx_h, w, mean)
    return written(po, name) + judge_segments('gather_segment_sum', name, kind, raw(po), ref, S, deg, mean)


@pytest.fixture(scope='module')
def sides(lib):
    return ladder_sides()


@pytest.mark.parametrize('F', [4, 108, 1028, 4096, 5000])
def test_gather_segment_sum_on_the_ladder(F, lib, sides):
    """One lane; a second blockIdx.y column that holds one lane (F = 1028); four full columns; a last column partly
    filled.  The ladder's CSR with mean = 1 and its CSC with per-edge weights (exact: powers of two; random: the real
    cinv, the model reading the same fp32 values); w = NULL with mean = 0."""
    failed = []
    for kind in ('exact', 'random'):
        failed += run_gather(lib, 'csr', F, kind, 'none', 1, sides)
        failed += run_gather(lib, 'csc', F, kind, 'pow2' if kind == 'exact' else 'cinv', 0, sides)
        failed += run_gather(lib, 'csr', F, kind, 'none', 0, sides)
    failed += run_gather(lib, 'csr', F, 'exact', 'pow2', 1, sides)
    assert not failed, failed


def test_gather_segment_sum_refusals(lib, sides):
    """F % 4 != 0; `rows` or `out` off 16 bytes; more than 65535 * 256 columns of four: -1 before anything runs."""
    g, table, _ = sides
    ptr, idx = table['csr'][:2]
    rows = lr.rows('exact', g.N, 8)
    for label, F, skew_in, skew_out in (('F % 4', 6, 0, 0), ('rows off 16 bytes', 8, 1, 0), ('out off 16 bytes', 8, 0, 2),
                                        ('F / 4 > 65535 * 256', 4 * (65535 * 256 + 1), 0, 0)):
        pr, po = place_flat(rows, F32, skew=skew_in), place_flat((g.N, 8), F32, skew=skew_out)
        rc = lib.ampconv_gather_segment_sum(pr.ptr, ptr.data_ptr(), idx.data_ptr(), None, 0, g.N, F, po.ptr, stream())
        torch.cuda.synchronize()
        assert rc == BADARG and not untouched(po, label), (label, rc)


# --------------------------------------------------------------------------------------------------------- segment_mean
def run_segment_mean(lib, F, kind, sides, n_rows=None):
    g = sides[0]
    csr = g.csr()
    n = g.N if n_rows is None else n_rows
    name = f'segment_mean F={F} {kind} rows={n}'
    rowptr, eperm = csr.rowptr.cpu().numpy(), csr.eperm.cpu().numpy()
    named = np.zeros(g.E, bool)
    named[eperm[:rowptr[n]]] = True
    msg = lr.poison(lr.rows(kind, g.E, F), ~named)                          # NaN in the message rows no edge names
    pm, po = place_flat(msg, F32), place_flat((n, F), F32)
    rc = lib.ampconv_segment_mean(pm.ptr, csr.rowptr.data_ptr(), csr.eperm.data_ptr(), n, F, po.ptr, stream())
    torch.cuda.synchronize()
    if rc != 0:
        return [f'{name}: returned {rc}'] + untouched(po, name)
    ref, S = lr.segment_mean(msg, rowptr[:n + 1], eperm, F)
    return written(po, name) + judge_segments('segment_mean', name, kind, raw(po), ref, S, g.indeg[:n], 1)


@pytest.mark.parametrize('F', [1, 3, 255, 256, 257, 5120])
def test_segment_mean_on_the_ladder(F, lib, sides):
    failed = []
    for kind in ('exact', 'random'):
        failed += run_segment_mean(lib, F, kind, sides)
    assert not failed, failed


def test_segment_mean_leaves_unnamed_messages_unread(lib, sides):
    """Over the first 30 rows only: the messages of the later rows' edges hold NaN and infinity."""
    failed = run_segment_mean(lib, 257, 'random', sides, n_rows=30) + run_segment_mean(lib, 3, 'exact', sides, n_rows=30)
    assert not failed, failed


def test_segment_mean_without_edges(lib):
    rowptr, eperm, po = i32(np.zeros(8)), i32(np.zeros(1)), place_flat((7, 5), F32)
    assert lib.ampconv_segment_mean(None, rowptr.data_ptr(), eperm.data_ptr(), 7, 5, po.ptr, stream()) == 0
    torch.cuda.synchronize()
    assert not written(po, 'E = 0') and not raw(po).view(np.int32).any()


def test_aggregate_equals_the_call(lib, sides):
    """AMPConv.aggregate (its own graph build over the destinations) gives the bits of the call on the ladder."""
    from ampnet_amd import AMPConv
    g = sides[0]
    csr = g.csr()
    msg = torch.from_numpy(lr.rows('random', g.E, 257)).cuda()
    out = torch.empty(g.N, 257, device='cuda:0')
    _lib.check(lib.ampconv_segment_mean(msg.data_ptr(), csr.rowptr.data_ptr(), csr.eperm.data_ptr(), g.N, 257, out.data_ptr(),
                                        stream()), 'ampconv_segment_mean')
    got = AMPConv(4, 2).to('cuda:0').aggregate(msg, torch.from_numpy(g.dst).cuda(), dim_size=g.N)
    assert torch.equal(got, out)


# ------------------------------------------------------------------------------------------------------------ mask_rows
def bits(p):
    return p.bits().cpu().numpy().astype(np.int64)


def run_mask_rows(lib, dtype, n, F, skew, rowptr_h, name):
    """Rows to be zeroed hold NaN and infinity and must come back as +0 BITS; every other element of the allocation --
    the other rows, the margins -- must be bit-identical afterwards."""
    empty = np.diff(rowptr_h) == 0
    Y = lr.poison(lr.rows('random', n, F), empty)
    p = place_flat(Y, dtype, skew=skew)
    before = bits(p)
    rc = lib.ampconv_mask_rows(p.ptr, i32(rowptr_h).data_ptr(), n, F, CODE[dtype], stream())
    torch.cuda.synchronize()
    if rc != 0:
        return [f'{name}: returned {rc}']
    after, idx = bits(p), p.index.cpu().numpy()
    bad = []
    if after[idx[empty]].any():
        bad.append(f'{name}: {int((after[idx[empty]] != 0).sum())} elements of the rows to zero are not +0')
    keep = np.ones(len(after), bool)
    keep[idx[empty].reshape(-1)] = False
    same = after[keep] == before[keep]
    if not same.all():
        bad.append(f'{name}: {int((~same).sum())} elements outside the rows to zero changed')
    return bad


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
def test_mask_rows_at_every_row_length_and_alignment(dtype, lib):
    """Row lengths of 4, 8, 12 bytes (element stores), 16, 1024, 1040, 1200 (16-byte stores, once past the wavefront's
    1024-byte stride), 1028 (element stores over several strides); the same with the base 4 bytes off a 16-byte
    boundary, where rows of whole 16 bytes take the element path too.  N = 5 and 7: a last workgroup partly filled,
    with a row to zero in it."""
    esize = 4 if dtype == F32 else 2
    failed = []
    for n in (1, 4, 5, 7, 40):
        rowptr = np.concatenate([[0], np.cumsum(np.arange(n) % 2)])         # the even nodes are empty, node n - 1 of 5, 7 too
        for nbytes in (4, 8, 12, 16, 1024, 1040, 1200, 1028):
            for off in (0, 4):
                failed += run_mask_rows(lib, dtype, n, nbytes // esize, off // esize, rowptr,
                                        f'mask_rows N={n} row={nbytes} B base+{off}')
    assert not failed, failed


@pytest.mark.parametrize('which', [1, 2, 3])
def test_mask_rows_with_a_node_list(which, lib):
    """With the `ptr` array of ampconv_active_nodes, exactly the rows of the nodes NOT listed are zeroed."""
    g = graph('B')
    csr = g.csr()
    N = g.N
    nws = lib.ampconv_active_nodes_workspace_bytes(N)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device='cuda:0')
    ids, ptr, count = (torch.empty(k, dtype=torch.int32, device='cuda:0') for k in (N + 8, N + 1, 1))
    _lib.check(lib.ampconv_active_nodes(csr.rowptr.data_ptr(), csr.cscptr.data_ptr(), N, which, ids.data_ptr(), ptr.data_ptr(),
                                        count.data_ptr(), ws.data_ptr(), nws, stream()), 'ampconv_active_nodes')
    listed = {1: g.indeg > 0, 2: g.outdeg > 0, 3: (g.indeg > 0) | (g.outdeg > 0)}[which]
    assert int(count) == listed.sum() and np.array_equal(np.diff(ptr.cpu().numpy()) == 1, listed) and not listed.all()
    failed = []
    for dtype, F in ((F32, 260), (F32, 3), (BF16, 520), (BF16, 6)):
        failed += run_mask_rows(lib, dtype, N, F, 0, ptr.cpu().numpy(), f'mask_rows which={which} {dtype} F={F}')
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------- masked_colsum
def third_empty(n):
    """A CSR row pointer over n nodes in which the segments of the nodes n % 3 == 1 are empty."""
    deg = np.arange(n) % 4 + 1
    deg[np.arange(n) % 3 == 1] = 0
    return np.concatenate([[0], np.cumsum(deg)])


def run_colsum(lib, dtype, n, L, D, kind):
    name = f'masked_colsum {"f32" if dtype == F32 else "bf16"} N={n} L={L} D={D} {kind}'
    rowptr = third_empty(n)
    dY = lr.rows(kind, n, L * D)
    if dtype == BF16:
        dY = torch.from_numpy(dY).bfloat16().float().numpy()
    ref, S = lr.masked_colsum(dY.reshape(n, L, D), rowptr)
    pin = place_flat(lr.poison(dY, np.diff(rowptr) == 0), dtype)           # NaN and infinity in the rows to leave out
    rp = i32(rowptr)
    outs = []
    for _ in range(2):
        po = place_flat(((1 + _lib.COLSUM_BLOCKS) * D,), F32)
        rc = lib.ampconv_masked_colsum(pin.ptr, rp.data_ptr(), n, L, D, po.ptr, CODE[dtype], stream())
        torch.cuda.synchronize()
        if rc != 0:
            return [f'{name}: returned {rc}']
        if not po.outside_intact():
            return [f'{name}: bytes behind the (1 + {_lib.COLSUM_BLOCKS}) D floats of `out` were written']
        outs.append(raw(po)[:D])
    bad = []
    if (outs[0].view(np.int32) == np.int32(SENTINEL[F32])).any():
        bad.append(f'{name}: results were not written')
    if not np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)):
        bad.append(f'{name}: two calls differ')
    if kind == 'exact':
        miss = lr.exact_problems(outs[0], ref)
        return bad + ([f'{name}: {miss}/{D} columns are not bit-equal to the model'] if miss else [])
    share = lr.colsum_share(outs[0], ref, S)
    note('masked_colsum', share, name, '1e-6 max_c sum |x| + 1e-6')
    return bad + ([f'{name}: {share:.3g} times the column-sum bar'] if share > 1 else [])


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('n', [1, 3, 1023, 1024, 1025, 2049, 4100])
def test_masked_colsum_at_every_node_count(n, dtype, lib):
    """Both sides of 1, 2, 3 and 5 nodes per slice (1024 slices), at (L, D) = (5, 100) and (20, 257)."""
    failed = []
    for L, D in ((5, 100), (20, 257)):
        for kind in ('exact', 'random'):
            failed += run_colsum(lib, dtype, n, L, D, kind)
    assert not failed, failed


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('L', [1, 2, 3, 4, 5, 20])
def test_masked_colsum_at_every_token_and_column_count(L, dtype, lib):
    """The four-way unroll and its tail (L), fewer and more columns than threads (D), at N = 1025."""
    failed = []
    for D in (1, 3, 100, 256, 257, 300):
        for kind in ('exact', 'random'):
            failed += run_colsum(lib, dtype, 1025, L, D, kind)
    assert not failed, failed


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
def test_masked_colsum_without_nodes(dtype, lib):
    D = 100
    po = place_flat(((1 + _lib.COLSUM_BLOCKS) * D,), F32)
    assert lib.ampconv_masked_colsum(None, None, 0, 5, D, po.ptr, CODE[dtype], stream()) == 0
    torch.cuda.synchronize()
    assert po.outside_intact() and not raw(po)[:D].view(np.int32).any()
    assert (raw(po)[D:].view(np.int32) == np.int32(SENTINEL[F32])).all()
