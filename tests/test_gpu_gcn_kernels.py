"""csrc/gcn.hip one library call at a time (ampnet_amd._lib, no Python wrapper in between) against the numpy fp64 model
of tests/gcn_reference.py, on ladders around the kernels' own tile sizes.

test_gpu_gcn.py runs the models' shapes through ampnet_amd.gcn, where several loops of the kernels take one trip only.
Here: a second and a partial output tile of the input kernels (kJ = 16), a second and a partial row tile of the weight
gradient (kWgRows = 64 rows, 64 chunks), the column sum past its 1024 chunks of 32 rows, long segments around the part
size (AMPCONV_GCN_PART) and more parts and long rows than the two long-segment kernels have workgroups, and the edges of
kRows = 16, kPrepF = kWgF = 64, kKC = 128 and of the four rows per workgroup of the norm kernel.

Buffers: every tensor the library touches lies between guard bands of 0xFF bytes (tests/site_guards.py); a workspace is
exactly *_workspace_bytes long and 0xFF throughout before the call (NaN as a float, -1 as an int), so a slot that is
read before it is written shows; output rows are wider than C and their padding must still hold 0xFF afterwards; input
rows are padded with NaN.  `close` refuses a value that is not finite before it compares.
Tolerances: the project's flat atol 1e-5, rtol 1e-4 on per-row outputs (h, out); the magnitude-scaled bar on sums over
the nodes (dW under the label gW, dtable under g_table, the column sum), dinv at rtol 2e-7 (test_gpu_gcn.py).
Inputs are CPU-seeded; the fp64 results are computed once per case and cached."""
import functools
import math

import numpy as np
import pytest
import torch

import gcn_reference as R
from site_guards import FILL, Guarded, bits, close, header_constant

from ampnet_amd import _lib
from ampnet_amd.graph import _stream

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OK, E_BADARG, E_WORKSPACE = 0, -1, -3           # include/ampconv.h, the status enum
LONG = header_constant('AMPCONV_GCN_LONG_SEGMENT')
PART = header_constant('AMPCONV_GCN_PART')
F32, U8 = torch.float32, torch.uint8


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def _ok(rc, name):
    torch.cuda.synchronize()
    assert rc == OK, (name, rc)


def _p(buf):
    return None if buf is None else buf.ptr


def _put(t, offset=0):
    return None if t is None else Guarded.of(DEV, t, offset)


def _rows_in(t, ld, offset=0):
    """t [N, C] as rows `ld` floats apart, NaN in the padding, between guard bands."""
    N, C = t.shape
    host = torch.full((N, ld), float('nan'))
    host[:, :C] = t
    return Guarded.of(DEV, host, offset)


def _rows_out(buf, N, C, ld, name):
    """The [N, C] block of an output buffer of N rows of ld floats, after checking that the bands around the buffer and
    the columns >= C of every row still hold the fill."""
    assert buf.intact(), f'{name}: a byte outside the buffer was written'
    rows = buf.t.view(N, ld)
    assert bool((bits(rows[:, C:]) == -1).all()), f'{name}: a padding column was written'
    return rows[:, :C]


def _linear_out(buf, name):
    assert buf.intact(), f'{name}: a guard element was written'
    assert buf.written(), f'{name}: an element was left unwritten'
    return buf.t


def _untouched(buf):
    return bool((buf.backing == FILL).all())


# ---- 1 / 2. the first layer over the embedded input -------------------------------------------------------------------
NS = (1, 15, 16, 17, 33)                         # kRows = 16 rows per workgroup of the forward
FS = (1, 63, 64, 65, 127, 128, 129, 257)         # kPrepF = kWgF = 64, kKC = 128
CS = (17, 18, 19, 32, 15, 16, 33, 1)             # kJ = 16 outputs per tile (in the order the walk below wants)
VS = (('embedded', 1), ('embedded', 3), ('embedded', 65), ('zscore', 0), ('raw', 0))    # the ABI ties the mode to De


def _input_cases():
    """40 of the 5 x 8 x 8 x 5 combinations: N and F walk their lists together (5 and 8 are coprime: every pair once), C
    walks with F and is shifted by two per round of N, the variant changes per round of F.
    test_input_cases_cover_the_ladder holds the set to the coverage rule."""
    return [(NS[i % 5], FS[i % 8], CS[(i % 8 + 2 * (i // 5)) % 8], VS[i // 8][1], VS[i // 8][0]) for i in range(40)]


INPUT_CASES = _input_cases()
# the row tiles of the weight gradient: chunks = min(ceil(N / 64), 64), a chunk is ceil(N / chunks) rows, walked in tiles
# of 64.  63, 64, 65: one chunk, then two of 33 / 32.  4096: 64 chunks of 64 (the last N with one tile).  4097: chunks of 65
# (two tiles, the second of one row; the last chunk has 2 rows).  4160: 65 everywhere.  8200: chunks of 129: three tiles,
# the last of one row (the last chunk: 73 rows, two tiles).
LARGE_NS = (63, 64, 65, 4096, 4097, 4160, 8200)
LARGE_VS = (('embedded', 1), ('embedded', 3), ('zscore', 0), ('raw', 0))
BWD_LARGE = [(N, (63, 64, 65)[(i + k) % 3], C, LARGE_VS[(i + 2 * k) % 4][1], LARGE_VS[(i + 2 * k) % 4][0])
             for i, N in enumerate(LARGE_NS) for k, C in enumerate((17, 33))]


def _case_id(c):
    return 'N%d_F%d_C%d_De%d_%s' % c


def wgrad_tiles(N):
    """(rows per chunk, tiles of the longest chunk) from input_wgrad_kernel's launch arithmetic (wgrad_chunks, kWgRows)."""
    chunks = min(max(-(-N // 64), 1), 64)
    per = -(-N // chunks)
    return per, -(-per // 64)


def test_input_cases_cover_the_ladder():
    assert len(set(INPUT_CASES)) == 40
    axes = {'N': (0, NS), 'F': (1, FS), 'C': (2, CS), 'De': (3, (0, 1, 3, 65)), 'mode': (4, ('embedded', 'zscore', 'raw'))}
    for a, (ia, values) in axes.items():
        for v in values:
            mine = [c for c in INPUT_CASES if c[ia] == v]
            assert mine, (a, v)
            for b, (ib, _) in axes.items():
                if a == b or {a, b} == {'De', 'mode'}:         # De > 0 is the embedded mode and nothing else (ampconv.h)
                    continue
                assert len({c[ib] for c in mine}) >= 2, f'{a} = {v} meets one value of {b} only'
    for C in CS:
        if C > 16:
            assert any(c[2] == C and c[1] > 128 for c in INPUT_CASES), f'C = {C} never meets F > 128'
    assert {m for *_, De, m in INPUT_CASES if De == 0} == {'zscore', 'raw'}
    for N in LARGE_NS:
        assert {c[2] for c in BWD_LARGE if c[0] == N} == {17, 33}
    assert all(c[1] <= 65 and c[3] <= 3 for c in BWD_LARGE)
    assert [wgrad_tiles(N) for N in LARGE_NS] == [(63, 1), (64, 1), (33, 1), (64, 1), (65, 2), (65, 2), (129, 3)]


@functools.lru_cache(maxsize=None)
def input_operands(N, F, C, De, mode):
    """x standard normal with one constant column (F >= 2: column F // 2, all 1, or all 0 in the raw mode, so that z is
    exactly 0 there); mean and inv_std by sklearn's rule in fp64 on the host, rounded to fp32: kernel and model read the
    same two vectors (ampconv_feat_zscore_stats has its own tests)."""
    g = torch.Generator().manual_seed(1000003 * N + 1009 * F + 31 * C + De)
    x = torch.randn(N, F, generator=g)
    fc = F // 2 if F >= 2 else None
    if fc is not None:
        x[:, fc] = 0.0 if mode == 'raw' else 1.0
    bound = math.sqrt(6.0 / (F * (De + 1) + C))
    W = (torch.rand(C, F * (De + 1), generator=g) * 2 - 1) * bound
    table = torch.randn(F, De, generator=g) if De else None
    grad = torch.randn(N, C, generator=g)
    mean = inv_std = None
    if mode != 'raw':
        x64 = x.numpy().astype(np.float64)
        m, v = x64.mean(axis=0), x64.var(axis=0)
        scale = np.where(v > 1e-12 * np.maximum(1.0, m * m), np.sqrt(v), 1.0)
        mean, inv_std = torch.from_numpy(m.astype(np.float32)), torch.from_numpy((1.0 / scale).astype(np.float32))
        if fc is not None:
            assert mean[fc] == 1.0 and inv_std[fc] == 1.0
    return x, W, table, grad, mean, inv_std, fc


@functools.lru_cache(maxsize=None)
def input_reference(N, F, C, De, mode):
    x, W, table, grad, mean, inv_std, _ = input_operands(N, F, C, De, mode)
    stats = None if mean is None else (mean.numpy(), inv_std.numpy())
    tab = None if table is None else table.numpy()
    h = R.input_linear(x.numpy(), W.numpy(), tab, mode, stats)
    dW, dtable = R.input_linear_backward(x.numpy(), W.numpy(), tab, grad.numpy(), mode, stats)
    return h, dW, dtable


@pytest.mark.parametrize('case', INPUT_CASES, ids=_case_id)
def test_input_fwd_ladder(lib, case):
    N, F, C, De, mode = case
    x, W, table, _, mean, inv_std, _ = input_operands(*case)
    ld_h = C + 3
    bx, bW, bt, bm, bi = _put(x), _put(W), _put(table), _put(mean), _put(inv_std)
    h = Guarded(DEV, F32, N * ld_h)
    nws = lib.ampconv_gcn_input_workspace_bytes(N, F, C)
    ws = Guarded(DEV, U8, nws)
    _ok(lib.ampconv_gcn_input_fwd(bx.ptr, N, F, _p(bm), _p(bi), bW.ptr, _p(bt), De, C, h.ptr, ld_h, ws.ptr, nws, _stream()),
        'ampconv_gcn_input_fwd')
    tag = f'input_fwd {_case_id(case)}'
    assert ws.intact(), f'{tag}: a byte past the workspace was written'
    close(_rows_out(h, N, C, ld_h, tag).cpu().numpy(), input_reference(*case)[0], f'{tag}: h')


@pytest.mark.parametrize('case', INPUT_CASES + BWD_LARGE, ids=_case_id)
def test_input_bwd_ladder(lib, case):
    N, F, C, De, mode = case
    x, W, table, grad, mean, inv_std, fc = input_operands(*case)
    ld_g = C + 1
    bx, bW, bt, bm, bi = _put(x), _put(W), _put(table), _put(mean), _put(inv_std)
    bg = _rows_in(grad, ld_g)
    dW = Guarded(DEV, F32, C * F * (De + 1))
    dtable = Guarded(DEV, F32, F * De) if De else None
    nws = lib.ampconv_gcn_input_workspace_bytes(N, F, C)
    ws = Guarded(DEV, U8, nws)
    _ok(lib.ampconv_gcn_input_bwd(bx.ptr, N, F, _p(bm), _p(bi), bW.ptr, _p(bt), De, C, bg.ptr, ld_g, dW.ptr, _p(dtable),
                                  ws.ptr, nws, _stream()), 'ampconv_gcn_input_bwd')
    tag = f'input_bwd {_case_id(case)}'
    assert ws.intact(), f'{tag}: a byte past the workspace was written'
    _, want_dW, want_dtable = input_reference(*case)
    got = _linear_out(dW, f'{tag}: dW').cpu().numpy().reshape(C, F * (De + 1))
    close(got, want_dW, f'{tag}: gW', scaled=True)                            # a sum over the nodes
    if De:
        close(_linear_out(dtable, f'{tag}: dtable').cpu().numpy().reshape(F, De), want_dtable, f'{tag}: g_table', scaled=True)
    if fc is not None:                      # z is exactly 0 in this column, whatever g holds: no tolerance to hide behind
        assert (got.reshape(C, F, De + 1)[:, fc, De] == 0.0).all(), f'{tag}: dW of the constant column'


# ---- 3. the column sum ------------------------------------------------------------------------------------------------
# colsum_chunks = min(ceil(N / 32), 1024): up to N = 32768 a chunk is at most 32 rows; 32769 -> 33 rows (and chunks past
# the end of g that sum nothing), 70001 -> 69 rows.
COLSUM_CASES = [(N, C) for N in (0, 1, 31, 32, 33) for C in (1, 63, 64, 65, 130)] + \
               [(N, C) for N in (32768, 32769, 70001) for C in (1, 65)]


def test_colsum_cases_pass_the_chunk_cap():
    rows = {N: -(-N // min(max(-(-N // 32), 1), 1024)) for N, _ in COLSUM_CASES}
    assert rows[32768] == 32 and rows[32769] == 33 and rows[70001] == 69 and max(rows[N] for N in (1, 31, 32, 33)) == 32


@pytest.mark.parametrize('N, C', COLSUM_CASES, ids=lambda v: str(v))
def test_colsum(lib, N, C):
    """g = N(0.25, 1): the sum stays near N / 4.  A column of zero-mean values can sum to anything near 0 while its partial
    sums are of order sqrt(N); with C = 1 that one cancelled number would set the scale of its own bar."""
    gen = torch.Generator().manual_seed(77 * N + C)
    g = torch.randn(N, C, generator=gen) + 0.25
    want = R.colsum(g.numpy()) if N else np.zeros(C)
    nws = lib.ampconv_gcn_colsum_workspace_bytes(N, C)
    outs = []
    for ld, repeat in ((C, 2), (C + 3, 1)):
        bg = _rows_in(g, ld)
        for _ in range(repeat):
            out, ws = Guarded(DEV, F32, C), Guarded(DEV, U8, nws)
            _ok(lib.ampconv_gcn_colsum(bg.ptr, ld, N, C, out.ptr, ws.ptr, nws, _stream()), 'ampconv_gcn_colsum')
            assert ws.intact(), f'colsum N={N} C={C} ld={ld}: a byte past the workspace was written'
            outs.append(_linear_out(out, f'colsum N={N} C={C} ld={ld}: out').clone())
    close(outs[0].cpu().numpy(), want, f'colsum N={N} C={C}: out', scaled=True)        # a sum over the nodes
    assert torch.equal(bits(outs[0]), bits(outs[1])), 'two calls differ'
    assert torch.equal(bits(outs[0]), bits(outs[2])), f'ld = {C + 3} differs from ld = {C}: the order is not fixed'
    if N == 0:
        assert bool((bits(outs[0]) == 0).all())
    # Nonzero integers of at most 8: every partial sum is an integer below 2^24, exact in fp32 in whatever order.  The bar
    # above is relative to a sum of order N / 4 and cannot see ONE row left out or added twice at the large N; this can.
    gi = (torch.randint(1, 9, (N, C), generator=gen) * (2 * torch.randint(0, 2, (N, C), generator=gen) - 1)).float()
    bg, out, ws = _rows_in(gi, C + 3), Guarded(DEV, F32, C), Guarded(DEV, U8, nws)
    _ok(lib.ampconv_gcn_colsum(bg.ptr, C + 3, N, C, out.ptr, ws.ptr, nws, _stream()), 'ampconv_gcn_colsum')
    got = _linear_out(out, f'colsum N={N} C={C} integers: out').cpu().numpy().astype(np.float64)
    assert (got == gi.numpy().astype(np.float64).sum(axis=0)).all(), f'colsum N={N} C={C}: a sum of integers is not exact'


# ---- 4. norm and aggregate on a CSR built by hand ---------------------------------------------------------------------
PART_LADDER = (0, 1, LONG - 1, LONG, LONG + 1, PART - 1, PART, PART + 1, 2 * PART - 1, 2 * PART, 2 * PART + 1, 3 * PART + 1)
GRID_N = 4100


@functools.lru_cache(maxsize=None)
def graph(name):
    """(ptr, idx, edge_index) with int32 ptr [N + 1] and idx [E]; the segment lengths are exactly the ones named here.
    'parts': N = 23 (N % 4 == 3); the lengths of PART_LADDER on rows 0..11 -- below, at and past AMPCONV_GCN_LONG_SEGMENT,
    then one to four parts of AMPCONV_GCN_PART entries whose last part holds PART - 1, PART or a single entry -- then 11
    rows of 0..8 entries; neighbours uniform over the OTHER nodes, then about 5 % of the entries made self-loops.
    'grid': 4100 rows of exactly AMPCONV_GCN_LONG_SEGMENT entries, neighbours uniform over all nodes."""
    rng = np.random.default_rng(len(name))
    if name == 'parts':
        lengths = np.array(list(PART_LADDER) + list(rng.integers(0, 9, 11)))
    else:
        lengths = np.full(GRID_N, LONG)
    N = lengths.size
    ptr = np.zeros(N + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(lengths)
    rows = np.repeat(np.arange(N), lengths)
    if name == 'parts':
        idx = (rows + 1 + rng.integers(0, N - 1, rows.size)) % N
        loops = rng.random(rows.size) < 0.05
        idx[loops] = rows[loops]
        assert 0.04 < (idx == rows).mean() < 0.06
    else:
        idx = rng.integers(0, N, rows.size)
    assert (np.diff(ptr) == lengths).all() and idx.min() >= 0 and idx.max() < N
    return ptr, idx.astype(np.int32), np.stack([idx, rows]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def graph_operands(name, C):
    N = graph(name)[0].size - 1
    g = torch.Generator().manual_seed(500 + N + C)
    return torch.randn(N, C, generator=g), torch.randn(C, generator=g)


@functools.lru_cache(maxsize=None)
def graph_reference(name, C, loops, fill, with_bias):
    h, b = graph_operands(name, C)
    ei = graph(name)[2]
    N = h.size(0)
    return (R.gcn_norm(ei, N, fill == 2.0, loops)[3], R.aggregate(h.numpy(), ei, b.numpy() if with_bias else None, fill == 2.0, loops))


def _check_graph(lib, name, C, loops, fill, with_bias):
    ptr, idx, _ = graph(name)
    N, E = ptr.size - 1, idx.size
    h, b = graph_operands(name, C)
    want_dinv, want = graph_reference(name, C, loops, fill, with_bias)
    tag = f'{name} C={C} loops={loops} fill={fill} bias={with_bias}'
    dptr, didx = torch.from_numpy(ptr).to(DEV), torch.from_numpy(idx).to(DEV)
    dinv = Guarded(DEV, F32, N)
    _ok(lib.ampconv_gcn_norm(dptr.data_ptr(), didx.data_ptr(), N, int(loops), fill, dinv.ptr, _stream()), 'ampconv_gcn_norm')
    np.testing.assert_allclose(_linear_out(dinv, f'{tag}: dinv').cpu().numpy(), want_dinv, rtol=2e-7, atol=0)
    bias = _put(b) if with_bias else None
    nws = lib.ampconv_gcn_aggregate_workspace_bytes(N, E, C)
    max_rows, max_parts = E // LONG, E // PART + E // LONG                   # gcn.hip: long_max_rows, long_max_parts
    assert nws == 16 + 8 * max_rows + 8 * max_parts + 4 * max_parts * C
    pad = (C + 3) // 4 * 4 + 4                      # 16-byte path: a multiple of 4 floats, wider than C, base aligned

    def run(ld, offset, with_ws, what):
        bh = _rows_in(h, ld, offset)
        out = Guarded(DEV, F32, N * ld, offset)
        ws = Guarded(DEV, U8, nws) if with_ws else None
        _ok(lib.ampconv_gcn_aggregate(bh.ptr, ld, C, dptr.data_ptr(), didx.data_ptr(), dinv.ptr, int(loops), fill, _p(bias),
                                      out.ptr, ld, N, E, _p(ws), nws if with_ws else 0, _stream()), 'ampconv_gcn_aggregate')
        assert ws is None or ws.intact(), f'{tag} {what}: a byte past the workspace was written'
        got = _rows_out(out, N, C, ld, f'{tag} {what}').clone()
        close(got.cpu().numpy(), want, f'{tag} {what}: out')
        return got

    out16 = run(pad, 0, True, '16-byte loads')
    out4 = run(C + 3, 4, True, '4-byte loads')     # C = 1, 5, 17, 65: ld % 4 == 0, the offset alone rules the 16-byte path out
    assert torch.equal(bits(out16), bits(out4)), f'{tag}: the two load widths differ'
    run(pad, 0, False, 'no workspace')              # every segment walked by its lane group
    return max_rows, max_parts


VARIANTS = ((True, 1.0, True), (True, 2.0, False), (False, 1.0, True))      # add_self_loops, fill, bias


@pytest.mark.parametrize('loops, fill, with_bias', VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize('C', (1, 4, 5, 17, 64, 65))
def test_norm_and_aggregate_on_the_part_ladder(lib, C, loops, fill, with_bias):
    assert _lib.GCN_PART == PART and _lib.GCN_LONG_SEGMENT == LONG
    lengths = np.diff(graph('parts')[0])
    assert lengths.size == 23 and tuple(lengths[:12]) == PART_LADDER and lengths[12:].max() <= 8
    assert [-(-n // PART) for n in PART_LADDER[5:]] == [1, 1, 2, 2, 2, 3, 4] and PART_LADDER[-1] % PART == 1
    _check_graph(lib, 'parts', C, loops, fill, with_bias)


@pytest.mark.parametrize('C, loops, fill, with_bias', ((4, True, 1.0, True), (5, False, 1.0, False)), ids=lambda v: str(v))
def test_aggregate_beyond_one_wave_of_workgroups(lib, C, loops, fill, with_bias):
    """4100 long rows of one part each: gcn_long_parts_kernel runs on min(max_parts, 4096) workgroups and
    gcn_long_combine_kernel on min(max_rows, 1024), so both grid-stride loops take further trips."""
    assert _lib.GCN_PART == PART and (np.diff(graph('grid')[0]) == LONG).all()
    max_rows, max_parts = _check_graph(lib, 'grid', C, loops, fill, with_bias)
    assert GRID_N > min(max_parts, 4096) and GRID_N > min(max_rows, 1024)     # the launch bounds of ampconv_gcn_aggregate


# ---- 5. what the header promises to refuse ----------------------------------------------------------------------------
def test_argument_checks(lib):
    """Expected codes: include/ampconv.h, GCN baseline, ERRORS.  Every call below has valid buffers of full size behind its
    pointers, so a call that is wrongly accepted computes into them and the test fails on its return code alone."""
    st = _stream()
    N, F, C, De = 4, 3, 2, 1
    z = lambda *s: torch.zeros(*s, device=DEV)
    x, mean, inv_std, W, table, g = z(N, F), z(F), torch.ones(F, device=DEV), z(C, F * (De + 1)), z(F, De), z(N, C)
    W0 = z(C, F)
    h, dW, dtable = Guarded(DEV, F32, N * C), Guarded(DEV, F32, C * F * (De + 1)), Guarded(DEV, F32, F * De)
    dW0 = Guarded(DEV, F32, C * F)
    nin = lib.ampconv_gcn_input_workspace_bytes(N, F, C)
    assert nin > 0 and nin % 16 == 0
    win = torch.empty(nin + 16, dtype=U8, device=DEV)
    assert win.data_ptr() % 16 == 0
    P = lambda t: t.data_ptr()

    def fwd(ld_h=C, ws=P(win), nws=nin, tab=P(table), de=De, w=P(W), n=N):
        return lib.ampconv_gcn_input_fwd(P(x), n, F, P(mean), P(inv_std), w, tab, de, C, h.ptr, ld_h, ws, nws, st)

    def bwd(ld_g=C, ws=P(win), nws=nin, tab=P(table), de=De, w=P(W), dw=dW.ptr, dt=dtable.ptr):
        return lib.ampconv_gcn_input_bwd(P(x), N, F, P(mean), P(inv_std), w, tab, de, C, P(g), ld_g, dw, dt, ws, nws, st)

    assert fwd(ld_h=C - 1) == E_BADARG and bwd(ld_g=C - 1) == E_BADARG
    assert fwd(ws=P(win) + 4) == E_WORKSPACE and bwd(ws=P(win) + 4) == E_WORKSPACE         # not 16-byte aligned
    assert fwd(nws=nin - 1) == E_WORKSPACE and bwd(nws=nin - 1) == E_WORKSPACE
    assert bwd(dt=None) == E_BADARG                                                       # De > 0 without dtable
    assert fwd(tab=P(table), de=0, w=P(W0)) == E_BADARG                                   # De == 0 with a table
    assert bwd(tab=P(table), de=0, w=P(W0), dw=dW0.ptr, dt=None) == E_BADARG
    assert fwd(n=0) == OK                                                                 # N == 0 succeeds

    # the aggregate: two rows, the first one long (entries: node 0), so that the workspace is looked at
    E = LONG
    ptr = torch.tensor([0, E, E], dtype=torch.int32, device=DEV)
    idx = torch.zeros(E, dtype=torch.int32, device=DEV)
    hh, dinv = z(2, 4), torch.ones(2, device=DEV)
    out = Guarded(DEV, F32, 2 * 4)
    nag = lib.ampconv_gcn_aggregate_workspace_bytes(2, E, 4)
    assert nag > 0
    wag = torch.empty(nag + 16, dtype=U8, device=DEV)

    def agg(ld_h=4, ld_out=4, ws=P(wag), nws=nag, n=2):
        return lib.ampconv_gcn_aggregate(P(hh), ld_h, 4, P(ptr), P(idx), P(dinv), 1, 1.0, None, out.ptr, ld_out, n, E, ws, nws, st)

    assert agg(ld_h=3) == E_BADARG and agg(ld_out=3) == E_BADARG
    assert agg(ws=P(wag) + 4) == E_WORKSPACE and agg(nws=nag - 1) == E_WORKSPACE
    assert agg(n=0) == OK

    # the column sum
    ncs = lib.ampconv_gcn_colsum_workspace_bytes(N, C)
    assert ncs > 0
    wcs = torch.empty(ncs, dtype=U8, device=DEV)
    cs = Guarded(DEV, F32, C)
    assert lib.ampconv_gcn_colsum(P(g), C - 1, N, C, cs.ptr, P(wcs), ncs, st) == E_BADARG
    assert lib.ampconv_gcn_colsum(P(g), C, N, C, cs.ptr, P(wcs), ncs - 1, st) == E_WORKSPACE

    # the norm
    dn = Guarded(DEV, F32, 2)
    for fill in (-1.0, float('nan')):
        assert lib.ampconv_gcn_norm(P(ptr), P(idx), 2, 1, fill, dn.ptr, st) == E_BADARG
    assert lib.ampconv_gcn_norm(P(ptr), P(idx), 0, 1, 1.0, dn.ptr, st) == OK

    torch.cuda.synchronize()
    for name, buf in (('h', h), ('dW', dW), ('dtable', dtable), ('dW (De = 0)', dW0), ('out', out), ('colsum', cs),
                      ('dinv', dn)):
        assert _untouched(buf), f'{name} was written by a refused call or one with N = 0'
