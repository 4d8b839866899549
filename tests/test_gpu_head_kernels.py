"""csrc/head.hip one library call at a time (ampnet_amd._lib, no Python wrapper in between) against the numpy fp64 model
of tests/head_reference.py, on ladders derived from the kernels' own constants.

test_gpu_head.py runs the models' shapes through the autograd wrappers; here every geometry that `make_geom` and
`dispatch` of head.hip can yield is entered on purpose -- the group width G, the number of `p0` passes of the backward,
the number of kCT class chunks, W in LDS or in global memory (separately for forward and backward, whose LDS layouts
differ by `red_floats`), the 16-byte and the element-wise path -- and the test's id names it.  `_geom` below mirrors that
arithmetic; every case first asserts that the mirror puts it where its id says.  The path is steered as a caller would
steer it: by D, by the row stride and by the alignment of the base (a view 4 resp. 2 bytes into an allocation).

Every case runs ampconv_head_fwd and ampconv_head_bwd (log_softmax and sigmoid), ampconv_head_nll_fwd (node weights, 4
masks and logp; and none of the three) and ampconv_head_nll_bwd (the same two, the second with dpooled = NULL; and a
gradient mask that selects no row).  Labels include -100 (skipped), C and -3 (counted in bad_labels, never used as an
index).  Every tensor lies between guard bands (tests/site_guards.py), the gaps of a strided pooled hold NaN, the
workspace is exactly ampconv_head_workspace_bytes long; every backward is launched twice and must give the same bits.
Tolerances: out, logp and fp32 dpooled at the project's flat atol 1e-5, rtol 1e-4; dW and db under the labels gW, gb, i.e.
the scaled bar; the loss sums scaled likewise (sums over N rows, as in test_gpu_head.py); bf16 dpooled atol = rtol = 2e-2;
count, correct and bad_labels exact.  For `correct` every case asserts on the CPU that the two largest fp64 logits of
every counted row differ by at least 1e-5; the case's seed is the first for which that holds."""
import functools
import types

import numpy as np
import pytest
import torch

import head_reference as ref
from site_guards import BF16_TOL, MISALIGN, TORCH_DTYPE, Guarded, bits, close, header_constant

pytestmark = pytest.mark.gpu

MAX_CLASSES = header_constant('AMPCONV_HEAD_MAX_CLASSES')
MAX_MASKS = header_constant('AMPCONV_HEAD_MAX_MASKS')
SLOTS = header_constant('AMPCONV_HEAD_METRICS_SLOTS')
SHIFT = header_constant('AMPCONV_HEAD_LOSS_SHIFT')
IGNORE = header_constant('AMPCONV_HEAD_IGNORE_INDEX')
THREADS = 256                                   # csrc/head.hip:29   kThreads
K_CT = 8                                        # csrc/head.hip:30   kCT
K_MAX_BLOCKS = 1024                             # csrc/head.hip:31   kMaxBlocks
LDS_BYTES = 64 * 1024                           # csrc/head.hip:32   kLdsBytes
NPV = {'f32': 4, 'bf16': 8}
CODE = {'f32': 0, 'bf16': 1}
KINDS = {'log_softmax': 0, 'sigmoid': 1}
GAP = 1e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from ampnet_amd import _lib
    return _lib.load()


def _call(lib, name, *args):
    rc = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)


def _f64(t):
    return t.float().numpy().astype(np.float64)


# ---- the mirror of head.hip's dispatch arithmetic ----------------------------------------------------------------------
def _up4(n):
    return (n + 3) & ~3


def _geom(N, D, C, dtype, stride=None, aligned=True, bwd=False):
    """dispatch + make_geom + lds_bytes + grid_of."""
    stride = D if stride is None else stride
    vec = aligned and D % NPV[dtype] == 0 and stride % NPV[dtype] == 0
    NP = NPV[dtype] if vec else 1
    P, G = D // NP, 4
    while G < P and G < 64:
        G <<= 1
    R = THREADS // G
    tiles = -(-N // R)
    red = G * K_CT * NP + K_CT if bwd else 0
    rest = (_up4(C) + _up4(R * C) + red) * 4
    w_floats = _up4(C * D)
    wlds = rest + w_floats * 4 <= LDS_BYTES
    return types.SimpleNamespace(vec=vec, NP=NP, P=P, G=G, R=R, tiles=tiles, wlds=wlds, passes=-(-P // G), chunks=-(-C // K_CT),
                                 lds=rest + (w_floats * 4 if wlds else 0), blocks=min(tiles, K_MAX_BLOCKS))


def _home(wlds):
    return 'lds' if wlds else 'global'


def _case_id(dtype, D, C, stride=None, offset=0):
    f, b = _geom(9, D, C, dtype, stride, offset == 0), _geom(9, D, C, dtype, stride, offset == 0, bwd=True)
    return (f'{dtype}_D{D}_C{C}_{"vec" if f.vec else "elem"}_G{f.G}_pass{f.passes}_chunk{f.chunks}_W{_home(f.wlds)}fwd_W{_home(b.wlds)}bwd'
            + ('_unaligned' if offset else '') + (f'_stride{stride}' if stride else ''))


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _counted_gap(pooled, W, b, y, masks, C):
    """The smallest distance between the two largest fp64 logits over the rows that some mask counts."""
    if C == 1:
        return np.inf
    used, _ = ref.selection(y.numpy(), masks.numpy(), C)
    z = np.sort(ref.logits(_f64(pooled), W.numpy(), b.numpy())[used.any(axis=0)], axis=1)
    return float((z[:, -1] - z[:, -2]).min()) if z.size else np.inf


@functools.lru_cache(maxsize=4)
def _inputs(N, D, C, dtype):
    """pooled in the storage dtype, W, b, labels with one -100, one C and one -3 (rows 1, 2, 4, each selected by mask 0),
    node weights, four masks of which the last selects nothing, dout: the first seed that keeps `correct` away from ties."""
    for seed in range(64):
        pooled, W, b, y, w, two = ref.make_inputs(N, D, C, seed)
        pooled = pooled.to(TORCH_DTYPE[dtype])
        g = torch.Generator().manual_seed(seed + N)
        masks = torch.cat([two, torch.rand(1, N, generator=g) < 0.3, torch.zeros(1, N, dtype=torch.bool)]).to(torch.uint8)
        y = y.clone()
        if N >= 8:
            y[1], y[2], y[4] = IGNORE, C, -3
            masks[0, [1, 2, 4]] = 1
        dout = torch.randn(N, C, generator=g)
        if _counted_gap(pooled, W, b, y, masks, C) >= GAP:
            return pooled, W, b, y, w, masks, dout
    raise AssertionError('no seed keeps the counted rows away from argmax ties')


def _metrics(buf):
    m = buf.np().astype(np.int64)
    return {'loss_sum': [float(m[3 * i]) / 2.0 ** SHIFT for i in range(MAX_MASKS)], 'count': [int(m[3 * i + 1]) for i in range(MAX_MASKS)],
            'correct': [int(m[3 * i + 2]) for i in range(MAX_MASKS)], 'bad_labels': int(m[SLOTS - 1])}


def _check_case(lib, dev, N, D, C, dtype, offset=0, stride=None):
    tdt, code = TORCH_DTYPE[dtype], CODE[dtype]
    stride_ = D if stride is None else stride
    pooled, W, b, y, w, masks, dout = _inputs(N, D, C, dtype)
    assert _counted_gap(pooled, W, b, y, masks, C) >= GAP           # on the CPU, before any kernel output
    M = masks.shape[0]
    assert M == MAX_MASKS
    pn, Wn, bn, yn, wn, mn = _f64(pooled), W.numpy(), b.numpy(), y.numpy(), w.numpy(), masks.numpy()
    tol = BF16_TOL if dtype == 'bf16' else {}

    X = Guarded(dev, tdt, (N - 1) * stride_ + D, offset)           # the gaps between strided rows stay NaN
    X.t.as_strided((N, D), (stride_, 1)).copy_(pooled)
    Wg, Bg, DOUT = Guarded.of(dev, W), Guarded.of(dev, b), Guarded.of(dev, dout)
    Yg, WN, MASKS = Guarded.of(dev, y), Guarded.of(dev, w), Guarded.of(dev, masks)
    OUT = Guarded(dev, torch.float32, N * C)
    DP, DW, DB = Guarded(dev, tdt, N * D, offset), Guarded(dev, torch.float32, C * D), Guarded(dev, torch.float32, C)
    need = lib.ampconv_head_workspace_bytes(N, D, C)
    assert need == min(-(-N // 4), K_MAX_BLOCKS) * C * (D + 1) * 4
    WS = Guarded(dev, torch.uint8, need)
    head = (X.ptr, N, D, stride_, Wg.ptr)
    inputs = (X, Wg, Bg, DOUT, Yg, WN, MASKS)

    def backward(name, args, want, label, dpooled=True):
        runs = []
        for _ in range(2):
            DP.refill(), DW.refill(), DB.refill(), WS.refill()
            _call(lib, name, *args, DP.ptr if dpooled else None, DW.ptr, DB.ptr, WS.ptr, need, code, None)
            assert DP.intact() and DW.intact() and DB.intact() and WS.intact() and DW.written() and DB.written(), label
            if dpooled:
                assert DP.written(), label
                close(DP.np(N, D), want[0], 'dpooled ' + label, **tol)
            else:
                assert bool((DP.backing == 0xFF).all()), label     # NULL: nothing written anywhere
            close(DW.np(C, D), want[1], 'gW ' + label)
            close(DB.np(), want[2], 'gb ' + label)
            runs.append([bits(t.t).clone() for t in (DP, DW, DB)])
        for first, second in zip(*runs):
            assert torch.equal(first, second), label + ': two launches, different bits'

    # the plain head, both kinds; the backward from the SAVED output of the forward
    for kind, k in KINDS.items():
        OUT.refill()
        _call(lib, 'ampconv_head_fwd', *head, Bg.ptr, C, k, OUT.ptr, code, None)
        assert OUT.intact() and OUT.written(), kind
        want_out = ref.head_fwd(pn, Wn, bn, kind)
        close(OUT.np(N, C), want_out, f'out {kind}')
        if C == 1 and kind == 'log_softmax':
            assert bool((OUT.t == 0).all())
        backward('ampconv_head_bwd', (*head, C, k, DOUT.ptr, OUT.ptr), ref.head_bwd(pn, Wn, dout.numpy(), want_out, kind), kind)

    # the loss: with node weights, 4 masks and logp; then with none of them
    METRICS, SCRATCH, LOSS = Guarded(dev, torch.int64, SLOTS), Guarded(dev, torch.int64, SLOTS), Guarded(dev, torch.float32, 1)
    gm = 2
    for what, (w_ptr, m_ptr, masks_n, M_, gm_, logp) in {'weights masks logp': (WN.ptr, MASKS.ptr, mn, M, gm, True),
                                                         'bare': (None, None, None, 1, 0, False)}.items():
        OUT.refill(), SCRATCH.refill(), LOSS.refill()
        METRICS.t.zero_()
        _call(lib, 'ampconv_head_nll_fwd', *head, Bg.ptr, C, Yg.ptr, w_ptr, m_ptr, M_, gm_, OUT.ptr if logp else None,
              METRICS.ptr, SCRATCH.ptr, LOSS.ptr, code, None)
        assert OUT.intact() and METRICS.intact() and SCRATCH.intact() and LOSS.intact() and LOSS.written(), what
        want = ref.nll_fwd(pn, Wn, bn, yn, wn if w_ptr else None, masks_n)
        got = _metrics(METRICS)
        assert torch.equal(METRICS.t, SCRATCH.t), what             # the call's own sums, added to a zeroed buffer
        # the loss and loss_sum are sums over N rows: scaled like the parameter gradients
        close(LOSS.np()[0], want['loss_sum'][gm_], f'loss {what}', scaled=True)
        close(got['loss_sum'][:M_], want['loss_sum'], f'loss_sum {what}', scaled=True)
        assert got['count'][:M_] == want['count'] and got['correct'][:M_] == want['correct'], what
        assert got['bad_labels'] == want['bad_labels'] == (2 if N >= 8 else 0), what
        assert all(v == 0 for key in ('loss_sum', 'count', 'correct') for v in got[key][M_:]), what
        if logp:
            assert OUT.written(), what
            close(OUT.np(N, C), want['logp'], f'logp {what}')
        else:
            assert bool((OUT.backing == 0xFF).all()), what

    G15 = Guarded.of(dev, torch.tensor([1.5]))
    nll = (*head, Bg.ptr, C, Yg.ptr)
    backward('ampconv_head_nll_bwd', (*nll, WN.ptr, MASKS.ptr, M, gm, G15.ptr), ref.nll_bwd(pn, Wn, bn, yn, wn, mn, gm, 1.5),
             f'loss of mask {gm}')
    backward('ampconv_head_nll_bwd', (*nll, None, None, 1, 0, G15.ptr), ref.nll_bwd(pn, Wn, bn, yn, None, None, 0, 1.5),
             'bare loss', dpooled=False)
    # a gradient mask that selects no row: exact zeros everywhere
    backward('ampconv_head_nll_bwd', (*nll, WN.ptr, MASKS.ptr, M, M - 1, G15.ptr),
             (np.zeros((N, D)), np.zeros((C, D)), np.zeros(C)), 'empty mask')
    for t in (DP, DW, DB):
        assert bool((bits(t.t) == 0).all())
    assert all(t.intact() for t in inputs) and G15.intact()


# ---- the width ladder --------------------------------------------------------------------------------------------------
# (dtype, D, base offset, row stride or None) -> (vec, G, p0 passes of the backward)
WIDTHS = {
    **{('f32', D, 0, None): (True, G, n) for D, G, n in ((4, 4, 1), (16, 4, 1), (20, 8, 1), (64, 16, 1), (100, 32, 1), (128, 32, 1),
                                                       (132, 64, 1), (256, 64, 1), (260, 64, 2), (512, 64, 2), (1024, 64, 4))},
    **{('bf16', D, 0, None): (True, G, n) for D, G, n in ((8, 4, 1), (64, 8, 1), (264, 64, 1), (512, 64, 1), (520, 64, 2), (1024, 64, 2))},
    **{('f32', D, 0, None): (False, G, n) for D, G, n in ((1, 4, 1), (3, 4, 1), (63, 64, 1), (65, 64, 2), (130, 64, 3))},
    ('f32', 64, MISALIGN['f32'], None): (False, 64, 1),
    ('f32', 100, MISALIGN['f32'], None): (False, 64, 2),
    ('bf16', 100, 0, None): (False, 64, 2),                        # 100 bf16 channels are no whole pieces
    ('bf16', 64, MISALIGN['bf16'], None): (False, 64, 1),
    ('f32', 128, 0, 129): (False, 64, 2),                          # whole pieces, but every other row starts off a boundary
    ('f32', 128, 0, 160): (True, 32, 1),                           # a strided view that keeps the pieces
}


@pytest.mark.parametrize('key', list(WIDTHS), ids=lambda k: _case_id(k[0], k[1], 7, k[3], k[2]))
def test_width_ladder(key, lib, dev):
    """C = 7 (one chunk), N = two tiles and a row.  The widths are both sides of every step of G, and of the number of
    `p0` passes of the backward: 256 | 260 fp32 (the second pass has one live lane), 512 (two full passes), 1024 (four);
    bf16 512 | 520; element-wise 63 | 64 | 65 and 130 (three passes, the last with two live lanes); D = 64 and 100 reach the
    element-wise kernels through the base alone, D = 128 through a row stride of 129."""
    dtype, D, offset, stride = key
    vec, G, passes = WIDTHS[key]
    q = _geom(9, D, 7, dtype, stride, offset == 0, bwd=True)
    assert (q.vec, q.G, q.passes, q.chunks) == (vec, G, passes, 1), q
    N = 2 * q.R + 1
    assert _geom(N, D, 7, dtype, stride, offset == 0).blocks == 3
    _check_case(lib, dev, N, D, 7, dtype, offset, stride)


# ---- classes -----------------------------------------------------------------------------------------------------------
CLASSES = [1, 7, K_CT, K_CT + 1, 2 * K_CT, 2 * K_CT + 1, MAX_CLASSES - 1, MAX_CLASSES]


@pytest.mark.parametrize('C', CLASSES, ids=lambda C: _case_id('f32', 260, C))
def test_class_ladder_with_two_row_passes(C, lib, dev):
    """D = 260 fp32 needs two `p0` passes, so with C = 9 and 17 both loops of the backward turn at once; C = 8 | 9 and
    16 | 17 are both sides of a chunk, 63 | 64 a ragged and a full last chunk at the class limit.  Up to C = 17 W is staged
    in LDS: more than one chunk together with WLDS, which the models' shapes never reach."""
    q = _geom(9, 260, C, 'f32', bwd=True)
    assert (q.vec, q.passes, q.chunks) == (True, 2, -(-C // K_CT)) and q.wlds == (C <= 2 * K_CT + 1)
    _check_case(lib, dev, 2 * q.R + 1, 260, C, 'f32')


@pytest.mark.parametrize('dtype,D,C', [('f32', 3, 9), ('bf16', 520, 17), ('f32', 4, MAX_CLASSES)], ids=lambda v: str(v))
def test_class_chunks_on_other_paths(dtype, D, C, lib, dev):
    """Several chunks element-wise (D = 3), in bf16 with two passes, and the widest scratch: G = 4, R = 64, C = 64."""
    q = _geom(9, D, C, dtype, bwd=True)
    assert q.chunks > 1 and q.wlds
    _check_case(lib, dev, 2 * q.R + 1, D, C, dtype)


# ---- the home of W -----------------------------------------------------------------------------------------------------
def _largest_lds_C(D, dtype, bwd):
    return max(C for C in range(1, MAX_CLASSES + 1) if _geom(9, D, C, dtype, bwd=bwd).wlds)


def _home_cases():
    D = 256
    cf, cb = _largest_lds_C(D, 'f32', False), _largest_lds_C(D, 'f32', True)
    assert cb < cf < MAX_CLASSES                                 # the backward's red_floats push W out of LDS sooner
    return [('f32', D, cb), ('f32', D, cb + 1), ('f32', D, cf), ('f32', D, cf + 1)]


@pytest.mark.parametrize('dtype,D,C', _home_cases(), ids=[_case_id(*c) for c in _home_cases()])
def test_home_of_W(dtype, D, C, lib, dev):
    """At D = 256 fp32: the largest C whose backward layout still fits 64 KiB and the next one (forward stages W in LDS,
    backward reads it from global memory), then the largest C whose forward layout fits and the next one."""
    f, b = _geom(9, D, C, dtype), _geom(9, D, C, dtype, bwd=True)
    assert f.lds <= LDS_BYTES and b.lds <= LDS_BYTES
    cf, cb = _largest_lds_C(D, dtype, False), _largest_lds_C(D, dtype, True)
    assert f.wlds == (C <= cf) and b.wlds == (C <= cb)
    _check_case(lib, dev, 2 * f.R + 1, D, C, dtype)


# ---- rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D', [('f32', 4), ('f32', 256), ('f32', 3), ('bf16', 64)], ids=lambda v: str(v))
def test_row_ladder(dtype, D, lib, dev):
    """N = 1, R - 1, R, R + 1 with R = 256 / G rows per tile: G = 4 (R = 64), G = 64 (R = 4), element-wise D = 3, bf16."""
    R = _geom(1, D, 7, dtype).R
    for N in (1, R - 1, R, R + 1):
        assert _geom(N, D, 7, dtype).blocks == (2 if N > R else 1)
        _check_case(lib, dev, N, D, 7, dtype)


def test_grid_stride_at_the_narrowest_row(lib, dev):
    """D = 4: G = 4, R = 64, so N = 1024 * 64 + 3 rows are 1025 tiles on 1024 workgroups: workgroup 0 takes a second tile of
    three rows.  The other end from test_gpu_head.py's (20011, 256, 64), where R = 4."""
    N, D, C = K_MAX_BLOCKS * 64 + 3, 4, 7
    q = _geom(N, D, C, 'f32', bwd=True)
    assert (q.R, q.tiles, q.blocks) == (64, K_MAX_BLOCKS + 1, K_MAX_BLOCKS)
    _check_case(lib, dev, N, D, C, 'f32')
