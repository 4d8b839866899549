"""csrc/glue.hip one library call at a time (ampnet_amd._lib, no Python wrapper in between) against the numpy fp64 model
of tests/glue_reference.py, on ladders that are derived from the kernels' own constants.

test_gpu_glue.py runs the models' shapes through the autograd wrappers; here every path that the launch code of glue.hip
can take is entered on purpose, and the test's id names it.  The path is steered as a caller would steer it: by the
alignment of the base (a view 4 resp. 2 bytes into an allocation) and by the element count, never by an environment
knob.  `_elementwise_plan` and `_pool_plan` below mirror the dispatch arithmetic of glue.hip; every case first asserts
that the mirror puts it on the path its id names.

Every tensor the library touches lies between guard bands (tests/site_guards.py); after every call the bands must be
intact and every output element written.
Tolerances: fp32 the project's flat atol 1e-5, rtol 1e-4; bf16 storage atol = rtol = 2e-2, as in test_gpu_glue.py.
ReLU's kink: the pre-activation is the stored input itself, and `draw` keeps it at least 1e-3 away from 0."""
import functools
import types

import numpy as np
import pytest
import torch

import glue_reference as ref
from site_guards import MISALIGN, TOL, TORCH_DTYPE, Guarded, bits, close, draw

pytestmark = pytest.mark.gpu

K_UNROLL = 4                                    # csrc/glue.hip:17   kUnroll
K_MAX_BLOCKS = 2048                             # csrc/glue.hip:18   kMaxBlocks
THREADS = 256                                   # the launch bounds of every kernel of glue.hip
TILE = THREADS * K_UNROLL                       # pieces per workgroup and trip of act_dropout_{fwd,bwd}_vec
ACT = {'identity': 0, 'relu': 1, 'elu': 2}
POOLING = {'mean': 0, 'token0': 1}
SEED = 0x1234567890ABCDEF
PS = [0.0, 0.1, 0.6]
NP = {'f32': 4, 'bf16': 8}                      # elements of a 16-byte piece
CODE = {'f32': 0, 'bf16': 1}


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


# ---- the mirror of glue.hip's launch arithmetic ------------------------------------------------------------------------
def _elementwise_plan(n, dtype, aligned):
    """ampconv_act_dropout_{fwd,bwd}: 16-byte pieces iff every base is aligned and n is whole pieces; capped_blocks."""
    vec = aligned and n % NP[dtype] == 0
    units, per = (n // NP[dtype], TILE) if vec else (n, THREADS)
    blocks = min(-(-units // per), K_MAX_BLOCKS)
    trips = -(-units // (blocks * per))
    return types.SimpleNamespace(vec=vec, units=units, blocks=blocks, trips=trips,
                                 last_trip=units - (trips - 1) * blocks * per)          # units left for the last trip


def _pool_plan(N, D, dtype, aligned):
    """ampconv_pool_{fwd,bwd}: a lane per (node, piece) resp. (node, channel); pool_grid."""
    vec = aligned and D % NP[dtype] == 0
    per_node = D // NP[dtype] if vec else D
    return types.SimpleNamespace(vec=vec, per_node=per_node, units=N * per_node, blocks=-(-N * per_node // THREADS))


LARGEST = (K_MAX_BLOCKS * TILE + TILE + 7) * NP['bf16']       # elements of the top of the ladder


@functools.lru_cache(maxsize=2)
def _fields(n):
    """THE MASK's 16-bit fields of the first n flat indices under SEED: a shorter tensor's are a prefix of them."""
    return ref.fields(SEED, n).astype(np.uint16)


def _keep(p, shape):
    n = int(np.prod(shape))
    big = _fields(LARGEST if n > 1 << 20 else 1 << 20)
    return (big[:n] >= ref.mask_params(p)[0]).reshape(shape)


def _mask_args(p):
    thr, scale = ref.mask_params(p)
    return SEED, thr, float(scale)


@functools.lru_cache(maxsize=2)
def _drawn(n, dtype):
    g = torch.Generator().manual_seed(7 * n + len(dtype))
    return draw(g, dtype, n), draw(g, dtype, n)


def _flat_inputs(n, dtype):
    """x and dy of n elements; the multi-million-element cases of a dtype share one draw and take prefixes of it."""
    if n <= 1 << 20:
        return _drawn(n, dtype)
    x, dy = _drawn(LARGEST // NP['bf16'] * NP[dtype], dtype)
    return x[:n], dy[:n]


def _act_dropout_case(lib, dev, n, dtype, offset, combos):
    """fwd, then bwd from the SAVED OUTPUT of that fwd (the contract of include/ampconv.h: ReLU and ELU take their slope
    from y / scale; the identity is handed y = NULL), for every (activation, p) of `combos`."""
    x, dy = _flat_inputs(n, dtype)
    X, DY = Guarded.of(dev, x, offset), Guarded.of(dev, dy, offset)
    Y, DX = Guarded(dev, x.dtype, n, offset), Guarded(dev, x.dtype, n, offset)
    xn, dyn = _f64(x), _f64(dy)
    for a, p in combos:
        keep = _keep(p, (n,))
        label = f'{a} p={p}'
        Y.refill(), DX.refill()
        _call(lib, 'ampconv_act_dropout_fwd', X.ptr, n, ACT[a], *_mask_args(p), Y.ptr, CODE[dtype], None)
        assert Y.intact() and Y.written(), label
        got = Y.np()
        close(got, ref.act_dropout_fwd(xn, a, SEED, p, keep), 'y ' + label, **TOL[dtype])
        if a == 'identity':                                      # the inputs hold no zero: the zeros of y ARE the mask
            assert np.array_equal(got != 0, keep), label
        _call(lib, 'ampconv_act_dropout_bwd', DY.ptr, None if a == 'identity' else Y.ptr, n, ACT[a], *_mask_args(p),
              DX.ptr, CODE[dtype], None)
        assert DX.intact() and DX.written() and Y.intact(), label
        want = ref.act_dropout_bwd(xn, dyn, a, SEED, p, keep)
        got = DX.np()
        close(got, want, 'dx ' + label, **TOL[dtype])
        assert np.array_equal(got != 0, want != 0), label
    assert X.intact() and DY.intact()


ALL = [(a, p) for a in ACT for p in PS]
LARGE = [('identity', 0.6), ('elu', 0.1)]       # the multi-million-element cases: no ReLU, and one of these two each

# pieces, workgroups, trips of the grid-stride loop, what the last trip holds
VEC_LADDER = [
    (1, 1, 1, 'partial'),
    (TILE - 1, 1, 1, 'partial'),
    (TILE, 1, 1, 'full'),
    (TILE + 1, 2, 1, 'full+partial'),
    (K_MAX_BLOCKS * TILE, K_MAX_BLOCKS, 1, 'full'),
    (K_MAX_BLOCKS * TILE + 1, K_MAX_BLOCKS, 2, 'partial'),
    (K_MAX_BLOCKS * TILE + TILE + 7, K_MAX_BLOCKS, 2, 'full+partial'),
]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('pieces,blocks,trips,last', VEC_LADDER,
                         ids=[f'vec_pieces{q}_wg{b}_trip{t}_{w}' for q, b, t, w in VEC_LADDER])
def test_act_dropout_16_byte_path(pieces, blocks, trips, last, dtype, lib, dev):
    """act_dropout_{fwd,bwd}_vec.  1, TILE - 1: only the partial-tile branch; TILE: only the unrolled one; TILE + 1: a
    second workgroup; kMaxBlocks tiles: the full grid, one trip each; one piece more: workgroup 0 comes round again for a
    partial tile; a tile and 7 pieces more: a full tile on the second trip (workgroup 0) and a partial one (workgroup 1)."""
    plan = _elementwise_plan(pieces * NP[dtype], dtype, aligned=True)
    assert plan.vec and (plan.units, plan.blocks, plan.trips) == (pieces, blocks, trips)
    full, part = divmod(plan.last_trip if trips > 1 else pieces, TILE)
    assert last == '+'.join(w for w, there in (('full', full), ('partial', part)) if there)
    rung = [q for q, _, _, _ in VEC_LADDER].index(pieces) + (dtype == 'bf16')       # both of LARGE at every size, over the dtypes
    _act_dropout_case(lib, dev, pieces * NP[dtype], dtype, 0, LARGE[rung % 2:][:1] if pieces > TILE + 1 else ALL)


SCALAR_LADDER = [(1, 1, 1), (THREADS - 1, 1, 1), (THREADS, 1, 1), (THREADS + 1, 2, 1), (K_MAX_BLOCKS * THREADS + 3, K_MAX_BLOCKS, 2)]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('n,blocks,trips', SCALAR_LADDER, ids=[f'scalar_unaligned_n{n}_wg{b}_trip{t}' for n, b, t in SCALAR_LADDER])
def test_act_dropout_element_wise_path_by_base(n, blocks, trips, dtype, lib, dev):
    """act_dropout_{fwd,bwd}_scalar behind a base that is 4 (fp32) resp. 2 (bf16) bytes off: both sides of one workgroup,
    and 3 elements past the full grid, i.e. the grid stride of the scalar kernels."""
    plan = _elementwise_plan(n, dtype, aligned=False)
    assert not plan.vec and (plan.blocks, plan.trips) == (blocks, trips)
    _act_dropout_case(lib, dev, n, dtype, MISALIGN[dtype], LARGE if n > 4 * THREADS else ALL)      # half a million elements: both


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_act_dropout_element_wise_path_by_length(dtype, lib, dev):
    """An aligned base whose n is one element more than whole pieces: scalar_aligned, two workgroups."""
    n = NP[dtype] * THREADS // 4 + 1
    plan = _elementwise_plan(n, dtype, aligned=True)
    assert not plan.vec and plan.blocks == -(-n // THREADS) > 1
    _act_dropout_case(lib, dev, n, dtype, 0, ALL)


@pytest.mark.parametrize('p', [0.1, 0.6])
def test_mask_is_the_same_bits_on_every_path(p, lib, dev):
    """One logical tensor of TILE + 1 pieces through the 16-byte and the element-wise kernels, in fp32 and in bf16: the
    zeros of the four outputs are the same elements, those of glue_reference.keep_mask."""
    n = (TILE + 1) * NP['bf16']
    keep = ref.keep_mask(SEED, ref.mask_params(p)[0], (n,))
    x32 = _flat_inputs(n, 'bf16')[0].float()                     # exactly representable in both storages
    for dtype in ('f32', 'bf16'):
        for offset in (0, MISALIGN[dtype]):
            assert _elementwise_plan(n, dtype, offset == 0).vec == (offset == 0)
            X = Guarded.of(dev, x32.to(TORCH_DTYPE[dtype]), offset)
            Y = Guarded(dev, TORCH_DTYPE[dtype], n, offset)
            _call(lib, 'ampconv_act_dropout_fwd', X.ptr, n, 0, *_mask_args(p), Y.ptr, CODE[dtype], None)
            assert Y.intact() and np.array_equal(Y.np() != 0, keep), (dtype, offset)


# ---- pooling -----------------------------------------------------------------------------------------------------------
L_LADDER = [1, K_UNROLL - 1, K_UNROLL, K_UNROLL + 1, 2 * K_UNROLL + 1]          # 1, 3, 4, 5, 9: the kUnroll remainders 1, 3, 0, 1


def _pool_case(lib, dev, N, D, dtype, offset, combos):
    """pool_fwd and pool_bwd of x [N, L, D] for every L of the ladder, both poolings and every (activation, p) of
    `combos`; the identity's backward is handed x = NULL."""
    tdt = TORCH_DTYPE[dtype]
    for L in L_LADDER:
        g = torch.Generator().manual_seed(100000 * N + 100 * D + L)
        x, dp = draw(g, dtype, N, L * D), draw(g, dtype, N, D)
        X, DP = Guarded.of(dev, x, offset), Guarded.of(dev, dp, offset)
        OUT, DX = Guarded(dev, tdt, N * D, offset), Guarded(dev, tdt, N * L * D, offset)
        xn, dpn = _f64(x), _f64(dp)
        for pooling in POOLING:
            for a, p in combos:
                label = f'L={L} {pooling} {a} p={p}'
                OUT.refill(), DX.refill()
                _call(lib, 'ampconv_pool_fwd', X.ptr, N, L, D, ACT[a], POOLING[pooling], *_mask_args(p), OUT.ptr,
                      CODE[dtype], None)
                assert OUT.intact() and OUT.written(), label
                close(OUT.np(N, D), ref.pool_fwd(xn, L, D, a, pooling, SEED, p), 'pooled ' + label, **TOL[dtype])
                _call(lib, 'ampconv_pool_bwd', None if a == 'identity' else X.ptr, DP.ptr, N, L, D, ACT[a],
                      POOLING[pooling], *_mask_args(p), DX.ptr, CODE[dtype], None)
                assert DX.intact() and DX.written(), label
                close(DX.np(N, L * D), ref.pool_bwd(xn, dpn, L, D, a, pooling, SEED, p), 'dx ' + label, **TOL[dtype])
                if pooling == 'token0':                          # the rows behind token 0: bit-zero
                    assert bool((bits(DX.t.view(N, L, D)[:, 1:]) == 0).all()), label
        assert X.intact() and DP.intact()


POOL_COMBOS = [('identity', 0.6), ('relu', 0.0), ('relu', 0.6), ('elu', 0.1), ('elu', 0.6)]
# (pieces per row, nodes): one lane per (node, piece).  P = 1: 255, 256 and 257 units, i.e. one lane short of a
# workgroup, a whole one, one lane into the second.  P = 3: 255 units.  P = 25 (D = 100 fp32): a wave spans three nodes
# (64 / 25 = 2.56) and P does not divide 64.  P = 32: exactly 256 units, two nodes per wave.  P = 33: a wave starts
# mid-row, 264 units.
POOL_VEC = [(1, 255), (1, 256), (1, 257), (3, 85), (25, 11), (32, 8), (33, 8)]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('P,N', POOL_VEC, ids=[f'vec_P{P}_N{N}_units{P * N}' for P, N in POOL_VEC])
def test_pool_16_byte_path(P, N, dtype, lib, dev):
    D = P * NP[dtype]
    plan = _pool_plan(N, D, dtype, aligned=True)
    assert plan.vec and plan.per_node == P and plan.units == P * N and plan.blocks == (1 if P * N <= THREADS else 2)
    _pool_case(lib, dev, N, D, dtype, 0, POOL_COMBOS)


# (D, nodes, base offset in elements): rows no piece divides (D = 1, 3) and whole-piece rows behind an unaligned base
POOL_SCALAR = [(1, 257, 0), (3, 86, 0), (3, 86, 1), (100, 3, 1), (128, 3, 1)]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('D,N,skew', POOL_SCALAR, ids=[f'scalar_D{D}_N{N}_{"unaligned" if s else "aligned"}' for D, N, s in POOL_SCALAR])
def test_pool_element_wise_path(D, N, skew, dtype, lib, dev):
    """pool_{fwd,bwd}_scalar: a lane per (node, channel), N D a few lanes past one workgroup."""
    plan = _pool_plan(N, D, dtype, aligned=not skew)
    assert not plan.vec and plan.per_node == D and plan.blocks == 2
    _pool_case(lib, dev, N, D, dtype, skew * MISALIGN[dtype], POOL_COMBOS)
