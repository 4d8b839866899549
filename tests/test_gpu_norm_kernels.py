"""csrc/norm.hip one library call at a time (ampnet_amd._lib, no Python wrapper in between) against the numpy fp64 model
of tests/norm_reference.py, on ladders derived from the kernels' own constants.

test_gpu_norm.py runs the models' shapes through the autograd wrappers; here every (G, K, U) that `row_shape` and
`tokens_per_step` of norm.hip can yield is entered on purpose, in fp32 and bf16, on the 16-byte and on the element-wise
path, and the test's id names it.  `_plan` below mirrors that dispatch arithmetic; every case first asserts that the
mirror puts it on the path its id names.  The path is steered as a caller would steer it: by D and by the alignment of
the base (a view 4 resp. 2 bytes into an allocation).

Every tensor the library touches lies between guard bands (tests/site_guards.py); workspaces are exactly
ampconv_norm_workspace_bytes long; after every call the bands must be intact and every output element written.  Every
backward that reduces over tokens is launched twice and must give the same bits.
Tolerances: y, pooled, dx at the project's flat atol 1e-5, rtol 1e-4; weight.grad and bias.grad (sums over all tokens)
under those labels, i.e. the scaled bar; bf16 storage atol = rtol = 2e-2 (test_gpu_norm.py).  The statistics: `_check_stats`.
ReLU's kink: an fp32 pre-activation may change sign against fp64 where |z| is at rounding level, and one such element
moves weight.grad by O(1).  Every ReLU case therefore asserts on the CPU, before any kernel output is looked at, that the
fp64 model's pre-activation has min |z| >= 1e-5 over the whole case; the case's seed is the first one for which that
holds, and no element is left out of any comparison.  ReLU stays on the small ladder shapes; the multi-million-element
grid-stride cases run the identity and ELU, whose slope is continuous at 0.
Conditioning: rows narrower than 16 channels take tokens whose mean is exactly representable (`_tokens` says why)."""
import functools
import types

import numpy as np
import pytest
import torch

import glue_reference as glue
import norm_reference as ref
from site_guards import MISALIGN, TOL, TORCH_DTYPE, Guarded, bits, close, draw, header_constant

pytestmark = pytest.mark.gpu

MAX_D = header_constant('AMPCONV_NORM_MAX_D')
THREADS = 256                                   # csrc/norm.hip:19   kThreads
K_MAX_BLOCKS = 2048                             # csrc/norm.hip:20   kMaxBlocks (also the number of slots)
K_IN_FLIGHT = 4                                 # csrc/norm.hip:21   kInFlight
SCALAR_K = MAX_D // 64                          # csrc/norm.hip:23   kScalarK
K_RUNS = 16                                     # csrc/norm.hip:24   kRuns
ACT = {'identity': 0, 'relu': 1, 'elu': 2}
POOLING = {'mean': 0, 'token0': 1}
NP = {'f32': 4, 'bf16': 8}
CODE = {'f32': 0, 'bf16': 1}
SEED = 0x1234567890ABCDEF
EPS = 1e-5
RELU_MARGIN = 1e-5


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


# ---- the mirror of norm.hip's dispatch arithmetic ----------------------------------------------------------------------
def _plan(dtype, D, aligned=True):
    """row_shape + tokens_per_step: vec (16-byte pieces), P pieces per row, G lanes per token, K pieces per lane, U tokens
    per step, and `share`: the tokens one workgroup takes per trip of the plain kernels."""
    vec = aligned and D % NP[dtype] == 0
    if vec:
        P, G = D // NP[dtype], 4
        while G < 64 and G < P:
            G <<= 1
        K = -(-P // G)
        assert K <= (4 if dtype == 'f32' else 2)                 # with_row_shape: anything else is AMPCONV_E_BADARG
    else:
        P, G, K = D, 64, SCALAR_K
    U = 1 if K >= K_IN_FLIGHT else K_IN_FLIGHT // K
    return types.SimpleNamespace(vec=vec, P=P, G=G, K=K, U=U, groups=THREADS // G, share=THREADS // G * U,
                                 lane_adds=K * (NP[dtype] if vec else 1) + G.bit_length() - 1)


def _grid(units, plan):
    """grid_of: workgroups for `units` groups' worth of work (token steps of the plain calls, nodes of the pooled ones)"""
    return min(-(-units // plan.groups), K_MAX_BLOCKS)


def _plain_blocks(T, plan):
    return _grid(-(-T // plan.U), plan)


def _name(dtype, D, plan):
    return f'{dtype}_D{D}_{"vec" if plan.vec else "elem"}_G{plan.G}_K{plan.K}_U{plan.U}'


# ---- inputs ------------------------------------------------------------------------------------------------------------
NARROW = 16                                     # rows narrower than this get tokens whose mean is exact, see _tokens


def _tokens(g, dtype, T, D):
    """x [1, T * D] in the storage dtype.  From NARROW channels up: standard normal values.  Narrower rows: fixed-point
    values (fp32: multiples of 2^-10 up to +-4; bf16: of 2^-5) whose last channel is moved by less than D units so that
    the token's sum is a multiple of D units.  Sum, mean and x - mean are then exact in fp32 as in fp64.
    Why: stats holds the mean as an fp32 number, so whatever the kernel does xhat = (x - mu) rstd carries an ABSOLUTE
    error of up to 2^-25 |mu| rstd, which dropout's scale and gamma (up to 5 together here) carry into y and rstd once
    more into dx.  The flat bar gives that 1e-5, so a token needs about |mu| rstd < 10, i.e. |mean| / std of its D
    values below 10: a t statistic of 10 sqrt(D).  At D >= 16 no random token ever comes near (t > 40 on 15 degrees of
    freedom); at D = 3 and 4 the t distribution's tail puts about one token in a thousand beyond it, hundreds among
    the half million of the grid-stride case, and rstd can reach 1 / sqrt(eps) = 316.  With standard normal tokens
    the D = 3 width case and the D = 4 grid-stride case each had one element at 102 % resp. 110 % of the bar on the
    MI355X, all others far inside.  That is the conditioning of LayerNorm over three or four values, not of the kernel,
    so the narrow rows take it out of the inputs; every path, index and mask is exercised as before."""
    if D >= NARROW:
        return draw(g, dtype, 1, T * D)
    unit, top = (2.0 ** -10, 4096) if dtype == 'f32' else (2.0 ** -5, 128)
    k = (torch.randn(T, D, generator=g) * (top // 4)).round().clamp(-top, top).to(torch.int64)
    k[:, -1] -= torch.remainder(k.sum(dim=1), D)
    x = (k.double() * unit).to(TORCH_DTYPE[dtype])
    assert bool((x.double() == k.double() * unit).all()) and bool((torch.remainder(k.sum(dim=1), D) == 0).all())
    return x.view(1, T * D)


@functools.lru_cache(maxsize=8)
def _inputs(T, D, dtype, seed=0):
    """x [1, T * D] and dy of that shape in the storage dtype, gamma and beta [D] fp32 (both away from 1 resp. 0)."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * T + D)
    x, dy = _tokens(g, dtype, T, D), draw(g, dtype, 1, T * D)
    gamma = 1 + 0.5 * torch.randn(D, generator=g)
    beta = 0.5 * torch.randn(D, generator=g)
    beta = torch.where(beta.abs() < 0.05, torch.full_like(beta, 0.25), beta)
    return x, dy, gamma, beta


def _pre_activation(x, D, gamma, beta, affine):
    xhat = ref.token_stats(_f64(x), D, EPS)[2]
    return xhat * _f64(gamma) + _f64(beta) if affine else xhat


@functools.lru_cache(maxsize=None)
def _relu_seed(T, D, dtype, affine):
    """The first seed whose fp64 pre-activation z = xhat gamma + beta stays RELU_MARGIN away from 0 on every element."""
    for seed in range(64):
        x, _, gamma, beta = _inputs(T, D, dtype, seed)
        if np.abs(_pre_activation(x, D, gamma, beta, affine)).min() >= RELU_MARGIN:
            return seed
    raise AssertionError('no seed keeps the pre-activation away from the kink')


def _case_inputs(T, D, dtype, a, affine):
    seed = _relu_seed(T, D, dtype, affine) if a == 'relu' else 0
    x, dy, gamma, beta = _inputs(T, D, dtype, seed)
    if a == 'relu':                                              # on the CPU, before any kernel output
        assert np.abs(_pre_activation(x, D, gamma, beta, affine)).min() >= RELU_MARGIN
    return x, dy, gamma, beta


def _mask_args(p):
    thr, scale = glue.mask_params(p)
    return SEED, thr, float(scale)


def _check_stats(got, want, xn, D, plan, label):
    """(mean, 1 / sqrt(var + eps)) against the fp64 model, by the derivation of test_statistics_match_the_fp64_model:
    rtol 1e-5; the mean of a token can be arbitrarily close to zero, so it also gets the absolute rounding error of an fp32
    sum: every addition rounds at 2^-24 of a partial sum <= sum |x|, and no value passes through more than the lane's own
    additions (K pieces of 4 or 8 elements: at most 16; 16 one-element pieces on the element-wise path) plus the log2 G
    of the butterfly (at most 6)."""
    assert plan.lane_adds <= 22 and (plan.vec or plan.lane_adds == 16 + 6)
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), label
    mu_atol = plan.lane_adds * 2.0 ** -24 * np.abs(xn.reshape(-1, D)).mean(axis=1)
    err = np.abs(got[:, 0] - want[:, 0])
    assert (err <= 1e-5 * np.abs(want[:, 0]) + mu_atol).all(), (label, float(err.max()))
    np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=1e-5, atol=0, err_msg=label)


class _Params:
    """gamma, beta and the buffers of their gradients and of the slot workspace, for a call on T tokens."""

    def __init__(self, lib, dev, T, D, gamma, beta, affine, grads):
        self.G = Guarded.of(dev, gamma) if affine else None
        self.B = Guarded.of(dev, beta) if affine else None
        self.gn, self.bn = (_f64(gamma), _f64(beta)) if affine else (None, None)
        self.DG = Guarded(dev, torch.float32, D) if grads else None
        self.DB = Guarded(dev, torch.float32, D) if grads else None
        need = lib.ampconv_norm_workspace_bytes(T, D)
        assert need == min(T, K_MAX_BLOCKS) * 2 * D * 4
        self.need = need if grads else 0
        self.WS = Guarded(dev, torch.uint8, need) if grads else None

    def fwd(self):
        return (self.G.ptr if self.G else None, self.B.ptr if self.B else None)

    def bwd(self):
        return (self.DG.ptr if self.DG else None, self.DB.ptr if self.DB else None, self.WS.ptr if self.WS else None, self.need)

    def check_grads(self, want_dg, want_db, label, dtype):
        if self.DG is None:
            return ()
        assert self.DG.intact() and self.DB.intact() and self.WS.intact() and self.DG.written() and self.DB.written(), label
        close(self.DG.np(), want_dg, 'weight.grad ' + label, **TOL[dtype])
        close(self.DB.np(), want_db, 'bias.grad ' + label, **TOL[dtype])
        return (bits(self.DG.t).clone(), bits(self.DB.t).clone())

    def refill(self):
        for g in (self.DG, self.DB, self.WS):
            if g is not None:
                g.refill()

    def inputs_intact(self):
        return all(g.intact() for g in (self.G, self.B) if g is not None)


def _check_plain(lib, dev, T, D, dtype, offset, a, p, affine=True, grads=True):
    """ampconv_norm_fwd, then ampconv_norm_bwd (twice) on the stats it wrote."""
    plan = _plan(dtype, D, aligned=offset == 0)
    x, dy, gamma, beta = _case_inputs(T, D, dtype, a, affine)
    tdt, label = TORCH_DTYPE[dtype], f'T={T} {a} p={p} affine={affine}'
    X, DY = Guarded.of(dev, x, offset), Guarded.of(dev, dy, offset)
    Y, DX = Guarded(dev, tdt, T * D, offset), Guarded(dev, tdt, T * D, offset)
    STATS = Guarded(dev, torch.float32, 2 * T)
    par = _Params(lib, dev, T, D, gamma, beta, affine, grads)
    xn, dyn = _f64(x), _f64(dy)
    _call(lib, 'ampconv_norm_fwd', X.ptr, T, D, *par.fwd(), EPS, ACT[a], *_mask_args(p), Y.ptr, STATS.ptr, CODE[dtype], None)
    assert Y.intact() and Y.written() and STATS.intact() and STATS.written(), label
    want_y, want_stats = ref.norm_fwd(xn, D, par.gn, par.bn, EPS, a, SEED, p)
    close(Y.np(1, T * D), want_y, 'y ' + label, **TOL[dtype])
    _check_stats(STATS.np(T, 2), want_stats, xn, D, plan, label)
    if a == 'identity' and p > 0:
        keep = glue.keep_mask(SEED, glue.mask_params(p)[0], (1, T * D))
        if np.array_equal(want_y != 0, keep):                    # no z is exactly 0 (D = 1 without beta: all are): the zeros ARE the mask
            assert np.array_equal(Y.np(1, T * D) != 0, keep), label
    want_dx, want_dg, want_db = ref.norm_bwd(xn, dyn, D, par.gn, par.bn, EPS, a, SEED, p)
    runs = []
    for _ in range(2):
        DX.refill(), par.refill()
        _call(lib, 'ampconv_norm_bwd', X.ptr, DY.ptr, STATS.ptr, T, D, *par.fwd(), ACT[a], *_mask_args(p), DX.ptr,
              *par.bwd(), CODE[dtype], None)
        assert DX.intact() and DX.written(), label
        if not runs:
            close(DX.np(1, T * D), want_dx, 'dx ' + label, **TOL[dtype])
        runs.append((bits(DX.t).clone(),) + par.check_grads(want_dg, want_db, label, dtype))
    for first, second in zip(*runs):
        assert torch.equal(first, second), label + ': two launches, different bits'
    assert X.intact() and DY.intact() and STATS.intact() and par.inputs_intact()
    return Y


def _check_pool(lib, dev, N, L, D, dtype, offset, a, p, pooling, affine=True, grads=True):
    """ampconv_norm_pool_fwd, then ampconv_norm_pool_bwd (twice).  stats is exactly [N, tokens, 2] between its bands:
    token-0 pooling must write [N, 2] and not a byte more."""
    plan = _plan(dtype, D, aligned=offset == 0)
    x, _, gamma, beta = _case_inputs(N * L, D, dtype, a, affine)
    x = x.view(N, L * D)
    dp = draw(torch.Generator().manual_seed(N * L + D), dtype, N, D)
    tdt, label = TORCH_DTYPE[dtype], f'N={N} L={L} {pooling} {a} p={p} affine={affine}'
    tokens = 1 if pooling == 'token0' else L
    X, DP = Guarded.of(dev, x, offset), Guarded.of(dev, dp, offset)
    OUT, DX = Guarded(dev, tdt, N * D, offset), Guarded(dev, tdt, N * L * D, offset)
    STATS = Guarded(dev, torch.float32, 2 * N * tokens)
    par = _Params(lib, dev, N * L, D, gamma, beta, affine, grads)
    xn, dpn = _f64(x), _f64(dp)
    args = (L, D, par.gn, par.bn, EPS, a, pooling, SEED, p)
    _call(lib, 'ampconv_norm_pool_fwd', X.ptr, N, L, D, *par.fwd(), EPS, ACT[a], POOLING[pooling], *_mask_args(p), OUT.ptr,
          STATS.ptr, CODE[dtype], None)
    assert OUT.intact() and OUT.written() and STATS.intact() and STATS.written(), label
    want, want_stats = ref.norm_pool_fwd(xn, *args)
    close(OUT.np(N, D), want, 'pooled ' + label, **TOL[dtype])
    rows = xn.reshape(N, L, D)[:, :tokens].reshape(-1, D)
    _check_stats(STATS.np(N * tokens, 2), want_stats, rows, D, plan, label)
    want_dx, want_dg, want_db = ref.norm_pool_bwd(xn, dpn, *args)
    runs = []
    for _ in range(2):
        DX.refill(), par.refill()
        _call(lib, 'ampconv_norm_pool_bwd', X.ptr, DP.ptr, STATS.ptr, N, L, D, *par.fwd(), ACT[a], POOLING[pooling],
              *_mask_args(p), DX.ptr, *par.bwd(), CODE[dtype], None)
        assert DX.intact() and DX.written(), label
        if not runs:
            close(DX.np(N, L * D), want_dx, 'dx ' + label, **TOL[dtype])
        if pooling == 'token0':                                  # the rows behind token 0: bit-zero
            assert bool((bits(DX.t.view(N, L, D)[:, 1:]) == 0).all()), label
        runs.append((bits(DX.t).clone(),) + par.check_grads(want_dg, want_db, label, dtype))
    for first, second in zip(*runs):
        assert torch.equal(first, second), label + ': two launches, different bits'
    assert X.intact() and DP.intact() and STATS.intact() and par.inputs_intact()


# ---- the width ladder --------------------------------------------------------------------------------------------------
# (D, G, K, U) the case means to hit: both sides of every step of G and of K
F32_VEC = [(4, 4, 1, 4), (16, 4, 1, 4), (20, 8, 1, 4), (32, 8, 1, 4), (36, 16, 1, 4), (64, 16, 1, 4), (68, 32, 1, 4),
           (128, 32, 1, 4), (132, 64, 1, 4), (256, 64, 1, 4), (260, 64, 2, 2), (512, 64, 2, 2), (516, 64, 3, 1),
           (768, 64, 3, 1), (772, 64, 4, 1), (1024, 64, 4, 1)]
BF16_VEC = [(8, 4, 1, 4), (32, 4, 1, 4), (40, 8, 1, 4), (64, 8, 1, 4), (72, 16, 1, 4), (128, 16, 1, 4), (136, 32, 1, 4),
            (256, 32, 1, 4), (264, 64, 1, 4), (512, 64, 1, 4), (520, 64, 2, 2), (1024, 64, 2, 2)]
ELEM = (64, SCALAR_K, 1)
WIDTHS = ([('f32', D, 0, g, k, u) for D, g, k, u in F32_VEC] + [('bf16', D, 0, g, k, u) for D, g, k, u in BF16_VEC] +
          [('f32', D, 0 if D % 4 else MISALIGN['f32']) + ELEM for D in (1, 3, 63, 64, 65, 1023)] +      # 64: by the base
          [('bf16', D, 0) + ELEM for D in (4, 1022)] +
          [(dt, D, MISALIGN[dt]) + ELEM for dt in ('f32', 'bf16') for D in (100, 128)])


def _width_id(case):
    dtype, D, offset, G, K, U = case
    vec = offset == 0 and D % NP[dtype] == 0
    return f'{dtype}_D{D}_{"vec" if vec else "elem"}_G{G}_K{K}_U{U}' + ('_unaligned' if offset else '')


def _assert_path(case):
    dtype, D, offset, G, K, U = case
    plan = _plan(dtype, D, aligned=offset == 0)
    assert (plan.G, plan.K, plan.U) == (G, K, U), (case, plan)
    assert _name(dtype, D, plan) + ('_unaligned' if offset else '') == _width_id(case)
    return plan


def test_the_mirror_on_a_row_worked_by_hand():
    """fp32 D = 260: 65 pieces, a 64-lane group, two pieces per lane, two tokens per step; and the ladder reaches every (G, K)."""
    plan = _plan('f32', 260)
    assert (plan.vec, plan.P, plan.G, plan.K, plan.U) == (True, 65, 64, 2, 2)
    assert {(G, K) for _, _, _, G, K, _ in WIDTHS} >= {(g, 1) for g in (4, 8, 16, 32, 64)} | {(64, 2), (64, 3), (64, 4), (64, 16)}


@pytest.mark.parametrize('case', WIDTHS, ids=_width_id)
def test_width_ladder(case, lib, dev):
    """One workgroup's share of tokens and one more (a second workgroup with a single token; the pooled calls: one node
    more than a workgroup's groups, L = U + 1 so that the token loop takes a full and a partial step).  The widths are both
    sides of every step of G (4 | 5, 8 | 9, 16 | 17, 32 | 33 pieces), of K (64 | 65, 128 | 129, 192 | 193 pieces: the last k
    holds a single live lane) and, element-wise, of the wave (63, 64, 65 channels), the shortest rows (1, 3) and the
    longest whose last k is masked in the middle of the wave (1023, bf16 1022); D = 100 and 128 reach the element-wise
    kernels through the base alone."""
    dtype, D, offset = case[:3]
    plan = _assert_path(case)
    T = plan.share + 1
    assert _plain_blocks(T, plan) == 2
    _check_plain(lib, dev, T, D, dtype, offset, 'relu', 0.6)
    _check_plain(lib, dev, T, D, dtype, offset, 'elu', 0.0)
    _check_plain(lib, dev, T, D, dtype, offset, 'identity', 0.6, affine=False, grads=False)
    _check_plain(lib, dev, T, D, dtype, offset, 'elu', 0.6, grads=False)
    N, L = plan.groups + 1, plan.U + 1
    assert _grid(N, plan) == 2
    _check_pool(lib, dev, N, L, D, dtype, offset, 'elu', 0.6, 'mean')
    _check_pool(lib, dev, N, L, D, dtype, offset, 'relu', 0.6, 'token0')
    _check_pool(lib, dev, N, L, D, dtype, offset, 'identity', 0.0, 'mean', affine=False, grads=False)


# ---- tokens per step ---------------------------------------------------------------------------------------------------
STEPS = [('f32', 128, 0, 32, 1, 4), ('f32', 260, 0, 64, 2, 2), ('bf16', 520, 0, 64, 2, 2), ('f32', 1024, 0, 64, 4, 1),
         ('f32', 65, 0) + ELEM, ('bf16', 128, MISALIGN['bf16']) + ELEM]


@pytest.mark.parametrize('case', STEPS, ids=_width_id)
def test_token_ladder(case, lib, dev):
    """T = 1, U - 1, U, U + 1: a step that is short, exactly full, and a full one followed by a single token, for each U
    that tokens_per_step yields (4, 2, 1, and 1 again on the element-wise path)."""
    dtype, D, offset = case[:3]
    plan = _assert_path(case)
    for T in sorted({1, plan.U - 1, plan.U, plan.U + 1} - {0}):
        assert _plain_blocks(T, plan) == 1
        _check_plain(lib, dev, T, D, dtype, offset, 'elu', 0.6)
        _check_plain(lib, dev, T, D, dtype, offset, 'relu', 0.0, affine=False, grads=False)


@pytest.mark.parametrize('case', STEPS, ids=_width_id)
def test_pooled_ladder(case, lib, dev):
    """L = 1, U - 1, U, U + 1, 2 U + 1 tokens per node; N = 1 and one node more than a workgroup has groups; both poolings.
    Token-0 pooling with L > 1: the rows of dx behind token 0 are bit-zero and stats is [N, 2] and not a byte more."""
    dtype, D, offset = case[:3]
    plan = _assert_path(case)
    for N in (1, plan.groups + 1):
        assert _grid(N, plan) == (1 if N == 1 else 2)
        for L in sorted({1, plan.U - 1, plan.U, plan.U + 1, 2 * plan.U + 1} - {0}):
            for pooling in POOLING:
                _check_pool(lib, dev, N, L, D, dtype, offset, 'elu', 0.6, pooling)
                _check_pool(lib, dev, N, L, D, dtype, offset, 'relu', 0.0, pooling, affine=False, grads=False)


# ---- the grid stride ---------------------------------------------------------------------------------------------------
STRIDES = [('f32', 4, 0, 4, 1, 4), ('f32', 1024, 0, 64, 4, 1)]


@pytest.mark.parametrize('case', STRIDES, ids=_width_id)
def test_grid_stride_against_the_reference(case, lib, dev):
    """Five tokens more than kMaxBlocks workgroups take in one trip, at the narrowest row (G = 4, U = 4: 64 groups of 4
    tokens, 8 MB) and at the widest (G = 64, U = 1: 4 groups of 1 token, 34 MB): workgroups 0 and 1 come round a second
    time (`tb += groups`), and what they add there goes into the same slot."""
    dtype, D, offset = case[:3]
    plan = _assert_path(case)
    T = K_MAX_BLOCKS * plan.share + 5
    assert _plain_blocks(T, plan) == K_MAX_BLOCKS and -(-T // plan.U) > K_MAX_BLOCKS * plan.groups
    _check_plain(lib, dev, T, D, dtype, offset, 'elu', 0.6)
    if D == 4:
        _check_plain(lib, dev, T, D, dtype, offset, 'identity', 0.6, affine=False, grads=False)


@pytest.mark.parametrize('case', STRIDES, ids=_width_id)
def test_pooled_grid_stride_against_the_reference(case, lib, dev):
    """N = three nodes more than kMaxBlocks workgroups have groups, L = 2 (`n += groups`)."""
    dtype, D, offset = case[:3]
    plan = _assert_path(case)
    N = K_MAX_BLOCKS * plan.groups + 3
    assert _grid(N, plan) == K_MAX_BLOCKS and N > K_MAX_BLOCKS * plan.groups
    _check_pool(lib, dev, N, 2, D, dtype, offset, 'elu', 0.6 if D == 4 else 0.0, 'mean')       # 17 M elements: without the mask
    if D == 4:
        _check_pool(lib, dev, N, 2, D, dtype, offset, 'identity', 0.6, 'token0')


# ---- norm_reduce_slots -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slots', [1, K_RUNS - 1, K_RUNS, K_RUNS + 1, K_MAX_BLOCKS], ids=lambda s: f'slots{s}_elem_G64_K16_U1')
def test_slot_counts(slots, lib, dev):
    """norm_reduce_slots cuts the slots into kRuns = 16 runs of ceil(slots / 16): fewer slots than runs (1, 15: runs of
    one, the rest empty), exactly 16, 17 (runs of two, the ninth holds one, seven are empty), and all 2048.  Chosen
    through T on the element-wise path, where a workgroup holds 4 tokens: D = 65 fp32, 130 columns, i.e. a ragged fifth
    workgroup of the reduction."""
    dtype, D = 'f32', 65
    plan = _plan(dtype, D)
    assert not plan.vec and plan.share == 4
    T = plan.share * slots - 1
    assert _plain_blocks(T, plan) == slots
    _check_plain(lib, dev, T, D, dtype, 0, 'elu', 0.6)
    if slots <= K_RUNS + 1:
        N = plan.groups * slots - 1
        assert _grid(N, plan) == slots
        _check_pool(lib, dev, N, 2, D, dtype, 0, 'relu', 0.6, 'mean')


# ---- the mask ----------------------------------------------------------------------------------------------------------
def test_mask_is_the_same_bits_on_every_path(lib, dev):
    """One logical [33, 128] tensor through the 16-byte and the element-wise kernels, in fp32 and in bf16, identity under
    p = 0.6: the zeros of the four outputs are the same elements, those of glue_reference.keep_mask."""
    T, D, p = 33, 128, 0.6
    keep = glue.keep_mask(SEED, glue.mask_params(p)[0], (1, T * D))
    for dtype in ('f32', 'bf16'):
        for offset in (0, MISALIGN[dtype]):
            assert _plan(dtype, D, offset == 0).vec == (offset == 0)
            Y = _check_plain(lib, dev, T, D, dtype, offset, 'identity', p)
            assert np.array_equal(Y.np(1, T * D) != 0, keep), (dtype, offset)
