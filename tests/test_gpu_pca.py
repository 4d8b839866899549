"""ampnet_amd.pca on the GPU: the three C calls of csrc/pca.hip ONE CALL AT A TIME through ctypes against the fp64
models of tests/pca_reference.py, then pca() end to end against pca_model and scikit-learn's recorded outputs
(tests/golden/pca/), its properties and the model hook.

Call by call (as tests/test_gpu_linear_kernels.py): x is a row-strided view inside NaN margins and NaN gaps, outputs lie
in NaN-filled buffers with margins, the workspace is NaN-filled; after a call nothing outside the output may have changed
and everything inside must be finite.  The bounds are derived, not tuned:
    Gram:        |Sm - gram_model|  <= (kPcaRun + 2) 2^-24 (|A|^T |A|)   fp32 sums over a run of kPcaRun rows, fp64 above
    projection:  |out - model|      <= (W + 2) 2^-24 |scale| (|A| |V|)   fp32 sums over W columns
    means:       bit-equal to numpy.float32(x.astype(float64).mean(axis))
Every sweep names all its failing cases in one assertion.

End to end the flat bound is 4 x YARDSTICK: for each fixture input the largest error against pca_model of a plain fp32
composite (fp32 centring, torch.linalg.svd in fp32; pca_reference.fp32_composite_error), measured on the CPU.  The factor
4 covers the different summation order of a method that should be more accurate, not less."""
import glob
import os
import types

import numpy as np
import pytest
import torch

import pca_reference as pr
from conftest import GOLDEN_DIR, load_golden
from edge_runner import stream

from ampnet_amd import _lib

pytestmark = pytest.mark.gpu

RUN = _lib.PCA_RUN
R_LADDER = (1, 2, 15, 16, 17, 33, RUN - 1, RUN + 1, 3000)
W_LADDER = (1, 3, 16, 17, 63, 64, 65, 130, 257)
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}
MARGIN = 8                      # elements in front of and behind every buffer: 16 bytes of bf16, so the base stays aligned
BADARG, EWORKSPACE = -1, -3

# the fp32 composite's largest error against pca_model per fixture input (fp32 input, the input rounded to bf16), measured
# on the CPU with pca_reference.fp32_composite_error (torch 2.x CPU, LAPACK gesdd); the end-to-end bound is 4 x this
YARDSTICK = {('pca_rows_40x12', 'fp32'): 5.445e-07, ('pca_rows_40x12', 'bf16'): 3.612e-07,
             ('pca_columns_12x40', 'fp32'): 3.031e-07, ('pca_columns_12x40', 'bf16'): 5.341e-07,
             ('pca_rows_64x64', 'fp32'): 3.594e-07, ('pca_rows_64x64', 'bf16'): 4.674e-07}
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, 'pca', 'pca_*.npz')))


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def dev():
    return torch.device('cuda:0')


class Placed:
    """A [rows, cols] view with row stride ld inside a NaN-filled 1-d buffer with NaN margins."""

    def __init__(self, rows, cols, ld, dtype, data=None):
        self.shape, self.ld = (rows, cols), ld
        self.backing = torch.full((2 * MARGIN + rows * ld,), float('nan'), dtype=dtype, device=dev())
        self.view = torch.as_strided(self.backing, (rows, cols), (ld, 1), MARGIN)
        if data is not None:
            self.view.copy_(torch.as_tensor(data).to(dev(), dtype))
        self.inside = torch.zeros(self.backing.numel(), dtype=torch.bool, device=dev())
        torch.as_strided(self.inside, (rows, cols), (ld, 1), MARGIN).fill_(True)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def values(self):
        return self.view.double().cpu().numpy() if self.view.dtype != torch.float64 else self.view.cpu().numpy()

    def problems(self, name):
        bad = []
        if not torch.isnan(self.backing[~self.inside]).all():
            bad.append(f'{name}: bytes outside the output were written')
        if not torch.isfinite(self.backing[self.inside]).all():
            bad.append(f'{name}: elements of the output were not written (or are not finite)')
        return bad

    def untouched(self):
        return bool(torch.isnan(self.backing).all())


def nan_workspace(nbytes):
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device=dev())


def rows_of(R, W, dtype, seed):
    """Random rows with a mean that is not small against their spread, as the kernels' fp32 values (bf16: rounded)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((R, W)) + 0.5 * rng.standard_normal(W)[None, :]).astype(np.float32)
    return torch.as_tensor(x).to(dtype).float().numpy()


def shifts_of(x, shift, seed):
    rng = np.random.default_rng(seed + 1000)
    rs = (x.mean(1) + 0.01 * rng.standard_normal(x.shape[0])).astype(np.float32) if shift in ('row', 'both') else None
    cs = (x.mean(0) + 0.01 * rng.standard_normal(x.shape[1])).astype(np.float32) if shift in ('col', 'both') else None
    return rs, cs


def dptr(a):
    return None if a is None else a.data_ptr()


def to_dev(a):
    return None if a is None else torch.as_tensor(a).to(dev())


# ----------------------------------------------------------------------------------------------------------- Gram
def run_gram(lib, R, W, ld, dt, shift, twice=False):
    name = f'gram R{R} W{W} ld{ld} {dt} shift={shift}'
    x = rows_of(R, W, DTYPES[dt], 7 * R + W)
    rs, cs = shifts_of(x, shift, R + W)
    px, pS = Placed(R, W, ld, DTYPES[dt], x), Placed(W, W, W, torch.float64)
    drs, dcs = to_dev(rs), to_dev(cs)
    ws = nan_workspace(lib.ampconv_pca_gram_workspace_bytes(R, W))
    rc = lib.ampconv_pca_gram(px.ptr, R, W, ld, dptr(drs), dptr(dcs), pS.ptr, ws.data_ptr(), ws.numel(), _lib.DTYPES[DTYPES[dt]],
                              stream())
    torch.cuda.synchronize()
    if rc != 0:
        return [f'{name}: returned {rc}']
    bad = pS.problems(name)
    if bad:
        return bad
    got = pS.values()
    ref, scale = pr.gram_model(x, rs, cs)
    over = np.abs(got - ref) > (RUN + 2) * pr.U24 * scale
    if over.any():
        share = float((np.abs(got - ref) / np.maximum((RUN + 2) * pr.U24 * scale, 1e-300)).max())
        bad.append(f'{name}: {int(over.sum())}/{over.size} elements over the bound, the worst {share:.3g} times it')
    if not (got == got.T).all():
        bad.append(f'{name}: the output is not exactly symmetric')
    if twice:
        pS2 = Placed(W, W, W, torch.float64)
        ws2 = nan_workspace(lib.ampconv_pca_gram_workspace_bytes(R, W))
        rc = lib.ampconv_pca_gram(px.ptr, R, W, ld, dptr(drs), dptr(dcs), pS2.ptr, ws2.data_ptr(), ws2.numel(),
                                  _lib.DTYPES[DTYPES[dt]], stream())
        torch.cuda.synchronize()
        if rc != 0 or not torch.equal(pS.view, pS2.view):
            bad.append(f'{name}: a second call (rc {rc}) is not bitwise equal to the first')
    return bad


@pytest.mark.parametrize('shift', ['none', 'row', 'col'])
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
def test_gram_on_the_ladders(dt, shift, lib):
    """Every R x W of the ladders at ldx = W and W + 3: rows below, at and above a tile and a run, widths below, at and
    above a 16-column tile, a 64-column quarter and a 128-column panel (257: three panels, six blocks)."""
    failed = []
    for R in R_LADDER:
        for W in W_LADDER:
            for ld in (W, W + 3):
                failed += run_gram(lib, R, W, ld, dt, shift, twice=(W in (17, 257) and ld == W))
    assert not failed, failed


def test_gram_splits_follow_the_shape(lib):
    """3000 rows are more than one split of the rows at every width of the ladder; up to 256 they are one; the
    workspace holds one fp64 W x W partial per split and stays under 64 MiB from the second split on."""
    for W in W_LADDER + (2048,):
        n = lib.ampconv_pca_gram_splits(3000, W)
        assert n > 1, (W, n)
        assert lib.ampconv_pca_gram_splits(256, W) == 1
        assert lib.ampconv_pca_gram_workspace_bytes(3000, W) >= n * W * W * 8
        assert n * W * W * 8 <= 64 << 20
    assert lib.ampconv_pca_gram_splits(1_000_000, 256) * 256 * 256 * 8 <= 64 << 20
    assert lib.ampconv_pca_gram_splits(1_000_000, 2048) == 2


def test_gram_with_both_shifts(lib):
    failed = []
    for R, W in ((33, 17), (257, 130)):
        failed += run_gram(lib, R, W, W + 3, 'fp32', 'both')
    assert not failed, failed


def test_calls_refuse_what_they_do_not_take(lib):
    x = torch.zeros(4, 8, device=dev())
    S = torch.full((8, 8), float('nan'), dtype=torch.float64, device=dev())
    out = torch.full((4, 8), float('nan'), device=dev())
    ws = nan_workspace(1 << 16)
    f32 = _lib.AMPCONV_F32
    gram = lambda **k: lib.ampconv_pca_gram(*[k.get(n, d) for n, d in (('x', x.data_ptr()), ('R', 4), ('W', 8), ('ld', 8), ('rs', None),
                                              ('cs', None), ('S', S.data_ptr()), ('ws', ws.data_ptr()), ('wsb', ws.numel()),
                                              ('dtype', f32), ('stream', stream()))])
    assert gram() == 0
    S.fill_(float('nan'))
    for bad in (dict(R=0), dict(W=0), dict(W=2049, ld=2049), dict(ld=7), dict(x=None), dict(S=None), dict(dtype=2)):
        assert gram(**bad) == BADARG, bad
    assert gram(ws=None) == EWORKSPACE and gram(wsb=8) == EWORKSPACE
    V = torch.zeros(8, 2, device=dev())
    proj = lambda **k: lib.ampconv_pca_project(*[k.get(n, d) for n, d in (('x', x.data_ptr()), ('R', 4), ('W', 8), ('ld', 8), ('rs', None),
                                                 ('cs', None), ('V', V.data_ptr()), ('k', 2), ('scale', None), ('out', out.data_ptr()),
                                                 ('ldo', 8), ('dtype', f32), ('stream', stream()))])
    for bad in (dict(k=0), dict(k=129), dict(ldo=1), dict(V=None), dict(out=None), dict(R=0), dict(ld=7), dict(dtype=-1)):
        assert proj(**bad) == BADARG, bad
    m = torch.full((8,), float('nan'), device=dev())
    shift = lambda **k: lib.ampconv_pca_shift(*[k.get(n, d) for n, d in (('x', x.data_ptr()), ('R', 4), ('W', 8), ('ld', 8), ('axis', 0),
                                                ('out', m.data_ptr()), ('ws', ws.data_ptr()), ('wsb', ws.numel()), ('dtype', f32),
                                                ('stream', stream()))])
    for bad in (dict(axis=2), dict(R=0), dict(W=0), dict(out=None), dict(x=None)):
        assert shift(**bad) == BADARG, bad
    assert shift(ws=None) == EWORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(S).all() and torch.isnan(out).all() and torch.isnan(m).all()


# ---------------------------------------------------------------------------------------------------------- means
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
def test_means_on_the_ladders(dt, lib):
    failed = []
    for R in R_LADDER:
        for W in W_LADDER:
            x = rows_of(R, W, DTYPES[dt], 3 * R + W)
            for ld in (W, W + 3):
                px = Placed(R, W, ld, DTYPES[dt], x)
                for axis in (0, 1):
                    name = f'mean R{R} W{W} ld{ld} {dt} axis {axis}'
                    po = Placed(1, W if axis == 0 else R, W if axis == 0 else R, torch.float32)
                    ws = nan_workspace(lib.ampconv_pca_shift_workspace_bytes(R, W, axis))
                    rc = lib.ampconv_pca_shift(px.ptr, R, W, ld, axis, po.ptr, ws.data_ptr(), ws.numel(),
                                               _lib.DTYPES[DTYPES[dt]], stream())
                    torch.cuda.synchronize()
                    if rc != 0:
                        failed.append(f'{name}: returned {rc}')
                        continue
                    failed += po.problems(name)
                    got, ref = po.view.cpu().numpy()[0], pr.shift_model(x, axis)
                    if not np.array_equal(got, ref):
                        failed.append(f'{name}: {int((got != ref).sum())}/{ref.size} means differ from the fp64 mean rounded once')
    assert not failed, failed


def test_column_means_over_many_chunks(lib):
    """100 000 rows: more than one chunk of the two-level reduction, and two calls are bitwise equal."""
    x = rows_of(100_000, 5, torch.float32, 1)
    dx = to_dev(x)
    outs = []
    for _ in range(2):
        out = torch.empty(5, device=dev())
        ws = nan_workspace(lib.ampconv_pca_shift_workspace_bytes(100_000, 5, 0))
        assert lib.ampconv_pca_shift(dx.data_ptr(), 100_000, 5, 5, 0, out.data_ptr(), ws.data_ptr(), ws.numel(), 0, stream()) == 0
        outs.append(out.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], pr.shift_model(x, 0))


# ----------------------------------------------------------------------------------------------------- projection
def run_project(lib, R, W, k, ld, ldo, dt, shift, scaled):
    name = f'project R{R} W{W} k{k} ld{ld} ldo{ldo} {dt} shift={shift} scale={scaled}'
    x = rows_of(R, W, DTYPES[dt], 5 * R + W + k)
    rs, cs = shifts_of(x, shift, R + W + k)
    rng = np.random.default_rng(R + 31 * W + k)
    V = rng.standard_normal((W, k)).astype(np.float32)
    scale = None
    if scaled:
        scale = (1.0 / (0.5 + rng.random(k))).astype(np.float32)
        scale[k // 2] = 0.0                                       # a rank-deficient direction
    px, po = Placed(R, W, ld, DTYPES[dt], x), Placed(R, k, ldo, torch.float32)
    drs, dcs, dV, dsc = to_dev(rs), to_dev(cs), to_dev(V), to_dev(scale)
    rc = lib.ampconv_pca_project(px.ptr, R, W, ld, dptr(drs), dptr(dcs), dV.data_ptr(), k, dptr(dsc), po.ptr, ldo,
                                 _lib.DTYPES[DTYPES[dt]], stream())
    torch.cuda.synchronize()
    if rc != 0:
        return [f'{name}: returned {rc}']
    bad = po.problems(name)
    if bad:
        return bad
    got = po.values()
    ref, bscale = pr.project_model(x, V, rs, cs, scale)
    over = np.abs(got - ref) > (W + 2) * pr.U24 * bscale
    if over.any():
        share = float((np.abs(got - ref) / np.maximum((W + 2) * pr.U24 * bscale, 1e-300)).max())
        bad.append(f'{name}: {int(over.sum())}/{over.size} elements over the bound, the worst {share:.3g} times it')
    if scaled and not (got[:, k // 2] == 0).all():
        bad.append(f'{name}: the column with scale 0 is not zeros')
    return bad


@pytest.mark.parametrize('k', [1, 2, 17, 128])
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
def test_project_on_the_ladders(dt, k, lib):
    """Rows below, at and above a workgroup's 64, widths below, at and above a 32-column step, every k of the list with
    and without scale, a leading dimension of the output, each shift."""
    failed = []
    for R in (1, 2, 17, 64, 65, 200):
        for W in (1, 3, 31, 32, 33, 130, 257):
            for shift, scaled, pad in (('none', False, 0), ('row', True, 3), ('col', False, 3), ('both', True, 0)):
                failed += run_project(lib, R, W, k, W + pad, k + pad, dt, shift, scaled)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------ end to end
FIELDS = ('scores', 'components', 'singular_values', 'explained_variance', 'explained_variance_ratio')


def fit(x, k, samples, dt='fp32'):
    from ampnet_amd import pca
    return pca(torch.as_tensor(x).to(dev(), DTYPES[dt]), k, samples=samples)


def result_arrays(res):
    return {n: getattr(res, n).double().cpu().numpy() for n in FIELDS + ('all_explained_variance_ratio', 'mean')}


def invariants(got, name):
    comp = got['components']
    bad = []
    orth = float(np.abs(comp @ comp.T - np.eye(comp.shape[0])).max())
    if orth > 1e-5:
        bad.append(f'{name}: components are not orthonormal ({orth:.3g})')
    for n in ('explained_variance', 'singular_values', 'all_explained_variance_ratio'):
        if (np.diff(got[n]) > 0).any():
            bad.append(f'{name}: {n} is not descending')
    r = got['all_explained_variance_ratio']
    if (r < 0).any() or (r > 1).any() or r.sum() > 1 + 1e-6 or got['explained_variance_ratio'].sum() > 1 + 1e-6:
        bad.append(f'{name}: the ratios are not in [0, 1] with a sum <= 1')
    at = np.abs(comp).argmax(axis=1)
    if not (comp[np.arange(comp.shape[0]), at] > 0).all():
        bad.append(f'{name}: a component whose largest-magnitude entry is not positive')
    return bad


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_pca_against_the_model_and_scikit_learn(path, dt):
    """pca() on the fixture input in the fixture's mode, and on its transpose in the other mode (the same problem, the
    transpose never formed by the library): against pca_model of the input as the GPU holds it and, for fp32, against
    scikit-learn's recorded outputs; then the four invariants."""
    g = load_golden(path)
    base, k, samples = os.path.basename(path)[:-4], int(g['k']), str(g['samples'])
    x = torch.as_tensor(g['x']).to(DTYPES[dt]).float().numpy()
    model = pr.pca_model(x, k, samples)
    bound = 4 * YARDSTICK[base, dt]
    other = 'columns' if samples == 'rows' else 'rows'
    failed = []
    for xin, mode in ((x, samples), (np.ascontiguousarray(x.T), other)):
        got = result_arrays(fit(xin, k, mode, dt))
        refs = [('pca_model', model)] + ([('scikit-learn', g)] if dt == 'fp32' else [])
        for ref_name, ref in refs:
            for n in FIELDS:
                err = float(np.abs(got[n] - ref[n]).max())
                print(f'[pca] {base} {dt} samples={mode} {n} vs {ref_name}: max err {err:.3e} = {err / bound:.2f} of the bound {bound:.3e}')
                if err > bound:
                    failed.append(f'{base} {dt} samples={mode} {n} vs {ref_name}: {err:.3e} > {bound:.3e}')
        nv = min(x.shape)
        err = float(np.abs(got['all_explained_variance_ratio'][:nv] - model['all_explained_variance_ratio']).max())
        if got['all_explained_variance_ratio'].shape != (nv,) or err > bound:
            failed.append(f'{base} {dt} samples={mode} all_explained_variance_ratio: {err:.3e}')
        if float(np.abs(got['mean'] - model['mean']).max()) > 2.0 ** -23 * float(np.abs(model['mean']).max()):
            failed.append(f'{base} {dt} samples={mode}: mean')
        failed += invariants(got, f'{base} {dt} samples={mode}')
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------ properties
def test_scores_are_the_transform_of_the_input_and_new_rows_project():
    g = load_golden(FIXTURES[1])
    res = fit(g['x'], 5, 'rows')
    x = torch.as_tensor(g['x']).to(dev())
    assert torch.equal(res.scores, res.transform(x))
    y = x[3:20] * 1.5
    ref = (y.double() - res.mean.double()) @ res.components.double().t()
    assert float((res.transform(y).double() - ref).abs().max()) <= 4 * YARDSTICK['pca_rows_40x12', 'fp32']
    wide = torch.full((40, 15), float('nan'), device=dev())
    wide[:, 1:13] = x
    assert torch.equal(res.scores, fit(wide[:, 1:13], 5, 'rows').scores)            # a row-strided view, read in place
    with pytest.raises(ValueError):
        res.transform(x[:, :5])
    with pytest.raises(ValueError):
        fit(g['x'], 5, 'columns').transform(x)


@pytest.mark.parametrize('samples', ['rows', 'columns'])
def test_a_constant_per_feature_leaves_the_scores(samples):
    """Adding a constant to every feature of the data -- to every column for samples='rows', to every row for 'columns' --
    changes the mean and nothing else.  The input is first cut to 12 fractional bits and the constants are multiples of
    1/4, so the sums are exact in fp32: both fits see the same data, moved."""
    path = FIXTURES[1] if samples == 'rows' else FIXTURES[0]
    x = (np.round(load_golden(path)['x'].astype(np.float64) * 4096) / 4096).astype(np.float32)
    P = x.shape[1] if samples == 'rows' else x.shape[0]
    c = (np.arange(P) % 5 - 2).astype(np.float32) * 0.25
    moved = x + (c[None, :] if samples == 'rows' else c[:, None])
    assert (moved.astype(np.float64) == x.astype(np.float64) + (c[None, :] if samples == 'rows' else c[:, None])).all()
    a, b = result_arrays(fit(x, 5, samples)), result_arrays(fit(moved, 5, samples))
    bound = 4 * YARDSTICK[os.path.basename(path)[:-4], 'fp32']
    for n in FIELDS:
        assert float(np.abs(a[n] - b[n]).max()) <= bound, n
    assert float(np.abs(b['mean'] - a['mean'] - c).max()) <= 1e-6


def test_two_samples_work():
    x = np.array([[1.0, 2.0, 4.0], [3.0, -2.0, 5.0]], dtype=np.float32)
    for samples, xin in (('rows', x), ('columns', np.ascontiguousarray(x.T))):
        got, ref = result_arrays(fit(xin, 1, samples)), pr.pca_model(xin, 1, samples)
        for n in FIELDS:                                          # results up to 4.4: 8 ulp of fp32 there
            assert float(np.abs(got[n] - ref[n]).max()) <= 4e-6, (samples, n)
        assert abs(got['explained_variance_ratio'][0] - 1) <= 1e-6


def test_rank_deficient_directions():
    """An exactly rank-2 input (small integers, centred exactly): the singular values past the rank are reported (close
    to 0, never negative or NaN), the samples='columns' components there are zeros, the scores there vanish, and the
    leading two directions match the model."""
    rng = np.random.default_rng(5)
    X = 9.0 * (rng.integers(-3, 4, (9, 2)).astype(np.float64) @ rng.integers(-3, 4, (2, 7)).astype(np.float64))
    X = (X - X.mean(axis=0)).astype(np.float32)                   # multiples of 1 / 9 times 9: integers, exact in fp32
    for samples, xin in (('rows', X), ('columns', np.ascontiguousarray(X.T))):
        got, ref = result_arrays(fit(xin, 4, samples)), pr.pca_model(xin, 4, samples)
        S = got['singular_values']
        assert np.isfinite(S).all() and (S >= 0).all() and (S[2:] <= 1e-3 * S[0]).all(), S
        assert float(np.abs(got['scores'][:, :2] - ref['scores'][:, :2]).max()) <= 1e-5 * float(np.abs(ref['scores']).max())
        assert float(np.abs(got['components'][:2] - ref['components'][:2]).max()) <= 1e-5
        assert float(np.abs(got['scores'][:, 2:]).max()) <= 1e-3 * S[0]
        if samples == 'columns':
            assert (got['components'][2:] == 0).all()
        assert np.isfinite(got['components']).all() and np.isfinite(got['scores']).all()
    z = result_arrays(fit(np.ones((5, 4), dtype=np.float32), 2, 'rows'))               # no variance at all
    assert (z['explained_variance_ratio'] == 0).all() and (z['singular_values'] == 0).all() and (z['scores'] == 0).all()


# ------------------------------------------------------------------------------------------------------ model hook
def test_model_hook_fills_and_freezes_the_table():
    from ampnet_amd import AMPGCN, pca
    torch.manual_seed(0)
    N, F, D, L = 30, 12, 8, 4
    x = torch.randn(N, F, device=dev())
    ei = torch.randint(0, N, (2, 90), device=dev())
    data = types.SimpleNamespace(x=x, edge_index=ei)
    for down in (True, False):
        model = AMPGCN(device=dev(), embedding_dim=D, num_heads=2, num_node_features=F, num_sampled_vectors=L if down else F,
                       output_dim=3, feat_emb_dim=D - 1, downsample_feature_vectors=down, feature_repeats=1,
                       dropout_rate=0.0, dropout_adj_rate=0.0).to(dev())
        res = model.init_feature_table_from_pca(x, freeze=True)
        want = pca(x, D - 1, samples='columns').scores
        assert res.scores.shape == (F, D - 1) and torch.equal(model.feature_embedding_table.weight, want)
        assert not model.feature_embedding_table.weight.requires_grad
        out = model(data)
        assert out.shape == (N, 3) and torch.isfinite(out).all()
        out.sum().backward()
        with_grad = [n for n, p in model.named_parameters() if p.grad is not None]
        assert 'feature_embedding_table.weight' not in with_grad and 'conv1.multi_head_attention.in_proj_weight' in with_grad
        assert torch.equal(model.feature_embedding_table.weight, want)
    thaw = AMPGCN(device=dev(), embedding_dim=D, num_heads=2, num_node_features=F, num_sampled_vectors=L, output_dim=3,
                  feat_emb_dim=D - 1, dropout_rate=0.0, dropout_adj_rate=0.0).to(dev())
    thaw.init_feature_table_from_pca(x, freeze=False)
    thaw(data).sum().backward()
    assert thaw.feature_embedding_table.weight.grad is not None
    with pytest.raises(ValueError):
        thaw.init_feature_table_from_pca(x[:, :5])
