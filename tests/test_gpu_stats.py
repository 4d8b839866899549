"""ampnet_amd.tensor_stats (csrc/stats.hip) on the GPU against the numpy model of tests/stats_reference.py.

Bars.  Every count, min, max, absmax, every histogram count, below / above, the median and the quantiles are EXACTLY the
model's (the order statistics bit for bit).  For all-finite inputs the median is also bitwise torch.median's on the device.
mean, absmean and std are within rtol 1e-6 of the fp64 model on inputs with |mean| <= 100 std: the fp64 accumulation error
of n <= 1e7 terms is below 1e-9 relative, the sum_sq / n - mean^2 cancellation amplifies it by at most
(mean^2 + var) / var <= 1e4 + 1, which leaves about three orders of head-room; the achieved error is printed.

Sizes, with C = CHUNK = the elements a workgroup handles per iteration: 0, 1, 3, 63, 64, 65, C - 1, C, C + 1, 4 C + 5
(five workgroups flush into the same counts) and 1027 C + 7 (more chunks than the 1024 workgroups a tensor gets: the
grid-stride loop).  Contents at 4 C + 5."""
import functools

import numpy as np
import pytest
import torch

import stats_reference as ref

pytestmark = pytest.mark.gpu

BINS, QS = 50, (0.25, 0.9)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _C():
    from ampnet_amd import _lib
    return _lib.STATS_CHUNK


def _sizes():
    C = _C()
    return [0, 1, 3, 63, 64, 65, C - 1, C, C + 1, 4 * C + 5]


def _to_dtype(x, dtype):
    """(host tensor of `dtype`, what the model takes for it): float32 as it is, bfloat16 as its bit patterns."""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    if dtype == 'bf16':
        t = t.to(torch.bfloat16)
        return t, t.view(torch.int16).numpy().view(np.uint16)
    return t, t.numpy()


@functools.lru_cache(maxsize=None)
def _contents(dtype):
    """{name: (host tensor, model input)} at 4 C + 5 elements: drawn once, shared, never modified."""
    n = 4 * _C() + 5
    rng = np.random.default_rng(11)
    x = ref.normal(n, 12)
    zeros = np.zeros(n, np.float32)
    zeros[rng.random(n) < 0.5] = -0.0
    pm = x.copy()
    pm[rng.random(n) < 0.3] = 0.0
    pm[rng.random(n) < 0.3] = -0.0
    raw = {'normal': x, 'relu': np.maximum(x, np.float32(0)), 'zeros': np.zeros(n, np.float32),
           'constant': np.full(n, 2.5, np.float32), 'sorted': np.sort(x),
           'ties': rng.choice(np.array([-1.5, -0.25, 0.0, 0.75, 3.0], np.float32), n), 'signed zeros': zeros,
           'zeros mixed in': pm, 'non-finite': ref.sprinkle(x, 13), 'gradients': ref.log_uniform(n, 14)}
    return {k: _to_dtype(v, dtype) for k, v in raw.items()}


@functools.lru_cache(maxsize=None)
def _want(dtype, name, bins=BINS, rng=None):
    return ref.stats(_contents(dtype)[name][1], bins=bins, range=rng, median=True, quantiles=QS)


def _same_float(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes() or (np.isnan(a) and np.isnan(b))


def _check(got, want, what):
    for k in ('numel', 'finite', 'nan', 'inf', 'zeros', 'negative'):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ('min', 'max', 'absmax'):
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), (what, k, got[k], want[k])
    if 'hist' in want:
        assert got['hist'].dtype == np.uint64 and np.array_equal(got['hist'], want['hist']), \
            (what, 'hist', np.flatnonzero(got['hist'] != want['hist'])[:8])
        assert (got['below'], got['above']) == (want['below'], want['above']), (what, got['below'], got['above'])
        assert int(got['hist'].sum()) + got['below'] + got['above'] == got['finite'], what
    if 'median' in want:
        assert _same_float(got['median'], want['median']), (what, 'median', got['median'], want['median'])
    if 'quantiles' in want:
        assert all(_same_float(a, b) for a, b in zip(got['quantiles'], want['quantiles'])), \
            (what, got['quantiles'], want['quantiles'])
    n = want['finite']
    if n == 0:
        assert np.isnan([got['mean'], got['absmean'], got['std']]).all(), what
        return
    keys = ['mean', 'absmean'] + (['std'] if n > 1 and abs(want['mean']) <= 100 * want['std'] else [])
    if n == 1:
        assert np.isnan(got['std']), what
    for k in keys:
        scale = abs(want[k])
        err = abs(got[k] - want[k]) / scale if scale else abs(got[k] - want[k])
        print(f'[tol] {what} {k}: {got[k]:.9e} vs {want[k]:.9e}, rel err {err:.2e} (bar 1e-6)')
        assert err <= 1e-6, (what, k, got[k], want[k])


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_sizes(dev, dtype):
    """All sizes in one call: 10 descriptors, workgroup counts 0, 1, 2 and 5."""
    from ampnet_amd import tensor_stats
    pairs = {f'n={n}': _to_dtype(ref.sprinkle(ref.normal(n, 20 + i), 40 + i, 0.02), dtype) for i, n in enumerate(_sizes())}
    got = tensor_stats({k: t.to(dev) for k, (t, _) in pairs.items()}, bins=BINS, median=True, quantiles=QS).read()
    assert list(got) == list(pairs)
    for k, (_, model_in) in pairs.items():
        _check(got[k], ref.stats(model_in, bins=BINS, median=True, quantiles=QS), f'{dtype} {k}')
        assert got[k]['edges'].shape == (BINS + 1,)
    assert got['n=0']['finite'] == 0 and np.isnan(got['n=0']['median']) and got['n=0']['hist'].sum() == 0


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_contents(dev, dtype):
    from ampnet_amd import tensor_stats
    data = _contents(dtype)
    got = tensor_stats({k: t.to(dev) for k, (t, _) in data.items()}, bins=BINS, median=True, quantiles=QS).read()
    for k in data:
        _check(got[k], _want(dtype, k), f'{dtype} {k}')
    assert got['relu']['hist'][0] > got['relu']['finite'] // 2                     # the one hot bin
    assert got['constant']['hist'][0] == got['constant']['finite']                 # hi == lo: everything in bin 0
    assert got['non-finite']['nan'] > 0 and got['non-finite']['inf'] > 0
    assert got['signed zeros']['zeros'] == got['signed zeros']['numel'] and got['signed zeros']['negative'] == 0
    t = got['ties']
    assert t['median'] in (-1.5, -0.25, 0.0, 0.75, 3.0) and t['hist'][0] > 0 and t['hist'][-1] > 0     # lo and hi themselves


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_median_is_torch_median_on_the_device(dev, dtype):
    from ampnet_amd import tensor_stats
    data = _contents(dtype)
    names = [k for k in data if k != 'non-finite']
    got = tensor_stats([data[k][0].to(dev) for k in names], median=True).read()
    for k, g in zip(names, got):
        want = torch.median(data[k][0].to(dev)).float().cpu().numpy()
        assert np.float32(g['median']).tobytes() == want.tobytes() or (g['median'] == 0 and want == 0), (dtype, k)


def test_many_chunks_per_workgroup(dev):
    """1027 C + 7 elements: 1028 chunks on 1024 workgroups, so four workgroups take a second chunk (the last one partial),
    and all 1024 flush into the same counts; 2048 bins, 1 % non-finite."""
    from ampnet_amd import tensor_stats
    n = 1027 * _C() + 7
    x = ref.sprinkle(ref.normal(n, 30), 31)
    got = tensor_stats(torch.from_numpy(x).to(dev), bins=2048, median=True, quantiles=(0.01, 0.999)).read()
    _check(got, ref.stats(x, bins=2048, median=True, quantiles=(0.01, 0.999)), 'large')


def test_user_range_on_another_stream(dev):
    """A range narrower than the data, its ends values of the data: host pair, device pair on the default stream, device
    pair on a side stream -- the same counts, equal to the model's."""
    from ampnet_amd import tensor_stats
    t, model_in = _contents('f32')['normal']
    lo, hi = float(np.sort(model_in)[1000]), float(np.sort(model_in)[-1000])
    want = ref.stats(model_in, bins=30, range=(lo, hi), median=True, quantiles=QS)
    assert want['below'] == 1000 and want['above'] == 999 and want['hist'][0] > 0 and want['hist'][-1] > 0
    x = t.to(dev)
    pair = torch.tensor([lo, hi], dtype=torch.float32, device=dev)
    host = tensor_stats(x, bins=30, range=(lo, hi), median=True, quantiles=QS).read()
    default = tensor_stats(x, bins=30, range=pair, median=True, quantiles=QS).read()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        pending = tensor_stats(x, bins=30, range=pair, median=True, quantiles=QS)
    other = pending.read()                                                         # read under the default stream
    torch.cuda.current_stream(dev).wait_stream(side)
    for got, what in ((host, 'host range'), (default, 'device range'), (other, 'side stream')):
        _check(got, want, what)
        assert np.allclose(got['edges'][[0, -1]], [lo, hi])
    for k in ('mean', 'absmean', 'std'):
        assert default[k] == other[k] == host[k]                                    # the same bits on either stream


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_unaligned_slices_and_nan_guards(dev, dtype):
    """A contiguous slice one element into a larger buffer -- 4-byte (fp32) or 2-byte (bf16) aligned only, the
    element-wise loads -- whose neighbours on both sides are NaN: none of them is counted, and every number, the fp64
    sums included, has the bits of the aligned call."""
    from ampnet_amd import tensor_stats
    t, model_in = _contents(dtype)['gradients']
    n = t.numel()
    buf = torch.full((n + 64,), float('nan'), dtype=t.dtype, device=dev)
    view = buf[1:1 + n]
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 if dtype == 'f32' else 2)
    got, aligned = tensor_stats([view, t.to(dev)], bins=BINS, median=True, quantiles=QS).read()
    _check(got, _want(dtype, 'gradients'), f'{dtype} slice')
    assert got['nan'] == 0
    for k in ('mean', 'absmean', 'std'):
        assert got[k] == aligned[k], k


@pytest.mark.parametrize('count', [24, 25])
def test_descriptor_batches(dev, count):
    """24 tensors are one batch of descriptors, 25 a second one; sizes and dtypes mixed."""
    from ampnet_amd import _lib, tensor_stats
    assert _lib.STATS_MAX_TENSORS == 24
    sizes = [(37 * i * i + 1) % 9000 for i in range(count)]
    sizes[3] = 0
    pairs = [_to_dtype(ref.normal(n, 50 + i), 'bf16' if i % 3 == 1 else 'f32') for i, n in enumerate(sizes)]
    got = tensor_stats([t.to(dev) for t, _ in pairs], bins=30, median=True, quantiles=(0.75,)).read()
    assert len(got) == count
    for i, (_, model_in) in enumerate(pairs):
        _check(got[i], ref.stats(model_in, bins=30, median=True, quantiles=(0.75,)), f'tensor {i} of {count}')


def test_two_calls_give_the_same_bits(dev):
    from ampnet_amd import tensor_stats
    xs = {k: t.to(dev) for k, (t, _) in _contents('f32').items()}
    a = tensor_stats(xs, bins=BINS, median=True, quantiles=QS)
    b = tensor_stats(xs, bins=BINS, median=True, quantiles=QS)           # both outstanding
    assert torch.equal(a._out, b._out)
    ra, rb = a.read(), b.read()
    for k in xs:
        for f in ('mean', 'absmean', 'std', 'median'):
            assert ra[k][f] == rb[k][f] or (np.isnan(ra[k][f]) and np.isnan(rb[k][f]))


def test_one_tensor_and_no_extras(dev):
    from ampnet_amd import tensor_stats
    t, model_in = _contents('f32')['normal']
    got = tensor_stats(t.to(dev).view(3, -1)).read()                       # any shape, as long as it is contiguous
    assert 'hist' not in got and 'median' not in got and 'quantiles' not in got
    _check(got, ref.stats(model_in), 'moments only')
    assert tensor_stats([]).read() == []


def test_what_is_not_supported_raises(dev):
    from ampnet_amd import tensor_stats
    x = torch.randn(64, 8, device=dev)
    for bad, match in ((x.half(), 'float16'), (x.cpu(), 'not on the GPU'), (x.t(), 'not contiguous'), (x.long(), 'int64')):
        with pytest.raises(ValueError, match=match):
            tensor_stats(bad)
    with pytest.raises(ValueError, match='bins=2049'):
        tensor_stats(x, bins=2049)
    with pytest.raises(ValueError, match='order statistics'):
        tensor_stats(x, median=True, quantiles=(0.1, 0.2, 0.3, 0.4))
    with pytest.raises(ValueError, match='quantiles'):
        tensor_stats(x, quantiles=(1.5,))
    with pytest.raises(ValueError, match='range'):
        tensor_stats(x, bins=4, range=(1.0, 0.0))
