"""The numpy model of the tensor statistics (tests/stats_reference.py) against implementations that know nothing of it:
numpy's fp64 moments, np.sort / np.quantile(method='lower') / torch.median, and np.histogram.  No GPU.

Histogram: the header's fp32 bin rule and numpy's fp64 edges legitimately disagree for values within a rounding of an edge.
The condition: at most 1e-3 of the elements land in another bin, and every such element moves by exactly one bin.
Measured on these 10^6-element inputs (differing elements at 30 / 50 / 2048 bins): N(0,1) 0 / 0 / 62, ReLU(N(0,1)) 0 / 0 / 7,
the log-uniform gradients 110 / 320 / 153."""
import numpy as np
import pytest
import torch

import stats_reference as ref

N = 1_000_000


def _inputs():
    x = ref.normal(N, 1)
    return {'normal': x, 'relu': np.maximum(x, np.float32(0)), 'log-uniform': ref.log_uniform(N, 2)}


INPUTS = _inputs()


@pytest.mark.parametrize('name', list(INPUTS))
def test_moments_against_numpy_fp64(name):
    x = ref.sprinkle(INPUTS[name], 3)
    got = ref.stats(x)
    fin = np.isfinite(x)
    d = x[fin].astype(np.float64)
    assert got['numel'] == x.size and got['finite'] == int(fin.sum())
    assert got['nan'] == int(np.isnan(x).sum()) and got['inf'] == int(np.isinf(x).sum()) and got['nan'] and got['inf']
    assert got['zeros'] == int((d == 0).sum()) and got['negative'] == int((d < 0).sum())
    assert got['min'] == d.min() and got['max'] == d.max() and got['absmax'] == np.abs(d).max()
    np.testing.assert_allclose([got['mean'], got['absmean'], got['std']], [d.mean(), np.abs(d).mean(), np.std(d, ddof=1)],
                               rtol=1e-12)


def test_counts_come_from_the_bits():
    x = np.array([0.0, -0.0, 1.0, -1.0, np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45], np.float32)
    got = ref.stats(x, median=True)
    assert (got['finite'], got['nan'], got['inf'], got['zeros'], got['negative']) == (6, 2, 2, 2, 2)
    assert got['min'] == -1.0 and got['max'] == 1.0 and got['median'] == 0.0
    b = ref.stats(ref.bf16_bits(x))
    assert (b['finite'], b['nan'], b['inf'], b['zeros'], b['negative']) == (6, 2, 2, 4, 1)     # 1e-45 rounds to 0 in bf16
    e = ref.stats(np.zeros(0, np.float32), bins=4, median=True, quantiles=(0.25,))
    assert e['finite'] == 0 and np.isnan([e['mean'], e['std'], e['min'], e['max'], e['median'], e['quantiles'][0]]).all()
    assert e['hist'].sum() == 0
    assert np.isnan(ref.stats(np.ones(1, np.float32))['std'])


def test_bf16_patterns_round_like_torch():
    x = np.concatenate([ref.normal(10_000, 4), ref.log_uniform(10_000, 5), [np.inf, -np.inf, 0.0, -0.0]]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(ref.bf16_bits(x), want)


@pytest.mark.parametrize('n', [100_000, 100_001, 100_003])
def test_selection_against_sort_quantile_and_torch_median(n):
    for x in (ref.normal(n, 6), np.maximum(ref.normal(n, 7), np.float32(0)), ref.log_uniform(n, 8)):
        qs = (0.25, 0.75, 0.9)
        got = ref.stats(x, median=True, quantiles=qs)
        want = np.sort(x)[(n - 1) // 2]
        assert np.float32(got['median']).tobytes() == want.tobytes()
        assert np.float32(got['median']).tobytes() == torch.median(torch.from_numpy(x)).numpy().tobytes()
        for q, g in zip(qs, got['quantiles']):
            assert g == np.quantile(x, q, method='lower'), (n, q)
    assert ref.rank_of(0.5, n) == (n - 1) // 2


def test_selection_skips_what_is_not_finite():
    x = ref.sprinkle(ref.normal(50_001, 9), 10)
    fin = x[np.isfinite(x)]
    got = ref.stats(x, median=True, quantiles=(0.0, 1.0))
    assert got['median'] == np.sort(fin)[(fin.size - 1) // 2]
    assert got['quantiles'] == [fin.min(), fin.max()]


@pytest.mark.parametrize('bins', [30, 50, 2048])
@pytest.mark.parametrize('name', list(INPUTS))
def test_histogram_against_numpy(name, bins):
    x = INPUTS[name]
    lo, hi = x.min(), x.max()
    b, below, above = ref.bin_index(x, lo, hi, bins)
    assert below == 0 and above == 0
    counts, edges = np.histogram(x, bins, range=(lo, hi))
    theirs = np.clip(np.searchsorted(edges, x, side='right') - 1, 0, bins - 1)       # np.histogram's bin of every element
    assert np.array_equal(np.bincount(theirs, minlength=bins), counts)
    moved = b != theirs
    print(f'[hist] {name}, {bins} bins: {int(moved.sum())} of {x.size} elements in another bin (cap {x.size // 1000})')
    assert moved.sum() <= 1e-3 * x.size
    assert (np.abs(b[moved] - theirs[moved]) == 1).all()
    assert np.array_equal(ref.histogram(x, lo, hi, bins)[0], np.bincount(b, minlength=bins).astype(np.uint64))


def test_histogram_edges_and_outside():
    x = np.array([-2.0, -1.0, -1.0, 0.0, 0.999, 1.0, 1.0, 3.0], np.float32)
    h, below, above = ref.histogram(x, -1.0, 1.0, 4)
    assert (below, above) == (1, 1) and h.tolist() == [2, 0, 1, 3]        # lo goes to bin 0, hi to the last bin
    h, below, above = ref.histogram(np.full(5, 2.5, np.float32), 2.5, 2.5, 7)
    assert (below, above) == (0, 0) and h.tolist() == [5, 0, 0, 0, 0, 0, 0]


def test_binding_mirrors_the_header():
    import ctypes
    import os
    import re
    from conftest import ROOT
    from ampnet_amd import _lib, stats
    header = open(os.path.join(ROOT, 'include', 'ampconv.h')).read()
    define = lambda name: int(re.search(rf'#define\s+{name}\s+(\d+)', header).group(1))
    assert define('AMPCONV_STATS_MAX_TENSORS') == _lib.STATS_MAX_TENSORS == stats.MAX_TENSORS == 24
    assert define('AMPCONV_STATS_CHUNK') == _lib.STATS_CHUNK == stats.CHUNK
    assert define('AMPCONV_STATS_MAX_BINS') == _lib.STATS_MAX_BINS == stats.MAX_BINS == 2048
    assert define('AMPCONV_STATS_MAX_RANKS') == _lib.STATS_MAX_RANKS == stats.MAX_RANKS == 4
    for name in ('ampconv_stats_workspace_bytes', 'ampconv_stats_moments', 'ampconv_stats_histogram', 'ampconv_stats_select'):
        assert name in _lib.SIGNATURES, name
    assert ctypes.sizeof(_lib.StatsTensor) == 24 and _lib.StatsTensor.numel.offset == 8 and _lib.StatsTensor.dtype.offset == 16
    # ampconv_stats_record_t: six int64, three doubles, four floats
    assert stats.RECORD.itemsize == _lib.STATS_RECORD_BYTES == 6 * 8 + 3 * 8 + 4 * 4
    assert [stats.RECORD.fields[k][1] for k in ('numel', 'sum', 'min', 'absmax')] == [0, 48, 72, 80]


def test_host_side_checks_need_no_device():
    from ampnet_amd import TensorStats, tensor_stats
    x = torch.randn(8, 4)
    with pytest.raises(ValueError, match='not on the GPU'):
        tensor_stats(x)
    with pytest.raises(ValueError, match='not on the GPU'):
        tensor_stats({'a': x}, bins=4)
    with pytest.raises(ValueError, match='bins=2049'):
        tensor_stats(x, bins=2049)
    with pytest.raises(ValueError, match='order statistics'):
        tensor_stats(x, median=True, quantiles=(0.1, 0.2, 0.3, 0.4))
    with pytest.raises(ValueError, match='got a list'):
        tensor_stats([[1.0, 2.0]])
    empty = tensor_stats([])
    assert isinstance(empty, TensorStats) and len(empty) == 0 and empty.read() == []


def test_model_has_the_reference_diagnostics_signatures():
    """experiments/cora_benchmark_graphsaint.py:111-114 calls them positionally; src/ampnet/module/amp_gcn.py:278,308,345."""
    import inspect
    from ampnet_amd import AMPGCN
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(AMPGCN.plot_grad_flow)[:4] == ['self', 'save_path', 'epoch_idx', 'iter']
    assert names(AMPGCN.visualize_gradients)[:5] == ['self', 'save_path', 'epoch_idx', 'iter', 'color']
    assert names(AMPGCN.visualize_activations)[:6] == ['self', 'save_path', 'data', 'epoch_idx', 'iter', 'color']
    assert inspect.signature(AMPGCN.visualize_gradients).parameters['color'].default == 'C0'
    assert names(AMPGCN.gradient_stats) == ['self', 'bins', 'median'] and names(AMPGCN.activation_stats) == [
        'self', 'data', 'bins', 'feature_indices']
    assert 'mode' in AMPGCN.gradient_stats.__doc__ and 'restored' in AMPGCN.activation_stats.__doc__


def test_stats_kernels_do_not_spill():
    """hipcc's resource remarks for csrc/stats.hip (build/obj/stats.o.usage.json, written by __graft_entry__.build())."""
    import json
    import os
    from conftest import ROOT
    import __graft_entry__ as ge
    ge.build()
    path = os.path.join(ROOT, 'build', 'obj', 'stats.o.usage.json')
    assert os.path.exists(path), 'build() compiled csrc/stats.hip but left no build/obj/stats.o.usage.json'
    usage = json.load(open(path))
    kernels = [k for k in usage if 'stats_' in k]
    assert len(kernels) == 5, kernels        # moments_chunks, moments_finish, count<ValueBins>, count<DigitBins>, select_pick
    assert all(usage[k]['spill'] == 0 for k in kernels), usage
