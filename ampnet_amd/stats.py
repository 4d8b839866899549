"""Statistics of tensors where they lie (csrc/stats.hip): counts of finite / NaN / infinite / zero / negative elements,
min, max, fp64 moments, a histogram and exact order statistics, for a whole list of tensors in a handful of launches and
ONE read-back.

The reference's diagnostics (src/ampnet/module/amp_gcn.py:278-405) copy every weight gradient and five [N, L*D]
activation tensors to the host and run seaborn / numpy on them.  A plot needs a few dozen numbers per tensor:

    pending = tensor_stats({'conv1': h1, 'conv2': h2}, bins=50, median=True)     # launches on the current stream, returns
    ...                                                                          # at once; queue as many as you like
    for name, s in pending.read().items():                                       # the only synchronisation
        print(name, s['mean'], s['std'], s['median'], s['zeros'] / s['numel'], s['nan'] + s['inf'])

What is counted how -- elements are classified from their bits, only finite ones enter min / max / the sums / the
histogram / the selection; the bin rule; the rank of a quantile -- is fixed in include/ampconv.h, "tensor statistics".
There is no `mode` (amp_gcn.py:297): on continuous data it is the minimum, on ReLU output it is 0, and `zeros` says that.
float32 or bfloat16 contiguous tensors on one GPU; no CPU or eager fallback.
"""
import ctypes
from collections.abc import Mapping

import numpy as np
import torch

from . import _lib
from .graph import _stream

CHUNK = _lib.STATS_CHUNK                 # elements one workgroup handles per iteration (AMPCONV_STATS_CHUNK)
MAX_TENSORS = _lib.STATS_MAX_TENSORS     # descriptors per launch; more tensors take further batches of launches
MAX_BINS = _lib.STATS_MAX_BINS
MAX_RANKS = _lib.STATS_MAX_RANKS         # order statistics per call, the median included

_SUPPORTED = ('tensor_stats supports contiguous float32 or bfloat16 tensors on one GPU, 0 <= bins <= '
              f'{MAX_BINS} and at most {MAX_RANKS} order statistics, the median included (ampnet_amd has no CPU or eager '
              'fallback)')
# ampconv_stats_record_t
RECORD = np.dtype([('numel', '<i8'), ('finite', '<i8'), ('nan', '<i8'), ('inf', '<i8'), ('zero', '<i8'), ('negative', '<i8'),
                   ('sum', '<f8'), ('sum_abs', '<f8'), ('sum_sq', '<f8'), ('min', '<f4'), ('max', '<f4'), ('absmax', '<f4'),
                   ('reserved', '<f4')])
assert RECORD.itemsize == _lib.STATS_RECORD_BYTES


def _round8(n):
    return (n + 7) & ~7


class TensorStats:
    """The pending result of one tensor_stats call: its launches are enqueued, its numbers are on the device.  `read()`
    copies them to the host -- one copy, the only synchronisation -- and returns them; any number of TensorStats may be
    outstanding.  `names`: the keys of a mapping, else None."""

    def __init__(self, keys, kind, numels, bins, quantiles, median, out, sections, done=None):
        self.names = keys
        self._kind, self._numels, self.bins, self.quantiles, self.median = kind, numels, bins, quantiles, median
        self._out, self._sections, self._done = out, sections, done
        self._result = None

    def __len__(self):
        return len(self._numels)

    def read(self):
        """Per tensor a dict: numel, finite, nan, inf, zeros, negative (counts; zeros: +0 and -0, negative: finite x < 0);
        min, max, absmax (exact; NaN without a finite element); mean, absmean, std (unbiased, n - 1, NaN for n <= 1) over
        the finite elements; with bins: hist (uint64 numpy array), edges (bins + 1 float64), below, above; with median:
        median (torch.median's lower median, an element of the tensor); with quantiles: quantiles (a list, numpy's method
        'lower').  Returned as the call was made: one dict for one tensor, a list for a sequence, {name: dict} for a
        mapping.  Synchronises the first time; later calls return the same object."""
        if self._result is not None:
            return self._result
        n, bins = len(self._numels), self.bins
        if self._done is not None:
            self._done.synchronize()                                        # the launches ran on the stream of the call
        host = self._out.cpu().numpy()                                      # the one read-back
        self._out = self._done = None
        at = self._sections
        rec = host[at['records']:at['records'] + n * RECORD.itemsize].view(RECORD)
        counts = host[at['counts']:at['counts'] + n * (bins + 2) * 8].view(np.uint64).reshape(n, bins + 2) if bins else None
        rng = host[at['range']:at['range'] + n * 8].view(np.float32).reshape(n, 2) if 'range' in at else None
        nq = len(self.quantiles) + int(self.median)
        sel = host[at['select']:at['select'] + n * nq * 4].view(np.float32).reshape(n, nq) if nq else None
        rows = []
        nan = float('nan')
        for i in range(n):
            r = rec[i]
            f = int(r['finite'])
            mean = float(r['sum']) / f if f else nan
            var = (float(r['sum_sq']) - float(r['sum']) * float(r['sum']) / f) / (f - 1) if f > 1 else nan
            row = {'numel': int(r['numel']), 'finite': f, 'nan': int(r['nan']), 'inf': int(r['inf']),
                   'zeros': int(r['zero']), 'negative': int(r['negative']),
                   'min': float(r['min']), 'max': float(r['max']), 'absmax': float(r['absmax']),
                   'mean': mean, 'absmean': float(r['sum_abs']) / f if f else nan,
                   'std': float(np.sqrt(max(var, 0.0))) if f > 1 else nan}
            if bins:
                lo, hi = (rng[i] if rng is not None else (r['min'], r['max']))
                row['hist'] = counts[i, :bins].copy()
                row['edges'] = np.linspace(float(lo), float(hi), bins + 1)
                row['below'], row['above'] = int(counts[i, bins]), int(counts[i, bins + 1])
            if self.median:
                row['median'] = float(sel[i, 0])
            if self.quantiles:
                row['quantiles'] = [float(v) for v in sel[i, int(self.median):]]
            rows.append(row)
        if self._kind == 'one':
            self._result = rows[0]
        elif self._kind == 'map':
            self._result = dict(zip(self.names, rows))
        else:
            self._result = rows
        return self._result


def _host_range(range, n, keys):
    """[n, 2] float32 host array of a (lo, hi) pair, or of one pair per tensor (sequence, or mapping by name)."""
    if isinstance(range, Mapping):
        if keys is None or set(range) != set(keys):
            raise ValueError('range given by name needs the names of the tensors')
        range = [range[k] for k in keys]
    a = np.asarray(range, dtype=np.float32)
    if a.shape == (2,):
        a = np.broadcast_to(a, (n, 2))
    if a.shape != (n, 2):
        raise ValueError(f'range has to be (lo, hi) or one such pair per tensor, got shape {a.shape} for {n} tensors')
    if not np.isfinite(a).all() or (a[:, 1] < a[:, 0]).any():
        raise ValueError('range needs finite lo <= hi')
    return np.array(a, dtype=np.float32, order='C', copy=True)          # writable: torch.from_numpy wants that


def tensor_stats(tensors, bins=0, range=None, median=False, quantiles=()):
    """Statistics of one tensor, a sequence of tensors or a {name: tensor} mapping; returns a TensorStats at once (the
    launches are on the current stream, nothing synchronises; `read()` does).

    bins: 0 (no histogram) .. MAX_BINS equal bins over `range`: None -- each tensor's own finite [min, max], taken on the
    device from the pass before --, (lo, hi), one pair per tensor, or a float32 device tensor of shape [2] / [n, 2] (read
    on the device).  Elements outside count as `below` / `above`.  median, quantiles: exact order statistics, the lower
    median and numpy's method 'lower'; together at most MAX_RANKS.  A tensor with numel == 0 is legal: counts 0, the rest
    NaN.  More than MAX_TENSORS tensors are taken in further batches of launches.

    Neither the tensors nor the workspace are kept alive by the result.  That is safe for memory the caching allocator
    handed out on the calling stream (a freed block is not reused before the launches have run); a tensor that was
    allocated on ANOTHER stream needs the usual `t.record_stream(torch.cuda.current_stream())` before it is freed."""
    if isinstance(tensors, torch.Tensor):
        kind, keys, items = 'one', None, [tensors]
    elif isinstance(tensors, Mapping):
        kind, keys, items = 'map', list(tensors.keys()), list(tensors.values())
    else:
        kind, keys, items = 'seq', None, list(tensors)
    bins = int(bins)
    if not 0 <= bins <= MAX_BINS:
        raise ValueError(f'bins={bins}; {_SUPPORTED}')
    quantiles = tuple(float(q) for q in quantiles)
    if any(not 0.0 <= q <= 1.0 for q in quantiles):
        raise ValueError(f'quantiles have to lie in [0, 1], got {quantiles}')
    qs = ((0.5,) if median else ()) + quantiles
    if len(qs) > MAX_RANKS:
        raise ValueError(f'{len(qs)} order statistics were asked for; {_SUPPORTED}')
    device = None
    for t in items:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'got a {type(t).__name__}; {_SUPPORTED}')
        if not t.is_cuda:
            raise ValueError(f'a tensor is on {t.device}, not on the GPU; {_SUPPORTED}')
        if t.dtype not in _lib.DTYPES:
            raise ValueError(f'a tensor is {t.dtype}; {_SUPPORTED}')
        if not t.is_contiguous():
            raise ValueError(f'a tensor of shape {tuple(t.shape)} is not contiguous; {_SUPPORTED}')
        if device is None:
            device = t.device
        elif t.device != device:
            raise ValueError(f'tensors on {device} and {t.device}; {_SUPPORTED}')
    n = len(items)
    if n == 0:
        return TensorStats(keys, kind, [], bins, quantiles, bool(median), torch.empty(0, dtype=torch.uint8),
                           {'records': 0, 'counts': 0, 'select': 0})
    device_range = isinstance(range, torch.Tensor)
    if device_range:
        if range.dtype != torch.float32 or range.device != device or tuple(range.shape) not in ((2,), (n, 2)):
            raise ValueError(f'a device range has to be a float32 tensor of shape [2] or [{n}, 2] on {device}, got '
                             f'{range.dtype} {tuple(range.shape)} on {range.device}')
    elif range is not None:
        range = _host_range(range, n, keys)
    if range is not None and not bins:
        raise ValueError('range was given without bins')
    # one device buffer for everything that is read back: records | counts | range | order statistics
    sections, size = {}, 0
    for name, nbytes in (('records', n * RECORD.itemsize), ('counts', n * (bins + 2) * 8 if bins else 0),
                         ('range', n * 8 if range is not None else -1), ('select', n * len(qs) * 4)):
        if nbytes >= 0:
            sections[name] = size
            size += _round8(nbytes)
    lib = _lib.load()
    table = (_lib.StatsTensor * n)(*[(t.data_ptr() if t.numel() else None, t.numel(), _lib.DTYPES[t.dtype]) for t in items])
    with torch.cuda.device(device):
        out = torch.zeros(size, dtype=torch.uint8, device=device)            # the counts start at zero
        base = out.data_ptr()
        ws = torch.empty(lib.ampconv_stats_workspace_bytes(table, n), dtype=torch.uint8, device=device)
        stream = _stream()
        records = base + sections['records']
        _lib.check(lib.ampconv_stats_moments(table, n, records, ws.data_ptr(), ws.numel(), stream), 'ampconv_stats_moments')
        if bins:
            rng = None
            if range is not None:
                view = out[sections['range']:sections['range'] + n * 8].view(torch.float32).view(n, 2)
                view.copy_(range.expand(n, 2) if device_range else torch.from_numpy(range), non_blocking=True)
                rng = base + sections['range']
            _lib.check(lib.ampconv_stats_histogram(table, n, bins, rng, records, base + sections['counts'], stream),
                       'ampconv_stats_histogram')
        if qs:
            q = (ctypes.c_double * len(qs))(*qs)
            _lib.check(lib.ampconv_stats_select(table, n, q, len(qs), records, base + sections['select'], ws.data_ptr(),
                                                ws.numel(), stream), 'ampconv_stats_select')
        done = torch.cuda.Event()
        done.record()                                                        # read() may be called under another stream
    # neither the inputs nor the workspace are kept: the allocator is stream-ordered, a block freed now is not handed out
    # again before the launches above have run (a queue of pending results must not pin a batch's activations)
    return TensorStats(keys, kind, [t.numel() for t in items], bins, quantiles, bool(median), out, sections, done)
