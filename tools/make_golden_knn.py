#!/usr/bin/env python3
"""tests/golden/knn/knn_xor_*.npz from the REFERENCE's graph construction (synthetic_benchmark/synthetic_xor.py:24-101:
create_duplicated_xor_data, scikit-learn's NearestNeighbors behind it), for ampnet_amd.knn_graph.

TEST INFRASTRUCTURE; runs on the CPU where the reference checkout and scikit-learn are (as oracle/make_golden.py does).
The reference file is loaded unmodified by file path and nothing of it is copied: a fixture holds the data its function
returned for a seed -- x (float32, exactly as returned), y, edge_index -- with k, feature_repeats, seed and two numbers:

    bound = (D + 4) 2^-24 2 max|x|^2    a worst-case bound B on the error of the fp32 expansion |a|^2 + |b|^2 - 2 <a, b>
    gap   = the smallest fp64 difference between any row's (k + 1)-th and (k + 2)-th nearest squared distance, the fp64
            distances taken from the float32 x as stored

A fixture that a test compares for EXACT edge_index equality needs gap >= 4 B (asserted here): then no fp32 evaluation of
the expansion can swap a row's last neighbour with the first one left out.  knn_xor_400 (the reference's own size) has no
such seed below 200; it is written with exact = 0 and held to the all-rows optimality check instead.

The fixtures live in tests/golden/knn/: conftest.golden_files() takes every tests/golden/*.npz for an AMPConv layer.

    python tools/make_golden_knn.py [--reference DIR]
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.join(ROOT, 'tests', 'golden', 'knn')

#         name            n    k  feature_repeats seed exact
CASES = (('knn_xor_64', 64, 3, 1, 3, True),
         ('knn_xor_128', 128, 10, 5, 2, True),
         ('knn_xor_400', 400, 10, 5, 1, False))


def load_reference(ref_dir):
    for name in ('networkx', 'matplotlib', 'matplotlib.pyplot'):       # plotting only: stand-ins if not installed
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    spec = importlib.util.spec_from_file_location('ref_synthetic_xor', os.path.join(ref_dir, 'synthetic_benchmark', 'synthetic_xor.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def gap_and_bound(x, k):
    x64 = x.astype(np.float64)
    d2 = np.sort(((x64[:, None, :] - x64[None, :, :]) ** 2).sum(2), axis=1)       # the node itself at column 0
    gap = float((d2[:, k + 1] - d2[:, k]).min())
    bound = float((x.shape[1] + 4) * 2.0 ** -24 * 2.0 * float((x64 * x64).sum(1).max()))
    return gap, bound


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    args = ap.parse_args(argv)
    ref = load_reference(args.reference)
    os.makedirs(OUT_DIR, exist_ok=True)
    for name, n, k, repeats, seed, exact in CASES:
        np.random.seed(seed)
        x, y, _, edge_index = ref.create_duplicated_xor_data(num_samples=n, num_nearest_neighbors=k, feature_repeats=repeats)
        x, y, edge_index = x.numpy(), y.numpy(), edge_index.numpy()
        assert x.dtype == np.float32 and edge_index.shape == (2, n * (k + 1)), (x.dtype, edge_index.shape)
        gap, bound = gap_and_bound(x, k)
        if exact:
            assert gap >= 4 * bound, f'{name}: gap {gap:.3e} < 4 B = {4 * bound:.3e}: pick another seed'
        np.savez(os.path.join(OUT_DIR, name + '.npz'), x=x, y=y, edge_index=edge_index.astype(np.int64), k=np.int64(k),
                 feature_repeats=np.int64(repeats), seed=np.int64(seed), gap=np.float64(gap), bound=np.float64(bound),
                 exact=np.int64(exact))
        print(f'{name}: x {x.shape}, E {edge_index.shape[1]}, gap {gap:.3e}, B {bound:.3e}, gap / B {gap / bound:.3g}, '
              f'exact {int(exact)}')


if __name__ == '__main__':
    main()
