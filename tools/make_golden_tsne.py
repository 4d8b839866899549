#!/usr/bin/env python3
"""tests/golden/tsne/tsne_*.npz: seeded Gaussian blobs and what scikit-learn's t-SNE code returns for them, stage by
stage, for tests/test_tsne_cpu.py and tests/test_gpu_tsne.py.

TEST INFRASTRUCTURE; runs on the CPU where scikit-learn is installed (written with 1.7.2, whose private functions it
calls: _utils._binary_search_perplexity, _t_sne._joint_probabilities_nn, _t_sne._kl_divergence_bh).  Per fixture:

    x                      the input as the library takes it, float32 (blobs on a 2^-5 grid: the file stays small);
                           samples='columns' fixtures hold [features, samples] and scikit-learn gets x^T
    nbr_idx, nbr_dist2     NearestNeighbors' k = min(M - 1, int(3 perplexity + 1)) neighbours, nearest first, and the
                           squared distances as float32, the dtype _joint_probabilities_nn hands to the search
    cond_p                 _binary_search_perplexity(nbr_dist2, perplexity), stored as float32 in the format of
                           ampconv_tsne_affinities (tsne_reference.cond_f32: a positive value never as 0)
    indptr, indices, val   _joint_probabilities_nn's CSR; val float32, as _kl_divergence_bh reads it
    head                   float32 probabilities do not compress and a file has to stay under 100 kB: nbr_dist2 and cond_p
                           hold the first `head` rows and val the entries of those rows (indptr[head] of them).  The ids
                           -- nbr_idx, indptr, indices -- are whole, and val is normalised by the sum over ALL rows
    y_wide, y_start        seeded embeddings at scale 3 and 1e-4; grad_*, err_*: _kl_divergence_bh(angle=0.0) on them
    kl_auto, kl_lr10       TSNE(init='pca', random_state=s).kl_divergence_ for s = 0..3 at learning_rate='auto' / 10
    emb_auto               the embedding of s = 0 at 'auto'
    search_agreement       max |search_model - scikit-learn| over cond_p in fp64, before the float32 rounding
    gradient_agreement     max |gradient_model - _kl_divergence_bh| over both embeddings (scikit-learn's side is fp32)
    search_margin          tests/tsne_reference.search_model's margin on nbr_dist2
    gap, bound             the smallest fp64 difference between any sample's k-th and (k + 1)-th nearest squared distance,
                           and B = (P + 4) 2^-24 2 max|x|^2, the worst-case error of an fp32 evaluation of |a|^2 + |b|^2 -
                           2 <a, b> (tools/make_golden_knn.py).  gap > 2 B is asserted: no such evaluation can swap a
                           sample's last neighbour with the first one left out, so the CSR's ids are pinned exactly

The fixtures live in tests/golden/tsne/: conftest.golden_files() takes every tests/golden/*.npz for an AMPConv layer.

    python tools/make_golden_tsne.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import sklearn
    from scipy.sparse import csr_matrix
    from sklearn.manifold import TSNE, _t_sne, _utils
    from sklearn.neighbors import NearestNeighbors
    import tsne_reference as tr
    os.makedirs(tr.GOLDEN_DIR, exist_ok=True)
    for name, shape, perplexity, samples, seed, head in tr.CASES:
        M, P = shape if samples == 'rows' else shape[::-1]
        X32 = (np.round(tr.blobs(M, P, seed) * 32) / 32).astype(np.float32)
        x = X32 if samples == 'rows' else np.ascontiguousarray(X32.T)
        assert x.shape == shape
        X = X32.astype(np.float64)
        k = min(M - 1, int(3.0 * perplexity + 1))
        nn = NearestNeighbors(n_neighbors=k).fit(X)
        dist, idx = nn.kneighbors()
        d2 = (dist ** 2).astype(np.float32)
        _, far = tr.exact_neighbors(X, k + 1) if k + 1 < M else (None, None)
        gap = float((far[:, k] - far[:, k - 1]).min()) if far is not None else np.inf
        bound = float((P + 4) * 2.0 ** -24 * 2.0 * (X * X).sum(1).max())
        assert gap > 2 * bound, f'{name}: gap {gap:.3e} <= 2 B = {2 * bound:.3e}: pick another seed'
        cond = _utils._binary_search_perplexity(d2, perplexity, 0)
        model, _, margin = tr.search_model(d2, perplexity)
        search_agreement = float(np.abs(model - cond).max())

        graph = nn.kneighbors_graph(mode='distance')
        graph.data **= 2
        Pj = _t_sne._joint_probabilities_nn(graph, perplexity, 0)
        Pj.sort_indices()
        indptr, indices, val = Pj.indptr.astype(np.int64), Pj.indices.astype(np.int64), Pj.data.astype(np.float32)
        mp, mi, mv = tr.joint_model(idx, cond)
        assert np.array_equal(mp, indptr) and np.array_equal(mi, indices), name
        joint_agreement = float(np.abs(mv / Pj.data - 1).max())

        rng = np.random.default_rng(seed + 1000)
        out, gradient_agreement = {}, 0.0
        for tag, scale in (('wide', 3.0), ('start', 1e-4)):
            y = (rng.normal(0.0, scale, (M, 2))).astype(np.float32)
            Pcsr = csr_matrix((val, indices, indptr), shape=(M, M))
            err, grad = _t_sne._kl_divergence_bh(y.ravel().copy(), Pcsr, 1, M, 2, angle=0.0, skip_num_points=0, verbose=False,
                                                 compute_error=True, num_threads=1)
            merr, mgrad = tr.gradient_model(y, indptr, indices, val)
            gradient_agreement = max(gradient_agreement, float(np.abs(mgrad - grad.reshape(M, 2)).max()))
            out['y_' + tag], out['grad_' + tag], out['err_' + tag] = y, grad.reshape(M, 2).astype(np.float32), np.float64(err)
            out['err_model_' + tag] = np.float64(merr)

        kl = {}
        for tag, lr in (('auto', 'auto'), ('lr10', 10.0)):
            fits = [TSNE(n_components=2, perplexity=perplexity, learning_rate=lr, init='pca', random_state=s).fit(X) for s in range(4)]
            kl[tag] = np.array([f.kl_divergence_ for f in fits])
            if tag == 'auto':
                out['emb_auto'] = fits[0].embedding_.astype(np.float32)
        path = os.path.join(tr.GOLDEN_DIR, name + '.npz')
        np.savez_compressed(path, x=x, samples=np.array(samples), perplexity=np.float64(perplexity), k=np.int64(k),
                            head=np.int64(head), nbr_idx=idx.astype(np.int16), nbr_dist2=d2[:head], cond_p=tr.cond_f32(cond[:head]),
                            indptr=indptr.astype(np.int32), indices=indices.astype(np.int16), val=val[:indptr[head]],
                            kl_auto=kl['auto'], kl_lr10=kl['lr10'],
                            search_agreement=np.float64(search_agreement), gradient_agreement=np.float64(gradient_agreement),
                            joint_agreement=np.float64(joint_agreement), search_margin=np.float64(margin), gap=np.float64(gap), bound=np.float64(bound),
                            sklearn_version=np.array(sklearn.__version__), **out)
        print(f'{name}: x {x.shape} {samples}, k {k}, nnz {indices.size}, search {search_agreement:.2e} (margin {margin:.2e}), '
              f'gap / B {gap / bound:.3g}, joint {joint_agreement:.2e}, gradient {gradient_agreement:.2e}, err {float(out["err_wide"]):.6f} / model '
              f'{float(out["err_model_wide"]):.6f}, kl auto {kl["auto"].round(4)}, lr10 {kl["lr10"].round(4)}, '
              f'{os.path.getsize(path)} bytes')
        assert os.path.getsize(path) < 100_000, path


if __name__ == '__main__':
    main()
