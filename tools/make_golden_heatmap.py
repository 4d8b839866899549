"""Generate tests/golden/heatmap/heatmap_*.npz with the REFERENCE's calculate_attn_heatmap.

TEST INFRASTRUCTURE; runs only where the reference checkout is present (REF below, or AMPNET_REFERENCE in the
environment).  experiments/visualize_cora_attn_coeffs.py is parsed with `ast` and ONLY the definitions of
calculate_attn_heatmap and get_edge_indices_between_nodes are executed (the script's imports -- seaborn, the Cora
download -- are never run), as oracle/make_golden_ampgcn.py loads its class by path.  Nothing of their text is here.

Each fixture is built on an existing golden that carries the reference's own attn_output_weights (for all its edges, or
for the subset `w_edges`, which is then the edge mask), so the chain reference weights -> reference function -> fixture
holds.  (A directory of their own: tests/conftest.py's golden_files() takes every *.npz directly under tests/golden
for a layer fixture.)  Stored per fixture (data only):
  base              name of the golden it belongs to
  token_features    [N, L] seeded feature ids, drawn WITH replacement inside a node (repeats occur)
  node_class        [N]
  edge_mask         [E] bool: the edges the golden has weights for
  src_features, dst_features, src_class, dst_class
  heat_class        the reference function's table for that class pair, cropped to [len(src), len(dst)]
  all_features      the sorted ids in use; heat_all [A, A]: the same function with every class collapsed to one and
                    every feature selected (the reference's table is fixed at 30 x 30, so it is called once per
                    30 x 30 block of feature ids)

    python tools/make_golden_heatmap.py
"""
import ast
import os
import types

import numpy as np
import torch

REF = os.environ.get('AMPNET_REFERENCE', '/root/reference')
SCRIPT = os.path.join(REF, 'experiments', 'visualize_cora_attn_coeffs.py')
OUT_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
WANTED = ('calculate_attn_heatmap', 'get_edge_indices_between_nodes')


def load_reference_functions():
    tree = ast.parse(open(SCRIPT).read(), SCRIPT)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(d.name for d in defs) == sorted(WANTED)
    ns = {'np': np, 'torch': torch}
    exec(compile(ast.Module(body=defs, type_ignores=[]), SCRIPT, 'exec'), ns)
    return ns['calculate_attn_heatmap']


def reference_table(calc, W, tok, edge_index, cls, src, dst, src_class, dst_class):
    """The reference's table for feature lists of any length: one call per block of at most 30 x 30 ids."""
    data = types.SimpleNamespace(edge_index=torch.from_numpy(edge_index), y=torch.from_numpy(cls))
    out = np.zeros((len(src), len(dst)))
    for r0 in range(0, len(src), 30):
        for c0 in range(0, len(dst), 30):
            rs, cs = src[r0:r0 + 30], dst[c0:c0 + 30]
            block = calc(W, tok, data, rs, cs, src_class, dst_class)
            out[r0:r0 + len(rs), c0:c0 + len(cs)] = block[:len(rs), :len(cs)]
    return out


# base golden, vocabulary size, number of selected source / destination features, classes, seed
CASES = [('cora_L20_D128_H4', 60, 30, 30, 2, 0),
         ('wide_L4_D64_H8', 14, 9, 8, 2, 0),
         ('cfg3_L20_D128_H8', 40, 30, 28, 2, 0),
         ('ampgcn_L40_D100_H2', 40, 24, 30, 2, 0)]


def make(calc, base, vocab, n_src, n_dst, n_cls, seed):
    z = np.load(os.path.join(OUT_DIR, base + '.npz'))
    N, L = int(z['N']), int(z['L'])
    edge_index, w_edges, W = z['edge_index'], z['w_edges'], z['attn_output_weights'].astype(np.float64)
    E = edge_index.shape[1]
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(200, size=vocab, replace=False)).astype(np.int64)      # the feature ids in use
    tok = ids[rng.integers(0, vocab, size=(N, L))]
    cls = rng.integers(0, n_cls, size=N).astype(np.int64)
    src = rng.permutation(ids)[:n_src]
    dst = rng.permutation(ids)[:n_dst]
    mask = np.zeros(E, dtype=bool)
    mask[w_edges] = True
    sub = edge_index[:, w_edges]                                                     # the edges W belongs to, in W's order
    pairs = [(a, b) for a in range(n_cls) for b in range(n_cls)]
    counts = [int(((cls[sub[0]] == a) & (cls[sub[1]] == b)).sum()) for a, b in pairs]
    src_class, dst_class = pairs[int(np.argmax(counts))]
    heat_class = reference_table(calc, W, tok, sub, cls, src, dst, src_class, dst_class)
    one = np.zeros(N, dtype=np.int64)
    heat_all = reference_table(calc, W, tok, sub, one, ids, ids, 0, 0)
    for name, t in (('heat_class', heat_class), ('heat_all', heat_all)):
        frac = float((t != 0).mean())
        assert frac >= 1 / 3, f'{base}: only {frac:.2f} of {name} is non-zero, pick another seed'
        print(f'{base}: {name} {t.shape}, {100 * frac:.0f} % non-zero, {max(counts)} edges in the class pair')
    assert any(len(set(row)) < L for row in tok.tolist()) or L == 1
    os.makedirs(os.path.join(OUT_DIR, 'heatmap'), exist_ok=True)
    np.savez_compressed(os.path.join(OUT_DIR, 'heatmap', f'heatmap_{base}.npz'), base=np.array(base), token_features=tok,
                        node_class=cls, edge_mask=mask, src_features=src, dst_features=dst,
                        src_class=np.int64(src_class), dst_class=np.int64(dst_class), heat_class=heat_class,
                        all_features=ids, heat_all=heat_all)


if __name__ == '__main__':
    calc = load_reference_functions()
    for case in CASES:
        make(calc, *case)
