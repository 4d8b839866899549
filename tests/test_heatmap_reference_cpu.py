"""Pins tests/heatmap_reference.py -- the fp64 model and the bar of tests/test_gpu_heatmap_kernel.py -- three ways: on the
reference's fixtures (tests/golden/heatmap/) the model, fed Q and K projected in float64, reproduces the recorded
attention weights, the counts of test_heatmap_cpu.heat_restatement and both recorded tables; on a hand-made graph every
selection rule of include/ampconv.h is checked against weights written out in closed form; and the bar rejects a count
off by one, one weight off by 2e-5, a transposed edge and a row map read against the column extent, while it passes the
float32-rounded model.  No kernel runs here."""
import os

import numpy as np
import pytest

import heatmap_reference as hr
import linear_reference as lr
from test_heatmap_cpu import HEATMAP_FIXTURES, class_selection, heat_restatement, load_heatmap_fixture


def flat_share(got, ref):
    """Share of the project's flat bar (conftest.ATOL, RTOL) that |got - ref| uses."""
    return float((np.abs(got - ref) / (lr.ATOL + lr.RTOL * np.abs(ref))).max())


def positions(tok, features):
    pos = np.full(int(max(tok.max(), np.max(features))) + 1, -1, np.int32)
    pos[np.asarray(features)] = np.arange(len(features))
    return pos[tok]


@pytest.mark.parametrize('path', HEATMAP_FIXTURES, ids=[os.path.basename(p)[:-4] for p in HEATMAP_FIXTURES])
def test_model_reproduces_the_reference_fixtures(path):
    f, g = load_heatmap_fixture(path)
    N, L, D, H = (int(g[k]) for k in 'NLDH')
    x = g['x'].astype(np.float64).reshape(N * L, D)
    Wi, bi = g['in_proj_weight'].astype(np.float64), g['in_proj_bias'].astype(np.float64)
    Q = (x @ Wi[:D].T + bi[:D]).reshape(N, L, H, D // H)
    K = (x @ Wi[D:2 * D].T + bi[D:2 * D]).reshape(N, L, H, D // H)
    src, dst = g['edge_index']
    we = g['w_edges']
    used = flat_share(lr.attn_weights(Q, K, src[we], dst[we])[0], g['attn_output_weights'])
    print(f'[bar] attn_weights vs fixture: {100 * used:.1f} % of the flat bar')
    assert used <= 1
    W = np.zeros((len(src),) + g['attn_output_weights'].shape[1:])
    W[we] = g['attn_output_weights']
    tok, weights = f['token_features'], {}
    for name, rf, cf, sel in (('heat_class', f['src_features'], f['dst_features'], class_selection(f, g['edge_index'])),
                              ('heat_all', f['all_features'], f['all_features'], f['edge_mask'])):
        S, cnt = hr.heat_tables(Q, K, src, dst, N, sel.astype(np.uint8), positions(tok, rf), positions(tok, cf),
                                len(rf), len(cf), weights=weights)
        _, cnt_ref, _ = heat_restatement(W, tok, g['edge_index'], rf, cf, sel)
        assert np.array_equal(cnt, cnt_ref), name
        assert hr.coverage(cnt) >= 1 / 3
        heat = np.divide(S, cnt, out=np.zeros_like(S), where=cnt != 0)
        used = flat_share(heat, f[name])
        print(f'[bar] {name}: {100 * used:.1f} % of the flat bar')
        assert used <= 1, name


# ---------------------------------------------------------------------------------------- the hand-made case
# 3 nodes, L = 2, H = 1, dh = 1: the score of (destination token i of d, source token j of s) is q[d][i] k[s][j], so
# W[i, j] = exp(q[d][i] k[s][j]) / sum_j' exp(q[d][i] k[s][j']) in closed form.  ln 3 and ln 7 give the weights
# 1/4, 3/4 and 1/8, 7/8 against a zero; a zero query gives 1/2, 1/2.
LN3, LN7 = np.log(3.0), np.log(7.0)
HQ = np.array([[0.0, 1.0], [1.0, -1.0], [1.0, 1.0]])
HK = np.array([[0.0, LN3], [LN7, 0.0], [LN3, LN7]])
HSRC, HDST = np.array([0, 1, 1, 2, 2]), np.array([1, 2, 2, 0, 2])          # (1 -> 2) twice: a multi-edge; a self-loop
# rows = 2, cols = 3.  Node 0 holds ONE source feature twice (row 1, row 1); node 2's source token 1 sits at position
# 2 = rows: not selected as a row although 2 < cols; node 2's destination token 0 sits at 2: a valid column.
HROW = np.array([[1, 1], [0, 1], [1, 2]], np.int32)
HCOL = np.array([[0, 1], [1, 0], [2, -1]], np.int32)
HROWS, HCOLS = 2, 3


def hand_w(s, d, i, j):
    p = [np.exp(HQ[d][i] * HK[s][jj]) for jj in range(2)]
    return p[j] / (p[0] + p[1])


def hand_tables(edges, rowpos=HROW, colpos=HCOL, rows=HROWS, cols=HCOLS):
    """The rule, term by term, over the listed edge ids."""
    S, cnt = np.zeros((rows, cols)), np.zeros((rows, cols), np.int64)
    for e in edges:
        s, d = HSRC[e], HDST[e]
        for i in range(2):
            for j in range(2):
                r, c = rowpos[s][j], colpos[d][i]
                if 0 <= r < rows and 0 <= c < cols:
                    S[r, c] += hand_w(s, d, i, j)
                    cnt[r, c] += 1
    return S, cnt


def hand_call(src=HSRC, dst=HDST, mask=None, **kw):
    Q, K = HQ.reshape(3, 2, 1, 1), HK.reshape(3, 2, 1, 1)
    return hr.heat_tables(Q, K, src, dst, 3, mask, kw.get('rowpos', HROW), kw.get('colpos', HCOL), kw.get('rows', HROWS),
                          kw.get('cols', HCOLS))


def same(got, want):
    return np.array_equal(got[1], want[1]) and np.abs(got[0] - want[0]).max() <= 1e-15


def test_closed_form_weights_are_the_models():
    W = lr.attn_weights(HQ.reshape(3, 2, 1, 1), HK.reshape(3, 2, 1, 1), HSRC, HDST)[0]
    for e in range(5):
        for i in range(2):
            for j in range(2):
                assert abs(W[e, i, j] - hand_w(HSRC[e], HDST[e], i, j)) <= 1e-15
    assert abs(W[0, 0, 1] - 0.75) <= 1e-15 and abs(W[1, 0, 0] - 0.875) <= 1e-15       # (0 -> 1): q = 1; (1 -> 2): q = 1
    assert W[3, 0, 0] == 0.5                                                          # (2 -> 0): q = 0


def test_selection_rules_on_the_hand_made_case():
    full = hand_tables(range(5))
    assert same(hand_call(), full) and hr.coverage(full[1]) >= 1 / 3
    # a masked edge: any non-zero byte selects
    for e in range(5):
        mask = np.array([1, 2, 255, 1, 128], np.uint8)
        mask[e] = 0
        assert same(hand_call(mask=mask), hand_tables([k for k in range(5) if k != e])), e
    assert same(hand_call(mask=np.ones(5, np.uint8)), full)
    # a source id of -1, a destination id of N: ignored, whatever the other end is
    src, dst = HSRC.copy(), HDST.copy()
    src[0], dst[4] = -1, 3
    assert same(hand_call(src=src, dst=dst), hand_tables([1, 2, 3]))
    src, dst = HSRC.copy(), HDST.copy()
    src[3], dst[1] = 3, -1
    assert same(hand_call(src=src, dst=dst), hand_tables([0, 2, 4]))
    # position 2 = rows < cols: the self-loop (2 -> 2) has row position 2 on source token 1 (dropped) and column
    # position 2 on destination token 0 (kept); its other destination token is -1
    S, cnt = hand_call(src=HSRC[4:], dst=HDST[4:])
    want = np.zeros((2, 3))
    want[1, 2] = hand_w(2, 2, 0, 0)
    assert np.array_equal(cnt, (want != 0).astype(np.int64)) and np.abs(S - want).max() <= 1e-15
    # ... and with the extents exchanged the same positions select the other way round
    S, cnt = hand_call(src=HSRC[4:], dst=HDST[4:], rows=3, cols=2)
    assert cnt.sum() == 0 and not S.any()                    # column position 2 = cols is out, -1 is out
    # a feature held twice in a node counts once per token: node 0 -> 1 puts both source tokens into row 1
    S, cnt = hand_call(src=HSRC[:1], dst=HDST[:1])
    assert cnt.tolist() == [[0, 0, 0], [2, 2, 0]]
    assert abs(S[1, 1] - 1.0) <= 1e-15 and abs(S[1, 0] - 1.0) <= 1e-15      # a whole softmax row each
    # a multi-edge counts once per copy
    one, two = hand_call(src=HSRC[1:2], dst=HDST[1:2]), hand_call(src=HSRC[1:3], dst=HDST[1:3])
    assert np.array_equal(two[1], 2 * one[1]) and np.abs(two[0] - 2 * one[0]).max() <= 1e-15 and one[1].sum() > 0


# ------------------------------------------------------------------------------------------------------- the bar
def _case(shape=(20, 32, 4), N=6, E=24):
    L, dh, H = shape
    rng = np.random.default_rng(5)
    Q, K = lr.tiles('random', shape, N), lr.tiles('random', shape, N, seed=1)
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    W = lr.attn_weights(Q, K, src, dst)[0]
    return Q, K, src, dst, W


def test_share_rejects_what_it_must_and_passes_the_rounded_model():
    Q, K, src, dst, W = _case()
    N, L = Q.shape[:2]
    for rowpos, colpos, rows, cols in (hr.unique_maps(N, L), hr.selected_maps(N, L)[:4]):
        S, cnt = hr.accumulate(W, src, dst, rowpos, colpos, rows, cols)
        assert hr.coverage(cnt) >= 1 / 3
        sums = hr.accumulate(hr.quantised(W.astype(np.float32)), src, dst, rowpos, colpos, rows, cols, np.int64)[0]
        used = hr.share(sums, cnt, S, cnt)
        print(f'[bar] float32-rounded model, {rows} x {cols}: {100 * used:.2f} % of the bar')
        assert used <= 1
        r, c = np.argwhere(cnt > 0)[0]
        off = cnt.copy()
        off[r, c] += 1
        assert hr.share(sums, off, S, cnt) == np.inf
        assert (cnt == 0).any()
        stale = sums.copy()
        stale[cnt == 0] = 1                                   # a cell without a term must hold no sum
        assert hr.share(stale, cnt, S, cnt) == np.inf
        # one weight off by 2e-5 in a cell of one term whose weight leaves the relative part of the bar below 1e-5
        r, c = np.argwhere((cnt == 1) & (S < 0.09))[0]
        bad = sums.copy()
        bad[r, c] += int(2e-5 * 2 ** hr.SHIFT)
        assert hr.share(bad, cnt, S, cnt) > 1
    assert hr.share(np.zeros((2, 2), np.int64), np.zeros((2, 2), np.int64), np.zeros((2, 2)), np.zeros((2, 2), np.int64)) == 0.0


def test_bar_rejects_wrong_kernels():
    """The tables a subtly wrong kernel would give, built from the same weights: i and j swapped inside an edge; the row
    map read against the column extent; Q taken from the source and K from the destination; one token's head mean over
    H - 1 heads."""
    Q, K, src, dst, W = _case()
    N, L = Q.shape[:2]
    H = Q.shape[2]
    q = lambda w: hr.quantised(np.asarray(w).astype(np.float32))          # noqa: E731
    rowpos, colpos, rows, cols = hr.unique_maps(N, L)
    S, cnt = hr.accumulate(W, src, dst, rowpos, colpos, rows, cols)
    tables = lambda w, **k: hr.accumulate(q(w), k.get('src', src), k.get('dst', dst), k.get('rowpos', rowpos),   # noqa: E731
                                          k.get('colpos', colpos), rows, cols, np.int64)
    assert hr.share(*tables(W), S, cnt) <= 1
    assert hr.share(*tables(W.transpose(0, 2, 1)), S, cnt) > 1                               # i / j swapped
    assert hr.share(*tables(lr.attn_weights(K, Q, src, dst)[0]), S, cnt) > 1                 # operands exchanged
    short = W.copy()
    short[3, 5] *= (H - 1) / H                                                               # one token, one head lost
    assert hr.share(*tables(short), S, cnt) > 1
    # selected maps, rows = 48 < cols = 64
    rowpos, colpos, rows, cols, _ = hr.selected_maps(N, L)
    wild = rowpos.copy()
    wild[rowpos < 0] = np.arange((rowpos < 0).sum()) % 16 + 48          # 48..63: valid only as a column
    S, cnt = hr.accumulate(W, src, dst, wild, colpos, rows, cols)
    assert np.array_equal(cnt, hr.accumulate(W, src, dst, rowpos, colpos, rows, cols)[1])
    wide = hr.accumulate(q(W), src, dst, wild, colpos, cols, cols, np.int64)                 # rows held to `cols`
    assert wide[1][rows:].sum() > 0                                      # ... lands behind the table's last row
    assert hr.share(*hr.accumulate(q(W), src, dst, colpos, rowpos, rows, cols, np.int64), S, cnt) == np.inf   # maps exchanged
