"""Pins tests/linear_reference.py -- the per-call fp64 models and the bars the GPU tests of the softmax-free path and of
the node-side helpers use (tests/test_gpu_linear_kernels.py, tests/test_gpu_node_ops.py) -- two ways: the models,
composed in the order of ampnet_amd/conv/linear.py, reproduce the whole-layer oracle at fp64 round-off; and the bars
pass a float32 emulation of every kernel's arithmetic and reject the same emulation broken once per mutant.  No GPU."""
import numpy as np

import conftest
import edge_reference as er
import linear_reference as lr
from edge_layouts import layout_strides
from edge_runner import graph
from oracle.ampconv_numpy import AMPConvOracle, segment_mean as oracle_segment_mean

RTOL = 1e-12


def close(got, want, name):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print(f'{name}: max err {err:.3e} at max |want| {scale:.3e}')
    assert got.shape == want.shape and err <= RTOL * scale, name


def test_the_models_composed_as_the_layer_reproduce_the_oracle():
    """Graph A with the destinations' rows (xq) and the sources' rows (xkv) apart -- the oracle sees them as a graph of
    2 N nodes, edge (N + s -> d) -- so Q rows are not K / V rows: forward outer -> segment mean -> apply ->
    out-projection -> mask, backward its transpose, in the order of LinearAMPConvFunction's bipartite branch."""
    assert (lr.ATOL, lr.RTOL) == (conftest.ATOL, conftest.RTOL)
    g = graph('A')
    N, L, H, dh = g.N, 3, 2, 4
    D = H * dh
    rs = 1.0 / np.sqrt(dh)
    rng = np.random.default_rng(3)
    xq, xkv, dy = (rng.standard_normal((N, L * D)) for _ in range(3))
    Win, bin_, Wo, bo = (rng.standard_normal(s) * 0.3 for s in ((3 * D, D), (3 * D,), (D, D), (D,)))
    ei = np.stack([g.src + N, g.dst])
    o = AMPConvOracle(Win, bin_, Wo, bo, H, softmax=False)
    y_ref, w_ref = o.forward(np.concatenate([xq, xkv]), ei, need_weights=True)
    dx_ref, dWin_ref, dbin_ref, dWo_ref, dbo_ref = o.backward(np.concatenate([dy, rng.standard_normal((N, L * D))]))

    rowptr, col = er.csr_of(g.src, g.dst, N)
    cscptr, crow = er.csr_of(g.dst, g.src, N)                 # the source-sorted side: crow = destination of each edge
    cinv = 1.0 / g.indeg[crow]
    xq2, xkv2 = xq.reshape(N * L, D), xkv.reshape(N * L, D)
    Q = (xq2 @ Win[:D].T + bin_[:D]).reshape(N, L, H, dh)
    K = (xkv2 @ Win[D:2 * D].T + bin_[D:2 * D]).reshape(N, L, H, dh)
    V = (xkv2 @ Win[2 * D:].T + bin_[2 * D:]).reshape(N, L, H, dh)
    # forward
    M, _ = lr.linear_outer(K, V, 1.0)
    Mbar, _ = lr.gather_segment_sum(M.reshape(N, -1), rowptr, col, None, True)
    obar, _ = lr.linear_apply(Q, Mbar.reshape(N, H, dh, dh), False, rs)
    y = lr.mask_rows((obar.reshape(N * L, D) @ Wo.T + bo).reshape(N, L * D), rowptr)
    close(y, y_ref[:N], 'y')
    assert not y[g.indeg == 0].any() and not y_ref[N:].any()
    # backward
    dbo, _ = lr.masked_colsum(dy.reshape(N, L, D), rowptr)
    dWo = dy.reshape(N * L, D).T @ obar.reshape(N * L, D)                 # obar is 0 on the masked rows
    dO = lr.mask_rows((dy.reshape(N * L, D) @ Wo).reshape(N, L * D), rowptr).reshape(N, L, H, dh)
    dMbar, _ = lr.linear_outer(Q, dO, rs)
    dM, _ = lr.gather_segment_sum(dMbar.reshape(N, -1), cscptr, crow, cinv, False)
    dM = dM.reshape(N, H, dh, dh)
    dQ, _ = lr.linear_apply(dO, Mbar.reshape(N, H, dh, dh), True, rs)
    dK, _ = lr.linear_apply(V, dM, True, 1.0)
    dV, _ = lr.linear_apply(K, dM, False, 1.0)
    dq2, dk2, dv2 = (t.reshape(N * L, D) for t in (dQ, dK, dV))
    close(dq2 @ Win[:D], dx_ref[:N].reshape(N * L, D), 'dx (destinations)')
    close(dk2 @ Win[D:2 * D] + dv2 @ Win[2 * D:], dx_ref[N:].reshape(N * L, D), 'dx (sources)')
    close(np.concatenate([dq2.T @ xq2, dk2.T @ xkv2, dv2.T @ xkv2]), dWin_ref, 'dW_in')
    close(np.concatenate([dq2.sum(0), dk2.sum(0), dv2.sum(0)]), dbin_ref, 'db_in')
    close(dWo, dWo_ref, 'dW_out')
    close(dbo, dbo_ref, 'db_out')
    # the side outputs and the PyG mean
    W, S = lr.attn_scores(Q, K, g.src, g.dst)
    close(W, w_ref, 'attn_scores')
    assert (S >= np.abs(W) * (1 - 1e-12)).all()
    _, ws_ref = AMPConvOracle(Win, bin_, Wo, bo, H, softmax=True).forward(np.concatenate([xq, xkv]), ei)
    close(lr.attn_weights(Q, K, g.src, g.dst)[0], ws_ref, 'attn_weights')
    msg = rng.standard_normal((g.E, 5))
    eperm = np.argsort(g.dst, kind='stable')
    close(lr.segment_mean(msg, rowptr, eperm, 5)[0], oracle_segment_mean(msg, g.dst, N), 'segment_mean')


# ------------------------------------------------------------ float32 emulations of the kernels' arithmetic
f32 = np.float32


def fma(a, b, acc):
    """fmaf on float32 arrays (the product enters the sum unrounded)."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(f32)


def read_view(flat, strides, N, L, H, dh):
    """The logical [N, L, H, dh] tile a kernel reads through (node, row, head) strides."""
    ns, rs, hs = strides
    n, l, h, c = np.ix_(np.arange(N) * ns, np.arange(L) * rs, np.arange(H) * hs, np.arange(dh))
    return flat[n + l + h + c]


def emu_outer(A, B, scale):
    N, L, H, dh = A.shape
    acc = np.zeros((N, H, dh, dh), f32)
    for l in range(L):
        acc = fma(A[:, l, :, :, None], B[:, l, :, None, :], acc)
    return acc * f32(scale)


def emu_apply(A, M, transpose, scale):
    N, L, H, dh = A.shape
    m = M.transpose(0, 1, 3, 2) if transpose else M
    acc = np.zeros((N, L, H, dh), f32)
    for k in range(dh):
        acc = fma(A[:, :, :, k, None], m[:, None, :, k, :], acc)
    return acc * f32(scale)


def emu_gather(rows, ptr, idx, w, mean, drop_last_of_odd=False, ignore_w=False, wrong_length_row=None):
    """Two chains (even and odd positions of the segment), their sum times fl32(1 / length)."""
    out = np.zeros((len(ptr) - 1, rows.shape[1]), f32)
    for r in range(len(ptr) - 1):
        beg, end = int(ptr[r]), int(ptr[r + 1])
        stop = end - 1 if drop_last_of_odd and (end - beg) % 2 else end
        ab = [np.zeros(rows.shape[1], f32), np.zeros(rows.shape[1], f32)]
        for p in range(beg, stop):
            wp = f32(1) if w is None or ignore_w else f32(w[p])
            ab[(p - beg) % 2] = fma(np.full(rows.shape[1], wp, f32), rows[idx[p]], ab[(p - beg) % 2])
        n = end - beg + (1 if r == wrong_length_row else 0)
        sc = (f32(1) / f32(n) if end > beg else f32(0)) if mean else f32(1)
        out[r] = (ab[0] + ab[1]) * sc
    return out


def emu_segment_mean(msg, rowptr, eperm, drop_last_of_odd=False, wrong_length_row=None):
    out = np.zeros((len(rowptr) - 1, msg.shape[1]), f32)
    for n in range(len(rowptr) - 1):
        beg, end = int(rowptr[n]), int(rowptr[n + 1])
        acc = np.zeros(msg.shape[1], f32)
        for p in range(beg, end - 1 if drop_last_of_odd and (end - beg) % 2 else end):
            acc = acc + msg[eperm[p]]
        k = end - beg + (1 if n == wrong_length_row else 0)
        out[n] = acc * (f32(1) / f32(k) if end > beg else f32(0))
    return out


def emu_mask_rows(Y, rowptr, let_through=None):
    out = Y.copy()
    for n in np.flatnonzero(rowptr[1:] == rowptr[:-1]):
        if n != let_through:
            out[n] = 0
    return out


def emu_colsum(dY, rowptr, blocks=1024, skip_tail=False, let_through=None):
    """Fixed slices of ceil(N / blocks) nodes, four chains over the tokens, the tail on the first; then the ordered
    sum of the slices."""
    N, L, D = dY.shape
    rpb = -(-N // blocks)
    out = np.zeros(D, f32)
    with np.errstate(invalid='ignore'):                   # the mutant that lets a NaN row through
        for n0 in range(0, N, rpb):
            a = [np.zeros(D, f32) for _ in range(4)]
            for n in range(n0, min(n0 + rpb, N)):
                if rowptr[n + 1] == rowptr[n] and n != let_through:
                    continue
                for l in range(L - L % 4):
                    a[l % 4] = a[l % 4] + dY[n, l].astype(f32)
                for l in range(L - L % 4, L if not skip_tail else L - L % 4):
                    a[0] = a[0] + dY[n, l].astype(f32)
            out = out + ((a[0] + a[1]) + (a[2] + a[3]))
    return out


def third_empty(N, seed=0):
    """A CSR row pointer over N nodes in which about a third of the segments are empty."""
    deg = np.random.default_rng(41 + seed).integers(1, 4, N)
    deg[np.arange(N) % 3 == 1] = 0
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)


def test_the_bars_reject_wrong_kernels():
    """Each kernel's arithmetic in numpy float32 on the inputs of the GPU tests: the bars pass it as it is and fail it
    broken once -- the last edge of odd segments dropped, `w` ignored, one row's mean over the wrong length, M for M^T,
    nld's head stride on an nhld tile, the L % 4 tail of the column sum skipped, a masked row let through."""
    lad = graph('L')
    rowptr, col = lad.rowptr, lad.col
    deg = np.diff(rowptr)
    loose = ~lr.pow2(deg)[:, None]
    eperm = np.argsort(lad.dst, kind='stable')
    odd_row = int(np.flatnonzero((deg % 2 == 1) & (deg > 1))[0])
    report = []

    def verdicts(name, kind, clean, mutants, bar):
        ok = bar(clean)
        report.append(f'{name} [{kind}]: clean {"passes" if ok else "FAILS"}')
        assert ok, report[-1]
        for label, got in mutants.items():
            assert not bar(got), f'{name} [{kind}]: the bar lets the mutant "{label}" pass'

    # ---- gather_segment_sum: the ladder's CSR, mean; weights: powers of two (exact) / the real 1 / degree (random)
    F = 108
    for kind in ('exact', 'random'):
        rows = lr.rows(kind, lad.N, F)
        w = lr.pow2_weights(lad.E) if kind == 'exact' else (1.0 / np.maximum(lad.indeg, 1)[col]).astype(f32)
        for mean in (1, 0):
            ref, S = lr.gather_segment_sum(rows, rowptr, col, w, mean)
            bar = ((lambda got: lr.exact_problems(got, ref, loose if mean else None) == 0) if kind == 'exact' else
                   (lambda got: lr.random_share(got, ref, S, deg[:, None]) <= 1))
            mutants = {'last edge of odd segments dropped': emu_gather(rows, rowptr, col, w, mean, drop_last_of_odd=True),
                       'w ignored': emu_gather(rows, rowptr, col, w, mean, ignore_w=True)}
            if mean:
                mutants['wrong segment length in one row'] = emu_gather(rows, rowptr, col, w, mean,
                                                                        wrong_length_row=odd_row)
            verdicts(f'gather_segment_sum mean={mean}', kind, emu_gather(rows, rowptr, col, w, mean), mutants, bar)

    # ---- segment_mean
    for kind in ('exact', 'random'):
        msg = lr.rows(kind, lad.E, 3)
        ref, S = lr.segment_mean(msg, rowptr, eperm, 3)
        bar = ((lambda got: lr.exact_problems(got, ref, loose) == 0) if kind == 'exact' else
               (lambda got: lr.random_share(got, ref, S, deg[:, None]) <= 1))
        verdicts('segment_mean', kind, emu_segment_mean(msg, rowptr, eperm),
                 {'last edge of odd segments dropped': emu_segment_mean(msg, rowptr, eperm, drop_last_of_odd=True),
                  'wrong segment length in one row': emu_segment_mean(msg, rowptr, eperm, wrong_length_row=odd_row)}, bar)

    # ---- linear_outer, linear_apply at (5, 6, 3) and the odd head width (3, 7, 2); A of `outer` lies as nhld
    N = 8
    for shape in ((5, 6, 3), (3, 7, 2)):
        L, dh, H = shape
        for kind in ('exact', 'random'):
            A, B, M = lr.tiles(kind, shape, N), lr.tiles(kind, shape, N, seed=1), lr.matrices(kind, shape, N)
            ns, rsd, hs, _ = layout_strides('nhld', N, L, H, dh)
            flat = np.ascontiguousarray(A.transpose(0, 2, 1, 3)).reshape(-1)            # [N, H, L, dh]: the nhld placement
            assert np.array_equal(read_view(flat, (ns, rsd, hs), N, L, H, dh), A)
            wrong_head = read_view(flat, (ns, rsd, layout_strides('nld', N, L, H, dh)[2]), N, L, H, dh)
            for scale in (1.0, 0.5):
                ref, S = lr.linear_outer(A, B, scale)
                bar = ((lambda got: lr.exact_problems(got, ref) == 0) if kind == 'exact' else
                       (lambda got: lr.random_share(got, ref, S, L) <= 1))
                verdicts(f'linear_outer {shape} scale={scale}', kind, emu_outer(A, B, scale),
                         {"nld's head stride on an nhld tile": emu_outer(wrong_head, B, scale),
                          'scale ignored': emu_outer(A, B, 1.0) if scale != 1.0 else emu_outer(A, B, 2.0)}, bar)
            # M that differs from its transpose in ONE pair of elements of one (node, head)
            Msym = M + M.transpose(0, 1, 3, 2)
            Msym[N // 2, H - 1, 0, dh - 1] += 1
            for name, mat in (('M', M), ('M nearly symmetric', Msym)):
                for t in (0, 1):
                    ref, S = lr.linear_apply(A, mat, t, 0.5)
                    bar = ((lambda got: lr.exact_problems(got, ref) == 0) if kind == 'exact' else
                           (lambda got: lr.random_share(got, ref, S, dh) <= 1))
                    verdicts(f'linear_apply {shape} {name} transpose={t}', kind, emu_apply(A, mat, t, 0.5),
                             {'M for M^T' if t else 'M^T for M': emu_apply(A, mat, 1 - t, 0.5),
                              "nld's head stride on an nhld tile": emu_apply(wrong_head, mat, t, 0.5)}, bar)

    # ---- mask_rows: NaN and infinity in the rows to be zeroed
    N, Fm = 7, 260
    rp = third_empty(N)
    empty = np.diff(rp) == 0
    Y = lr.poison(lr.rows('random', N, Fm), empty)
    want = lr.mask_rows(Y, rp)

    def mask_bar(got):
        return np.array_equal(got.view(np.int32), want.view(np.int32))
    verdicts('mask_rows', 'NaN rows', emu_mask_rows(Y, rp),
             {'a masked row let through': emu_mask_rows(Y, rp, let_through=int(np.flatnonzero(empty)[0]))}, mask_bar)

    # ---- masked_colsum at N = 1025 (two nodes per slice), L = 5 (one unrolled step and a tail)
    N, L, D = 1025, 5, 100
    rp = third_empty(N)
    empty = np.diff(rp) == 0
    for kind in ('exact', 'random'):
        for bf16 in (False, True):
            dY = lr.rows(kind, N, L * D).reshape(N, L, D)
            dY = lr.to_bf16(dY) if bf16 else dY
            ref, S = lr.masked_colsum(dY, rp)
            clean = emu_colsum(lr.poison(dY, empty), rp)
            bar = ((lambda got: lr.exact_problems(got, ref) == 0) if kind == 'exact' else
                   (lambda got: lr.colsum_share(got, ref, S) <= 1))
            verdicts(f'masked_colsum bf16={bf16}', kind, clean,
                     {'the L % 4 tail skipped': emu_colsum(dY, rp, skip_tail=True),
                      'a masked row let through (NaN)': emu_colsum(lr.poison(dY, empty), rp,
                                                                   let_through=int(np.flatnonzero(empty)[5])),
                      'a masked row let through (finite)': emu_colsum(dY, rp, let_through=int(np.flatnonzero(empty)[5]))},
                     bar)
    print('\n'.join(report))
