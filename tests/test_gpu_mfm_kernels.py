"""csrc/mfm.hip one library call at a time (ampnet_amd._lib, no Python wrapper in between) against the numpy fp64 model of
tests/mfm_reference.py.

Ladder: N in {0, 1, 63, 64, 65, 257}, L in {1, 2, 40}, D = De + 1 in {1, 3, 4, 100, 128, 257} -- every value of each in some
case, the combinations chosen so that every path is entered: the element-wise kernels (D = 1, 3, 257, and an unaligned
base), 16-byte pieces (fp32 D = 4, 100, 128; bf16 D = 128), bf16's 8-byte pieces (D = 4, 100), groups of 4 to 64 lanes, more
pieces than lanes (D = 257: five passes of the sums), one tile and many, a ragged last tile.  `_geom` mirrors make_geom and
dispatch of mfm.hip; the ids name the path.  Every case runs both modes and five masks: none (threshold 0), all (65536),
a single token (replayed), drawn at 0.15 and at 0.75; one shape has rows of idx == -1 and replays a mask that names them.
Rows of unmasked tokens hold NaN in h and dout; every tensor lies between guard bands (tests/site_guards.py); the workspace
is exactly ampconv_mfm_workspace_bytes long; every call is launched twice and must give the same bits.
Tolerances: resid, loss and fp32 dh at the project's flat atol 1e-5, rtol 1e-4 (inputs O(1), w uniform in +-1/sqrt(D) as
head_reference.make_inputs); bf16 dh atol = rtol = 2e-2; dw, db and dmask_token under the labels gW, gb (the scaled bar of
test_gpu_head.py) AND within depth * 2^-24 * S of the fp64 model, S the sum of the absolute values of the terms and depth
the longest chain of additions a term passes (its lane's tiles, the slots of a workgroup, the workgroups) plus 4 for the
roundings of a term itself: the worst-case bound of fp32 summation in that order.  Masks, counts and bit patterns exact."""
import functools
import types

import numpy as np
import pytest
import torch

import mfm_reference as ref
from site_guards import BF16_TOL, MISALIGN, TORCH_DTYPE, Guarded, bits, close, header_constant

pytestmark = pytest.mark.gpu

SHIFT = header_constant('AMPCONV_MFM_LOSS_SHIFT')
THREADS, K_MAX_BLOCKS = 256, 1024               # csrc/mfm.hip kThreads, kMaxBlocks
CODE = {'f32': 0, 'bf16': 1}
F = 13                                          # feature columns of the featuriser inputs
SEED = 2 ** 63 + 5
MASKS = ('none', 'all', 'single', 'p15', 'p75')
THRESHOLD = {'none': 0, 'all': 65536, 'p15': 9830, 'p75': 49152}

# (N, L, D, rows of idx == -1, misaligned base)
SHAPES = [(0, 2, 4, False, False), (1, 1, 1, False, False), (1, 40, 100, False, False), (63, 2, 3, False, False),
          (63, 40, 3, False, False), (64, 1, 4, False, False), (64, 40, 128, False, False), (65, 2, 100, True, False),
          (65, 40, 257, False, False), (257, 1, 128, False, False), (257, 2, 1, False, False), (257, 40, 100, False, False),
          (257, 2, 257, False, False), (65, 2, 128, False, True)]


def _geom(T, D, dtype, aligned=True, width=None, scalar=False):
    """dispatch + make_geom + grid_of of mfm.hip for the loss kernels and token_grad."""
    if dtype == 'f32':
        NP = 4 if aligned and D % 4 == 0 else 1
    else:
        NP = 8 if aligned and D % 8 == 0 else 4 if aligned and D % 4 == 0 else 1
    if scalar:
        NP = 1
    P, G = (D if width is None else width) // NP, 4
    while G < P and G < 64:
        G <<= 1
    R = THREADS // G
    tiles = -(-T // R)
    blocks = min(tiles, K_MAX_BLOCKS)
    depth = (-(-tiles // blocks) if blocks else 0) + R + blocks + 4
    return types.SimpleNamespace(NP=NP, P=P, G=G, R=R, tiles=tiles, blocks=blocks, passes=-(-P // G), depth=depth)


def _case_id(shape, dtype):
    N, L, D, empty, off = shape
    q = _geom(max(N * L, 1), D, dtype, not off)
    return (f'{dtype}_N{N}_L{L}_D{D}_{"elem" if q.NP == 1 else f"piece{q.NP}"}_G{q.G}_pass{q.passes}'
            + ('_empty_rows' if empty else '') + ('_unaligned' if off else ''))


CASES = [(s, d) for s in SHAPES for d in ('f32', 'bf16')]


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


@functools.lru_cache(maxsize=2)
def _inputs(N, L, D, empty):
    """CPU tensors shared by the dtypes of a shape, never modified."""
    g = torch.Generator().manual_seed(1000 * N + 10 * L + D)
    De = D - 1
    x = torch.randn(max(N, 1), F, generator=g)[:N]
    mean = torch.randn(F, generator=g) * 0.1
    inv_std = torch.rand(F, generator=g) + 0.5
    idx = torch.randint(0, F, (N, L), generator=g, dtype=torch.int32)
    if empty:
        idx[3], idx[40] = -1, -1
    table = torch.randn(F, De, generator=g)
    token = torch.randn(D, generator=g)
    h = torch.randn(N, L, D, generator=g)
    dout = torch.randn(N, L, D, generator=g)
    w = (torch.rand(D, generator=g) * 2 - 1) / D ** 0.5
    b = (torch.rand(1, generator=g) * 2 - 1) / D ** 0.5
    return types.SimpleNamespace(x=x, mean=mean, inv_std=inv_std, idx=idx, table=table, token=token, h=h, dout=dout, w=w, b=b)


def _mask_of(kind, idx, empty):
    """(model mask bool [N, L], masked_in bytes or None, threshold)."""
    idx = idx.numpy()
    N, L = idx.shape
    if kind == 'single':
        given = np.zeros((N, L), dtype=np.uint8)
        if N:
            given[N // 2, L // 2] = 3                                     # any non-zero byte
            if empty:
                given[3], given[40, 0] = 1, 1                             # names tokens of idx == -1: ANDed away
        return (given != 0) & (idx >= 0), torch.from_numpy(given), 0
    thr = THRESHOLD[kind]
    return ref.token_mask(idx, SEED, thr), None, thr


def _within_bound(got, want, S, depth, name):
    got, want, S = (np.asarray(a, np.float64).reshape(-1) for a in (got, want, S))
    bound = depth * ref.U32 * S + 1e-30
    err = np.abs(got - want)
    print(f'[bound] {name}: max err / bound {float((err / bound).max()) if err.size else 0.0:.3e} (depth {depth})')
    assert (err <= bound).all(), f'{name}: max err {err.max():.3e} exceeds depth * 2^-24 * S = {bound[err.argmax()]:.3e}'


@pytest.mark.parametrize('case', CASES, ids=[_case_id(*c) for c in CASES])
def test_every_call_against_the_model(case, dev, lib):
    (N, L, D, empty, unaligned), dtype = case
    De, T, td, code = D - 1, N * L, TORCH_DTYPE[dtype], CODE[dtype]
    off = MISALIGN[dtype] if unaligned else 0
    i = _inputs(N, L, D, empty)
    q = _geom(max(T, 1), D, dtype, not unaligned)
    ws_bytes = int(lib.ampconv_mfm_workspace_bytes(N, L, D))
    assert ws_bytes == (min(-(-T // 4), K_MAX_BLOCKS) * (D + 1) * 4 if N else 0)
    assert q.blocks * (D + 1) * 4 <= ws_bytes or N == 0

    X, MEAN, ISTD, IDX = (Guarded.of(dev, t) for t in (i.x, i.mean, i.inv_std, i.idx))
    TABLE, TOKEN, W, B = (Guarded.of(dev, t) for t in (i.table, i.token, i.w, i.b))
    feat = (X.ptr, MEAN.ptr, ISTD.ptr, IDX.ptr, TABLE.ptr, N, F, L, De)
    # the featuriser's own build on the same inputs: in the storage dtype, and in fp32 for z
    PLAIN, PLAIN32 = Guarded(dev, td, T * D), Guarded(dev, torch.float32, T * D)
    if N:
        _call(lib, 'ampconv_feat_build_as', *feat, PLAIN.ptr, code, None)
        _call(lib, 'ampconv_feat_build_as', *feat, PLAIN32.ptr, 0, None)
    plain = PLAIN.t.view(N, L, D)
    z32 = PLAIN32.t.view(N, L, D)[..., De]
    token_bits = bits(TOKEN.t.to(td))
    hq, doutq = i.h.to(td), i.dout.to(td)                                  # the stored values
    WS = Guarded(dev, torch.uint8, ws_bytes)
    G3 = Guarded.of(dev, torch.tensor([3.0]))

    for kind in MASKS:
        want_mask, given, thr = _mask_of(kind, i.idx, empty)
        GIVEN = Guarded.of(dev, given) if given is not None else None
        mask_t = torch.from_numpy(want_mask)
        count = int(want_mask.sum())
        for mode in (ref.TOKEN, ref.VALUE):
            what = f'{kind} mode {mode}'
            # ---- build --------------------------------------------------------------------------------------------------
            OUT, MASKED, TARGET = Guarded(dev, td, T * D, off), Guarded(dev, torch.uint8, T), Guarded(dev, torch.float32, T)
            runs = []
            for _ in range(2):
                for o in (OUT, MASKED, TARGET):
                    o.refill()
                _call(lib, 'ampconv_mfm_build', *feat, TOKEN.ptr, SEED, thr, mode, GIVEN.ptr if GIVEN else None, OUT.ptr,
                      MASKED.ptr, TARGET.ptr, code, None)
                runs.append((bits(OUT.t).clone(), MASKED.t.clone(), bits(TARGET.t).clone()))
            for a, c in zip(*runs):
                assert torch.equal(a, c), f'build {what}: two launches differ'
            for o, name in ((OUT, 'out'), (MASKED, 'masked'), (TARGET, 'target')):
                assert o.intact(), f'build {what}: wrote outside {name}'
                assert o.written() or T == 0, f'build {what}: {name} has unwritten elements'
            got_mask = MASKED.t.view(N, L).cpu()
            assert np.array_equal(got_mask.numpy(), want_mask.astype(np.uint8)), f'build {what}: mask'
            out = OUT.t.view(N, L, D)
            m = mask_t.to(dev)
            assert torch.equal(bits(out[~m]), bits(plain[~m])), f'build {what}: unmasked tokens are not feat_build_as'
            if mode == ref.TOKEN:
                assert bool((bits(out[m]) == token_bits).all()), f'build {what}: masked tokens are not the mask token'
            else:
                assert torch.equal(bits(out[m][:, :De]), bits(plain[m][:, :De])), f'build {what}: embedding slots'
                assert bool((bits(out[m][:, De]) == token_bits[De]).all()), f'build {what}: value slot'
            assert torch.equal(bits(TARGET.t.view(N, L)), bits(z32.contiguous())), f'build {what}: target is not z'
            if thr == 0 and GIVEN is None:
                assert torch.equal(bits(out), bits(plain))
            if N:                                                          # the model, on top of the bit checks
                mo, mm, mt = ref.build(i.x.numpy(), i.mean.numpy(), i.inv_std.numpy(), i.idx.numpy(), i.table.numpy(),
                                       i.token.numpy(), want_mask, mode)
                close(OUT.np(N, L, D), torch.from_numpy(mo).to(td).float().numpy(), f'out {what}', atol=1e-6, rtol=1e-6)

            # ---- token_grad ---------------------------------------------------------------------------------------------
            dq = doutq.clone()
            dq[~mask_t] = float('nan')
            DOUT, DTOK = Guarded.of(dev, dq, off), Guarded(dev, torch.float32, D)
            runs = []
            for _ in range(2):
                DTOK.refill(), WS.refill()
                _call(lib, 'ampconv_mfm_token_grad', DOUT.ptr, MASKED.ptr, N, L, De, mode, DTOK.ptr, WS.ptr, ws_bytes, code, None)
                runs.append(bits(DTOK.t).clone())
            assert torch.equal(*runs), f'token_grad {what}: two launches differ'
            assert DTOK.intact() and DTOK.written() and WS.intact()
            want, S = ref.token_grad(doutq.float().numpy(), want_mask, mode)
            tq = _geom(max(T, 1), D, dtype, not unaligned, 1 if mode == ref.VALUE else None, mode == ref.VALUE)
            close(DTOK.np(), want, f'gW dmask_token {what}')
            _within_bound(DTOK.np(), want, S, tq.depth, f'dmask_token {what}')
            if mode == ref.VALUE:
                assert bool((bits(DTOK.t[:De]) == 0).all())
            if count == 0:
                assert bool((bits(DTOK.t) == 0).all())

        # ---- loss forward (the mask of the last build; the mode does not enter) ----------------------------------------
        hq_nan = hq.clone()
        hq_nan[~mask_t] = float('nan')
        H, TGT = Guarded.of(dev, hq_nan, off), Guarded.of(dev, TARGET.t.cpu())
        RESID, STATE, LOSS = Guarded(dev, torch.float32, T), Guarded(dev, torch.int64, 2), Guarded(dev, torch.float32, 1)
        SUMS = Guarded.of(dev, torch.tensor([1000, 7], dtype=torch.int64))
        runs = []
        for k in range(2):
            for o in (RESID, STATE, LOSS):
                o.refill()
            _call(lib, 'ampconv_mfm_loss_fwd', H.ptr, MASKED.ptr, TGT.ptr, W.ptr, B.ptr, N, L, D, RESID.ptr,
                  SUMS.ptr if k == 0 else None, STATE.ptr, LOSS.ptr, code, None)
            runs.append((bits(RESID.t).clone(), STATE.t.clone(), bits(LOSS.t).clone()))
        for a, c in zip(*runs):
            assert torch.equal(a, c), f'loss_fwd {kind}: two launches differ'
        for o in (RESID, STATE, LOSS, SUMS):
            assert o.intact() and (o.written() or o.nbytes == 0)
        fwd = ref.loss_fwd(hq.float().numpy(), want_mask, TARGET.np(N, L), i.w.numpy(), i.b.numpy())
        resid = RESID.np(N, L)
        close(resid, fwd['resid'], f'resid {kind}')
        assert bool((bits(RESID.t.view(N, L)[~mask_t.to(dev)]) == 0).all()), f'loss_fwd {kind}: unmasked residuals'
        state = STATE.t.cpu().tolist()
        assert state[1] == fwd['count'] == count
        assert abs(state[0] - ref.fixed_sum(resid)) <= count, (state[0], ref.fixed_sum(resid))
        assert SUMS.t.cpu().tolist() == [1000 + state[0], 7 + state[1]]
        close(LOSS.np()[0], fwd['loss'], f'loss {kind}')
        assert LOSS.np()[0] == np.float32(np.float64(state[0]) / 2.0 ** SHIFT / max(state[1], 1))

        # ---- loss backward: the model's residuals rounded to fp32, the count and a junk sum in `state`, *g = 3 -----------
        r32 = torch.from_numpy(fwd['resid'].astype(np.float32))
        RIN, SIN = Guarded.of(dev, r32), Guarded.of(dev, torch.tensor([-12345, count], dtype=torch.int64))
        DH, DW, DB = Guarded(dev, td, T * D, off), Guarded(dev, torch.float32, D), Guarded(dev, torch.float32, 1)
        runs = []
        for k in range(3):                                                 # the third without dh
            for o in (DH, DW, DB, WS):
                o.refill()
            _call(lib, 'ampconv_mfm_loss_bwd', H.ptr, MASKED.ptr, RIN.ptr, W.ptr, SIN.ptr, G3.ptr, N, L, D,
                  DH.ptr if k < 2 else None, DW.ptr, DB.ptr, WS.ptr, ws_bytes, code, None)
            runs.append((bits(DH.t).clone(), bits(DW.t).clone(), bits(DB.t).clone()))
            assert DH.intact() and DW.intact() and DB.intact() and WS.intact()
            assert DW.written() and DB.written() and (DH.written() or k == 2 or T == 0)
        for a, c in zip(runs[0], runs[1]):
            assert torch.equal(a, c), f'loss_bwd {kind}: two launches differ'
        assert torch.equal(runs[0][1], runs[2][1]) and torch.equal(runs[0][2], runs[2][2]), 'dw, db depend on dh'
        assert bool((runs[2][0] == -1).all()), 'dh = NULL: something was written'
        for o in (DH, DW, DB):
            o.refill()
        _call(lib, 'ampconv_mfm_loss_bwd', H.ptr, MASKED.ptr, RIN.ptr, W.ptr, SIN.ptr, G3.ptr, N, L, D, DH.ptr, DW.ptr, DB.ptr,
              WS.ptr, ws_bytes, code, None)
        bwd = ref.loss_bwd(hq.float().numpy(), want_mask, r32.numpy(), i.w.numpy(), count, 3.0)
        close(DH.np(N, L, D), bwd['dh'], f'dh {kind}', **(BF16_TOL if dtype == 'bf16' else {}))
        assert bool((bits(DH.t.view(N, L, D)[~mask_t.to(dev)]) == 0).all()), f'loss_bwd {kind}: unmasked dh rows'
        close(DW.np(), bwd['dw'], f'gW dw {kind}')
        close(DB.np(), [bwd['db']], f'gb db {kind}')
        _within_bound(DW.np(), bwd['dw'], bwd['S_dw'], q.depth, f'dw {kind}')
        _within_bound(DB.np(), [bwd['db']], [bwd['S_db']], q.depth, f'db {kind}')
        if count == 0:
            assert LOSS.np()[0] == 0.0 and state == [0, 0]
            for o in (DH, DW, DB):
                assert bool((bits(o.t) == 0).all())


def test_error_codes(dev, lib):
    N, L, D = 8, 2, 4
    De = D - 1
    i = _inputs(N, L, D, False)
    t = {k: v.to(dev) for k, v in vars(i).items()}
    out, masked, target = torch.full((N, L, D), 7.0, device=dev), torch.full((N, L), 9, dtype=torch.uint8, device=dev), \
        torch.full((N, L), 7.0, device=dev)
    ws = torch.zeros(int(lib.ampconv_mfm_workspace_bytes(N, L, D)), dtype=torch.uint8, device=dev)
    dtok, dw, db = (torch.full((n,), 7.0, device=dev) for n in (D, D, 1))
    state, loss, g = torch.full((2,), 5, dtype=torch.int64, device=dev), torch.full((1,), 7.0, device=dev), torch.ones(1, device=dev)
    p = lambda x: x.data_ptr()                                             # noqa: E731

    def build(N=N, F_=F, L=L, De=De, thr=100, mode=0, dtype=0, x=p(t['x'])):
        return lib.ampconv_mfm_build(x, p(t['mean']), p(t['inv_std']), p(t['idx']), p(t['table']), N, F_, L, De, p(t['token']),
                                     1, thr, mode, None, p(out), p(masked), p(target), dtype, None)

    def token_grad(N=N, L=L, De=De, mode=0, dtype=0, ws_bytes=ws.numel()):
        return lib.ampconv_mfm_token_grad(p(t['dout']), p(masked), N, L, De, mode, p(dtok), p(ws), ws_bytes, dtype, None)

    def fwd(N=N, L=L, D=D, dtype=0, st=p(state)):
        return lib.ampconv_mfm_loss_fwd(p(t['h']), p(masked), p(target), p(t['w']), p(t['b']), N, L, D, p(target), None, st,
                                        p(loss), dtype, None)

    def bwd(N=N, L=L, D=D, dtype=0, ws_bytes=ws.numel()):
        return lib.ampconv_mfm_loss_bwd(p(t['h']), p(masked), p(target), p(t['w']), p(state), p(g), N, L, D, None, p(dw),
                                        p(db), p(ws), ws_bytes, dtype, None)

    assert build(N=-1) == -1 and build(L=0) == -1 and build(De=-1) == -1 and build(F_=0) == -1
    assert build(thr=65537) == -1 and build(mode=2) == -1 and build(mode=-1) == -1 and build(x=None) == -1
    assert build(dtype=7) == -2
    assert token_grad(N=-1) == -1 and token_grad(L=0) == -1 and token_grad(De=-1) == -1 and token_grad(mode=2) == -1
    assert token_grad(dtype=2) == -2 and token_grad(ws_bytes=ws.numel() - 1) == -3
    assert fwd(N=-1) == -1 and fwd(L=0) == -1 and fwd(D=0) == -1 and fwd(st=None) == -1 and fwd(dtype=5) == -2
    assert bwd(N=-1) == -1 and bwd(L=0) == -1 and bwd(D=0) == -1 and bwd(dtype=5) == -2 and bwd(ws_bytes=8) == -3
    assert lib.ampconv_mfm_workspace_bytes(-1, L, D) == 0 and lib.ampconv_mfm_workspace_bytes(0, L, D) == 0
    assert lib.ampconv_mfm_workspace_bytes(N, 0, D) == 0 and lib.ampconv_mfm_workspace_bytes(N, L, 0) == 0
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    assert bool((out == 7).all()) and bool((masked == 9).all()) and bool((target == 7).all()) and bool((loss == 7).all())
    assert bool((dtok == 7).all()) and bool((dw == 7).all()) and bool((db == 7).all()) and bool((state == 5).all())
    # threshold 65536 and N == 0 are fine
    assert build(thr=65536) == 0 and build(N=0, x=None) == 0
    torch.cuda.synchronize()
    assert bool((masked == 1).all())
