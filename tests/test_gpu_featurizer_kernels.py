"""The featuriser's C calls, ONE AT A TIME through ctypes: ampconv_feat_sample_present, ampconv_feat_zscore_stats,
ampconv_feat_build_as, ampconv_feat_table_grad_from (csrc/featurizer.hip), each against its numpy model of
tests/pipeline_reference.py on the inputs that module builds (tests/test_pipeline_reference_cpu.py shows that those inputs
tell the models from their mutants and holds the sampling stream to its chi-square bar: nothing here is statistical).

Every buffer lies inside a larger allocation (edge_layouts.place_flat / place_flat_int): inputs between NaN margins,
outputs in an allocation full of the sentinel -- the table gradient's too, so it arrives full of NaN --; after every
call nothing outside the output may have changed and everything inside must have been written.  Bars
(pipeline_reference's, derived there): indices equal element for element; tokens bit-equal (bf16: the rounded fp32
value); mean and inv_std within 1 ulp of the rounded fp64 value, the constant verdict equal; z within
2^-24 (2 |mean| inv_std + 4 |z|) of the fp64 z; the table gradient bit-equal on exact data, within (n + 4) 2^-24 S on
random data, rows never sampled exact zeros.  All features are finite: the library is built with -fno-honor-nans, under
which a NaN feature has no defined presence."""
import numpy as np
import pytest
import torch

import pipeline_reference as pr
from edge_layouts import place_flat, place_flat_int
from edge_runner import stream

from ampnet_amd import _lib

pytestmark = pytest.mark.gpu

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
CODE = {F32: _lib.AMPCONV_F32, BF16: _lib.AMPCONV_BF16}
BADARG, EDTYPE = -1, -2
SHARE = {}          # bar -> the largest share of it used, printed by every test that raises it


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def raw(p):
    """The values of a placed float buffer as float32 (fp32: bit for bit; bf16: exactly)."""
    return p.backing[p.index.reshape(-1)].reshape(p.index.shape).float().cpu().numpy()


def ints(p):
    return p.backing[p.index.reshape(-1)].reshape(p.index.shape).cpu().numpy()


def written(p, name):
    bad = []
    if not p.outside_intact():
        bad.append(f'{name}: bytes outside the output were written')
    if p.unwritten():
        bad.append(f'{name}: {p.unwritten()} elements of the output were not written')
    return bad


def untouched(*placed):
    return all(p.outside_intact() and p.unwritten() == p.index.numel() for p in placed)


def note(bar, share, name):
    if share > SHARE.get(bar, -1.0):
        SHARE[bar] = share
        print(f'[bar] {bar}: {100 * share:.1f} % at {name}')


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# -------------------------------------------------------------------------------------------------------- sample_present
def run_sample(lib, x, L, seed, name, skew=0):
    N, F = x.shape
    px, pi, pf = place_flat(x, F32, skew=skew), place_flat_int((N, L), I32), place_flat_int((1,), I32)
    rc = lib.ampconv_feat_sample_present(px.ptr, N, F, L, seed, pi.ptr, pf.ptr, stream())
    torch.cuda.synchronize()
    if rc != 0:
        return [f'{name}: returned {rc}']
    want, empty = pr.sample_present(x, L, seed)
    bad = written(pi, name + ' idx') + written(pf, name + ' flag')
    got = ints(pi)
    if not np.array_equal(got, want):
        rows = np.nonzero((got != want).any(axis=1))[0]
        bad.append(f'{name}: {len(rows)} rows differ from the stream, the first ones {rows[:8].tolist()}')
    if int(ints(pf)[0]) != empty:
        bad.append(f'{name}: empty flag {int(ints(pf)[0])}, expected {empty}')
    return bad


@pytest.mark.parametrize('F,L,seed', pr.sample_cases())
def test_sample_present_is_the_stream(F, L, seed, lib):
    """The 12 constructed rows and 60 random ones of pipeline_reference.sample_rows: the all-zero row gives -1 and the
    flag, its neighbours their stream; the rows behind it alone (rows misaligned by a skew of one float) leave the flag
    down and take the counters of THEIR row numbers."""
    x = pr.sample_rows(F)
    failed = run_sample(lib, x, L, seed, f'F={F} L={L} seed={seed}')
    failed += run_sample(lib, x[pr.EMPTY_ROW + 1:30], L, seed, f'F={F} L={L} seed={seed} rows 8..29', skew=1)
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------------- zscore_stats
@pytest.mark.parametrize('N', pr.ZSCORE_N)
def test_zscore_stats_and_the_assembled_z(N, lib):
    """mean, inv_std and the verdict per column family, then z as ampconv_feat_build_as assembles it from them (De = 0,
    every column a token): within the z bar of the fp64 z, and bit-equal to the float32 expression on the same fp32
    statistics."""
    failed = []
    for n, F, shift in (c for c in pr.zscore_cases() if c[0] == N):
        name = f'N={N} F={F} shift={shift}'
        x = pr.zscore_columns(N, F, shift)
        mean, inv_std, constant = pr.zscore_stats(x)
        assert not (np.abs(inv_std[~constant] - 1) < 1e-3).any()          # inv_std == 1 IS the verdict
        px, pm, ps = place_flat(x, F32), place_flat((F,), F32), place_flat((F,), F32)
        rc = lib.ampconv_feat_zscore_stats(px.ptr, N, F, pm.ptr, ps.ptr, stream())
        torch.cuda.synchronize()
        if rc != 0:
            failed.append(f'{name}: returned {rc}')
            continue
        failed += written(pm, name + ' mean') + written(ps, name + ' inv_std')
        gm, gs = raw(pm), raw(ps)
        if not np.array_equal(gs == 1, constant):
            failed.append(f'{name}: constant verdict differs in columns {np.nonzero((gs == 1) != constant)[0].tolist()}')
        um, us = pr.ulp_distance(gm, mean.astype(np.float32)).max(), pr.ulp_distance(gs, inv_std.astype(np.float32)).max()
        note('mean, ulp of 1', um, name), note('inv_std, ulp of 1', us, name)
        if um > 1 or us > 1:
            failed.append(f'{name}: mean {um} ulp, inv_std {us} ulp from the rounded fp64 value')
        idx = np.tile(np.arange(F, dtype=np.int32), (N, 1))
        pidx, ptab, pz = place_flat_int(idx, I32), place_flat(np.zeros(1, np.float32), F32), place_flat((N, F, 1), F32)
        rc = lib.ampconv_feat_build_as(px.ptr, pm.ptr, ps.ptr, pidx.ptr, ptab.ptr, N, F, F, 0, pz.ptr, CODE[F32], stream())
        torch.cuda.synchronize()
        if rc != 0:
            failed.append(f'{name}: feat_build_as returned {rc}')
            continue
        failed += written(pz, name + ' z')
        z = raw(pz)[..., 0]
        if not np.array_equal(bits(z), bits(pr.build_tokens_f32(x, gm, gs, idx, np.zeros((F, 0), np.float32))[..., 0])):
            failed.append(f'{name}: z is not (x - mean) * inv_std in float32')
        z64 = (x.astype(np.float64) - mean) * inv_std
        bar = pr.z_bar(mean, inv_std, z64)
        err = np.abs(z.astype(np.float64) - z64)
        share = float(np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0)).max())
        note('z bar', share, name)
        if not share <= 1:
            failed.append(f'{name}: z at {share:.3g} times its bar')
    assert not failed, failed


# --------------------------------------------------------------------------------------------------------- feat_build_as
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('De', pr.DE)
def test_feat_build_is_bit_equal(De, dtype, lib):
    x, mean, inv_std, idx, table = pr.token_inputs(De)
    N, F, L = pr.TOKEN_N, pr.TOKEN_F, pr.TOKEN_L
    px, pm, ps, pt = (place_flat(a, F32) for a in (x, mean, inv_std, table if De else np.zeros(1, np.float32)))
    pidx = place_flat_int(idx, I32)
    want = pr.build_tokens_f32(x, mean, inv_std, idx, table)
    calls = [('feat_build_as', dtype, lambda o: lib.ampconv_feat_build_as(px.ptr, pm.ptr, ps.ptr, pidx.ptr, pt.ptr, N, F, L, De,
                                                                          o.ptr, CODE[dtype], stream()))]
    if dtype == F32:
        calls.append(('feat_build', F32, lambda o: lib.ampconv_feat_build(px.ptr, pm.ptr, ps.ptr, pidx.ptr, pt.ptr, N, F, L, De,
                                                                          o.ptr, stream())))
    failed = []
    for name, dt, call in calls:
        po = place_flat((N, L, De + 1), dt)
        rc = call(po)
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        failed += written(po, name)
        miss = int((bits(raw(po)) != bits(pr.to_bf16(want) if dt == BF16 else want)).sum())
        if miss:
            failed.append(f'{name} De={De}: {miss}/{want.size} elements are not bit-equal')
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------- table_grad_from
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('De', pr.DE)
def test_table_grad_from(De, dtype, lib):
    """Hot row (4096 terms on one feature), random and with -1 tokens; exact and random data; dtable arrives full of NaN.
    De = 0 has no table: refused, nothing written."""
    N, L, F = pr.GRAD_N, pr.GRAD_L, pr.GRAD_F
    failed = []
    for pattern in pr.PATTERNS:
        for kind in ('exact', 'random'):
            name = f'De={De} {pattern} {kind}'
            dout, idx = pr.grad_inputs(De, pattern, kind)
            if dtype == BF16:
                dout = pr.to_bf16(dout)                            # the model reads what the kernel reads
            pd, pidx, pg = place_flat(dout, dtype), place_flat_int(idx, I32), place_flat((F, max(De, 1)), F32)
            rc = lib.ampconv_feat_table_grad_from(pd.ptr, pidx.ptr, N, L, De, F, pg.ptr, CODE[dtype], stream())
            torch.cuda.synchronize()
            if De == 0:
                if rc != BADARG or not untouched(pg):
                    failed.append(f'{name}: returned {rc}, or wrote')
                continue
            if rc != 0:
                failed.append(f'{name}: returned {rc}')
                continue
            failed += written(pg, name)
            got = raw(pg)
            ref, S, n = pr.table_grad(dout, idx, F)
            if bits(got[n[:, 0] == 0]).any():
                failed.append(f'{name}: rows no token names are not exact zeros')
            if kind == 'exact':
                miss = int((bits(got) != bits((ref + 0.0).astype(np.float32))).sum())
                if miss:
                    failed.append(f'{name}: {miss}/{got.size} elements are not bit-equal')
            else:
                share = pr.random_share(got, ref, S, n)
                note('table_grad (n + 4) 2^-24 S', share, name)
                if not share <= 1:
                    failed.append(f'{name}: {share:.3g} times the bound (n + 4) 2^-24 S')
    if dtype == F32 and De:                                         # the fp32 wrapper is the same call
        dout, idx = pr.grad_inputs(De, 'with -1', 'exact')
        pd, pidx, pg = place_flat(dout, F32), place_flat_int(idx, I32), place_flat((F, De), F32)
        rc = lib.ampconv_feat_table_grad(pd.ptr, pidx.ptr, N, L, De, F, pg.ptr, stream())
        torch.cuda.synchronize()
        ref = pr.table_grad(dout, idx, F)[0]
        if rc != 0 or written(pg, 'x') or (bits(raw(pg)) != bits((ref + 0.0).astype(np.float32))).any():
            failed.append(f'feat_table_grad De={De}: returned {rc} or differs')
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------- refusals
def test_featuriser_refusals(lib):
    """Read from the entry points: a NULL pointer, a size of 0 or below, more than INT32_MAX tokens, another dtype -- a
    status code before anything is launched, the outputs as they were."""
    N, F, L, De = 5, 9, 4, 3
    rng = np.random.default_rng(0)
    x, mean, inv_std, table = (place_flat(rng.random(s).astype(np.float32) + 0.5, F32) for s in ((N, F), (F,), (F,), (F, De)))
    idx = place_flat_int(rng.integers(0, F, (N, L)), I32)
    dout = place_flat(rng.random((N, L, De + 1)).astype(np.float32), F32)
    om, os_, oi, of, ot, og = (place_flat((F,), F32), place_flat((F,), F32), place_flat_int((N, L), I32), place_flat_int((1,), I32),
                               place_flat((N, L, De + 1), F32), place_flat((F, De), F32))
    s = stream()
    failed = []

    def refuse(label, rc, want=BADARG):
        torch.cuda.synchronize()
        if rc != want or not untouched(om, os_, oi, of, ot, og):
            failed.append(f'{label}: returned {rc} (expected {want}) or wrote')

    for k in range(3):
        a = [x.ptr, om.ptr, os_.ptr]
        a[k] = None
        refuse(f'zscore_stats NULL #{k}', lib.ampconv_feat_zscore_stats(a[0], N, F, a[1], a[2], s))
    for n, f in ((0, F), (-1, F), (N, 0), (N, -3)):
        refuse(f'zscore_stats N={n} F={f}', lib.ampconv_feat_zscore_stats(x.ptr, n, f, om.ptr, os_.ptr, s))
    for k in range(3):
        a = [x.ptr, oi.ptr, of.ptr]
        a[k] = None
        refuse(f'sample_present NULL #{k}', lib.ampconv_feat_sample_present(a[0], N, F, L, 1, a[1], a[2], s))
    for n, f, l in ((0, F, L), (-2, F, L), (N, 0, L), (N, -1, L), (N, F, 0), (N, F, -1), (2 ** 31, F, L)):
        refuse(f'sample_present N={n} F={f} L={l}', lib.ampconv_feat_sample_present(x.ptr, n, f, l, 1, oi.ptr, of.ptr, s))
    for k in range(6):
        a = [x.ptr, mean.ptr, inv_std.ptr, idx.ptr, table.ptr, ot.ptr]
        a[k] = None
        refuse(f'feat_build_as NULL #{k}', lib.ampconv_feat_build_as(*a[:5], N, F, L, De, a[5], CODE[F32], s))
    for n, f, l, d in ((0, F, L, De), (-1, F, L, De), (N, 0, L, De), (N, F, 0, De), (N, F, L, -1), (2 ** 29, F, L, De)):
        refuse(f'feat_build_as N={n} F={f} L={l} De={d}',
               lib.ampconv_feat_build_as(x.ptr, mean.ptr, inv_std.ptr, idx.ptr, table.ptr, n, f, l, d, ot.ptr, CODE[F32], s))
    for code in (2, -1, 7):
        refuse(f'feat_build_as dtype {code}', lib.ampconv_feat_build_as(x.ptr, mean.ptr, inv_std.ptr, idx.ptr, table.ptr, N, F, L, De,
                                                                       ot.ptr, code, s), EDTYPE)
        refuse(f'table_grad_from dtype {code}', lib.ampconv_feat_table_grad_from(dout.ptr, idx.ptr, N, L, De, F, og.ptr, code, s),
               EDTYPE)
    for k in range(3):
        a = [dout.ptr, idx.ptr, og.ptr]
        a[k] = None
        refuse(f'table_grad_from NULL #{k}', lib.ampconv_feat_table_grad_from(a[0], a[1], N, L, De, F, a[2], CODE[F32], s))
    for n, l, d, f in ((0, L, De, F), (N, 0, De, F), (N, L, 0, F), (N, L, -1, F), (N, L, De, 0), (2 ** 29, L, De, F)):
        refuse(f'table_grad_from N={n} L={l} De={d} F={f}',
               lib.ampconv_feat_table_grad_from(dout.ptr, idx.ptr, n, l, d, f, og.ptr, CODE[F32], s))
    assert not failed, failed


def test_given_feature_indices_are_range_checked():
    """FeatureTokens.forward(x, idx=...) -- the path of AMPGCN.forward(feature_indices=...) -- hands the indices to
    table[f] and x[n, f] on the device: a wrong shape, a wrong row count, a float tensor or a value outside [0, F) must be
    a Python error before anything is launched, not a device read out of bounds."""
    import types
    from ampnet_amd import AMPGCN
    from ampnet_amd.module import FeatureTokens
    dev = torch.device('cuda:0')
    N, F, L, De = 20, 30, 20, 31                       # the layer shape of test_ampgcn_model_matches_reference_structure
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, F, generator=g).to(dev)
    ft = FeatureTokens(F, De, L).to(dev)
    good = torch.randint(0, F, (N, L), generator=g)
    good[0, 0], good[N - 1, L - 1] = 0, F - 1
    tokens, idx = ft(x, good.to(dev))
    assert torch.equal(idx.cpu(), good.int())
    mean, inv_std = ft.zscore_stats(x)
    want = pr.build_tokens_f32(x.cpu().numpy(), mean.cpu().numpy(), inv_std.cpu().numpy(), good.numpy(),
                               ft.feature_embedding_table.weight.detach().cpu().numpy())
    assert np.array_equal(bits(tokens.detach().cpu().numpy()), bits(want.reshape(N, -1)))
    top, low, minus = good.clone(), good.clone(), good.clone()
    top[3, 2], low[N - 1, 0], minus[0, 1] = F, -F, -1
    model = AMPGCN(device=dev, embedding_dim=De + 1, num_heads=1, num_node_features=F, num_sampled_vectors=L, feat_emb_dim=De,
                   dropout_rate=0.0, dropout_adj_rate=0.0).to(dev)
    data = types.SimpleNamespace(x=x, edge_index=torch.randint(0, N, (2, 50), generator=g).to(dev))
    assert model(data, feature_indices=good.to(dev)).shape == (N, 7)
    for bad in (top, low, minus, good.flatten(), good[:N - 1], good[:, :, None], good.float(), good[:0]):
        with pytest.raises(ValueError, match='feature indices'):
            ft(x, bad.to(dev))
        with pytest.raises(ValueError, match='feature indices'):
            model(data, feature_indices=bad)
