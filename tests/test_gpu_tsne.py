"""ampnet_amd.tsne on the GPU: the three C calls of csrc/tsne.hip ONE CALL AT A TIME through ctypes against the fp64
models of tests/tsne_reference.py, the joint probabilities, then tsne() end to end against the loop model and
scikit-learn's recordings (tests/golden/tsne/).

Call by call (as tests/test_gpu_pca.py): inputs and outputs lie inside NaN-filled buffers with NaN margins, dist2 is a
row-strided view with NaN gaps, the workspace is filled with 0xFF; after a call nothing outside an output may have
changed and everything inside must be finite.  Every sweep names all its failing cases in one assertion.

The bounds follow from the kernels' summation structure, with u = 2^-24 (tests/tsne_reference.py holds the constants):

  affinities   2^-22 p per element: the search is fp64 and the CPU tests show that no stop decision of these inputs is
               within 1e-10 of flipping, so what is left is the fp32 rounding of p (u) and fp64 noise.
  repulsion    |neg_f - model| <= (RUN + 16) u sum_j |q^2 (y_i - y_j)|.  A term q^2 d: d = y_i - y_j one rounding (u);
               1 + dx^2 + dy^2 by two FMAs over terms of relative error 2u, all positive (4u); v_rcp_f32 1 ulp (2u): q
               6u, q^2 13u, the FMA's product 14u.  A run of RUN terms added in order in fp32: (RUN - 1) u.  fp64 above
               is noise; neg_f is rounded once (u).  14 + 255 + 1 < RUN + 16.
               |Z - model| <= (RUN + 8) u Z: 6u per term, (RUN - 1) u for the run.
  step         pos = sum (p q) d: p = exaggeration val (u), q 6u, p q 8u, d u, the FMA 10u; a lane adds at most
               PART / 64 = 16 terms (16u), the butterfly has six levels (6u): C_POS = 32.  grad = 4 fp32(pos - neg / Z)
               with the difference in fp64: e_grad = 4 (32 u sum |terms| + 2u |pos - neg / Z|).  gains are fp32
               statements on fp32 inputs: exact where the sign of update * grad is not in doubt, i.e. |grad| > e_grad.
               update = momentum update - lr gains grad: three roundings on top of lr gains e_grad; y_out one more
               (tsne_reference.step_bounds).  error: a term p log(p / (q / Z)) has the argument to 9u, logf to 2 ulp:
               u (25 sum |terms| + 12 sum p).
"""
import importlib

import numpy as np
import pytest
import torch

import tsne_reference as tr
from edge_runner import stream

from ampnet_amd import _lib

ts = importlib.import_module('ampnet_amd.tsne')
pytestmark = pytest.mark.gpu

U = tr.U
MARGIN = 8                       # elements in front of and behind every buffer: a multiple of 8 bytes for every dtype
BADARG, EWORKSPACE = -1, -3
NAMES = [c[0] for c in tr.CASES]


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def dev():
    return torch.device('cuda:0')


class Placed:
    """A [rows, cols] view with row stride ld inside a NaN-filled 1-d buffer with NaN margins (int64: filled with -7)."""

    def __init__(self, rows, cols, dtype, data=None, ld=None):
        ld = cols if ld is None else ld
        fill = float('nan') if dtype.is_floating_point else -7
        self.fill = fill
        self.backing = torch.full((2 * MARGIN + max(rows * ld, 1),), fill, dtype=dtype, device=dev())
        self.view = torch.as_strided(self.backing, (rows, cols), (ld, 1), MARGIN)
        if data is not None:
            self.view.copy_(torch.as_tensor(np.asarray(data).reshape(rows, cols)).to(dev(), dtype))
        self.inside = torch.zeros(self.backing.numel(), dtype=torch.bool, device=dev())
        torch.as_strided(self.inside, (rows, cols), (ld, 1), MARGIN).fill_(True)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def values(self):
        return self.view.cpu().numpy().astype(np.float64)

    def bits(self):
        return self.view.contiguous().view(torch.int32 if self.view.dtype == torch.float32 else torch.int64).cpu().numpy()

    def problems(self, name):
        bad = []
        if not torch.isnan(self.backing[~self.inside]).all():
            bad.append(f'{name}: bytes outside the output were written')
        if not torch.isfinite(self.backing[self.inside]).all():
            bad.append(f'{name}: elements of the output were not written (or are not finite)')
        return bad

    def untouched(self):
        return bool(torch.isnan(self.backing).all())


def nan_workspace(nbytes):
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device=dev())


# ----------------------------------------------------------------------------------------------------- affinities
def test_affinities_sweep(lib):
    bad = []
    for N, K in tr.AFFINITY_SWEEP:
        d, perplexity = tr.affinity_case(N, K)
        name = f'affinities N{N} K{K}'
        pd, pp, pb = Placed(N, K, torch.float32, d, ld=K + 3), Placed(N, K, torch.float32), Placed(N, 1, torch.float64)
        rc = lib.ampconv_tsne_affinities(pd.ptr, N, K, K + 3, perplexity, pp.ptr, pb.ptr, stream())
        torch.cuda.synchronize()
        if rc != 0:
            bad.append(f'{name}: rc {rc}')
            continue
        bad += pp.problems(name + ' p') + pb.problems(name + ' beta')
        P, beta, _ = tr.search_model(d, perplexity)
        got = pp.values()
        if not (np.abs(got - P) <= 2.0 ** -22 * P + 2.0 ** -149).all():
            bad.append(f'{name}: p off by {np.abs(got - P).max():.3e} (rows {np.unique(np.nonzero(np.abs(got - P) > 2.0 ** -22 * P + 2.0 ** -149)[0])[:5]})')
        if not np.array_equal(pb.values()[:, 0], beta):
            bad.append(f'{name}: beta differs from the model in {(pb.values()[:, 0] != beta).sum()} rows')
    assert not bad, '\n'.join(bad)


def test_affinities_bad_arguments(lib):
    d, _ = tr.affinity_case(8, 5)
    pd, pp, pb = Placed(8, 5, torch.float32, d), Placed(8, 5, torch.float32), Placed(8, 1, torch.float64)
    s = stream()
    for name, args in (('K = 0', (pd.ptr, 8, 0, 5, 2.0, pp.ptr, pb.ptr, s)), ('K = 257', (pd.ptr, 8, 257, 257, 2.0, pp.ptr, pb.ptr, s)),
                       ('ldd < K', (pd.ptr, 8, 5, 4, 2.0, pp.ptr, pb.ptr, s)), ('N = 0', (pd.ptr, 0, 5, 5, 2.0, pp.ptr, pb.ptr, s)),
                       ('perplexity 0', (pd.ptr, 8, 5, 5, 0.0, pp.ptr, pb.ptr, s)), ('NULL dist2', (None, 8, 5, 5, 2.0, pp.ptr, pb.ptr, s)),
                       ('NULL p', (pd.ptr, 8, 5, 5, 2.0, None, pb.ptr, s)), ('NULL beta', (pd.ptr, 8, 5, 5, 2.0, pp.ptr, None, s))):
        assert lib.ampconv_tsne_affinities(*args) == BADARG, name
    torch.cuda.synchronize()
    assert pp.untouched() and pb.untouched()


# ------------------------------------------------------------------------------------------- joint probabilities
def test_joint_probabilities_against_the_recording_and_a_star():
    """scikit-learn's recorded neighbour ids and conditional probabilities through ampnet_amd.tsne.joint_probabilities on
    the device: indptr and indices equal the recording exactly and the values lie within 2^-22 relative of it
    (tsne_reference.joint_bound).  tsne_rows_70x12 and tsne_columns_40x64 record every row and are held whole; the two
    fixtures that record the probabilities of their first rows only take the search model's for the other rows, and the
    entries held to the recording are those whose row and column are both recorded (tsne_reference.recorded_cond) --
    every entry is held to the joint model on the same inputs.  A star whose hub row has N - 1 entries; two calls give
    the same bits."""
    bad = []
    for name in NAMES:
        f = tr.load(name)
        x = f['x'].astype(np.float64)
        cond, pinned = tr.recorded_cond(f, x if str(f['samples']) == 'rows' else x.T)
        idx = torch.as_tensor(f['nbr_idx'].astype(np.int64)).to(dev())
        c32 = torch.as_tensor(cond).to(dev())
        indptr, indices, val = ts.joint_probabilities(idx, c32)
        again = ts.joint_probabilities(idx, c32)
        if not (np.array_equal(indptr.cpu().numpy(), f['indptr']) and np.array_equal(indices.cpu().numpy(), f['indices'])):
            bad.append(f'{name}: indptr / indices differ from the recording')
            continue
        _, _, mv = tr.joint_model(f['nbr_idx'], cond)
        if not (np.abs(val.cpu().numpy() - mv) <= 2.0 ** -22 * mv + 2.0 ** -149).all():
            bad.append(f'{name}: values off the model')
        n = f['val'].size
        rec = f['val'].astype(np.float64)
        if name in ('tsne_rows_70x12', 'tsne_columns_40x64') and not pinned.all():
            bad.append(f'{name}: not recorded whole')
        if not (np.abs(val.cpu().numpy()[:n] - rec) <= tr.joint_bound(rec))[pinned[:n]].all():
            bad.append(f'{name}: values off the recording')
        if not all(torch.equal(a, b) for a, b in zip((indptr, indices, val), again)):
            bad.append(f'{name}: two calls differ')
    N = 1500
    star = torch.zeros(N, 1, dtype=torch.int64, device=dev())
    star[0, 0] = 1
    indptr, indices, val = ts.joint_probabilities(star, torch.ones(N, 1, device=dev()))
    assert int(indptr[1]) == N - 1 and int(indptr[-1]) == 2 * (N - 1) and torch.equal(indices[:N - 1], torch.arange(1, N, device=dev()))
    assert abs(float(val.double().sum()) - 1) < 1e-6 and float(val[0]) == pytest.approx(2.0 / (2 * N), rel=1e-6)
    assert not bad, '\n'.join(bad)


# ------------------------------------------------------------------------------------------------------ repulsion
REPULSION_N = (2, 3, 63, 64, 65, 1000, tr.RUN - 1, tr.RUN, tr.RUN + 1, tr.TILE - 1, tr.TILE, tr.TILE + 1, tr.CHUNK - 1, tr.CHUNK,
               tr.CHUNK + 1)


def run_repulsion(lib, y):
    N = y.shape[0]
    py, pn, pz = Placed(N, 2, torch.float32, y), Placed(N, 2, torch.float32), Placed(1, 1, torch.float64)
    ws = nan_workspace(lib.ampconv_tsne_repulsion_workspace_bytes(N))
    rc = lib.ampconv_tsne_repulsion(py.ptr, N, pn.ptr, pz.ptr, ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return rc, py, pn, pz


def test_repulsion_sweep(lib):
    bad = []
    for N in REPULSION_N:
        for kind in (('start', 'wide', 'outlier') if N <= 1100 else ('outlier',)):
            name = f'repulsion N{N} {kind}'
            y = tr.embedding_case(N, kind)
            rc, py, pn, pz = run_repulsion(lib, y)
            if rc != 0:
                bad.append(f'{name}: rc {rc}')
                continue
            bad += pn.problems(name + ' neg_f') + pz.problems(name + ' Z')
            neg, Z, absf, _ = tr.repulsion_model(y)
            err = np.abs(pn.values() - neg)
            if not (err <= tr.C_NEG * U * absf + 2.0 ** -149).all():
                bad.append(f'{name}: neg_f off by {(err / np.maximum(tr.C_NEG * U * absf, 1e-300)).max():.3g} x the bound')
            if not abs(pz.values()[0, 0] - Z) <= tr.C_Z * U * Z:
                bad.append(f'{name}: Z {pz.values()[0, 0]!r} against {Z!r}')
            rc2, _, pn2, pz2 = run_repulsion(lib, y)
            if rc2 != 0 or not (np.array_equal(pn.bits(), pn2.bits()) and np.array_equal(pz.bits(), pz2.bits())):
                bad.append(f'{name}: two calls differ')
    assert not bad, '\n'.join(bad)


def test_repulsion_excludes_the_point_itself_by_index(lib):
    """A coincident OTHER point adds q = 1 to Z and no force (scikit-learn's tree skips it: include/ampconv.h); the
    point itself adds nothing."""
    y = np.array([[1.0, 2.0], [1.0, 2.0], [4.0, 6.0]], np.float32)
    rc, _, pn, pz = run_repulsion(lib, y)
    assert rc == 0
    q = 1.0 / 26.0
    assert pz.values()[0, 0] == pytest.approx(2 * 1.0 + 4 * q, rel=1e-6)
    assert np.allclose(pn.values()[0], [q * q * -3, q * q * -4], rtol=1e-6) and np.array_equal(pn.values()[0], pn.values()[1])


def test_repulsion_bad_arguments(lib):
    y = tr.embedding_case(10, 'wide')
    py, pn, pz = Placed(10, 2, torch.float32, y), Placed(10, 2, torch.float32), Placed(1, 1, torch.float64)
    ws = nan_workspace(lib.ampconv_tsne_repulsion_workspace_bytes(10))
    s = stream()
    assert lib.ampconv_tsne_repulsion_workspace_bytes(0) == 0 == lib.ampconv_tsne_repulsion_workspace_bytes((1 << 24) + 1)
    for name, args, want in (('N = 0', (py.ptr, 0, pn.ptr, pz.ptr, ws.data_ptr(), ws.numel(), s), BADARG),
                             ('N too large', (py.ptr, (1 << 24) + 1, pn.ptr, pz.ptr, ws.data_ptr(), ws.numel(), s), BADARG),
                             ('NULL y', (None, 10, pn.ptr, pz.ptr, ws.data_ptr(), ws.numel(), s), BADARG),
                             ('misaligned y', (py.ptr + 4, 10, pn.ptr, pz.ptr, ws.data_ptr(), ws.numel(), s), BADARG),
                             ('NULL Z', (py.ptr, 10, pn.ptr, None, ws.data_ptr(), ws.numel(), s), BADARG),
                             ('NULL workspace', (py.ptr, 10, pn.ptr, pz.ptr, None, ws.numel(), s), EWORKSPACE),
                             ('short workspace', (py.ptr, 10, pn.ptr, pz.ptr, ws.data_ptr(), 8, s), EWORKSPACE)):
        assert lib.ampconv_tsne_repulsion(*args) == want, name
    torch.cuda.synchronize()
    assert pn.untouched() and pz.untouched()


# ----------------------------------------------------------------------------------------------------------- step
@pytest.fixture(scope='module')
def step_inputs():
    return tr.step_case(5)


def run_step(lib, c, exag, mom, lr, want_error):
    N, nnz = c['N'], c['indices'].size
    f32, i64 = torch.float32, torch.int64
    p = dict(y=Placed(N, 2, f32, c['y']), out=Placed(N, 2, f32), upd=Placed(N, 2, f32, c['update']), gains=Placed(N, 2, f32, c['gains']),
             neg=Placed(N, 2, f32, c['neg']), Z=Placed(1, 1, torch.float64, [[c['Z']]]), indptr=Placed(N + 1, 1, i64, c['indptr']),
             indices=Placed(nnz, 1, i64, c['indices']), val=Placed(nnz, 1, f32, c['val']), err=Placed(2, 1, torch.float64))
    ws = nan_workspace(lib.ampconv_tsne_step_workspace_bytes(N, nnz))
    rc = lib.ampconv_tsne_step(p['y'].ptr, p['out'].ptr, p['upd'].ptr, p['gains'].ptr, N, p['indptr'].ptr, p['indices'].ptr,
                               p['val'].ptr, nnz, p['neg'].ptr, p['Z'].ptr, exag, mom, lr, 0.01,
                               p['err'].ptr if want_error else None, ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return rc, p


def check_step(name, p, e, c, want_error):
    """The failures of one step against tsne_reference.step_expectation."""
    bad = []
    for k in ('out', 'upd', 'gains') + (('err',) if want_error else ()):
        bad += p[k].problems(f'{name} {k}')
    if not want_error and not p['err'].untouched():
        bad.append(f'{name}: error written without being asked for')
    for k, src in (('y', 'y'), ('neg', 'neg'), ('val', 'val')):
        if not np.array_equal(p[k].values().reshape(-1), np.asarray(c[src], np.float64).reshape(-1)):
            bad.append(f'{name}: the input {k} was changed')
    clear = ~e['band']
    if (~clear).mean() > 0.01:
        bad.append(f'{name}: {(~clear).sum()} elements with an ambiguous gain decision')
    gains = p['gains'].values()
    if not np.array_equal(gains[clear], e['gains'].astype(np.float32).astype(np.float64)[clear]):
        bad.append(f'{name}: gains differ from the fp32 model in {(gains != e["gains"].astype(np.float32))[clear].sum()} elements')
    for k, want, bound in (('upd', e['update'], e['e_update']), ('out', e['y_out'], e['e_y'])):
        err = np.abs(p[k].values() - want)
        if not (err[clear] <= bound[clear]).all():
            bad.append(f'{name}: {k} off by {(err[clear] / bound[clear]).max():.3g} x the bound')
    if want_error:
        got = p['err'].values()[:, 0]
        if not abs(got[0] - e['error']) <= e['e_error']:
            bad.append(f'{name}: error {got[0]!r} against {e["error"]!r} (bound {e["e_error"]:.3e})')
        slack = float(((3.0 * np.abs(e['grad']) + e['e_grad']) ** 2)[~clear].sum())
        if not abs(got[1] - e['norm2']) <= e['e_norm2'] + slack:
            bad.append(f'{name}: squared norm {got[1]!r} against {e["norm2"]!r} (bound {e["e_norm2"]:.3e})')
    return bad


def test_step_sweep(lib, step_inputs):
    """Row lengths 0, 1, 63, 64, 65, a hub of N - 1 (three parts) and a row of 1100 (two parts); exaggeration 1 and 12;
    with and without the error; two calls give the same bits."""
    c, bad = step_inputs, []
    for exag, mom, lr in ((1.0, 0.8, 200.0), (12.0, 0.5, 200.0)):
        e = tr.step_expectation(c, exag, mom, lr)
        for want_error in (False, True):
            name = f'step exaggeration {exag} error {want_error}'
            rc, p = run_step(lib, c, exag, mom, lr, want_error)
            if rc != 0:
                bad.append(f'{name}: rc {rc}')
                continue
            bad += check_step(name, p, e, c, want_error)
            rc2, p2 = run_step(lib, c, exag, mom, lr, want_error)
            if rc2 != 0 or any(not np.array_equal(p[k].bits(), p2[k].bits()) for k in ('out', 'upd', 'gains')):
                bad.append(f'{name}: two calls differ')
    assert not bad, '\n'.join(bad)


def test_step_bad_arguments(lib, step_inputs):
    c = step_inputs
    N, nnz = c['N'], c['indices'].size
    rc, p = run_step(lib, c, 1.0, 0.8, 200.0, False)
    assert rc == 0
    before = {k: p[k].bits().copy() for k in ('out', 'upd', 'gains')}
    ws = nan_workspace(lib.ampconv_tsne_step_workspace_bytes(N, nnz))
    base = dict(y=p['y'].ptr, out=p['out'].ptr, upd=p['upd'].ptr, gains=p['gains'].ptr, N=N, indptr=p['indptr'].ptr,
                indices=p['indices'].ptr, val=p['val'].ptr, nnz=nnz, neg=p['neg'].ptr, Z=p['Z'].ptr, ws=ws.data_ptr(), wsn=ws.numel())
    for name, change, want in (('y_in == y_out', dict(out=p['y'].ptr), BADARG), ('N = 0', dict(N=0), BADARG), ('nnz < 0', dict(nnz=-1), BADARG),
                               ('NULL update', dict(upd=None), BADARG), ('NULL indptr', dict(indptr=None), BADARG),
                               ('NULL indices', dict(indices=None), BADARG), ('NULL Z', dict(Z=None), BADARG),
                               ('misaligned gains', dict(gains=p['gains'].ptr + 4), BADARG), ('NULL workspace', dict(ws=None), EWORKSPACE),
                               ('short workspace', dict(wsn=64), EWORKSPACE)):
        a = dict(base)
        a.update(change)
        got = lib.ampconv_tsne_step(a['y'], a['out'], a['upd'], a['gains'], a['N'], a['indptr'], a['indices'], a['val'], a['nnz'],
                                    a['neg'], a['Z'], 1.0, 0.8, 200.0, 0.01, None, a['ws'], a['wsn'], stream())
        assert got == want, name
    torch.cuda.synchronize()
    assert all(np.array_equal(before[k], p[k].bits()) for k in before)
    assert lib.ampconv_tsne_step_workspace_bytes(0, 5) == 0 == lib.ampconv_tsne_step_workspace_bytes(5, -1)


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module', params=NAMES)
def fit(request):
    """One fixture, its input on the device and ONE full default run, shared by the tests below."""
    from ampnet_amd import tsne
    f = tr.load(request.param)
    f['name'] = request.param
    f['samples'] = str(f['samples'])
    x = f['x'].astype(np.float64)
    f['X'] = x if f['samples'] == 'rows' else x.T
    f['xd'] = torch.as_tensor(f['x']).to(dev())
    f['run'] = tsne(f['xd'], perplexity=float(f['perplexity']), samples=f['samples'])
    return f


def test_affinities_from_our_own_neighbour_search(fit):
    """gap > 2 B (tools/make_golden_tsne.py): no fp32 evaluation of the distances can change a neighbour set, so the
    CSR's ids equal scikit-learn's exactly.  The values are held to the models run on OUR distances at 2^-22 -- the
    search's branch decisions are those of the model unless one lies within the fp64 noise of the tolerance.  They
    cannot equal the recording to rounding: our distances are fp32 evaluations (off by up to B, scikit-learn's by a
    float32 ulp), which moves the entropy by more than the margin of a stop decision, and two searches that stop a
    bisection step apart differ by up to the tolerance in H.  tsne_reference.search_sensitivity derives what that can
    do to each conditional probability and tsne_reference.joint_sensitivity to an entry of P, which is held to the
    recording within that plus the 2^-22 of the roundings.  (The bound is 3e-4 to 6e-3 of the median entry, most of it the worst-case B, and
    loose for a row's far tail, whose probabilities do move that much when a stop decision falls the other way; the
    test prints how much of it was used.)"""
    f, k = fit, int(fit['k'])
    idx, d2 = ts.nearest(f['xd'], k, f['samples'])
    want_idx, want_d2 = tr.exact_neighbors(f['X'], k)
    assert np.array_equal(np.sort(idx.cpu().numpy(), 1), np.sort(want_idx, 1))
    assert np.abs(np.sort(d2.cpu().numpy().astype(np.float64), 1) - want_d2).max() <= float(f['bound'])
    assert (d2[:, 1:] >= d2[:, :-1]).all()
    indptr, indices, val = (t.cpu().numpy() for t in f['run'].affinities)
    assert np.array_equal(indptr, f['indptr']) and np.array_equal(indices, f['indices'])
    cond, beta, margin = tr.search_model(d2.cpu().numpy(), float(f['perplexity']))
    _, _, mv = tr.joint_model(idx.cpu().numpy(), tr.cond_f32(cond))
    if margin >= 1e-10:
        assert (np.abs(val - mv) <= 2.0 ** -22 * mv + 2.0 ** -149).all()
        assert np.array_equal(f['run'].beta.cpu().numpy(), beta)
    n = f['val'].size
    rec = f['val'].astype(np.float64)
    B = float(f['bound']) + 2.0 ** -23 * float(want_d2.max())
    S = tr.joint_sensitivity(idx.cpu().numpy(), d2.cpu().numpy(), float(f['perplexity']), B)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    bound = S[rows, indices][:n] + tr.joint_bound(rec)
    print(f"{f['name']}: bound / value: median {np.median(bound / np.maximum(rec, 2.0 ** -126)):.3e}; largest difference to the "
          f"recording {(np.abs(val[:n] - rec) / bound).max():.3e} of the bound, {(np.abs(val[:n] - rec) / np.maximum(rec, 2.0 ** -126)).max():.3e} relative")
    assert (np.abs(val[:n] - rec) <= bound).all()


def test_ten_iterations_follow_the_model(lib, fit):
    """Ten iterations from init='pca', each held to the fp64 model of ONE step from the state the kernels themselves left
    (y, update, gains read back every iteration), within the step bound and with the ambiguity rule of the step test
    (capped at 1 %).  The state is handed on rather than a bound compounded: with learning_rate 50 and the exaggerated P
    the map of one iteration expands differences (tests/test_tsne_cpu.py asserts the factor on the smallest fixture), so
    a compounded bound would allow anything after a few iterations.  What this leaves: every step is pinned, tighter than
    a compounded bound would, but the LOOP as a whole -- the schedule, the hand-over between the two stages -- is pinned
    only by the KL acceptance, n_iter and the bit-equality of two runs (test_full_run_against_scikit_learn) and by the
    schedule test on the host."""
    f = fit
    indptr, indices, val = f['run'].affinities
    M = f['X'].shape[0]
    lr = max(M / 12.0 / 4.0, 50.0)
    state = ts.Descent(ts.pca_start(f['xd'], f['samples']), indptr, indices, val)
    csr = dict(N=M, indptr=indptr.cpu().numpy(), indices=indices.cpu().numpy(), val=val.cpu().numpy())
    bad = []
    for it in range(10):
        c = dict(csr, y=state.y[0].cpu().numpy(), update=state.update.cpu().numpy(), gains=state.gains.cpu().numpy())
        neg, Z, absf, _ = tr.repulsion_model(c['y'])
        out = state.step(12.0, 0.5, lr, True)
        got_neg, got_Z = state.neg.cpu().numpy().astype(np.float64), float(state.Z.cpu())
        if not ((np.abs(got_neg - neg) <= tr.C_NEG * U * absf + 2.0 ** -149).all() and abs(got_Z - Z) <= tr.C_Z * U * Z):
            bad.append(f'iteration {it}: repulsion off its bound')
        c.update(neg=state.neg.cpu().numpy(), Z=got_Z)               # the step is held to ITS inputs
        e = tr.step_expectation(c, 12.0, 0.5, lr)
        clear = ~e['band']
        if (~clear).mean() > 0.01:
            bad.append(f'iteration {it}: {(~clear).sum()} ambiguous elements')
        if not np.array_equal(state.gains.cpu().numpy()[clear], e['gains'].astype(np.float32)[clear]):
            bad.append(f'iteration {it}: gains')
        for nm, got, want, bound in (('update', state.update, e['update'], e['e_update']), ('y', state.y[0], e['y_out'], e['e_y'])):
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            if not (err[clear] <= bound[clear]).all():
                bad.append(f'iteration {it}: {nm} off by {(err[clear] / bound[clear]).max():.3g} x the bound')
        if not abs(out[0] - e['error']) <= e['e_error']:
            bad.append(f'iteration {it}: error {out[0]!r} against {e["error"]!r}')
    assert not bad, '\n'.join(bad)


def test_full_run_against_scikit_learn(fit):
    """The final KL divergence, recomputed from OUR embedding by the fp64 model (never taken from the code under test), is
    at most 1.10 x the largest of scikit-learn's four recorded seeds; neighbor_preservation is not below that of the
    recorded scikit-learn embedding less 10 % of it (the relative reading, the stricter of the two); n_iter is scikit-learn's for a run that no stopping rule ends; the
    reported divergence is the model's; a second run gives the same bits."""
    from ampnet_amd import neighbor_preservation, tsne
    f, run = fit, fit['run']
    y = run.embedding.cpu().numpy()
    assert run.embedding.dtype == torch.float32 and y.shape == (f['X'].shape[0], 2) and np.isfinite(y).all()
    indptr, indices, val = (t.cpu().numpy() for t in run.affinities)
    kl = tr.kl_model(y, indptr, indices, val)
    print(f"{f['name']}: KL {kl:.4f} (reported {run.kl_divergence:.4f}), scikit-learn {f['kl_auto']}")
    assert kl <= 1.10 * float(f['kl_auto'].max())
    assert run.n_iter == 999
    # the reported value is that of the last iteration's INPUT (as scikit-learn's): close to, not equal to, the final one
    assert run.kl_divergence == pytest.approx(kl, rel=0.05, abs=1e-3)
    again = tsne(f['xd'], perplexity=float(f['perplexity']), samples=f['samples'])
    assert torch.equal(again.embedding, run.embedding) and again.kl_divergence == run.kl_divergence and again.n_iter == run.n_iter
    k = min(10, int(f['k']))
    xs = torch.as_tensor(f['X'].astype(np.float32)).to(dev())
    ours = neighbor_preservation(xs, run.embedding, k)
    theirs = tr.neighbor_preservation_model(f['X'], f['emb_auto'], k)
    print(f"{f['name']}: neighbor preservation {ours:.3f}, scikit-learn's embedding {theirs:.3f}")
    assert ours >= 0.90 * theirs
    assert ours == pytest.approx(tr.neighbor_preservation_model(f['X'], y, k), abs=0.02)
    z = run.standardized().cpu().numpy()
    assert np.allclose(z.mean(0), 0, atol=1e-5) and np.allclose(z.std(0), 1, atol=1e-5)


def test_reference_learning_rate_and_stopping_rules(fit):
    """The reference script's learning_rate=10 against scikit-learn's recording; min_grad_norm ends each stage at its
    first check (n_iter 99, as the model's schedule), and an init tensor and neighbors=(idx, dist2) are taken."""
    from ampnet_amd import tsne
    f = fit
    kw = dict(perplexity=float(f['perplexity']), samples=f['samples'])
    run = tsne(f['xd'], learning_rate=10, **kw)
    indptr, indices, val = (t.cpu().numpy() for t in run.affinities)
    kl = tr.kl_model(run.embedding.cpu().numpy(), indptr, indices, val)
    print(f"{f['name']}: learning_rate 10: KL {kl:.4f}, scikit-learn {f['kl_lr10']}")
    assert kl <= 1.10 * float(f['kl_lr10'].max()) and run.n_iter == 999 and run.learning_rate == 10.0
    idx, d2 = ts.nearest(f['xd'], int(f['k']), f['samples'])
    y0 = ts.pca_start(f['xd'], f['samples'])
    early = tsne(f['xd'], min_grad_norm=1e30, init=y0, neighbors=(idx, d2), **kw)
    want = tr.descend(lambda i, w: (1.0, 1.0), tr.descend(lambda i, w: (1.0, 1.0), 0, 250, 250, 1e30)[1] + 1, 1000, 300, 1e30)[1]
    assert early.n_iter == want == 99
    assert all(torch.equal(a, b) for a, b in zip(early.affinities, fit['run'].affinities))


def test_bf16_rows_are_widened_on_load():
    """bfloat16 input (widened on load by knn and pca): the affinities are those of the models run on the bf16 VALUES
    wherever no neighbour decision is within the fp32 distance bound, the run is finite and two runs give the same bits."""
    from ampnet_amd import tsne
    f = tr.load('tsne_rows_70x12')
    xb = torch.as_tensor(f['x']).to(dev()).bfloat16()
    run, again = tsne(xb, perplexity=5.0), tsne(xb, perplexity=5.0)
    assert run.embedding.dtype == torch.float32 and torch.isfinite(run.embedding).all() and run.n_iter == 999
    assert torch.equal(run.embedding, again.embedding) and all(torch.equal(a, b) for a, b in zip(run.affinities, again.affinities))
    X = xb.float().cpu().numpy().astype(np.float64)
    k = int(f['k'])
    idx, far = tr.exact_neighbors(X, k + 1)
    bound = (X.shape[1] + 4) * 2.0 ** -24 * 2.0 * (X * X).sum(1).max()
    indptr, indices, val = (t.cpu().numpy() for t in run.affinities)
    assert (np.diff(indptr) >= k).all() and abs(val.astype(np.float64).sum() - 1) < 1e-5
    if (far[:, k] - far[:, k - 1]).min() > 2 * bound:
        cond, _, _ = tr.search_model(far[:, :k].astype(np.float32), 5.0)
        mp, mi, _ = tr.joint_model(idx[:, :k], tr.cond_f32(cond))
        assert np.array_equal(indptr, mp) and np.array_equal(indices, mi)
    kl = tr.kl_model(run.embedding.cpu().numpy(), indptr, indices, val)
    assert np.isfinite(kl) and run.kl_divergence == pytest.approx(kl, rel=0.05, abs=1e-3)


def test_merged_neighbours_double_the_chunks_when_one_is_exhausted(monkeypatch):
    """More than 64 neighbours come from knn over key chunks (key s in chunk s mod C).  600 points at k = 91 start with
    C = 4 chunks of 150 keys.  The 100 points with ids 0, 4, 8, ... form one tight cluster, so each of them finds all its
    91 nearest in chunk 0, which can give 64: the search has to notice and double to C = 8 (two chunks of 50 cluster
    points, none exhausted).  Small integer coordinates: the fp32 distances are exact, so the sorted distances of every
    row equal the exact ones (ties make the ids ambiguous, not the distances), and the ids are checked through them."""
    rng = np.random.default_rng(3)
    N, k = 600, 91
    x = rng.integers(-40, 41, (N, 3)).astype(np.float32)
    x[0:400:4] = rng.integers(-3, 4, (100, 3)) + np.array([300, 300, 300])
    calls = []
    real = ts.knn
    monkeypatch.setattr(ts, 'knn', lambda *a, **kw: (calls.append(kw['keys'].numel()), real(*a, **kw))[1])
    xd = torch.as_tensor(x).to(dev())
    idx, d2 = ts.nearest(xd, k)
    assert calls == [150] * 4 + [75] * 8                       # one attempt at C = 4, one at C = 8
    _, want = tr.exact_neighbors(x, k)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy().astype(np.float64)
    assert np.array_equal(d2, want)
    x64 = x.astype(np.float64)
    assert np.array_equal(((x64[:, None, :] - x64[idx]) ** 2).sum(2), want) and (idx != np.arange(N)[:, None]).all()
    assert all(len(set(row)) == k for row in idx.tolist())
