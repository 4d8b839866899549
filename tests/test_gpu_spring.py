"""ampnet_amd.spring on the GPU against the models of tests/spring_reference.py: the start, the repulsion and the step
kernel by kernel through ctypes, whole trajectories driven from the kernels' own positions, networkx's recorded values,
then spring_layout() end to end.

The bounds (u = 2^-24), all from spring_reference:

  repulsion    |rep - model| <= (RUN + 16) u sum_j |term_j| per coordinate (the header's bound: a run of RUN float32
               additions and the pair's own roundings).
  step         |y_out - model| <= iteration_bound: the two sums' bounds through the displacement, times 2 t / len (the
               normalisation) or t / 0.1 (the floored branch), plus the float32 roundings of delta and y_in + delta.  Rows
               whose raw length is within the displacement's bound of 0.01 could take the other branch: not compared.
  networkx     at 1 and 5 iterations within 4 x the deviation of the float32-arithmetic model from the fixture, floor
               1e-6 (the reference's own rounding sensitivity; the figures are in profiles/spring.md).
"""
import importlib
import math

import numpy as np
import pytest
import torch

import spring_reference as sr
from edge_runner import stream

from ampnet_amd import _lib

spring = importlib.import_module('ampnet_amd.spring')
pytestmark = pytest.mark.gpu

BADARG, EWORKSPACE = -1, -3
PART = sr.PART
NAN = float('nan')


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


@pytest.fixture(scope='module')
def fixtures():
    return {name: sr.load(name) for name in sr.CASES}


def dev():
    return torch.device('cuda:0')


def to_dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return t.to(dev(), dtype) if dtype is not None else t.to(dev())


def graph_of(f):
    return sr.adjacency_model(f['edge_index'], f['N'], None, f['symmetric'])


def new_state(t=0.07, dt=0.001, ran=0, done=0):
    s = torch.zeros(4, dtype=torch.float64, device=dev())
    s[0], s[1] = t, dt
    s.view(torch.int64)[2], s.view(torch.int64)[3] = ran, done
    return s


def read_state(s):
    host = s.cpu()
    return float(host[0]), float(host[1]), int(host.view(torch.int64)[2]), int(host.view(torch.int64)[3])


def call_repulsion(lib, y, state=None, rep=None):
    N, dim = y.shape
    rep = torch.full((N, dim), NAN, dtype=torch.float64, device=dev()) if rep is None else rep
    ws = torch.empty(max(int(lib.ampconv_spring_repulsion_workspace_bytes(N, dim)), 256), dtype=torch.uint8, device=dev())
    rc = lib.ampconv_spring_repulsion(y.data_ptr(), N, dim, rep.data_ptr(), _lib.ptr(state), ws.data_ptr(), ws.numel(), stream())
    assert rc == 0
    return rep


def call_step(lib, y, graph, rep, k, state, threshold=1e-4, val=True, fixed=None, part=None):
    """(y_out, rc): one ampconv_spring_step (part None) or ampconv_spring_step_split into a NaN-filled y_out."""
    N, dim = y.shape
    indptr, indices, v = graph
    out = torch.full((N, dim), NAN, dtype=torch.float32, device=dev())
    nnz = indices.numel()
    ws = torch.empty(max(int(lib.ampconv_spring_step_workspace_bytes(N, nnz, dim)), 256), dtype=torch.uint8, device=dev())
    head = (y.data_ptr(), out.data_ptr(), N, dim, indptr.data_ptr(), _lib.ptr(indices if nnz else None), _lib.ptr(v if val else None), nnz,
            _lib.ptr(fixed), rep.data_ptr(), k, threshold, state.data_ptr())
    if part is None:
        rc = lib.ampconv_spring_step(*head, ws.data_ptr(), ws.numel(), stream())
    else:
        rc = lib.ampconv_spring_step_split(*head, part, ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return out, rc


# ----------------------------------------------------------------------------------------------------------- the start
def test_start_equals_the_integer_model():
    for N, dim, seed in ((1, 2, 0), (257, 2, 0), (1000, 3, 5), (300, 2, 2 ** 63 + 11), (64, 3, -3)):
        y = spring.uniform_start(N, dim, seed, dev())
        assert y.dtype == torch.float32 and tuple(y.shape) == (N, dim)
        assert np.array_equal(y.cpu().numpy(), sr.uniform_start_model(N, dim, seed)), (N, dim, seed)
    assert not torch.equal(spring.uniform_start(100, 2, 0, dev()), spring.uniform_start(100, 2, 1, dev()))


def test_adjacency_on_the_device_equals_the_model(fixtures):
    for name in sr.CASES:
        f = fixtures[name]
        got = spring.adjacency(to_dev(f['edge_index']), f['N'], None, f['symmetric'])
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, (f['a_indptr'], f['a_indices'], f['a_val']))), name
    rng = np.random.default_rng(5)
    ei, w = rng.integers(0, 30, (2, 400)), rng.random(400).astype(np.float32)
    got = spring.adjacency(to_dev(ei), 30, to_dev(w), False)
    again = spring.adjacency(to_dev(ei), 30, to_dev(w), False)
    assert all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(got, sr.adjacency_model(ei, 30, w, False)))
    assert all(torch.equal(p, q) for p, q in zip(got, again))


# ----------------------------------------------------------------------------------------------------------- repulsion
REPULSION_N = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 8200)      # lane, run, query-tile, chunk boundaries


def repulsion_points(N, dim):
    """Uniform points with coincident ones and pairs closer than the clamp's 0.01."""
    rng = np.random.default_rng(1000 * N + dim)
    y = rng.random((N, dim), dtype=np.float32)
    for a, b in ((0, 1), (N // 2, N - 1), (N // 3, N // 3 + 1)):
        if a != b and b < N:
            y[b] = y[a]                                               # coincident: the term is exactly 0
    for a, b, off in ((2, 3, 0.003), (N // 4, N // 4 + 5, 0.0007), (N - 2, 5, 0.009)):
        if 0 <= a < N and 0 <= b < N and a != b and N > 8:
            y[b] = y[a] + np.float32(off) * np.float32(1.0 if dim == 2 else 0.5)      # closer than 0.01: the clamp
    return y


@pytest.mark.parametrize('dim', (2, 3))
def test_repulsion_sweep(lib, dim):
    bad = []
    for N in REPULSION_N:
        name = f'repulsion N{N} dim{dim}'
        y = repulsion_points(N, dim)
        yd = to_dev(y)
        before = yd.clone()
        rep, again = call_repulsion(lib, yd), call_repulsion(lib, yd)
        torch.cuda.synchronize()
        want, mag = sr.repulsion_model(y)
        got = rep.cpu().numpy()
        bound = sr.repulsion_bound(mag)
        err = np.abs(got - want)
        used = float((err / np.maximum(bound, 1e-300)).max())
        print(f'{name}: largest error {used:.3f} of the bound, largest |rep| {np.abs(want).max():.3e}')
        if not (np.isfinite(got).all() and (err <= bound).all()):
            bad.append(f'{name}: off by {used:.3g} x the bound')
        if not torch.equal(rep, again):
            bad.append(f'{name}: two calls differ')
        if not torch.equal(yd, before):
            bad.append(f'{name}: the positions were written')
        if N > 8:
            d = np.sqrt(((y[:, None, :].astype(np.float64) - y[None, :, :]) ** 2).sum(-1)) if N <= 1025 else None
            if d is not None and not ((d == 0).sum() > N and ((d > 0) & (d < 0.01)).any()):
                bad.append(f'{name}: the case holds no coincident or no clamped pair')
    assert not bad, '\n'.join(bad)


def test_repulsion_bad_arguments_and_the_latch(lib):
    y = to_dev(repulsion_points(100, 2))
    rep = torch.full((100, 2), NAN, dtype=torch.float64, device=dev())
    ws = torch.empty(max(int(lib.ampconv_spring_repulsion_workspace_bytes(100, 2)), 256), dtype=torch.uint8, device=dev())
    base = dict(y=y.data_ptr(), N=100, dim=2, rep=rep.data_ptr(), state=None, ws=ws.data_ptr(), wsn=ws.numel())
    for name, change, want in (('N = 0', dict(N=0), BADARG), ('N too large', dict(N=(1 << 24) + 1), BADARG), ('dim = 1', dict(dim=1), BADARG),
                               ('dim = 4', dict(dim=4), BADARG), ('NULL y', dict(y=None), BADARG), ('NULL rep', dict(rep=None), BADARG),
                               ('misaligned y', dict(y=y.data_ptr() + 4), BADARG), ('misaligned state', dict(state=rep.data_ptr() + 4), BADARG),
                               ('NULL workspace', dict(ws=None), EWORKSPACE), ('short workspace', dict(wsn=64), EWORKSPACE)):
        a = dict(base)
        a.update(change)
        assert lib.ampconv_spring_repulsion(a['y'], a['N'], a['dim'], a['rep'], a['state'], a['ws'], a['wsn'], stream()) == want, name
    torch.cuda.synchronize()
    assert torch.isnan(rep).all()
    call_repulsion(lib, y, new_state(done=1), rep)                    # done: rep is left as it is
    torch.cuda.synchronize()
    assert torch.isnan(rep).all()
    call_repulsion(lib, y, new_state(done=0), rep)
    torch.cuda.synchronize()
    assert torch.equal(rep, call_repulsion(lib, y))
    assert lib.ampconv_spring_start(None, 5, 2, 0, stream()) == BADARG and lib.ampconv_spring_start(y.data_ptr(), 5, 5, 0, stream()) == BADARG


# ---------------------------------------------------------------------------------------------------------------- step
ROW_LENGTHS = (0, 1, 63, 64, 65, PART, PART + 1, 3 * PART + 5)        # the last one is the hub


@pytest.fixture(scope='module')
def ladder():
    """A CSR whose first rows have the lengths of ROW_LENGTHS (distinct ascending columns, self-loops and a column of a
    coincident point among them), every later row 0 to 3 entries; weights in [0.5, 1.5)."""
    rng = np.random.default_rng(7)
    N = 3 * PART + 40
    lengths = list(ROW_LENGTHS) + [int(v) for v in rng.integers(0, 4, N - len(ROW_LENGTHS))]
    cols = [np.sort(rng.choice(N, n, replace=False)) for n in lengths]
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    indices = np.concatenate(cols).astype(np.int64)
    val = (0.5 + rng.random(indices.size)).astype(np.float32)
    return dict(N=N, graph=(indptr, indices, val), dgraph=tuple(to_dev(a) for a in (indptr, indices, val)))


def ladder_points(N, dim):
    y = np.random.default_rng(dim).random((N, dim), dtype=np.float32)
    y[N - 1] = y[7]                                                   # a point that coincides with the hub
    y[N - 2] = y[7] + np.float32(0.002)                               # and one inside the clamp
    return y


@pytest.mark.parametrize('dim', (2, 3))
def test_step_on_the_row_length_ladder(lib, ladder, dim):
    N, (indptr, indices, val), dgraph = ladder['N'], ladder['graph'], ladder['dgraph']
    assert tuple(np.diff(indptr)[:len(ROW_LENGTHS)]) == ROW_LENGTHS
    y = ladder_points(N, dim)
    yd = to_dev(y)
    k, t, dt = 1.0 / math.sqrt(N), 0.07, 0.001
    rep_model, _ = sr.repulsion_model(y)
    rep = to_dev(rep_model)
    bad = []
    for weights in (True, False):
        name = f'dim{dim} {"weighted" if weights else "val NULL"}'
        state = new_state(t, dt)
        out, rc = call_step(lib, yd, dgraph, rep, k, state, val=weights)
        assert rc == 0
        info = sr.iteration_model(y, indptr, indices, val if weights else None, k, t, rep=rep_model)
        bound, sure = sr.iteration_bound(info, k, t)
        got = out.cpu().numpy()
        err = np.abs(got.astype(np.float64) - info['y_out'])
        used = float((err / bound)[sure].max())
        print(f'{name}: largest error {used:.3f} of the bound over {int(sure.sum())} of {N} rows; err {info["err"]:.3e}')
        if not (np.isfinite(got).all() and (err <= bound)[sure].all() and sure[:len(ROW_LENGTHS)].all()):
            bad.append(f'{name}: y_out off by {used:.3g} x the bound, or a ladder row not compared')
        if not torch.equal(yd, to_dev(y)):
            bad.append(f'{name}: y_in was written')
        if read_state(state) != (t - dt, dt, 1, int(info['err'] < 1e-4)):
            bad.append(f'{name}: state {read_state(state)}')
        for part in (64, 1024, 4096):
            other, rc = call_step(lib, yd, dgraph, rep, k, new_state(t, dt), val=weights, part=part)
            if rc != 0 or not torch.equal(other, out):
                bad.append(f'{name}: part {part}: the bits differ from ampconv_spring_step')
        if not weights:
            ones = (dgraph[0], dgraph[1], torch.ones_like(dgraph[2]))
            other, _ = call_step(lib, yd, ones, rep, k, new_state(t, dt))
            if not torch.equal(other, out):
                bad.append(f'{name}: val == NULL differs from a weight-1 array')
        # a fixed mask: those rows keep their bits, the others move as before (the iteration is synchronous)
        mask = torch.zeros(N, dtype=torch.uint8, device=dev())
        mask[[0, 5, 7, 100, N - 1]] = 1
        state = new_state(t, dt)
        held, _ = call_step(lib, yd, dgraph, rep, k, state, val=weights, fixed=mask)
        m = mask.bool()
        if not (torch.equal(held[m].view(torch.int32), yd[m].view(torch.int32)) and torch.equal(held[~m], out[~m])):
            bad.append(f'{name}: the fixed mask')
        want_err = info['delta'].astype(np.float64).copy()
        want_err[m.cpu().numpy()] = 0
        if read_state(state)[2:] != (1, int(np.sqrt((want_err ** 2).sum()) / N < 1e-4)):
            bad.append(f'{name}: the state under a fixed mask')
    assert not bad, '\n'.join(bad)


def test_step_done_decision_follows_the_threshold(lib, ladder):
    """The same step under thresholds on either side of its sqrt(sum delta^2) / N: done is the comparison."""
    N, (indptr, indices, val), dgraph = ladder['N'], ladder['graph'], ladder['dgraph']
    y = ladder_points(N, 2)
    rep_model, _ = sr.repulsion_model(y)
    k = 1.0 / math.sqrt(N)
    info = sr.iteration_model(y, indptr, indices, val, k, 0.07, rep=rep_model)
    for factor, want in ((1.01, 1), (0.99, 0)):
        state = new_state(0.07, 0.001)
        _, rc = call_step(lib, to_dev(y), dgraph, to_dev(rep_model), k, state, threshold=factor * info['err'])
        assert rc == 0 and read_state(state)[3] == want, factor


def test_three_collinear_points_without_edges(lib):
    """(-a, 0), (0, 0), (a, 0): the two repulsions of the middle point cancel exactly, its length 0 takes the
    `len < 0.01 -> 0.1` branch (0 / 0 otherwise) and it stays where it is; the outer points move apart by t."""
    a, t = 0.25, 0.1
    for dim in (2, 3):
        y = np.zeros((3, dim), np.float32)
        y[0, 0], y[2, 0] = -a, a
        yd = to_dev(y)
        rep = call_repulsion(lib, yd)
        graph = (torch.zeros(4, dtype=torch.int64, device=dev()), torch.zeros(0, dtype=torch.int64, device=dev()), torch.zeros(0, device=dev()))
        state = new_state(t, 0.01)
        out, rc = call_step(lib, yd, graph, rep, 1.0 / math.sqrt(3), state)
        assert rc == 0
        got, r = out.cpu().numpy(), rep.cpu().numpy()
        assert (r[1] == 0).all() and r[0, 0] == -r[2, 0] and abs(r[0, 0] + 1.5 / a) < 1e-5
        assert (got[1] == 0).all() and not np.signbit(got[1]).any()
        assert np.allclose(got[[0, 2], 0], [-a - t, a + t], rtol=1e-6, atol=0) and (got[:, 1:] == 0).all()
        assert read_state(state) == (t - 0.01, 0.01, 1, 0)


def test_done_latch_freezes_everything(lib, ladder):
    N, dgraph = ladder['N'], ladder['dgraph']
    yd = to_dev(ladder_points(N, 2))
    rep = torch.full((N, 2), NAN, dtype=torch.float64, device=dev())                  # never read once done is set
    for part in (None, 64):
        state = new_state(0.0123, 0.001, ran=17, done=1)
        out, rc = call_step(lib, yd, dgraph, rep, 0.02, state, part=part)
        assert rc == 0 and torch.equal(out.view(torch.int32), yd.view(torch.int32))
        assert read_state(state) == (0.0123, 0.001, 17, 1)


def test_step_bad_arguments(lib):
    N, dim = 10, 2
    y = torch.rand(N, dim, device=dev())
    out = torch.full((N, dim), NAN, device=dev())
    indptr, indices, val = torch.arange(N + 1, device=dev()), torch.arange(N, device=dev()).roll(1), torch.ones(N, device=dev())
    rep = torch.zeros(N, dim, dtype=torch.float64, device=dev())
    state = new_state()
    ws = torch.empty(max(int(lib.ampconv_spring_step_workspace_bytes(N, N, dim)), 256), dtype=torch.uint8, device=dev())
    base = dict(y=y.data_ptr(), out=out.data_ptr(), N=N, dim=dim, indptr=indptr.data_ptr(), indices=indices.data_ptr(), val=val.data_ptr(), nnz=N,
                rep=rep.data_ptr(), k=0.3, state=state.data_ptr(), part=64, ws=ws.data_ptr(), wsn=ws.numel())
    for name, change, want in (('y_in == y_out', dict(out=y.data_ptr()), BADARG), ('N = 0', dict(N=0), BADARG), ('dim = 1', dict(dim=1), BADARG),
                               ('dim = 4', dict(dim=4), BADARG), ('nnz < 0', dict(nnz=-1), BADARG), ('k = 0', dict(k=0.0), BADARG),
                               ('k < 0', dict(k=-1.0), BADARG), ('k nan', dict(k=NAN), BADARG), ('k inf', dict(k=float('inf')), BADARG),
                               ('part 32', dict(part=32), BADARG), ('part 100', dict(part=100), BADARG), ('NULL indptr', dict(indptr=None), BADARG),
                               ('NULL indices', dict(indices=None), BADARG), ('NULL rep', dict(rep=None), BADARG), ('NULL state', dict(state=None), BADARG),
                               ('misaligned y', dict(y=y.data_ptr() + 4), BADARG), ('misaligned val', dict(val=val.data_ptr() + 2), BADARG),
                               ('misaligned state', dict(state=state.data_ptr() + 4), BADARG), ('NULL workspace', dict(ws=None), EWORKSPACE),
                               ('short workspace', dict(wsn=8), EWORKSPACE)):
        a = dict(base)
        a.update(change)
        got = lib.ampconv_spring_step_split(a['y'], a['out'], a['N'], a['dim'], a['indptr'], a['indices'], a['val'], a['nnz'], None, a['rep'],
                                            a['k'], 1e-4, a['state'], a['part'], a['ws'], a['wsn'], stream())
        assert got == want, name
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and read_state(state) == (0.07, 0.001, 0, 0)
    # out-of-range columns are clamped, never followed out of the array
    wild = indices.clone()
    wild[0], wild[1] = -5, N + 100
    got, rc = call_step(lib, y, (indptr, wild, val), rep, 0.3, new_state())
    clamped = indices.clone()
    clamped[0], clamped[1] = 0, N - 1
    want, _ = call_step(lib, y, (indptr, clamped, val), rep, 0.3, new_state())
    assert rc == 0 and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize('name', ('sbm64', 'grid8', 'sbm512'))
def test_trajectory_from_the_kernels_own_positions(fixtures, name):
    """50 iterations; at every one the fp64 model is driven from the kernels' y_in, so nothing compounds."""
    f = fixtures[name]
    graph = graph_of(f)
    N, k = f['N'], 1.0 / math.sqrt(f['N'])
    lay = spring.SpringLayout(to_dev(f['pos0']), *(to_dev(a) for a in graph), k, 50, 1e-4)
    t, dt = sr.temperature_model(f['pos0'], 50)
    assert read_state(lay.state) == (t, dt, 0, 0)
    bad, worst, skipped, close = [], 0.0, 0, 0
    for it in range(50):
        y_in = lay.y[0].cpu().numpy()
        lay.step()
        got = lay.y[0].cpu().numpy()
        info = sr.iteration_model(y_in, *graph, k, t)
        bound, sure = sr.iteration_bound(info, k, t)
        err = np.abs(got.astype(np.float64) - info['y_out'])
        worst = max(worst, float((err / bound)[sure].max()))
        skipped += int((~sure).sum())
        if not (np.isfinite(got).all() and (err <= bound)[sure].all()):
            bad.append(f'iteration {it}: y_out off by {(err / bound)[sure].max():.3g} x the bound')
        t -= dt
        gt, gdt, ran, done = read_state(lay.state)
        if (gt, gdt, ran) != (t, dt, it + 1):
            bad.append(f'iteration {it}: state {(gt, gdt, ran)} against {(t, dt, it + 1)}')
        if abs(info['err'] - 1e-4) > 1e-3 * 1e-4:
            if done != int(info['err'] < 1e-4):
                bad.append(f'iteration {it}: done = {done}, the model has {info["err"]:.6e}')
        else:
            close += 1
        if done:
            break
    print(f'{name}: largest error {worst:.3f} of the bound, {skipped} rows not compared, {close} decisions too close to call')
    assert skipped <= N and not bad, '\n'.join(bad)


def test_path2_stops_after_43_iterations_and_stays(fixtures):
    f = fixtures['path2']
    graph = graph_of(f)
    lay = spring.SpringLayout(to_dev(f['pos0']), *(to_dev(a) for a in graph), 1.0 / math.sqrt(2), 50, 1e-4)
    want32, ran32 = sr.fr_model(sr.dense(*graph, 2), f['pos0'], dtype=np.float32)
    seen = []
    for _ in range(50):
        lay.step()
        seen.append((lay.y[0].clone(), read_state(lay.state)))
    assert ran32 == 43 and lay.iterations_run == 43
    assert [s[1][2] for s in seen] == list(range(1, 44)) + [43] * 7 and [s[1][3] for s in seen] == [0] * 42 + [1] * 8
    assert all(torch.equal(y, seen[42][0]) and st == seen[42][1] for y, st in seen[43:])
    dev32 = np.abs(lay.y[0].cpu().numpy().astype(np.float64) - want32).max()
    print(f'path2: the kernels against the float32-arithmetic model over all 50 iterations: {dev32:.3e}')
    assert dev32 <= 1e-6                                              # measured 4.5e-8 (profiles/spring.md)
    assert np.abs(lay.y[0].cpu().numpy() - f['pos_50']).max() <= 1e-6
    from ampnet_amd import spring_layout
    res = spring_layout(to_dev(f['edge_index']), 2, pos=to_dev(f['pos0']), scale=None)
    assert res.iterations_run == 43 and torch.equal(res.pos, lay.y[0])


def test_a_start_with_other_strides_gives_the_bits_of_the_contiguous_one(fixtures):
    """pos as a transposed view (strides (1, N)): both position buffers are dense row-major all the same, so after an odd
    number of iterations -- the result then lies in the second buffer -- and after an even one the run equals the run
    from the contiguous copy bit for bit."""
    from ampnet_amd import spring_layout
    for name, dim in (('sbm64', 2), ('grid8', 3)):
        f = fixtures[name]
        N, ei = f['N'], to_dev(f['edge_index'])
        y0 = np.random.default_rng(dim).random((N, dim), dtype=np.float32)
        dense, view = to_dev(y0), to_dev(np.ascontiguousarray(y0.T)).t()
        assert not view.is_contiguous() and view.stride() == (1, N) and torch.equal(view, dense)
        for n in (1, 2, 5):
            for scale in (None, 1.0):
                a = spring_layout(ei, N, pos=dense, dim=dim, iterations=n, scale=scale)
                b = spring_layout(ei, N, pos=view, dim=dim, iterations=n, scale=scale)
                assert torch.equal(a.pos.contiguous().view(torch.int32), b.pos.contiguous().view(torch.int32)), (name, n, scale)
                assert not torch.equal(a.pos, dense)
        graph = tuple(to_dev(g) for g in graph_of(f))
        lays = [spring.SpringLayout(start, *graph, 1.0 / math.sqrt(N), 50) for start in (dense, view)]
        for step in range(3):
            for lay in lays:
                lay.step()
            assert all(lay.y[0].is_contiguous() and lay.y[1].is_contiguous() for lay in lays)
            assert torch.equal(lays[0].y[0], lays[1].y[0]) and torch.equal(lays[0].state, lays[1].state), (name, step)
        assert torch.equal(view, dense)                               # the start itself is never written


# ------------------------------------------------------------------------------------------ networkx's recorded values
@pytest.mark.parametrize('name', sr.CASES)
def test_parity_with_networkx_at_1_and_5_iterations(fixtures, name):
    from ampnet_amd import spring_layout
    f = fixtures[name]
    A = sr.dense(*graph_of(f), f['N'])
    ei, pos0 = to_dev(f['edge_index']), to_dev(f['pos0'])
    bad = []
    for n in (1, 5):
        want = f[f'pos_{n}'].astype(np.float64)
        own = float(np.abs(sr.fr_model(A, f['pos0'], iterations=n, dtype=np.float32)[0].astype(np.float64) - want).max())
        bar = max(4.0 * own, 1e-6)
        res = spring_layout(ei, f['N'], pos=pos0, iterations=n, scale=None, symmetric=f['symmetric'])
        dev_ = float(np.abs(res.pos.cpu().numpy().astype(np.float64) - want).max())
        print(f'{name} n={n}: float32 model deviates {own:.3e}, bar {bar:.3e}, kernels deviate {dev_:.3e}')
        if not dev_ <= bar:
            bad.append(f'{name} n={n}: {dev_:.3e} against the bar {bar:.3e}')
        if res.iterations_run != n or res.k != 1.0 / math.sqrt(f['N']):
            bad.append(f'{name} n={n}: iterations_run {res.iterations_run}, k {res.k}')
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize('name', ('sbm64', 'grid8', 'cycle33', 'sbm512', 'xor_digraph_40'))
def test_default_runs(fixtures, name):
    from ampnet_amd import spring_layout
    f = fixtures[name]
    N, ei = f['N'], to_dev(f['edge_index'])
    kw = dict(symmetric=f['symmetric'])
    res = spring_layout(ei, N, seed=0, **kw)
    pos = res.pos.cpu().numpy()
    assert res.pos.dtype == torch.float32 and pos.shape == (N, 2) and np.isfinite(pos).all()
    assert abs(float(np.abs(pos).max()) - 1.0) <= 2 * np.spacing(np.float32(1.0))
    assert np.abs(pos.astype(np.float64).mean(0)).max() <= 1e-6
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(res.graph, (f['a_indptr'], f['a_indices'], f['a_val'])))
    start = sr.edge_ratio(spring.uniform_start(N, 2, 0, dev()).cpu().numpy(), f['edge_index'])
    end = sr.edge_ratio(pos, f['edge_index'])
    print(f'{name}: edge / non-edge distance {start:.3f} -> {end:.3f} ({end / start:.3f} x), {res.iterations_run} iterations')
    assert end < 0.6 * start
    again, other = spring_layout(ei, N, seed=0, **kw), spring_layout(ei, N, seed=1, **kw)
    assert torch.equal(again.pos, res.pos) and not torch.equal(other.pos, res.pos) and torch.isfinite(other.pos).all()
    moved = spring_layout(ei, N, seed=0, scale=2.5, center=(1.0, -3.0), **kw).pos.cpu().numpy().astype(np.float64)
    assert abs(np.abs(moved - [1.0, -3.0]).max() - 2.5) <= 2 * np.spacing(np.float32(4.0))      # ulps of the coordinates, up to 5.5
    assert np.abs(moved.mean(0) - [1.0, -3.0]).max() <= 1e-6
    raw = spring_layout(ei, N, seed=0, scale=None, **kw).pos
    assert np.abs(sr.rescale_model(raw.cpu().numpy()) - pos).max() <= 2 * np.spacing(np.float32(1.0))      # the finish is networkx's


def test_directed_differs_from_symmetric_and_three_dimensions(fixtures):
    from ampnet_amd import spring_layout
    f = fixtures['xor_digraph_40']
    ei = to_dev(f['edge_index'])
    directed, both = spring_layout(ei, 40, symmetric=False), spring_layout(ei, 40, symmetric=True)
    assert not torch.equal(directed.pos, both.pos) and both.graph[1].numel() > directed.graph[1].numel()
    ones = spring_layout(ei, 40, symmetric=False, weight=torch.ones(ei.size(1), device=dev()))
    assert torch.equal(ones.pos, directed.pos)                        # weight 1 is no weight
    heavy = spring_layout(ei, 40, symmetric=False, weight=torch.full((ei.size(1),), 3.0, device=dev()))
    assert not torch.equal(heavy.pos, directed.pos) and torch.isfinite(heavy.pos).all()
    f = fixtures['sbm64']
    cube = spring_layout(to_dev(f['edge_index']), 64, dim=3, center=(0.0, 1.0, 2.0))
    p = cube.pos.cpu().numpy().astype(np.float64)
    assert p.shape == (64, 3) and np.isfinite(p).all() and np.abs(p.mean(0) - [0.0, 1.0, 2.0]).max() <= 1e-6
    assert torch.equal(cube.pos, spring_layout(to_dev(f['edge_index']), 64, dim=3, center=(0.0, 1.0, 2.0)).pos)
    assert p[:, 2].std() > 0.05                                        # the third coordinate is laid out too


def test_trivial_graphs_fixed_nodes_and_partial_positions(fixtures):
    from ampnet_amd import spring_layout
    none = torch.zeros(2, 0, dtype=torch.int64, device=dev())
    empty = spring_layout(none, 0)
    assert tuple(empty.pos.shape) == (0, 2) and empty.iterations_run == 0
    one = spring_layout(none, 1, center=(2.0, -1.0))
    assert one.pos.tolist() == [[2.0, -1.0]] and spring_layout(none, 1, dim=3).pos.tolist() == [[0.0, 0.0, 0.0]]
    edgeless = spring_layout(none, 50)                                 # repulsion only
    assert torch.isfinite(edgeless.pos).all() and edgeless.graph[1].numel() == 0
    f = fixtures['grid8']
    ei, N = to_dev(f['edge_index']), 64
    pos = torch.full((N, 2), NAN, device=dev())
    pos[0], pos[7], pos[63] = torch.tensor([0.0, 0.0]), torch.tensor([4.0, 0.5]), torch.tensor([3.0, 4.0])
    fixed = torch.tensor([0, 63], device=dev())
    start = spring_layout(ei, N, pos=pos, fixed=fixed, iterations=0, seed=3, center=(0.5, 0.25))
    rand = (spring.uniform_start(N, 2, 3, dev()).double() * 4.0 + torch.tensor([0.5, 0.25], dtype=torch.float64, device=dev())).float()
    given = ~torch.isnan(pos).any(1)
    assert torch.equal(start.pos[given], pos[given]) and torch.equal(start.pos[~given], rand[~given])
    assert start.k == 4.0 / math.sqrt(N) and start.iterations_run == 0
    res = spring_layout(ei, N, pos=pos, fixed=fixed, seed=3)
    mask = torch.zeros(N, dtype=torch.bool, device=dev())
    mask[fixed] = True
    same = spring_layout(ei, N, pos=pos, fixed=mask, seed=3)
    assert torch.equal(res.pos[fixed], pos[fixed]) and not torch.equal(res.pos[7], pos[7]) and torch.isfinite(res.pos).all()
    assert torch.equal(res.pos, same.pos) and res.k == 4.0 / math.sqrt(N)
    want, _ = sr.layout_model(start.pos.cpu().numpy(), *graph_of(f), k=res.k, fixed=mask.cpu().numpy())
    assert np.array_equal(want[[0, 63]], res.pos.cpu().numpy()[[0, 63]])
    with pytest.raises(ValueError, match='fixed without positions'):
        spring_layout(ei, N, pos=pos, fixed=torch.tensor([1], device=dev()))


# ---------------------------------------------------------------------------------------------------------- validation
def test_rejected_arguments_raise_before_any_launch(monkeypatch):
    from ampnet_amd import spring_layout
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]], device=dev())
    pos = torch.zeros(5, 2, device=dev())

    def launched(*a, **k):
        raise AssertionError('a stage ran before the arguments were checked')

    for name in ('adjacency', 'uniform_start', 'SpringLayout', 'rescale'):
        monkeypatch.setattr(spring, name, launched)
    w = torch.ones(3, device=dev())
    for kw in (dict(dim=1), dict(dim=4), dict(k=0.0), dict(k=-2.0), dict(k='x'), dict(iterations=-1), dict(iterations=2.5), dict(threshold='x'),
               dict(scale='big'), dict(center=(0.0,)), dict(center=(0.0, 0.0, 0.0)), dict(seed=1.5), dict(symmetric=1), dict(weight=w),
               dict(weight=w[:2], symmetric=False), dict(weight=w.cpu(), symmetric=False), dict(weight=w.long(), symmetric=False),
               dict(pos=pos[:, :1]), dict(pos=pos[:4]), dict(pos=pos.double()), dict(pos=pos.cpu()), dict(fixed=torch.tensor([0], device=dev())),
               dict(pos=pos, fixed=[0]), dict(pos=pos, fixed=torch.tensor([0])), dict(pos=pos, fixed=torch.zeros(4, dtype=torch.bool, device=dev())),
               dict(pos=pos, fixed=torch.tensor([9], device=dev())), dict(pos=torch.full((5, 2), NAN, device=dev()), fixed=torch.tensor([1], device=dev())),
               dict(pos=torch.full((5, 2), -float('inf'), device=dev())), dict(pos=torch.full((5, 2), float('inf'), device=dev()))):
        with pytest.raises(ValueError):
            spring_layout(ei, 5, **kw)
    for bad_ei, n in ((ei.cpu(), 5), (ei.int(), 5), (ei[0], 5), (ei.t(), 5), (ei, -1), (ei, 2.0), (ei, (1 << 24) + 1), (ei, 0), (ei, 3),
                      (torch.tensor([[0, -1], [1, 2]], device=dev()), 5)):
        with pytest.raises(ValueError):
            spring_layout(bad_ei, n)
