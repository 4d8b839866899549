"""The specification of ampnet_amd.spring in numpy (include/ampconv.h, "Spring layout"): networkx 3.4.2's
Fruchterman-Reingold loop restated statement by statement (fr_model: in fp64 it reproduces nx.spring_layout bit for bit
on the dense-path fixtures), the same loop in float32 arithmetic (the reference's own rounding sensitivity, from which
the parity bars come), the adjacency, the start stream, one iteration with the two sums kept apart and their absolute
term sums (from which the error bounds come), and the quality figure of the end-to-end tests.

The fixtures under tests/golden/spring are written by tools/make_golden_spring.py with networkx installed; nothing here
imports networkx."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'spring')
CASES = ('sbm64', 'grid8', 'cycle33', 'path2', 'sbm512', 'xor_digraph_40')
DENSE_CASES = tuple(c for c in CASES if c != 'sbm512')               # N < 500: networkx's dense path, fp64 positions
ITERATIONS = (1, 5, 50)
RUN, PART = 256, 1024                                                # AMPCONV_SPRING_RUN, AMPCONV_SPRING_PART
MIN_DIST, MIN_DIST2 = float(np.float32(0.01)), float(np.float32(1e-4))      # the kernels' float32 constants, widened
U = 2.0 ** -24
MASK = (1 << 64) - 1


def load(name):
    with np.load(os.path.join(GOLDEN_DIR, name + '.npz'), allow_pickle=False) as z:
        f = {k: z[k] for k in z.files}
    f['edge_index'] = f['edge_index'].astype(np.int64)
    f['N'], f['symmetric'] = int(f['num_nodes']), bool(f['symmetric'])
    return f


# --------------------------------------------------------------------------------------------------------- the stream
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def draw(seed, a, b):
    """The library's counter-based stream on Python integers."""
    return splitmix64((seed & MASK) ^ splitmix64((a * 0x100000001B3 + b) & MASK))


def uniform_start_model(N, dim, seed):
    """float32 [N, dim]: y[i, c] = (draw(seed, i, c) >> 40) 2^-24."""
    return np.array([[(draw(seed, i, c) >> 40) * 2.0 ** -24 for c in range(dim)] for i in range(N)], np.float32).reshape(N, dim)


# ------------------------------------------------------------------------------------------------------- the adjacency
def adjacency_model(edge_index, N, weight=None, symmetric=True):
    """(indptr, indices, val float32): the CSR of the matrix networkx lays out (ampnet_amd.spring.adjacency)."""
    r, c = np.asarray(edge_index[0], np.int64), np.asarray(edge_index[1], np.int64)
    if weight is None:
        key = r * N + c
        if symmetric:
            key = np.concatenate((key, c * N + r))
        key = np.unique(key)
        val = np.ones(key.size, np.float32)
    else:
        assert not symmetric
        order = np.argsort(r * N + c, kind='stable')
        key, inverse = np.unique((r * N + c)[order], return_inverse=True)
        total = np.zeros(key.size, np.float64)
        np.add.at(total, inverse, np.asarray(weight, np.float64)[order])          # in the order of the edge list
        val = total.astype(np.float32)
    indptr = np.searchsorted(key, np.arange(N + 1, dtype=np.int64) * N)
    return indptr.astype(np.int64), (key % max(N, 1)).astype(np.int64), val


def dense(indptr, indices, val, N, dtype=np.float64):
    A = np.zeros((N, N), dtype)
    A[np.repeat(np.arange(N), np.diff(indptr)), indices] = val
    return A


# ----------------------------------------------------------------------------------------------- networkx's loop, whole
def fr_model(A, pos0, k=None, fixed=None, iterations=50, threshold=1e-4, dtype=np.float64):
    """(pos, iterations run): networkx's _fruchterman_reingold on the dense matrix A from the start pos0, statement by
    statement.  dtype=float64 is networkx on its dense path (N < 500); dtype=float32 is the same loop with positions,
    matrix and every array operation in float32 -- the float32-arithmetic model that the parity bars are taken from."""
    A = np.asarray(A, dtype)
    pos = np.array(pos0, dtype)
    nnodes = A.shape[0]
    if k is None:
        k = np.sqrt(1.0 / nnodes)
    k = dtype(k) if dtype is np.float32 else k
    # every scalar is pinned to dtype, so the float32 model's bits do not depend on numpy's scalar promotion rules
    t = dtype(max(max(pos.T[0]) - min(pos.T[0]), max(pos.T[1]) - min(pos.T[1]))) * dtype(0.1)
    dt = t / dtype(iterations + 1)
    ran = 0
    for _ in range(iterations):
        delta = pos[:, np.newaxis, :] - pos[np.newaxis, :, :]
        distance = np.linalg.norm(delta, axis=-1)
        np.clip(distance, dtype(0.01), None, out=distance)
        displacement = np.einsum('ijk,ij->ik', delta, (k * k / distance ** 2 - A * distance / k))
        length = np.linalg.norm(displacement, axis=-1)
        length = np.where(length < dtype(0.01), dtype(0.1), length)
        delta_pos = np.einsum('ij,i->ij', displacement, t / length)
        if fixed is not None:
            delta_pos[fixed] = 0.0
        pos += delta_pos.astype(dtype)
        t = dtype(t - dt)
        ran += 1
        if (np.linalg.norm(delta_pos) / nnodes) < threshold:
            break
    return pos, ran


def rescale_model(pos, scale=1.0, center=None):
    """networkx's rescale_layout(pos, scale) + center."""
    pos = np.array(pos, np.float64)
    pos -= pos.mean(axis=0)
    lim = np.abs(pos).max()
    if lim > 0:
        pos *= scale / lim
    return pos + (0.0 if center is None else np.asarray(center, np.float64))


# ------------------------------------------------------------------------------------------- one iteration, sum by sum
def repulsion_model(y, rows=256):
    """(rep, abs) float64 [N, dim]: rep_i = sum_j (y_i - y_j) / max(|y_i - y_j|^2, 1e-4f) over all j on the float32
    positions y, exactly as the header states it, and the sums of the terms' magnitudes (the error bounds' scale)."""
    y = np.asarray(y, np.float32).astype(np.float64)
    rep, mag = np.zeros_like(y), np.zeros_like(y)
    for r in range(0, y.shape[0], rows):
        d = y[r:r + rows, None, :] - y[None, :, :]
        q = 1.0 / np.maximum((d * d).sum(-1), MIN_DIST2)
        term = d * q[:, :, None]
        rep[r:r + rows], mag[r:r + rows] = term.sum(1), np.abs(term).sum(1)
    return rep, mag


def repulsion_bound(mag):
    """|rep - exact| per coordinate: a run of RUN float32 additions, 16 for the pair's own roundings (header)."""
    return (RUN + 16) * U * mag


def attraction_model(y, indptr, indices, val=None):
    """(att, abs) float64 [N, dim]: att_i = sum over row i of w max(sqrt(|y_i - y_j|^2), 0.01f) (y_i - y_j)."""
    y = np.asarray(y, np.float32).astype(np.float64)
    N = y.shape[0]
    rows = np.repeat(np.arange(N), np.diff(indptr))
    d = y[rows] - y[indices]
    w = np.maximum(np.sqrt((d * d).sum(-1)), MIN_DIST) * (1.0 if val is None else np.asarray(val, np.float64))
    term = d * w[:, None]
    att, mag = np.zeros_like(y), np.zeros_like(y)
    np.add.at(att, rows, term)
    np.add.at(mag, rows, np.abs(term))
    return att, mag


def attraction_bound(mag):
    """|att - exact| per coordinate: a butterfly of 6 float32 additions over the lanes, the entry's own roundings
    (difference, d^2, sqrt, the weight's product, the FMA: under 10) -- 16 in all; the groups are added in fp64."""
    return 16 * U * mag


def iteration_model(y, indptr, indices, val, k, t, fixed=None, rep=None):
    """One iteration of the header from the float32 positions y, in fp64: a dict with rep, att, their magnitude sums,
    disp, len (after the floor), floored, delta (float32), y_out (float32) and err = sqrt(sum delta^2) / N.  rep: the
    repulsion to take as given (its error is then none of this iteration's: rmag = 0)."""
    y32 = np.asarray(y, np.float32)
    rep, rmag = repulsion_model(y32) if rep is None else (np.asarray(rep, np.float64), np.zeros(y32.shape))
    att, amag = attraction_model(y32, indptr, indices, val)
    disp = k * k * rep - att / k
    raw = np.sqrt((disp * disp).sum(-1))
    floored = raw < 0.01
    length = np.where(floored, 0.1, raw)
    delta = (disp * (t / length)[:, None]).astype(np.float32)
    if fixed is not None:
        delta[np.asarray(fixed, bool)] = 0
    y_out = y32 + delta
    err = np.sqrt((delta.astype(np.float64) ** 2).sum()) / y32.shape[0]
    return dict(rep=rep, att=att, rmag=rmag, amag=amag, disp=disp, raw=raw, len=length, floored=floored, delta=delta, y_out=y_out,
                err=err)


def iteration_bound(info, k, t):
    """(bound float64 [N, dim], sure bool [N]): what |y_out - model| may be per coordinate, from the two sums' bounds.
    e = k^2 E_rep + E_att / k bounds the displacement's error per coordinate, |e| its norm.  Where the length is not
    floored delta = t disp / |disp| and normalising a vector moves by at most 2 |e| / |disp|, so |d delta| <= 2 t |e| / len;
    where it is floored delta = disp t / 0.1 is linear and |d delta| <= t |e| / 0.1.  Then two float32 roundings (delta,
    y_in + delta) and fp64 noise.  sure: the row's choice between the two cases cannot differ from the model's (its raw
    length is further than |e| from 0.01); the other rows are not compared."""
    e = k * k * repulsion_bound(info['rmag']) + attraction_bound(info['amag']) / k
    en = np.sqrt((e * e).sum(-1))
    sure = np.abs(info['raw'] - 0.01) > en
    move = np.where(info['floored'], t * en / 0.1, 2.0 * t * en / info['len'])
    y_out = np.abs(info['y_out'].astype(np.float64))
    # both sides round delta and the sum once each: half an ulp, at most 2^-24 relative, twice
    bound = move[:, None] + 2 * U * np.abs(info['delta'].astype(np.float64)) + 2 * U * (y_out + move[:, None]) + 1e-12
    return bound, sure


def temperature_model(y0, iterations):
    """(t0, dt) in fp64: 0.1 x the larger extent of the first two columns of the float32 start, and t0 / (iterations + 1)."""
    y = np.asarray(y0, np.float32).astype(np.float64)
    t0 = max(y[:, 0].max() - y[:, 0].min(), y[:, 1].max() - y[:, 1].min()) * 0.1
    return t0, t0 / (iterations + 1)


def layout_model(y0, indptr, indices, val, k=None, fixed=None, iterations=50, threshold=1e-4):
    """(y float32, iterations run): the header's iteration free-running from y0 -- float32 positions, the sums, the
    displacement and the temperature in fp64 -- with the stopping rule."""
    y = np.asarray(y0, np.float32)
    k = 1.0 / np.sqrt(y.shape[0]) if k is None else k
    t, dt = temperature_model(y, iterations)
    ran = 0
    for _ in range(iterations):
        info = iteration_model(y, indptr, indices, val, k, t, fixed)
        y = info['y_out']
        t -= dt
        ran += 1
        if info['err'] < threshold:
            break
    return y, ran


# ------------------------------------------------------------------------------------------------------------- quality
def edge_ratio(pos, edge_index):
    """The mean length of an edge (self-loops left out) over the mean distance of the pairs that are no edge."""
    pos = np.asarray(pos, np.float64)
    N = pos.shape[0]
    D = np.sqrt(((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1))
    E = np.zeros((N, N), bool)
    E[edge_index[0], edge_index[1]] = True
    E |= E.T
    np.fill_diagonal(E, False)
    other = ~E
    np.fill_diagonal(other, False)
    return D[E].mean() / D[other].mean()
