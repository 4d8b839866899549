"""numpy fp64 model of the GCN baseline (include/ampconv.h, "GCN baseline"): gcn_norm, the layer forward and backward
straight from the edge list (no CSR), the reference's embedded input in its MATERIALISED form (src/ampnet/module/
gcn_classifier.py:91-109) with gradients to the weight and the table, and the whole model with the node_norm-weighted
NLL.  PyG is not installed: this restatement of PyG 2.0-2.1's gcn_norm / GCNConv is what the kernels are held to."""
import numpy as np


def normalised_edges(edge_index, num_nodes, improved=False, add_self_loops=True):
    """(src, dst, w) after add_remaining_self_loops: every loop of the input dropped, one loop of weight fill per node;
    without add_self_loops the edges as they are, weight 1."""
    src, dst = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    w = np.ones(src.shape[0], dtype=np.float64)
    if add_self_loops:
        keep = src != dst
        loops = np.arange(num_nodes, dtype=np.int64)
        src, dst = np.concatenate([src[keep], loops]), np.concatenate([dst[keep], loops])
        w = np.concatenate([w[keep], np.full(num_nodes, 2.0 if improved else 1.0)])
    return src, dst, w


def gcn_norm(edge_index, num_nodes, improved=False, add_self_loops=True):
    """(src, dst, norm, dinv): norm[e] = dinv[src] w dinv[dst], dinv = deg^-1/2 with 0 for deg == 0."""
    src, dst, w = normalised_edges(edge_index, num_nodes, improved, add_self_loops)
    deg = np.zeros(num_nodes, dtype=np.float64)
    np.add.at(deg, dst, w)
    dinv = np.zeros(num_nodes, dtype=np.float64)
    dinv[deg > 0] = deg[deg > 0] ** -0.5
    return src, dst, dinv[src] * w * dinv[dst], dinv


def aggregate(h, edge_index, bias=None, improved=False, add_self_loops=True):
    """out[d] = sum_{e: dst(e) = d} norm[e] h[src(e)] + bias."""
    h = np.asarray(h, dtype=np.float64)
    src, dst, norm, _ = gcn_norm(edge_index, h.shape[0], improved, add_self_loops)
    out = np.zeros_like(h)
    np.add.at(out, dst, norm[:, None] * h[src])
    return out if bias is None else out + np.asarray(bias, dtype=np.float64)


def aggregate_backward(g, edge_index, improved=False, add_self_loops=True):
    """(dh, dbias) of aggregate for the upstream gradient g: the transposed operator and the column sum."""
    g = np.asarray(g, dtype=np.float64)
    src, dst, norm, _ = gcn_norm(edge_index, g.shape[0], improved, add_self_loops)
    dh = np.zeros_like(g)
    np.add.at(dh, src, norm[:, None] * g[dst])
    return dh, g.sum(axis=0)


def colsum(g):
    """out[c] = sum_n g[n, c]."""
    return np.asarray(g, dtype=np.float64).sum(axis=0)


def dense_operator(edge_index, num_nodes, improved=False, add_self_loops=True):
    """A_hat [N, N] with out = A_hat h."""
    src, dst, norm, _ = gcn_norm(edge_index, num_nodes, improved, add_self_loops)
    A = np.zeros((num_nodes, num_nodes), dtype=np.float64)
    np.add.at(A, (dst, src), norm)
    return A


def zscore(x):
    """sklearn's StandardScaler().fit_transform: population variance, constant columns scaled by 1."""
    x = np.asarray(x, dtype=np.float64)
    mean, var = x.mean(axis=0), x.var(axis=0)
    scale = np.where(var > 1e-12 * np.maximum(1.0, mean * mean), np.sqrt(var), 1.0)
    return (x - mean) / scale


def embedded_input(z, table):
    """The reference's [N, F (De + 1)] input: per node cat(table, z[n][:, None]) reshaped to one row."""
    N, F = z.shape
    table = np.asarray(table, dtype=np.float64)
    tokens = np.empty((N, F, table.shape[1] + 1), dtype=np.float64)      # the per-node cat, written in place
    tokens[:, :, :-1] = table
    tokens[:, :, -1] = z
    return tokens.reshape(N, F * (table.shape[1] + 1))


def first_layer_input(x, table, mode, stats=None):
    """stats: (mean, inv_std) to use as they are, z = (x - mean) inv_std, in place of zscore's own (a test of the input
    kernels alone hands both sides the same fp32 statistics)."""
    x = np.asarray(x, dtype=np.float64)
    if mode == 'raw':
        z = x
    elif stats is None:
        z = zscore(x)
    else:
        z = (x - np.asarray(stats[0], dtype=np.float64)) * np.asarray(stats[1], dtype=np.float64)
    return embedded_input(z, table) if mode == 'embedded' else z


def input_linear(x, W, table, mode='embedded', stats=None):
    """h = X0 W^T on the materialised input X0."""
    return first_layer_input(x, table, mode, stats) @ np.asarray(W, dtype=np.float64).T


def input_linear_factored(x, W, table):
    """The same product without X0: sum_f z[n, f] W[j, f, De] + sum_f sum_k table[f, k] W[j, f, k]."""
    z, table = zscore(x), np.asarray(table, dtype=np.float64)
    F, De = table.shape
    W3 = np.asarray(W, dtype=np.float64).reshape(-1, F, De + 1)
    return z @ W3[:, :, De].T + np.einsum('fk,jfk->j', table, W3[:, :, :De])


def input_linear_backward(x, W, table, g, mode='embedded', stats=None):
    """(dW, dtable) through the materialised input (dtable None outside the embedded mode)."""
    X0, g = first_layer_input(x, table, mode, stats), np.asarray(g, dtype=np.float64)
    dW = g.T @ X0
    if mode != 'embedded':
        return dW, None
    F, De = np.asarray(table).shape
    dX0 = (g @ np.asarray(W, dtype=np.float64)).reshape(g.shape[0], F, De + 1)
    return dW, dX0[:, :, :De].sum(axis=0)


def log_softmax(a):
    a = a - a.max(axis=1, keepdims=True)
    return a - np.log(np.exp(a).sum(axis=1, keepdims=True))


def model(x, edge_index, params, mode='embedded', y=None, node_norm=None, mask=None, improved=False,
          add_self_loops=True):
    """Eval-mode forward of the 2-layer GCN (no dropout) and, with labels, the loss (nll * node_norm)[mask].sum() and
    its gradients.  params: the state dict as arrays.  Returns {'logp', 'hidden', 'loss', 'grads'}."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    table = P['feature_embedding_table.weight']
    W1, b1, W2, b2 = P['conv1.lin.weight'], P['conv1.bias'], P['conv2.lin.weight'], P['conv2.bias']
    N = np.asarray(x).shape[0]
    kw = dict(improved=improved, add_self_loops=add_self_loops)
    X0 = first_layer_input(x, table, mode)
    a1 = aggregate(X0 @ W1.T, edge_index, b1, **kw)
    r = np.maximum(a1, 0.0)
    a2 = aggregate(r @ W2.T, edge_index, b2, **kw)
    logp = log_softmax(a2)
    out = {'logp': logp, 'hidden': r, 'aggregated': aggregate(r, edge_index, None, **kw)}
    if y is None:
        return out
    y = np.asarray(y, dtype=np.int64)
    wgt = np.ones(N) if node_norm is None else np.asarray(node_norm, dtype=np.float64)
    if mask is not None:
        wgt = wgt * np.asarray(mask, dtype=np.float64)
    out['loss'] = float(-(wgt * logp[np.arange(N), y]).sum())
    dz = np.exp(logp) * wgt[:, None]
    dz[np.arange(N), y] -= wgt
    dh2, db2 = aggregate_backward(dz, edge_index, **kw)
    dW2 = dh2.T @ r
    da1 = (dh2 @ W2) * (a1 > 0)
    dh1, db1 = aggregate_backward(da1, edge_index, **kw)
    dW1 = dh1.T @ X0
    grads = {'conv1.lin.weight': dW1, 'conv1.bias': db1, 'conv2.lin.weight': dW2, 'conv2.bias': db2}
    if mode == 'embedded':
        F, De = table.shape
        grads['feature_embedding_table.weight'] = (dh1 @ W1).reshape(N, F, De + 1)[:, :, :De].sum(axis=0)
    else:
        grads['feature_embedding_table.weight'] = None          # unused by the forward: no gradient
    out['grads'] = grads
    return out
