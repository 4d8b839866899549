#!/usr/bin/env python3
"""Bitwise fingerprint of every projection / edge path a layer call can take, through the public API only, so that the
same file runs on two checkouts and their outputs can be compared (profiles/conv_projection_refactor.md):

    python tools/ab_conv_paths.py OUT.json            # in each checkout, one fresh process per run
    python tools/ab_conv_paths.py --compare A.json B.json
    python tools/ab_conv_paths.py --launches A_kernel_trace.csv B_kernel_trace.csv     # rocprofv3 --kernel-trace of a run

Per case: forward + backward of one seeded layer on one seeded graph -- 64 nodes of which 24 have no edge at all, 400
edges, one destination with 150 in-edges and one source with 150 out-edges (a long-segment plan at the small-graph
chunk of 64) -- and the SHA-256 of the raw bytes of y, the input gradient(s) and the four parameter gradients.  Every
hashed tensor must be finite and non-zero; each case asserts the plan it is meant to take where public attributes
show it."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

N, ISOLATED, E, HUB = 64, 24, 400, 150


def graph(dev):
    import torch
    g = torch.Generator().manual_seed(11)
    live = N - ISOLATED                                                 # nodes 0 .. live-1 carry every edge
    src = torch.randint(0, live, (E,), generator=g)
    dst = torch.randint(0, live, (E,), generator=g)
    dst[dst == 3] = 4
    src[src == 7] = 8
    dst[:HUB] = 3                                                       # hub destination
    src[HUB:2 * HUB] = 7                                                # hub source
    ei = torch.stack([src, dst])
    assert int((ei[1] == 3).sum()) == HUB and int((ei[0] == 7).sum()) == HUB and int(ei.max()) < live
    return ei.to(dev)


def digest(name, t):
    import torch
    assert t is not None, name
    assert bool(torch.isfinite(t.float()).all()) and bool((t != 0).any()), f'{name}: not finite or all zero'
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(L, D, H, mode='forward', dtype='f32', gemm='native', scaled=False, softmax=True, wide_dy=False,
             expect=None):
    import torch
    from ampnet_amd import AMPConv, _lib
    from ampnet_amd.conv import functional as F_
    from ampnet_amd.graph import graph_cache
    from ampnet_amd.partitioned import NodePartition, PartitionedAMPConv
    dev = torch.device('cuda:0')
    F_.PROJ_SCALED_MIN_ELEMENTS = 0 if scaled else 1 << 62
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    torch.manual_seed(5)
    layer = AMPConv(D, H, softmax=softmax).to(dev)
    with torch.no_grad():
        layer.multi_head_attention.in_proj_bias.normal_(0, 0.1)
        layer.multi_head_attention.out_proj.bias.normal_(0, 0.1)
    layer = layer.to(td)
    layer.gemm_precision = gemm
    ei = graph(dev)
    g = torch.Generator().manual_seed(L * 1000 + D + H)
    rows = E if mode == 'message' else N
    xs = [torch.randn(rows, L * D, generator=g).to(dev, td).requires_grad_(True)
          for _ in range(2 if mode == 'message' else 1)]
    dy = torch.randn(rows, L * D, generator=g)
    if wide_dy:
        dy[2] *= 2.0 ** 20          # one row far above the rest: the backward pass leaves the scaled kernels
    dy = dy.to(dev, td)
    if mode == 'forward':
        y = layer(xs[0], ei)
        if expect == 'planes':
            assert layer._attn_plane_bounds is not None, 'expected the plane-format plan'
        elif dtype == 'f32':
            assert layer._attn_plane_bounds is None, 'did not expect the plane-format plan'
        if expect == 'lists':
            assert graph_cache.get(ei, N).active_nodes() is not None, 'expected node lists on this graph'
            assert F_.NODE_LISTS and F_.proj_native(gemm, td, D) and 16 <= L <= 128
        csr = graph_cache.get(ei, N)
        assert csr.hub_dst_chunks > 0 and csr.hub_src_chunks > 0, 'expected long-segment plans on both sides'
    elif mode == 'message':
        y = layer.message(xs[0], xs[1])
    else:
        part = NodePartition(N)
        assert part.world == 1
        wrapped = PartitionedAMPConv(layer, part)
        y = wrapped(part.local_rows(xs[0]), wrapped.prepare(ei))
    if expect in ('native', 'planes', 'lists', 'scaled', 'views'):
        assert F_.proj_native(gemm, td, D)
    if expect == 'gemm':
        assert not F_.proj_native(gemm, td, D)
    if expect == 'views':
        assert _lib.load().ampconv_scaled_supported(L, D, H) and D % 128 != 0
    (y.float() * dy.float()).sum().backward()
    torch.cuda.synchronize()
    m = layer.multi_head_attention
    out = {'y': digest('y', y)}
    for i, x in enumerate(xs):
        out[f'dx{i}'] = digest(f'dx{i}', x.grad)
    for name, p in (('gw', m.in_proj_weight), ('gb', m.in_proj_bias), ('gow', m.out_proj.weight),
                    ('gob', m.out_proj.bias)):
        out[name] = digest(name, p.grad)
    return out


CASES = {
    # name: run_case arguments
    'planes_dh32': dict(L=20, D=128, H=4, scaled=True, expect='planes'),
    'planes_dh16': dict(L=20, D=128, H=8, scaled=True, expect='planes'),
    'views': dict(L=40, D=100, H=2, scaled=True, expect='views'),
    'scaled_plain': dict(L=4, D=128, H=8, scaled=True, expect='scaled'),
    'plain': dict(L=13, D=64, H=2, expect='native'),
    'ragged_D6': dict(L=3, D=6, H=2, expect='gemm'),
    'planes_dh32_fp32gemm': dict(L=20, D=128, H=4, scaled=True, gemm='fp32', expect='gemm'),
    'planes_dh32_wide_dy': dict(L=20, D=128, H=4, scaled=True, wide_dy=True, expect='planes'),
    'bf16_lists': dict(L=20, D=128, H=4, dtype='bf16', expect='lists'),
    'message_native': dict(L=20, D=128, H=4, mode='message', expect='native'),
    'message_scaled': dict(L=20, D=128, H=4, mode='message', scaled=True, expect='scaled'),
    'message_fp32gemm': dict(L=20, D=128, H=4, mode='message', gemm='fp32', expect='gemm'),
    'linear_forward': dict(L=20, D=128, H=4, softmax=False),
    'linear_message': dict(L=20, D=128, H=4, softmax=False, mode='message'),
    'partitioned_native': dict(L=20, D=128, H=4, mode='partitioned', expect='native'),
    'partitioned_fp32gemm': dict(L=20, D=128, H=4, mode='partitioned', gemm='fp32', expect='gemm'),
}


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    bad = 0
    for case in a:
        row = ['equal' if a[case][k] == b[case].get(k) else 'DIFFERENT' for k in a[case]]
        bad += row.count('DIFFERENT')
        print('| `' + case + '` | ' + ' | '.join(f'{k} {v}' for k, v in zip(a[case], row)) + ' |')
    print(f'{sum(len(v) for v in a.values())} tensors, {bad} different')
    return 1 if bad else 0


MARKER = 'erfinv'       # one launch of a kernel nothing else here runs, in front of every case: splits a kernel trace


def launches(path):
    """{case: ordered kernel names} of a rocprofv3 kernel-trace CSV of one run of this file."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    names, out = iter(CASES), {}
    for r in rows:
        if MARKER in r['Kernel_Name']:
            cur = out.setdefault(next(names), [])
        elif out:
            cur.append(r['Kernel_Name'])
    assert len(out) == len(CASES), (len(out), len(CASES))
    return out


def compare_launches(a_path, b_path):
    import difflib
    a, b = launches(a_path), launches(b_path)
    for case in CASES:
        diff = [d for d in difflib.ndiff(a[case], b[case]) if d[0] in '+-']
        print(f'{case}: {len(a[case])} / {len(b[case])} launches, ' + ('identical' if not diff else 'DIFFERENT'))
        for d in diff:
            print('   ', d[:160])
    return 0


def main():
    if sys.argv[1] == '--compare':
        return compare(sys.argv[2], sys.argv[3])
    if sys.argv[1] == '--launches':
        return compare_launches(sys.argv[2], sys.argv[3])
    import torch
    out = {}
    for name in CASES:
        torch.cuda.synchronize()
        torch.full((1,), 0.5, device='cuda:0').erfinv_()
        out[name] = run_case(**CASES[name])
        print(name, 'ok', flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
