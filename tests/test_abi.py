"""CPU checks of the boundary: libampconv.so loads, exports every symbol that
include/ampconv.h declares (no compute calls here), and the host-side class
mirrors the reference's API and error behaviour."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'ampconv.h')


def _declared():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(ampconv_[a-z_0-9]+)\s*\(', src)))


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    return os.path.join(ROOT, 'ampnet_amd', 'libampconv.so')


def test_header_declares_the_path():
    names = _declared()
    for n in ('ampconv_csr_build', 'ampconv_fwd_edge', 'ampconv_bwd_edge_dst', 'ampconv_bwd_edge_src',
              'ampconv_attn_weights', 'ampconv_segment_mean', 'ampconv_mask_rows',
              'ampconv_masked_colsum', 'ampconv_version'):
        assert n in names


def test_library_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(built)
    for n in _declared():
        assert hasattr(lib, n), f'{n} declared in include/ampconv.h but not exported'
    lib.ampconv_version.restype = ctypes.c_int
    from ampnet_amd import _lib
    header_version = int(re.search(r'#define\s+AMPCONV_VERSION\s+(\d+)', open(HEADER).read()).group(1))
    assert lib.ampconv_version() == header_version == _lib.EXPECTED_ABI


def test_python_binding_matches_header(built):
    from ampnet_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()
    _lib.load()


def test_error_strings(built):
    from ampnet_amd import _lib
    lib = _lib.load()
    assert lib.ampconv_error_string(0) == b'ok'
    assert b'bad argument' in lib.ampconv_error_string(-1)
    with pytest.raises(_lib.AmpconvError):
        _lib.check(-2, 'x')


def test_class_api_matches_reference():
    # src/ampnet/conv/amp_conv.py:10-22: ctor args, attribute and state-dict names
    from ampnet_amd import AMPConv
    torch.manual_seed(1)
    m = AMPConv(embed_dim=16, num_heads=4)
    assert m.embed_dim == 16 and m.num_heads == 4
    assert m.attn_output is None and m.attn_output_weights is None
    assert list(m.state_dict().keys()) == [
        'multi_head_attention.in_proj_weight', 'multi_head_attention.in_proj_bias',
        'multi_head_attention.out_proj.weight', 'multi_head_attention.out_proj.bias']
    for name in ('forward', 'message', 'aggregate', 'propagate'):
        assert callable(getattr(m, name))
    # identical init RNG consumption as the reference's container module
    torch.manual_seed(1)
    ref = torch.nn.MultiheadAttention(16, 4, batch_first=True, bias=True)
    assert torch.equal(ref.in_proj_weight, m.multi_head_attention.in_proj_weight)
    assert torch.equal(ref.out_proj.weight, m.multi_head_attention.out_proj.weight)
    m.attn_output_weights = None                  # attribute stays assignable like the reference's


def test_error_behaviour_no_cpu_fallback():
    from ampnet_amd import AMPConv, InvalidConfiguration
    m = AMPConv(8, 2)
    ei = torch.tensor([[0], [1]])
    with pytest.raises(ValueError, match='GPU only'):
        m(torch.randn(4, 16), ei)
    with pytest.raises(RuntimeError):              # reference: reshape raises RuntimeError
        m(torch.randn(4, 15), ei)
    with pytest.raises(InvalidConfiguration):
        m.message(torch.randn(3, 9), torch.randn(3, 9))
    with pytest.raises(AssertionError):            # embed_dim % num_heads, asserted by torch MHA ctor
        AMPConv(10, 3)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from ampnet_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_lib.AmpconvError, match='no non-HIP fallback'):
        _lib.load()


def test_abi_version_mismatch_fails_loudly(built, monkeypatch):
    """A library of another ABI version must not load (its argument lists differ)."""
    from ampnet_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'EXPECTED_ABI', _lib.EXPECTED_ABI + 1)
    with pytest.raises(_lib.AmpconvError, match='ABI version'):
        _lib.load()


def test_softmax_stats_bytes_follows_the_family_of_the_destination_pass(built, monkeypatch):
    """ampconv_softmax_stats_bytes sizes the buffer the destination pass writes its statistics into: it must name the
    layout of the very family that pass picks, for both dtypes and under both environment switches.  Layouts: 40 floats
    per (edge, head) for edge_mfma.hip, 2 * 16 * ceil(L / 16) for the workgroup-per-unit kernels, none for the others.
    Host code only: no kernel runs."""
    from ampnet_amd import _lib
    lib = _lib.load()

    def small(L, D, H):                                          # edge_small.hip: L <= 4, a head = 4 .. 32 lanes of a wave
        dh = D // H
        return L <= 4 and any(D % v == 0 and dh % v == 0 and D // v <= 64 and dh // v in (4, 8, 16, 32) for v in (1, 2, 4))

    def expected(E, L, D, H, bf16, force_generic, small_off):
        dh = D // H
        one_wave = L <= 20 and dh in (16, 32)                    # edge_mfma.hip / edge_mfma_bf16.hip
        block = L <= 64 and 2 <= dh <= 64 and dh % 2 == 0        # edge_block_x3.hip
        if bf16:
            per_unit = 0 if one_wave or not block else 32 * ((L + 15) // 16)
        elif force_generic or (not small_off and small(L, D, H)):
            per_unit = 0
        elif one_wave:
            per_unit = 40
        else:
            per_unit = 32 * ((L + 15) // 16) if block else 0
        return E * H * per_unit * 4

    def switch(name, value):                                     # read by the library on every call
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)

    E = 1000
    for force_generic in (False, True):
        for small_off in (False, True):
            switch('AMPCONV_FORCE_GENERIC', '1' if force_generic else None)
            switch('AMPCONV_SMALL', '0' if small_off else None)
            for L in (1, 4, 13, 16, 17, 20, 21, 40, 64, 65):
                for dh in (3, 8, 16, 32, 50, 64, 66):
                    for H in (1, 2, 8):
                        for code in (_lib.AMPCONV_F32, _lib.AMPCONV_BF16):
                            got = lib.ampconv_softmax_stats_bytes(E, L, dh * H, H, code)
                            want = expected(E, L, dh * H, H, code == _lib.AMPCONV_BF16, force_generic, small_off)
                            assert got == want, (L, dh, H, code, force_generic, small_off)
    # the checked example shapes; no buffer for no edges or an invalid shape
    switch('AMPCONV_FORCE_GENERIC', None)
    switch('AMPCONV_SMALL', None)
    assert lib.ampconv_softmax_stats_bytes(E, 20, 256, 8, _lib.AMPCONV_F32) == E * 8 * 40 * 4
    for code in (_lib.AMPCONV_F32, _lib.AMPCONV_BF16):
        assert lib.ampconv_softmax_stats_bytes(E, 40, 100, 2, code) == E * 2 * 96 * 4
    assert lib.ampconv_softmax_stats_bytes(E, 4, 64, 8, _lib.AMPCONV_F32) == 0
    assert lib.ampconv_softmax_stats_bytes(E, 4, 64, 8, _lib.AMPCONV_BF16) == E * 8 * 32 * 4
    assert lib.ampconv_softmax_stats_bytes(0, 20, 256, 8, _lib.AMPCONV_F32) == 0
    assert lib.ampconv_softmax_stats_bytes(E, 20, 250, 8, _lib.AMPCONV_F32) == 0
    assert lib.ampconv_softmax_stats_bytes(E, 20, 256, 8, 7) == 0


def test_long_segment_chunk_follows_the_graph_size(monkeypatch):
    """64 edges per chunk on small graphs (a chunk is one wave's serial walk), 128 from a million edges up
    (DESIGN.md section 5); AMPCONV_HUB_CHUNK pins it."""
    from ampnet_amd import _lib
    monkeypatch.setattr(_lib, 'HUB_CHUNK', 0)
    assert _lib.hub_chunk(10_556) == 64 and _lib.hub_chunk((1 << 20) - 1) == 64
    assert _lib.hub_chunk(1 << 20) == 128 and _lib.hub_chunk(40_000_000) == 128
    monkeypatch.setattr(_lib, 'HUB_CHUNK', 256)
    assert _lib.hub_chunk(100) == 256 and _lib.hub_chunk(40_000_000) == 256


def test_bench_node_phase_roofline_object(monkeypatch):
    """`node_phase_mfma` of the bench line: three fp16 products per fp32 product for the native fp32 projections (six
    bf16 ones with the scaled mode switched off), one for bf16 storage, none for the library fp32 GEMMs (they run on
    the fp32 pipe)."""
    import bench
    from ampnet_amd.conv import functional as F_
    flops = 24 * 20 * 256 * 256 * 1_000_000
    for scaled, n in ((True, 3), (False, 6)):
        monkeypatch.setattr(F_, 'PROJ_SCALED', scaled)
        o = bench._node_phase_mfma(flops, 0.1725, 'f32', 'native')
        assert o['bound'] == 'mfma' and o['matrix_products_per_fp32_product'] == n and o['peak_TFLOPs'] == 2500.0
        assert abs(o['achieved_TFLOPs_16bit_issued'] - n * flops / 0.1725 / 1e12) < 1e-6
        assert abs(o['frac'] - o['achieved_TFLOPs_16bit_issued'] / 2500.0) < 1e-12
    assert bench._node_phase_mfma(flops, 0.12, 'bf16', 'native')['matrix_products_per_fp32_product'] == 1
    assert bench._node_phase_mfma(flops, 0.24, 'f32', 'fp32') is None
    assert bench._node_phase_mfma(flops, 0.0, 'f32', 'native') is None



def test_bench_dumped_outputs_are_a_fixed_row_sample(monkeypatch):
    """bench.py --dump-outputs: y and x.grad are cut to the SAME fixed, seeded rows (all rows, in order, when they fit),
    float32, and everything together stays within the size limit; the parameter gradients are whole."""
    import bench
    import numpy as np
    layer = torch.nn.Linear(64, 32)
    x = torch.randn(1000, 64, requires_grad=True)
    y = layer(x)
    y.backward(torch.randn_like(y))
    params = list(layer.named_parameters())
    full = bench._outputs(y, x, params)
    assert np.array_equal(full['y'], y.detach().numpy()) and np.array_equal(full['x.grad'], x.grad.numpy())
    assert np.array_equal(full['weight.grad'], layer.weight.grad.numpy()) and full['bias.grad'].shape == (32,)
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 64 << 10)
    a, b = bench._outputs(y, x, params), bench._outputs(y, x, params, {'node_idx': np.arange(10.0)})
    assert sum(v.nbytes for v in a.values()) <= 64 << 10 and sum(v.nbytes for v in b.values()) <= 64 << 10
    assert all(v.dtype == np.float32 for v in a.values()) and b['node_idx'].dtype == np.float64
    rows = [int(np.nonzero((y.detach().numpy() == r).all(axis=1))[0][0]) for r in a['y']]
    assert 0 < len(rows) < 1000 and rows == sorted(set(rows))
    assert np.array_equal(a['x.grad'], x.grad.numpy()[rows]) and np.array_equal(bench._outputs(y, x, params)['y'], a['y'])

def test_register_budgets_of_the_kernels_that_must_not_spill():
    """hipcc's kernel-resource-usage remarks, kept by __graft_entry__.build() in build/obj/*.usage.json.
    * proj_rows_kernel streams its rows with inline-assembly loads whose waits are counted by hand: a register spilled
      between such a load and its wait would be saved before the data has landed.  Every variant with assembly loads
      spills nothing; the two ragged six-product shapes, which do spill, keep compiler-managed loads (kAsmRows).
    * bwd_src_mfma_t4 / bwd_dst_mfma_t4 (config 4's dominant kernels) run at three waves per SIMD, i.e. at most 168
      registers, and a spill reload inside their edge loop carries a vmcnt(0) that drains the prefetched tiles
      (measured: +4.5 % with two spilled registers)."""
    import glob
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = glob.glob(os.path.join(root, 'build', 'obj', '*.usage.json'))
    if not files:
        import pytest
        # a library built in-tree without its usage records is a broken build, not a reason to skip
        # (on the GPU box neither travels -- build/obj is scratch there -- and the skip stands)
        assert not glob.glob(os.path.join(root, 'build', 'obj', '*.o')), \
            'build/obj holds objects but no *.usage.json: rebuild with __graft_entry__.build(force=True)'
        pytest.skip('no build/obj/*.usage.json: run __graft_entry__.build() first')
    usage = {}
    for f in files:
        usage.update(json.load(open(f)))
    rows = {k: v for k, v in usage.items() if 'proj_rows_kernel' in k and 'bf16' not in k}
    assert len(rows) == 10              # 2 tile shapes x (ragged x {six products, scaled} + plane output)
    for k, v in rows.items():
        ragged_six = 'ELb1ELb0ELb0EEEv' in k                  # <..., RAGGED = true, HP = false, PLANES = false>
        assert ragged_six or v['spill'] == 0, (k, v)          # (ragged six-product: compiler-managed loads, spills are safe)
    # the plane-format edge kernels (config 4's edge phase since round 5): forward at four waves per SIMD, both backward
    # passes at three, nothing spilled
    for name, budget, variants in (('fwd_f16x2', 128, 4), ('bwd_dst_f16x2', 168, 8), ('bwd_src_f16x2', 168, 8)):
        ks = [k for k in usage if name in k]
        assert len(ks) == variants, (name, ks)           # {L = 20, L < 20} x {dh = 32, 16} (x {statistics hand-off, own softmax})
        for k in ks:
            assert usage[k]['spill'] == 0 and usage[k]['vgprs'] <= budget, (k, usage[k])
    # the workgroup-per-unit kernels on three bf16 planes (the AMPGCN class-default shape): a spill reload in the edge loop
    # waits with vmcnt(0) behind the prefetched tiles (measured on the first version: the forward kernel with 12 spilled
    # registers ran as if it had no prefetch at all); forward at three waves per SIMD, both backward passes at two
    for name, budget, variants in (('fwd_x3', 168, 16), ('bwd_dst_x3', 256, 32), ('bwd_src_x3', 256, 16)):
        ks = [k for k in usage if name in k]
        assert len(ks) == variants, (name, ks)           # {2, 4 floats per lane} x {1..4 token tiles} x {dh <= 32, dh <= 64} (x {statistics})
        for k in ks:
            assert usage[k]['spill'] == 0 and usage[k]['vgprs'] <= budget, (k, usage[k])
    # ... and their two-plane fp16 siblings behind the bound-carrying entry points (ampconv_*_edge_scaled): forward at four
    # waves per SIMD, both backward passes at three
    for name, budget, variants in (('fwd_xh', 128, 16), ('bwd_dst_xh', 168, 32), ('bwd_src_xh', 168, 16)):
        ks = [k for k in usage if name in k]
        assert len(ks) == variants, (name, ks)
        for k in ks:
            assert usage[k]['spill'] == 0 and usage[k]['vgprs'] <= budget, (k, usage[k])
    # ... and the single-plane kernels of bf16 storage on the same structure
    for name, budget, variants in (('fwd_xb', 128, 16), ('bwd_dst_xb', 168, 32), ('bwd_src_xb', 168, 16)):
        ks = [k for k in usage if name in k]
        assert len(ks) == variants, (name, ks)
        for k in ks:
            assert usage[k]['spill'] == 0 and usage[k]['vgprs'] <= budget, (k, usage[k])
    hot = [k for k in usage if ('bwd_src_mfma_t4ILi32ELb1ELb1E' in k or 'bwd_dst_mfma_t4ILi32ELb1ELb1ELb1E' in k
                                or 'fwd_mfma_t4ILi32ELb1ELb1E' in k)]
    assert len(hot) == 3, hot
    for k in hot:
        assert usage[k]['spill'] == 0 and usage[k]['vgprs'] <= 168, (k, usage[k])


def test_shipped_isa_keeps_the_transposed_read_fences():
    """The ISA that __graft_entry__.build() keeps for every source that reads MFMA fragments with ds_read_b64_tr_b16
    (build/obj/<source>-hip-amdgcn-amd-amdhsa-gfx950.s) against tools/scan_tr_hazard.py's gate: no MFMA consumes a
    transposed fragment without a full lgkmcnt(0) drain in between, and no transposed read redefines a fragment register
    within 8 issue cycles of the MFMA that reads it.  Those two things are what separates the weight-gradient build that
    gave wrong sums (-DAMPCONV_WG_NOFENCE rebuilds it) from the one that does not; the fences in the
    sources are scheduling requests, and this is the check that hipcc honoured them."""
    import glob
    import os
    import sys
    import pytest
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    sys.path.insert(0, root)
    import scan_tr_hazard
    import __graft_entry__ as g
    srcs = [s for s in sorted(glob.glob(os.path.join(g.CSRC, '*.hip'))) if g.uses_transposed_reads(s)]
    assert len(srcs) >= 4, srcs                      # proj_gemm, proj_gemm_bf16, edge_mfma_bf16, edge_mfma_f16x2
    objdir = os.path.join(root, 'build', 'obj')
    if not glob.glob(os.path.join(objdir, '*.o')):
        pytest.skip('no build/obj: run __graft_entry__.build() first (the GPU box receives the built library only)')
    for s in srcs:
        isa = os.path.join(objdir, os.path.basename(s)[:-4] + '-hip-amdgcn-amd-amdhsa-gfx950.s')
        assert os.path.exists(isa), f'{isa} missing: rebuild with __graft_entry__.build(force=True)'
        assert os.path.getmtime(isa) >= os.path.getmtime(s), f'{isa} is older than its source'
        text = open(isa).read()
        assert 'ds_read_b64_tr_b16' in text, isa
        hits = scan_tr_hazard.gate(isa)
        assert not hits, {k: v[:2] for k, v in hits.items()}
