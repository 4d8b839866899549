"""CPU checks of the fused glue (ampnet_amd/glue.py): the numpy model of the mask contract of include/ampconv.h meets
its statistical bar (the GPU kernels are then held to that model by EXACT equality, tests/test_gpu_glue.py), the host
side refuses tensors that are not on the GPU, and AMPGCN(fused_glue=True) keeps the reference's state-dict keys."""
import numpy as np
import pytest
import torch

import glue_reference as ref

N_MASK = 1 << 20


@pytest.mark.parametrize('p', [0.1, 0.6])
def test_reference_mask_statistics(p):
    thr, scale = ref.mask_params(p)
    q = 1.0 - thr / 65536.0                                     # the effective keep probability
    assert abs(float(scale) * q - 1.0) < 1e-6                   # the scale is its inverse: E[keep * scale] = 1
    keep = ref.keep_mask(1234, thr, (N_MASK,))
    sigma = np.sqrt(q * (1 - q) / N_MASK)
    assert abs(keep.mean() - q) < 5 * sigma, (keep.mean(), q, sigma)
    sigma4 = np.sqrt(q * (1 - q) / (N_MASK // 4))
    for f in range(4):                                          # each 16-bit field of the group hash on its own
        rate = keep[f::4].mean()
        assert abs(rate - q) < 5 * sigma4, (f, rate, q, sigma4)
    other = ref.keep_mask(1235, thr, (N_MASK,))
    d = 2 * q * (1 - q)                                         # two independent masks differ with this probability
    assert abs((keep != other).mean() - d) < 5 * np.sqrt(d * (1 - d) / N_MASK)
    assert np.array_equal(keep, ref.keep_mask(1234, thr, (N_MASK,)))
    assert np.array_equal(keep[:1000], ref.keep_mask(1234, thr, (1000,)))      # a function of (seed, i) alone


def test_reference_mask_edges():
    assert ref.keep_mask(7, 0, (4096,)).all()                   # threshold 0 keeps everything
    assert ref.mask_params(0.0) == (0, np.float32(1.0))
    assert ref.mask_params(0.1)[0] == 6554 and ref.mask_params(0.6)[0] == 39322
    # splitmix64 against the published test vector of the generator (state 0: first output)
    assert int(ref.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF


def test_host_mask_parameters_match_the_reference():
    from ampnet_amd.glue import mask_params
    for p in (0.0, 0.1, 0.5, 0.6):
        thr, scale = mask_params(p)
        rthr, rscale = ref.mask_params(p)
        assert thr == rthr and np.float32(scale) == rscale
    assert mask_params(0.6, training=False) == (0, 1.0)
    for bad in (-0.1, 1.0, 0.999999):
        with pytest.raises(ValueError):
            mask_params(bad)


def test_non_gpu_input_raises():
    from ampnet_amd import ActDropout, TokenReadout, act_dropout, act_dropout_pool
    x = torch.randn(4, 12)
    with pytest.raises(ValueError, match='no CPU fallback'):
        act_dropout(x, 0.1)
    with pytest.raises(ValueError, match='no CPU fallback'):
        act_dropout(x, 0.0, 'identity')
    with pytest.raises(ValueError, match='no CPU fallback'):
        act_dropout_pool(x, 4, 0.1)
    with pytest.raises(ValueError, match='no CPU fallback'):
        ActDropout(0.1)(x)
    with pytest.raises(ValueError, match='no CPU fallback'):
        TokenReadout(4, 0.1).eval()(x)
    assert not list(ActDropout(0.1).parameters()) and not list(TokenReadout(4).parameters())


def test_site_seeds_are_fresh_per_training_call():
    from ampnet_amd import ActDropout
    a, b = ActDropout(0.1, 'relu', seed=3, site=1), ActDropout(0.1, 'relu', seed=3, site=2)
    assert a.last_seed is None
    s = [a._next_seed(), a._next_seed(), b._next_seed()]
    assert len(set(s)) == 3 and a.last_seed == s[1]
    assert ActDropout(0.1, 'relu', seed=3, site=1)._next_seed() == s[0]        # reproducible from (seed, site, call)
    a.eval()
    assert a._next_seed() == 0 and a.last_seed == s[1]                         # eval draws nothing


def test_fused_model_keeps_the_state_dict_keys():
    from ampnet_amd import AMPGCN
    kw = dict(device='cpu', embedding_dim=8, num_heads=2, num_node_features=11, num_sampled_vectors=3, output_dim=2,
              feat_emb_dim=7, val_emb_dim=1)
    for pooling in (True, False):
        torch.manual_seed(0)
        plain = AMPGCN(average_pooling_flag=pooling, **kw)
        torch.manual_seed(0)
        fused = AMPGCN(average_pooling_flag=pooling, fused_glue=True, **kw)
        assert list(plain.state_dict().keys()) == list(fused.state_dict().keys())
        assert [n for n, _ in plain.named_modules()] == [n for n, _ in fused.named_modules()]
        for (_, a), (_, b) in zip(plain.state_dict().items(), fused.state_dict().items()):
            assert torch.equal(a, b)                            # same consumption of torch's generator at construction
        assert isinstance(fused.drop1, torch.nn.Dropout) and isinstance(fused.drop3, torch.nn.Dropout)
        assert not plain.fused_glue and fused.fused_glue
