"""bf16-storage training, the parts that need no GPU: the numpy model of the mixed-precision step
(tests/optim_mixed_reference.py) and its rounding helper, the stall of a bf16 parameter under torch.optim.Adam that the
fp32 master exists for, and the construction of AMPGCN(storage_dtype=torch.bfloat16) and of FusedAdam over it."""
import numpy as np
import pytest
import torch

import optim_mixed_reference as mixed


def _torch_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def test_bf16_rounding_helper_is_torchs():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    vals = bits.view(np.float32)
    vals = vals[~np.isnan(vals)]
    assert vals.size > 4000
    assert np.array_equal(mixed.bf16_round(vals).view(np.uint32), _torch_bf16(vals).view(np.uint32))
    # ties: exactly half a bf16 ulp above an even and above an odd mantissa, both signs; one bit to either side of a tie
    ties = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,
                     0x00008000, 0x00018000, 0x80008000], dtype=np.uint32).view(np.float32)
    got = mixed.bf16_round(ties).view(np.uint32)
    assert np.array_equal(got, _torch_bf16(ties).view(np.uint32))
    assert list(got[:4]) == [0x3F800000, 0x3F820000, 0xBF800000, 0xBF820000]          # to even
    top = np.array([np.inf, -np.inf, np.finfo(np.float32).max, -np.finfo(np.float32).max, 3.3895314e38, 0.0, -0.0],
                   dtype=np.float32)                                                  # 3.3895314e38: the largest bf16
    got = mixed.bf16_round(top)
    assert np.array_equal(got.view(np.uint32), _torch_bf16(top).view(np.uint32))
    assert np.isinf(got[2]) and np.isinf(got[3]) and got[4] == top[4]
    assert np.isnan(mixed.bf16_round(np.array([np.nan], np.float32))[0])


def test_a_bf16_parameter_stalls_under_adam_and_the_master_does_not():
    """lr = 1e-3 (the distributed reference script's), constant gradient 1: Adam's update is lr per step whatever the step
    count.  At 1.0 half a bf16 ulp is 2^-9 = 1.95e-3 downwards: every update is rounded away."""
    p16 = torch.nn.Parameter(torch.ones(1, dtype=torch.bfloat16))
    p32 = torch.nn.Parameter(torch.ones(1))
    opts = [torch.optim.Adam([p], lr=1e-3) for p in (p16, p32)]
    for _ in range(100):
        for p, o in zip((p16, p32), opts):
            p.grad = torch.ones_like(p)
            o.step()
    assert p16.item() == 1.0
    assert abs(p32.item() - 0.9) < 1e-5                        # 0.9000013: the accumulated fp32 error of 100 steps
    model = mixed.MixedAdam([np.ones(1, np.float32)], [mixed.BF16], lr=1e-3)
    for _ in range(100):
        model.step([np.ones(1, np.float32)])
    assert abs(float(model.master[0][0]) - 0.9) < 1e-4
    assert float(model.p[0][0]) == float(mixed.bf16_round(model.master[0].astype(np.float32))[0]) == 0.8984375


def test_mixed_model_on_fp32_tensors_is_the_fp32_model():
    import optim_reference as ref
    params, grads = ref.make_params(ref.SIZES, 1), ref.make_grads(ref.SIZES, 2)
    a = ref.Adam(params, lr=0.1, weight_decay=1e-4, max_grad_norm=1.0).step(grads, 0.5)
    b = mixed.MixedAdam(params, [mixed.F32] * len(params), lr=0.1, weight_decay=1e-4, max_grad_norm=1.0).step(grads, 0.5)
    assert all(np.array_equal(x, y) for x, y in zip(a.p, b.master)) and a.norm == b.norm
    # a bf16 tensor starts from the rounded parameter and is stored as the rounded master
    c = mixed.MixedAdam(params, [mixed.BF16] * len(params), lr=0.1).step(grads)
    assert all(np.array_equal(p, mixed.bf16_round(m.astype(np.float32))) for p, m in zip(c.p, c.master))


CFG = dict(device='cpu', embedding_dim=8, num_heads=2, num_node_features=11, num_sampled_vectors=4, output_dim=3, feat_emb_dim=7,
           dropout_rate=0.0, dropout_adj_rate=0.0)


@pytest.mark.parametrize('flags', [{}, {'layer_norm': True}, {'average_pooling_flag': False}], ids=['plain', 'norm', 'token0'])
def test_bf16_storage_model_parameters(flags):
    from ampnet_amd import AMPGCN
    torch.manual_seed(5)
    ref = AMPGCN(**CFG, **flags)
    torch.manual_seed(5)
    model = AMPGCN(**CFG, **flags, storage_dtype=torch.bfloat16)
    assert model.storage_dtype == torch.bfloat16 and ref.storage_dtype == torch.float32
    assert list(model.state_dict()) == list(ref.state_dict())
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if name.startswith(('conv1.', 'conv2.')):
            assert p.dtype == torch.bfloat16 and torch.equal(p, q.to(torch.bfloat16)), name
        else:
            assert p.dtype == torch.float32 and torch.equal(p, q), name
    assert all(p.dtype == torch.float32 for p in ref.parameters())                   # the default is unchanged
    assert model._tokens[0].token_dtype == torch.bfloat16 and ref._tokens[0].token_dtype == torch.float32


def test_other_storage_dtypes_are_refused():
    from ampnet_amd import AMPGCN
    for dt in (torch.float16, torch.float64):
        with pytest.raises(ValueError, match='storage_dtype'):
            AMPGCN(**CFG, storage_dtype=dt)


@pytest.mark.parametrize('cast', [lambda m: m.float(), lambda m: m.to(torch.bfloat16)], ids=['float', 'bfloat16'])
def test_a_cast_of_the_whole_model_is_refused_at_forward(cast):
    from ampnet_amd import AMPGCN
    import types
    model = cast(AMPGCN(**CFG, storage_dtype=torch.bfloat16))
    data = types.SimpleNamespace(x=torch.ones(5, 11), edge_index=torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError, match='storage_dtype'):                          # before anything touches a device
        model(data)


def test_fused_adam_accepts_bf16_and_refuses_other_dtypes():
    from ampnet_amd import AMPGCN, FusedAdam
    model = AMPGCN(**CFG, storage_dtype=torch.bfloat16)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    assert len(opt.state) == 0
    sd = opt.full_precision_state_dict(model)                                       # before any step: p.float()
    assert list(sd) == list(model.state_dict()) and all(t.dtype == torch.float32 for t in sd.values())
    w = model.conv1.multi_head_attention.in_proj_weight
    assert torch.equal(sd['conv1.multi_head_attention.in_proj_weight'], w.detach().float())
    for dt in (torch.float16, torch.float64):
        p = torch.nn.Parameter(torch.zeros(3, dtype=dt))
        bad = FusedAdam([p])                                                        # accepted here, refused at step
        p.grad = torch.zeros_like(p)
        with pytest.raises(ValueError, match=f'a parameter is {dt}; .*float32 or bfloat16 parameters'):
            bad.step()
        assert len(bad.state) == 0


def test_load_state_dict_keeps_fp32_state_of_bf16_parameters():
    """torch casts loaded state to the parameter's dtype; the moments and the master of a bf16 parameter must come back
    with all their fp32 bits."""
    from ampnet_amd import FusedAdam
    p = torch.nn.Parameter(torch.ones(4, dtype=torch.bfloat16))
    q = torch.nn.Parameter(torch.ones(2))
    opt = FusedAdam([p, q], lr=1e-3)
    fine = torch.tensor([1.0001, 0.9003, 1e-7, 3.00001])                           # none of them a bf16 value
    opt.state[p].update(step=3, exp_avg=fine.clone(), exp_avg_sq=fine.clone() * 2, master=fine.clone() * 3)
    opt.state[q].update(step=3, exp_avg=torch.ones(2), exp_avg_sq=torch.ones(2))
    sd = opt.state_dict()
    twin = FusedAdam([torch.nn.Parameter(torch.ones(4, dtype=torch.bfloat16)), torch.nn.Parameter(torch.ones(2))])
    twin.load_state_dict(sd)
    st = twin.state[twin.param_groups[0]['params'][0]]
    assert st['step'] == 3 and sorted(st) == ['exp_avg', 'exp_avg_sq', 'master', 'step']
    for k, want in (('exp_avg', fine), ('exp_avg_sq', fine * 2), ('master', fine * 3)):
        assert st[k].dtype == torch.float32 and torch.equal(st[k], want), k
        assert st[k].data_ptr() != sd['state'][0][k].data_ptr()                     # a copy, not the checkpoint's tensor
    assert sorted(twin.state[twin.param_groups[0]['params'][1]]) == ['exp_avg', 'exp_avg_sq', 'step']
