"""Pin oracle/decoder_oracle.py (the fp64 decode-step restatement that tests/test_gpu_head_kernels.py checks
lvq_qwen2_decode_step against) against transformers' Qwen2DecoderLayer run in float64 on a whole causal sequence."""
import pytest
import torch

from oracle import decoder_oracle as DO


@pytest.mark.parametrize("pos0,theta", [(0, 1e6), (879, 1e6), (32000, 1e4)])
def test_decode_layer_matches_transformers_qwen2(pos0, theta):
    import transformers
    from transformers.models.qwen2 import modeling_qwen2 as Q
    d, H, Hk, inter, B, T, eps = 64, 4, 2, 96, 2, 7, 1e-6
    dh, dkv = d // H, d // H * Hk
    cfg = transformers.Qwen2Config(hidden_size=d, intermediate_size=inter, num_attention_heads=H, num_key_value_heads=Hk,
                                   num_hidden_layers=1, rms_norm_eps=eps, rope_theta=theta, max_position_embeddings=65536,
                                   vocab_size=32)
    cfg._attn_implementation = "eager"
    layer = Q.Qwen2DecoderLayer(cfg, 0).double().eval()
    g = torch.Generator().manual_seed(pos0 + 5)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (0.3 if p.dim() == 2 else 1.0))
        layer.input_layernorm.weight.add_(1.0)
        layer.post_attention_layernorm.weight.add_(1.0)
    x = torch.randn(B, T, d, generator=g, dtype=torch.float64)
    pos = torch.arange(pos0, pos0 + T)[None].expand(B, T)
    rot = Q.Qwen2RotaryEmbedding(cfg)
    mask = torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)[None, None].expand(B, 1, T, T)
    with torch.no_grad():
        want = layer(x, attention_mask=mask, position_ids=pos, position_embeddings=rot(x, pos))
        want = want[0] if isinstance(want, tuple) else want
    a, m = layer.self_attn, layer.mlp
    W = dict(ln1=layer.input_layernorm.weight.detach(), ln2=layer.post_attention_layernorm.weight.detach(),
             wqkv=torch.cat((a.q_proj.weight, a.k_proj.weight, a.v_proj.weight)).detach(),
             bqkv=torch.cat((a.q_proj.bias, a.k_proj.bias, a.v_proj.bias)).detach(), wo=a.o_proj.weight.detach(),
             wgu=torch.cat((m.gate_proj.weight, m.up_proj.weight)).detach(), wdown=m.down_proj.weight.detach())
    kc, vc = torch.zeros(B, 0, dkv, dtype=torch.float64), torch.zeros(B, 0, dkv, dtype=torch.float64)
    for t in range(T):                                 # token by token against the cache of the earlier ones
        got, k_new, v_new = DO.decode_layer(x[:, t], W, kc, vc, pos0 + t, H, Hk, eps, theta)
        kc, vc = torch.cat((kc, k_new[:, None]), 1), torch.cat((vc, v_new[:, None]), 1)
        # transformers keeps the RMSNorm statistics and cos / sin in fp32 even in a float64 model: ~1e-7 of the output
        assert (got - want[:, t]).abs().max().item() < 2e-6 * want.abs().max().item(), t
    # the cache holds the keys as transformers rotates them (apply_rotary_pos_emb on the k projection)
    cos, sin = rot(x, pos)
    k = layer.self_attn.k_proj(layer.input_layernorm(x)).view(B, T, Hk, dh).transpose(1, 2)
    _, k_rot = Q.apply_rotary_pos_emb(k, k, cos, sin)
    assert (kc - k_rot.transpose(1, 2).reshape(B, T, dkv)).abs().max().item() < 2e-6 * kc.abs().max().item()
    # the frequencies are transformers' own
    assert torch.equal(rot.inv_freq.float(), 1.0 / (theta ** (torch.arange(0, dh, 2).float() / dh)))
