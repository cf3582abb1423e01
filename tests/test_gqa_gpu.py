"""Grouped-query attention on the GPU: the grouped q.K^T / p.V kernels against the pinned MHA kernels run per group
member, the one-call layer step (decode_kv with Hq = G * Hkv) against the restated pipeline, the grouped prefill
attention against fp32 torch with repeated K / V, and KVQuantAttention / patch_llama with a GQA model."""
import math

import pytest
import torch

from tests import gqa_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# every width and shape up to 4096 tokens; at 128K every width at (8, 4) and every shape at 4 bit
CASES = [(b, h, g, L) for b in (2, 3, 4) for (h, g) in ((1, 2), (4, 7), (8, 4), (8, 8)) for L in (1, 37, 4096, 131072)
         if L < 131072 or (h, g) == (8, 4) or b == 4]
# ragged multi-chunk lengths, KV head counts that the score plan does not divide evenly (3, 5) and Hkv = 2
CASES += [(b, 8, 4, 4096 + 37) for b in (2, 3, 4)] + [(b, 3, 2, L) for b in (3, 4) for L in (37, 4096 + 37, 65536 + 5)] + \
    [(4, 5, 3, 4096 + 37), (2, 5, 3, 65536 + 5), (4, 2, 4, 37), (3, 2, 4, 4096 + 37), (4, 2, 4, 131072 + 37)]


@pytest.mark.parametrize("bits,Hkv,G,L", CASES)
def test_score_gqa_vs_mha(bits, Hkv, G, L):
    gqa_check.score_against_mha(bits, Hkv, G, L, max_len=L + 3, pos_offset=5, device=DEV, seed=bits * 100 + G)


@pytest.mark.parametrize("bits,Hkv,G,L", CASES)
def test_mix_gqa_vs_mha(bits, Hkv, G, L):
    gqa_check.mix_against_mha(bits, Hkv, G, L, max_len=L + 3, device=DEV, seed=bits * 100 + G)


def test_gqa_1m_tokens():
    gqa_check.score_against_mha(4, 8, 4, 1 << 20, device=DEV, seed=7)
    gqa_check.mix_against_mha(4, 8, 4, 1 << 20, device=DEV, seed=7)


@pytest.mark.parametrize("Hkv,G", [(8, 4), (2, 4)])
@pytest.mark.parametrize("sinks", [0, 5])
def test_decode_kv_gqa_layer_step(Hkv, G, sinks):
    from kvquant_amd.cache import QuantK, QuantV, decode_kv
    from oracle.glue import OracleQuantK, OracleQuantV
    from tests import decode_check, util
    bits, prefill, steps, max_len = 4, 40, 4, 64
    C, Hq = Hkv * 128, Hkv * G
    quant, scale, shift = decode_check.quantizer(bits, seed=3, C=C)
    n = prefill + steps
    ks = util.k_tokens(n, scale, shift, seed=31)
    vs = util.v_tokens_no_ties(n, Cn=C, seed=41, k=int(((1 - 0.99) / 2) * C) + 1)
    gen = torch.Generator().manual_seed(51)
    kw = dict(bits=bits, hidden_size=C, num_heads=Hkv, max_position_embeddings=max_len, include_sparse=True,
              sparsity_threshold=0.99, first_few_fp16=0)
    ok, ov = OracleQuantK(rope_theta=10000.0, **kw), OracleQuantV(**kw)
    kw["first_few_fp16"] = sinks
    gk, gv = QuantK(rope_theta=10000.0, device=DEV, **kw), QuantV(device=DEV, **kw)
    for c in (ok, ov, gk, gv):
        c.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99)
    kp = ks[:prefill].half().float().t().reshape(Hkv, 128, prefill).contiguous()
    vp = vs[:prefill].half().float().t().reshape(Hkv, 128, prefill).contiguous()
    ok.parallel_pack(kp)
    gk.parallel_pack(kp.to(DEV))
    uv, ui, lv, li = OracleQuantV.topk_inputs(vs[:prefill].half().float(), 0.99, C)
    ov.parallel_pack(vp, uv, ui, lv, li)
    gv.parallel_pack(vp.to(DEV))
    gk.klen += sinks
    gv.vlen += sinks
    k_sink = torch.randn(Hkv, 128, sinks, generator=gen).half().to(DEV) if sinks else None
    v_sink = torch.randn(Hkv, sinks, 128, generator=gen).half().to(DEV) if sinks else None
    from kvquant_amd import ops
    thetas = ops.rope_freqs(10000.0, torch.device(DEV)).cpu()     # theta_j as the kernels evaluate them
    worst = 0.0
    for i in range(steps):
        k16, v16 = ks[prefill + i].half(), vs[prefill + i].half()
        q16 = torch.randn(Hq, 128, generator=gen).half()
        ok.forward_fused_sparse(q16.view(Hkv, G, 1, 128)[:, 0], k16)                  # (the oracle's append)
        uv, ui, lv, li = OracleQuantV.topk_inputs(v16.float().unsqueeze(0), 0.99, C)
        ov.forward_fused_sparse(torch.zeros(Hkv, 1, ok.klen, dtype=torch.half), v16, uv[0], ui[0], lv[0], li[0])
        q = q16.to(DEV)
        Lc = ok.klen
        khat, vhat = gqa_check.dequant_k(ok, Lc), gqa_check.dequant_v(ov, Lc)
        if sinks:
            out, sp = decode_kv(gk, gv, q, k16.to(DEV), v16.to(DEV), k_sink=k_sink, v_sink=v_sink)
            ss = (torch.matmul(q.unsqueeze(1), k_sink.repeat_interleave(G, 0)) / math.sqrt(128))[:, 0, :]
            ref = gqa_check.attention_fp64(khat, vhat, q16, G, thetas, sinks, ss, v_sink.repeat_interleave(G, 0))
        else:
            out, sp = decode_kv(gk, gv, q, k16.to(DEV), v16.to(DEV))
            ref = gqa_check.attention_fp64(khat, vhat, q16, G, thetas, 0)
        assert out.shape == (1, Hq, 128)
        err = float((out[0].cpu().double() - ref).abs().max() / ref.abs().max())
        worst = max(worst, err)
        assert err < 1e-3, (i, err)
    L = n
    assert torch.equal(ok.kcache[:, :, :L], gk.kcache[:, :, :L].cpu())
    assert torch.equal(ov.vcache[:, :, :L], gv.vcache[:, :, :L].cpu())
    assert torch.equal(ok.outlier_indices[:L], gk.outlier_indices[:L].cpu())
    assert torch.equal(ok.outliers[:L].view(torch.int32), gk.outliers[:L].cpu().view(torch.int32))
    assert torch.equal(ok.outlier_indices[:L].t(), gk.outlier_indices_t[:, :L].cpu())           # the K mirror
    assert torch.equal(ok.outliers[:L].t().contiguous().view(torch.int32), gk.outliers_t[:, :L].cpu().view(torch.int32))
    assert torch.equal(ov.outlier_indices[:L], gv.outlier_indices[:L].cpu())
    assert torch.equal(ov.outliers[:L].view(torch.int32), gv.outliers[:L].cpu().view(torch.int32))
    assert torch.equal(ov.lookup_table[:L].view(torch.int32), gv.lookup_table[:L].cpu().view(torch.int32))
    print("GQA layer step Hkv=%d G=%d sinks=%d: worst rel err %.2e" % (Hkv, G, sinks, worst))


@pytest.mark.parametrize("Hq,Hkv,S", [(8, 2, 300), (32, 8, 129), (7, 1, 64)])
def test_prefill_attention_gqa(Hq, Hkv, S):
    from kvquant_amd import ops
    g = torch.Generator(device=DEV).manual_seed(S)
    q = torch.randn(Hq, S, 128, generator=g, device=DEV).half()
    k = torch.randn(Hkv, S, 128, generator=g, device=DEV).half()
    v = torch.randn(Hkv, S, 128, generator=g, device=DEV).half()
    out = ops.prefill_attention(q, k, v).view(S, Hq, 128).transpose(0, 1).float()
    G = Hq // Hkv
    kr, vr = k.float().repeat_interleave(G, 0), v.float().repeat_interleave(G, 0)
    s = torch.matmul(q.float(), kr.transpose(1, 2)) / math.sqrt(128)
    s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool, device=DEV), 1), float("-inf"))
    ref = torch.matmul(torch.softmax(s, dim=-1), vr)
    assert float((out - ref).abs().max()) < 2e-3


def test_attention_gqa_module_runs():
    """KVQuantAttention with 8 query / 2 KV heads through its own projections: shapes of the projections and caches,
    prefill + 3 decode tokens produce finite outputs of the right shape.  (Numbers: tests/test_gqa_model_gpu.py.)"""
    from kvquant_amd.attention import KVQuantAttention
    from tests import decode_check
    torch.manual_seed(0)
    a = KVQuantAttention(hidden_size=1024, num_heads=8, num_key_value_heads=2, abits=4, maxseqlen=64, device=DEV)
    assert a.k_proj.out_features == 256 and a.kcache.num_heads == 2
    quant, _, _ = decode_check.quantizer(4, seed=1, C=256)
    a.load_quantizers(quant, quant)
    x = torch.randn(1, 20, 1024, device=DEV).half() * 0.1
    y = a(x)
    assert y.shape == (1, 20, 1024) and bool(torch.isfinite(y).all())
    for _ in range(3):
        y = a(torch.randn(1, 1, 1024, device=DEV).half() * 0.1)
        assert y.shape == (1, 1, 1024) and bool(torch.isfinite(y).all())
