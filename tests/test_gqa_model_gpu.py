"""A stock 2-layer LlamaForCausalLM with 8 query / 2 KV heads, patched with patch_llama, against the deployment rule
restated by the oracle with the KV heads repeated after dequantisation (tests/gqa_ppl.py); and KVQuantAttention with
num_key_value_heads == num_heads against the MHA construction, bit for bit."""
import pytest
import torch

from tests import gqa_ppl

pytestmark = pytest.mark.gpu
NORTH_STAR = 0.01 / 5.47   # as tests/test_llama_gpu.py: 1.83e-3 relative perplexity


@pytest.mark.parametrize("knobs", [dict(), dict(n_prompt=256), dict(first_few_fp16=5)])
def test_gqa_model_ppl_vs_deploy_rule(knobs):
    # token by token (>= 16 generated tokens through decode_kv_gqa), a parallel prefill through kvq_prefill_attention_gqa
    # + decode, and 5 fp16 sink tokens (the sink-filling branch with repeated KV heads, then the step with sink scores)
    # (a 2-layer model trained on the seeded Markov stream, 512 evaluated tokens, as the MHA acceptance test does)
    r = gqa_ppl.run(n_tokens=512, bits=4, **knobs)
    print("GQA 8/2 heads nuq4 %s: fp16 ppl %.4f, kernel ppl %.4f, deploy rule %.4f, rel delta %.2e" %
          (knobs, r["ppl_fp16"], r["ppl_kernel"], r["ppl_deploy_rule"], r["rel_delta"]))
    assert r["ppl_fp16"] < 20, "the stand-in model did not train"
    assert abs(r["rel_delta"]) <= NORTH_STAR, r


def test_mha_construction_unchanged():
    """num_key_value_heads == num_heads builds and runs the MHA attention: bit-identical outputs to num_key_value_heads=None"""
    from kvquant_amd.attention import KVQuantAttention
    from tests import decode_check
    quant, _, _ = decode_check.quantizer(4, seed=2, C=1024)
    outs = []
    for kv in (None, 8):
        torch.manual_seed(0)
        a = KVQuantAttention(hidden_size=1024, num_heads=8, num_key_value_heads=kv, abits=4, maxseqlen=64, device="cuda:0")
        a.load_quantizers(quant, quant)
        assert a.num_kv_groups == 1 and a.k_proj.out_features == 1024
        g = torch.Generator(device="cuda:0").manual_seed(1)
        ys = [a(torch.randn(1, 24, 1024, generator=g, device="cuda:0").half() * 0.1)]
        for _ in range(4):
            ys.append(a(torch.randn(1, 1, 1024, generator=g, device="cuda:0").half() * 0.1))
        outs.append(ys)
    for y0, y1 in zip(*outs):
        assert torch.equal(y0, y1)
