"""A stock 2-layer LlamaForCausalLM (8 / 2 heads) with llama3 or YaRN rope_parameters over a small original length,
trained on the seeded Markov stream and patched with patch_llama, against the deployment rule rotating with HF's scaled
tables (tests/rope_ppl.py): token by token, parallel prefill + decode, and warm-cache chunks; generate() continues on a
warm cache.  Kernels that rotate with the theta rule instead of the model's table fail the bar."""
import pytest
import torch

from tests import rope_ppl

pytestmark = pytest.mark.gpu
NORTH_STAR = 0.01 / 5.47   # as tests/test_llama_gpu.py: 1.83e-3 relative perplexity


@pytest.mark.parametrize("kind,route", [("llama3", "token"), ("llama3", "prefill"), ("llama3", "chunk"),
                                        ("yarn", "token")])
def test_scaled_rope_model_ppl_vs_deploy_rule(kind, route):
    r = rope_ppl.run(kind, route)
    print("%s %s: fp16 ppl %.4f, kernel ppl %.4f, deploy rule %.4f, rel delta %.2e" %
          (kind, route, r["ppl_fp16"], r["ppl_kernel"], r["ppl_deploy_rule"], r["rel_delta"]))
    assert r["ppl_fp16"] < 20, "the stand-in model did not train"
    assert abs(r["rel_delta"]) <= NORTH_STAR, r


def test_generate_continues_on_a_warm_cache():
    from kvquant_amd import llama as kl
    model, ids, quantizers = rope_ppl.trained("llama3")
    m = rope_ppl.patched(model, quantizers)
    core = m.model.layers[0].self_attn.kvq
    assert core.rope.rope_type == "llama3" and core.kcache.rope is core.rope
    a = kl.generate(m, ids[:, :200], max_new_tokens=8)
    n1 = core.kcache.klen
    b = kl.generate(m, ids[:, 200:260], max_new_tokens=8)
    assert a.shape[1] == 208 and b.shape[1] == 68
    assert n1 >= 207 and core.kcache.klen == n1 + 60 + (n1 - 200)
    assert bool(((b[0, 60:] >= 0) & (b[0, 60:] < m.config.vocab_size)).all())
