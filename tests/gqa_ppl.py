"""Grouped-query attention variant of the perplexity comparator of tests/ppl_harness.py: a stock LlamaForCausalLM
with num_key_value_heads < num_attention_heads, and the deployment rule (oracle.glue restatement of the quantise ->
dequantise of every token, ppl_harness.DeployRuleLinear) applied to the Hkv-head k_proj / v_proj outputs, the
dequantised KV heads then repeated per group (transformers' repeat_kv) in front of the deployment path's attention
arithmetic (ppl_harness._deploy_arith_forward).  TEST INFRASTRUCTURE (imports the oracle)."""
import copy
import types

import torch
import torch.nn as nn

from tests import ppl_harness as ph


def make_gqa_model(layers=2, vocab=4096, hidden=1024, heads=8, kv_heads=2, inter=2048, seed=0, device="cuda",
                   maxseqlen=512, dtype=torch.float16, **knobs):
    from transformers import LlamaConfig, LlamaForCausalLM
    from kvquant_amd import llama as kl
    cfg = LlamaConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers,
                      num_attention_heads=heads, num_key_value_heads=kv_heads, max_position_embeddings=maxseqlen,
                      attention_bias=False, tie_word_embeddings=False)
    cfg = kl.kvquant_config(cfg, maxseqlen=maxseqlen, **knobs)
    torch.manual_seed(seed)
    return LlamaForCausalLM(cfg).to(dtype).to(device).eval()


class RepeatKV(nn.Module):
    """y [..., Hkv*hd] of the wrapped module -> [..., Hkv*G*hd] with every KV head repeated G times (repeat_kv)"""

    def __init__(self, inner, G, hd):
        super().__init__()
        self.inner, self.G, self.hd = inner, G, hd

    def forward(self, x):
        y = self.inner(x)
        s = y.shape
        return y.reshape(*s[:-1], s[-1] // self.hd, self.hd).repeat_interleave(self.G, dim=-2).reshape(*s[:-1], s[-1] * self.G)


@torch.no_grad()
def deploy_rule_ppl_gqa(model, ids, quantizers, bits, first_few_fp16=-1, norm=False, n_prompt=0):
    """ppl_harness.deploy_rule_ppl for a GQA model: K / V quantised over the Hkv*hd channels the caches hold, KV heads
    repeated after dequantisation"""
    m = copy.deepcopy(model)
    cfg = m.config
    H, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    G, hd = H // Hkv, cfg.hidden_size // cfg.num_attention_heads
    theta = getattr(cfg, "rope_theta", None) or (getattr(cfg, "rope_parameters", None) or {}).get("rope_theta", 10000.0)
    for i, layer in enumerate(m.model.layers):
        at = layer.self_attn
        for name, is_k in (("k_proj", True), ("v_proj", False)):
            lin = getattr(at, name)
            dq = ph.DeployRuleLinear(lin, quantizers["model.layers.%d.self_attn.%s" % (i, name)], bits, is_k, Hkv,
                                     first_few_fp16, norm)
            wrap = RepeatKV(dq, G, hd)
            wrap.lin = RepeatKV(lin, G, hd)      # (the fp16 sink / prompt rows of _deploy_arith_forward read .lin)
            setattr(at, name, wrap)
        at.kvq_heads, at.kvq_hd, at.kvq_theta = H, hd, float(theta)
        at.kvq_ff = max(first_few_fp16, 0)
        at.kvq_nprompt = n_prompt
        at.kvq_scores64 = False
        at.forward = types.MethodType(ph._deploy_arith_forward, at)
    return ph.ppl_full_sequence(m, ids)


def run(n_tokens=512, bits=4, first_few_fp16=0, n_prompt=0, seed=0, device="cuda", vocab=4096, train_steps=300):
    """perplexity of the patched GQA model (kernel path: token by token, or a parallel prefill of n_prompt tokens and
    decode) against deploy_rule_ppl_gqa on the same model, tokens and calibrated quantizers.  As in
    tests/test_llama_gpu.py the model is first trained on the seeded Markov stream (ideal perplexity 5.48), so that a
    relative perplexity difference means what it means for a real model (a random-init model sits at the vocabulary
    size, where the comparison is noise)."""
    from kvquant_amd import calibrate
    model = make_gqa_model(vocab=vocab, seed=seed, device=device, maxseqlen=n_tokens + 64, dtype=torch.float32,
                           abits=bits, include_sparse=True, first_few_fp16=first_few_fp16)
    stream = ph.MarkovStream(vocab, seed=seed)
    ph.train_markov(model, stream, steps=train_steps)
    model = model.half().eval()
    ids = stream.sample(1, n_tokens).to(device)
    calib = stream.sample(1, 2048).to(device)
    quantizers = calibrate.calibrate_llama(model, calib, bits=bits, include_sparse=True, sparsity_threshold=0.99)
    ff = first_few_fp16 if first_few_fp16 else -1
    fp16 = ph.ppl_full_sequence(model, ids)
    ker = ph.kernel_path_ppl(model, ids, quantizers, n_prompt=n_prompt)
    dep = deploy_rule_ppl_gqa(model, ids, quantizers, bits, first_few_fp16=ff, n_prompt=n_prompt)
    return {"ppl_fp16": fp16, "ppl_kernel": ker, "ppl_deploy_rule": dep, "rel_delta": (ker - dep) / dep}
