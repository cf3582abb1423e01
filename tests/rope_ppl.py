"""Scaled-RoPE variant of the perplexity comparator of tests/ppl_harness.py / tests/gqa_ppl.py: a stock 2-layer
LlamaForCausalLM (8 query / 2 KV heads, head_dim 128) whose config carries rope_parameters llama3 or yarn with a small
original_max_position_embeddings (128), so that the scaling matters inside 512 tokens.  The kernel path is the model
patched with patch_llama; the deployment rule is the oracle's quantise -> dequantise of every token (DeployRuleLinear)
in front of the deployment path's attention arithmetic, rotating with transformers' scaled tables: keys in fp32 at
fl32(inv_freq_j * pos) with (cos, sin) times the attention factor, the query with HF's fp16 rows (emb.cos() * af).half().
TEST INFRASTRUCTURE (imports the oracle)."""
import copy
import math
import types

import torch
import torch.nn.functional as F

from tests import gqa_ppl
from tests import ppl_harness as ph

ROPE = {
    "llama3": dict(rope_type="llama3", rope_theta=10000.0, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                   original_max_position_embeddings=128),
    "yarn": dict(rope_type="yarn", rope_theta=10000.0, factor=4.0, original_max_position_embeddings=128),
}


def make_model(kind, layers=2, vocab=4096, hidden=1024, heads=8, kv_heads=2, inter=2048, seed=0, device="cuda",
               maxseqlen=576, dtype=torch.float32, **knobs):
    from transformers import LlamaConfig, LlamaForCausalLM
    from kvquant_amd import llama as kl
    cfg = LlamaConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers,
                      num_attention_heads=heads, num_key_value_heads=kv_heads, head_dim=hidden // heads,
                      max_position_embeddings=maxseqlen, attention_bias=False, tie_word_embeddings=False,
                      rope_parameters=dict(ROPE[kind]))
    cfg = kl.kvquant_config(cfg, maxseqlen=maxseqlen, **knobs)
    torch.manual_seed(seed)
    return LlamaForCausalLM(cfg).to(dtype).to(device).eval()


def _deploy_arith_forward_rope(self, hidden_states, position_embeddings=None, attention_mask=None,
                               past_key_values=None, **kwargs):
    """ppl_harness._deploy_arith_forward with the scaled tables (self.kvq_inv f32 [64], self.kvq_af)"""
    bsz, T, _ = hidden_states.shape
    H, hd = self.kvq_heads, self.kvq_hd
    dev = hidden_states.device
    q = self.q_proj(hidden_states).view(T, H, hd).transpose(0, 1).half()
    k = self.k_proj(hidden_states).view(T, H, hd).transpose(0, 1).float()        # fake-quantised already
    v = self.v_proj(hidden_states).view(T, H, hd).transpose(0, 1).float()
    inv, af = self.kvq_inv.to(dev), self.kvq_af
    pos = torch.arange(T, device=dev, dtype=torch.float32)
    ang = inv.unsqueeze(0) * pos.unsqueeze(1)                                    # fl32(inv_j * pos)
    cos = torch.cat((ang.cos(), ang.cos()), -1) * af
    sin = torch.cat((ang.sin(), ang.sin()), -1) * af

    def rot(x):
        return torch.cat((-x[..., hd // 2:], x[..., :hd // 2]), dim=-1)
    emb = torch.cat((ang, ang), dim=-1)
    c16, s16 = (emb.cos() * af).half(), (emb.sin() * af).half()                  # LlamaRotaryEmbedding's rows
    qr = q * c16 + rot(q) * s16
    kr = k * cos + rot(k) * sin
    scores = torch.matmul(qr.float(), kr.transpose(1, 2))
    w = (scores.half().float() * (1.0 / math.sqrt(hd))).half().float()
    mask = torch.ones(T, T, device=dev, dtype=torch.bool).tril()
    w = w.masked_fill(~mask, float("-inf"))
    p = torch.softmax(w, dim=-1, dtype=torch.float32).half().float()
    out = torch.matmul(p, v).half()
    npr = self.kvq_nprompt
    if npr > 0:
        # the prompt's own rows: a parallel prefill attends to the UNQUANTISED fp16 K / V
        kh = self.k_proj.lin(hidden_states.half()).view(T, H, hd).transpose(0, 1)[:, :npr]
        vh = self.v_proj.lin(hidden_states.half()).view(T, H, hd).transpose(0, 1)[:, :npr]
        khr = kh * c16[:npr] + rot(kh) * s16[:npr]
        sp = torch.matmul(qr[:, :npr].float(), khr.float().transpose(1, 2)) * (1.0 / math.sqrt(hd))
        sp = sp.masked_fill(~mask[:npr, :npr], float("-inf"))
        pp = torch.softmax(sp, dim=-1, dtype=torch.float32).half().float()
        out[:, :npr] = torch.matmul(pp, vh.float()).half()
    out = out.transpose(0, 1).reshape(1, T, H * hd)
    return self.o_proj(out.to(hidden_states.dtype)), None


@torch.no_grad()
def deploy_rule_ppl(model, ids, quantizers, bits, n_prompt=0):
    m = copy.deepcopy(model)
    cfg = m.config
    H, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    G, hd = H // Hkv, cfg.hidden_size // cfg.num_attention_heads
    emb = m.model.rotary_emb
    for i, layer in enumerate(m.model.layers):
        at = layer.self_attn
        for name, is_k in (("k_proj", True), ("v_proj", False)):
            lin = getattr(at, name)
            dq = ph.DeployRuleLinear(lin, quantizers["model.layers.%d.self_attn.%s" % (i, name)], bits, is_k, Hkv, -1,
                                     False)
            wrap = gqa_ppl.RepeatKV(dq, G, hd)
            wrap.lin = gqa_ppl.RepeatKV(lin, G, hd)
            setattr(at, name, wrap)
        at.kvq_heads, at.kvq_hd = H, hd
        at.kvq_inv, at.kvq_af = emb.inv_freq.float(), float(emb.attention_scaling)
        at.kvq_nprompt = n_prompt
        at.forward = types.MethodType(_deploy_arith_forward_rope, at)
    return ph.ppl_full_sequence(m, ids)


def patched(model, quantizers):
    from kvquant_amd import llama as kl
    m = copy.deepcopy(model)
    kl.patch_llama(m)
    kl.load_quantizers(m, quantizers, include_sparse=True, sparsity_threshold=0.99)
    return m


@torch.no_grad()
def chunk_path_ppl(model, ids, quantizers, n_prompt, chunk):
    """patched model: a parallel prefill of n_prompt tokens, then chunks of `chunk` tokens through model(...) on the warm
    caches (KVQuantAttention.attend_multi -> cache.chunk_kv); perplexity of the whole sequence"""
    m = patched(model, quantizers)
    n = ids.shape[1]
    logits = [m(ids[:, :n_prompt], use_cache=False).logits.float()]
    for s in range(n_prompt, n, chunk):
        logits.append(m(ids[:, s:s + chunk], use_cache=False).logits.float())
    lg = torch.cat(logits, dim=1)[0, :-1]
    return float(torch.exp(F.cross_entropy(lg, ids[0, 1:])))


_TRAINED = {}


def trained(kind, bits=4, n_tokens=512, seed=0, device="cuda", vocab=4096, train_steps=300):
    """(model fp16, evaluation ids, quantizers); the training run is cached per process and rope kind"""
    from kvquant_amd import calibrate
    if kind not in _TRAINED:
        model = make_model(kind, vocab=vocab, seed=seed, device=device, maxseqlen=n_tokens + 64, abits=bits,
                           include_sparse=True, first_few_fp16=0)
        stream = ph.MarkovStream(vocab, seed=seed)
        ph.train_markov(model, stream, steps=train_steps)
        model = model.half().eval()
        ids = stream.sample(1, n_tokens).to(device)
        calib = stream.sample(1, 2048).to(device)
        quantizers = calibrate.calibrate_llama(model, calib, bits=bits, include_sparse=True, sparsity_threshold=0.99)
        _TRAINED[kind] = (model, ids, quantizers)
    return _TRAINED[kind]


def run(kind, route="token", n_prompt=256, chunk=64, bits=4):
    """perplexity of the patched model (route "token": token by token; "prefill": parallel prefill of n_prompt tokens +
    decode; "chunk": prefill + chunks of `chunk` tokens on the warm caches) against the deployment rule with HF's tables"""
    model, ids, quantizers = trained(kind, bits=bits)
    fp16 = ph.ppl_full_sequence(model, ids)
    if route == "token":
        ker = ph.kernel_path_ppl(model, ids, quantizers)
        dep = deploy_rule_ppl(model, ids, quantizers, bits)
    elif route == "prefill":
        ker = ph.kernel_path_ppl(model, ids, quantizers, n_prompt=n_prompt)
        dep = deploy_rule_ppl(model, ids, quantizers, bits, n_prompt=n_prompt)
    else:
        ker = chunk_path_ppl(model, ids, quantizers, n_prompt, chunk)
        dep = deploy_rule_ppl(model, ids, quantizers, bits, n_prompt=n_prompt)
    return {"ppl_fp16": fp16, "ppl_kernel": ker, "ppl_deploy_rule": dep, "rel_delta": (ker - dep) / dep}
