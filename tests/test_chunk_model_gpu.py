"""Multi-token chunks on a warm model: a prompt, then continuation chunks of 64 tokens through model(...), against the
same tokens fed one at a time (the q_len == 1 path); and generate() called twice on the same caches."""
import pytest
import torch
import torch.nn as nn

from tests import gqa_ppl
from tests import ppl_harness as ph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORTH_STAR = 0.01 / 5.47   # as tests/test_llama_gpu.py: 1.83e-3 relative perplexity
N_PROMPT, N_TOKENS, CHUNK = 192, 512, 64

_MODELS = {}


def _model(kind):
    """a 2-layer stand-in trained on the seeded Markov stream, patched, with calibrated nuq4 quantizers"""
    from kvquant_amd import calibrate
    from kvquant_amd import llama as kl
    if kind not in _MODELS:
        knobs = dict(abits=4, include_sparse=True, first_few_fp16=0 if kind == "mha" else 5)
        if kind == "mha":
            m = ph.make_model(layers=2, vocab=4096, hidden=1024, heads=8, device=DEV, maxseqlen=1024, dtype=torch.float32,
                              **knobs)
        else:
            m = gqa_ppl.make_gqa_model(vocab=4096, device=DEV, maxseqlen=1024, dtype=torch.float32, **knobs)
        stream = ph.MarkovStream(4096, seed=0)
        ph.train_markov(m, stream, steps=200)
        m = m.half().eval()
        ids = stream.sample(1, N_TOKENS).to(DEV)
        q = calibrate.calibrate_llama(m, stream.sample(1, 2048).to(DEV), bits=4, include_sparse=True,
                                      sparsity_threshold=0.99)
        kl.patch_llama(m)
        _MODELS[kind] = (m, ids, q, stream)
    return _MODELS[kind]


@torch.no_grad()
def _continuation_logits(m, ids, q, step):
    from kvquant_amd import llama as kl
    kl.load_quantizers(m, q, include_sparse=True, sparsity_threshold=0.99)       # (resets the caches)
    logits = [m(ids[:, :N_PROMPT], use_cache=False).logits[0, -1:]]
    for s in range(N_PROMPT, N_TOKENS - 1, step):
        logits.append(m(ids[:, s:min(s + step, N_TOKENS - 1)], use_cache=False).logits[0])
    return torch.cat(logits).float()                                            # predicts ids[N_PROMPT:]


@pytest.mark.parametrize("kind", ["mha", "gqa"])
def test_chunks_vs_token_by_token(kind):
    m, ids, q, _ = _model(kind)
    a = _continuation_logits(m, ids, q, CHUNK)
    b = _continuation_logits(m, ids, q, 1)
    tgt = ids[0, N_PROMPT:]
    ppl_a = float(torch.exp(nn.functional.cross_entropy(a, tgt)))
    ppl_b = float(torch.exp(nn.functional.cross_entropy(b, tgt)))
    agree = float((a.argmax(-1) == b.argmax(-1)).float().mean())
    rel = (ppl_a - ppl_b) / ppl_b
    print("%s: ppl chunks of %d %.4f, token by token %.4f, rel %.2e, greedy agreement %.4f" %
          (kind, CHUNK, ppl_a, ppl_b, rel, agree))
    assert ppl_b < 20, "the stand-in model did not train"
    assert abs(rel) <= NORTH_STAR
    assert agree >= 0.98


@pytest.mark.parametrize("kind", ["mha", "gqa"])
def test_generate_twice(kind, monkeypatch):
    """generate(A) then generate(B) on the warm caches: B continues the conversation (positions follow klen); its first
    new token is that of the token-by-token route"""
    from kvquant_amd import attention
    from kvquant_amd import llama as kl
    m, ids, q, stream = _model(kind)
    A, B = ids[:, :100], stream.sample(1, 80).to(DEV)
    firsts = []
    for chunked in (True, False):
        monkeypatch.setattr(attention, "CHUNK_ATTEND", chunked)
        kl.load_quantizers(m, q, include_sparse=True, sparsity_threshold=0.99)
        s1 = kl.generate(m, A, max_new_tokens=8)
        klen = m.model.layers[0].self_attn.kvq.kcache.klen
        s2 = kl.generate(m, B, max_new_tokens=4)
        assert s1.shape[1] == 108 and s2.shape[1] == 84
        assert m.model.layers[0].self_attn.kvq.kcache.klen == klen + 80 + 3
        firsts.append(int(s2[0, 80]))
    assert firsts[0] == firsts[1]
