"""Speculative generate() on the stand-in models of tests/test_chunk_model_gpu.py (MHA, and GQA with 5 sink tokens):
draft_len = 0 is today's loop; with drafts that are always right, always wrong, or looked up in a repetitive prompt, the
caches end as plain generate() leaves them and the tokens are the model's own greedy ones."""
import pytest
import torch

from tests.test_chunk_model_gpu import _model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_PROMPT, N_NEW, DRAFT = 192, 128, 7
AGREE = 0.98        # tests/test_chunk_model_gpu.py::test_chunks_vs_token_by_token: chunk-against-decode greedy agreement

_PLAIN = {}


def _reset(m, q):
    from kvquant_amd import llama as kl
    kl.load_quantizers(m, q, include_sparse=True, sparsity_threshold=0.99)


def _plain(kind):
    """the plain greedy run on freshly reset caches, once per model: (prompt, its continuation [1, N_PROMPT + N_NEW])"""
    from kvquant_amd import llama as kl
    if kind not in _PLAIN:
        m, ids, q, _ = _model(kind)
        prompt = ids[:, :N_PROMPT].clone()
        _reset(m, q)
        _PLAIN[kind] = (prompt, kl.generate(m, prompt, max_new_tokens=N_NEW))
    return _PLAIN[kind]


def _layers(m):
    return [layer.self_attn.kvq for layer in m.model.layers]


@torch.no_grad()
def _check_invariants(m, q, prompt, seq):
    """klen, zeros behind it, and the teacher-forced self-consistency of the generated tokens"""
    n_prompt = prompt.shape[1]
    assert torch.equal(seq[:, :n_prompt], prompt)
    n_new = seq.shape[1] - n_prompt
    assert n_new == N_NEW
    for core in _layers(m):
        kc, vc = core.kcache, core.vcache
        assert kc.klen == vc.vlen == n_prompt + n_new - 1
        n = kc.klen - core.first_few_fp16
        for t in (kc.kcache[:, :, n:], kc.outliers[n:], kc.outlier_indices[n:], kc.outliers_t[:, n:],
                  kc.outlier_indices_t[:, n:], vc.vcache[:, :, n:], vc.lookup_table[n:], vc.outliers[n:],
                  vc.outlier_indices[n:]):
            assert not t.any()
    _reset(m, q)
    m(prompt, use_cache=False)
    logits = m(seq[:, n_prompt:-1], use_cache=False).logits[0].float()      # row i predicts new token i + 1
    agree = float((logits.argmax(-1) == seq[0, n_prompt + 1:]).float().mean())
    print("teacher-forced greedy agreement %.4f" % agree)
    assert agree >= AGREE
    return agree


@pytest.mark.parametrize("kind", ["mha", "gqa"])
def test_draft_len_zero_is_plain_generate(kind):
    from kvquant_amd import llama as kl
    m, ids, q, _ = _model(kind)
    prompt, plain = _plain(kind)
    _reset(m, q)
    stats = {}
    seq = kl.generate(m, prompt, max_new_tokens=N_NEW, draft_len=0, stats=stats)
    assert torch.equal(seq, plain)
    assert _layers(m)[0].kcache.klen == N_PROMPT + N_NEW - 1


@pytest.mark.parametrize("kind", ["mha", "gqa"])
def test_perfect_drafts(kind):
    from kvquant_amd import llama as kl, ops
    m, ids, q, _ = _model(kind)
    prompt, plain = _plain(kind)
    cfg = m.config
    assert ops.chunk_attention_route(cfg.num_attention_heads, cfg.num_key_value_heads, 1 + DRAFT) == \
        ("grouped" if kind == "gqa" else "heads")

    def replay(seq, k):
        return plain[0, seq.numel():seq.numel() + k].tolist()
    _reset(m, q)
    stats = {}
    seq = kl.generate(m, prompt, max_new_tokens=N_NEW, draft_len=DRAFT, drafter=replay, stats=stats)
    print(kind, stats, "tokens equal to the plain run: %d / %d" % (int((seq == plain).sum()) - N_PROMPT, N_NEW))
    assert stats["accepted"] > 0
    assert stats["forwards"] < N_NEW
    assert stats["forwards"] == stats["rounds"] + 1 and stats["accepted"] <= stats["drafted"]
    _check_invariants(m, q, prompt, seq)


@pytest.mark.parametrize("kind", ["mha", "gqa"])
def test_always_wrong_drafts(kind):
    from kvquant_amd import llama as kl
    m, ids, q, _ = _model(kind)
    prompt, _ = _plain(kind)
    vocab = m.config.vocab_size

    def wrong(seq, k):
        return [(int(seq[-1]) + 1) % vocab] * k
    _reset(m, q)
    stats = {}
    seq = kl.generate(m, prompt, max_new_tokens=N_NEW, draft_len=DRAFT, drafter=wrong, stats=stats)
    print(kind, stats)
    assert stats["drafted"] > 0
    _check_invariants(m, q, prompt, seq)


@pytest.mark.parametrize("kind", ["mha", "gqa"])
def test_ngram_drafts_on_a_repetitive_prompt(kind):
    from kvquant_amd import llama as kl
    m, ids, q, _ = _model(kind)
    prompt = ids[:, :32].repeat(1, N_PROMPT // 32)
    _reset(m, q)
    stats = {}
    seq = kl.generate(m, prompt, max_new_tokens=N_NEW, draft_len=DRAFT, stats=stats)
    print(kind, stats)
    assert stats["drafted"] > 0 and stats["forwards"] == stats["rounds"] + 1
    _check_invariants(m, q, prompt, seq)


def test_sampling_is_refused():
    from kvquant_amd import llama as kl
    m, ids, q, _ = _model("mha")
    with pytest.raises(ValueError):
        kl.generate(m, ids[:, :8], max_new_tokens=4, draft_len=DRAFT, do_sample=True)
