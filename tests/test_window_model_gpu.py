"""Sliding-window layers in a model (patch_llama(sliding_window=...)): a random-init 2-layer stand-in (hidden 256, two
query heads over one KV head, head_dim 128, fp16) with quantizers calibrated on seeded random ids.  (6) the receptive
field of two windowed layers, bit for bit; (7) a stream past the ring's capacity, plain and with chain drafts;
(8) the window read from a Mistral config."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOCAB, W, SLACK = 512, 40, 88

_QUANT = {}


def _config(cls, sinks=0, **extra):
    from kvquant_amd import llama as kl
    cfg = cls(vocab_size=VOCAB, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
              num_key_value_heads=1, head_dim=128, max_position_embeddings=4096, attention_bias=False,
              tie_word_embeddings=False, **extra)
    return kl.kvquant_config(cfg, maxseqlen=1024, abits=4, include_sparse=True, first_few_fp16=sinks)


def _fresh(cls, sinks=0, **extra):
    """the un-patched model (seeded: every instance has the same weights)"""
    torch.manual_seed(0)
    return cls(_config(cls.config_class, sinks, **extra)).half().to(DEV).eval()


def _quantizers():
    from transformers import LlamaForCausalLM
    from kvquant_amd import calibrate
    if "q" not in _QUANT:
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(0, VOCAB, (1, 512), generator=g).to(DEV)
        _QUANT["q"] = calibrate.calibrate_llama(_fresh(LlamaForCausalLM), ids, bits=4, include_sparse=True,
                                                sparsity_threshold=0.99)
    return _QUANT["q"]


def _model(sinks=0, cls=None, extra=None, **patch):
    from transformers import LlamaForCausalLM
    from kvquant_amd import llama as kl
    q = _quantizers()
    m = _fresh(cls or LlamaForCausalLM, sinks, **(extra or {}))
    kl.patch_llama(m, **patch)
    kl.load_quantizers(m, q, include_sparse=True, sparsity_threshold=0.99)
    return m


def _cores(m):
    return [layer.self_attn.kvq for layer in m.model.layers]


@torch.no_grad()
def _feed(m, ids):
    """a prefill of 40, one chunk (which the layers cut into pieces), the last 30 tokens one at a time"""
    n = ids.shape[1]
    outs = [m(ids[:, :40], use_cache=False).logits[0], m(ids[:, 40:n - 30], use_cache=False).logits[0]]
    outs += [m(ids[:, i:i + 1], use_cache=False).logits[0] for i in range(n - 30, n)]
    return torch.cat(outs)


# ---- 6. receptive field --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sinks", [0, 5])
def test_receptive_field_of_two_windowed_layers(sinks):
    from kvquant_amd import llama as kl
    m = _model(sinks, sliding_window=W, window_slack=SLACK)
    for core in _cores(m):
        assert core.sliding_window == W and core.kcache.max_len == core.vcache.max_len == 128
        assert core.kcache.window == core.vcache.window == W
    g = torch.Generator().manual_seed(2)
    A, B, X = (torch.randint(0, VOCAB, (1, n), generator=g).to(DEV) for n in (150, 150, 120))
    assert not bool((A == B).all())
    B[:, :sinks] = A[:, :sinks]
    logits = []
    for P in (A, B):
        kl.reset_caches(m)
        logits.append(_feed(m, torch.cat((P, X), dim=1))[150:])
        for core in _cores(m):
            assert core.kcache.klen == core.vcache.vlen == 270
    torch.cuda.synchronize()
    a, b = logits
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    first = 2 * (W - 1) + 1
    assert torch.equal(a[first:], b[first:])
    assert not torch.equal(a[0], b[0])


# ---- 7. streaming past the capacity -------------------------------------------------------------------------------
def test_generate_past_the_capacity():
    from kvquant_amd import llama as kl
    m = _model(5, sliding_window=W, window_slack=SLACK)
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, VOCAB, (1, 60), generator=g).to(DEV)
    seq = kl.generate(m, prompt, max_new_tokens=100)
    assert seq.shape[1] == 160 and torch.equal(seq[:, :60], prompt)
    for core in _cores(m):
        kc, vc = core.kcache, core.vcache
        assert kc.klen == vc.vlen == 159 > kc.max_len
        assert kc.kcache.shape[2] == vc.vcache.shape[2] == vc.lookup_table.shape[0] == kc.outliers.shape[0] == 128
    # chain drafts (always the same guess: nearly every round rolls back) on the windowed model
    kl.reset_caches(m)
    stats = {}
    spec = kl.generate(m, prompt, max_new_tokens=100, draft_len=4, drafter=lambda s, k: [int(s[-1])] * k, stats=stats)
    assert spec.shape[1] == 160 and torch.equal(spec[:, :60], prompt)
    assert stats["drafted"] > 0
    for core in _cores(m):
        assert core.kcache.klen == core.vcache.vlen == 159
    with pytest.raises(ValueError):
        kl.generate(m, prompt, max_new_tokens=4, draft_len=4, draft_branches=2)
    with pytest.raises(ValueError):
        kl.keep_path(m, 4, [0, 2])
    with kl.draft_tree(m, [0, 0, 1]):
        with pytest.raises(ValueError):
            m(prompt[:, :3], use_cache=False)


# ---- 8. config reading ---------------------------------------------------------------------------------------------
@torch.no_grad()
def test_window_read_from_a_mistral_config():
    from transformers import MistralForCausalLM
    from kvquant_amd.attention import window_capacity
    m = _model(cls=MistralForCausalLM, extra=dict(sliding_window=W))
    for core in _cores(m):
        assert core.sliding_window == W and core.kcache.window == W
        assert core.kcache.max_len == window_capacity(W, 256) == 320
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, VOCAB, (1, 100), generator=g).to(DEV)
    out = m(ids, use_cache=False).logits
    assert out.shape[1] == 100 and torch.isfinite(out).all()
    assert _cores(m)[0].kcache.klen == 100
    lin = _model(cls=MistralForCausalLM, extra=dict(sliding_window=W), sliding_window=0)
    for core in _cores(lin):
        assert core.sliding_window is None and core.kcache.window is None and core.kcache.max_len == 1024
    ref = lin(ids, use_cache=False).logits
    assert torch.isfinite(ref).all() and _cores(lin)[0].kcache.klen == 100
    assert not torch.equal(out[0, W:], ref[0, W:])          # (rows past the window see fewer keys)
