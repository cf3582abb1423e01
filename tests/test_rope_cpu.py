"""Scaled RoPE (kvquant_amd.rope) without a GPU: the tables are transformers' own bit for bit, from both config styles,
RotaryDynamic forms the rows LlamaRotaryEmbedding forms, and the routes without a frequency table refuse scaled RoPE."""
import types

import pytest
import torch

transformers = pytest.importorskip("transformers")
from transformers import LlamaConfig  # noqa: E402
from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS  # noqa: E402
from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding  # noqa: E402

from kvquant_amd import rope as R  # noqa: E402
from kvquant_amd.attention import KVQuantAttention, RotaryDynamic  # noqa: E402

LLAMA31 = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
               original_max_position_embeddings=8192)
CASES = {
    # LLaMA-3.1-8B's real parameters
    "llama3": (5e5, LLAMA31, 131072),
    "linear": (1e4, dict(rope_type="linear", factor=4.0), 16384),
    "yarn": (1e6, dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=32768), 131072),
    "dynamic": (1e4, dict(rope_type="dynamic", factor=2.0), 4096),
}


def hf_config(name):
    theta, params, mpe = CASES[name]
    return LlamaConfig(hidden_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                       max_position_embeddings=mpe, rope_parameters=dict(params, rope_theta=theta))


def legacy_config(name):
    """a transformers 4.x style config: rope_theta + rope_scaling (the old key 'type')"""
    theta, params, mpe = CASES[name]
    old = {("type" if k == "rope_type" else k): v for k, v in params.items()}
    return types.SimpleNamespace(rope_theta=theta, rope_scaling=old, max_position_embeddings=mpe, head_dim=128)


def hf_table(name, seq_len=None):
    """transformers' table; dynamic: as LlamaRotaryEmbedding's dynamic update asks for it -- the init table up to
    max_position_embeddings, beyond it seq_len = max(position_ids) + 1, a tensor"""
    cfg = hf_config(name)
    if seq_len is None:
        return ROPE_INIT_FUNCTIONS[CASES[name][1]["rope_type"]](cfg, None)
    n = None if seq_len <= cfg.max_position_embeddings else torch.tensor(seq_len)
    return ROPE_INIT_FUNCTIONS["dynamic"](cfg, None, seq_len=n)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a, b))


@pytest.mark.parametrize("name", ["llama3", "linear", "yarn"])
@pytest.mark.parametrize("style", ["config", "legacy", "args"])
def test_fixed_tables_bit_identical(name, style):
    theta, params, mpe = CASES[name]
    if style == "config":
        spec = R.RopeSpec.from_config(hf_config(name))
    elif style == "legacy":
        spec = R.RopeSpec.from_config(legacy_config(name))
    else:
        spec = R.spec_of(theta, dict(params), mpe)
    assert spec.rope_type == name and not spec.is_default
    inv, af = spec.table()
    ref, ref_af = hf_table(name)
    assert same(inv, ref.float())
    assert af == float(ref_af)
    if name == "yarn":
        assert af != 1.0
    else:
        assert af == 1.0


def test_llama3_scales_long_wavelengths():
    """the llama3 rule divides every frequency whose wavelength exceeds 8192 / low_freq_factor by 8"""
    inv, _ = R.spec_of(5e5, dict(LLAMA31)).table()
    base = 1.0 / (5e5 ** (torch.arange(0, 128, 2, dtype=torch.int64).float() / 128))
    wl = 2 * torch.pi / base
    assert torch.equal(inv[wl < 8192 / 4.0], base[wl < 8192 / 4.0])
    assert torch.allclose(inv[wl > 8192], base[wl > 8192] / 8)


@pytest.mark.parametrize("style", ["config", "legacy"])
def test_dynamic_tables_bit_identical(style):
    spec = R.RopeSpec.from_config(hf_config("dynamic") if style == "config" else legacy_config("dynamic"))
    assert spec.dynamic
    prev = None
    for n in (1, 100, 4096, 4097, 8192, 3 * 4096 + 7, 100000):
        inv, af = spec.table(None, n)
        ref, ref_af = hf_table("dynamic", n)
        assert same(inv, ref.float()) and af == float(ref_af), n
        if n > 4096 and prev is not None:
            assert not torch.equal(inv, prev)     # past the original length the table moves with the length
        prev = inv
    # up to max_position_embeddings the table is the unscaled one
    assert torch.equal(spec.table(None, 10)[0], spec.table(None, 4096)[0])


def test_default_spec_has_no_table():
    for spec in (R.spec_of(1e4), R.spec_of(5e5, None), R.RopeSpec.from_config(LlamaConfig(head_dim=128))):
        assert spec.is_default and spec.table() is None


@pytest.mark.parametrize("name", ["llama3", "linear", "yarn", "dynamic"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_rotary_rows_match_llama_rotary_embedding(name, dtype):
    cfg = hf_config(name)
    spec = R.RopeSpec.from_config(cfg)
    ours = RotaryDynamic(128, base=CASES[name][0], rope=spec)
    RotaryDynamic.clear_cache()
    x = torch.zeros(1, 4, dtype=dtype)
    mpe = CASES[name][2]
    for start, end in ((0, 37), (5000, 5001), (mpe - 3, mpe + 9), (2 * mpe + 100, 2 * mpe + 101)):
        hf = LlamaRotaryEmbedding(cfg)        # (a fresh module: HF's dynamic update keeps state between calls)
        pos = torch.arange(start, end, dtype=torch.int64)[None]
        c_ref, s_ref = hf(x, pos)
        c, s = ours(x, start, end)
        assert same(c, c_ref[0]) and same(s, s_ref[0]), (name, start, end)


def test_rotary_default_unchanged():
    """a default spec keeps the theta rule's rows exactly"""
    a = RotaryDynamic(128, base=5e5)
    b = RotaryDynamic(128, base=5e5, rope=R.spec_of(5e5))
    x = torch.zeros(1, dtype=torch.float16)
    for se in ((0, 16), (100000, 100001)):
        ca, sa = a(x, *se)
        cb, sb = b(x, *se)
        assert torch.equal(ca, cb) and torch.equal(sa, sb)


@pytest.mark.parametrize("bad, what", [
    (dict(rope_type="longrope", factor=4.0, short_factor=[1.0] * 64, long_factor=[1.0] * 64), "longrope"),
    (dict(rope_type="proportional", factor=2.0), "proportional"),
    (dict(rope_type="nope", factor=2.0), "nope"),
    (dict(rope_type="linear", factor=2.0, partial_rotary_factor=0.5), "partial_rotary_factor"),
])
def test_unsupported_types_raise(bad, what):
    with pytest.raises(ValueError, match=what):
        R.spec_of(1e4, bad, 4096)


def test_unsupported_routes_raise():
    llama3 = dict(LLAMA31)
    with pytest.raises(ValueError, match="use_orig_sparse"):
        KVQuantAttention(hidden_size=1024, num_heads=8, abits=4, maxseqlen=64, device="cpu", make_proj=False,
                         use_orig_sparse=True, rope_theta=5e5, rope_scaling=llama3)
    with pytest.raises(ValueError, match="dynamic"):
        KVQuantAttention(hidden_size=1024, num_heads=8, abits=4, maxseqlen=64, device="cpu", make_proj=False,
                         first_few_fp16=4, rope_scaling=dict(rope_type="dynamic", factor=2.0), max_position_embeddings=64)
    from kvquant_amd import cache
    kc = types.SimpleNamespace(include_sparse=True, rope=R.spec_of(5e5, llama3))
    vc = types.SimpleNamespace(include_sparse=True)
    q = torch.zeros(8, 128)
    with pytest.raises(ValueError, match="shard_attention"):
        cache.shard_attention(kc, vc, q)
    with pytest.raises(ValueError, match="HeadShard"):
        cache.HeadShard(4, 1024, 8, (0, 4), 64, device="cpu", rope_theta=5e5, rope_scaling=llama3)


def test_rope_argument_checks():
    from kvquant_amd import ops
    inv = torch.ones(64)
    for af in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="attention factor"):
            ops._rope((inv, af), inv.device)
    with pytest.raises(ValueError, match="rope"):
        ops._rope((torch.ones(32), 1.0), inv.device)
    spec = R.spec_of(1e4, dict(rope_type="linear", factor=2.0))
    with pytest.raises(ValueError, match="finite"):
        spec.pin_table(torch.zeros(64), 1.0)


def test_patch_llama_takes_the_models_table():
    """rope_spec_of: a stock LlamaForCausalLM with llama3 rope_parameters -> its own rotary_emb table"""
    from transformers import LlamaForCausalLM
    from kvquant_amd.llama import rope_spec_of
    cfg = LlamaConfig(vocab_size=64, hidden_size=256, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=1, head_dim=128, max_position_embeddings=1024,
                      rope_parameters=dict(LLAMA31, rope_theta=5e5, original_max_position_embeddings=128))
    model = LlamaForCausalLM(cfg)
    spec = rope_spec_of(model)
    inv, af = spec.table()
    assert spec.rope_type == "llama3"
    assert torch.equal(inv, model.model.rotary_emb.inv_freq.float())
    assert af == model.model.rotary_emb.attention_scaling
    ref, _ = ROPE_INIT_FUNCTIONS["llama3"](cfg, None)
    assert torch.equal(inv, ref)
