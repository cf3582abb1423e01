"""Speculative decoding, host side (no GPU): the prompt-lookup drafter, the greedy acceptance rule, the grouped chunk
attention entry points and the shapes their workspace function takes."""
import pytest
import torch

from kvquant_amd import _lib
from kvquant_amd.spec import accept_draft, ngram_draft


def test_ngram_longest_match_wins():
    # the 1-gram "3" occurs last at index 8 (-> 9), the 3-gram "1 2 3" only at 0 (-> 4): the 3-gram decides
    seq = torch.tensor([1, 2, 3, 4, 5, 7, 2, 6, 3, 9, 1, 2, 3])
    assert ngram_draft(seq, 2) == [4, 5]
    assert ngram_draft(seq, 2, max_ngram=1) == [9, 1]
    # the 3-gram "8 2 3" never occurred, the 2-gram "2 3" did
    assert ngram_draft(torch.tensor([1, 2, 3, 4, 5, 8, 2, 3]), 3) == [4, 5, 8]


def test_ngram_most_recent_occurrence_wins():
    seq = torch.tensor([1, 2, 3, 10, 11, 1, 2, 3, 20, 21, 1, 2, 3])
    assert ngram_draft(seq, 2) == [20, 21]


def test_ngram_cut_at_k_and_at_the_end():
    seq = torch.tensor([5, 6, 7, 8, 9, 5, 6, 7])
    assert ngram_draft(seq, 1) == [8]
    assert ngram_draft(seq, 4) == [8, 9, 5, 6]
    assert ngram_draft(seq, 31) == [8, 9, 5, 6, 7]           # (everything behind the match, to the end)
    assert ngram_draft(torch.tensor([4, 4]), 5) == [4]        # (an occurrence may overlap the suffix)
    assert ngram_draft(seq, 0) == []


def test_ngram_no_match():
    assert ngram_draft(torch.tensor([1, 2, 3, 4]), 4) == []
    assert ngram_draft(torch.tensor([7]), 4) == []
    assert ngram_draft(torch.tensor([], dtype=torch.long), 4) == []


def test_ngram_is_pure():
    seq = torch.tensor([1, 2, 1, 2, 1])
    keep = seq.clone()
    assert ngram_draft(seq, 3) == ngram_draft(seq, 3) == [2, 1]
    assert torch.equal(seq, keep)


@pytest.mark.parametrize("draft,rows,want", [
    ([5, 6, 7], [9, 6, 7, 8], (0, 9)),           # none: the first row's own token
    ([5, 6, 7], [5, 6, 1, 8], (2, 1)),           # some: a later match (row 3) does not count
    ([5, 6, 7], [5, 6, 7, 8], (3, 8)),           # all: the bonus token
    ([], [4], (0, 4)),                           # empty draft: an ordinary decode step
])
def test_accept_draft(draft, rows, want):
    assert accept_draft(draft, rows) == want
    assert accept_draft(torch.tensor(draft, dtype=torch.long), torch.tensor(rows)) == want


def test_accept_draft_row_count():
    with pytest.raises(ValueError):
        accept_draft([1, 2], [1, 2])


def test_llama_exports_the_pure_functions():
    from kvquant_amd import llama
    assert llama.ngram_draft is ngram_draft and llama.accept_draft is accept_draft
    assert callable(llama.rollback)


def test_exported():
    lib = _lib.lib()
    for name in ("kvq_chunk_attention_grouped", "kvq_chunk_attention_grouped_rope",
                 "kvq_chunk_attention_grouped_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.kvq_version() == 403


def test_grouped_workspace_size():
    lib = _lib.lib()
    ws, ws_heads = lib.kvq_chunk_attention_grouped_workspace_bytes, lib.kvq_chunk_attention_workspace_bytes
    assert ws(8, 8, 8, 1000) == 0                 # G = 1
    assert ws(8, 2, 33, 1000) == 0                # S > 32
    assert ws(8, 2, 8, 1000) > 0
    assert ws(8, 2, 32, 1000) > 0 and ws(32, 8, 1, 131072) > 0
    # whatever the per-head plan refuses
    for bad in [(32, 7, 16, 100), (72, 8, 16, 100), (0, 8, 16, 100), (32, 8, 0, 100), (32, 8, 16, -1)]:
        assert ws(*bad) == 0 and ws_heads(*bad) == 0, bad
    # partials keep the layout [Hq][nsplit][S][...]: a whole number of (S x 128 + S x 2) float rows per head and split
    assert ws(32, 8, 16, 131072) >= 32 * 16 * (128 + 2) * 4


def test_grouped_einval_before_launch():
    """the grouped entry validates like kvq_chunk_attention: a refused call returns before anything is dereferenced"""
    import ctypes
    P = 4096
    ly = _lib.Layer(bits=4, H=2, hd=128, thr_k=3, max_len=1024, rope_theta=10000.0, pos_offset=0, kmat=P, klut=P,
                    klut_off=P, klo=P, khi=P, koutliers=P, kidx=P, koutliers_t=P, kidx_t=P, klut_ends=None,
                    klut_score=None, vmat=P, vlut_rows=P, vlut_sorted=P, voutliers=P, vidx=P, vnorm=None,
                    v_mix_rows=None, flags=0)
    f = _lib.lib().kvq_chunk_attention_grouped

    def call(Hq=8, S=8, c0=100, q=P, ws=P, wsb=1 << 30):
        return f(ctypes.byref(ly), Hq, S, c0, q, 1024, 128, None, None, 0, P, ws, wsb, None)
    assert call(Hq=2) == -1                       # G = 1
    assert call(S=33) == -1                       # S > 32
    assert call(q=None) == -1
    assert call(c0=1020) == -1                    # c0 + S > max_len
    assert call(ws=None) == -3 and call(wsb=16) == -3


# ---- rollback: plain torch slice fills, so the bookkeeping is checked here on CPU caches --------------------------------
def _caches(sinks=0, compact=False, norm=True, **kw):
    from kvquant_amd.cache import QuantK, QuantV
    args = dict(bits=4, hidden_size=256, num_heads=2, max_position_embeddings=32, include_sparse=True,
                first_few_fp16=sinks, device="cpu", compact=compact)
    kc, vc = QuantK(**args, **kw), QuantV(**args)
    if norm:
        vc.lookup_table2 = torch.zeros_like(vc.lookup_table)
    return kc, vc


def _column_arrays(kc, vc):
    """(tensor, axis of the column) of every array in which a compressed column owns storage"""
    arrs = [(kc.kcache, 2), (kc.outliers, 0), (kc.outlier_indices, 0), (kc.outliers_t, 1), (kc.outlier_indices_t, 1),
            (vc.vcache, 2), (vc.lookup_table, 0), (vc.lookup_table2, 0), (vc.outliers, 0), (vc.outlier_indices, 0)]
    return [(t, ax) for t, ax in arrs if t is not None]


@pytest.mark.parametrize("sinks,compact", [(0, False), (5, False), (0, True)])
def test_truncate_zeroes_exactly_the_dropped_columns(sinks, compact):
    kc, vc = _caches(sinks, compact)
    arrs = _column_arrays(kc, vc)
    assert len(arrs) == (6 if compact else 10)
    for t, _ in arrs:
        t.fill_(1)
    kc.klen = vc.vlen = sinks + 10                # compressed columns 0 .. 9
    kc.truncate(3)
    vc.truncate(3)
    assert kc.klen == vc.vlen == sinks + 7
    for t, ax in arrs:
        t = t.movedim(ax, 0)
        assert bool((t[:7] == 1).all()) and bool((t[7:10] == 0).all()) and bool((t[10:] == 1).all())
    kc.truncate(0)
    assert kc.klen == sinks + 7
    kc.truncate(7)
    vc.truncate(7)
    assert kc.klen == vc.vlen == sinks


def test_truncate_errors():
    kc, vc = _caches(sinks=5)
    kc.klen = vc.vlen = 8
    for c in (kc, vc):
        with pytest.raises(ValueError):
            c.truncate(4)                          # into the sink tokens
        with pytest.raises(ValueError):
            c.truncate(-1)
    assert kc.klen == vc.vlen == 8
    kc.klen = vc.vlen = 3                          # the sink cache is still filling
    with pytest.raises(ValueError):
        kc.truncate(1)
    ko, _ = _caches(use_orig_sparse=True)
    ko.klen = 4
    with pytest.raises(NotImplementedError):
        ko.truncate(1)


def test_attention_rollback():
    from kvquant_amd.attention import KVQuantAttention
    a = KVQuantAttention(hidden_size=512, num_heads=4, abits=4, first_few_fp16=5, maxseqlen=64, device="cpu",
                         make_proj=False)
    a.kcache.klen = a.vcache.vlen = 3
    with pytest.raises(ValueError):
        a.rollback(1)                              # still filling the sinks
    a.kcache.klen = a.vcache.vlen = 9
    with pytest.raises(ValueError):
        a.rollback(5)
    a.rollback(4)
    assert a.kcache.klen == a.vcache.vlen == 5
    a.kcache.klen = 7
    with pytest.raises(ValueError):
        a.rollback(1)                              # K and V out of step


def test_generate_refuses_sampling_and_bad_draft_len():
    from kvquant_amd import llama
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(ValueError):
        llama.generate(None, ids, draft_len=4, do_sample=True)
    with pytest.raises(ValueError):
        llama.generate(None, ids, draft_len=32)


# ---- the speculative loop of generate() around a fake model: next token = (7 * token + 3) % V, caches = a length ------
class _FakeModel:
    V = 50

    def __init__(self, sinks=0, maxseqlen=256):
        import types
        from kvquant_amd.attention import KVQuantAttention
        core = KVQuantAttention(hidden_size=256, num_heads=2, abits=4, first_few_fp16=sinks, maxseqlen=maxseqlen,
                                device="cpu", make_proj=False)
        attn = types.SimpleNamespace(kvq=core)
        self.model = types.SimpleNamespace(layers=[types.SimpleNamespace(self_attn=attn)])
        self.core, self.fed = core, []

    def parameters(self):
        return iter([torch.zeros(1)])

    def __call__(self, ids, use_cache=False):
        import types
        self.fed.append(ids.shape[1])
        self.core.kcache.klen += ids.shape[1]
        self.core.vcache.vlen += ids.shape[1]
        assert self.core.kcache.klen - self.core.first_few_fp16 <= self.core.kcache.max_len
        logits = torch.nn.functional.one_hot((ids * 7 + 3) % self.V, self.V).float()
        return types.SimpleNamespace(logits=logits)


def _truth(seq, k):
    out, t = [], int(seq[-1])
    for _ in range(k):
        t = (7 * t + 3) % _FakeModel.V
        out.append(t)
    return out


@pytest.mark.parametrize("drafter", ["truth", "wrong", "half", "ngram", "empty"])
@pytest.mark.parametrize("sinks", [0, 5])
def test_speculative_loop_equals_plain(drafter, sinks):
    from kvquant_amd import llama
    fn = {"truth": _truth, "wrong": lambda s, k: [(int(s[-1]) + 1) % 50] * k,
          "half": lambda s, k: _truth(s, k)[:k // 2] + [49] * (k - k // 2), "ngram": None,
          "empty": lambda s, k: []}[drafter]
    prompt = torch.tensor([[3, 1, 4]])
    plain_m = _FakeModel(sinks)
    plain = llama.generate(plain_m, prompt, max_new_tokens=40)
    m, stats = _FakeModel(sinks), {}
    seq = llama.generate(m, prompt, max_new_tokens=40, draft_len=7, drafter=fn, stats=stats)
    assert torch.equal(seq, plain)
    assert m.core.kcache.klen == m.core.vcache.vlen == plain_m.core.kcache.klen == 3 + 40 - 1
    assert stats["forwards"] == len(m.fed) == stats["rounds"] + 1
    assert stats["drafted"] == sum(m.fed[1:]) - stats["rounds"] and max(m.fed[1:]) <= 8
    if drafter == "truth":
        assert stats["accepted"] == stats["drafted"] and stats["forwards"] < 10
    if drafter in ("wrong", "empty"):
        assert stats["accepted"] == 0 and stats["forwards"] == 40
    if drafter == "half":
        assert 0 < stats["accepted"] < stats["drafted"]
    if sinks:
        assert m.fed[1] == 1                      # nothing is drafted while the sink cache fills (klen 3 < 5)


def test_speculative_loop_eos_min_length_and_cache_end():
    from kvquant_amd import llama
    prompt = torch.tensor([[3, 1, 4]])
    plain = llama.generate(_FakeModel(), prompt, max_new_tokens=40)
    eos = int(plain[0, 20])                        # the 18th new token
    for min_length in (0, 30):
        ref_m = _FakeModel()
        ref = llama.generate(ref_m, prompt, max_new_tokens=40, eos_token_id=eos, pad_token_id=0, min_length=min_length)
        m = _FakeModel()
        seq = llama.generate(m, prompt, max_new_tokens=40, eos_token_id=eos, pad_token_id=0, min_length=min_length,
                             draft_len=7, drafter=_truth)
        assert torch.equal(seq, ref)
        assert m.core.kcache.klen == ref_m.core.kcache.klen == seq.shape[1] - 1
    # a cache with room for 12 tokens: drafts are cut so that it is never passed (the fake model asserts it)
    m = _FakeModel(maxseqlen=12)
    seq = llama.generate(m, prompt, max_new_tokens=10, draft_len=7, drafter=_truth)
    assert seq.shape[1] == 13 and m.core.kcache.klen == 12
