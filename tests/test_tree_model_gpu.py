"""generate(draft_len=k, draft_branches=b) on the trained stand-in models of tests/test_spec_model_gpu.py (MHA, and GQA
with 5 sink tokens): b = 1 is the chain loop; with an oracle tree whose FIRST branch is wrong and whose second is the
model's own continuation the second branch is what gets accepted; prompt-lookup trees on a prompt in which one n-gram
has two continuations; the caches end as plain generate() leaves them."""
import pytest
import torch

from tests import test_spec_model_gpu as tsm
from tests.test_chunk_model_gpu import _model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_PROMPT, N_NEW, DRAFT = tsm.N_PROMPT, tsm.N_NEW, tsm.DRAFT


@pytest.mark.parametrize("kind", ["mha", "gqa"])
def test_one_branch_is_the_chain_loop(kind):
    from kvquant_amd import llama as kl
    m, ids, q, _ = _model(kind)
    prompt, plain = tsm._plain(kind)

    def replay(seq, k):
        return plain[0, seq.numel():seq.numel() + k].tolist()
    runs = []
    for kw in ({}, dict(draft_branches=1)):
        tsm._reset(m, q)
        stats = {}
        runs.append((kl.generate(m, prompt, max_new_tokens=N_NEW, draft_len=DRAFT, drafter=replay, stats=stats, **kw),
                     stats))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert sorted(runs[1][1]) == ["accepted", "drafted", "forwards", "rounds"]


@pytest.mark.parametrize("kind", ["mha", "gqa"])
def test_oracle_tree_second_branch(kind):
    """every round: a wrong branch (the true tokens + 1 mod vocab) first, the true continuation second"""
    from kvquant_amd import llama as kl
    m, ids, q, _ = _model(kind)
    prompt, plain = tsm._plain(kind)
    vocab = m.config.vocab_size

    def true_branch(seq, k):
        return plain[0, seq.numel():seq.numel() + k].tolist()

    def wrong_branch(seq, k):
        return [(t + 1) % vocab for t in true_branch(seq, k)]

    def tree(seq, k):
        good = true_branch(seq, DRAFT)
        bad = [(t + 1) % vocab for t in good]
        n = len(good)
        return bad + good, list(range(n)) + [0] + list(range(n + 1, 2 * n))
    # the chain with the same true-branch length (tests/test_spec_model_gpu.py::test_perfect_drafts), and the chain that
    # is given only the first (wrong) branch
    tsm._reset(m, q)
    chain = {}
    kl.generate(m, prompt, max_new_tokens=N_NEW, draft_len=DRAFT, drafter=true_branch, stats=chain)
    tsm._reset(m, q)
    wrong = {}
    kl.generate(m, prompt, max_new_tokens=N_NEW, draft_len=DRAFT, drafter=wrong_branch, stats=wrong)
    tsm._reset(m, q)
    stats = {}
    seq = kl.generate(m, prompt, max_new_tokens=N_NEW, draft_len=2 * DRAFT, draft_branches=2, drafter=tree, stats=stats)
    print(kind, "tree", stats, "chain", chain, "wrong-branch chain", wrong,
          "tokens equal to the plain run: %d / %d" % (int((seq == plain).sum()) - N_PROMPT, N_NEW))
    assert wrong["drafted"] > 0 and wrong["accepted"] == 0
    assert stats["forwards"] == stats["rounds"] + 1 and stats["accepted"] <= stats["drafted"]
    assert stats["accepted"] > 0 and stats["forwards"] < N_NEW
    assert stats["accepted"] * chain["rounds"] == chain["accepted"] * stats["rounds"]      # accepted / rounds
    tsm._check_invariants(m, q, prompt, seq)


def _ambiguous_prompt(m, q, ids):
    """a repetitive prompt (z a t Y1.. z a t Y2.. five times, then a) in which the 3-gram (z, a, t) has two
    continuations, t being the token the model itself puts behind the prompt -- found by feeding the prompt (the
    stand-in is close to an order-1 Markov model: t depends on `a`, not on the t of the earlier blocks)"""
    a, z = int(ids[0, 15]), int(ids[0, 60])
    y1, y2 = ids[0, 16:30].tolist(), ids[0, 32:46].tolist()
    assert y1[0] != y2[0]
    t = int(ids[0, 61])
    for _ in range(4):
        prompt = torch.tensor([([a, t] + y1 + [z] + [a, t] + y2 + [z]) * 5 + [a]], device=DEV)
        tsm._reset(m, q)
        with torch.no_grad():
            nxt = int(m(prompt, use_cache=False).logits[0, -1].argmax())
        if nxt == t:
            return prompt, (y2[0], y1[0])
        t = nxt
    raise AssertionError("the stand-in model's token behind the prompt does not settle")


@pytest.mark.parametrize("kind", ["mha", "gqa"])
def test_prompt_lookup_trees(kind):
    """a repetitive prompt in which the suffix n-gram of the first round has two different continuations: the first tree
    branches at the root (most recent occurrence first)"""
    from kvquant_amd import llama as kl
    from kvquant_amd.spec import ngram_tree_draft
    m, ids, q, _ = _model(kind)
    prompt, first = _ambiguous_prompt(m, q, ids)
    seen = []

    def drafter(seq, k):
        t, p = ngram_tree_draft(seq, k, branches=2)
        seen.append((t, p))
        return t, p
    tsm._reset(m, q)
    stats = {}
    seq = kl.generate(m, prompt, max_new_tokens=N_NEW, draft_len=2 * DRAFT, draft_branches=2, drafter=drafter,
                      stats=stats)
    print(kind, stats)
    assert seen[0][1][:2] == [0, 0] and tuple(seen[0][0][:2]) == first, "the first tree does not branch: %r" % (seen[0],)
    assert stats["drafted"] > 0 and stats["forwards"] == stats["rounds"] + 1
    assert stats["accepted"] <= stats["drafted"]
    tsm._check_invariants(m, q, prompt, seq)                   # klen, zeros behind it, teacher-forced agreement
    # the default drafter of draft_branches = 2 is that drafter
    tsm._reset(m, q)
    stats2 = {}
    seq2 = kl.generate(m, prompt, max_new_tokens=N_NEW, draft_len=2 * DRAFT, draft_branches=2, stats=stats2)
    assert torch.equal(seq2, seq) and stats2 == stats


def test_refusals():
    from kvquant_amd import llama as kl
    from tests import ppl_harness as ph
    m, ids, q, _ = _model("mha")
    with pytest.raises(ValueError):
        kl.generate(m, ids[:, :8], max_new_tokens=4, draft_len=DRAFT, draft_branches=2, do_sample=True)
    with pytest.raises(ValueError):
        kl.generate(m, ids[:, :8], max_new_tokens=4, draft_branches=2)               # branches without draft_len
    c = ph.make_model(layers=1, vocab=256, hidden=256, heads=2, inter=256, device=DEV, maxseqlen=128, abits=4,
                      include_sparse=True)
    kl.patch_llama(c, compact=True)
    with pytest.raises(ValueError):
        kl.generate(c, ids[:, :8] % 256, max_new_tokens=4, draft_len=DRAFT, draft_branches=2)
    assert c.model.layers[0].self_attn.kvq.kcache.klen == 0
