"""Speculative decoding on the compressed cache, the host-side pieces: the default drafter (prompt lookup) and the
greedy acceptance rule.  Pure functions of token ids -- no GPU, no library call; kvquant_amd.llama.generate(draft_len=k)
feeds `[last token] + draft` through the model as one chunk (cache.chunk_kv: one pass over the packed cache for all
rows), keeps what accept_draft() accepts and rolls the rest back (KVQuantAttention.rollback)."""
import torch

MAX_DRAFT = 31      # 1 + draft rows fit the 32-row block of kvq_chunk_attention_grouped


def ngram_draft(seq, k, max_ngram=3):
    """Prompt lookup: the most recent EARLIER occurrence of the last n tokens of `seq` (1-D tensor of token ids), for
    n = max_ngram down to 1 -- the longest n-gram that occurs wins -- and the up to k tokens that followed it there.
    Returns a list of ints, empty when nothing matches (or k <= 0)."""
    seq = torch.as_tensor(seq).reshape(-1)
    L = int(seq.numel())
    if k <= 0:
        return []
    for n in range(min(int(max_ngram), L - 1), 0, -1):
        # windows starting at 0 .. L-n-1: every occurrence that is followed by at least one token
        hit = (seq.unfold(0, n, 1)[:L - n] == seq[L - n:]).all(dim=1).nonzero()
        if hit.numel():
            j = int(hit[-1]) + n
            return seq[j:j + k].tolist()
    return []


def accept_draft(draft, row_argmax):
    """Greedy verification.  draft: the proposed token ids d_0 .. d_{m-1}; row_argmax: the arg-max of the m + 1 logit
    rows of the forward that fed [last token, d_0, .., d_{m-1}] (row i predicts the token after its i-th input).
    Accepts the longest prefix with d_i == row_argmax[i]; returns (n_accepted, next_token), next_token =
    row_argmax[n_accepted]: the model's own token after the accepted prefix."""
    draft = [int(t) for t in draft]
    rows = [int(t) for t in row_argmax]
    if len(rows) != len(draft) + 1:
        raise ValueError("accept_draft: %d draft tokens need %d rows, got %d" % (len(draft), len(draft) + 1, len(rows)))
    n = 0
    while n < len(draft) and draft[n] == rows[n]:
        n += 1
    return n, rows[n]
