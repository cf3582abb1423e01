"""Speculative decoding on the compressed cache, the host-side pieces: the default drafter (prompt lookup) and the
greedy acceptance rule.  Pure functions of token ids -- no GPU, no library call; kvquant_amd.llama.generate(draft_len=k)
feeds `[last token] + draft` through the model as one chunk (cache.chunk_kv: one pass over the packed cache for all
rows), keeps what accept_draft() accepts and rolls the rest back (KVQuantAttention.rollback).
Draft TREES (generate(draft_len=k, draft_branches=b >= 2)): ngram_tree_draft() merges the continuations of several
earlier occurrences of the suffix n-gram into a trie, the model verifies all of its nodes in one forward (tree mask and
per-node positions: kvq_chunk_attention_tree), accept_tree() walks the arg-max path and KVQuantAttention.keep_path()
keeps exactly that path in the caches."""
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


def ngram_tree_draft(seq, k, max_ngram=3, branches=4):
    """Prompt lookup with alternatives.  The suffix n-gram is chosen as in ngram_draft (n = max_ngram down to 1, the
    longest that occurs earlier wins); its up to `branches` most recent earlier occurrences, most recent first, are the
    candidates, and their continuations are merged into a trie: equal prefixes share nodes, the children of a node
    carry distinct tokens.  Nodes are added breadth-first -- depth 1 of every candidate, then depth 2, ... in candidate
    order -- until k draft nodes exist.  Returns (tokens, parent) for the draft nodes 1 .. m in topological order:
    tokens[i - 1] is node i's token, parent[i - 1] its parent node (0: the root, i.e. the last token of seq).  With one
    occurrence (or branches = 1) tokens is ngram_draft(seq, k, max_ngram) and parent the chain 0, 1, ..; ([], []) when
    nothing matches (or k <= 0)."""
    seq = torch.as_tensor(seq).reshape(-1)
    L = int(seq.numel())
    if k <= 0 or branches <= 0:
        return [], []
    for n in range(min(int(max_ngram), L - 1), 0, -1):
        hit = (seq.unfold(0, n, 1)[:L - n] == seq[L - n:]).all(dim=1).nonzero().reshape(-1)
        if not hit.numel():
            continue
        starts = [int(h) + n for h in hit.tolist()[::-1][:int(branches)]]
        conts = [seq[j:j + k].tolist() for j in starts]
        tokens, parent, children = [], [], {}          # children: (node, token) -> child node
        at = [0] * len(conts)                          # the trie node each candidate has reached
        for d in range(max(len(c) for c in conts)):
            for ci, c in enumerate(conts):
                if d >= len(c) or at[ci] < 0:
                    continue
                key = (at[ci], int(c[d]))
                if key not in children:
                    if len(tokens) >= k:
                        at[ci] = -1                    # out of budget: this candidate ends here
                        continue
                    tokens.append(int(c[d]))
                    parent.append(at[ci])
                    children[key] = len(tokens)
                at[ci] = children[key]
        return tokens, parent
    return [], []


def accept_tree(tokens, parent, row_argmax):
    """Greedy verification of a draft tree.  tokens / parent: the draft nodes 1 .. m (ngram_tree_draft); row_argmax: the
    arg-max of the m + 1 logit rows of the forward that fed [last token] + tokens under the tree mask (row i predicts
    the token after node i).  From the root, step to the child whose token equals the current row's arg-max until
    there is none.  Returns (keep, next_token): the rows of the path in ascending order, root included, and the arg-max
    of the last kept row -- the model's own token behind the path."""
    tokens = [int(t) for t in tokens]
    parent = [int(p) for p in parent]
    rows = [int(t) for t in row_argmax]
    if len(parent) != len(tokens) or len(rows) != len(tokens) + 1:
        raise ValueError("accept_tree: %d tokens, %d parents, %d rows (m, m, m + 1 expected)"
                         % (len(tokens), len(parent), len(rows)))
    keep, cur = [0], 0
    while True:
        nxt = next((i + 1 for i in range(cur, len(tokens)) if parent[i] == cur and tokens[i] == rows[cur]), None)
        if nxt is None:
            return keep, rows[cur]
        keep.append(nxt)
        cur = nxt


def cut_tree(tokens, parent, max_nodes, max_depth):
    """The draft nodes (tokens, parent) that fit a round: the first max_nodes of them (a prefix of a topological order is
    a tree) without those deeper than max_depth, renumbered.  ValueError for a parent that is no earlier node."""
    tokens, parent = list(tokens)[:max_nodes], list(parent)[:max_nodes]
    if len(tokens) != len(parent):
        raise ValueError("cut_tree: %d tokens, %d parents" % (len(tokens), len(parent)))
    depth, new_id, out_t, out_p = {0: 0}, {0: 0}, [], []
    for i, (tok, par) in enumerate(zip(tokens, parent), start=1):
        par = int(par)
        if not 0 <= par < i:
            raise ValueError("draft tree: parent %d of node %d is no earlier node" % (par, i))
        if par not in new_id or depth[par] + 1 > max_depth:
            continue                                   # too deep, or below a node that was
        depth[i] = depth[par] + 1
        new_id[i] = len(out_t) + 1
        out_t.append(int(tok))
        out_p.append(new_id[par])
    return out_t, out_p
