"""Draft trees over the compressed cache (cache.chunk_kv(parent=...) / kvq_chunk_attention_tree): the fp64 statement of
the tree semantics and the tree shapes of the checks.  A chunk of S rows is a tree in topological order (row 0 the root,
parent[i] < i); row i sees the sink tokens, every compressed column < c0 and the columns c0 + j of itself and its
ancestors; column c0 + j is rotated at position sinks + c0 + depth[j].  Dequantisation comes from tests/chunk_check.py
(tests/rope_check.py with a frequency table), which rotate column c at sinks + c: the chunk's columns are turned back by
that angle and forward by the angle of their depth here, in fp64 with the same fl32 angles.  The mask is derived from
`parent` by walking up from every row -- no bit sets, nothing taken from the library.
Shared by tests/test_tree_attn_gpu.py and tools/tree_bench.py."""
import math
import random

import torch

from tests import chunk_check as cc
from tests import rope_check as rc

HD = 128


def depths(parent):
    """depth of every row by walking up to the root"""
    out = []
    for i in range(len(parent)):
        d, j = 0, i
        while j != 0:
            j = parent[j]
            d += 1
        out.append(d)
    return out


def visible(parent):
    """bool [S, S]: row i sees node j iff j is i or an ancestor of i"""
    S = len(parent)
    m = torch.zeros(S, S, dtype=torch.bool)
    for i in range(S):
        j = i
        m[i, j] = True
        while j != 0:
            j = parent[j]
            m[i, j] = True
    return m


def chain(S):
    return [0] + list(range(S - 1))


def star(S):
    """every draft node at depth 1"""
    return [0] * S


def two_branches(S):
    """two chains from the root: nodes 1 .. a and a + 1 .. S - 1, a = S // 2"""
    a = S // 2
    return [0] + [i - 1 for i in range(1, a + 1)] + [0 if i == a + 1 else i - 1 for i in range(a + 1, S)]


def random_tree(S, seed):
    r = random.Random(seed)
    return [0] + [r.randrange(i) for i in range(1, S)]


SHAPES = {"chain": chain, "star": star, "two": two_branches, "random": lambda S: random_tree(S, 1234 + S)}


def paths(parent):
    """the root-to-leaf paths of a tree, each a list of ascending rows"""
    S = len(parent)
    leaves = [i for i in range(S) if i not in parent[1:]]
    out = []
    for leaf in leaves:
        p, j = [leaf], leaf
        while j != 0:
            j = parent[j]
            p.append(j)
        out.append(p[::-1])
    return out


def reference(kc, vc, q, c0, parent, k_sink=None, v_sink=None, rope=None):
    """fp64 statement of the tree chunk: q fp16 [Hq, S, 128] (row i already rotated at sinks + c0 + depth[i]) over the
    caches whose columns c0 .. c0+S-1 hold the tree's nodes.  rope: None (the theta rule) or (inv_freq, attention
    factor).  Returns f64 [S, Hq, 128]."""
    from kvquant_amd import ops
    Hkv = kc.num_heads
    Hq, S, _ = q.shape
    assert len(parent) == S
    G = Hq // Hkv
    Lc = c0 + S
    if rope is None:
        kr, vh = cc.dequant(kc, vc, Lc)
        freq = ops.rope_freqs(kc.rope_theta, device=kc.device)
    else:
        kr, vh = rc.dequant(kc, vc, Lc, rope[0], rope[1])
        freq = rope[0].float()
    # the chunk's columns: back by the angle of their column, forward by the angle of their depth (fl32 angles)
    dev = kc.device
    sinks = kc.first_few_fp16
    col_pos = torch.arange(c0, Lc, device=dev, dtype=torch.float32) + sinks
    dep_pos = torch.tensor(depths(parent), device=dev, dtype=torch.float32) + (c0 + sinks)
    a_old = (freq[:, None] * col_pos[None, :]).double()
    a_new = (freq[:, None] * dep_pos[None, :]).double()
    lo, hi = kr[:, :64, c0:], kr[:, 64:, c0:]
    c, s = a_old.cos(), a_old.sin()
    lo0, hi0 = c * lo + s * hi, -s * lo + c * hi
    c, s = a_new.cos(), a_new.sin()
    kr = kr.clone()
    kr[:, :64, c0:] = c * lo0 - s * hi0
    kr[:, 64:, c0:] = s * lo0 + c * hi0
    mask = torch.ones(S, Lc, dtype=torch.bool, device=dev)
    mask[:, c0:] = visible(parent).to(dev)
    out = torch.empty(S, Hq, HD, dtype=torch.float64, device=dev)
    for h in range(Hq):
        hk = h // G
        qh = q[h].double()
        sc = ((qh @ kr[hk]) / math.sqrt(HD)).masked_fill(~mask, float("-inf"))
        vv = vh[hk].t()
        if k_sink is not None:
            sc = torch.cat(((qh @ k_sink[hk].double()) / math.sqrt(HD), sc), dim=1)
            vv = torch.cat((v_sink[hk].double(), vv), dim=0)
        out[:, h] = torch.softmax(sc, dim=-1) @ vv
    return out
