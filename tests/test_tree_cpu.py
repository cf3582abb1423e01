"""Draft trees, the host-side pieces (no GPU): the prompt-lookup tree drafter, the acceptance walk, the cut that fits a
tree to a round, the depth / ancestor tables, and the library's argument checks that precede any launch."""
import ctypes

import pytest
import torch

from kvquant_amd import spec


# ---- ngram_tree_draft -------------------------------------------------------------------------------------------------
# the suffix 1 2 3 occurs three times before: most recent first followed by 4 7 1 2 3, by 9 8 1 2 3 .., by 4 5 1 2 3 ..
SEQ = [1, 2, 3, 4, 5, 1, 2, 3, 9, 8, 1, 2, 3, 4, 7, 1, 2, 3]


def _check_tree(tokens, parent):
    assert len(tokens) == len(parent)
    for i, p in enumerate(parent, start=1):
        assert 0 <= p < i                                   # topological: a parent is an earlier node (0: the root)
    kids = {}
    for i, (t, p) in enumerate(zip(tokens, parent), start=1):
        assert t not in kids.setdefault(p, set()), "two children of node %d carry token %d" % (p, t)
        kids[p].add(t)


def test_trie_merges_shared_prefixes():
    tokens, parent = spec.ngram_tree_draft(SEQ, 6, max_ngram=3, branches=4)
    # depth 1: 4 (candidates 0 and 2 share it), 9; depth 2: 7 under 4, 8 under 9, 5 under 4; depth 3: 1 under 7
    assert tokens == [4, 9, 7, 8, 5, 1]
    assert parent == [0, 0, 1, 2, 1, 3]
    _check_tree(tokens, parent)


def test_breadth_first_budget():
    full, fpar = spec.ngram_tree_draft(SEQ, 64, branches=4)
    for k in range(1, 12):
        tokens, parent = spec.ngram_tree_draft(SEQ, k, branches=4)
        _check_tree(tokens, parent)
        n = min(k, len(full))
        assert (tokens, parent) == (full[:n], fpar[:n])        # a smaller budget is a prefix of the breadth-first order
    # the budget is spent level by level: with 2 nodes only depth 1 exists, with 5 nothing of depth 3
    assert spec.ngram_tree_draft(SEQ, 2, branches=4) == ([4, 9], [0, 0])
    t5, p5 = spec.ngram_tree_draft(SEQ, 5, branches=4)
    assert (t5, p5) == ([4, 9, 7, 8, 5], [0, 0, 1, 2, 1])


def test_branches_limit_and_order():
    # two candidates: the two most recent occurrences, most recent first
    assert spec.ngram_tree_draft(SEQ, 4, branches=2) == ([4, 9, 7, 8], [0, 0, 1, 2])


def test_single_occurrence_is_ngram_draft():
    seq = [5, 6, 7, 8, 9, 10, 6, 7]
    want = spec.ngram_draft(seq, 4)
    assert want == [8, 9, 10, 6]
    assert spec.ngram_tree_draft(seq, 4) == (want, [0, 1, 2, 3])
    for k in (1, 3, 6, 31):
        chain = spec.ngram_draft(SEQ, k)
        assert spec.ngram_tree_draft(SEQ, k, branches=1) == (chain, list(range(len(chain))))
    g = torch.Generator().manual_seed(0)
    for _ in range(20):
        s = torch.randint(0, 6, (40,), generator=g)
        chain = spec.ngram_draft(s, 5)
        assert spec.ngram_tree_draft(s, 5, branches=1) == (chain, list(range(len(chain))))
        _check_tree(*spec.ngram_tree_draft(s, 9, branches=4))


def test_nothing_matches():
    assert spec.ngram_tree_draft([1, 2, 3, 4], 5) == ([], [])
    assert spec.ngram_tree_draft(SEQ, 0) == ([], [])
    assert spec.ngram_tree_draft([7], 3) == ([], [])


# ---- accept_tree ------------------------------------------------------------------------------------------------------
TOK, PAR = [4, 9, 7, 8, 5, 1], [0, 0, 1, 2, 1, 3]


def test_accept_empty_tree():
    assert spec.accept_tree([], [], [42]) == ([0], 42)


def test_accept_full_path():
    #            row: 0  1  2  3  4  5  6
    assert spec.accept_tree(TOK, PAR, [4, 7, 0, 1, 0, 0, 33]) == ([0, 1, 3, 6], 33)


def test_accept_stops_at_first_mismatch():
    assert spec.accept_tree(TOK, PAR, [4, 6, 0, 1, 0, 0, 33]) == ([0, 1], 6)      # row 1 wants 6: no such child
    assert spec.accept_tree(TOK, PAR, [3, 7, 0, 1, 0, 0, 33]) == ([0], 3)


def test_accept_sibling_choice():
    assert spec.accept_tree(TOK, PAR, [9, 0, 8, 0, 77, 0, 0]) == ([0, 2, 4], 77)  # the second child of the root
    assert spec.accept_tree(TOK, PAR, [4, 5, 0, 0, 0, 11, 0]) == ([0, 1, 5], 11)  # the second child of node 1


def test_accept_checks_lengths():
    with pytest.raises(ValueError):
        spec.accept_tree(TOK, PAR, [1, 2, 3])


def test_chain_acceptance_agrees_with_accept_draft():
    draft = [3, 1, 4, 1, 5]
    for rows in ([3, 1, 4, 1, 5, 9], [3, 1, 7, 1, 5, 9], [2, 1, 4, 1, 5, 9]):
        n, nxt = spec.accept_draft(draft, rows)
        assert spec.accept_tree(draft, list(range(5)), rows) == (list(range(n + 1)), nxt)


# ---- cut_tree ---------------------------------------------------------------------------------------------------------
def test_cut_tree():
    assert spec.cut_tree(TOK, PAR, 6, 3) == (TOK, PAR)
    assert spec.cut_tree(TOK, PAR, 4, 3) == ([4, 9, 7, 8], [0, 0, 1, 2])
    assert spec.cut_tree(TOK, PAR, 6, 2) == ([4, 9, 7, 8, 5], [0, 0, 1, 2, 1])   # node 6 (depth 3) leaves
    assert spec.cut_tree(TOK, PAR, 6, 1) == ([4, 9], [0, 0])
    # a node below a dropped node leaves with it, the others are renumbered
    assert spec.cut_tree([1, 2, 3, 4], [0, 1, 2, 0], 4, 2) == ([1, 2, 4], [0, 1, 0])
    with pytest.raises(ValueError):
        spec.cut_tree([1, 2], [0, 2], 2, 5)


# ---- depth and ancestor sets ------------------------------------------------------------------------------------------
def test_tree_tables_hand_written():
    from kvquant_amd import ops
    from tests import tree_check as tc
    #         0
    #       / | \
    #      1  2  5
    #     / \     \
    #    3   4     6
    parent = [0, 0, 0, 1, 1, 0, 5]
    depth, anc = ops.tree_tables(parent)
    assert depth == [0, 1, 1, 2, 2, 1, 2]
    assert anc == [0b1, 0b11, 0b101, 0b1011, 0b10011, 0b100001, 0b1100001]
    assert depth == tc.depths(parent)
    vis = tc.visible(parent)
    for i in range(7):
        assert [bool(anc[i] >> j & 1) for j in range(7)] == vis[i].tolist()
    assert sorted(tc.paths(parent)) == [[0, 1, 3], [0, 1, 4], [0, 2], [0, 5, 6]]
    # parent[0] is ignored; a chain
    assert ops.tree_tables([9, 0, 1, 2])[0] == [0, 1, 2, 3]
    for bad in ([0, 1], [0, 0, 2], [0, 0, 3], [0, -1]):
        with pytest.raises(ValueError):
            ops.tree_tables(bad)
    with pytest.raises(ValueError):
        ops.tree_tables([0] * 33)
    for name, S in (("star", 7), ("two", 7), ("two", 32), ("random", 32), ("chain", 2)):
        p = tc.SHAPES[name](S)
        d, a = ops.tree_tables(p)
        assert d == tc.depths(p) and len(p) == S
        assert all(a[i] < (1 << S) for i in range(S))           # no bit at or above S


# ---- the library's checks (before any launch: safe without a GPU) -----------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from kvquant_amd import build
    build.build()
    from kvquant_amd import _lib
    return _lib.lib()


def test_tree_workspace_shapes(lib):
    ws = lib.kvq_chunk_attention_tree_workspace_bytes
    assert lib.kvq_version() == 403
    assert ws(8, 2, 7, 60) > 0 and ws(16, 2, 32, 1000) > 0
    assert ws(2, 2, 7, 60) > 0                                  # G = 1 through the grouped body
    assert ws(8, 2, 33, 60) == 0 and ws(8, 2, 1, 60) == 0       # S > 32, S < 2
    assert ws(18, 2, 7, 60) == 0 and ws(7, 2, 7, 60) == 0       # G = 9, Hq no multiple of Hkv
    assert ws(8, 2, 7, -1) == 0
    # the grouped entry keeps its shapes
    assert lib.kvq_chunk_attention_grouped_workspace_bytes(2, 2, 7, 60) == 0
    assert lib.kvq_chunk_attention_grouped_workspace_bytes(8, 2, 1, 60) > 0


def test_tree_and_keep_einval_before_launch(lib):
    from kvquant_amd import _lib
    ly = _lib.Layer()
    ly.bits, ly.H, ly.hd, ly.thr_k, ly.max_len = 4, 2, 128, 21, 2048
    par = (ctypes.c_uint8 * 7)(0, 0, 1, 2, 3, 4, 5)
    # (a layer without buffers: every call ends at a check, whatever the tree)
    assert lib.kvq_chunk_attention_tree(ctypes.byref(ly), 8, 7, 60, None, 128, 1024, None, None, 0, None, None, 0, par,
                                        None) == -1
    assert lib.kvq_chunk_attention_tree(None, 8, 7, 60, None, 128, 1024, None, None, 0, None, None, 0, None, None) == -1
    keep = (ctypes.c_uint8 * 3)(0, 2, 5)
    assert lib.kvq_keep_columns(ctypes.byref(ly), 60, 7, keep, 3, None) == -1       # neither side has buffers
    assert lib.kvq_keep_columns(None, 60, 7, keep, 3, None) == -1
    assert lib.kvq_keep_columns(ctypes.byref(ly), 60, 7, None, 3, None) == -1
