"""Draft trees on the compressed cache: kvq_chunk_attention_tree (tree mask and per-node positions on the grouped
kernel) against the fp64 statement of tests/tree_check.py, the chain through the tree entry against the grouped kernel
bit for bit, root-to-leaf paths against chain chunks on twin caches, and kvq_keep_columns (the accepted path moves into
contiguous columns) against twin caches that took only the kept tokens, bit for bit."""
import ctypes

import pytest
import torch

from tests import chunk_check as cc
from tests import rope_check as rc
from tests import test_spec_attn_gpu as tsa
from tests import tree_check as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HKV, MAX_LEN = 2, 2048

# (bits, norm, sinks, G, S, L0 = compressed tokens cached before the chunk, tree shape): every value of bits 2 / 3 / 4,
# Q-Norm on / off, sinks 0 / 5, G 1 / 2 / 4 / 8, S 2 / 7 / 32, L0 60 / 1000 and the three shapes occurs.  L0 = 60 with
# S = 7 crosses a 64-column tile with a ragged last tile (the chunk's columns lie in two tiles); L0 = 1000 is 16 tiles
# in several splits; L0 = 60 with S = 32 puts the chunk behind a tile that only holds four of the cached columns
CASES = [
    (4, False, 0, 2, 7, 60, "two"),
    (4, False, 5, 4, 32, 1000, "random"),
    (4, True, 0, 8, 2, 60, "star"),
    (3, False, 5, 8, 7, 60, "random"),
    (3, True, 0, 1, 32, 1000, "two"),
    (2, True, 5, 8, 32, 1000, "star"),
    (2, False, 0, 2, 7, 1000, "star"),
    (2, False, 5, 1, 2, 60, "star"),
    (4, False, 0, 4, 32, 60, "random"),
]


def _setup(bits, norm, sinks, G, S, L0, seed=0):
    kc, vc, scale, shift = cc.make_caches(bits, HKV, MAX_LEN, sinks=sinks, norm=norm, device=DEV, seed=seed)
    kp, vp = cc.tokens(L0 + S, HKV, scale, shift, DEV, seed=seed + 11)
    cc.fill(kc, vc, kp[:, :, :L0], vp[:, :, :L0])
    ks, vs = cc.sink_caches(HKV, sinks, DEV, seed + 12) if sinks else (None, None)
    q = cc.queries(HKV * G, S, DEV, seed + 13)
    return kc, vc, q, ks, vs, kp[:, :, L0:].contiguous(), vp[:, :, L0:].contiguous()


def _run(bits, norm, sinks, G, S, L0, shape, seed=0):
    from kvquant_amd.cache import chunk_kv
    kc, vc, q, ks, vs, k, v = _setup(bits, norm, sinks, G, S, L0, seed)
    parent = tc.SHAPES[shape](S)
    out = chunk_kv(kc, vc, q, k, v, k_sink=ks, v_sink=vs, parent=parent)
    torch.cuda.synchronize()
    return kc, vc, q, ks, vs, parent, out


def _what(bits, norm, sinks, G, S, L0, shape):
    return "nuq%d%s sinks=%d %d/%d L0=%d S=%d %s" % (bits, " norm" if norm else "", sinks, HKV * G, HKV, L0, S, shape)


@pytest.mark.parametrize("bits,norm,sinks,G,S,L0,shape", CASES)
def test_tree_vs_fp64(bits, norm, sinks, G, S, L0, shape):
    kc, vc, q, ks, vs, parent, out = _run(bits, norm, sinks, G, S, L0, shape)
    assert out.shape == (S, HKV * G, 128) and torch.isfinite(out).all()
    assert kc.klen == vc.vlen == sinks + L0 + S
    cc.check(out, tc.reference(kc, vc, q, L0, parent, ks, vs), "tree " + _what(bits, norm, sinks, G, S, L0, shape))


def test_statement_of_a_chain_is_the_chunk_statement():
    """tests/tree_check.py turns the chunk's columns back and forward again: for a chain that is the identity"""
    kc, vc, q, ks, vs, parent, out = _run(4, False, 5, 2, 7, 60, "chain")
    a, b = tc.reference(kc, vc, q, 60, parent, ks, vs), cc.reference(kc, vc, q, 60, ks, vs)
    assert float((a - b).abs().max()) < 1e-9 * float(b.abs().max())


def test_the_tree_matters():
    """the chain statement of the same inputs is far from the tree's output (mask and positions both differ)"""
    case = CASES[1]
    kc, vc, q, ks, vs, parent, out = _run(*case)
    L0 = case[5]
    cc.check(out, tc.reference(kc, vc, q, L0, parent, ks, vs), "tree " + _what(*case))
    d = float((out.double() - cc.reference(kc, vc, q, L0, ks, vs)).abs().max())
    print("tree output against the chain statement: %.2e of the largest output" % (d / float(out.abs().max())))
    assert d > 1e-3 * float(out.abs().max())


def test_tree_scaled_rope_vs_fp64():
    """llama3 frequencies (kvquant_amd.rope) through the _rope twin, star and random trees"""
    from kvquant_amd.cache import chunk_kv
    bits, G, L0, S = 4, 4, 1000, 7
    for shape in ("star", "random"):
        kc, vc, k, v, ks, vs = rc.make(bits, HKV, L0, S, "llama3", device=DEV)
        parent = tc.SHAPES[shape](S)
        q = cc.queries(HKV * G, S, DEV, 13)
        out = chunk_kv(kc, vc, q, k, v, parent=parent)
        torch.cuda.synchronize()
        inv, af = kc.rope_table(L0 + S)
        cc.check(out, tc.reference(kc, vc, q, L0, parent, rope=(inv, af)), "tree llama3 %s" % shape)
        # (the table matters: the theta rule's statement is far from this output)
        assert float((out.double() - tc.reference(kc, vc, q, L0, parent)).abs().max()) > 1e-3 * float(out.abs().max())


@pytest.mark.parametrize("bits,norm,sinks,G,S,L0", [(4, False, 5, 2, 7, 60), (2, True, 5, 8, 32, 1000),
                                                     (3, False, 0, 4, 2, 1000)])
def test_chain_through_the_tree_entry_is_the_grouped_kernel(bits, norm, sinks, G, S, L0):
    from kvquant_amd import ops
    from kvquant_amd.cache import chunk_kv, layer_struct
    kc, vc, q, ks, vs, k, v = _setup(bits, norm, sinks, G, S, L0)
    assert ops.chunk_attention_route(HKV * G, HKV, S) == "grouped"
    grouped = chunk_kv(kc, vc, q, k, v, k_sink=ks, v_sink=vs)
    tree = ops.chunk_attention_tree(layer_struct(kc, vc), HKV * G, L0, q, tc.chain(S), k_sink=ks, v_sink=vs)
    torch.cuda.synchronize()
    assert torch.equal(tree, grouped)


def test_chain_through_the_tree_entry_scaled_rope():
    from kvquant_amd import ops
    from kvquant_amd.cache import chunk_kv, layer_struct
    bits, G, L0, S = 4, 4, 1000, 7
    kc, vc, k, v, ks, vs = rc.make(bits, HKV, L0, S, "llama3", device=DEV)
    q = cc.queries(HKV * G, S, DEV, 13)
    grouped = chunk_kv(kc, vc, q, k, v)
    tree = ops.chunk_attention_tree(layer_struct(kc, vc), HKV * G, L0, q, tc.chain(S), rope=kc.rope_table(L0 + S))
    torch.cuda.synchronize()
    assert torch.equal(tree, grouped)


def test_tree_deterministic():
    a = _run(*CASES[1])[6]
    b = _run(*CASES[1])[6]
    assert torch.equal(a, b)


@pytest.mark.parametrize("sinks,L0", [(0, 60), (5, 1000)])
def test_paths_against_chain_chunks(sinks, L0):
    """every root-to-leaf path of a two-branch tree: its rows agree with a chain chunk of only that path's tokens on a
    twin cache (the bars of the fp64 comparison, not bitwise: the columns sit at other places in the tile)"""
    from kvquant_amd.cache import chunk_kv
    bits, G, S = 4, 4, 7
    kc, vc, q, ks, vs, k, v = _setup(bits, False, sinks, G, S, L0)
    parent = tc.two_branches(S)
    out = chunk_kv(kc, vc, q, k, v, k_sink=ks, v_sink=vs, parent=parent)
    paths = tc.paths(parent)
    assert paths == [[0, 1, 2, 3], [0, 4, 5, 6]]
    for path in paths:
        kc2, vc2, _, _, _, _, _ = _setup(bits, False, sinks, G, S, L0)
        chain = chunk_kv(kc2, vc2, q[:, path].contiguous(), k[:, :, path].contiguous(), v[:, :, path].contiguous(),
                         k_sink=ks, v_sink=vs)
        torch.cuda.synchronize()
        cc.check(out[path], chain.double(), "path %s against its chain chunk, sinks=%d L0=%d" % (path, sinks, L0))


# ---- keep_columns -----------------------------------------------------------------------------------------------------
def _twins(sinks, S, keep, L0=1000, bits=2, norm=True):
    """A: S nodes packed, `keep` kept; B: only the kept tokens packed.  (2 bit + Q-Norm: lookup_table2 is live)"""
    kc, vc, scale, shift = cc.make_caches(bits, HKV, MAX_LEN, sinks=sinks, norm=norm, device=DEV)
    kp, vp = cc.tokens(L0 + S + 1, HKV, scale, shift, DEV, seed=11)
    cc.fill(kc, vc, kp[:, :, :L0], vp[:, :, :L0])
    kc.parallel_pack(kp[:, :, L0:L0 + S].contiguous())
    vc.parallel_pack(vp[:, :, L0:L0 + S].contiguous())
    kb, vb, _, _ = cc.make_caches(bits, HKV, MAX_LEN, sinks=sinks, norm=norm, device=DEV)
    cc.fill(kb, vb, kp[:, :, :L0], vp[:, :, :L0])
    cols = [L0 + j for j in keep]
    kb.parallel_pack(kp[:, :, cols].contiguous())
    vb.parallel_pack(vp[:, :, cols].contiguous())
    return (kc, vc), (kb, vb), kp[:, :, L0 + S], vp[:, :, L0 + S]


def _assert_zero_behind(kc, vc):
    n = kc.klen - kc.first_few_fp16
    for t in (kc.kcache[:, :, n:], kc.outliers[n:], kc.outlier_indices[n:], kc.outliers_t[:, n:],
              kc.outlier_indices_t[:, n:], vc.vcache[:, :, n:], vc.lookup_table[n:], vc.lookup_table2[n:],
              vc.outliers[n:], vc.outlier_indices[n:]):
        assert not t.any()


KEEPS = [(7, [0, 2, 3, 6]), (7, [0]), (7, list(range(7))), (7, [0, 6]), (32, [0, 3, 4, 9, 17, 18, 31]), (32, [0]),
         (32, list(range(32))), (32, [0] + list(range(16, 32)))]


@pytest.mark.parametrize("sinks", [0, 5])
@pytest.mark.parametrize("S,keep", KEEPS)
def test_keep_columns_exact(sinks, S, keep):
    from kvquant_amd.cache import decode_kv, keep_kv
    G, L0 = 4, 1000
    (kc, vc), (kb, vb), k1, v1 = _twins(sinks, S, keep)
    keep_kv(kc, vc, S, keep)                                   # one launch for K and V
    torch.cuda.synchronize()
    assert kc.klen == vc.vlen == sinks + L0 + len(keep)
    tsa._assert_same_state((kc, vc), (kb, vb))
    _assert_zero_behind(kc, vc)
    # a decode step on both twins
    ks, vs = cc.sink_caches(HKV, sinks, DEV, 12) if sinks else (None, None)
    q = cc.queries(HKV * G, 1, DEV, 15)[:, 0].contiguous()
    outs = [decode_kv(a, b, q, k1.reshape(-1).contiguous(), v1.reshape(-1).contiguous(), k_sink=ks, v_sink=vs)[0]
            for a, b in ((kc, vc), (kb, vb))]
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    tsa._assert_same_state((kc, vc), (kb, vb))


@pytest.mark.parametrize("S,keep", [(7, [0, 2, 3, 6]), (32, [0, 3, 4, 9, 17, 18, 31])])
def test_keep_columns_per_cache(S, keep):
    """QuantK.keep_columns / QuantV.keep_columns: one side each"""
    (kc, vc), (kb, vb), _, _ = _twins(5, S, keep)
    kc.keep_columns(S, keep)
    assert kc.klen == 5 + 1000 + len(keep) and vc.vlen == 5 + 1000 + S
    vc.keep_columns(S, keep)
    torch.cuda.synchronize()
    tsa._assert_same_state((kc, vc), (kb, vb))
    _assert_zero_behind(kc, vc)


@pytest.mark.parametrize("S,n", [(7, 3), (32, 1), (32, 20), (7, 7)])
def test_keep_of_a_prefix_is_truncate(S, n):
    from kvquant_amd.cache import keep_kv
    (kc, vc), (kb, vb), _, _ = _twins(5, S, list(range(S)))
    keep_kv(kc, vc, S, list(range(n)))
    kb.truncate(S - n)
    vb.truncate(S - n)
    torch.cuda.synchronize()
    tsa._assert_same_state((kc, vc), (kb, vb))


def test_attention_layer_keep_path_after_a_tree_chunk():
    """KVQuantAttention: a tree chunk under the tree spec, keep_path, then the twin that took only the path"""
    from kvquant_amd.attention import KVQuantAttention
    from tests import decode_check
    H, Hkv, S = 8, 2, 7
    parent = tc.two_branches(S)
    path = [0, 4, 5, 6]
    quant, scale, shift = decode_check.quantizer(4, seed=4, C=Hkv * 128)
    g = torch.Generator(device=DEV).manual_seed(3)
    x = lambda *shape: (torch.randn(*shape, generator=g, device=DEV) * 0.5).half()   # noqa: E731
    q0, k0, v0 = x(1, H, 40, 128), x(1, Hkv, 40, 128), x(1, Hkv, 40, 128)
    q1, k1, v1 = x(1, H, S, 128), x(1, Hkv, S, 128), x(1, Hkv, S, 128)
    cores, outs = [], []
    for tree in (True, False):
        core = KVQuantAttention(hidden_size=H * 128, num_heads=H, abits=4, include_sparse=True, first_few_fp16=5,
                                maxseqlen=256, device=DEV, make_proj=False, num_key_value_heads=Hkv)
        core.load_quantizers(quant, quant, include_sparse=True, sparsity_threshold=0.99)
        core.attend(q0, k0, v0)
        if tree:
            core.tree = parent
            out = core.attend(q1, k1, v1)
            with pytest.raises(ValueError):
                core.attend(q1[:, :, :5], k1[:, :, :5], v1[:, :, :5])            # row count differs from the spec's
            core.tree = None
            assert core.kcache.klen == 40 + S
            core.keep_path(S, path)
            outs.append(out[:, path])
        else:
            # the chain chunk of the path's tokens: positions 40 .. 43 are the path's depths
            outs.append(core.attend(q1[:, :, path], k1[:, :, path], v1[:, :, path]))
        cores.append(core)
    torch.cuda.synchronize()
    assert cores[0].kcache.klen == cores[1].kcache.klen == 40 + len(path)
    tsa._assert_same_state((cores[0].kcache, cores[0].vcache), (cores[1].kcache, cores[1].vcache))
    # (fp16 outputs of [1, rows, hidden]: rows of the tree chunk against the chain chunk, the bars of the fp64 comparison)
    cc.check(outs[0].float().reshape(len(path), H, 128), outs[1].double().reshape(len(path), H, 128),
             "attention layer: tree rows of a path against its chain chunk")


# ---- argument errors: KVQ_EINVAL or ValueError, caches unchanged ------------------------------------------------------
def _snapshot(kc, vc):
    return [None if getattr(c, n) is None else getattr(c, n).clone()
            for c, names in ((kc, tsa.K_ARRAYS), (vc, tsa.V_ARRAYS)) for n in names] + [kc.klen, vc.vlen]


def _assert_unchanged(kc, vc, snap):
    now = _snapshot(kc, vc)
    assert now[-2:] == snap[-2:]
    for a, b in zip(now[:-2], snap[:-2]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))


def test_argument_errors_leave_the_caches_alone():
    from kvquant_amd import _lib, ops
    from kvquant_amd.cache import chunk_kv, keep_kv, layer_struct
    kc, vc, q, ks, vs, k, v = _setup(4, False, 0, 4, 7, 60)
    snap = _snapshot(kc, vc)
    with pytest.raises(ValueError):
        chunk_kv(kc, vc, q, k, v, parent=[0, 0, 1, 3, 2, 1, 0])               # parent[3] >= 3
    with pytest.raises(ValueError):
        chunk_kv(kc, vc, q, k, v, parent=[0, 0, 1])                           # 7 rows, 3 entries
    kq, kk, kv_ = cc.queries(HKV * 4, 33, DEV, 3), torch.cat([k] * 5, dim=2)[:, :, :33], torch.cat([v] * 5, dim=2)[:, :, :33]
    with pytest.raises(ValueError):
        chunk_kv(kc, vc, kq, kk.contiguous(), kv_.contiguous(), parent=[0] * 33)       # S = 33
    # the library itself: KVQ_EINVAL before any launch
    lib, layer = _lib.lib(), layer_struct(kc, vc)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.empty(33, HKV * 4, 128, device=DEV)

    def tree_call(S, parent):
        arr = (ctypes.c_uint8 * len(parent))(*parent)
        return lib.kvq_chunk_attention_tree(ctypes.byref(layer), HKV * 4, S, 60, kq.data_ptr(), kq.stride(0), kq.stride(1),
                                            None, None, 0, out.data_ptr(), ws.data_ptr(), ws.numel(), arr, None)
    assert tree_call(7, [0, 0, 1, 3, 2, 1, 0]) == -1
    assert tree_call(7, [0, 1, 1, 1, 1, 1, 1]) == -1                          # parent[1] = 1
    assert tree_call(33, [0] * 33) == -1
    assert tree_call(1, [0]) == -1
    assert lib.kvq_chunk_attention_tree_workspace_bytes(HKV * 4, HKV, 33, 60) == 0
    _assert_unchanged(kc, vc, snap)
    # keep: not ascending, keep[0] != 0, out of range, S beyond the cached tokens
    kc.parallel_pack(k)
    vc.parallel_pack(v)
    snap = _snapshot(kc, vc)
    for S, keep in ((7, [0, 3, 2]), (7, [0, 2, 2]), (7, [1, 2]), (7, []), (7, [0, 7]), (33, [0, 1]), (68, [0, 1])):
        for fn in (lambda: keep_kv(kc, vc, S, keep), lambda: kc.keep_columns(S, keep), lambda: vc.keep_columns(S, keep)):
            with pytest.raises(ValueError):
                fn()

    def keep_call(S, keep):
        arr = (ctypes.c_uint8 * max(len(keep), 1))(*keep)
        return lib.kvq_keep_columns(ctypes.byref(layer), 60, S, arr, len(keep), None)
    assert keep_call(7, [0, 3, 2]) == -1 and keep_call(7, [1, 2]) == -1 and keep_call(7, [0, 7]) == -1
    assert keep_call(33, [0, 1]) == -1 and keep_call(7, []) == -1
    assert lib.kvq_keep_columns(ctypes.byref(layer), MAX_LEN - 3, 7, (ctypes.c_uint8 * 2)(0, 1), 2, None) == -1
    torch.cuda.synchronize()
    _assert_unchanged(kc, vc, snap)


def test_compact_caches_are_refused():
    from kvquant_amd import _lib, ops
    from kvquant_amd.cache import QuantK, QuantV, chunk_kv, keep_kv, layer_struct
    from tests import decode_check
    C = HKV * 128
    quant, scale, shift = decode_check.quantizer(4, seed=4, C=C)
    kw = dict(bits=4, hidden_size=C, num_heads=HKV, max_position_embeddings=256, include_sparse=True,
              sparsity_threshold=0.99, device=DEV, compact=True)
    kc, vc = QuantK(rope_theta=10000.0, **kw), QuantV(**kw)
    kc.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99)
    vc.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99)
    kp, vp = cc.tokens(40, HKV, scale.to(DEV), shift.to(DEV), DEV, seed=11)
    cc.fill(kc, vc, kp, vp)
    before = (kc.kcache.clone(), kc.outlier_indices_t.clone(), vc.vcache.clone(), vc.outlier_indices.clone())
    for fn in (lambda: keep_kv(kc, vc, 7, [0, 2]), lambda: kc.keep_columns(7, [0, 2]), lambda: vc.keep_columns(7, [0, 2])):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(ValueError):
        chunk_kv(kc, vc, cc.queries(HKV * 4, 7, DEV, 1), kp[:, :, :7].contiguous(), vp[:, :, :7].contiguous(),
                 parent=tc.star(7))
    with pytest.raises(_lib.KvqError):                      # the library: KVQ_EINVAL, a compact cache has no value arrays
        ops.keep_columns(layer_struct(kc, vc), 33, 7, [0, 2], kc.device)
    torch.cuda.synchronize()
    assert kc.klen == vc.vlen == 40
    for a, b in zip(before, (kc.kcache, kc.outlier_indices_t, vc.vcache, vc.outlier_indices)):
        assert torch.equal(a, b)
