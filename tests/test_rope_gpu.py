"""Scaled RoPE on the GPU (tests/rope_check.py): every K rotation reachable from KVQuantAttention -- the MHA decode step
(one call and the multi-call route), the dense q.K^T, the GQA decode step and chunk attention (MHA and GQA) -- against
the fp64 statement with llama3 / YaRN tables; an explicit theta table with attention factor 1 gives the NULL path's
bits on every route; a dynamic table moves between two steps past the original length."""
import pytest
import torch

from tests import chunk_check as cc
from tests import rope_check as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _table(kc, L):
    t = kc.rope_table(L)
    assert t is not None
    return t


# (bits, sinks, Hkv, G, L, kind): L = compressed + sink tokens after the step's append
DECODE = [
    (4, 0, 32, 1, 4096, "llama3"),
    (3, 5, 32, 1, 4096, "yarn"),
    (4, 0, 32, 1, 32768, "yarn"),
    (3, 5, 32, 1, 131072, "llama3"),
    (4, 0, 8, 1, 1 << 20, "yarn"),
    (4, 0, 8, 4, 4096, "llama3"),
    (3, 0, 8, 4, 32768, "yarn"),
    (4, 0, 8, 4, 131072, "llama3"),
]


@pytest.mark.parametrize("bits,sinks,Hkv,G,L,kind", DECODE)
def test_decode_step_vs_fp64(bits, sinks, Hkv, G, L, kind):
    kc, vc, k, v, ks, vs = rc.make(bits, Hkv, L - 1, 1, kind, sinks=sinks, device=DEV)
    q = cc.queries(Hkv * G, 1, DEV, 13)[:, 0].contiguous()
    inv, af = _table(kc, kc.klen + 1)
    out = rc.decode_step(kc, vc, q, k, v, ks, vs)
    torch.cuda.synchronize()
    heads = None if L <= 32768 else [0, 5, Hkv * G - 1]
    ref = rc.decode_reference(kc, vc, q, L - sinks, inv, af, ks, vs, heads=heads)
    got = out if heads is None else out[heads]
    rc.check_decode(got, ref, "decode nuq%d sinks=%d %d/%d L=%d %s" % (bits, sinks, Hkv * G, Hkv, L, kind))
    if kind == "yarn":   # the attention factor is applied once to the compressed keys: without it the bar fails
        ref1 = rc.decode_reference(kc, vc, q, L - sinks, inv, 1.0, ks, vs, heads=heads)
        assert float((got.double() - ref1).abs().max() / ref1.abs().max()) > 1e-3
    # the theta rule is not what the table says (the test fails with the table ignored)
    from kvquant_amd import ops
    ref0 = rc.decode_reference(kc, vc, q, L - sinks, ops.rope_freqs(kc.rope.rope_theta, DEV), 1.0, ks, vs, heads=heads)
    assert float((got.double() - ref0).abs().max() / ref0.abs().max()) > 1e-3


# (bits, sinks, Hkv, G, L0, S, kind)
CHUNK = [
    (4, 0, 8, 1, 4096, 64, "llama3"),
    (3, 5, 8, 4, 32768, 100, "yarn"),
    (4, 0, 8, 4, 131072, 256, "llama3"),
]


@pytest.mark.parametrize("bits,sinks,Hkv,G,L0,S,kind", CHUNK)
def test_chunk_vs_fp64(bits, sinks, Hkv, G, L0, S, kind):
    from kvquant_amd.cache import chunk_kv
    kc, vc, k, v, ks, vs = rc.make(bits, Hkv, L0, S, kind, sinks=sinks, device=DEV)
    q = cc.queries(Hkv * G, S, DEV, 13)
    inv, af = _table(kc, L0 + S)
    c0 = L0 - sinks
    out = chunk_kv(kc, vc, q, k, v, k_sink=ks, v_sink=vs)
    torch.cuda.synchronize()
    heads, rows = (None, None) if L0 <= 32768 else ([0, 13, Hkv * G - 1], [0, 1, S // 2, S - 1])
    ref = rc.chunk_reference(kc, vc, q, c0, inv, af, ks, vs, heads=heads, rows=rows)
    got = out if heads is None else out[rows][:, heads]
    cc.check(got, ref, "chunk nuq%d sinks=%d %d/%d L0=%d S=%d %s" % (bits, sinks, Hkv * G, Hkv, L0, S, kind))


def _twins(route, bits, sinks, Hkv, G, L, monkeypatch):
    """the route run on twin caches: rope = None (the theta rule) and an explicit ops.rope_freqs(theta) table with
    attention factor 1.  Returns the two outputs."""
    from kvquant_amd import cache, ops
    outs = []
    for explicit in (False, True):
        kc, vc, k, v, ks, vs = rc.make(bits, Hkv, L - 1 if route != "chunk" else L, 1 if route != "chunk" else 48, None,
                                       sinks=sinks, device=DEV, seed=3)
        if explicit:
            tab = (ops.rope_freqs(kc.rope_theta, DEV), 1.0)
            kc.rope_table = lambda n, tab=tab: tab
        q = cc.queries(Hkv * G, 48, DEV, 13)
        if route == "chunk":
            outs.append(cache.chunk_kv(kc, vc, q, k, v, k_sink=ks, v_sink=vs))
        elif route == "dense":
            # include_sparse=False caches: QuantK.append_and_score (kvq_score_k)
            kd = cache.QuantK(bits=bits, hidden_size=Hkv * 128, num_heads=Hkv, max_position_embeddings=L + 8,
                              device=DEV, rope_theta=kc.rope_theta)
            kd.lookup_table = kc.lookup_table
            if explicit:
                kd.rope_table = kc.rope_table
            for t in range(3):
                ops.append_k(bits, kd.kcache, kd.lookup_table, k[:, :, 0].reshape(-1).float().contiguous(), t)
            kd.klen = 3
            outs.append(kd.append_and_score(q[:, :1].transpose(0, 1).float().contiguous(),
                                            k[:, :, 0].reshape(-1).float().contiguous()))
        else:
            if route == "multicall":
                monkeypatch.setattr(cache, "ONE_CALL_PER_LAYER", False)
            if route == "fused":
                monkeypatch.setattr(cache, "FUSED_ATTEND", True)
            outs.append(rc.decode_step(kc, vc, q[:, 0].contiguous(), k, v, ks, vs))
        monkeypatch.undo()
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("route,bits,sinks,Hkv,G,L", [
    ("step", 4, 0, 32, 1, 4096), ("step", 3, 5, 32, 1, 20000), ("multicall", 4, 5, 32, 1, 4096),
    ("multicall", 2, 0, 32, 1, 20000), ("dense", 4, 0, 8, 1, 300), ("gqa", 4, 0, 8, 4, 4096), ("gqa", 3, 0, 8, 4, 20000),
    ("chunk", 4, 5, 8, 1, 4096), ("chunk", 3, 0, 8, 4, 20000)])
def test_explicit_theta_table_is_bit_identical(route, bits, sinks, Hkv, G, L, monkeypatch):
    a, b = _twins(route, bits, sinks, Hkv, G, L, monkeypatch)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), route


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("entry", ["heads", "grouped", "tree"])
def test_explicit_theta_table_is_bit_identical_on_every_chunk_entry(entry, bits, monkeypatch):
    """every scaled-RoPE instantiation of the chunk kernel (per-head, grouped, tree; 2 / 3 / 4 bit) against its
    theta-rule twin: S = 7 rows over 60 cached columns (the chunk straddles a 64-column tile with a ragged last tile),
    G = 4 (rowless waves in the grouped geometry)"""
    from kvquant_amd import cache, ops
    from tests import tree_check as tc
    Hkv, G, L0, S = 2, 4, 60, 7
    monkeypatch.setattr(ops, "CHUNK_GROUPED", entry != "heads")
    assert ops.chunk_attention_route(Hkv * G, Hkv, S) == ("heads" if entry == "heads" else "grouped")
    q = cc.queries(Hkv * G, S, DEV, 13)
    outs = []
    for explicit in (False, True):
        kc, vc, k, v, ks, vs = rc.make(bits, Hkv, L0, S, None, device=DEV, seed=3)
        rope = (ops.rope_freqs(kc.rope_theta, DEV), 1.0) if explicit else None
        cache.chunk_kv(kc, vc, q, k, v)                # (packs the chunk into columns L0 .. L0 + S - 1)
        layer = cache.layer_struct(kc, vc)
        if entry == "tree":
            outs.append(ops.chunk_attention_tree(layer, Hkv * G, L0, q, tc.SHAPES["random"](S), rope=rope))
        else:
            outs.append(ops.chunk_attention(layer, Hkv * G, L0, q, rope=rope))
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), (entry, bits)


def test_fused_attend_with_table_takes_the_kernel_pair(monkeypatch):
    """KVQ_FUSED_ATTEND=1 (the opt-in fused kernel) with a frequency table: the step takes the kernel pair, whose
    output the explicit theta table reproduces bit for bit"""
    from kvquant_amd import _lib
    a, b = _twins("fused", 4, 0, 32, 1, 4096, monkeypatch)
    assert _lib.lib().kvq_decode_step_route() == 1
    assert (a - b).abs().max() < 1e-2 * a.abs().max()


def test_dynamic_table_moves_past_the_original_length():
    """dynamic NTK (max_position_embeddings 4096): two consecutive steps at 4500 and 4501 rotate with different tables,
    each step matches the fp64 statement with its own table"""
    mpe = 4096
    kc, vc, k, v, ks, vs = rc.make(4, 8, 4499, 2, "dynamic", device=DEV, max_position_embeddings=mpe)
    q = cc.queries(8, 2, DEV, 13)
    tabs = []
    for i in range(2):
        inv, af = [x.clone() if torch.is_tensor(x) else x for x in _table(kc, kc.klen + 1)]
        tabs.append(inv)
        out = rc.decode_step(kc, vc, q[:, i].contiguous(), k[:, :, i:], v[:, :, i:])
        torch.cuda.synchronize()
        ref = rc.decode_reference(kc, vc, q[:, i].contiguous(), kc.klen, inv, af)
        rc.check_decode(out, ref, "dynamic step %d (L=%d)" % (i, kc.klen))
    assert not torch.equal(tabs[0], tabs[1])
    assert torch.equal(kc.rope_table(100)[0], kc.rope_table(mpe)[0])


def test_bad_rope_arguments_are_refused_before_any_launch():
    from kvquant_amd import _lib, ops
    kc, vc, k, v, ks, vs = rc.make(4, 8, 100, 1, "llama3", device=DEV)
    inv, _ = kc.rope_table(101)
    ly = ops.make_layer(kc, vc, kc.lookup_table, kc.lookup_table)[0]
    out = torch.empty(1, 8, 128, device=DEV)
    q = cc.queries(8, 1, DEV, 1)[:, 0].contiguous()
    before = kc.kcache.clone()
    for r in (_lib.Rope(None, 1.0), _lib.Rope(inv.data_ptr(), 0.0), _lib.Rope(inv.data_ptr(), float("nan")),
              _lib.Rope(inv.data_ptr() + 2, 1.0)):
        ws = torch.empty(1 << 26, dtype=torch.uint8, device=DEV)
        base = (ws.data_ptr() + 255) & ~255
        rcode = _lib.lib().kvq_decode_step_rope(ly, 100, 100, q.data_ptr(), k[:, :, 0].contiguous().data_ptr(),
                                               v[:, :, 0].contiguous().data_ptr(), 1, None, None, None, out.data_ptr(), 1,
                                               base, ws.numel() - 256, r, ops._stream())
        assert rcode != 0
    torch.cuda.synchronize()
    assert torch.equal(before, kc.kcache)
