"""Sliding-window attention over ring caches on the GPU (tests/window_check.py): a ring cache and its linear twin take
the same stream.  (1) every resident ring column equals the twin's column of the same token after every append, across
the wrap; (2) kvq_chunk_attention_window[_grouped] against the fp64 statement over the twin, with fully masked tiles
(C = 192, W = 100) and a fully masked split (C = 640, W = 300); (3) no window in sight: the plain entries' bits;
(4) masked columns contribute exactly nothing; (5) refusals, truncate."""
import ctypes

import pytest
import torch

from tests import chunk_check as cc
from tests import window_check as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _window(st, Hq, n0, q, grouped):
    from kvquant_amd import ops
    return ops.chunk_attention_window(st.layer(), Hq, n0, st.W, q, k_sink=st.ks, v_sink=st.vs, rope=st.rope_table(),
                                      grouped=grouped)


# ---- 1. state ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,sinks,norm", [(4, 0, False), (2, 5, True), (3, 0, False)])
def test_ring_columns_equal_the_twins(bits, sinks, norm):
    """appends of 1 .. 150 tokens, several of them across the wrap of a 192-column ring (N = 150 -> 210, 380 -> 450),
    two wraps in all; Q-Norm adds lookup_table2"""
    st = wc.Stream(bits, 2, 192, 100, 470, sinks=sinks, norm=norm, device=DEV, seed=1)
    for S in (150, 60, 1, 17, 93, 59, 1, 69, 17, 3):
        st.pack(S)
        wc.assert_state(st)
        assert st.kc.klen == st.vc.vlen == sinks + st.N and st.kc.high_water == st.N
    assert st.N == 470
    assert st.kc.kcache.shape[2] == 192 and st.vc.lookup_table.shape[0] == 192


# ---- 2. outputs against the fp64 statement over the twin -------------------------------------------------------------
# C = 192, W = 100: 99 packed tokens, then chunks; N = 192 (S = 93 = C - W + 1) and N = 228 are steps whose masked span
# covers a whole 64-column tile
SCHEDULE = (93, 1, 17, 17, 1, 40, 93, 17, 40, 1, 31)
FULL = [(4, 4, 0, None), (4, 4, 5, None), (4, 1, 0, None), (4, 1, 5, None),
        (3, 4, 5, None), (2, 4, 0, None), (4, 4, 0, "llama3")]


@pytest.mark.parametrize("bits,G,sinks,rope", FULL)
def test_window_vs_fp64_two_wraps(bits, G, sinks, rope):
    Hkv, C, W = 2, 192, 100
    Hq = Hkv * G
    st = wc.Stream(bits, Hkv, C, W, 99 + sum(SCHEDULE), sinks=sinks, device=DEV, seed=2, rope=rope)
    st.pack(99)
    seen = set()
    for step, S in enumerate(SCHEDULE):
        n0 = st.N
        st.pack(S)
        seen.add(st.N)
        q = cc.queries(Hq, S, DEV, 13 + step)
        ref = st.reference(q, n0)
        for grouped in ([False, True] if (G >= 2 and S <= 32) else [False]):
            out = _window(st, Hq, n0, q, grouped)
            assert torch.isfinite(out).all()
            cc.check(out, ref, "window nuq%d %d/%d sinks=%d N=%d S=%d %s%s" % (
                bits, Hq, Hkv, sinks, st.N, S, "grouped" if grouped else "heads", " " + rope if rope else ""))
    assert {192, 228, 450} <= seen


@pytest.mark.parametrize("sinks", [0, 5])
@pytest.mark.parametrize("S", [1, 64])
def test_window_vs_fp64_masked_split(S, sinks):
    """C = 640 (10 tiles, two splits), W = 300: at N = 1280 and N = 1920 the ring has wrapped exactly, and for S = 1 every
    visible column lies in split 1.  Without sinks split 0 then holds nothing a row sees: it writes the (-inf, 0)
    partial and the merge takes its skip; with sinks (attended in split 0) its partial is the sink tokens' alone.  S = 64
    reaches back into split 0."""
    from kvquant_amd import ops
    Hkv, G, C, W = 1, 2, 640, 300
    a256 = lambda x: (x + 255) & ~255                   # (the partials of TWO splits)
    assert ops._L().kvq_chunk_attention_window_workspace_bytes(Hkv * G, Hkv, S, 1280 - S, W, C) == \
        a256(Hkv * G * 2 * S * cc.HD * 4) + a256(Hkv * G * 2 * S * 8)
    st = wc.Stream(4, Hkv, C, W, 1920, sinks=sinks, device=DEV, seed=3)
    st.pack(640)
    for stop in (1280, 1920):
        st.pack(stop - S - st.N)
        n0 = st.N
        st.pack(S)
        assert st.N == stop
        q = cc.queries(Hkv * G, S, DEV, stop)
        ref = st.reference(q, n0)
        for grouped in ([False, True] if S <= 32 else [False]):
            out = _window(st, Hkv * G, n0, q, grouped)
            assert torch.isfinite(out).all()
            cc.check(out, ref, "window C=640 sinks=%d N=%d S=%d %s" % (sinks, stop, S, "grouped" if grouped else "heads"))


# ---- 3. nothing masked, nothing wrapped: the plain entries' bits ------------------------------------------------------
@pytest.mark.parametrize("bits,Hkv,G,C,W,n0,S", [
    (4, 2, 4, 192, 150, 60, 17), (3, 2, 4, 192, 176, 159, 17), (2, 2, 1, 192, 160, 100, 33),
    (4, 1, 2, 640, 320, 10, 300)])
def test_no_window_in_sight_equals_the_plain_entries(bits, Hkv, G, C, W, n0, S):
    from kvquant_amd import ops
    Hq = Hkv * G
    st = wc.Stream(bits, Hkv, C, W, n0 + S, sinks=5, device=DEV, seed=4)
    st.pack(n0)
    st.pack(S)
    assert st.N <= C and W >= st.N
    q = cc.queries(Hq, S, DEV, 7)
    for grouped in ([False, True] if (G >= 2 and S <= 32) else [False]):
        name = "kvq_chunk_attention_grouped" if grouped else "kvq_chunk_attention"
        plain = ops._chunk_call("chunk_attention", name, st.layer(), Hq, n0, q, None, st.ks, st.vs, None)
        out = _window(st, Hq, n0, q, grouped)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        assert torch.equal(out, plain), name


# ---- 4. masking is exact ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,sinks", [(17, 0), (40, 5)])
def test_masked_columns_contribute_nothing(S, sinks):
    """two rings whose streams share only the last W + S - 1 tokens (stale columns differ, visible ones do not) give the
    same bits through chunk_kv; a third that differs in ONE visible token does not"""
    from kvquant_amd.cache import chunk_kv
    Hkv, G, C, W, N = 2, 4, 192, 100, 450
    shared = W + S - 1
    a = wc.Stream(4, Hkv, C, W, N, sinks=sinks, device=DEV, seed=5)
    b = wc.Stream(4, Hkv, C, W, N, sinks=sinks, device=DEV, seed=5, token_seed=77)
    c = wc.Stream(4, Hkv, C, W, N, sinks=sinks, device=DEV, seed=5)
    assert not torch.equal(a.k[:, :, :N - shared], b.k[:, :, :N - shared])
    b.k[:, :, N - shared:], b.v[:, :, N - shared:] = a.k[:, :, N - shared:], a.v[:, :, N - shared:]
    c.v[:, :, N - 50] = -c.v[:, :, N - 50]
    q = cc.queries(Hkv * G, S, DEV, 21)
    outs = []
    for st in (a, b, c):
        for piece in (150, 150, N - 300 - S):
            st.pack(piece)
        k, v = st.take(S)
        outs.append(chunk_kv(st.kc, st.vc, q, k, v, k_sink=st.ks, v_sink=st.vs))
        st.tk.parallel_pack(k.float())
        st.tv.parallel_pack(v.float())
        assert st.kc.klen == sinks + N
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], outs[2])
    # (and chunk_kv's answer is the statement's)
    a.N = N
    cc.check(outs[0], a.reference(q, N - S), "chunk_kv on a ring, S=%d sinks=%d" % (S, sinks))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
def _rc(st, Hq, S, n0, window, grouped=False, layer=None):
    """the entry's return code with a valid q / out / workspace"""
    from kvquant_amd import ops
    q = cc.queries(Hq, max(S, 1), DEV, 1)
    out = torch.empty((max(S, 1), Hq, 128), dtype=torch.float32, device=DEV)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) & ~255
    fn = getattr(ops._L(), "kvq_chunk_attention_window_grouped" if grouped else "kvq_chunk_attention_window")
    return fn(ctypes.byref(layer if layer is not None else st.layer()), Hq, S, n0, window, q.data_ptr(), q.stride(0),
              q.stride(1), None, None, 0, out.data_ptr(), base, (1 << 22) - 256, None,
              torch.cuda.current_stream().cuda_stream)


def test_refusals_of_the_entries():
    from kvquant_amd import cache, ops
    L = ops._L()
    st = wc.Stream(4, 2, 192, 100, 120, device=DEV, seed=6)
    st.pack(120)
    odd = wc.make_ring(4, 2, 200, 100, device=DEV, seed=6, window=False)       # (a linear cache: 200 columns are no ring)
    odd_layer = cache.layer_struct(odd[0], odd[1])
    assert odd_layer.max_len == 200
    EINVAL = -1
    assert _rc(st, 8, 17, 103, 100) == 0 and _rc(st, 8, 17, 103, 100, grouped=True) == 0
    torch.cuda.synchronize()
    # (Hq, Hkv, S, n0, window, max_len)
    bad = [(8, 2, 17, 103, 0, 192), (8, 2, 17, 103, -3, 192), (8, 2, 94, 26, 100, 192), (8, 2, 17, 103, 177, 192),
           (8, 2, 17, 103, 100, 200), (8, 2, 17, -1, 100, 192), (8, 2, 17, 2 ** 31 - 17, 100, 192),
           (8, 2, 0, 103, 100, 192), (7, 2, 17, 103, 100, 192), (18, 2, 17, 103, 100, 192), (8, 2, 17, 103, 100, 0)]
    for Hq, Hkv, S, n0, W, C in bad:
        assert L.kvq_chunk_attention_window_workspace_bytes(Hq, Hkv, S, n0, W, C) == 0, (Hq, Hkv, S, n0, W, C)
        assert L.kvq_chunk_attention_window_grouped_workspace_bytes(Hq, Hkv, S, n0, W, C) == 0, (Hq, Hkv, S, n0, W, C)
        if C == 192 and Hkv == 2:
            assert _rc(st, Hq, S, n0, W) == EINVAL, (Hq, S, n0, W)
            assert _rc(st, Hq, S, n0, W, grouped=True) == EINVAL, (Hq, S, n0, W)
    assert L.kvq_chunk_attention_window_workspace_bytes(8, 2, 93, 27, 100, 192) > 0       # W + S - 1 == C
    assert _rc(st, 8, 17, 0, 100, layer=odd_layer) == EINVAL                                # max_len % 64
    # position overflow shows with pos_offset only: the workspace function cannot see it
    far = wc.Stream(4, 2, 192, 100, 8, sinks=5, device=DEV, seed=6)
    assert L.kvq_chunk_attention_window_workspace_bytes(8, 2, 17, 2 ** 31 - 20, 100, 192) > 0
    assert _rc(far, 8, 17, 2 ** 31 - 20, 100) == EINVAL
    # the grouped twin: G == 1 and S > 32
    assert L.kvq_chunk_attention_window_grouped_workspace_bytes(2, 2, 17, 103, 100, 192) == 0
    assert L.kvq_chunk_attention_window_grouped_workspace_bytes(8, 2, 33, 87, 100, 192) == 0
    assert _rc(st, 2, 17, 103, 100, grouped=True) == EINVAL and _rc(st, 8, 33, 87, 100, grouped=True) == EINVAL
    with pytest.raises(ValueError):
        ops.chunk_attention_window(st.layer(), 8, 103, 0, cc.queries(8, 17, DEV, 1))
    with pytest.raises(ValueError):
        ops.chunk_attention_window(st.layer(), 8, 26, 100, cc.queries(8, 94, DEV, 1))


def test_refusals_of_the_caches():
    from kvquant_amd import cache
    st = wc.Stream(4, 2, 192, 100, 300, device=DEV, seed=6)
    st.pack(150)
    k, v = st.take(1)
    q = cc.queries(8, 1, DEV, 1)
    with pytest.raises(ValueError, match="chunk_kv"):
        cache.decode_kv(st.kc, st.vc, q[:, 0].contiguous(), k.reshape(-1), v.reshape(-1))
    with pytest.raises(ValueError, match="chunk_kv"):
        st.kc.append_and_score(q[:2, :1].float().transpose(0, 1).contiguous(), k.reshape(-1).float())
    with pytest.raises(ValueError, match="chunk_kv"):
        st.vc.append_and_mix(torch.zeros(1, 2, 151, device=DEV), v.reshape(-1).float())
    with pytest.raises(ValueError, match="chunk_kv"):
        cache.shard_attention(st.kc, st.vc, q[:2, 0].contiguous())
    for call in (lambda: st.kc.keep_columns(4, [0, 2]), lambda: st.vc.keep_columns(4, [0, 2]),
                 lambda: cache.keep_kv(st.kc, st.vc, 4, [0, 2])):
        with pytest.raises(ValueError, match="ring"):
            call()
    with pytest.raises(ValueError):                                      # W + S - 1 > C
        k94, v94 = st.take(94)
        cache.chunk_kv(st.kc, st.vc, cc.queries(8, 94, DEV, 1), k94, v94)
    with pytest.raises(ValueError):
        cache.chunk_kv(st.kc, st.vc, cc.queries(8, 4, DEV, 1), *st.take(4), parent=[0, 0, 1, 1])
    assert st.kc.klen == 150 and st.kc.high_water == 150                 # (nothing was packed by the refused calls)
    kw = dict(bits=4, hidden_size=256, num_heads=2, max_position_embeddings=192, device=DEV)
    for cls in (cache.QuantK, cache.QuantV):
        for extra in (dict(include_sparse=True, compact=True), dict(include_sparse=False)):
            with pytest.raises(ValueError):
                cls(window=100, **kw, **extra)
        with pytest.raises(ValueError):
            cls(window=100, include_sparse=True, **dict(kw, max_position_embeddings=200))
        with pytest.raises(ValueError):
            cls(window=0, include_sparse=True, **kw)
    with pytest.raises(ValueError):
        cache.QuantK(window=100, include_sparse=True, use_orig_sparse=True, **kw)


def test_a_refused_chunk_leaves_the_ring_as_it_was():
    """what only the window entry refuses -- q layout, position overflow -- is refused by chunk_kv BEFORE it packs"""
    from kvquant_amd import cache
    st = wc.Stream(4, 2, 192, 100, 200, sinks=5, device=DEV, seed=6)
    st.pack(150)
    k, v = st.take(4)
    q = cc.queries(8, 4, DEV, 1)
    before = [t.clone() for _, t, _ in wc.column_arrays(st.kc, st.vc)]
    for bad_q in (q.float(), q[:7], q[:, :, :64], cc.queries(8, 5, DEV, 1)[:, :4, 1:129]):
        with pytest.raises(ValueError):
            cache.chunk_kv(st.kc, st.vc, bad_q, k, v, k_sink=st.ks, v_sink=st.vs)
    st.kc.klen = st.vc.vlen = 2 ** 31 - 3                 # the next chunk's positions pass 2^31
    with pytest.raises(ValueError):
        cache.chunk_kv(st.kc, st.vc, q, k, v, k_sink=st.ks, v_sink=st.vs)
    assert st.kc.klen == st.vc.vlen == 2 ** 31 - 3 and st.kc.high_water == st.vc.high_water == 150
    for a, (_, b, _) in zip(before, wc.column_arrays(st.kc, st.vc)):
        assert torch.equal(a, b)
    st.kc.klen = st.vc.vlen = 155
    out = cache.chunk_kv(st.kc, st.vc, q, k, v, k_sink=st.ks, v_sink=st.vs)
    assert torch.isfinite(out).all() and st.kc.klen == 159


def test_truncate_on_a_ring():
    """a rollback inside the slack leaves the ring as if the dropped tokens had never come: re-appending other tokens
    gives the statement's output for the tokens actually kept; past the slack it raises and changes nothing"""
    from kvquant_amd.cache import chunk_kv
    Hkv, G, C, W = 2, 4, 192, 100
    st = wc.Stream(4, Hkv, C, W, 500, sinks=5, device=DEV, seed=8)
    for piece in (150, 150, 60, 40):          # N = 400; the last piece crosses the wrap (columns 168 .. 191, 0 .. 15)
        st.pack(piece)
    assert st.N == 400 and st.kc.high_water == 400
    for c in (st.kc, st.vc):
        with pytest.raises(ValueError):       # 400 - 94 - 100 + 1 < 400 - 192
            c.truncate(94)
    assert st.kc.klen == st.vc.vlen == 405
    wc.assert_state(st)
    for c in (st.kc, st.vc, st.tk, st.tv):    # 93 = C - W + 1 is the slack; 40 drops the piece across the wrap
        c.truncate(40)
    st.N = 360
    assert st.kc.klen == st.vc.vlen == 365 and st.kc.high_water == 400
    for _, arr, ax in wc.column_arrays(st.kc, st.vc):
        dropped = torch.cat((arr.narrow(ax, 168, 24), arr.narrow(ax, 0, 16)), dim=ax)
        assert not dropped.any()
    # other tokens take the dropped ones' place (the stream's tokens 460 ..)
    S = 17
    k, v = st.k[:, :, 460:460 + S].contiguous(), st.v[:, :, 460:460 + S].contiguous()
    q = cc.queries(Hkv * G, S, DEV, 9)
    out = chunk_kv(st.kc, st.vc, q, k, v, k_sink=st.ks, v_sink=st.vs)
    st.tk.parallel_pack(k.float())
    st.tv.parallel_pack(v.float())
    st.N = 360 + S
    assert torch.isfinite(out).all()
    cc.check(out, st.reference(q, 360), "after truncate(40) on a ring")
    # every column a later token can still see equals the twin's (older survivors of the overwritten lap are stale)
    wc.assert_state(st, lo_token=st.kc.high_water - C)
