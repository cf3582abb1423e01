"""Chunk attention over the compressed cache (cache.chunk_kv -> kvq_chunk_attention): outputs against the fp64 statement
of the semantics over the dequantised cache and against the same tokens fed one at a time through decode_kv; the cache
state after a chunk against S decode appends, bit for bit."""
import pytest
import torch

from tests import chunk_check as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (bits, norm, sinks, Hkv, G, L0 (cached tokens, sinks included), S)
CASES = [
    (4, False, 0, 4, 1, 1, 2),
    (4, False, 5, 4, 1, 6, 17),
    (4, False, 0, 4, 4, 777, 64),
    (3, False, 5, 4, 1, 4100, 200),
    (3, False, 0, 2, 4, 1000, 1000),
    (2, False, 0, 4, 1, 3000, 17),
    (2, True, 5, 4, 4, 2049, 64),
    (4, False, 5, 2, 4, 32768, 200),
    (2, False, 5, 4, 1, 32768, 1000),
]


def _run(bits, norm, sinks, Hkv, G, L0, S, seed=0):
    from kvquant_amd.cache import chunk_kv
    max_len = L0 + S + 64
    kc, vc, scale, shift = cc.make_caches(bits, Hkv, max_len, sinks=sinks, norm=norm, device=DEV, seed=seed)
    kp, vp = cc.tokens(L0 - sinks + S, Hkv, scale, shift, DEV, seed=seed + 11)
    n0 = L0 - sinks
    cc.fill(kc, vc, kp[:, :, :n0], vp[:, :, :n0])
    ks, vs = cc.sink_caches(Hkv, sinks, DEV, seed + 12) if sinks else (None, None)
    q = cc.queries(Hkv * G, S, DEV, seed + 13)
    k, v = kp[:, :, n0:].contiguous(), vp[:, :, n0:].contiguous()
    out = chunk_kv(kc, vc, q, k, v, k_sink=ks, v_sink=vs)
    torch.cuda.synchronize()
    return kc, vc, q, k, v, ks, vs, out, n0


@pytest.mark.parametrize("bits,norm,sinks,Hkv,G,L0,S", CASES)
def test_chunk_vs_fp64(bits, norm, sinks, Hkv, G, L0, S):
    kc, vc, q, k, v, ks, vs, out, c0 = _run(bits, norm, sinks, Hkv, G, L0, S)
    assert out.shape == (S, Hkv * G, 128) and torch.isfinite(out).all()
    ref = cc.reference(kc, vc, q, c0, ks, vs)
    cc.check(out, ref, "nuq%d%s sinks=%d Hkv=%d G=%d L0=%d S=%d" % (bits, " norm" if norm else "", sinks, Hkv, G, L0, S))


@pytest.mark.parametrize("bits,norm,sinks,Hkv,G,L0,S", [CASES[1], CASES[2], CASES[3], CASES[6]])
def test_chunk_state_and_outputs_vs_decode(bits, norm, sinks, Hkv, G, L0, S):
    """a twin cache fed the same tokens one at a time through decode_kv ends bit-equal; the outputs agree to the fp16
    rounding of the decode path's scores (the reference's dtype order, which the chunk kernel does not imitate)"""
    kc, vc, q, k, v, ks, vs, out, c0 = _run(bits, norm, sinks, Hkv, G, L0, S)
    kc2, vc2, scale, shift = cc.make_caches(bits, Hkv, L0 + S + 64, sinks=sinks, norm=norm, device=DEV, seed=0)
    kp, vp = cc.tokens(L0 - sinks + S, Hkv, scale, shift, DEV, seed=11)
    cc.fill(kc2, vc2, kp[:, :, :c0], vp[:, :, :c0])
    twin = cc.decode_twin(kc2, vc2, q, k, v, ks, vs)
    torch.cuda.synchronize()
    assert kc.klen == kc2.klen and vc.vlen == vc2.vlen
    for name in ("kcache", "outliers", "outlier_indices", "outliers_t", "outlier_indices_t"):
        assert torch.equal(getattr(kc, name), getattr(kc2, name)), "K " + name
    for name in ("vcache", "lookup_table", "outliers", "outlier_indices"):
        assert torch.equal(getattr(vc, name), getattr(vc2, name)), "V " + name
    if norm:
        assert torch.equal(vc.lookup_table2, vc2.lookup_table2)
    d = (out - twin).abs().amax(dim=-1) / twin.abs().amax(dim=-1)
    print("chunk vs %d decode steps: max row err %.2e" % (S, float(d.max())))
    assert float(d.max()) < 1e-2


def test_chunk_deterministic():
    a = _run(4, False, 5, 4, 4, 4100, 200)[7]
    b = _run(4, False, 5, 4, 4, 4100, 200)[7]
    assert torch.equal(a, b)


def test_chunk_long_128k():
    """L0 = 131072, S = 512, 32 heads, nuq4 + 1 %: sampled heads and rows against the fp64 statement"""
    kc, vc, q, k, v, ks, vs, out, c0 = _run(4, False, 0, 32, 1, 131072, 512)
    heads, rows = [0, 13, 31], [0, 1, 255, 256, 400, 511]
    ref = cc.reference(kc, vc, q, c0, heads=heads, rows=rows)
    cc.check(out[rows][:, heads], ref, "nuq4 H=32 L0=131072 S=512 (sampled)")
