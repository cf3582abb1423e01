"""Chunk attention, host side (no GPU): the entry points exist, the workspace size is a function of the shape, every bad
argument is refused before any launch, and KVQuantAttention routes q_len > 1 on a warm cache as documented."""
import ctypes
import math

import pytest
import torch

from kvquant_amd import _lib

EINVAL, EWORKSPACE = -1, -3
P = 4096            # a fake device pointer: every refused call returns before anything is dereferenced


def test_exported():
    lib = _lib.lib()
    for name in ("kvq_chunk_attention", "kvq_chunk_attention_workspace_bytes"):
        assert hasattr(lib, name), name
    assert lib.kvq_version() // 100 == _lib.ABI_MAJOR


def test_workspace_size():
    lib = _lib.lib()
    ws = lib.kvq_chunk_attention_workspace_bytes
    assert ws(32, 32, 512, 131072) == ws(32, 32, 512, 131072) > 0
    assert ws(32, 8, 512, 4096) > 0
    # grows with S; with L (more splits) while the grid is small
    assert ws(32, 32, 8192, 131072) > ws(32, 32, 512, 131072) > ws(32, 32, 16, 131072)
    assert ws(32, 32, 16, 131072) > ws(32, 32, 16, 256)
    assert ws(32, 32, 4096, 131072) <= 1 << 30     # (cache.chunk_kv calls it in pieces of 4096 rows)
    for bad in [(32, 7, 16, 100), (72, 8, 16, 100), (0, 8, 16, 100), (32, 32, 0, 100), (32, 32, 16, -1),
                (32, 32, 65537, 0), (130, 65, 16, 100)]:
        assert ws(*bad) == 0, bad


def _layer(**kw):
    d = dict(bits=4, H=4, hd=128, thr_k=3, max_len=1024, rope_theta=10000.0, pos_offset=0, kmat=P, klut=P, klut_off=P,
             klo=P, khi=P, koutliers=P, kidx=P, koutliers_t=P, kidx_t=P, klut_ends=None, klut_score=None, vmat=P,
             vlut_rows=P, vlut_sorted=P, voutliers=P, vidx=P, vnorm=None, v_mix_rows=None, flags=0)
    d.update(kw)
    return _lib.Layer(**d)


def _call(ly, Hq=4, S=16, c0=100, q=P, qsh=2048, qss=128, ks=None, vs=None, ns=0, out=P, ws=P, wsb=1 << 30):
    return _lib.lib().kvq_chunk_attention(None if ly is None else ctypes.byref(ly), Hq, S, c0, q, qsh, qss, ks, vs, ns,
                                          out, ws, wsb, None)


@pytest.mark.parametrize("kw,args", [
    (dict(), dict(q=None)),
    (dict(), dict(out=None)),
    (dict(bits=5), dict()),
    (dict(hd=64), dict()),
    (dict(thr_k=0), dict()),
    (dict(), dict(Hq=6)),                  # Hq not a multiple of Hkv
    (dict(), dict(Hq=36)),                 # G > 8
    (dict(), dict(S=0)),
    (dict(), dict(c0=-1)),
    (dict(), dict(c0=1020, S=5)),          # c0 + S > max_len
    (dict(pos_offset=-1), dict()),
    (dict(kmat=None), dict()),
    (dict(vmat=None), dict()),
    (dict(klut=None), dict()),
    (dict(koutliers_t=None), dict()),      # compact caches carry no mirror rows: not taken
    (dict(kidx_t=None), dict()),
    (dict(voutliers=None), dict()),
    (dict(vidx=None), dict()),
    (dict(vlut_rows=None), dict()),
    (dict(), dict(ns=65, ks=P, vs=P)),     # more sink tokens than one tile
    (dict(), dict(ns=4)),                  # sinks without their caches
    (dict(), dict(qss=100)),               # q rows not 16-byte vectors
    (dict(), dict(q=P + 8)),
    (dict(), dict(out=P + 4)),
])
def test_einval(kw, args):
    assert _call(_layer(**kw), **args) == EINVAL


def test_null_layer_and_workspace():
    assert _call(None) == EINVAL
    assert _call(_layer(), ws=None) == EWORKSPACE
    assert _call(_layer(), wsb=16) == EWORKSPACE
    assert _call(_layer(), ws=P + 16) == EWORKSPACE


@pytest.mark.parametrize("klen,q_len,sinks,fast,route", [
    (10, 5, 0, True, [("chunk", 5)]),
    (10, 5, 4, True, [("chunk", 5)]),
    (2, 9, 5, True, [("token", 3), ("chunk", 6)]),      # crosses the sink boundary
    (2, 4, 5, True, [("token", 3), ("token", 1)]),      # one token left after the sinks
    (1, 3, 5, True, [("token", 3)]),                    # still filling the sinks
    (10, 5, 0, False, [("token", 5)]),                  # configuration without the kernel
    (3, 8, 5, False, [("token", 2), ("token", 6)]),
])
def test_chunk_route(klen, q_len, sinks, fast, route):
    from kvquant_amd.attention import chunk_route
    assert chunk_route(klen, q_len, sinks, fast) == route


class _Rec:
    def __init__(self):
        self.calls = []


def _attention(monkeypatch, rec, sinks=0, G=1, stub_tokens=True, **kw):
    """a CPU KVQuantAttention whose compressed-cache calls are stubs that record what they were given (stub_tokens:
    q_len == 1 calls of attend() too)"""
    from kvquant_amd import attention as at
    a = at.KVQuantAttention(hidden_size=512 * G, num_heads=4 * G, num_key_value_heads=4, abits=4, first_few_fp16=sinks,
                            maxseqlen=256, device="cpu", make_proj=False, **kw)
    a.kcache.include_sparse = a.vcache.include_sparse = True

    def fake_chunk(kc, vc, q, k, v, k_sink=None, v_sink=None):
        S = q.shape[1]
        rec.calls.append(("chunk", kc.klen, S, k_sink is not None))
        kc.klen += S
        vc.vlen += S
        return torch.zeros(S, q.shape[0], 128)
    monkeypatch.setattr(at, "chunk_kv", fake_chunk)
    if not stub_tokens:
        return a
    orig = at.KVQuantAttention.attend

    def attend(self, q, k, v):
        if q.shape[2] == 1:
            rec.calls.append(("token", self.kcache.klen))
            self.kcache.klen += 1
            self.vcache.vlen += 1
            return torch.zeros(1, 1, self.hidden_size, dtype=q.dtype)
        return orig(self, q, k, v)
    monkeypatch.setattr(at.KVQuantAttention, "attend", attend)
    return a


def _qkv(a, n, dtype=torch.float16):
    H, Hkv = a.num_heads, a.num_key_value_heads
    return (torch.zeros(1, H, n, 128, dtype=dtype), torch.zeros(1, Hkv, n, 128, dtype=dtype),
            torch.zeros(1, Hkv, n, 128, dtype=dtype))


@pytest.mark.parametrize("G", [1, 4])
def test_attend_routes(monkeypatch, G):
    rec = _Rec()
    a = _attention(monkeypatch, rec, sinks=5, G=G)
    a.kcache.klen = a.vcache.vlen = 2
    out = a.attend_multi(*_qkv(a, 9))
    assert out.shape == (1, 9, 512 * G)
    assert rec.calls == [("token", 2), ("token", 3), ("token", 4), ("chunk", 5, 6, True)]
    assert a.kcache.klen == 11


@pytest.mark.parametrize("knob", ["compact", "fp32", "dense", "env"])
def test_attend_fallbacks(monkeypatch, knob):
    from kvquant_amd import attention as at
    rec = _Rec()
    a = _attention(monkeypatch, rec, compact=knob == "compact")
    if knob == "dense":
        a.kcache.include_sparse = False
    if knob == "env":
        monkeypatch.setattr(at, "CHUNK_ATTEND", False)
    a.kcache.klen = a.vcache.vlen = 10
    a.attend_multi(*_qkv(a, 4, torch.float32 if knob == "fp32" else torch.float16))
    assert rec.calls == [("token", 10), ("token", 11), ("token", 12), ("token", 13)]


def _randn_qkv(a, n, gen):
    H, Hkv = a.num_heads, a.num_key_value_heads
    return (torch.randn(1, H, n, 128, generator=gen).half(), torch.randn(1, Hkv, n, 128, generator=gen).half(),
            torch.randn(1, Hkv, n, 128, generator=gen).half())


@pytest.mark.parametrize("G", [1, 4])
def test_sink_filling_phase(monkeypatch, G):
    """five single tokens into an empty cache with 5 fp16 sink tokens: every output bit-equal to the plain statement
    of the phase (post-RoPE keys, KV heads repeated per group, fp16 matmuls around an fp32 softmax rounded to fp16)"""
    from kvquant_amd.attention import rotate_half
    a = _attention(monkeypatch, _Rec(), sinks=5, G=G, stub_tokens=False)
    gen = torch.Generator().manual_seed(100 + G)
    keys = torch.zeros(1, 4, 128, 0, dtype=torch.float16)
    vals = torch.zeros(1, 4, 0, 128, dtype=torch.float16)
    for t in range(5):
        q, k, v = _randn_qkv(a, 1, gen)
        out = a.attend(q, k, v)
        cos, sin = a.rotary_emb(v, t, t + 1)
        q_rope = q * cos + rotate_half(q) * sin
        k_rope = k * cos + rotate_half(k) * sin
        keys = torch.cat((keys, k_rope.transpose(2, 3)), dim=3)
        vals = torch.cat((vals, v), dim=2)
        w = torch.matmul(q_rope, keys.repeat_interleave(G, dim=1)) / math.sqrt(128)
        w = torch.softmax(w, dim=-1, dtype=torch.float32).half()
        ref = torch.matmul(w, vals.repeat_interleave(G, dim=1)).transpose(1, 2).reshape(1, 1, 512 * G)
        assert out.dtype == torch.float16 and torch.equal(out, ref), t
    assert a.kcache.klen == 5 and a.vcache.vlen == 5


@pytest.mark.parametrize("sinks", [0, 5])
@pytest.mark.parametrize("G", [1, 4])
def test_prefill_and_decode_routing(monkeypatch, G, sinks):
    """a 7-token prompt goes through ONE ops.prefill_attention call and the packs of the tokens behind the fp16 sink
    tokens; a decode token through ONE decode_kv call that gets the sink caches exactly when there are sink tokens"""
    from kvquant_amd import attention as at
    from kvquant_amd.cache import QuantK, QuantV
    a = _attention(monkeypatch, _Rec(), sinks=sinks, G=G, stub_tokens=False)
    prefills, packs, decodes = [], [], []

    def fake_prefill(q, k, v, softmax_scale=None):
        prefills.append((tuple(q.shape), tuple(k.shape), tuple(v.shape)))
        return torch.zeros(q.shape[1], q.shape[0] * 128, dtype=torch.float16)

    def fake_pack_k(self, k, *args, **kw):
        packs.append(("k", tuple(k.shape)))
        self.klen += k.shape[-1]

    def fake_pack_v(self, v, *args, **kw):
        packs.append(("v", tuple(v.shape)))
        self.vlen += v.shape[-1]

    def fake_decode(kc, vc, q, k, v, sink_scores=None, k_sink=None, v_sink=None):
        decodes.append((tuple(q.shape), sink_scores, k_sink, v_sink))
        return torch.zeros(1, q.shape[0], 128), None
    monkeypatch.setattr(at.ops, "prefill_attention", fake_prefill)
    monkeypatch.setattr(QuantK, "parallel_pack", fake_pack_k)
    monkeypatch.setattr(QuantV, "parallel_pack", fake_pack_v)
    monkeypatch.setattr(at.ops, "rope_q_f16", lambda q, cos, sin: q)
    monkeypatch.setattr(at, "decode_kv", fake_decode)

    q, k, v = _randn_qkv(a, 7, torch.Generator().manual_seed(200 + G))
    out = a.attend(q, k, v)
    assert out.shape == (1, 7, 512 * G)
    assert prefills == [((4 * G, 7, 128), (4, 7, 128), (4, 7, 128))]
    if sinks:
        cos, sin = a.rotary_emb(v, 0, 7)
        k_rope = k * cos + at.rotate_half(k) * sin
        assert torch.equal(a.kcache_fp16, k_rope[:, :, :5].transpose(2, 3))
        assert torch.equal(a.vcache_fp16, v[:, :, :5])
        assert packs == [("k", (4, 128, 2)), ("v", (4, 128, 2))]
    else:
        assert packs == [("k", (4, 128, 7)), ("v", (4, 128, 7))]
    assert a.kcache.klen == 7 and a.vcache.vlen == 7

    tok = _randn_qkv(a, 1, torch.Generator().manual_seed(300 + G))
    out = a.attend(*tok)
    assert out.shape == (1, 1, 512 * G)
    assert len(decodes) == 1
    q_shape, sink_scores, k_sink, v_sink = decodes[0]
    assert q_shape == (4 * G, 128) and sink_scores is None
    assert (k_sink is not None) == (sinks > 0) and (v_sink is not None) == (sinks > 0)
    if sinks:
        assert k_sink.shape == (4, 128, 5) and v_sink.shape == (4, 5, 128)
    if G > 1:
        a.kcache.include_sparse = False
        with pytest.raises(ValueError):
            a.attend(*tok)
        assert len(decodes) == 1
