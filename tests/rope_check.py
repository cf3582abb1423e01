"""Scaled RoPE over the compressed cache (kvquant_amd.rope): seeded caches filled with a prompt, one decode step or a
chunk with a frequency table, and the fp64 statement over the dequantised caches with the table's angles
fl32(inv_freq_j * pos) and the attention factor on the compressed keys.  Shared by tests/test_rope_gpu.py and
tools/gqa_bench.py / tools/chunk_bench.py (--rope)."""
import math

import torch

from tests import chunk_check as cc
from tests import gqa_check

HD = 128


def spec(kind, max_position_embeddings=None):
    """the RopeSpecs of the checks: LLaMA-3.1's llama3 parameters, YaRN factor 4 over 32K (theta 1e6), dynamic NTK"""
    from kvquant_amd import rope
    if kind == "llama3":
        return rope.spec_of(5e5, dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                      original_max_position_embeddings=8192))
    if kind == "yarn":
        return rope.spec_of(1e6, dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=32768))
    if kind == "dynamic":
        return rope.spec_of(1e4, dict(rope_type="dynamic", factor=2.0), max_position_embeddings)
    raise ValueError(kind)


def make(bits, Hkv, L0, extra, kind, sinks=0, seed=0, device="cuda", max_position_embeddings=None):
    """caches of Hkv heads holding L0 tokens (sinks of them in the fp16 side caches), a RopeSpec of `kind` (None: the
    default theta rule) and `extra` further tokens to feed.  Returns (kc, vc, k, v, k_sink, v_sink): k, v fp16 [Hkv, 128,
    extra] pre-RoPE."""
    kc, vc, scale, shift = cc.make_caches(bits, Hkv, L0 + extra + 64, sinks=sinks, device=device, seed=seed)
    if kind is not None:
        kc.rope = spec(kind, max_position_embeddings)
    kp, vp = cc.tokens(L0 - sinks + extra, Hkv, scale, shift, device, seed=seed + 11)
    n0 = L0 - sinks
    cc.fill(kc, vc, kp[:, :, :n0], vp[:, :, :n0])
    ks, vs = cc.sink_caches(Hkv, sinks, device, seed + 12) if sinks else (None, None)
    return kc, vc, kp[:, :, n0:].contiguous(), vp[:, :, n0:].contiguous(), ks, vs


def dequant(kc, vc, Lc, inv, af, heads=None):
    """(af * Khat rotated at fl32(inv_j * (sinks + column)), Vhat) f64 [len(heads), 128, Lc]"""
    H, bits, n = kc.num_heads, kc.bits, 2 ** kc.bits
    heads = list(range(H)) if heads is None else list(heads)
    ktab = kc.lookup_table2 if (kc.norm and bits == 2) else kc.lookup_table
    codes = gqa_check.unpack_codes(kc.kcache[:, :, :Lc], bits)
    kh = torch.gather(ktab.reshape(H, HD, n).double(), 2, codes).reshape(H * HD, Lc)
    kh.t().scatter_add_(1, kc.outlier_indices[:Lc].long(), kc.outliers[:Lc].double())
    kh = kh.reshape(H, HD, Lc)[heads]
    pos = torch.arange(Lc, device=kc.device, dtype=torch.float32) + kc.first_few_fp16
    ang = (inv.float()[:, None] * pos[None, :]).double()
    c, s = ang.cos() * af, ang.sin() * af
    lo, hi = kh[:, :64], kh[:, 64:]
    kr = torch.cat((c * lo - s * hi, s * lo + c * hi), dim=1)
    del kh, lo, hi, c, s
    vcodes = gqa_check.unpack_codes(vc.vcache[:, :, :Lc], bits)
    rows = vc.mix_table()[:Lc].double()
    vh = torch.gather(rows.t().unsqueeze(0).expand(H * HD, -1, -1), 1, vcodes.reshape(H * HD, 1, Lc)).reshape(H * HD, Lc)
    vh.t().scatter_add_(1, vc.outlier_indices[:Lc].long(), vc.outliers[:Lc].double())
    return kr, vh.reshape(H, HD, Lc)[heads]


def decode_reference(kc, vc, q16, L, inv, af, k_sink=None, v_sink=None, heads=None):
    """the decode step restated over L compressed columns (after the append), rounded like the reference (fp16 score,
    fp16 division by sqrt(128), fp32 softmax, fp16 probabilities), fp64 p.V; query head h reads KV head h // G.
    Returns f64 [len(heads), 128]."""
    Hq = q16.shape[0]
    G = Hq // kc.num_heads
    heads = list(range(Hq)) if heads is None else list(heads)
    kvh = sorted({h // G for h in heads})
    kr, vh = dequant(kc, vc, L, inv, af, kvh)
    out = torch.empty(len(heads), HD, dtype=torch.float64, device=q16.device)
    for j, h in enumerate(heads):
        i = kvh.index(h // G)
        sc = q16[h].double() @ kr[i]
        w = (sc.float().half() / math.sqrt(HD)).half()
        vv = vh[i]
        if k_sink is not None:
            ss = (q16[h].unsqueeze(0) @ k_sink[h // G]) / math.sqrt(HD)
            w = torch.cat((ss[0].half(), w))
        p = torch.softmax(w.float(), dim=-1).half()
        n = 0 if k_sink is None else k_sink.shape[2]
        o = (vv * p[None, n:].double()).sum(-1)
        if k_sink is not None:
            o = o + (p[:n].float() @ v_sink[h // G].float()).double()
        out[j] = o
    return out


def chunk_reference(kc, vc, q, c0, inv, af, k_sink=None, v_sink=None, heads=None, rows=None):
    """chunk_check.reference with the table's angles and the attention factor: f64 [len(rows), len(heads), 128]"""
    Hkv = kc.num_heads
    Hq, S, _ = q.shape
    G = Hq // Hkv
    heads = list(range(Hq)) if heads is None else list(heads)
    kvh = sorted({h // G for h in heads})
    kr, vh = dequant(kc, vc, c0 + S, inv, af, kvh)
    rows = torch.arange(S, device=q.device) if rows is None else torch.as_tensor(rows, device=q.device)
    col = torch.arange(c0 + S, device=q.device)
    mask = col[None, :] > (c0 + rows)[:, None]
    out = torch.empty(len(rows), len(heads), HD, dtype=torch.float64, device=q.device)
    for j, h in enumerate(heads):
        i = kvh.index(h // G)
        qh = q[h, rows].double()
        sc = ((qh @ kr[i]) / math.sqrt(HD)).masked_fill(mask, float("-inf"))
        vv = vh[i].t()
        if k_sink is not None:
            sc = torch.cat(((qh @ k_sink[h // G].double()) / math.sqrt(HD), sc), dim=1)
            vv = torch.cat((v_sink[h // G].double(), vv), dim=0)
        out[:, j] = torch.softmax(sc, dim=-1) @ vv
    return out


def decode_step(kc, vc, q16, k, v, k_sink=None, v_sink=None):
    """one decode_kv step of the first of the fed tokens: out f32 [Hq, 128]"""
    from kvquant_amd.cache import decode_kv
    ki = k[:, :, 0].reshape(-1).contiguous()
    vi = v[:, :, 0].reshape(-1).contiguous()
    if k_sink is not None:
        out, _ = decode_kv(kc, vc, q16, ki, vi, k_sink=k_sink, v_sink=v_sink)
    else:
        out, _ = decode_kv(kc, vc, q16, ki, vi)
    return out[0]


def check_decode(got, ref, what, tol=1e-3):
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    print("%s: rel err %.2e" % (what, err))
    assert err < tol, "%s: %.3e" % (what, err)
    return err
