"""Chunk attention over the compressed cache (cache.chunk_kv / kvq_chunk_attention): seeded caches filled with a
prompt, the fp64 torch statement of the chunk semantics over the dequantised cache, and twin caches fed token by token
through decode_kv.  Shared by tests/test_chunk_attn_gpu.py and tools/chunk_bench.py."""
import math

import torch

from tests import decode_check, gqa_check

HD = 128


def make_caches(bits, Hkv, max_len, sinks=0, norm=False, device="cuda", seed=0):
    """(QuantK, QuantV) over Hkv heads with the seeded quantizer of tests/decode_check.py"""
    from kvquant_amd.cache import QuantK, QuantV
    C = Hkv * HD
    quant, scale, shift = decode_check.quantizer(bits, seed=seed + bits, C=C)
    if norm:
        quant = tuple(quant) + (torch.tensor(1.07), torch.tensor(-0.02))
    kw = dict(bits=bits, hidden_size=C, num_heads=Hkv, max_position_embeddings=max_len, include_sparse=True,
              sparsity_threshold=0.99, first_few_fp16=sinks, device=device)
    kc, vc = QuantK(rope_theta=10000.0, **kw), QuantV(**kw)
    kc.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99, norm=norm)
    vc.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99, norm=norm)
    return kc, vc, scale.to(device), shift.to(device)


def tokens(n, Hkv, scale, shift, device, seed):
    """fp16 pre-RoPE keys [Hkv, 128, n] (per-channel scale / shift, heavy tails) and values [Hkv, 128, n]"""
    g = torch.Generator(device=device).manual_seed(seed)
    C = Hkv * HD
    k = torch.randn(n, C, generator=g, device=device) * scale + shift
    k = k + (torch.rand(n, C, generator=g, device=device) < 0.004) * torch.randn(n, C, generator=g, device=device) * 8
    v = torch.randn(n, C, generator=g, device=device) + 0.3
    v = v + (torch.rand(n, C, generator=g, device=device) < 0.004) * torch.randn(n, C, generator=g, device=device) * 6
    k, v = k.half(), v.half()
    return k.t().reshape(Hkv, HD, n).contiguous(), v.t().reshape(Hkv, HD, n).contiguous()


def sink_caches(Hkv, sinks, device, seed):
    """fp16 sink caches: post-RoPE K [Hkv, 128, sinks], V [Hkv, sinks, 128]"""
    g = torch.Generator(device=device).manual_seed(seed)
    ks = (torch.randn(Hkv, HD, sinks, generator=g, device=device) * 1.5).half()
    vs = (torch.randn(Hkv, sinks, HD, generator=g, device=device) + 0.3).half()
    return ks, vs


def fill(kc, vc, k, v):
    """the prompt's compressed tokens (behind the caches' sink tokens, which count in klen) via parallel_pack"""
    kc.klen = vc.vlen = kc.first_few_fp16
    kc.parallel_pack(k.float())
    vc.parallel_pack(v.float())


def queries(Hq, S, device, seed, scale=0.35):
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(Hq, S, HD, generator=g, device=device) * scale).half()


def dequant(kc, vc, Lc):
    """(Khat rotated at each column's position, Vhat) f64 [Hkv, 128, Lc] of the packed caches: the score / mix tables
    of the decode kernels + the outlier residuals of the reference rows, angles fl32(theta_j * (sinks + column))"""
    from kvquant_amd import ops
    H, bits, n = kc.num_heads, kc.bits, 2 ** kc.bits
    ktab = kc.lookup_table2 if (kc.norm and bits == 2) else kc.lookup_table
    codes = gqa_check.unpack_codes(kc.kcache[:, :, :Lc], bits)
    kh = torch.gather(ktab.reshape(H, HD, n).double(), 2, codes).reshape(H * HD, Lc)
    kh.t().scatter_add_(1, kc.outlier_indices[:Lc].long(), kc.outliers[:Lc].double())
    kh = kh.reshape(H, HD, Lc)
    th = ops.rope_freqs(kc.rope_theta, device=kc.device)
    pos = torch.arange(Lc, device=kc.device, dtype=torch.float32) + kc.first_few_fp16
    ang = (th[:, None] * pos[None, :]).double()
    c, s = ang.cos(), ang.sin()
    lo, hi = kh[:, :64], kh[:, 64:]
    kr = torch.cat((c * lo - s * hi, s * lo + c * hi), dim=1)
    vcodes = gqa_check.unpack_codes(vc.vcache[:, :, :Lc], bits)
    rows = vc.mix_table()[:Lc].double()                                        # [Lc, n]
    vh = torch.gather(rows.t().unsqueeze(0).expand(H * HD, -1, -1), 1, vcodes.reshape(H * HD, 1, Lc)).reshape(H * HD, Lc)
    vh.t().scatter_add_(1, vc.outlier_indices[:Lc].long(), vc.outliers[:Lc].double())
    return kr, vh.reshape(H, HD, Lc)


def reference(kc, vc, q, c0, k_sink=None, v_sink=None, heads=None, rows=None):
    """fp64 statement of the chunk semantics: query i of q [Hq, S, 128] over the sink tokens and compressed columns
    [0, c0 + i].  heads / rows: the subset to evaluate (default all).  Returns f64 [len(rows), len(heads), 128]."""
    Hkv = kc.num_heads
    Hq, S, _ = q.shape
    G = Hq // Hkv
    Lc = c0 + S
    kr, vh = dequant(kc, vc, Lc)
    heads = list(range(Hq)) if heads is None else list(heads)
    rows = torch.arange(S, device=q.device) if rows is None else torch.as_tensor(rows, device=q.device)
    col = torch.arange(Lc, device=q.device)
    mask = col[None, :] > (c0 + rows)[:, None]                                  # [R, Lc]
    out = torch.empty(len(rows), len(heads), HD, dtype=torch.float64, device=q.device)
    for j, h in enumerate(heads):
        hk = h // G
        qh = q[h, rows].double()                                                # [R, 128]
        sc = (qh @ kr[hk]) / math.sqrt(HD)
        sc = sc.masked_fill(mask, float("-inf"))
        vv = vh[hk].t()                                                         # [Lc, 128]
        if k_sink is not None:
            sc = torch.cat(((qh @ k_sink[hk].double()) / math.sqrt(HD), sc), dim=1)
            vv = torch.cat((v_sink[hk].double(), vv), dim=0)
        out[:, j] = torch.softmax(sc, dim=-1) @ vv
    return out


def check(got, ref, what):
    """the bars of tests/test_prefill_attn_gpu.py: per output row max |delta| <= 2e-3 x row max, |mean signed error|
    < 1e-4 of the largest output; returns (worst row ratio, bias, worst fp16 ulps)"""
    got = got.double()
    d = (got - ref).abs().amax(dim=-1)
    m = ref.abs().amax(dim=-1)
    worst = float((d / m.clamp_min(1e-30)).max())
    bias = float((got - ref).mean() / ref.abs().max())
    ulps = float(gqa_check.fp16_ulps(got.float(), ref.float()).max())
    print("%s: row err %.2e, bias %.1e, max %.1f fp16 ulps" % (what, worst, bias, ulps))
    assert worst <= 2e-3, "%s: row error %.3e" % (what, worst)
    assert abs(bias) < 1e-4, "%s: bias %.3e" % (what, bias)
    return worst, bias, ulps


def decode_twin(kc, vc, q, k, v, k_sink=None, v_sink=None):
    """the same chunk fed token by token through decode_kv (the q_len == 1 path): f32 [S, Hq, 128]"""
    from kvquant_amd.cache import decode_kv
    S = q.shape[1]
    outs = []
    for i in range(S):
        ki = k[:, :, i].reshape(-1).contiguous()
        vi = v[:, :, i].reshape(-1).contiguous()
        qi = q[:, i].contiguous()
        if k_sink is not None:
            o, _ = decode_kv(kc, vc, qi, ki, vi, k_sink=k_sink, v_sink=v_sink)
        else:
            o, _ = decode_kv(kc, vc, qi, ki, vi)
        outs.append(o[0])
    return torch.stack(outs)
