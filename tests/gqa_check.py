"""Grouped-query attention (GQA) checks shared by tests/test_gqa_gpu.py and tools/gqa_bench.py: seeded random
compressed caches of Hkv KV heads, and the grouped kernels against the pinned MHA kernels run once per group member
(query head kv * G + g reads KV head kv)."""
import numpy as np
import torch

HD = 128


def random_cache(bits, Hkv, L, max_len, n_out, device, seed=0, edge_rows=True):
    """packed K / V words, K table [Hkv, 128, 2^bits], V rows [max_len, 2^bits], K outlier mirror [n_out, max_len] and
    V outlier rows [max_len, n_out] (global channels ascending per token, some capped-away zero entries).  edge_rows:
    token 0 has entries at the first and last channel of every KV head it can reach, token 1 all entries in the last
    KV head."""
    g = torch.Generator(device=device).manual_seed(seed)
    W = HD // 32 * bits
    C = Hkv * HD
    kmat = torch.randint(-2 ** 31, 2 ** 31 - 1, (Hkv, W, max_len), generator=g, device=device, dtype=torch.int64).to(torch.int32)
    vmat = torch.randint(-2 ** 31, 2 ** 31 - 1, (Hkv, W, max_len), generator=g, device=device, dtype=torch.int64).to(torch.int32)
    klut = torch.randn(Hkv, HD, 2 ** bits, generator=g, device=device)
    # (per-token codebook rows lut * sf + off with off > 0 on average, as value rows of real activations often are: the
    #  attention outputs keep the scale of the values instead of cancelling to ~1/sqrt(L) of it)
    vrows = 0.5 * torch.randn(max_len, 2 ** bits, generator=g, device=device) + 1.0
    idx = torch.randint(0, C, (max_len, n_out), generator=g, device=device, dtype=torch.int32).sort(dim=1).values
    val = torch.randn(max_len, n_out, generator=g, device=device)
    val = torch.where(torch.rand(max_len, n_out, generator=g, device=device) < 0.1, torch.zeros_like(val), val)
    if edge_rows and max_len >= 2:
        e = []
        for kv in range(Hkv):
            e += [kv * HD, kv * HD + HD - 1]
        e = (e * n_out)[:n_out]
        idx[0] = torch.tensor(sorted(e), dtype=torch.int32, device=device)
        last = (Hkv - 1) * HD
        idx[1] = torch.tensor(sorted(last + (np.arange(n_out) * 37) % HD), dtype=torch.int32, device=device)
    vidx = torch.randint(0, C, (max_len, n_out), generator=g, device=device, dtype=torch.int32).sort(dim=1).values
    vval = torch.randn(max_len, n_out, generator=g, device=device)
    if edge_rows and max_len >= 2:
        vidx[0], vidx[1] = idx[0], idx[1]
    return dict(kmat=kmat, vmat=vmat, klut=klut, vrows=vrows, kout_t=val.t().contiguous(), kidx_t=idx.t().contiguous(),
                vout=vval, vidx=vidx)


def fp16_ulps(a, b):
    """element-wise difference of a and b after rounding both to fp16, in fp16 ulps of the larger magnitude"""
    a16 = a.half().float().cpu().numpy()
    b16 = b.half().float().cpu().numpy()
    sp = np.spacing(np.maximum(np.abs(a16), np.abs(b16)).astype(np.float16)).astype(np.float32)
    return np.abs(a16 - b16) / sp


def check_rows(got, ref, what, rel=1e-5, scale=None, ulp_floor=1.0 / 64):
    """max |delta| <= rel * max |row| per row, and no element more than one fp16 ulp apart after rounding.  A row of
    fewer than 16 scores is measured against the largest score of the slice (all KV heads): a single score that is a
    cancellation of 128 terms carries the rounding of its terms, not of its own magnitude, in any summation order."""
    d = (got - ref).abs().amax(dim=-1)
    m = ref.abs().amax(dim=-1) if scale is None else scale.abs().amax(dim=-1)
    if ref.shape[-1] < 16 and scale is None:
        m = torch.full_like(m, float(ref.abs().max()))
    bad = d > rel * m + 1e-30
    assert not bool(bad.any()), "%s: row error %.3e" % (what, float((d / m.clamp_min(1e-30)).max()))
    # (fp16 ulps are compared where they measure the sum's rounding: at 1/64 of the row's largest score and above --
    #  a near-zero score is a cancellation whose absolute error is that of its terms, bounded by the bar above)
    u = fp16_ulps(got, ref)
    big = (ref.abs() >= m.unsqueeze(-1) * ulp_floor).cpu().numpy()
    worst = float(u[big].max()) if big.any() else 0.0
    assert worst <= 1.0, "%s: %.1f fp16 ulps" % (what, worst)


def score_against_mha(bits, Hkv, G, L, max_len=None, n_out=12, pos_offset=0, device="cuda", seed=0):
    from kvquant_amd import ops
    max_len = max_len or L
    c = random_cache(bits, Hkv, L, max_len, n_out, device, seed)
    Hq = Hkv * G
    q = torch.randn(Hq, HD, generator=torch.Generator(device=device).manual_seed(seed + 1), device=device)
    got = torch.empty(Hq, L, device=device)
    ops.score_k_gqa(bits, q, c["kmat"], got, c["klut"], L, 10000.0, pos_offset, c["kout_t"], c["kidx_t"])
    for g in range(G):
        qg = q.view(Hkv, G, HD)[:, g].contiguous().unsqueeze(0)
        ref = torch.empty(1, Hkv, L, device=device)
        ops.score_k_mirror(bits, qg, c["kmat"], ref, c["klut"], L, 10000.0, pos_offset, c["kout_t"], c["kidx_t"],
                           accumulate=False)
        check_rows(got.view(Hkv, G, L)[:, g], ref[0], "score g=%d" % g)


def mix_against_mha(bits, Hkv, G, L, max_len=None, n_out=12, device="cuda", seed=0):
    from kvquant_amd import ops
    max_len = max_len or L
    c = random_cache(bits, Hkv, L, max_len, n_out, device, seed)
    Hq = Hkv * G
    p = torch.rand(Hq, L, generator=torch.Generator(device=device).manual_seed(seed + 2), device=device)
    p = (p / p.sum(dim=1, keepdim=True)).half().float().contiguous()
    got = torch.empty(Hq, HD, device=device)
    ops.mix_v_gqa(bits, p, c["vmat"], got, c["vrows"], L, c["vout"], c["vidx"])
    for g in range(G):
        pg = p.view(Hkv, G, L)[:, g].contiguous().unsqueeze(0)
        ref = torch.empty(1, Hkv, HD, device=device)
        ops.mix_v(bits, pg, c["vmat"], ref, c["vrows"], L, c["vout"], c["vidx"], accumulate=False)
        check_rows(got.view(Hkv, G, HD)[:, g], ref[0], "mix g=%d" % g, ulp_floor=0.0)   # (every element: the bars of the issue)


def unpack_codes(mat, bits):
    """codes [H, 128, L] of a packed cache [H, 128/32*bits, L]: code i of a 32-channel group is bits [bits*i, bits*i + bits)
    of the group's little-endian word concatenation (the layouts of KCU:1240-1244, 1395-1424, 2712-2716)"""
    H, W, L = mat.shape
    w = mat.to(torch.int64) & 0xffffffff
    out = torch.empty(H, 128, L, dtype=torch.int64, device=mat.device)
    mask = (1 << bits) - 1
    for grp in range(4):
        for i in range(32):
            st = bits * i
            k, off = st // 32, st % 32
            v = w[:, grp * bits + k] >> off
            if off + bits > 32:
                v = v | (w[:, grp * bits + k + 1] << (32 - off))
            out[:, grp * 32 + i] = v & mask
    return out


def dequant_k(ok, L):
    """Khat [H, 128, L] f64 of an oracle K cache: per-channel table value + the token's outlier residuals"""
    H, n = ok.num_heads, 2 ** ok.bits
    codes = unpack_codes(ok.kcache[:, :, :L], ok.bits)
    lut = ok.lookup_table.reshape(H, 128, n).double()
    kh = torch.gather(lut, 2, codes).reshape(H * 128, L)
    kh.t().scatter_add_(1, ok.outlier_indices[:L].long(), ok.outliers[:L].double())
    return kh.reshape(H, 128, L)


def dequant_v(ov, L):
    """Vhat [H, 128, L] f64 of an oracle V cache: the token's codebook row value + its outlier residuals"""
    H = ov.num_heads
    codes = unpack_codes(ov.vcache[:, :, :L], ov.bits)
    rows = ov.lookup_table[:L].double()                                    # [L, n]
    vh = torch.gather(rows.t().unsqueeze(0).expand(H * 128, -1, -1), 1, codes.reshape(H * 128, 1, L)).reshape(H * 128, L)
    vh.t().scatter_add_(1, ov.outlier_indices[:L].long(), ov.outliers[:L].double())
    return vh.reshape(H, 128, L)


def attention_fp64(khat, vhat, q16, G, thetas, pos0, sink_scores=None, v_sink=None):
    """the decode attention restated in torch over dequantised caches with the KV heads repeated per group
    (repeat_interleave(G)): fp64 scores with the kernels' angles fl32(theta_j * pos), rounded like the reference
    (half(score) / sqrt(hd) in fp16, fp32 softmax, fp16 probabilities), fp64 p.V (+ fp16 sink tokens)"""
    import math
    H, _, L = khat.shape
    kr = khat.repeat_interleave(G, 0)                                      # [Hq, 128, L]
    vr = vhat.repeat_interleave(G, 0)
    pos = (torch.arange(L, dtype=torch.float32) + pos0)
    ang = (thetas.float().unsqueeze(1) * pos.unsqueeze(0)).double()        # [64, L]
    c, s = ang.cos(), ang.sin()
    q = q16.double()                                                       # [Hq, 128]
    lo, hi = kr[:, :64], kr[:, 64:]
    sc = (q[:, :64, None] * (c * lo - s * hi) + q[:, 64:, None] * (s * lo + c * hi)).sum(1)   # [Hq, L]
    w = (sc.float().half() / math.sqrt(128)).half()
    if sink_scores is not None:
        w = torch.cat([sink_scores.cpu(), w], dim=1)
    p = torch.softmax(w.float(), dim=-1).half()
    n = 0 if sink_scores is None else sink_scores.shape[1]
    out = (vr * p[:, None, n:].double()).sum(-1)                           # [Hq, 128]
    if v_sink is not None:
        out = out + torch.matmul(p[:, None, :n].float(), v_sink.cpu().float())[:, 0].double()
    return out
