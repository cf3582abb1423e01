"""Grouped-query attention decode benchmark: LLaMA-3-8B's KV shape (32 query heads, 8 KV heads, head_dim 128),
nuq4 + 1 % outliers by default, 32 layers, batch 1, seeded random compressed caches of L tokens.  Per context
length: ms per decode step of the KV path (32 x kvq_decode_step_gqa through cache.decode_kv), tokens/s, per-layer us of
the grouped q.K^T and p.V launches (library events, as bench.py takes them), algorithmic bytes of the two kernels and
their fraction of 8 TB/s, and the same step for the MHA-expanded equivalent (decode_kv over 32-head caches of the same
length: what a model with its KV heads repeated runs without GQA support).  Prints ONE JSON line.

    python tools/gqa_bench.py [--ctx 4096,32768,131072] [--extra-bits 3,2] [--steps 8] [--warmup 3] [--layers 32]
                              [--rope llama3]
--rope llama3 (or yarn): the grouped step is timed once more with every layer's cache rotating with that scaled-RoPE
table (tests/rope_check.py spec; LLaMA-3.1's parameters): rope_gqa_ms_per_step and its ratio to the theta rule."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM = 8e12


def synth_quantizer(bits, C, gen, dev):
    """bench.py's synthetic quantizer at C channels: per-channel 0.5 / 99.5 % thresholds of a scaled normal, centroids
    at normal quantiles"""
    scale = torch.exp(0.5 * torch.randn(C, generator=gen, device=dev))
    shift = 0.3 * torch.randn(C, generator=gen, device=dev)
    upper = (shift + 2.576 * scale).cpu().numpy()[None, :]
    lower = (shift - 2.576 * scale).cpu().numpy()[None, :]
    n = 2 ** bits
    c = torch.special.ndtri((torch.arange(n, dtype=torch.float64) + 0.5) / n)
    c = (c / c.abs().max() * 0.97).float().numpy().reshape(n, 1)
    return (upper, lower, [c]), scale, shift


def synth_tokens(S, scale, shift, gen, dev):
    """bench.py's synthetic activations: scaled normal keys, normal values, 1 % of the entries x6"""
    C = scale.numel()
    k = torch.randn(S, C, generator=gen, device=dev) * scale + shift
    v = torch.randn(S, C, generator=gen, device=dev)
    k = torch.where(torch.rand(S, C, generator=gen, device=dev) < 0.01, k * 6.0, k)
    v = torch.where(torch.rand(S, C, generator=gen, device=dev) < 0.01, v * 6.0, v)
    return k.half(), v.half()


def make_layer(bits, H, L, max_len, seed, dev, chunk=8192):
    """a layer's caches holding L synthetic tokens packed by the library's own prefill pack (as bench.py fills its
    caches: realistic codes, outlier rows and per-token codebook rows)"""
    from kvquant_amd.cache import QuantK, QuantV
    C = H * 128
    g = torch.Generator(device=dev).manual_seed(seed)
    quant, scale, shift = synth_quantizer(bits, C, g, dev)
    kw = dict(bits=bits, hidden_size=C, num_heads=H, max_position_embeddings=max_len, include_sparse=True,
              sparsity_threshold=0.99, first_few_fp16=0)
    kc, vc = QuantK(rope_theta=500000.0, device=dev, **kw), QuantV(device=dev, **kw)
    kc.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99)
    vc.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99)
    done = 0
    while done < L:
        S = min(chunk, L - done)
        k, v = synth_tokens(S, scale, shift, g, dev)
        kc.parallel_pack(k.view(S, H, 128).permute(1, 2, 0))
        vc.parallel_pack(v.view(S, H, 128).permute(1, 2, 0))
        done += S
    return kc, vc, scale, shift


class Events:
    """library events (kvq_decode_step_events: before / after q.K^T, before / after p.V) of one layer call per step"""

    def __init__(self, n):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.quads = []
        for _ in range(n):
            q = (ctypes.c_void_p * 4)()
            for i in range(4):
                e = ctypes.c_void_p()
                assert self.hip.hipEventCreate(ctypes.byref(e)) == 0
                q[i] = e
            self.quads.append(q)

    def arm(self, i):
        from kvquant_amd import _lib
        _lib.lib().kvq_decode_step_events(self.quads[i])

    def us(self, i, a, b):
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.quads[i][a], self.quads[i][b]) == 0
        return ms.value * 1000.0


def run_step(layers, Hq, steps, warmup, dev, kernel_events):
    """warmup + steps decode tokens through every layer.  Returns ms per step (no synchronisation inside the timed
    region), the mean whole-layer time (torch events around one layer call per step: append, q.K^T, softmax, p.V and
    everything between them) and, with kernel_events, the mean q.K^T and p.V times from the library's events."""
    from kvquant_amd.cache import decode_kv
    g = torch.Generator(device=dev).manual_seed(9)
    n = warmup + steps
    q = torch.randn(n, Hq, 128, generator=g, device=dev).half()
    toks = [synth_tokens(n, sc, sh, g, dev) for (_, _, sc, sh) in layers]
    ev = Events(steps) if kernel_events else None
    le = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for it in range(n):
        if it == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for i, (kc, vc, _, _) in enumerate(layers):
            k, v = toks[i][0][it], toks[i][1][it]
            timed = it >= warmup and i == it % len(layers)
            if timed:
                j = it - warmup
                if ev:
                    ev.arm(j)
                le[j][0].record()
            decode_kv(kc, vc, q[it], k, v)
            if timed:
                le[j][1].record()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1000.0 / steps
    layer_us = sum(a.elapsed_time(b) for a, b in le) * 1000.0 / steps
    if not ev:
        return ms, layer_us, None, None
    qk = sum(ev.us(j, 0, 1) for j in range(steps)) / steps
    pv = sum(ev.us(j, 2, 3) for j in range(steps)) / steps
    return ms, layer_us, qk, pv


def alg_bytes(bits, Hkv, L, n_out):
    k = Hkv * L * 16 * bits + L * n_out * 8          # packed K words + K outlier mirror (value + index)
    v = Hkv * L * 16 * bits + L * n_out * 8 + L * (2 ** bits) * 4   # packed V + V outlier rows + per-token codebook rows
    return k, v


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", default="4096,32768,131072")
    ap.add_argument("--extra-bits", default="3,2", help="widths measured at the longest context besides 4 bit")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--no-mha", action="store_true")
    ap.add_argument("--rope", default=None, help="also time the grouped step with this scaled RoPE (llama3, yarn)")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    Hq, Hkv = 32, 8
    ctxs = [int(x) for x in a.ctx.split(",") if x]
    runs = [(4, L) for L in ctxs] + [(int(b), max(ctxs)) for b in a.extra_bits.split(",") if b]
    lines = []
    for bits, L in runs:
        # (a multiple of 256, as bench.py's: the MHA p.V kernel takes max_len % 4 == 0 only, other lengths run its slow fallback)
        max_len = (L + 2 * (a.warmup + a.steps) + 8 + 255) // 256 * 256
        rec = {"bits": bits, "ctx": L, "Hq": Hq, "Hkv": Hkv, "layers": a.layers}
        layers = [make_layer(bits, Hkv, L, max_len, 100 + i, dev) for i in range(a.layers)]
        n_out = layers[0][0].num_outliers
        ms, lay, qk, pv = run_step(layers, Hq, a.steps, a.warmup, dev, True)
        kb, vb = alg_bytes(bits, Hkv, L, n_out)
        rec.update(gqa_ms_per_step=round(ms, 3), gqa_tokens_per_s=round(1000.0 / ms, 1), gqa_layer_us=round(lay, 2),
                   gqa_qk_us=round(qk, 2), gqa_pv_us=round(pv, 2), alg_bytes_qk=kb, alg_bytes_pv=vb,
                   frac_8tbs_qk=round(kb / (qk * 1e-6) / HBM, 3), frac_8tbs_pv=round(vb / (pv * 1e-6) / HBM, 3))
        if a.rope:
            from tests import rope_check
            spec = rope_check.spec(a.rope)
            for kc, _, _, _ in layers:
                kc.rope = spec
            ms_r, lay_r, qk_r, _ = run_step(layers, Hq, a.steps, a.warmup, dev, True)
            rec.update(rope=a.rope, rope_gqa_ms_per_step=round(ms_r, 3), rope_gqa_qk_us=round(qk_r, 2),
                       rope_over_theta=round(ms_r / ms, 4))
        del layers
        torch.cuda.empty_cache()
        if not a.no_mha:
            # (MHA: the library's q.K^T events are comparable; its p.V route records event 2 inside the fused softmax
            #  launch, so only the whole layer is reported for the p.V side)
            layers = [make_layer(bits, Hq, L, max_len, 200 + i, dev) for i in range(a.layers)]
            ms2, lay2, qk2, _ = run_step(layers, Hq, a.steps, a.warmup, dev, True)
            rec.update(mha_ms_per_step=round(ms2, 3), mha_tokens_per_s=round(1000.0 / ms2, 1), mha_layer_us=round(lay2, 2),
                       mha_qk_us=round(qk2, 2), gqa_over_mha=round(ms / ms2, 3), gqa_over_mha_layer=round(lay / lay2, 3))
            del layers
            torch.cuda.empty_cache()
        lines.append(rec)
        print("# " + json.dumps(rec), file=sys.stderr, flush=True)
    prop = torch.cuda.get_device_properties(0)
    print(json.dumps({"tool": "gqa_bench", "device": prop.name, "arch": getattr(prop, "gcnArchName", ""),
                      "cus": prop.multi_processor_count, "runs": lines}))


if __name__ == "__main__":
    main()
