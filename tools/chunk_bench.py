#!/usr/bin/env python
"""Chunk attention over the compressed cache, per layer: pack + kvq_chunk_attention of S new tokens on a cache of L0
tokens, against S sequential decode_kv steps (the token-by-token route).  nuq4 + 1 % outliers, 32 query heads over 32
(MHA) or 8 (GQA) KV heads, no sink tokens.

Every time comes from HIP events around synchronised work (median of --reps runs after one warm-up).  Above 64 steps
the decode route is timed for 64 steps and scaled to S (its step time grows by S / L0 over the chunk, < 2 % at
L0 >= 32K and S <= 512; the rows say so with "decode_scaled_from").  The attention FLOP rate counts the two products
of the causal chunk, 4 * S * (L0 + S / 2) * 128 * Hq, against the 2.5 PF of the fp16 matrix cores.

--rope llama3 (or yarn): every row also times kvq_chunk_attention with that scaled-RoPE table (tests/rope_check.py
spec; LLaMA-3.1's parameters) -- attn_ms_rope and its ratio to the theta rule.

usage: python tools/chunk_bench.py [--out FILE] [--reps N] [--quick] [--rope llama3]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kvquant_amd import ops  # noqa: E402
from kvquant_amd.cache import chunk_kv, decode_kv, layer_struct  # noqa: E402
from tests import chunk_check as cc  # noqa: E402

PEAK = 2.5e15
DECODE_MAX_STEPS = 64


def timed(fn, reps):
    ts = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i:
            ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="only L0 = 131072, S = 512, MHA (the acceptance row)")
    ap.add_argument("--rope", default=None, help="also time the chunk attention with this scaled RoPE (llama3, yarn)")
    args = ap.parse_args()
    rope_spec = None
    if args.rope:
        from tests import rope_check
        rope_spec = rope_check.spec(args.rope)
    dev = "cuda:0"
    Hq = 32
    L0s = [131072] if args.quick else [4096, 32768, 131072]
    Ss = [512] if args.quick else [16, 128, 512, 2048]
    rows = []
    for Hkv in ([32] if args.quick else [32, 8]):
        max_len = max(L0s) + max(Ss) + 64
        kc, vc, scale, shift = cc.make_caches(4, Hkv, max_len, device=dev)
        kp, vp = cc.tokens(max(L0s) + max(Ss), Hkv, scale, shift, dev, seed=11)
        cc.fill(kc, vc, kp[:, :, :max(L0s)], vp[:, :, :max(L0s)])
        for L0 in L0s:
            for S in Ss:
                q = cc.queries(Hq, S, dev, seed=13)
                k, v = kp[:, :, L0:L0 + S].contiguous(), vp[:, :, L0:L0 + S].contiguous()

                def chunk():
                    kc.klen = vc.vlen = L0
                    chunk_kv(kc, vc, q, k, v)
                t_chunk = timed(chunk, args.reps)
                layer = layer_struct(kc, vc)

                def attn_only():
                    ops.chunk_attention(layer, Hq, L0, q)
                t_attn = timed(attn_only, args.reps)
                t_rope = None
                if rope_spec is not None:
                    tab = rope_spec.table(dev, L0 + S)

                    def attn_rope():
                        ops.chunk_attention(layer, Hq, L0, q, rope=tab)
                    t_rope = timed(attn_rope, args.reps)
                n = min(S, DECODE_MAX_STEPS)
                qs = [q[:, i].contiguous() for i in range(n)]
                ks = [k[:, :, i].reshape(-1).contiguous() for i in range(n)]
                vs = [v[:, :, i].reshape(-1).contiguous() for i in range(n)]

                def steps():
                    kc.klen = vc.vlen = L0
                    for i in range(n):
                        decode_kv(kc, vc, qs[i], ks[i], vs[i])
                t_dec = timed(steps, max(1, args.reps // 2)) * S / n
                kc.klen = vc.vlen = L0
                flop = 4.0 * S * (L0 + S / 2) * 128 * Hq
                r = dict(Hq=Hq, Hkv=Hkv, L0=L0, S=S, bits=4, pack_plus_attn_ms=t_chunk * 1e3, attn_ms=t_attn * 1e3,
                         attn_pflops=flop / t_attn / 1e15, attn_share_of_2p5pf=flop / t_attn / PEAK,
                         decode_steps_ms=t_dec * 1e3, decode_scaled_from=n if n < S else None,
                         speedup_vs_decode=t_dec / t_chunk)
                if t_rope is not None:
                    r.update(rope=args.rope, attn_ms_rope=t_rope * 1e3, rope_over_theta=t_rope / t_attn)
                rows.append(r)
                print(json.dumps(r), flush=True)
        del kc, vc, kp, vp
        torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
