#!/usr/bin/env python
"""Draft verification over the compressed cache, per layer: one verify round (pack + chunk attention of S = 1 + draft
rows) with the grouped kernel (kvq_chunk_attention_grouped) and with the per-head kernel (KVQ_CHUNK_GROUPED=0, the
route before the grouped kernel existed), against the decode steps it replaces.  nuq4 + 1 % outliers, 32 query heads
over 8 and over 4 KV heads, no sink tokens, L0 = 131072 and 32768 cached tokens, S in {4, 8, 16, 32}.

Every time comes from HIP events around synchronised work; the two routes alternate inside one loop on the same caches
and each number is the median of --reps runs after one warm-up.  Per point:
  verify_grouped_ms / verify_heads_ms   pack + attention of the S rows, the two routes (and attn_*_ms: attention only)
  decode_steps_ms                       S decode_kv (GQA) steps
  decode_step_ms                        one such step
  grouped_over_heads                    verify_grouped / verify_heads (< 1: the grouped kernel wins)
  break_even_tokens                     verify_grouped / decode_step: tokens a round has to yield (accepted + 1) to pay

usage: python tools/spec_bench.py [--out FILE] [--reps N] [--quick]"""
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


def timed_alternating(fns, reps):
    """median seconds of each function of `fns`, run in turn reps + 1 times (the first turn is the warm-up)"""
    ts = [[] for _ in fns]
    for i in range(reps + 1):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i:
                ts[j].append(a.elapsed_time(b) * 1e-3)
    return [statistics.median(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_bench_mi355x.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="only 32 / 8 heads, L0 = 32768")
    args = ap.parse_args()
    dev = "cuda:0"
    Hq = 32
    L0s = [32768] if args.quick else [131072, 32768]
    Ss = [4, 8, 16, 32]
    rows = []
    for Hkv in ([8] if args.quick else [8, 4]):
        max_len = max(L0s) + max(Ss) + 64
        kc, vc, scale, shift = cc.make_caches(4, Hkv, max_len, device=dev)
        kp, vp = cc.tokens(max(L0s) + max(Ss), Hkv, scale, shift, dev, seed=11)
        cc.fill(kc, vc, kp[:, :, :max(L0s)], vp[:, :, :max(L0s)])
        for L0 in L0s:
            for S in Ss:
                q = cc.queries(Hq, S, dev, seed=13)
                k, v = kp[:, :, L0:L0 + S].contiguous(), vp[:, :, L0:L0 + S].contiguous()

                def verify(grouped):
                    def run():
                        ops.CHUNK_GROUPED = grouped
                        kc.klen = vc.vlen = L0
                        chunk_kv(kc, vc, q, k, v)
                    return run
                verify(True)()
                layer = layer_struct(kc, vc)

                def attn(grouped):
                    def run():
                        ops.CHUNK_GROUPED = grouped
                        ops.chunk_attention(layer, Hq, L0, q)
                    return run
                ops.CHUNK_GROUPED = True
                route = ops.chunk_attention_route(Hq, Hkv, S)
                t_vg, t_vh, t_ag, t_ah = timed_alternating([verify(True), verify(False), attn(True), attn(False)],
                                                           args.reps)
                ops.CHUNK_GROUPED = True
                qs = [q[:, i].contiguous() for i in range(S)]
                ks = [k[:, :, i].reshape(-1).contiguous() for i in range(S)]
                vs = [v[:, :, i].reshape(-1).contiguous() for i in range(S)]

                def steps(n):
                    def run():
                        kc.klen = vc.vlen = L0
                        for i in range(n):
                            decode_kv(kc, vc, qs[i], ks[i], vs[i])
                    return run
                t_steps, t_step = timed_alternating([steps(S), steps(1)], args.reps)
                kc.klen = vc.vlen = L0
                r = dict(Hq=Hq, Hkv=Hkv, G=Hq // Hkv, L0=L0, S=S, bits=4, route=route,
                         verify_grouped_ms=t_vg * 1e3, verify_heads_ms=t_vh * 1e3, attn_grouped_ms=t_ag * 1e3,
                         attn_heads_ms=t_ah * 1e3, decode_steps_ms=t_steps * 1e3, decode_step_ms=t_step * 1e3,
                         grouped_over_heads=t_vg / t_vh, attn_grouped_over_heads=t_ag / t_ah,
                         break_even_tokens=t_vg / t_step, break_even_tokens_heads=t_vh / t_step)
                rows.append(r)
                print(json.dumps(r), flush=True)
        del kc, vc, kp, vp
        torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
