#!/usr/bin/env python
"""Sliding-window attention on ring caches, per layer: nuq4 + 1 % outliers, 32 query heads over 8 KV heads, no sink
tokens, windows W = 4096 and 32768 with the default slack of 256 (rings of 4352 / 33024 columns, wrapped twice before
anything is timed).

(a) one decode token on the ring -- pack + kvq_chunk_attention_window, S = 1 (cache.chunk_kv) -- against decode_kv over
    a LINEAR cache that holds W tokens after the append: the GQA decode step at the same resident length;
(b) chunks of S = 16 and S = 257 (= capacity - window + 1) on the ring against plain chunk_kv at c0 = W on a linear cache.

The two sides of a comparison alternate in one process; a timed window is --inner calls between two HIP events around
synchronised work, the figure the median of --reps windows after --warmup untimed ones.  ratio = ring / linear.

usage: python tools/window_bench.py [--out FILE] [--reps N] [--inner N] [--warmup N] [--windows 4096,32768]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kvquant_amd.attention import window_capacity  # noqa: E402
from kvquant_amd.cache import chunk_kv, decode_kv  # noqa: E402
from tests import chunk_check as cc  # noqa: E402
from tests import window_check as wc  # noqa: E402


def window_ms(fn, inner):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def alternate(f, g, reps, warmup, inner):
    """medians (ms per call) of f and g, their timed windows alternating"""
    tf, tg = [], []
    for i in range(warmup + reps):
        x, y = window_ms(f, inner), window_ms(g, inner)
        if i >= warmup:
            tf.append(x)
            tg.append(y)
    return statistics.median(tf), statistics.median(tg), (min(tf), max(tf)), (min(tg), max(tg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--windows", default="4096,32768")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_bench needs a GPU (no CPU fallback)")
    dev, Hq, Hkv, bits = "cuda:0", 32, 8, 4
    rows = []
    for W in [int(x) for x in args.windows.split(",")]:
        C = window_capacity(W, 256)
        rk, rv, scale, shift = wc.make_ring(bits, Hkv, C, W, device=dev)
        lk, lv, _, _ = wc.make_ring(bits, Hkv, (W + 257 + 63) & ~63, W, device=dev, window=False)
        kp, vp = cc.tokens(C, Hkv, scale, shift, dev, seed=11)
        N0 = 2 * C + 100                                   # tokens on the ring before a timed call: wrapped twice
        for n in (C, C, 100):
            rk.parallel_pack(kp[:, :, :n].float())
            rv.parallel_pack(vp[:, :, :n].float())
        assert rk.klen == N0 and rk.high_water == N0
        lk.parallel_pack(kp[:, :, :W].float())             # the linear cache: W tokens, later calls rewrite what follows
        lv.parallel_pack(vp[:, :, :W].float())
        for S in (1, 16, 257):
            q = cc.queries(Hq, S, dev, seed=13)
            k, v = kp[:, :, 200:200 + S].contiguous(), vp[:, :, 200:200 + S].contiguous()

            def ring():
                rk.klen = rv.vlen = rk.high_water = rv.high_water = N0
                chunk_kv(rk, rv, q, k, v)
            if S == 1:
                q1, k1, v1 = q[:, 0].contiguous(), k.reshape(-1).contiguous(), v.reshape(-1).contiguous()

                def linear():                              # W resident tokens after the append
                    lk.klen = lv.vlen = W - 1
                    decode_kv(lk, lv, q1, k1, v1)
                what = "decode_kv, %d resident tokens" % W
            else:
                def linear():
                    lk.klen = lv.vlen = W
                    chunk_kv(lk, lv, q, k, v)
                what = "chunk_kv at c0 = %d" % W
            tr, tl, sr, sl = alternate(ring, linear, args.reps, args.warmup, args.inner)
            r = dict(Hq=Hq, Hkv=Hkv, bits=bits, window=W, capacity=C, ring_tokens_before=N0, S=S, linear=what,
                     ring_ms=tr, linear_ms=tl, ring_over_linear=tr / tl, ring_ms_min_max=sr, linear_ms_min_max=sl,
                     reps=args.reps, inner=args.inner)
            rows.append(r)
            print(json.dumps(r), flush=True)
        del rk, rv, lk, lv, kp, vp
        torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
