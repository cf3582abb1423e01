#!/usr/bin/env python
"""Draft-tree verification over the compressed cache, per layer: one TREE round (pack + kvq_chunk_attention_tree of S
rows + kvq_keep_columns of a 4-node path) against one CHAIN round with the unchanged grouped kernel (pack +
kvq_chunk_attention_grouped + truncate of the rejected tail), and kvq_keep_columns alone against the torch slice fills
of truncate.  nuq4 + 1 % outliers, 32 query heads over 8 and over 4 KV heads, no sink tokens, L0 = 131072 and 32768
cached tokens, S in {8, 32}; the tree is two branches from the root, the kept path the root and three nodes of the second.

Every time comes from HIP events around synchronised work; the routes alternate inside one loop on the same caches and
each number is the median of --reps runs after one warm-up.  Per point:
  tree_round_ms / chain_round_ms     the two rounds          tree_over_chain          their ratio
  tree_attn_ms / chain_attn_ms       attention only          tree_attn_over_chain     their ratio
  keep_ms / truncate_ms              keeping 4 of S columns (one launch) / dropping S - 4 (torch slice fills)

usage: python tools/tree_bench.py [--out FILE] [--reps N] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kvquant_amd import ops  # noqa: E402
from kvquant_amd.cache import chunk_kv, keep_kv, layer_struct  # noqa: E402
from tests import chunk_check as cc  # noqa: E402
from tests import tree_check as tc  # noqa: E402


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
    return [statistics.median(t) for t in ts], [max(t) - min(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_bench_mi355x.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="only 32 / 8 heads, L0 = 32768")
    args = ap.parse_args()
    dev = "cuda:0"
    Hq, KEEP = 32, 4
    L0s = [32768] if args.quick else [131072, 32768]
    Ss = [8, 32]
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
                parent = tc.two_branches(S)
                path = [0] + [S // 2 + 1 + i for i in range(KEEP - 1)]
                assert ops.chunk_attention_route(Hq, Hkv, S) == "grouped"

                def tree_round():
                    kc.klen = vc.vlen = L0
                    chunk_kv(kc, vc, q, k, v, parent=parent)
                    keep_kv(kc, vc, S, path)

                def chain_round():
                    kc.klen = vc.vlen = L0
                    chunk_kv(kc, vc, q, k, v)
                    kc.truncate(S - KEEP)
                    vc.truncate(S - KEEP)
                tree_round()
                layer = layer_struct(kc, vc)

                def tree_attn():
                    ops.chunk_attention_tree(layer, Hq, L0, q, parent)

                def chain_attn():
                    ops.chunk_attention(layer, Hq, L0, q)

                def keep():
                    kc.klen = vc.vlen = L0 + S
                    keep_kv(kc, vc, S, path)

                def truncate():
                    kc.klen = vc.vlen = L0 + S
                    kc.truncate(S - KEEP)
                    vc.truncate(S - KEEP)
                (t_tr, t_cr, t_ta, t_ca, t_k, t_t), spread = timed_alternating(
                    [tree_round, chain_round, tree_attn, chain_attn, keep, truncate], args.reps)
                kc.klen = vc.vlen = L0
                r = dict(Hq=Hq, Hkv=Hkv, G=Hq // Hkv, L0=L0, S=S, bits=4, kept=KEEP,
                         tree_round_ms=t_tr * 1e3, chain_round_ms=t_cr * 1e3, tree_over_chain=t_tr / t_cr,
                         tree_attn_ms=t_ta * 1e3, chain_attn_ms=t_ca * 1e3, tree_attn_over_chain=t_ta / t_ca,
                         keep_ms=t_k * 1e3, truncate_ms=t_t * 1e3,
                         tree_round_spread_ms=spread[0] * 1e3, chain_round_spread_ms=spread[1] * 1e3)
                rows.append(r)
                print(json.dumps(r), flush=True)
        del kc, vc, kp, vp
        torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
