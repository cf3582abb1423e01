"""Exact tests of the matrix-core attention kernels (kvq_chunk_attn.hip, kvq_prefill_attn.hip, kvq_flash_tile.h).

THE CENSUS: every query is exactly zero, every dequantised value a small integer.  Every score is then 0, a visible key
weighs 2^0 = 1 and a masked one 2^-inf = 0, the running sums are integers below 2^24 (exact in fp32) and the output is
one division: out[row, h, d] * n_vis(row) == the sum of Vint[c, d] over the columns and sink tokens the row sees, up to
one rounding.  Vint spells the token: channel d < 24 holds bit d of the token's id n, channel 24 <= d < 128 holds
[n mod 104 == d - 24]; one outlier entry of 2.0 rides on every 7th token (KV head (n // 7) mod Hkv, so that it counts
for one KV head and must not count for the others) and, with more than one KV head, on every 11th (KV head
(n // 11 + 1) mod Hkv), both at channels >= 24.  The value cache's arrays are written directly: codebook rows
[0, 1, 0, 1, ...], packed codes whose low bit is the wanted value (pack_codes, the inverse of gqa_check.unpack_codes).

THE NEEDLE: the K cache holds the SAME pre-RoPE token in every column (through parallel_pack), so a column's rotated key
depends on its position alone; the query of a row is gain x the rotated key of a target token, so the softmax peaks at
the column that sits at the target's position and channels 0 .. 23 of the output spell the id of the column attended.

The expected counts come from the mask statements in token space (causal, window, tree_check.visible), nothing from
the library.  Shared by tests/test_census_attn_gpu.py, tests/test_needle_attn_gpu.py and tests/test_census_cpu.py."""
import math

import torch

from tests import tree_check as tc

HD = 128
ID_BITS = 24
RESIDUES = HD - ID_BITS        # 104
SINK_ID0 = 1 << 20             # sink token j has id SINK_ID0 + j: disjoint from every compressed token's id


# ---- packed codes ------------------------------------------------------------------------------------------------
def pack_codes(codes, bits):
    """packed words int32 [H, 128/32*bits, L] of codes [H, 128, L] in 0 .. 2^bits - 1: the inverse of
    gqa_check.unpack_codes (code i of a 32-channel group is bits [bits*i, bits*i + bits) of the group's little-endian
    word concatenation)"""
    H, D, L = codes.shape
    codes = codes.to(torch.int64)
    w = torch.zeros(H, D // 32 * bits, L, dtype=torch.int64, device=codes.device)
    for grp in range(D // 32):
        for i in range(32):
            st = bits * i
            k, off = st // 32, st % 32
            c = codes[:, grp * 32 + i]
            w[:, grp * bits + k] |= (c << off) & 0xffffffff
            if off + bits > 32:
                w[:, grp * bits + k + 1] |= c >> (32 - off)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


# ---- the integer values ------------------------------------------------------------------------------------------
def base_values(ids):
    """int64 [n, 128] in {0, 1}: channel d < 24 is bit d of the id, channel d >= 24 is [id mod 104 == d - 24]"""
    ids = ids.to(torch.int64)
    d = torch.arange(HD, device=ids.device)
    lo = (ids[:, None] >> d[None, :ID_BITS]) & 1
    hi = (ids[:, None] % RESIDUES == d[None, ID_BITS:] - ID_BITS).to(torch.int64)
    return torch.cat((lo, hi), dim=1)


def outlier_entries(ids, Hkv):
    """the outlier row of every token: (global channel int64 [n, 2], value f32 [n, 2]), ascending channels, (0, 0.0)
    where a token has no entry.  Every 7th token: 2.0 in KV head (n // 7) mod Hkv; with Hkv > 1 every 11th token: 2.0
    in KV head (n // 11 + 1) mod Hkv.  Channels 24 .. 127 of the head."""
    ids = ids.to(torch.int64)
    on7 = ids % 7 == 0
    g7 = ((ids // 7) % Hkv) * HD + ID_BITS + (ids // 7 * 5) % RESIDUES
    on11 = (ids % 11 == 0) & (Hkv > 1)
    g11 = ((ids // 11 + 1) % Hkv) * HD + ID_BITS + (ids // 11 * 3 + 50) % RESIDUES
    idx = torch.stack((torch.where(on7, g7, torch.zeros_like(g7)), torch.where(on11, g11, torch.zeros_like(g11))), 1)
    val = torch.stack((on7, on11), 1).float() * 2.0
    idx, order = idx.sort(dim=1, stable=True)
    return idx, val.gather(1, order)


def values(ids, Hkv):
    """Vint int64 [Hkv, n, 128]: base_values of the token + its outlier entries in the KV head that owns the channel"""
    n = ids.numel()
    flat = base_values(ids).repeat(1, Hkv)                                   # token-major, global channels
    idx, val = outlier_entries(ids, Hkv)
    flat.scatter_add_(1, idx, val.to(torch.int64))
    return flat.reshape(n, Hkv, HD).permute(1, 0, 2).contiguous()


def sink_values(sinks, device):
    """int64 [sinks, 128]: the sink tokens' values (every KV head the same), ids SINK_ID0 + j"""
    return base_values(SINK_ID0 + torch.arange(sinks, device=device))


def decode_ids(out):
    """the id spelled by channels 0 .. 23 of out [..., 128]: int64 [...]"""
    bits = (out[..., :ID_BITS] > 0.5).to(torch.int64)
    return (bits << torch.arange(ID_BITS, device=out.device)).sum(-1)


# ---- expected counts from the mask statements (token space) ----------------------------------------------------------
def _cum(vals):
    """cum[:, n] = sum of vals[:, :n]: int64 [Hkv, L + 1, 128]"""
    return torch.cat((torch.zeros_like(vals[:, :1]), vals.cumsum(1)), dim=1)


def count_causal(vals, c0, S, sink_vals=None):
    """row i sees tokens [0, c0 + i] (col <= c0 + row) and the sinks: (count int64 [S, Hkv, 128], n_vis int64 [S])"""
    rows = torch.arange(S, device=vals.device)
    return _finish(_cum(vals)[:, c0 + rows + 1].permute(1, 0, 2), c0 + rows + 1, sink_vals)


def count_window(vals, n0, S, W, sink_vals=None):
    """row i sees tokens n0 + i - W < n <= n0 + i and the sinks"""
    rows = torch.arange(S, device=vals.device)
    hi = n0 + rows + 1
    lo = (n0 + rows - W + 1).clamp_min(0)
    cum = _cum(vals)
    return _finish((cum[:, hi] - cum[:, lo]).permute(1, 0, 2), hi - lo, sink_vals)


def count_tree(vals, c0, parent, sink_vals=None):
    """row i sees tokens < c0, the nodes tree_check.visible(parent) gives it and the sinks"""
    S = len(parent)
    vis = tc.visible(parent).to(vals.device).to(torch.int64)                 # [S, S]
    before = vals[:, :c0].sum(1)                                             # [Hkv, 128]
    chunk = (vis[:, None, :, None] * vals[None, :, c0:c0 + S]).sum(2)          # [S, Hkv, 128]
    return _finish(before[None] + chunk, c0 + vis.sum(1), sink_vals)


def _finish(count, n_vis, sink_vals):
    if sink_vals is not None and sink_vals.shape[0]:
        count = count + sink_vals.sum(0)[None, None, :]
        n_vis = n_vis + sink_vals.shape[0]
    return count.contiguous(), n_vis


def brute_counts(vals, vis, sink_vals=None):
    """the same by a double loop over rows and tokens: vis bool [S, L] (nested lists or a tensor)"""
    Hkv, L, _ = vals.shape
    S = len(vis)
    count = torch.zeros(S, Hkv, HD, dtype=torch.int64)
    n_vis = torch.zeros(S, dtype=torch.int64)
    for i in range(S):
        for n in range(L):
            if vis[i][n]:
                count[i] += vals[:, n].cpu()
                n_vis[i] += 1
        if sink_vals is not None:
            for j in range(sink_vals.shape[0]):
                count[i] += sink_vals[j].cpu()[None, :]
                n_vis[i] += 1
    return count, n_vis


# ---- visibility in token space (bool [S, L]) --------------------------------------------------------------------------
def vis_causal(c0, S, L, device="cpu"):
    col = torch.arange(L, device=device)
    return col[None, :] <= (c0 + torch.arange(S, device=device))[:, None]


def vis_window(n0, S, W, L, device="cpu"):
    col = torch.arange(L, device=device)
    row = (n0 + torch.arange(S, device=device))[:, None]
    return (col[None, :] <= row) & (col[None, :] > row - W)


def vis_tree(c0, parent, L, device="cpu"):
    S = len(parent)
    vis = torch.zeros(S, L, dtype=torch.bool, device=device)
    vis[:, :c0] = True
    vis[:, c0:c0 + S] = tc.visible(parent).to(device)
    return vis


# ---- the census bar -----------------------------------------------------------------------------------------------
def check(out, count, n_vis, G, what, channels=None, bar=None):
    """|out * n_vis - count| <= max(count, 1) * 2^-22 in fp64 for EVERY row, head and channel (four times the single
    rounding of the division of two exact integers).  out [S, Hq, 128], count int64 [S, Hkv, 128], n_vis int64 [S].
    channels / bar: the prefill kernel's residue channels and fp16 bar.  Returns the worst error / bar."""
    got = out.double() * n_vis.double()[:, None, None]
    exp = count.repeat_interleave(G, dim=1).double()
    lim = exp.clamp_min(1.0) * 2.0 ** -22 if bar is None else bar(exp)
    err = (got - exp).abs()
    if channels is not None:
        err, lim, got, exp = err[..., channels], lim[..., channels], got[..., channels], exp[..., channels]
    bad = ~(err <= lim)                                                      # (a NaN is bad)
    worst = float((err / lim).max()) if err.numel() else 0.0
    print("%s: census worst error %.3g of the bar over %d values" % (what, worst, err.numel()))
    if bool(bad.any()):
        i, h, d = [int(x) for x in bad.nonzero()[0]]
        d_full = d if channels is None else int(torch.arange(HD)[channels][d])
        raise AssertionError(
            "%s: %d of %d values off; first at row %d head %d channel %d: out * n_vis = %.6f, count = %d (n_vis %d; a "
            "residue channel d counts the visible tokens with n mod 104 == d - 24, an id channel those with bit d)"
            % (what, int(bad.sum()), bad.numel(), i, h, d_full, float(got[i, h, d]), int(exp[i, h, d]), int(n_vis[i])))
    return worst


def prefill_bar(exp):
    """the prefill kernel writes fp16: one fp16 rounding of the quotient (2^-11 relative, 2^-10 taken) plus the fp32
    quotient's own"""
    return exp * 2.0 ** -10 + 2.0 ** -20


# ---- the split plan (a transcription of chunk::plan in kvq_chunk_attn.hip, for docstrings and needle targets; the GPU
# tests hold it against the library's workspace functions) ----------------------------------------------------------------
K_TILE, ROWS_PER_WG, TARGET_WGS, MIN_TILES_PER_SPLIT, MAX_SPLITS = 64, 256, 512, 4, 64


def split_plan(Hq, Hkv, S, c0, grouped=False, cols=None):
    """(nqb, nsplit, tps, workspace bytes): cols = the resident columns of a ring (None: c0 + S)"""
    nqb = (S + ROWS_PER_WG - 1) // ROWS_PER_WG
    tiles = ((c0 + S if cols is None else cols) + K_TILE - 1) // K_TILE
    base = Hkv if grouped else Hq * nqb
    ns = (TARGET_WGS + base - 1) // base
    ns = max(1, min(ns, max(tiles // MIN_TILES_PER_SPLIT, 1), MAX_SPLITS))
    a256 = lambda x: (x + 255) & ~255
    nbytes = lambda n: a256(Hq * n * S * HD * 4) + a256(Hq * n * S * 8)
    while ns > 1 and nbytes(ns) > 1 << 30:
        ns -= 1
    tps = (tiles + ns - 1) // ns
    nsplit = (tiles + tps - 1) // tps
    return nqb, nsplit, tps, nbytes(nsplit)


# ---- fixtures: caches whose V is the census and whose K is seeded tokens (or one token everywhere) ------------------
def write_values(vc, cols, ids, seed=0):
    """columns `cols` (slice or int64 tensor) of the value cache hold the tokens `ids`: codebook rows [0, 1, 0, 1, ...]
    in the table p.V dequantises with (9.0 in the other one, where Q-Norm keeps two), packed codes whose low bit is the
    value and whose high bits are random, the outlier rows of outlier_entries (zero-filled, ascending channels)"""
    dev, H, bits = vc.device, vc.num_heads, vc.bits
    n = 2 ** bits
    ids = ids.to(dev)
    L = ids.numel()
    g = torch.Generator(device=dev).manual_seed(seed + 99)
    high = torch.randint(0, n // 2, (H, HD, L), generator=g, device=dev)
    codes = 2 * high + base_values(ids).t()[None]
    vc.vcache[:, :, cols] = pack_codes(codes, bits)
    mix = vc.mix_table()
    mix[cols] = (torch.arange(n, device=dev) % 2).float()
    for t in (vc.lookup_table, vc.lookup_table2):
        if t is not None and t is not mix:
            t[cols] = 9.0
    idx, val = outlier_entries(ids, H)
    oi = torch.zeros(L, vc.num_outliers, dtype=torch.int32, device=dev)
    ov = torch.zeros(L, vc.num_outliers, dtype=torch.float32, device=dev)
    oi[:, -2:], ov[:, -2:] = idx.to(torch.int32), val
    vc.outlier_indices[cols], vc.outliers[cols] = oi, ov


def needle_token(Hkv, scale, shift, device, seed):
    """the needle's pre-RoPE key [Hkv, 128, 1] fp16: channel c sits at shift_c +- min(2.4 scale_c, 1.5) -- inside the
    quantiser's range (+- 2.5 scale), near-equal pair energies wherever the seeded scales allow, so that the rotary
    autocorrelation peaks sharply within |q| <= 256 -- and two channels per KV head beyond it, OUTLIER_CHANNELS[0] at
    + 3.5 scale and OUTLIER_CHANNELS[1] at - 3.5 scale (one for the upper and one for the lower outlier slots, of which
    a cache of one KV head has one each), which leave through the outlier path (assert_outlier_path)"""
    g = torch.Generator().manual_seed(seed + 17)
    sign = (torch.randint(0, 2, (Hkv * HD,), generator=g) * 2 - 1).float().to(device)
    amp = torch.minimum(2.4 * scale, torch.full_like(scale, 1.5))
    for hk in range(Hkv):
        for c, sg in zip(OUTLIER_CHANNELS, (1.0, -1.0)):
            amp[hk * HD + c], sign[hk * HD + c] = 3.5 * scale[hk * HD + c], sg
    return (shift + sign * amp).half().reshape(Hkv, HD, 1)


OUTLIER_CHANNELS = (20, 90)


def assert_outlier_path(kc, cols):
    """the needle token's two outlier channels per KV head hold non-zero residuals in the outlier rows (and their
    token-contiguous mirror) of the first and last of `cols` packed columns: the K outlier path is the real one"""
    want = {hk * HD + c for hk in range(kc.num_heads) for c in OUTLIER_CHANNELS}
    for col in (0, cols - 1):
        rows = ((kc.outlier_indices[col], kc.outliers[col]), (kc.outlier_indices_t[:, col], kc.outliers_t[:, col]))
        for idx, val in rows:
            got = {i for i, v in zip(idx.tolist(), val.tolist()) if v != 0.0}
            assert want <= got, "needle fixture: column %d keeps residuals at channels %s, not at %s" % (
                col, sorted(got), sorted(want))


def _keys(n, Hkv, scale, shift, device, seed, same_key):
    from tests import chunk_check as cc
    if same_key:
        return needle_token(Hkv, scale, shift, device, seed).expand(Hkv, HD, n).contiguous()
    return cc.tokens(n, Hkv, scale, shift, device, seed + 11)[0]


def _sinks(Hkv, sinks, device, seed):
    from tests import chunk_check as cc
    if not sinks:
        return None, None, None
    ks = cc.sink_caches(Hkv, sinks, device, seed + 12)[0]
    sv = sink_values(sinks, device)
    return ks, sv.half()[None].repeat(Hkv, 1, 1).contiguous(), sv


class Linear:
    """a plain cache of L census tokens (token n in column n).  K: seeded heavy-tailed tokens through parallel_pack, or
    with same_key ONE of them in every column; V: written directly.  Chunks (c0, S) with c0 + S <= L all run on the one
    cache: the columns behind a chunk hold further tokens, which nothing may see."""

    def __init__(self, bits, Hkv, L, sinks=0, norm=False, same_key=False, seed=0, device="cuda:0"):
        from tests import chunk_check as cc
        self.bits, self.Hkv, self.L, self.sinks, self.device = bits, Hkv, L, sinks, device
        self.kc, self.vc, scale, shift = cc.make_caches(bits, Hkv, 64 * ((L + 63) // 64) + 64, sinks=sinks, norm=norm,
                                                        device=device, seed=seed)
        self.kc.klen = sinks
        self.kc.parallel_pack(_keys(L, Hkv, scale, shift, device, seed, same_key).float())
        self.vc.vlen = self.kc.klen
        if same_key:
            assert_outlier_path(self.kc, L)
        ids = torch.arange(L, device=device)
        write_values(self.vc, slice(0, L), ids, seed)
        self.vals = values(ids, Hkv)
        self.ks, self.vs, self.sink_vals = _sinks(Hkv, sinks, device, seed)

    def layer(self):
        from kvquant_amd.cache import layer_struct
        return layer_struct(self.kc, self.vc)


class Ring:
    """a ring of C columns with window W.  K: C seeded tokens (or one token everywhere) through parallel_pack -- under
    a zero query, or with the same token in every column, K does not depend on how often the ring has wrapped; V: at(N)
    writes, for the state after N tokens, the token cache.ring_token(c, N, C) into every resident column c."""

    def __init__(self, bits, Hkv, C, W, sinks=0, same_key=False, seed=0, device="cuda:0"):
        from tests import window_check as wc
        self.bits, self.Hkv, self.C, self.W, self.sinks, self.device, self.seed = bits, Hkv, C, W, sinks, device, seed
        self.kc, self.vc, scale, shift = wc.make_ring(bits, Hkv, C, W, sinks, False, device, seed)
        k = _keys(C, Hkv, scale, shift, device, seed, same_key).float()
        for c in range(0, C, 64):
            self.kc.parallel_pack(k[:, :, c:c + 64].contiguous())
        if same_key:
            assert_outlier_path(self.kc, C)
        self.ks, self.vs, self.sink_vals = _sinks(Hkv, sinks, device, seed)
        self.N = 0

    def at(self, N):
        from kvquant_amd.cache import ring_token
        cols = torch.arange(min(N, self.C), device=self.device)
        write_values(self.vc, cols, ring_token(cols, N, self.C), self.seed)
        self.N = N
        self.vals = values(torch.arange(N, device=self.device), self.Hkv)     # token space
        return self

    def layer(self):
        from kvquant_amd.cache import layer_struct
        return layer_struct(self.kc, self.vc)


# ---- the needle ---------------------------------------------------------------------------------------------------
MASS = 0.999
Q_MAX = 256.0


def statement(q, keys, vals, vis, n_sink):
    """the fp64 statement of every chunk entry over keys that are already rotated where the entry's statement puts
    them: q [Hq, S, 128]; keys f64 [Hkv, 128, n_sink + L] (sink keys first), vals f64 [Hkv, n_sink + L, 128]; vis bool
    [S, L] (the sinks are always visible).  Returns (out f64 [S, Hq, 128], p f64 [S, Hq, n_sink + L])."""
    Hq, S, _ = q.shape
    G = Hq // keys.shape[0]
    mask = torch.cat((torch.ones(S, n_sink, dtype=torch.bool, device=vis.device), vis), dim=1)
    out = torch.empty(S, Hq, HD, dtype=torch.float64, device=q.device)
    p = torch.empty(S, Hq, mask.shape[1], dtype=torch.float64, device=q.device)
    for h in range(Hq):
        sc = (q[h].double() @ keys[h // G]) / math.sqrt(HD)
        p[:, h] = torch.softmax(sc.masked_fill(~mask, float("-inf")), dim=-1)
        out[:, h] = p[:, h] @ vals[h // G]
    return out, p


def find_gains(s1, tgt, key_max):
    """per row the smallest gain of 8 * 1.25^k whose softmax mass on the target is >= MASS (with head room for the fp16
    rounding of q): s1 f64 [R, n] scaled scores at gain 1 (-inf where masked), tgt int64 [R], key_max f64 [R] the
    largest |entry| of the row's target key.  A row that would pass |q| = Q_MAX first keeps a gain of 0."""
    gain = torch.full_like(key_max, 8.0)
    done = torch.zeros_like(key_max, dtype=torch.bool)
    while True:
        mass = torch.softmax(gain[:, None] * s1, dim=-1).gather(1, tgt[:, None])[:, 0]
        done |= mass >= MASS + 2e-4
        grow = ~done & (gain * 1.25 * key_max <= Q_MAX)
        if not bool(grow.any()):
            return torch.where(done, gain, torch.zeros_like(gain))
        gain = torch.where(grow, gain * 1.25, gain)


def needle_queries(keys, targets, G, vis, n_sink):
    """q fp16 [Hq, S, 128]: q[h, row] = gain x keys[h // G][:, targets[row]] with the gain of find_gains per (KV head,
    row); targets int64 [S] index the key axis (sink j: j; token n: n_sink + n).  AssertionError (the fixture's, not
    the kernel's) if a target is not visible or no gain within |q| <= 256 reaches the mass.  Returns (q, largest
    gain)."""
    Hkv = keys.shape[0]
    S = targets.numel()
    targets = targets.to(keys.device)
    mask = torch.cat((torch.ones(S, n_sink, dtype=torch.bool, device=vis.device), vis), dim=1)
    assert bool(mask.gather(1, targets[:, None]).all()), "needle fixture: a target its row cannot see"
    kt = keys[:, :, targets].permute(0, 2, 1)                                   # [Hkv, S, 128]
    s1 = torch.cat([((kt[hk] @ keys[hk]) / math.sqrt(HD)).masked_fill(~mask, float("-inf")) for hk in range(Hkv)])
    gain = find_gains(s1, targets.repeat(Hkv), kt.abs().amax(dim=-1).reshape(-1))
    assert bool((gain > 0).all()), "needle fixture: no gain with |q| <= %g puts %.3f of the mass on %d of %d targets" % (
        Q_MAX, MASS, int((gain == 0).sum()), gain.numel())
    q = (gain.reshape(Hkv, S, 1) * kt).half()
    return q.repeat_interleave(G, dim=0).contiguous(), float(gain.max())


def schedule(personal, shared, vis_key, S):
    """targets int64 [R, S] (key-axis indices): row i takes its personal targets, the shared ones (boundaries every row
    that sees them could take) go to the row with the fewest targets so far among those that see them; a row that has
    run out repeats its targets.  personal: {row: [key index]}, shared: [key index], vis_key bool [S, n_keys]."""
    vis_key = vis_key.cpu()
    lists = [[] for _ in range(S)]
    for i, ts in personal.items():
        for t in ts:
            if 0 <= t < vis_key.shape[1] and bool(vis_key[i, t]) and t not in lists[i]:
                lists[i].append(t)
    for t in shared:
        if not 0 <= t < vis_key.shape[1]:
            continue
        rows = vis_key[:, t].nonzero().flatten().tolist()
        if rows and not any(t in lists[i] for i in rows):
            lists[min(rows, key=lambda i: (len(lists[i]), i))].append(t)
    R = max(len(x) for x in lists)
    assert all(lists), "every row has a target (its own column)"
    return torch.tensor([[x[r % len(x)] for x in lists] for r in range(R)], dtype=torch.int64)


def boundary_columns(c0, S, tps, n_cols):
    """the columns on both sides of every split edge, of c0, and of every tile edge of a case of up to 80 tiles.  A
    longer case (131072 columns: 2048 tile edges, 128 launches of 32 rows) takes, deliberately, a sample of its tile
    edges: the first, the last, those around c0 and one in the middle of EVERY split."""
    tiles = (n_cols + K_TILE - 1) // K_TILE
    if tiles <= 80:
        edges = set(range(1, tiles))
    else:
        edges = {1, tiles - 1, c0 // K_TILE, c0 // K_TILE + 1} | {t0 + tps // 2 for t0 in range(0, tiles, tps)}
    edges = {e for e in edges if 0 < e < tiles} | set(range(tps, tiles, tps))
    cols = {c0 - 1, c0}
    for e in edges:
        cols |= {K_TILE * e - 1, K_TILE * e}
    return sorted(c for c in cols if 0 <= c < n_cols)


def handful(S):
    """the first and last row, the middle, and the rows on both sides of the 32-row and 256-row block edges"""
    return sorted({i for i in (0, S - 1, S // 2, 31, 32, 255, 256, 511, 512) if 0 <= i < S})


def rotated(fx, L, rope):
    """(keys f64 [Hkv, 128, L] rotated at sinks + column, Vhat f64 [Hkv, 128, L], inv_freq f32 [64]) of a Linear
    fixture's caches by rope_check.dequant; rope: None (the theta rule) or (inv_freq, attention factor)"""
    from kvquant_amd import ops
    from tests import rope_check as rc
    inv, af = rope if rope is not None else (ops.rope_freqs(fx.kc.rope_theta, device=fx.kc.device), 1.0)
    kr, vh = rc.dequant(fx.kc, fx.vc, L, inv, af)
    return kr, vh, inv.float()


def tree_rotate(kr, c0, parent, sinks, inv):
    """tree_check's depth rule: the chunk's columns turned back by the angle of their column and forward by the angle
    of sinks + c0 + depth (fl32 angles), as tree_check.reference does"""
    S = len(parent)
    dev = kr.device
    col_pos = torch.arange(c0, c0 + S, device=dev, dtype=torch.float32) + sinks
    dep_pos = torch.tensor(tc.depths(parent), device=dev, dtype=torch.float32) + (c0 + sinks)
    a_old = (inv[:, None] * col_pos[None, :]).double()
    a_new = (inv[:, None] * dep_pos[None, :]).double()
    lo, hi = kr[:, :64, c0:c0 + S], kr[:, 64:, c0:c0 + S]
    c, s = a_old.cos(), a_old.sin()
    lo0, hi0 = c * lo + s * hi, -s * lo + c * hi
    c, s = a_new.cos(), a_new.sin()
    kr = kr[:, :, :c0 + S].clone()
    kr[:, :64, c0:] = c * lo0 - s * hi0
    kr[:, 64:, c0:] = s * lo0 + c * hi0
    return kr


def with_sinks(kr, vh, fx):
    """(keys [Hkv, 128, n_sink + L], vals [Hkv, n_sink + L, 128]) with the fixture's sink tokens in front"""
    vals = vh.transpose(1, 2)
    if fx.sinks:
        return torch.cat((fx.ks.double(), kr), dim=2), torch.cat((fx.vs.double(), vals), dim=1)
    return kr, vals.contiguous()


def expected_ids(targets, n_sink):
    """the id a key-axis index spells: SINK_ID0 + j for sink j, the token for a compressed column"""
    return torch.where(targets < n_sink, SINK_ID0 + targets, targets - n_sink)


# ---- the needle's precondition for ideal keys (no library) ----------------------------------------------------------
def ideal_keys(key, inv, L):
    """f64 [128, L]: the pre-RoPE key [128] rotated at positions 0 .. L - 1 with fl32 angles inv_j * pos"""
    pos = torch.arange(L, dtype=torch.float32)
    ang = (inv.float()[:, None] * pos[None, :]).double()
    c, s = ang.cos(), ang.sin()
    lo, hi = key.double()[:64, None], key.double()[64:, None]
    return torch.cat((c * lo - s * hi, s * lo + c * hi), dim=0)


def ideal_targets(L):
    """both ends, the tile edges next to them and a tile edge in the middle"""
    m = K_TILE * (L // (2 * K_TILE))
    last = K_TILE * ((L - 1) // K_TILE)
    return sorted({0, 1, 63, 64, 127, 128, m - 1, m, last - 1, last, L - 2, L - 1})
