"""Sliding-window attention on ring caches (kvq_chunk_attention_window, cache.QuantK(window=W)): a ring cache and its
LINEAR TWIN (a plain cache long enough for the whole stream) take the same seeded stream; the fp64 statement of the
window semantics is evaluated over the twin.  Shared by tests/test_window_attn_gpu.py and tools/window_bench.py."""
import math

import torch

from tests import chunk_check as cc
from tests import decode_check
from tests import rope_check as rc

HD = 128


def make_ring(bits, Hkv, C, W, sinks=0, norm=False, device="cuda", seed=0, window=True):
    """(QuantK, QuantV) as chunk_check.make_caches makes them, as a ring of C columns with window W (window=False: a
    plain cache of C columns with the same quantizer)"""
    from kvquant_amd.cache import QuantK, QuantV
    width = Hkv * HD
    quant, scale, shift = decode_check.quantizer(bits, seed=seed + bits, C=width)
    if norm:
        quant = tuple(quant) + (torch.tensor(1.07), torch.tensor(-0.02))
    kw = dict(bits=bits, hidden_size=width, num_heads=Hkv, max_position_embeddings=C, include_sparse=True,
              sparsity_threshold=0.99, first_few_fp16=sinks, device=device)
    if window:
        kw["window"] = W
    kc, vc = QuantK(rope_theta=10000.0, **kw), QuantV(**kw)
    kc.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99, norm=norm)
    vc.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99, norm=norm)
    kc.klen = vc.vlen = sinks          # (the fp16 sink tokens count in klen; the tests own the sink caches)
    return kc, vc, scale.to(device), shift.to(device)


class Stream:
    """a ring cache (C columns, window W) and its linear twin fed with the same `total` seeded tokens.  Every third
    token's key is scaled down so that its outlier row holds zeros where its neighbours' hold residuals."""

    def __init__(self, bits, Hkv, C, W, total, sinks=0, norm=False, device="cuda", seed=0, token_seed=None, rope=None):
        self.C, self.W, self.sinks, self.Hkv, self.device = C, W, sinks, Hkv, device
        self.kc, self.vc, scale, shift = make_ring(bits, Hkv, C, W, sinks, norm, device, seed)
        self.tk, self.tv, _, _ = make_ring(bits, Hkv, 64 * ((total + 63) // 64), W, sinks, norm, device, seed, window=False)
        if rope is not None:
            self.kc.rope = self.tk.rope = rc.spec(rope)
        self.k, self.v = cc.tokens(total, Hkv, scale, shift, device, seed=(seed if token_seed is None else token_seed) + 11)
        self.k[:, :, 2::3] *= 0.125
        self.ks, self.vs = cc.sink_caches(Hkv, sinks, device, seed + 12) if sinks else (None, None)
        self.N = 0

    def take(self, S):
        """the next S tokens [Hkv, 128, S] (k, v)"""
        return self.k[:, :, self.N:self.N + S].contiguous(), self.v[:, :, self.N:self.N + S].contiguous()

    def pack(self, S):
        """the next S tokens into both caches, no attention"""
        k, v = self.take(S)
        for c, x in ((self.kc, k), (self.vc, v), (self.tk, k), (self.tv, v)):
            c.parallel_pack(x.float())
        self.N += S

    def rope_table(self):
        """the table of the newest position (None: the theta rule)"""
        return self.kc.rope_table(self.sinks + self.N)

    def layer(self):
        from kvquant_amd.cache import layer_struct
        return layer_struct(self.kc, self.vc)

    def reference(self, q, n0, heads=None, rows=None):
        """fp64 statement over the twin for a chunk whose first token is n0 (the twin holds n0 + S tokens or more)"""
        return reference(self.tk, self.tv, q, n0, self.W, self.ks, self.vs, heads, rows, self.rope_table())


def reference(tk, tv, q, c0, W, k_sink=None, v_sink=None, heads=None, rows=None, rope=None):
    """chunk_check.reference over the linear twin with the extra mask column < c0 + row - W + 1: query i sees the sink
    tokens and columns (c0 + i - W, c0 + i].  rope: (inv_freq, attention factor) or None (the theta rule).  Returns f64
    [len(rows), len(heads), 128]."""
    from kvquant_amd import ops
    Hkv = tk.num_heads
    Hq, S, _ = q.shape
    G = Hq // Hkv
    Lc = c0 + S
    inv, af = rope if rope is not None else (ops.rope_freqs(tk.rope_theta, device=tk.device), 1.0)
    kr, vh = rc.dequant(tk, tv, Lc, inv, af)
    heads = list(range(Hq)) if heads is None else list(heads)
    rows = torch.arange(S, device=q.device) if rows is None else torch.as_tensor(rows, device=q.device)
    col = torch.arange(Lc, device=q.device)
    mask = (col[None, :] > (c0 + rows)[:, None]) | (col[None, :] < (c0 + rows - W + 1)[:, None])
    out = torch.empty(len(rows), len(heads), HD, dtype=torch.float64, device=q.device)
    for j, h in enumerate(heads):
        hk = h // G
        qh = q[h, rows].double()
        sc = ((qh @ kr[hk]) / math.sqrt(HD)).masked_fill(mask, float("-inf"))
        vv = vh[hk].t()
        if k_sink is not None:
            sc = torch.cat(((qh @ k_sink[hk].double()) / math.sqrt(HD), sc), dim=1)
            vv = torch.cat((v_sink[hk].double(), vv), dim=0)
        out[:, j] = torch.softmax(sc, dim=-1) @ vv
    return out


def column_arrays(kc, vc):
    """[(name, tensor, column axis)] of every array in which a column owns storage"""
    arrs = [("kcache", kc.kcache, 2), ("k outliers", kc.outliers, 0), ("k outlier_indices", kc.outlier_indices, 0),
            ("k outliers_t", kc.outliers_t, 1), ("k outlier_indices_t", kc.outlier_indices_t, 1),
            ("vcache", vc.vcache, 2), ("v lookup_table", vc.lookup_table, 0), ("v outliers", vc.outliers, 0),
            ("v outlier_indices", vc.outlier_indices, 0)]
    if vc.lookup_table2 is not None:
        arrs.append(("v lookup_table2", vc.lookup_table2, 0))
    return arrs


def assert_state(st, lo_token=0):
    """every resident ring column that holds a token >= lo_token equals the twin's column of that token, bit for bit"""
    from kvquant_amd.cache import ring_token
    res = min(st.N, st.C)
    cols = torch.arange(res, device=st.device)
    toks = torch.tensor([ring_token(c, st.N, st.C) for c in range(res)], device=st.device)
    keep = toks >= lo_token
    cols, toks = cols[keep], toks[keep]
    for (name, ring, ax), (_, twin, _) in zip(column_arrays(st.kc, st.vc), column_arrays(st.tk, st.tv)):
        a, b = ring.index_select(ax, cols), twin.index_select(ax, toks)
        assert torch.equal(a, b), "%s: ring and twin differ at N = %d" % (name, st.N)
