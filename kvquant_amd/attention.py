"""KVQuantAttention -- the reference's patched LlamaAttention / LlamaFlashAttention2
(ML = /root/reference/deployment/transformers/src/transformers/models/llama/
modeling_llama.py:1388-2011) around the MI355X QuantK/QuantV operators.

Same protocol: pre-RoPE keys are cached compressed, RoPE is applied to Q only
(the K kernel rotates the dequantised keys on the fly), the first
`first_few_fp16` tokens live in fp16 side caches with POST-RoPE keys ("attention
sinks", ML:1464-1466), prefill packs the whole prompt in parallel and decode
feeds one token at a time (batch 1, MHA, as the reference asserts at
ML:1408/1801).

Decode is GPU-resident: 6 kernel launches for the KV path, no host
synchronisation (the reference does two device->host round trips per layer per
token, ML:707-714 and 1803-1820).  Prefill attention is kvq_prefill_attention (MFMA
flash kernel, csrc/kvq_prefill_attn.hip) where the reference calls flash-attn.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from . import rope as rope_mod
from .cache import QuantK, QuantV, chunk_kv, decode_kv, keep_kv

# q_len > 1 on a warm cache (multi-turn prompts, draft verification, chunked fills) takes kvq_chunk_attention
# (cache.chunk_kv).  KVQ_CHUNK_ATTEND=0 feeds such chunks through the q_len == 1 path token by token instead (A/B runs).
CHUNK_ATTEND = os.environ.get("KVQ_CHUNK_ATTEND", "1") != "0"


def chunk_route(klen, q_len, sinks, fast):
    """How attend() feeds q_len tokens into a cache holding klen > 0 tokens: [(kind, n), ...] in order, kind "token"
    (n tokens one at a time through the q_len == 1 path) or "chunk" (n >= 2 tokens through chunk_kv).  Tokens that
    still fill the fp16 sink cache go one at a time; the rest is one chunk when `fast` (the configuration has the
    kernel) and more than one token remains."""
    fill = min(max(sinks - klen, 0), q_len)
    route = [("token", fill)] if fill else []
    rest = q_len - fill
    if rest:
        route.append(("chunk", rest) if (fast and rest >= 2) else ("token", rest))
    return route


def window_capacity(window, slack=256):
    """columns of the ring cache of a sliding-window layer: window + slack rounded up to the 64-column tile.  The slack
    is what a chunk may add (and a rollback take back) beyond the window: pieces of capacity - window + 1 rows."""
    W, slack = int(window), int(slack)
    if W < 1 or slack < 0:
        raise ValueError("sliding_window must be >= 1 and window_slack >= 0 (got %d, %d)" % (W, slack))
    return 64 * ((W + slack + 63) // 64)


def window_route(klen, q_len, sinks, window, capacity):
    """How a sliding-window layer feeds q_len tokens into caches holding klen tokens: [(kind, n), ...] in order.
    "prefill": the first min(q_len, sinks + window) >= 2 tokens of an empty cache through the prefill kernel (inside
    that piece the window hides nothing); "token": tokens that still fill the fp16 sink cache, one at a time; "chunk":
    everything else -- a single decode token included -- through chunk_kv on the ring, capacity - window + 1 rows at
    most per piece."""
    route, rest = [], int(q_len)
    if klen == 0:
        n = min(rest, sinks + window)
        if n >= 2:
            route.append(("prefill", n))
            klen, rest = n, rest - n
    fill = min(max(sinks - klen, 0), rest)
    if fill:
        route.append(("token", fill))
        rest -= fill
    step = capacity - window + 1
    while rest:
        n = min(rest, step)
        route.append(("chunk", n))
        rest -= n
    return route


_DEPTHS = {}      # the last tree's (depth index tensor, positions) per device: every layer of a model asks for the same


def _depth_index(parent, device):
    """(int64 tensor of the rows' depths on `device`, max depth + 1) of a draft tree's parent list"""
    key = (tuple(parent), str(device))
    hit = _DEPTHS.get("last")
    if hit is None or hit[0] != key:
        depth, _ = ops.tree_tables(parent)
        hit = (key, torch.tensor(depth, device=device), max(depth) + 1)
        _DEPTHS["last"] = hit
    return hit[1], hit[2]


def rotate_half(x):
    x1 = x[..., : x.shape[-1] // 2]
    x2 = x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


class RotaryDynamic(nn.Module):
    """LlamaRotaryEmbeddingDynamic (ML:159-177): cos/sin for positions
    [start, end) computed on the fly, in the activation dtype.
    rope (kvquant_amd.rope.RopeSpec, optional): scaled RoPE -- the frequencies of transformers' table and the rows
    (emb.cos() * af).to(dtype), (emb.sin() * af).to(dtype) as LlamaRotaryEmbedding forms them; dynamic NTK takes the
    table of seq_len = end.  None or a default spec: the theta rule above, unchanged."""

    def __init__(self, dim, base=10000.0, device=None, rope=None):
        super().__init__()
        self.rope = None if rope is None or rope.is_default else rope
        if self.rope is not None and not self.rope.dynamic:
            inv_freq, self.af = self.rope.table(None)
            inv_freq = inv_freq.to(device)
        else:
            inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.int64).float().to(device) / dim))
            self.af = 1.0
        self.register_buffer("inv_freq", inv_freq, persistent=False)
        self.dim, self.base = dim, float(base)
        # (the cache key of a scaled table: its parameters, so that layers with the same RoPE share the rows)
        self._rope_key = None if self.rope is None else (self.rope.rope_type, repr(sorted(self.rope.params.items())),
                                                         self.rope.max_position_embeddings)

    # The tables of the last positions asked for, per frequency table / device / dtype: every layer of a model asks for
    # the SAME positions one after the other, and at decode the seven small launches below were a sizeable share of a
    # layer's host time (profiles/r04_full_model.txt).  Same arithmetic, once per token instead of once per layer.
    _last = {}

    def forward(self, x, start_pos, end_pos):
        inv, af = self.inv_freq, self.af
        key = (self.dim, self.base, inv.dtype, inv.device, x.dtype)
        if self.rope is not None:
            if self.rope.dynamic:
                inv, af = self.rope.table(x.device, end_pos)
                key = key + (self._rope_key, max(int(end_pos), self.rope.max_position_embeddings))
            else:
                key = key + (self._rope_key,)
        # (only decode-size requests are kept -- a prefill's [S, dim] tables would be pinned until the next call, 512 MB
        #  after a 1M-token prompt -- and per CUDA stream: the cached tensors were produced on that stream)
        small = end_pos - start_pos <= RotaryDynamic.CACHE_MAX_POSITIONS
        if small:
            key = key + (torch.cuda.current_stream(x.device).cuda_stream if x.is_cuda else 0,)
            hit = RotaryDynamic._last.get(key)
            if hit is not None and hit[0] == (start_pos, end_pos):
                return hit[1], hit[2]
        t = torch.arange(start_pos, end_pos, device=x.device, dtype=torch.int64).type_as(inv)
        freqs = torch.outer(t, inv)
        emb = torch.cat((freqs, freqs), dim=-1)
        if self.rope is None:
            cos, sin = emb.cos().to(x.dtype), emb.sin().to(x.dtype)
        else:      # (LlamaRotaryEmbedding.forward: scaled in fp32, then rounded to the activation dtype)
            cos, sin = (emb.cos() * af).to(x.dtype), (emb.sin() * af).to(x.dtype)
        if small:
            RotaryDynamic._last[key] = ((start_pos, end_pos), cos, sin)
        return cos, sin

    CACHE_MAX_POSITIONS = 16

    @classmethod
    def clear_cache(cls):
        cls._last.clear()


def gqa_groups(num_heads, num_key_value_heads=None):
    """query heads per KV head of a layer with `num_heads` query heads and `num_key_value_heads` KV heads (None: MHA).
    Grouped-query attention takes 1 <= G <= 8 with num_heads = G * num_key_value_heads; raises ValueError otherwise."""
    if num_key_value_heads is None:
        return 1
    H, Hkv = int(num_heads), int(num_key_value_heads)
    if Hkv <= 0 or H % Hkv:
        raise ValueError("num_attention_heads = %d is not a multiple of num_key_value_heads = %d" % (H, Hkv))
    if H // Hkv > 8:
        raise ValueError("grouped-query attention with %d query heads per KV head: the kernels take at most 8" % (H // Hkv))
    return H // Hkv


class KVQuantAttention(nn.Module):
    fuse_sinks = True     # decode: the fp16 sink tokens' matmuls inside the decode launches (False: torch glue as in the reference)
    # draft tree of the NEXT multi-token attend(): the parent list of its rows (row 0 the root, parent[i] < i), or None.
    # Set and cleared by the caller (kvquant_amd.llama.draft_tree); see _attend_chunk and keep_path
    tree = None

    def __init__(self, hidden_size=4096, num_heads=32, abits=4, include_sparse=True, first_few_fp16=0,
                 maxseqlen=4096, rope_theta=10000.0, sparsity_threshold=0.99, device=None,
                 dtype=torch.float16, bias=False, make_proj=True, use_orig_sparse=False, compact=False,
                 num_key_value_heads=None, rope_scaling=None, max_position_embeddings=None, sliding_window=None,
                 window_slack=256):
        super().__init__()
        # sliding_window=W: the caches are RINGS of window_capacity(W, window_slack) columns (cache.QuantK(window=W)) and
        # every token sees the fp16 sink tokens and the W newest tokens up to its own; maxseqlen then bounds nothing
        self.sliding_window = None if not sliding_window else int(sliding_window)
        ring = {}
        if self.sliding_window is not None:
            maxseqlen = window_capacity(self.sliding_window, window_slack)
            ring = dict(window=self.sliding_window)
        # scaled RoPE: rope_scaling = a transformers rope_scaling / rope_parameters dict or a kvquant_amd.rope.RopeSpec
        # (max_position_embeddings: the model's, which dynamic NTK scales from); None = default RoPE (theta rule)
        self.rope = rope_mod.spec_of(rope_theta, rope_scaling, max_position_embeddings)
        if use_orig_sparse:
            rope_mod.require_default(self.rope, "use_orig_sparse (the uncapped CSR kernels)")
        self.hidden_size = hidden_size
        self.num_heads = num_heads
        self.head_dim = hidden_size // num_heads
        # grouped-query attention: num_key_value_heads KV heads, query head h reads KV head h // G (None: MHA)
        self.num_key_value_heads = num_heads if num_key_value_heads is None else int(num_key_value_heads)
        self.num_kv_groups = gqa_groups(num_heads, self.num_key_value_heads)
        gqa = self.num_kv_groups > 1
        if gqa and (compact or use_orig_sparse):
            raise ValueError("grouped-query attention: the compact outlier format and the uncapped (orig) CSR variants "
                             "are MHA only")
        kv_hidden = self.num_key_value_heads * self.head_dim
        if gqa and kv_hidden % 32:
            raise ValueError("grouped-query attention: num_key_value_heads * head_dim must be a multiple of 32")
        self.first_few_fp16 = first_few_fp16
        self.rope_theta = rope_theta
        kw = dict(device=device, dtype=dtype)
        if make_proj:     # (kvquant_amd.llama wraps a model's own projections and only uses attend())
            self.q_proj = nn.Linear(hidden_size, hidden_size, bias=bias, **kw)
            self.k_proj = nn.Linear(hidden_size, kv_hidden, bias=bias, **kw)
            self.v_proj = nn.Linear(hidden_size, kv_hidden, bias=bias, **kw)
            self.o_proj = nn.Linear(hidden_size, hidden_size, bias=bias, **kw)
        self.rotary_emb = RotaryDynamic(self.head_dim, base=rope_theta, device=device, rope=self.rope)
        self.kcache = QuantK(bits=abits, hidden_size=kv_hidden, num_heads=self.num_key_value_heads,
                             max_position_embeddings=maxseqlen, include_sparse=include_sparse,
                             sparsity_threshold=sparsity_threshold, rope_theta=rope_theta,
                             first_few_fp16=first_few_fp16, device=device, compact=compact, rope_scaling=self.rope,
                             **ring)
        self.vcache = QuantV(bits=abits, hidden_size=kv_hidden, num_heads=self.num_key_value_heads,
                             max_position_embeddings=maxseqlen, include_sparse=include_sparse,
                             sparsity_threshold=sparsity_threshold, first_few_fp16=first_few_fp16,
                             device=device, compact=compact, **ring)
        if first_few_fp16 > 0:
            self.kcache_fp16 = torch.zeros((1, self.num_key_value_heads, self.head_dim, first_few_fp16), dtype=dtype,
                                           device=self.kcache.device)
            self.vcache_fp16 = torch.zeros((1, self.num_key_value_heads, first_few_fp16, self.head_dim), dtype=dtype,
                                           device=self.kcache.device)

    def load_quantizers(self, k_quantizer, v_quantizer, include_sparse=True, sparsity_threshold=0.99, norm=False):
        """deployment/llama.py:186-198."""
        self.kcache.reset()
        self.vcache.reset()
        self.kcache.load_lookup_table(k_quantizer, include_sparse, sparsity_threshold, norm)
        self.vcache.load_lookup_table(v_quantizer, include_sparse, sparsity_threshold, norm)

    def reset(self):
        self.kcache.reset()
        self.vcache.reset()

    def rollback(self, n_tokens):
        """Drop the newest n_tokens tokens from both caches (the rejected tail of a verified draft): QuantK.truncate /
        QuantV.truncate.  Refused while the fp16 sink caches are still filling, and for tokens that live there."""
        kc, vc = self.kcache, self.vcache
        if kc.klen != vc.vlen:
            raise ValueError("rollback: K and V caches are out of step (%d / %d tokens)" % (kc.klen, vc.vlen))
        if kc.klen < self.first_few_fp16:
            raise ValueError("rollback while the fp16 sink cache is still filling (len %d < %d)"
                             % (kc.klen, self.first_few_fp16))
        if getattr(kc, "use_orig_sparse", False):
            raise NotImplementedError("rollback: the uncapped (orig) CSR state grows by concatenation")
        if not 0 <= int(n_tokens) <= kc.klen - self.first_few_fp16:
            raise ValueError("rollback(%d): %d compressed tokens behind the %d fp16 sink tokens"
                             % (n_tokens, kc.klen - self.first_few_fp16, self.first_few_fp16))
        kc.truncate(n_tokens)
        vc.truncate(n_tokens)

    def keep_path(self, S, keep):
        """Of the newest S tokens (the rows of a verified draft tree) keep the rows `keep` (ascending, keep[0] == 0: the
        accepted root-to-leaf path) in both caches, one launch (cache.keep_kv -> kvq_keep_columns); the lengths move back
        by S - len(keep).  keep = 0 .. n-1 is rollback(S - n).  Refused like rollback, and for compact caches."""
        kc = self.kcache
        if self.sliding_window is not None:
            raise ValueError("keep_path: draft trees are not taken on a sliding-window layer (ring caches)")
        if kc.klen < self.first_few_fp16:
            raise ValueError("keep_path while the fp16 sink cache is still filling (len %d < %d)"
                             % (kc.klen, self.first_few_fp16))
        keep_kv(kc, self.vcache, S, keep)

    # ------------------------------------------------------------------ core (post-projection states)
    def _sink_caches(self):
        """(k_sink, v_sink) of decode_kv / chunk_kv: the fp16 sink caches, or (None, None) without sink tokens"""
        if self.first_few_fp16 > 0:
            return self.kcache_fp16[0], self.vcache_fp16[0]
        return None, None

    def attend(self, query_states, key_states, value_states):
        """query_states: [1, H, q_len, hd], key / value_states: [1, num_key_value_heads, q_len, hd] (pre-RoPE),
        activation dtype.  Returns attn_output [1, q_len, hidden] (before o_proj).  Grouped-query attention
        (G = num_kv_groups > 1) runs the same three phases -- prefill, sink filling with the KV heads repeated per
        group, one-call decode -- and refuses the configurations for which MHA falls back to the multi-launch tail."""
        if self.sliding_window is not None:
            return self._attend_window(query_states, key_states, value_states)
        return self._attend_linear(query_states, key_states, value_states)

    def _attend_linear(self, query_states, key_states, value_states):
        """attend() over linear caches: prefill, sink filling, decode, chunks.  A sliding-window layer runs the prefill
        piece and the sink-filling tokens of its route through it (_attend_window); neither touches a ring's wrap."""
        bsz, H, q_len, hd = query_states.shape
        assert bsz == 1, "batch 1 only (ML:1801)"
        if self.tree is not None and not (q_len > 1 and self.kcache.klen > 0):
            raise ValueError("draft tree of %d rows: a chunk of %d row(s) on a cache of %d tokens is no tree round"
                             % (len(self.tree), q_len, self.kcache.klen))
        if q_len > 1 and self.kcache.klen > 0:
            return self.attend_multi(query_states, key_states, value_states)
        G = self.num_kv_groups
        sinks = self.first_few_fp16
        key_states = key_states.half()
        value_states = value_states.half()
        start = self.kcache.klen
        cos, sin = self.rotary_emb(value_states, start, start + q_len)
        fused = self.kcache.include_sparse and self.vcache.include_sparse
        if G > 1 and not (fused and hd == 128):
            raise ValueError("grouped-query attention needs include_sparse caches and head_dim 128")
        if q_len == 1 and start >= sinks:
            f16 = query_states.dtype == torch.float16 and (sinks == 0 or self.kcache_fp16.dtype == torch.float16)
            if G > 1 and not f16:
                raise ValueError("grouped-query attention decodes fp16 activations")
            if f16 and fused and hd == 128 and (G > 1 or sinks == 0 or self.fuse_sinks):
                # ---- decode over the compressed cache (ML:1948-2006), GPU-resident: the query's RoPE in one launch
                # (kvq_rope_q_f16: torch's fp16 roundings), then one library call for the layer's KV path
                # (kvq_decode_step; kvq_decode_step_gqa for G > 1)
                q_rope = ops.rope_q_f16(query_states.reshape(H, hd), cos[0], sin[0])
                k_sink, v_sink = self._sink_caches()
                out, _ = decode_kv(self.kcache, self.vcache, q_rope, key_states.flatten(), value_states.flatten(),
                                   k_sink=k_sink, v_sink=v_sink)
                return out.half().view(bsz, q_len, self.hidden_size)
        query_rope = (query_states * cos) + (rotate_half(query_states) * sin)

        if q_len > 1 and self.kcache.klen == 0:
            # ---- prefill (ML:1861-1927) ------------------------------------------------------------
            key_rope = (key_states * cos) + (rotate_half(key_states) * sin)
            # causal attention of the prompt on the matrix cores (kvq_prefill_attention[_gqa], hand-written MFMA flash
            # kernel; the reference calls flash-attn here, ML:1869-1873); output token-major, ready for o_proj
            attn_output = ops.prefill_attention(query_rope[0].half(), key_rope[0], value_states[0]) \
                .view(bsz, q_len, self.hidden_size).to(query_states.dtype)
            if sinks > 0:
                n = min(sinks, q_len)
                self.kcache_fp16[:, :, :, :n] = key_rope[:, :, :n, :].transpose(2, 3)
                self.vcache_fp16[:, :, :n, :] = value_states[:, :, :n, :]
                if q_len > sinks:
                    self.kcache.parallel_pack(key_states[0, :, sinks:, :].transpose(1, 2))
                    self.vcache.parallel_pack(value_states[0, :, sinks:, :].transpose(1, 2))
                self.kcache.klen += n
                self.vcache.vlen += n
            else:
                self.kcache.parallel_pack(key_states[0].transpose(1, 2))
                self.vcache.parallel_pack(value_states[0].transpose(1, 2))
            return attn_output

        assert q_len == 1, "decode feeds one token at a time (generation/utils.py kvquant hooks)"
        inv = 1.0 / math.sqrt(hd)
        if self.kcache.klen < sinks:
            # ---- still filling the fp16 sink caches (ML:1932-1946, 1981-1984); G > 1: KV heads repeated per group
            key_rope = (key_states * cos) + (rotate_half(key_states) * sin)
            self.kcache_fp16[:, :, :, self.kcache.klen] = key_rope.transpose(2, 3).squeeze(-1)
            self.kcache.klen += 1
            ks = self.kcache_fp16[:, :, :, :self.kcache.klen]
            w = torch.matmul(query_rope, ks if G == 1 else ks.repeat_interleave(G, dim=1)) / math.sqrt(hd)
            w = F.softmax(w, dim=-1, dtype=torch.float32).to(query_rope.dtype)
            self.vcache_fp16[:, :, self.vcache.vlen, :] = value_states.squeeze(2)
            self.vcache.vlen += 1
            vs = self.vcache_fp16[:, :, :self.vcache.vlen, :]
            out = torch.matmul(w, vs if G == 1 else vs.repeat_interleave(G, dim=1))
            return out.transpose(1, 2).reshape(bsz, q_len, self.hidden_size)

        # ---- decode over the compressed cache (ML:1948-2006), GPU-resident, multi-launch (MHA only: for G > 1 the
        # one-call decode above has returned or raised) ------------------------------------------------
        sink_scores = None
        fuse_sinks = fused and sinks > 0 and self.fuse_sinks and self.kcache_fp16.dtype == torch.float16
        if sinks > 0 and not fuse_sinks:
            sink_scores = (torch.matmul(query_rope, self.kcache_fp16) / math.sqrt(hd))[0, :, 0, :].contiguous()
        if fuse_sinks:
            # the sink tokens' two fp16 matmuls, division and add ride in the decode launches (decode_kv docstring;
            # the sum of the two parts is then rounded to fp16 once instead of twice)
            out, _ = decode_kv(self.kcache, self.vcache, query_rope[0, :, 0, :].contiguous(), key_states.flatten(),
                               value_states.flatten(), k_sink=self.kcache_fp16[0], v_sink=self.vcache_fp16[0])
            out = out.transpose(0, 1).half().unsqueeze(0)
            return out.transpose(1, 2).contiguous().reshape(bsz, q_len, self.hidden_size)
        if fused:
            out, sink_probs = decode_kv(self.kcache, self.vcache, query_rope[0, :, 0, :].contiguous(),
                                        key_states.flatten(), value_states.flatten(), sink_scores)
            out = out.transpose(0, 1).half()                                   # [H, 1, hd]
        else:
            q32 = query_rope[0].float().transpose(0, 1).contiguous()             # [1, H, hd]
            scores = self.kcache.append_and_score(q32, key_states.flatten().float())
            probs, sink_probs = ops.softmax_scale(scores[0], inv, sink_scores)
            out = self.vcache.forward_fused_sparse(probs.unsqueeze(1).half(), value_states)
        out = out.unsqueeze(0)
        if sinks > 0:
            out = out + torch.matmul(sink_probs.view(1, H, 1, sinks), self.vcache_fp16)
        return out.transpose(1, 2).contiguous().reshape(bsz, q_len, self.hidden_size)

    # ------------------------------------------------------------------ sliding-window layers (ring caches)
    def _attend_window(self, query_states, key_states, value_states):
        """attend() of a sliding-window layer (window_route): the existing prefill and sink filling for the start of
        the stream, everything else -- decode tokens, follow-up chunks, the rest of a long prompt, chain drafts --
        through _attend_chunk on the ring caches."""
        if self.tree is not None:
            raise ValueError("draft trees are not taken on a sliding-window layer (ring caches)")
        if not (query_states.dtype == torch.float16 and self.head_dim == 128
                and (self.first_few_fp16 == 0 or self.kcache_fp16.dtype == torch.float16)):
            raise ValueError("sliding-window attention runs the chunk kernel only: fp16 activations, fp16 sink caches, "
                             "head_dim 128")
        q_len = query_states.shape[2]
        route = window_route(self.kcache.klen, q_len, self.first_few_fp16, self.sliding_window, self.kcache.max_len)
        outs, i = [], 0
        for kind, n in route:
            q, k, v = (t[:, :, i:i + n] for t in (query_states, key_states, value_states))
            if kind == "chunk":
                outs.append(self._attend_chunk(q, k, v))
            elif kind == "prefill":
                outs.append(self._attend_linear(q, k, v))
            else:
                outs.extend(self._attend_linear(q[:, :, j:j + 1], k[:, :, j:j + 1], v[:, :, j:j + 1]) for j in range(n))
            i += n
        if len(outs) == 1:
            return outs[0]
        return torch.cat([o.to(query_states.dtype) for o in outs], dim=1)

    # ------------------------------------------------------------------ q_len > 1 on a warm cache
    def chunk_fast(self, query_states):
        """True if a chunk of this layer can take kvq_chunk_attention: Dense-and-Sparse caches in the reference outlier
        format (not compact, not the uncapped CSR variants), fp16 activations, head_dim 128, fp16 sink caches."""
        kc, vc, sinks = self.kcache, self.vcache, self.first_few_fp16
        return (CHUNK_ATTEND and kc.include_sparse and vc.include_sparse and not kc.compact and not vc.compact
                and not getattr(kc, "use_orig_sparse", False) and query_states.dtype == torch.float16
                and self.head_dim == 128 and (sinks == 0 or self.kcache_fp16.dtype == torch.float16))

    def attend_multi(self, query_states, key_states, value_states):
        """q_len > 1 tokens into a cache that already holds klen > 0 tokens (a follow-up prompt, a draft to verify, the
        next piece of a chunked fill): the positions continue at klen.  Tokens that still fill the fp16 sink cache go
        one at a time through the q_len == 1 path, the rest through chunk_kv (the chunk's own tokens are attended AS
        STORED, compressed, like token-by-token decoding) -- or one at a time where chunk_fast() is False."""
        q_len = query_states.shape[2]
        if self.tree is not None:
            # a tree cannot be fed token by token: every refusal is an error
            if not self.chunk_fast(query_states):
                raise ValueError("draft tree: this layer's configuration does not take the chunk kernel (it needs "
                                 "include_sparse caches in the reference outlier format, fp16 activations, head_dim 128)")
            if self.kcache.klen < self.first_few_fp16:
                raise ValueError("draft tree while the fp16 sink cache is still filling (len %d < %d)"
                                 % (self.kcache.klen, self.first_few_fp16))
            if q_len != len(self.tree):
                raise ValueError("draft tree of %d rows, chunk of %d" % (len(self.tree), q_len))
            return self._attend_chunk(query_states, key_states, value_states).to(query_states.dtype)
        route = chunk_route(self.kcache.klen, q_len, self.first_few_fp16, self.chunk_fast(query_states))
        outs, i = [], 0
        for kind, n in route:
            sl = slice(i, i + n)
            if kind == "chunk":
                outs.append(self._attend_chunk(query_states[:, :, sl], key_states[:, :, sl], value_states[:, :, sl]))
            else:
                for j in range(i, i + n):
                    t = slice(j, j + 1)
                    outs.append(self.attend(query_states[:, :, t], key_states[:, :, t], value_states[:, :, t]))
            i += n
        return torch.cat([o.to(query_states.dtype) for o in outs], dim=1)

    def _attend_chunk(self, query_states, key_states, value_states):
        """one chunk (q_len >= 2, klen >= sinks) through chunk_kv: query RoPE in torch's fp16 roundings (as
        kvq_rope_q_f16 does for one token), pack + kvq_chunk_attention"""
        bsz, H, q_len, hd = query_states.shape
        start = self.kcache.klen
        if self.tree is not None:
            # row i at the position of its depth: the rotary rows of klen .. klen + max depth, indexed by depth
            idx, n_pos = _depth_index(self.tree, query_states.device)
            cos, sin = self.rotary_emb(value_states, start, start + n_pos)
            cos, sin = cos[idx], sin[idx]
        else:
            cos, sin = self.rotary_emb(value_states, start, start + q_len)
        query_rope = (query_states * cos) + (rotate_half(query_states) * sin)
        k = key_states[0].half().transpose(1, 2)
        v = value_states[0].half().transpose(1, 2)
        k_sink, v_sink = self._sink_caches()
        kw = {} if self.tree is None else dict(parent=self.tree)      # (no tree: the call of every release before)
        out = chunk_kv(self.kcache, self.vcache, query_rope[0], k, v, k_sink=k_sink, v_sink=v_sink, **kw)
        return out.to(query_states.dtype).view(bsz, q_len, self.hidden_size)

    def forward(self, hidden_states):
        """hidden_states [1, q_len, hidden] -> [1, q_len, hidden]."""
        bsz, q_len, _ = hidden_states.shape
        shape = (bsz, q_len, self.num_heads, self.head_dim)
        kv_shape = (bsz, q_len, self.num_key_value_heads, self.head_dim)
        q = self.q_proj(hidden_states).view(shape).transpose(1, 2)
        k = self.k_proj(hidden_states).view(kv_shape).transpose(1, 2)
        v = self.v_proj(hidden_states).view(kv_shape).transpose(1, 2)
        return self.o_proj(self.attend(q, k, v))
