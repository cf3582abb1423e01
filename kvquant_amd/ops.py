"""Typed wrappers over the C ABI of libkvq.so (include/kvq.h): torch tensors in,
raw device pointers + torch's current stream out.  Argument checks raise
ValueError; a failing library call raises KvqError.  No CPU path."""
import ctypes
import os

import torch

from . import _lib

_ws = {}  # (slot, device index, stream) -> workspace tensor


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, dtype, name):
    if not torch.is_tensor(t):
        raise ValueError("%s: expected a tensor" % name)
    if not t.is_cuda:
        raise ValueError("%s: expected a GPU tensor (got %s); kvquant_amd has no CPU path" % (name, t.device))
    if t.dtype != dtype:
        raise ValueError("%s: expected dtype %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s: expected a contiguous tensor" % name)
    return t.data_ptr()


def _f(t, name):
    return _chk(t, torch.float32, name)


def _i(t, name):
    return _chk(t, torch.int32, name)


def _fo(t, name):
    """optional f32 tensor -> pointer / None (compact formats carry no value array: include/kvq.h)"""
    return None if t is None else _chk(t, torch.float32, name)


def _io(t, name):
    return None if t is None else _chk(t, torch.int32, name)


def _cache_dims(mat, bits):
    if mat.dim() != 3:
        raise ValueError("mat: expected [num_heads, head_dim/32*bits, max_len]")
    H, W, max_len = mat.shape
    if W % bits:
        raise ValueError("mat.shape[1]=%d is not a multiple of bits=%d" % (W, bits))
    return H, W // bits * 32, max_len


def _workspace(device, nbytes, slot="mix"):
    """Scratch buffers of the library calls (score tables + fp32 query, softmax partials, p.V slabs), one per
    (slot, device, STREAM): calls on one stream are ordered, so consecutive layers can share them; work on another
    stream of the same device (the reference runs a side stream, ML:1804-1820) gets its own and cannot clobber
    tables or partials that are still being read.  A buffer that has to grow is replaced on its own stream,
    where the caching allocator orders the reuse of the old one."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (slot, idx, torch.cuda.current_stream(idx).cuda_stream)
    w = _ws.get(key)
    if w is None or w.numel() < nbytes:
        # grow geometrically: the decode workspaces grow by a few hundred bytes per token, and a buffer sized exactly
        # would be replaced every other token once it is past the 1 MiB floor (allocator churn in the hot path)
        grown = 0 if w is None else w.numel() + (w.numel() >> 1)
        w = torch.empty(max(nbytes, grown, 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = w
    return w


class _Dev:
    """device guard equivalent to the reference's OptionalCUDAGuard"""

    def __init__(self, t):
        self.idx = t.device.index
        self.prev = None

    def __enter__(self):
        if self.idx is not None and self.idx != torch.cuda.current_device():
            self.prev = torch.cuda.current_device()
            torch.cuda.set_device(self.idx)

    def __exit__(self, *a):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)




def _L():
    return _lib.lib()


def _rope(rope, device):
    """scaled RoPE argument of the _rope entry points: None (the theta rule) or (inv_freq f32 [64] on `device`,
    attention factor) -> ctypes pointer to a struct kvq_rope, or None (include/kvq.h: kvq_rope)"""
    if rope is None:
        return None
    inv, af = rope
    if not (torch.is_tensor(inv) and tuple(inv.shape) == (64,)):
        raise ValueError("rope: expected (inv_freq f32 [64], attention_factor)")
    if inv.device != device:
        raise ValueError("rope: the frequency table is on %s, the cache on %s" % (inv.device, device))
    af = float(af)
    if not (af > 0 and af < float("inf")):
        raise ValueError("rope: attention factor %r must be finite and > 0" % af)
    return ctypes.byref(_lib.Rope(_f(inv, "inv_freq"), af))


def rope_freqs(theta, device=None):
    """theta_j = powf(theta, -2j/128), j < 64, as the score kernels evaluate them (on the device)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty(64, dtype=torch.float32, device=dev)
    with _Dev(out):
        _lib.check(_L().kvq_rope_freqs(float(theta), out.data_ptr(), _stream()), "kvq_rope_freqs")
    return out


def rope_q_f16(q, cos, sin):
    """q f16 [H, 128] (contiguous), cos / sin f16 [128] -> q * cos + rotate_half(q) * sin, f16 [H, 128], with torch's fp16
    roundings (kvq_rope_q_f16): the decode query's RoPE of the patched attention in one launch"""
    out = torch.empty_like(q)
    with _Dev(q):
        _lib.check(_L().kvq_rope_q_f16(_chk(q, torch.float16, "q"), _chk(cos, torch.float16, "cos"),
                                       _chk(sin, torch.float16, "sin"), out.data_ptr(), q.shape[0], q.shape[1], _stream()),
                   "kvq_rope_q_f16")
    return out


def append_k(bits, mat, lut, x, col):
    H, hd, max_len = _cache_dims(mat, bits)
    with _Dev(mat):
        _lib.check(_L().kvq_append_k(bits, _i(mat, "mat"), _f(lut, "lookup_table"), _f(x, "newvec"), H, hd,
                                     max_len, int(col), _stream()), "kvq_append_k")


def append_v(bits, mat, lut_rows, x, col):
    H, hd, max_len = _cache_dims(mat, bits)
    with _Dev(mat):
        _lib.check(_L().kvq_append_v(bits, _i(mat, "mat"), _f(lut_rows, "lookup_table"), _f(x, "newvec"), H, hd,
                                     max_len, int(col), _stream()), "kvq_append_v")


def append_k_sparse(bits, mat, lut, x, rescaled, lo, hi, col):
    H, hd, max_len = _cache_dims(mat, bits)
    with _Dev(mat):
        _lib.check(_L().kvq_append_k_sparse(bits, _i(mat, "mat"), _f(lut, "lookup_table"), _f(x, "newvec"),
                                            _f(rescaled, "outliers_rescaled"), _f(lo, "lower"), _f(hi, "upper"),
                                            H, hd, max_len, int(col), _stream()), "kvq_append_k_sparse")


def append_v_sparse(bits, mat, lut_rows, x, lo, hi, col):
    H, hd, max_len = _cache_dims(mat, bits)
    with _Dev(mat):
        _lib.check(_L().kvq_append_v_sparse(bits, _i(mat, "mat"), _f(lut_rows, "lookup_table"), _f(x, "newvec"),
                                            float(lo), float(hi), H, hd, max_len, int(col), _stream()),
                   "kvq_append_v_sparse")


def pack_k_sparse_parallel(bits, mat, lut, x, rescaled, lo, hi, col0=0):
    H, hd, max_len = _cache_dims(mat, bits)
    S = x.shape[-1]
    with _Dev(mat):
        _lib.check(_L().kvq_pack_k_sparse_parallel(bits, _i(mat, "mat"), _f(lut, "lookup_table"), _f(x, "newvec"),
                                                   _f(rescaled, "outliers_rescaled"), _f(lo, "lower"),
                                                   _f(hi, "upper"), H, hd, S, max_len, int(col0), _stream()),
                   "kvq_pack_k_sparse_parallel")


def pack_v_sparse_parallel(bits, mat, lut_rows, x, lo, hi, col0=0):
    H, hd, max_len = _cache_dims(mat, bits)
    S = x.shape[-1]
    with _Dev(mat):
        _lib.check(_L().kvq_pack_v_sparse_parallel(bits, _i(mat, "mat"), _f(lut_rows, "lookup_table"),
                                                   _f(x, "newvec"), _f(lo, "lower"), _f(hi, "upper"), H, hd, S,
                                                   max_len, int(col0), _stream()), "kvq_pack_v_sparse_parallel")


def score_k(bits, q, mat, mul, lut, L, theta, pos_offset, outliers=None, outlier_indices=None,
            accumulate=True, rope=None):
    """q [q_len,H,128] f32, mul [q_len,H,L] f32 (in place).  rope: None (theta rule) or (inv_freq, attention factor)."""
    H, hd, max_len = _cache_dims(mat, bits)
    if q.dim() != 3 or mul.dim() != 3 or q.shape[0] != mul.shape[0]:
        raise ValueError("vec must be [q_len, H, head_dim] and mul [q_len, H, kcachelen]")
    if mul.shape[2] != L:
        raise ValueError("mul.shape[2] must equal kcachelen")
    n_out = 0 if outliers is None else outliers.shape[1]
    with _Dev(q):
        nbytes = _L().kvq_score_k_workspace_bytes(bits, q.shape[0], H)
        ws = _workspace(q.device, nbytes, slot="score")
        _lib.check(_L().kvq_score_k_rope(
            bits, _f(q, "vec"), _i(mat, "mat"), _f(mul, "mul"), _f(lut, "lookup_table"), q.shape[0], H, hd,
            int(L), max_len, float(theta), int(pos_offset),
            None if outliers is None else _f(outliers, "outliers"),
            None if outliers is None else _i(outlier_indices, "outlier_indices"), n_out,
            1 if accumulate else 0, ws.data_ptr(), ws.numel(), _rope(rope, mat.device), _stream()), "kvq_score_k_rope")


def outlier_mirror_rows(outliers, outlier_indices, outliers_t, outlier_indices_t, t0, t1):
    """rows [t0, t1) of the reference's outlier rows [max_len, n_out] -> columns [t0, t1) of the token-contiguous
    mirror [n_out, max_len] (include/kvq.h: kvq_outlier_mirror_rows)."""
    max_len, n_out = outliers.shape
    if tuple(outlier_indices.shape) != (max_len, n_out) or tuple(outliers_t.shape) != (n_out, max_len) or \
            tuple(outlier_indices_t.shape) != (n_out, max_len):
        raise ValueError("outlier rows must be [max_len, n_out] and the mirror [n_out, max_len]")
    with _Dev(outliers):
        _lib.check(_L().kvq_outlier_mirror_rows(
            _f(outliers, "outliers"), _i(outlier_indices, "outlier_indices"), _f(outliers_t, "outliers_t"),
            _i(outlier_indices_t, "outlier_indices_t"), n_out, max_len, int(t0), int(t1), _stream()),
            "kvq_outlier_mirror_rows")


def score_k_mirror(bits, q, mat, mul, lut, L, theta, pos_offset, outliers_t, outlier_indices_t, accumulate=True):
    """score_k (q_len = 1) over the token-contiguous outlier mirror [n_out, max_len]: the decode kernel's variant behind
    the legacy call's semantics (include/kvq.h: kvq_score_k_mirror)."""
    H, hd, max_len = _cache_dims(mat, bits)
    if q.dim() != 3 or mul.dim() != 3 or q.shape[0] != 1 or mul.shape[0] != 1:
        raise ValueError("vec must be [1, H, head_dim] and mul [1, H, kcachelen]")
    if mul.shape[2] != L:
        raise ValueError("mul.shape[2] must equal kcachelen")
    n_out = outliers_t.shape[0]
    if tuple(outliers_t.shape) != (n_out, max_len) or tuple(outlier_indices_t.shape) != (n_out, max_len):
        raise ValueError("the outlier mirror must be [n_out, max_len]")
    with _Dev(q):
        nbytes = _L().kvq_score_k_workspace_bytes(bits, 1, H)
        ws = _workspace(q.device, nbytes, slot="score")
        _lib.check(_L().kvq_score_k_mirror(
            bits, _f(q, "vec"), _i(mat, "mat"), _f(mul, "mul"), _f(lut, "lookup_table"), H, hd, int(L), max_len,
            float(theta), int(pos_offset), _f(outliers_t, "outliers_t"), _i(outlier_indices_t, "outlier_indices_t"),
            n_out, 1 if accumulate else 0, ws.data_ptr(), ws.numel(), _stream()), "kvq_score_k_mirror")


def mix_v(bits, p, mat, mul, lut_rows, L, outliers=None, outlier_indices=None, accumulate=True):
    """p [q_len,H,L] f32, mul [q_len,H,128] f32 (in place)."""
    H, hd, max_len = _cache_dims(mat, bits)
    if p.dim() != 3 or mul.dim() != 3 or p.shape[0] != mul.shape[0]:
        raise ValueError("vec must be [q_len, H, vcachelen] and mul [q_len, H, head_dim]")
    if p.shape[2] != L:
        raise ValueError("vec.shape[2] must equal vcachelen")
    q_len = p.shape[0]
    # (outlier_indices without outliers: COMPACT rows, packed entries in the index array)
    n_out = 0 if outlier_indices is None else outlier_indices.shape[1]
    with _Dev(p):
        nbytes = _L().kvq_mix_v_workspace_bytes(bits, q_len, H, hd, int(L))
        ws = _workspace(p.device, nbytes)
        _lib.check(_L().kvq_mix_v(
            bits, _f(p, "vec"), _i(mat, "mat"), _f(mul, "mul"), _f(lut_rows, "lookup_table"), q_len, H, hd,
            int(L), max_len, _fo(outliers, "outliers"), _io(outlier_indices, "outlier_indices"), n_out,
            1 if accumulate else 0, ws.data_ptr(), ws.numel(), _stream()), "kvq_mix_v")


def _mirror(outliers_t, outlier_indices_t, thr_k, max_len):
    """(ptr, ptr) of the optional token-contiguous K outlier mirror [2*thr_k, max_len], or (None, None)"""
    if outlier_indices_t is None:
        if outliers_t is not None:
            raise ValueError("the outlier mirror needs its index array")
        return None, None
    if tuple(outlier_indices_t.shape) != (2 * thr_k, max_len) or \
            (outliers_t is not None and tuple(outliers_t.shape) != (2 * thr_k, max_len)):
        raise ValueError("the outlier mirror must be [%d, %d]" % (2 * thr_k, max_len))
    # (index array alone: the COMPACT mirror, packed entries fp16 residual << 16 | channel)
    return _fo(outliers_t, "outliers_t"), _i(outlier_indices_t, "outlier_indices_t")


def append_k_fused(bits, mat, lut, lut_off, x, lo, hi, outliers, outlier_indices, thr_k, col, outliers_t=None,
                   outlier_indices_t=None):
    """pack + rescale + exact top-thr_k selection + outlier row, one launch (include/kvq.h)."""
    H, hd, max_len = _cache_dims(mat, bits)
    if outliers.shape[1] != 2 * thr_k or outlier_indices.shape[1] != 2 * thr_k:
        raise ValueError("outlier buffers must be %d wide" % (2 * thr_k))
    with _Dev(mat):
        _lib.check(_L().kvq_append_k_fused(bits, _i(mat, "mat"), _f(lut, "lookup_table"), _f(lut_off, "lut_off"),
                                           _f(x, "newvec"), _f(lo, "lower"), _f(hi, "upper"),
                                           _f(outliers, "outliers"), _i(outlier_indices, "outlier_indices"),
                                           int(thr_k), H, hd, max_len, int(col),
                                           *_mirror(outliers_t, outlier_indices_t, thr_k, max_len), _stream()),
                   "kvq_append_k_fused")


def _vnorm(norm):
    """norm: None or (lut_rows2 f32 [max_len, 2^bits] or None, normscale, normoffset, zp_from_rows2,
    reference_tie_quirk) -> struct kvq_vopts (ctypes hands a const kvq_vopts * parameter its address) / None"""
    if norm is None:
        return None
    rows2, ns, no, zp2, quirk = norm
    return _lib.VNorm(None if rows2 is None else _f(rows2, "lookup_table2"), float(ns), float(no),
                      1 if zp2 else 0, 1 if quirk else 0)


def append_v_fused(bits, mat, lut_rows, lut_sorted, x, outliers, outlier_indices, thr_k, col, norm=None):
    """top-(thr_k+1) thresholds + codebook row + pack + outlier row, one launch."""
    H, hd, max_len = _cache_dims(mat, bits)
    if outliers.shape[1] != 2 * thr_k or outlier_indices.shape[1] != 2 * thr_k:
        raise ValueError("outlier buffers must be %d wide" % (2 * thr_k))
    if lut_sorted.numel() != 2 ** bits:
        raise ValueError("lut_sorted must have 2^bits entries")
    with _Dev(mat):
        _lib.check(_L().kvq_append_v_fused(bits, _i(mat, "mat"), _f(lut_rows, "lookup_table"),
                                           _f(lut_sorted, "lut"), _f(x, "newvec"), _f(outliers, "outliers"),
                                           _i(outlier_indices, "outlier_indices"), int(thr_k), H, hd, max_len,
                                           int(col), _vnorm(norm), _stream()), "kvq_append_v_fused")


def pack_k_fused(bits, mat, lut, lut_off, x, lo, hi, outliers, outlier_indices, thr_k, col0, outliers_t=None,
                 outlier_indices_t=None):
    """prefill: x f32 [H, hd, S] (channel-major prompt) -> columns col0.. of the cache + outlier rows, one launch."""
    H, hd, max_len = _cache_dims(mat, bits)
    S = x.shape[-1]
    if x.numel() != H * hd * S:
        raise ValueError("x must be [H, hd, S]")
    with _Dev(mat):
        _lib.check(_L().kvq_pack_k_fused(bits, _i(mat, "mat"), _f(lut, "lookup_table"), _f(lut_off, "lut_off"),
                                         _f(x, "newvec"), _f(lo, "lower"), _f(hi, "upper"),
                                         _fo(outliers, "outliers"), _io(outlier_indices, "outlier_indices"),
                                         int(thr_k), H, hd, max_len, int(col0), int(S),
                                         *_mirror(outliers_t, outlier_indices_t, thr_k, max_len), _stream()),
                   "kvq_pack_k_fused")


def pack_v_fused(bits, mat, lut_rows, lut_sorted, x, outliers, outlier_indices, thr_k, col0, norm=None):
    """prefill: x f32 [H, hd, S] -> cache columns, per-token codebook rows and outlier rows, one launch."""
    H, hd, max_len = _cache_dims(mat, bits)
    S = x.shape[-1]
    if x.numel() != H * hd * S:
        raise ValueError("x must be [H, hd, S]")
    with _Dev(mat):
        _lib.check(_L().kvq_pack_v_fused(bits, _i(mat, "mat"), _f(lut_rows, "lookup_table"), _f(lut_sorted, "lut"),
                                         _f(x, "newvec"), _fo(outliers, "outliers"),
                                         _i(outlier_indices, "outlier_indices"), int(thr_k), H, hd, max_len,
                                         int(col0), int(S), _vnorm(norm), _stream()), "kvq_pack_v_fused")


def softmax_scale(scores, inv_sqrt_hd, sink_scores=None):
    """scores: f32 [H, L] raw q.K^T; sink_scores: f16 [H, n_sink] already scaled, or None.
    Returns (probs f32 [H, L] holding fp16-rounded values, sink_probs f16 [H, n_sink] or None)."""
    if scores.dim() != 2:
        raise ValueError("scores must be [H, L]")
    H, L = scores.shape
    n_sink = 0 if sink_scores is None else sink_scores.shape[1]
    probs = torch.empty_like(scores)
    sink_probs = None if sink_scores is None else torch.empty_like(sink_scores)
    with _Dev(scores):
        nbytes = _L().kvq_softmax_workspace_bytes(H, L)
        ws = _workspace(scores.device, nbytes + (1 << 16), slot="softmax")
        _lib.check(_L().kvq_softmax_scale(
            _f(scores, "scores"), None if sink_scores is None else _chk(sink_scores, torch.float16, "sink_scores"),
            _f(probs, "probs"), None if sink_probs is None else sink_probs.data_ptr(), H, L, n_sink,
            float(inv_sqrt_hd), ws.data_ptr(), ws.numel(), _stream()), "kvq_softmax_scale")
    return probs, sink_probs


# ---- uncapped ("orig") CSR / CSC variants, 4 bit --------------------------------------------------
def _grow(ptr, minor, val, start, idx, v, pos):
    """the reference's host-side CSR/CSC growth (KCU:763-829, 1010-1060) on device tensors"""
    dev = idx.device
    cnt = idx.numel()
    if ptr.numel() == 0:
        ptr2 = torch.tensor([0, cnt], dtype=torch.int32, device=dev)
        minor2, val2 = idx, v
        nt = (cnt + 9) // 10
        start2 = torch.full((nt,), pos, dtype=torch.int32, device=dev)
    else:
        ptr2 = torch.cat((ptr.int(), torch.tensor([minor.numel() + cnt], dtype=torch.int32, device=dev)))
        if cnt > 0:
            minor2 = torch.cat((minor.int(), idx))
            val2 = torch.cat((val.float(), v))
            nt = (minor2.numel() + 9) // 10
            new_alloc = nt - start.numel()
            start2 = torch.cat((start.int(), torch.full((new_alloc,), pos, dtype=torch.int32, device=dev))) \
                if new_alloc > 0 else start
        else:
            minor2, val2, start2 = minor, val, start
            nt = (minor2.numel() + 9) // 10
    return ptr2, minor2, val2, start2, nt


def _append_orig(is_v, mat, lut, x, zeropoint, lo, hi, col):
    H, hd, max_len = _cache_dims(mat, 4)
    C = H * hd
    oi = torch.empty(C, dtype=torch.int32, device=mat.device)
    ov = torch.empty(C, dtype=torch.float32, device=mat.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=mat.device)
    with _Dev(mat):
        if is_v:
            _lib.check(_L().kvq_append_v_sparse_orig(_i(mat, "mat"), _f(lut, "lookup_table"), _f(x, "newvec"),
                                                     float(zeropoint), float(lo), float(hi), oi.data_ptr(),
                                                     ov.data_ptr(), cnt.data_ptr(), H, hd, max_len, int(col),
                                                     _stream()), "kvq_append_v_sparse_orig")
        else:
            _lib.check(_L().kvq_append_k_sparse_orig(_i(mat, "mat"), _f(lut, "lookup_table"), _f(x, "newvec"),
                                                     _f(zeropoint, "zeropoint"), _f(lo, "lower"), _f(hi, "upper"),
                                                     oi.data_ptr(), ov.data_ptr(), cnt.data_ptr(), H, hd, max_len,
                                                     int(col), _stream()), "kvq_append_k_sparse_orig")
    n = int(cnt.item())          # the reference synchronises here too (KCU:745-747)
    return oi[:n].clone(), ov[:n].clone(), cnt


def append_k_sparse_orig(mat, lut, x, zeropoint, row, col, val, start_rows, lo, hi, kcachelen):
    idx, v, cnt = _append_orig(False, mat, lut, x, zeropoint, lo, hi, kcachelen)
    rows, cols, vals, start, nt = _grow(row, col, val, start_rows, idx, v, kcachelen)
    return [rows, cols, vals, start, torch.tensor([nt], dtype=torch.int32), cnt]


def append_v_sparse_orig(mat, lut_rows, x, zeropoint, row, col, val, start_cols, lo, hi, vcachelen):
    idx, v, cnt = _append_orig(True, mat, lut_rows, x, zeropoint, lo, hi, vcachelen)
    cols, rows, vals, start, nt = _grow(col, row, val, start_cols, idx, v, vcachelen)
    return [rows, cols, vals, start, torch.tensor([nt], dtype=torch.int32), cnt]


def spmv_k_rope_csr(rowptr, cols, vals, q, mul, num_rows, L, theta, pos_offset):
    with _Dev(q):
        _lib.check(_L().kvq_spmv_k_rope_csr(_i(rowptr, "rows"), _i(cols, "cols") if cols.numel() else None,
                                            _f(vals, "vals") if vals.numel() else None, _f(q, "vec"), _f(mul, "mul"),
                                            int(num_rows), int(L), q.shape[2], float(theta), int(pos_offset),
                                            _stream()), "kvq_spmv_k_rope_csr")


def spmv_v_csc(colptr, rows, vals, p, mul, num_cols, L):
    H, hd = mul.shape[1], mul.shape[2]
    with _Dev(p):
        _lib.check(_L().kvq_spmv_v_csc(_i(colptr, "cols"), _i(rows, "rows") if rows.numel() else None,
                                       _f(vals, "vals") if vals.numel() else None, _f(p, "vec"), _f(mul, "mul"),
                                       int(num_cols), int(L), H, hd, _stream()), "kvq_spmv_v_csc")


# ---- one-launch decode prologue + prepared score ----------------------------------------------------
def _act(t, name):
    """activation vector: fp32 or fp16, contiguous, on the GPU -> (ptr, is_half)"""
    if t.dtype == torch.float16:
        return _chk(t, torch.float16, name), 1
    return _chk(t, torch.float32, name), 0


def _acts(q, k, v):
    """the activations of one token, all fp16 or all fp32 -> (q ptr, k ptr, v ptr, is_half)"""
    kp, kh = _act(k, "k")
    vp, vh = _act(v, "v")
    qp, qh = _act(q, "q")
    if not (kh == vh == qh):
        raise ValueError("q, k, v must share one dtype (fp32 or fp16)")
    return qp, kp, vp, qh


def _sinks(sinks, H):
    """(k_sink f16 [H, 128, n_sink], sink_scores f16 [H, n_sink] (out), inv_sqrt_hd) -> struct kvq_sinks (ctypes hands
    a const kvq_sinks * parameter its address), or None"""
    if sinks is None:
        return None
    k_sink, sink_scores, inv = sinks
    n_sink = sink_scores.shape[1]
    if tuple(k_sink.shape) != (H, 128, n_sink) or sink_scores.shape[0] != H:
        raise ValueError("sinks: k_sink [H, 128, n_sink] and sink_scores [H, n_sink] expected")
    return _lib.Sinks(_chk(k_sink, torch.float16, "k_sink"), _chk(sink_scores, torch.float16, "sink_scores"), n_sink,
                      float(inv))


def _aligned_workspace(device, nbytes, slot):
    """_workspace with its start rounded up to 256 bytes (the one-call entries carve aligned sub-buffers out of it)
    -> (base address, usable bytes from there, the tensor that owns them)"""
    ws = _workspace(device, nbytes + 256, slot=slot)
    base = (ws.data_ptr() + 255) & ~255
    return base, ws.numel() - (base - ws.data_ptr()), ws


def decode_prologue(bits, kmat, klut, klut_off, k, lo, hi, koutl, kidx, kcol, vmat, vlut_rows, vlut_sorted, v,
                    voutl, vidx, vcol, q, thr_k, koutl_t=None, kidx_t=None, klut_ends=None, klut_score=None,
                    vnorm=None, sinks=None):
    """K fused append + V fused append + K codebook images for score_k_prepared in ONE launch.
    q [H,128] (RoPE'd), k, v [C]: all fp32 or all fp16.  klut_score: table the score images are built from
    (default klut).  sinks = (k_sink f16 [H, 128, n_sink], sink_scores f16 [H, n_sink] (out), inv_sqrt_hd): the head
    workgroups also write the scaled scores of the fp16 sink tokens.  Returns the score workspace tensor."""
    H, hd, max_len = _cache_dims(kmat, bits)
    sk = _sinks(sinks, H)
    qp, kp, vp, kh = _acts(q, k, v)
    with _Dev(kmat):
        nbytes = _L().kvq_score_k_workspace_bytes(bits, 1, H)
        ws = _workspace(kmat.device, nbytes, slot="score")
        _lib.check(_L().kvq_decode_prologue(
            bits, _i(kmat, "kcache"), _f(klut, "lookup_table"), _f(klut_off, "lut_off"), kp, _f(lo, "lower"),
            _f(hi, "upper"), _f(koutl, "outliers"), _i(kidx, "outlier_indices"), int(kcol), _i(vmat, "vcache"),
            _f(vlut_rows, "lookup_table"), _f(vlut_sorted, "lut"), vp, _f(voutl, "outliers"),
            _i(vidx, "outlier_indices"), int(vcol), qp, kh, int(thr_k), H, hd, max_len,
            *_mirror(koutl_t, kidx_t, thr_k, max_len), None if klut_ends is None else _f(klut_ends, "lut_ends"),
            None if klut_score is None else _f(klut_score, "lut_score"), _vnorm(vnorm), sk, ws.data_ptr(),
            ws.numel(), _stream()), "kvq_decode_prologue")
    return ws


def score_k_prepared(bits, mat, mul, lut, L, theta, pos_offset, ws, outliers=None, outlier_indices=None,
                     accumulate=False, rope=None):
    """score kernel only (q_len = 1); tables + q were written to `ws` by decode_prologue."""
    H, hd, max_len = _cache_dims(mat, bits)
    n_out = 0 if outliers is None else outliers.shape[1]
    with _Dev(mat):
        _lib.check(_L().kvq_score_k_prepared_rope(
            bits, _i(mat, "mat"), _f(mul, "mul"), _f(lut, "lookup_table"), H, hd, int(L), max_len, float(theta),
            int(pos_offset), None if outliers is None else _f(outliers, "outliers"),
            None if outliers is None else _i(outlier_indices, "outlier_indices"), n_out, 1 if accumulate else 0,
            ws.data_ptr(), ws.numel(), _rope(rope, mat.device), _stream()), "kvq_score_k_prepared_rope")


def score_k_prepared_softmax(bits, mat, mul, lut, L, theta, pos_offset, ws, outliers, outlier_indices, inv_sqrt_hd,
                             n_parts, outliers_t=None, outlier_indices_t=None, f16_pair=False, rope=None):
    """sparse score kernel (tables already in `ws`, accumulate = 0) that also writes the per-(head, tile)
    softmax partials; returns the partials buffer (a workspace: consume it before the next call).
    f16_pair (3 bit, with the mirror): read the fp16 pair-sum tables (include/kvq.h: KVQ_SCORE_F16_PAIR_TABLES)."""
    H, hd, max_len = _cache_dims(mat, bits)
    with _Dev(mat):
        parts = _workspace(mat.device, H * n_parts * 8, slot="softmax")
        _lib.check(_L().kvq_score_k_prepared_softmax_rope(
            bits, _i(mat, "mat"), _f(mul, "mul"), _f(lut, "lookup_table"), H, hd, int(L), max_len, float(theta),
            int(pos_offset), _f(outliers, "outliers"), _i(outlier_indices, "outlier_indices"), outliers.shape[1],
            *_mirror(outliers_t, outlier_indices_t, outliers.shape[1] // 2, max_len),
            ws.data_ptr(), ws.numel(), float(inv_sqrt_hd), parts.data_ptr(), n_parts,
            _lib.SCORE_F16_PAIR_TABLES if f16_pair else 0, _rope(rope, mat.device), _stream()),
            "kvq_score_k_prepared_softmax_rope")
    return parts


def softmax_finish(scores, parts, n_parts, inv_sqrt_hd, sink_scores=None, v_sink=None, sink_out=None):
    """second softmax pass on partials written by score_k_prepared_softmax; scores f32 [H, L].
    v_sink (f16 [H, n_sink, 128]) + sink_out (f32 [1, H, 128]): the sink tokens' share of the attention output is
    written to sink_out by the same launch (mix_v then accumulates onto it)."""
    H, L = scores.shape
    n_sink = 0 if sink_scores is None else sink_scores.shape[1]
    probs = torch.empty_like(scores)
    sink_probs = None if n_sink == 0 else torch.empty_like(sink_scores)
    if v_sink is not None and (n_sink == 0 or sink_out is None or tuple(v_sink.shape) != (H, n_sink, 128)):
        raise ValueError("v_sink needs sink_scores, sink_out and the shape [H, n_sink, 128]")
    with _Dev(scores):
        _lib.check(_L().kvq_softmax_finish(
            _f(scores, "scores"), None if n_sink == 0 else _chk(sink_scores, torch.float16, "sink_scores"),
            parts.data_ptr(), n_parts, _f(probs, "probs"), None if n_sink == 0 else sink_probs.data_ptr(), H, L,
            n_sink, float(inv_sqrt_hd), None if v_sink is None else _chk(v_sink, torch.float16, "v_sink"),
            None if v_sink is None else _f(sink_out, "sink_out"), _stream()), "kvq_softmax_finish")
    return probs, sink_probs


def score_k_softmax(bits, mat, mul, lut, L, theta, pos_offset, ws, outliers, outlier_indices, inv_sqrt_hd,
                    sink_scores=None, outliers_t=None, outlier_indices_t=None, v_sink=None, sink_out=None, rope=None):
    """q.K^T (tables already in `ws`) + softmax: `mul` [1, H, L] receives the raw scores; returns
    (probs f32 [H, L] holding fp16 values, sink_probs f16 [H, n_sink] or None).  Sparse caches take the
    score kernel with the first softmax pass fused in (2 launches), others score_k_prepared +
    softmax_scale (3 launches)."""
    n_parts = _L().kvq_score_k_softmax_parts(bits, int(L), 1 if outliers is not None else 0)
    if n_parts == 0:
        if v_sink is not None:
            raise ValueError("v_sink needs the fused softmax partials (sparse cache)")
        score_k_prepared(bits, mat, mul, lut, L, theta, pos_offset, ws, outliers, outlier_indices, rope=rope)
        return softmax_scale(mul[0], inv_sqrt_hd, sink_scores)
    parts = score_k_prepared_softmax(bits, mat, mul, lut, L, theta, pos_offset, ws, outliers, outlier_indices,
                                     inv_sqrt_hd, n_parts, outliers_t, outlier_indices_t, rope=rope)
    return softmax_finish(mul[0], parts, n_parts, inv_sqrt_hd, sink_scores, v_sink, sink_out)


def score_k_mix_v(bits, kmat, scores, klut, L, theta, pos_offset, ws, koutliers, koutlier_indices, inv_sqrt_hd,
                  vmat, out, vlut_rows, voutliers, voutlier_indices, sink_scores=None, koutliers_t=None,
                  koutlier_indices_t=None, v_sink=None, f16_pair=False, rope=None):
    """q.K^T (tables already in `ws`) -> softmax -> p.V of one decode token in two streaming launches + the slab
    reduce: the score kernel writes raw scores and per-tile softmax partials, the p.V kernel normalises on the way
    (kvq_mix_v_softmax).  scores [1, H, L] scratch, out f32 [1, H, hd].  Returns sink_probs (f16 [H, n_sink]) or None."""
    n_parts = _L().kvq_score_k_softmax_parts(bits, int(L), 1 if koutliers is not None else 0)
    if n_parts == 0 or voutliers is None:
        probs, sink_probs = score_k_softmax(bits, kmat, scores, klut, L, theta, pos_offset, ws, koutliers,
                                            koutlier_indices, inv_sqrt_hd, sink_scores, koutliers_t,
                                            koutlier_indices_t, v_sink, out, rope=rope)
        mix_v(bits, probs.unsqueeze(0), vmat, out, vlut_rows, L, voutliers, voutlier_indices,
              accumulate=v_sink is not None)
        return sink_probs
    parts = score_k_prepared_softmax(bits, kmat, scores, klut, L, theta, pos_offset, ws, koutliers, koutlier_indices,
                                     inv_sqrt_hd, n_parts, koutliers_t, koutlier_indices_t, f16_pair=f16_pair,
                                     rope=rope)
    return mix_v_softmax(bits, scores, parts, n_parts, inv_sqrt_hd, vmat, out, vlut_rows, L, voutliers,
                         voutlier_indices, sink_scores, v_sink)


def mix_v_softmax(bits, scores, parts, n_parts, inv_sqrt_hd, mat, mul, lut_rows, L, outliers, outlier_indices,
                  sink_scores=None, v_sink=None):
    """kvq_mix_v_softmax: raw scores [1, H, L] + the score kernel's softmax partials -> mul f32 [1, H, hd]
    (overwritten; with v_sink f16 [H, n_sink, 128] it includes the sink tokens' share); returns sink_probs
    (f16 [H, n_sink]) or None."""
    H, hd, max_len = _cache_dims(mat, bits)
    n_sink = 0 if sink_scores is None else sink_scores.shape[1]
    sink_probs = None if n_sink == 0 else torch.empty_like(sink_scores)
    with _Dev(mat):
        nbytes = _L().kvq_mix_v_workspace_bytes(bits, 1, H, hd, int(L))
        wsv = _workspace(mat.device, nbytes)
        # room for the probabilities of the library's two-pass route: always handed over, so that the shapes its
        # streaming kernel does not take (unaligned rows or tables, H > 128, more than 2^31 packed words, ...) fall back
        # inside the library whatever its predicate is -- the two checks cannot drift apart (H * L * 4 bytes, cached)
        probs = _workspace(mat.device, H * int(L) * 4, slot="probs")
        _lib.check(_L().kvq_mix_v_softmax(
            bits, _f(scores, "scores"), parts.data_ptr(), n_parts, float(inv_sqrt_hd),
            None if n_sink == 0 else _chk(sink_scores, torch.float16, "sink_scores"),
            None if n_sink == 0 else sink_probs.data_ptr(), n_sink,
            None if v_sink is None else _chk(v_sink, torch.float16, "v_sink"),
            probs.data_ptr(), _i(mat, "mat"), _f(mul, "mul"), _f(lut_rows, "lookup_table"), H, hd, int(L), max_len,
            _fo(outliers, "outliers"), _i(outlier_indices, "outlier_indices"), outlier_indices.shape[1], 0,
            wsv.data_ptr(), wsv.numel(), _stream()), "kvq_mix_v_softmax")
    return sink_probs


# ---- token-sharded single stream ---------------------------------------------------------------------------------
def score_k_tables(bits, q, lut, H, sinks=None):
    """query-premultiplied K tables into the score workspace without an append (kvq_score_k_tables); returns the
    workspace tensor for score_k_prepared[_softmax].  sinks = (k_sink, sink_scores (out), inv_sqrt_hd): the scaled
    scores of the fp16 sink tokens this shard holds are written too."""
    qp, qh = _act(q, "q")
    sk = _sinks(sinks, H)
    with _Dev(lut):
        nbytes = _L().kvq_score_k_workspace_bytes(bits, 1, H)
        ws = _workspace(lut.device, nbytes, slot="score")
        _lib.check(_L().kvq_score_k_tables(bits, qp, qh, _f(lut, "lookup_table"), H, 128, sk, ws.data_ptr(), ws.numel(),
                                           _stream()), "kvq_score_k_tables")
    return ws


def softmax_stats(parts, n_parts, H, stats, sink_scores=None):
    """(max, normaliser) of every head's scaled scores from the score kernel's partials (+ the fp16 sink tokens' scaled
    scores f16 [H, n_sink] of the shard that holds them) -> stats f32 [H, 2]"""
    n_sink = 0 if sink_scores is None else sink_scores.shape[1]
    with _Dev(stats):
        _lib.check(_L().kvq_softmax_stats(parts.data_ptr(), int(n_parts),
                                          None if n_sink == 0 else _chk(sink_scores, torch.float16, "sink_scores"), n_sink,
                                          int(H), _f(stats, "stats"), _stream()),
                   "kvq_softmax_stats")


def combine_shards(packed, n_shards, H, hd, out):
    """exact merge of n_shards records [H*hd out | H x (M, Z)] (f32, contiguous) -> out f32 [1, H, hd]"""
    with _Dev(out):
        _lib.check(_L().kvq_combine_shards(_f(packed, "packed"), int(n_shards), int(H), int(hd), _f(out, "out"), _stream()),
                   "kvq_combine_shards")


def extract_heads(bits, h0, n_heads, src_k, src_v, dst_k, dst_v, src_col, dst_col, n):
    """columns [src_col, src_col + n) of the full-width caches src_k / src_v (QuantK / QuantV) -> columns [dst_col, ...)
    of the head shard dst_k / dst_v that holds heads [h0, h0 + n_heads): packed words, V codebook rows, the shard's share
    of the outlier rows (+ K mirror) -- kvq_extract_heads"""
    H, hd, src_max = _cache_dims(src_k.kcache, bits)
    Hs, _, dst_max = _cache_dims(dst_k.kcache, bits)
    if Hs != n_heads or _cache_dims(dst_v.vcache, bits)[0] != n_heads:
        raise ValueError("extract_heads: the shard caches hold %d heads, not %d" % (Hs, n_heads))
    sparse = src_k.include_sparse
    if sparse and (src_k.outliers is None or dst_k.outliers is None):
        raise NotImplementedError("extract_heads reads the reference outlier format (not compact caches)")
    n_out = int(src_k.num_outliers) if sparse else 0
    if sparse and (dst_k.num_outliers != n_out or dst_v.num_outliers != n_out):
        raise ValueError("extract_heads: the shard's outlier rows must be as wide as the full token's (%d)" % n_out)
    with _Dev(dst_k.kcache):
        _lib.check(_L().kvq_extract_heads(
            bits, H, hd, int(h0), int(n_heads), n_out, _i(src_k.kcache, "src kcache"), _i(src_v.vcache, "src vcache"),
            src_max, int(src_col), _fo(src_k.outliers if sparse else None, "src k outliers"),
            _io(src_k.outlier_indices if sparse else None, "src k outlier_indices"),
            _fo(src_v.outliers if sparse else None, "src v outliers"),
            _io(src_v.outlier_indices if sparse else None, "src v outlier_indices"),
            _f(src_v.lookup_table, "src v lookup_table"), _i(dst_k.kcache, "dst kcache"), _i(dst_v.vcache, "dst vcache"),
            dst_max, int(dst_col), _fo(dst_k.outliers if sparse else None, "dst k outliers"),
            _io(dst_k.outlier_indices if sparse else None, "dst k outlier_indices"),
            _fo(getattr(dst_k, "outliers_t", None) if sparse else None, "dst k outliers_t"),
            _io(getattr(dst_k, "outlier_indices_t", None) if sparse else None, "dst k outlier_indices_t"),
            _fo(dst_v.outliers if sparse else None, "dst v outliers"),
            _io(dst_v.outlier_indices if sparse else None, "dst v outlier_indices"),
            _f(dst_v.lookup_table, "dst v lookup_table"),
            None if src_v.lookup_table2 is None else _f(src_v.lookup_table2, "src v lookup_table2"),
            None if src_v.lookup_table2 is None else _f(dst_v.lookup_table2, "dst v lookup_table2"),
            int(n), _stream()), "kvq_extract_heads")


# ---- one decode token through one layer, one library call -----------------------------------------------------------
def make_layer(kc, vc, table, lut_off):
    """struct kvq_layer for a (QuantK, QuantV) pair: every pointer of the layer's compressed cache, built once and
    cached by the caller (the buffers are preallocated and never move).  Returns (struct, keep-alive tuple)."""
    H, hd, max_len = _cache_dims(kc.kcache, kc.bits)
    thr_k = kc.num_outliers // 2
    if _mirror(kc.outliers_t, kc.outlier_indices_t, thr_k, max_len)[1] is None:
        raise ValueError("decode_step needs the token-contiguous outlier mirror")
    vstruct = _vnorm(vc.vnorm_args())
    mix = vc.mix_table()
    ly = _lib.Layer(
        kc.bits, H, hd, thr_k, max_len, float(kc.rope_theta), int(kc.first_few_fp16),
        _i(kc.kcache, "kcache"), _f(kc.lookup_table, "lookup_table"), _f(lut_off, "lut_off"),
        _f(kc.outlier_threshold_lower, "lower"), _f(kc.outlier_threshold_upper, "upper"), _fo(kc.outliers, "outliers"),
        _io(kc.outlier_indices, "outlier_indices"), _fo(kc.outliers_t, "outliers_t"), _i(kc.outlier_indices_t, "outlier_indices_t"),
        None if kc.lut_ends is None else _f(kc.lut_ends, "lut_ends"), None if table is kc.lookup_table else _f(table, "lut_score"),
        _i(vc.vcache, "vcache"), _f(vc.lookup_table, "lookup_table"), _f(vc.lut, "lut"), _fo(vc.outliers, "outliers"),
        _i(vc.outlier_indices, "outlier_indices"), None if vstruct is None else ctypes.pointer(vstruct),
        None if mix is vc.lookup_table else _f(mix, "lookup_table2"),
        (_lib.LAYER_SCORE_F16_PAIR if (kc.bits == 3 and getattr(kc, "score_f16_pair", False)) else 0) |
        (_lib.LAYER_SCORE_F32_PAIR if (kc.bits == 3 and getattr(kc, "score_f32_pair", False)) else 0))
    return ly, (vstruct, table, lut_off, mix)


def decode_step(layer, col, q, k, v, out, fuse_softmax, sinks=None, v_sink=None, sink_probs=None, rope=None):
    """kvq_decode_step: prologue + q.K^T + softmax + p.V + reduce of one layer from ONE library call.  layer: struct
    from make_layer; col: append column (cached tokens before this one, sink tokens not counted); q [H, 128], k, v
    [C]: all fp16 or all fp32; out f32 [1, H, hd].  sinks = (k_sink, sink_scores (out), inv_sqrt_hd) with v_sink /
    sink_probs, or None."""
    qp, kp, vp, kh = _acts(q, k, v)
    sk = _sinks(sinks, layer.H)
    with _Dev(out):
        nbytes = _L().kvq_decode_step_workspace_bytes(layer.bits, layer.H, layer.hd, int(col) + 1)
        base, usable, ws = _aligned_workspace(out.device, nbytes, "step")
        _lib.check(_L().kvq_decode_step_rope(
            ctypes.byref(layer), int(col), int(col), qp, kp, vp, kh, sk,
            None if v_sink is None else _chk(v_sink, torch.float16, "v_sink"),
            None if sink_probs is None else sink_probs.data_ptr(), _f(out, "out"), int(fuse_softmax),
            base, usable, _rope(rope, out.device), _stream()), "kvq_decode_step_rope")


# ---- prefill attention on the matrix cores ----------------------------------------------------------------------
def prefill_attention(q, k, v, softmax_scale=None):
    """causal attention of a prompt: q fp16 [Hq, S, 128], k, v fp16 [Hkv, S, 128] views (any strides with a contiguous
    last dimension, e.g. transposes of [S, H, 128]); Hq = G * Hkv, 1 <= G <= 8, query head h attends with KV head
    h // G (kvq_prefill_attention for Hq = Hkv, kvq_prefill_attention_gqa otherwise).
    -> fp16 [S, Hq*128] (token-major, ready for o_proj)."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float16 and t.dim() == 3 and t.stride(2) == 1):
            raise ValueError("%s: expected an fp16 GPU tensor [H, S, head_dim] with a contiguous last dimension" % name)
    Hq, S, hd = q.shape
    Hkv = k.shape[0]
    if k.shape != v.shape or k.shape[1:] != q.shape[1:] or Hkv <= 0 or Hq % Hkv or not 1 <= Hq // Hkv <= 8:
        raise ValueError("prefill_attention: q [Hq, S, hd], k / v [Hkv, S, hd] with Hq = G * Hkv, 1 <= G <= 8")
    out = torch.empty((S, Hq, hd), dtype=torch.float16, device=q.device)
    scale = float(softmax_scale) if softmax_scale is not None else 1.0 / (hd ** 0.5)
    strides = (q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), out.stride(1), out.stride(0))
    with _Dev(q):
        if Hq == Hkv:
            _lib.check(_L().kvq_prefill_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), Hq, S, hd,
                                                 *strides, scale, _stream()), "kvq_prefill_attention")
        else:
            _lib.check(_L().kvq_prefill_attention_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), Hq, Hkv,
                                                     S, hd, *strides, scale, _stream()), "kvq_prefill_attention_gqa")
    return out.view(S, Hq * hd)


def head_shard_step(full_layer, shard_layer, h0, col, q, k, v, out, fuse_softmax, sinks=None, v_sink=None, sink_probs=None):
    """kvq_head_shard_step: whole-token append into the staging cache -> extract of the shard's heads -> the shard's
    attention, ONE library call.  q [n_heads, 128] (the shard's heads), k, v [C] (the whole token): all fp16 or all fp32;
    out f32 [1, n_heads, hd]; sinks = (k_sink, sink_scores (out), inv_sqrt_hd) of the shard's heads."""
    qp, kp, vp, kh = _acts(q, k, v)
    sk = _sinks(sinks, shard_layer.H)
    with _Dev(out):
        nbytes = _L().kvq_decode_step_workspace_bytes(shard_layer.bits, shard_layer.H, shard_layer.hd, int(col) + 1)
        base, usable, ws = _aligned_workspace(out.device, nbytes, "step")
        _lib.check(_L().kvq_head_shard_step(
            ctypes.byref(full_layer), ctypes.byref(shard_layer), int(h0), int(col), qp, kp, vp, kh, sk,
            None if v_sink is None else _chk(v_sink, torch.float16, "v_sink"),
            None if sink_probs is None else sink_probs.data_ptr(), _f(out, "out"), int(fuse_softmax), base, usable,
            _stream()), "kvq_head_shard_step")


# ---- grouped-query attention (GQA): Hq query heads over Hkv KV heads, query head h reads KV head h // G -------------
def gqa_supported(Hq, Hkv, hd=128):
    """1 <= G = Hq / Hkv <= 8 (integer), Hkv * hd <= 8192, hd = 128 (include/kvq.h: kvq_gqa_supported)"""
    return bool(_L().kvq_gqa_supported(int(Hq), int(Hkv), int(hd)))


def score_k_gqa(bits, q, mat, mul, lut, L, theta, pos_offset, outliers_t=None, outlier_indices_t=None, inv_sqrt_hd=None,
                parts=None, rope=None):
    """kvq_score_k_gqa: raw scores mul f32 [Hq, L] of q [Hq, 128] (fp32 or fp16) over a cache of Hkv heads; K outliers
    from the token-contiguous mirror [n_out, max_len] (or none).  parts (optional): f32 [Hq, n_parts, 2] that receives
    the first softmax pass (n_parts = score_k_gqa_parts(L))."""
    Hkv, hd, max_len = _cache_dims(mat, bits)
    qp, qh = _act(q, "q")
    Hq = q.shape[0]
    n_out = 0 if outlier_indices_t is None else outlier_indices_t.shape[0]
    with _Dev(mul):
        nbytes = _L().kvq_score_k_gqa_workspace_bytes(bits, Hq, Hkv)
        if nbytes == 0:
            raise ValueError("score_k_gqa: unsupported shape (Hq=%d, Hkv=%d, bits=%d)" % (Hq, Hkv, bits))
        ws = _workspace(mul.device, nbytes, slot="gqa_score")
        _lib.check(_L().kvq_score_k_gqa_rope(
            bits, qp, qh, _i(mat, "mat"), _f(mul, "mul"), _f(lut, "lut"), Hq, Hkv, hd, int(L), max_len, float(theta),
            int(pos_offset), _fo(outliers_t, "outliers_t"), _io(outlier_indices_t, "outlier_indices_t"), n_out,
            float(inv_sqrt_hd if inv_sqrt_hd is not None else 1.0 / hd ** 0.5),
            None if parts is None else _f(parts, "parts"), 0 if parts is None else parts.shape[1],
            ws.data_ptr(), ws.numel(), _rope(rope, mul.device), _stream()), "kvq_score_k_gqa_rope")
    return mul


def score_k_gqa_parts(L):
    return _L().kvq_score_k_gqa_parts(int(L))


def mix_v_gqa(bits, p, mat, mul, lut_rows, L, outliers=None, outlier_indices=None, accumulate=False):
    """kvq_mix_v_gqa: mul f32 [Hq, 128] (+)= p f32 [Hq, L] . Vhat of KV head h // G; V outliers in the reference rows."""
    Hkv, hd, max_len = _cache_dims(mat, bits)
    Hq = p.shape[0]
    n_out = 0 if outlier_indices is None else outlier_indices.shape[1]
    with _Dev(mul):
        nbytes = _L().kvq_mix_v_gqa_workspace_bytes(bits, Hq, Hkv, hd, int(L))
        if nbytes == 0:
            raise ValueError("mix_v_gqa: unsupported shape (Hq=%d, Hkv=%d, bits=%d, L=%d)" % (Hq, Hkv, bits, L))
        ws = _workspace(mul.device, nbytes, slot="gqa_mix")
        _lib.check(_L().kvq_mix_v_gqa(
            bits, _f(p, "p"), _i(mat, "mat"), _f(mul, "mul"), _f(lut_rows, "lut_rows"), Hq, Hkv, hd, int(L), max_len,
            _fo(outliers, "outliers"), _io(outlier_indices, "outlier_indices"), n_out, 1 if accumulate else 0,
            ws.data_ptr(), ws.numel(), _stream()), "kvq_mix_v_gqa")
    return mul


def decode_step_gqa(layer, Hq, col, q, k, v, out, sink_scores=None, v_sink=None, sink_probs=None, rope=None):
    """kvq_decode_step_gqa: append + grouped q.K^T + softmax + grouped p.V of one layer from ONE library call.
    layer: struct from make_layer (layer.H = KV heads); q [Hq, 128], k, v [Hkv*128]: all fp16 or all fp32; out f32
    [1, Hq, hd].  sink_scores: fp16 [Hq, n_sink] already scaled (sink_probs receives their probabilities);
    v_sink: fp16 [Hq, n_sink, 128], then out also holds the sink tokens' share."""
    qp, kp, vp, kh = _acts(q, k, v)
    n_sink = 0 if sink_scores is None else sink_scores.shape[1]
    with _Dev(out):
        nbytes = _L().kvq_decode_step_gqa_workspace_bytes(layer.bits, int(Hq), layer.H, layer.hd, int(col) + 1)
        if nbytes == 0:
            raise ValueError("decode_step_gqa: unsupported shape (Hq=%d, Hkv=%d)" % (Hq, layer.H))
        base, usable, ws = _aligned_workspace(out.device, nbytes, "step")
        _lib.check(_L().kvq_decode_step_gqa_rope(
            ctypes.byref(layer), int(Hq), int(col), qp, kp, vp, kh,
            None if sink_scores is None else _chk(sink_scores, torch.float16, "sink_scores"), n_sink,
            None if v_sink is None else _chk(v_sink, torch.float16, "v_sink"),
            None if sink_probs is None else _chk(sink_probs, torch.float16, "sink_probs"), _f(out, "out"),
            base, usable, _rope(rope, out.device), _stream()), "kvq_decode_step_gqa_rope")


# ---- a chunk of S new tokens over the compressed cache (MFMA flash kernel, kvq_chunk_attn.hip) ---------------------
# (draft trees -- chunk_attention_tree, keep_columns -- at the end of the file)
# Short chunks under grouped-query attention (G >= 2, S <= 32: draft verification) take the grouped kernel
# (kvq_chunk_attention_grouped: a K / V tile is decoded once per KV head instead of once per query head).
# KVQ_CHUNK_GROUPED=0 keeps the per-head kernel for every shape (A/B runs).
CHUNK_GROUPED = os.environ.get("KVQ_CHUNK_GROUPED", "1") != "0"


def chunk_attention_route(Hq, Hkv, S):
    """which kernel chunk_attention runs for S query rows of Hq heads over Hkv KV heads: "grouped"
    (kvq_chunk_attention_grouped) where the library takes the shape and CHUNK_GROUPED is on, else "heads"
    (kvq_chunk_attention)"""
    if CHUNK_GROUPED and _L().kvq_chunk_attention_grouped_workspace_bytes(int(Hq), int(Hkv), int(S), 0) > 0:
        return "grouped"
    return "heads"


def _chunk_args(q, Hq, k_sink, v_sink):
    """the q / sink argument checks of the chunk entries"""
    if not (torch.is_tensor(q) and q.is_cuda and q.dtype == torch.float16 and q.dim() == 3 and q.stride(2) == 1):
        raise ValueError("q: expected an fp16 GPU tensor [Hq, S, 128] with a contiguous last dimension")
    if q.shape[0] != Hq or q.shape[2] != 128:
        raise ValueError("q: expected [%d, S, 128], got %s" % (Hq, tuple(q.shape)))
    if (k_sink is None) != (v_sink is None):
        raise ValueError("k_sink and v_sink come together")


def _chunk_call(what, name, layer, Hq, c0, q, out, k_sink, v_sink, rope, parent=None, window=None):
    """the q / sink checks, output, workspace and call that chunk_attention, chunk_attention_tree and
    chunk_attention_window share: runs the library's <name>_rope (workspace from <name>_workspace_bytes; name None: by
    chunk_attention_route); parent: the tree entry's extra argument; window: the window entries' (whose names carry no
    _rope, whose c0 is n0 and whose workspace function also takes the ring's capacity)"""
    _chunk_args(q, Hq, k_sink, v_sink)
    S = int(q.shape[1])
    extra = ()
    if parent is not None:
        if len(parent) != S:
            raise ValueError("%s: %d rows, parent has %d entries" % (what, S, len(parent)))
        extra = (parent if isinstance(parent, ctypes.Array) else tree_parent_array(parent),)
    n_sink = 0 if k_sink is None else int(k_sink.shape[2])
    if out is None:
        out = torch.empty((S, Hq, 128), dtype=torch.float32, device=q.device)
    with _Dev(out):
        if name is None:
            name = "kvq_chunk_attention_grouped" if chunk_attention_route(Hq, layer.H, S) == "grouped" else "kvq_chunk_attention"
        at = (int(c0),) if window is None else (int(c0), int(window))
        nbytes = getattr(_L(), name + "_workspace_bytes")(int(Hq), layer.H, S, *at,
                                                          *(() if window is None else (int(layer.max_len),)))
        if nbytes == 0:
            raise ValueError("%s: unsupported shape (Hq=%d, Hkv=%d, S=%d, c0=%d%s)" % (
                what, Hq, layer.H, S, c0, "" if window is None else ", window=%d on %d columns" % (window, layer.max_len)))
        base, usable, ws = _aligned_workspace(out.device, nbytes, "chunk")
        fn = name + "_rope" if window is None else name
        _lib.check(getattr(_L(), fn)(
            ctypes.byref(layer), int(Hq), S, *at, q.data_ptr(), q.stride(0), q.stride(1),
            None if k_sink is None else _chk(k_sink, torch.float16, "k_sink"),
            None if v_sink is None else _chk(v_sink, torch.float16, "v_sink"), n_sink, _f(out, "out"),
            base, usable, *extra, _rope(rope, out.device), _stream()), fn)
    return out


def chunk_attention(layer, Hq, c0, q, out=None, k_sink=None, v_sink=None, rope=None):
    """kvq_chunk_attention: query i of q (fp16 [Hq, S, 128] view, contiguous last dimension; RoPE'd at position
    pos_offset + c0 + i) over the fp16 sink tokens and the compressed columns [0, c0 + i] of the layer (struct from
    make_layer, layer.H = KV heads; the chunk must already be packed into columns c0 .. c0+S-1).  k_sink fp16
    [Hkv, 128, n_sink] (post-RoPE) / v_sink fp16 [Hkv, n_sink, 128], or None.  Returns out f32 [S, Hq, 128].
    Shapes chunk_attention_route() sends to "grouped" run kvq_chunk_attention_grouped (same arguments and semantics)."""
    return _chunk_call("chunk_attention", None, layer, Hq, c0, q, out, k_sink, v_sink, rope)


def chunk_attention_window(layer, Hq, n0, window, q, out=None, k_sink=None, v_sink=None, rope=None, grouped=None):
    """kvq_chunk_attention_window[_grouped]: sliding-window attention of a chunk over a RING of C = layer.max_len
    compressed columns (token n in column n mod C; the chunk's tokens n0 .. n0+S-1 already packed).  Query i of q (fp16
    [Hq, S, 128] view, RoPE'd at pos_offset + n0 + i) sees the fp16 sink tokens and the `window` newest tokens up to its
    own, each column rotated at the position of the token it holds.  grouped: True / False picks the geometry, None
    leaves it to chunk_attention_route().  ValueError for what the library's workspace function refuses (window < 1,
    window + S - 1 > C, C % 64 != 0, n0 < 0 and every shape chunk_attention refuses).  Returns out f32 [S, Hq, 128]."""
    if grouped is None:
        grouped = chunk_attention_route(Hq, layer.H, int(q.shape[1]) if torch.is_tensor(q) and q.dim() == 3 else 0) == "grouped"
    name = "kvq_chunk_attention_window_grouped" if grouped else "kvq_chunk_attention_window"
    return _chunk_call("chunk_attention_window", name, layer, Hq, n0, q, out, k_sink, v_sink, rope, window=int(window))


def chunk_attention_window_check(layer, Hq, n0, window, q, k_sink=None, v_sink=None, rope=None, grouped=None):
    """ValueError for every call chunk_attention_window(...) would refuse, without a launch: the argument checks of the
    binding and the host checks of kvq_chunk_attention_window (shape, window, ring, position overflow, q strides and
    alignment, sinks).  For callers that must know before they pack the chunk (cache.chunk_kv).  Returns the geometry
    (`grouped`) the call will run, to be handed on to it."""
    _chunk_args(q, Hq, k_sink, v_sink)
    S = int(q.shape[1])
    for t, name in ((k_sink, "k_sink"), (v_sink, "v_sink")):
        if t is not None:
            _chk(t, torch.float16, name)
    _rope(rope, q.device)
    if grouped is None:
        grouped = chunk_attention_route(Hq, layer.H, S) == "grouped"
    ws = getattr(_L(), "kvq_chunk_attention_window_grouped_workspace_bytes" if grouped else
                 "kvq_chunk_attention_window_workspace_bytes")
    n_sink = 0 if k_sink is None else int(k_sink.shape[2])
    if ws(int(Hq), layer.H, S, int(n0), int(window), int(layer.max_len)) == 0 or \
            layer.pos_offset < 0 or int(n0) + S + layer.pos_offset >= 2 ** 31 or not 0 <= n_sink <= 64 or \
            (q.stride(0) | q.stride(1)) % 8 or q.data_ptr() % 16:
        raise ValueError("chunk_attention_window: unsupported call (Hq=%d, Hkv=%d, S=%d, n0=%d, window=%d on %d columns, "
                         "position offset %d, %d sink tokens, q strides %s)"
                         % (Hq, layer.H, S, n0, window, layer.max_len, layer.pos_offset, n_sink, tuple(q.stride())))
    return grouped


# ---- draft trees: tree mask + per-node positions on the grouped kernel, and the accepted path -------------------------
MAX_TREE = 32       # rows of a tree chunk (the 32-row block of the grouped kernel), root included


def _tree_parents(parent, min_rows, rows):
    """the one validation pass of a parent array: [0, parent[1], ...] as ints, ValueError unless the tree has
    min_rows .. MAX_TREE rows and comes in topological order"""
    S = len(parent)
    if not min_rows <= S <= MAX_TREE:
        raise ValueError("a tree chunk has %d .. %d rows (%s), got %d" % (min_rows, MAX_TREE, rows, S))
    par = [0] * S
    for i in range(1, S):
        par[i] = p = int(parent[i])
        if not 0 <= p < i:
            raise ValueError("parent[%d] = %d: nodes come in topological order (0 <= parent[i] < i)" % (i, p))
    return par


def tree_tables(parent):
    """(depth, anc) of a tree in topological order, as the library derives them from `parent` (parent[0] is ignored,
    parent[i] < i): depth[0] = 0, depth[i] = depth[parent[i]] + 1; anc[i] = the bit set of i and its ancestors.
    ValueError for a parent array that is no such tree or has more than MAX_TREE rows."""
    par = _tree_parents(list(parent), 1, "root included")
    depth, anc = [0] * len(par), [1] + [0] * (len(par) - 1)
    for i in range(1, len(par)):
        depth[i] = depth[par[i]] + 1
        anc[i] = anc[par[i]] | (1 << i)
    return depth, anc


def _host_bytes(values, name, S):
    values = [int(x) for x in values]
    if len(values) != S or any(not 0 <= x <= 255 for x in values):
        raise ValueError("%s: expected %d entries in 0 .. 255" % (name, S))
    return (ctypes.c_uint8 * S)(*values)


def tree_parent_array(parent):
    """the HOST array kvq_chunk_attention_tree takes, from a sequence of S ints (parent[0] is ignored): one pass that
    checks 2 <= S <= MAX_TREE and 0 <= parent[i] < i.  ValueError otherwise."""
    par = _tree_parents(parent, 2, "root + draft nodes")
    return (ctypes.c_uint8 * len(par))(*par)


def chunk_attention_tree(layer, Hq, c0, q, parent, out=None, k_sink=None, v_sink=None, rope=None):
    """kvq_chunk_attention_tree: chunk_attention for a draft TREE.  q fp16 [Hq, S, 128], 2 <= S <= 32 rows in
    topological order (row 0 the root, parent[i] < i the parent row of node i; parent: a host sequence of S ints,
    parent[0] ignored).  Query i (RoPE'd by the caller at position pos_offset + c0 + depth[i]) attends to the sink
    tokens, the compressed columns < c0 and the columns c0 + j of itself and its ancestors; column c0 + j is rotated at
    pos_offset + c0 + depth[j].  The chunk must already be packed into columns c0 .. c0+S-1 in row order.  Every
    1 <= G <= 8 runs the grouped geometry.  parent may be the array tree_parent_array() made of it (checked there).
    Returns out f32 [S, Hq, 128]."""
    return _chunk_call("chunk_attention_tree", "kvq_chunk_attention_tree", layer, Hq, c0, q, out, k_sink, v_sink, rope,
                       parent)


def side_layer(kc=None, vc=None):
    """struct kvq_layer that names the column-owning arrays of ONE side (a QuantK or a QuantV) for keep_columns; the
    other side's pointers are NULL.  Reference outlier format (a compact cache keeps no value arrays: refused by the
    library).  Returns (struct, keep-alive tuple)."""
    c = kc if kc is not None else vc
    mat = kc.kcache if kc is not None else vc.vcache
    H, hd, max_len = _cache_dims(mat, c.bits)
    sparse = bool(c.include_sparse)
    ly = _lib.Layer()
    ly.bits, ly.H, ly.hd, ly.thr_k, ly.max_len = c.bits, H, hd, (c.num_outliers // 2 if sparse else 0), max_len
    vstruct = None
    if kc is not None:
        ly.kmat = _i(kc.kcache, "kcache")
        if sparse:
            ly.koutliers, ly.kidx = _fo(kc.outliers, "outliers"), _io(kc.outlier_indices, "outlier_indices")
            ly.koutliers_t = _fo(kc.outliers_t, "outliers_t")
            ly.kidx_t = _io(kc.outlier_indices_t, "outlier_indices_t")
    else:
        ly.vmat = _i(vc.vcache, "vcache")
        ly.vlut_rows = _f(vc.lookup_table, "lookup_table")
        if sparse:
            ly.voutliers, ly.vidx = _fo(vc.outliers, "outliers"), _io(vc.outlier_indices, "outlier_indices")
        if vc.lookup_table2 is not None:
            vstruct = _lib.VNorm(_f(vc.lookup_table2, "lookup_table2"), 1.0, 0.0, 0, 0)
            ly.vnorm = ctypes.pointer(vstruct)
    return ly, (vstruct,)


def keep_columns(layer, c0, S, keep, device):
    """kvq_keep_columns: of the S newest compressed columns c0 .. c0+S-1 of the layer (struct from make_layer: K and V in
    one launch; or from side_layer) keep the n = len(keep) columns c0 + keep[j] -- they move to c0 + j, the S - n columns
    behind are zero again.  keep: host sequence, strictly ascending, keep[0] == 0, keep[j] < S <= 32.  The caller moves
    klen / vlen back by S - n."""
    keep = [int(x) for x in keep]
    S = int(S)
    if not 1 <= S <= MAX_TREE:
        raise ValueError("keep_columns: 1 <= S <= %d, got %d" % (MAX_TREE, S))
    if not keep or keep[0] != 0:
        raise ValueError("keep_columns: keep[0] must be 0 (the root stays), got %r" % (keep[:1],))
    if any(b <= a for a, b in zip(keep, keep[1:])) or keep[-1] >= S:
        raise ValueError("keep_columns: keep must be strictly ascending with entries < S = %d, got %r" % (S, keep))
    arr = _host_bytes(keep, "keep", len(keep))
    idx = device.index if device.index is not None else torch.cuda.current_device()
    with torch.cuda.device(idx):
        _lib.check(_L().kvq_keep_columns(ctypes.byref(layer), int(c0), S, arr, len(keep), _stream()), "kvq_keep_columns")
