"""Grouped-query attention, host side (no GPU): the ABI 403 entry points exist and refuse every unsupported shape,
pointer and workspace before any launch, and the head-count rules patch_llama / KVQuantAttention apply."""
import ctypes
import types

import pytest

from kvquant_amd import _lib

EINVAL, EWORKSPACE = -1, -3
P = 4096            # a fake device pointer: every refused call returns before anything is dereferenced
NEW = ["kvq_gqa_supported", "kvq_score_k_gqa_workspace_bytes", "kvq_score_k_gqa_parts", "kvq_score_k_gqa",
       "kvq_mix_v_gqa_workspace_bytes", "kvq_mix_v_gqa", "kvq_decode_step_gqa_workspace_bytes", "kvq_decode_step_gqa",
       "kvq_prefill_attention_gqa"]


def test_exported_and_version():
    lib = _lib.lib()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.kvq_version() == 403


# (Hq, Hkv, hd): indivisible, G > 8, hd != 128, Hkv * 128 > 8192
BAD = [(12, 8, 128), (72, 8, 128), (32, 8, 64), (130, 65, 128), (0, 8, 128)]


@pytest.mark.parametrize("Hq,Hkv,hd", BAD)
def test_score_gqa_einval(Hq, Hkv, hd):
    lib = _lib.lib()
    assert lib.kvq_gqa_supported(Hq, Hkv, hd) == 0
    assert lib.kvq_score_k_gqa_workspace_bytes(4, Hq, Hkv) == 0 or hd != 128
    rc = lib.kvq_score_k_gqa(4, P, 0, P, P, P, Hq, Hkv, hd, 100, 128, 10000.0, 0, P, P, 12, 0.088, None, 0, P, 1 << 30,
                             None)
    assert rc == EINVAL


@pytest.mark.parametrize("Hq,Hkv,hd", BAD)
def test_mix_gqa_einval(Hq, Hkv, hd):
    lib = _lib.lib()
    assert lib.kvq_mix_v_gqa_workspace_bytes(4, Hq, Hkv, hd, 100) == 0
    rc = lib.kvq_mix_v_gqa(4, P, P, P, P, Hq, Hkv, hd, 100, 128, P, P, 12, 0, P, 1 << 30, None)
    assert rc == EINVAL


@pytest.mark.parametrize("Hq,Hkv,hd", [b for b in BAD if b != (130, 65, 128)])   # (prefill: no cache-width limit)
def test_prefill_gqa_einval(Hq, Hkv, hd):
    lib = _lib.lib()
    rc = lib.kvq_prefill_attention_gqa(P, P, P, P, Hq, Hkv, 64, hd, 8192, 128, 8192, 128, 8192, 128, 128, 128 * Hq,
                                       0.088, None)
    assert rc == EINVAL


def _layer(Hkv, bits=4, thr_k=6, max_len=128):
    ly = _lib.Layer()
    ly.bits, ly.H, ly.hd, ly.thr_k, ly.max_len, ly.rope_theta = bits, Hkv, 128, thr_k, max_len, 10000.0
    for f in ("kmat", "klut", "klut_off", "klo", "khi", "koutliers", "kidx", "koutliers_t", "kidx_t", "vmat",
              "vlut_rows", "vlut_sorted", "voutliers", "vidx"):
        setattr(ly, f, P)
    return ly


@pytest.mark.parametrize("Hq,Hkv,hd", BAD)
def test_step_gqa_einval(Hq, Hkv, hd):
    lib = _lib.lib()
    ly = _layer(Hkv)
    ly.hd = hd
    assert lib.kvq_decode_step_gqa_workspace_bytes(4, Hq, Hkv, hd, 100) == 0
    rc = lib.kvq_decode_step_gqa(ctypes.byref(ly), Hq, 99, P, P, P, 1, None, 0, None, None, P, P, 1 << 40, None)
    assert rc == EINVAL


def test_null_pointers_einval():
    lib = _lib.lib()
    assert lib.kvq_score_k_gqa(4, None, 0, P, P, P, 32, 8, 128, 100, 128, 1e4, 0, P, P, 12, 0.088, None, 0, P, 1 << 30,
                               None) == EINVAL
    assert lib.kvq_score_k_gqa(4, P, 0, P, P, P, 32, 8, 128, 100, 128, 1e4, 0, None, P, 12, 0.088, None, 0, P, 1 << 30,
                               None) == EINVAL    # (index array without values: the compact format)
    assert lib.kvq_mix_v_gqa(4, None, P, P, P, 32, 8, 128, 100, 128, P, P, 12, 0, P, 1 << 30, None) == EINVAL
    assert lib.kvq_prefill_attention_gqa(None, P, P, P, 32, 8, 64, 128, 8192, 128, 2048, 128, 2048, 128, 128, 4096,
                                         0.088, None) == EINVAL
    assert lib.kvq_decode_step_gqa(None, 32, 99, P, P, P, 1, None, 0, None, None, P, P, 1 << 40, None) == EINVAL
    for f in ("koutliers_t", "kidx_t", "voutliers", "vidx", "kmat"):
        ly = _layer(8)
        setattr(ly, f, None)
        assert lib.kvq_decode_step_gqa(ctypes.byref(ly), 32, 99, P, P, P, 1, None, 0, None, None, P, P, 1 << 40,
                                       None) == EINVAL, f
    ly = _layer(8)
    assert lib.kvq_decode_step_gqa(ctypes.byref(ly), 32, 99, None, P, P, 1, None, 0, None, None, P, P, 1 << 40,
                                   None) == EINVAL
    assert lib.kvq_decode_step_gqa(ctypes.byref(ly), 32, 128, P, P, P, 1, None, 0, None, None, P, P, 1 << 40,
                                   None) == EINVAL   # column beyond max_len


def test_short_workspace():
    lib = _lib.lib()
    need = lib.kvq_score_k_gqa_workspace_bytes(4, 32, 8)
    assert need > 0
    assert lib.kvq_score_k_gqa(4, P, 0, P, P, P, 32, 8, 128, 100, 128, 1e4, 0, P, P, 12, 0.088, None, 0, P, need - 1,
                               None) == EWORKSPACE
    need = lib.kvq_mix_v_gqa_workspace_bytes(4, 32, 8, 128, 100000)
    assert need > 16
    assert lib.kvq_mix_v_gqa(4, P, P, P, P, 32, 8, 128, 100000, 100000, P, P, 12, 0, P, need - 1, None) == EWORKSPACE
    ly = _layer(8, max_len=4096)
    need = lib.kvq_decode_step_gqa_workspace_bytes(4, 32, 8, 128, 4000)
    assert need > 0
    assert lib.kvq_decode_step_gqa(ctypes.byref(ly), 32, 3999, P, P, P, 1, None, 0, None, None, P, 4096, need - 1,
                                   None) == EWORKSPACE
    assert lib.kvq_decode_step_gqa(ctypes.byref(ly), 32, 3999, P, P, P, 1, None, 0, None, None, P, 4096 + 16, need,
                                   None) == EWORKSPACE   # (not 256-byte aligned)


def _cfg(heads, kv_heads):
    return types.SimpleNamespace(num_attention_heads=heads, num_key_value_heads=kv_heads)


def test_head_count_rules():
    from kvquant_amd.attention import gqa_groups
    from kvquant_amd.llama import kv_heads_of
    assert kv_heads_of(_cfg(8, 2)) == 2
    assert kv_heads_of(_cfg(32, 8)) == 8
    assert kv_heads_of(_cfg(28, 4)) == 4           # G = 7 (Qwen2.5-7B)
    assert kv_heads_of(_cfg(32, 32)) == 32
    assert kv_heads_of(_cfg(32, None)) == 32
    assert gqa_groups(8, 2) == 4 and gqa_groups(8, None) == 1
    with pytest.raises(ValueError):
        kv_heads_of(_cfg(8, 3))
    with pytest.raises(ValueError):
        kv_heads_of(_cfg(32, 2))                   # G = 16
