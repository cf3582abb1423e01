"""Draft verification on the compressed cache: the grouped short-chunk kernel (kvq_chunk_attention_grouped: G >= 2,
S <= 32, a K / V tile decoded once per KV head) against the fp64 statement of tests/chunk_check.py, its determinism, and
rollback (QuantK / QuantV.truncate) against twin caches that never saw the dropped tokens, bit for bit."""
import pytest
import torch

from tests import chunk_check as cc
from tests import rope_check as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HKV, MAX_LEN = 2, 2048

# (bits, norm, sinks, G, S, L0 = compressed tokens cached before the chunk); every value of the issue's lists occurs:
# L0 = 60 with S = 7 crosses a tile boundary with a ragged last tile, L0 = 1000 is 16 tiles in several splits;
# G = 2 / 4 leave waves without rows, G = 8 keeps all eight busy
CASES = [
    (4, False, 0, 2, 7, 60),
    (4, False, 5, 4, 32, 1000),
    (4, True, 0, 8, 1, 60),
    (3, False, 5, 8, 7, 60),
    (3, True, 0, 4, 2, 1000),
    (2, True, 5, 8, 32, 1000),
    (2, False, 0, 2, 1, 1000),
    (2, False, 5, 4, 2, 60),
]


def _run(bits, norm, sinks, G, S, L0, seed=0):
    from kvquant_amd.cache import chunk_kv
    kc, vc, scale, shift = cc.make_caches(bits, HKV, MAX_LEN, sinks=sinks, norm=norm, device=DEV, seed=seed)
    kp, vp = cc.tokens(L0 + S, HKV, scale, shift, DEV, seed=seed + 11)
    cc.fill(kc, vc, kp[:, :, :L0], vp[:, :, :L0])
    ks, vs = cc.sink_caches(HKV, sinks, DEV, seed + 12) if sinks else (None, None)
    q = cc.queries(HKV * G, S, DEV, seed + 13)
    out = chunk_kv(kc, vc, q, kp[:, :, L0:].contiguous(), vp[:, :, L0:].contiguous(), k_sink=ks, v_sink=vs)
    torch.cuda.synchronize()
    return kc, vc, q, ks, vs, out


def _what(bits, norm, sinks, G, S, L0):
    return "nuq%d%s sinks=%d %d/%d L0=%d S=%d" % (bits, " norm" if norm else "", sinks, HKV * G, HKV, L0, S)


@pytest.mark.parametrize("bits,norm,sinks,G,S,L0", CASES)
def test_grouped_vs_fp64(bits, norm, sinks, G, S, L0):
    from kvquant_amd import ops
    assert ops.chunk_attention_route(HKV * G, HKV, S) == "grouped"
    kc, vc, q, ks, vs, out = _run(bits, norm, sinks, G, S, L0)
    assert out.shape == (S, HKV * G, 128) and torch.isfinite(out).all()
    cc.check(out, cc.reference(kc, vc, q, L0, ks, vs), "grouped " + _what(bits, norm, sinks, G, S, L0))


def test_switch_restores_the_per_head_kernel(monkeypatch):
    """KVQ_CHUNK_GROUPED=0 (the module flag): the same case through kvq_chunk_attention, same bars"""
    from kvquant_amd import ops
    case = CASES[1]
    grouped = _run(*case)[5]
    monkeypatch.setattr(ops, "CHUNK_GROUPED", False)
    assert ops.chunk_attention_route(HKV * case[3], HKV, case[4]) == "heads"
    kc, vc, q, ks, vs, out = _run(*case)
    cc.check(out, cc.reference(kc, vc, q, case[5], ks, vs), "heads " + _what(*case))
    d = float((out - grouped).abs().max() / out.abs().max())
    print("grouped vs per-head kernel: max |delta| %.2e of the largest output" % d)


def test_route():
    from kvquant_amd import ops
    assert ops.chunk_attention_route(32, 8, 32) == "grouped"
    assert ops.chunk_attention_route(32, 8, 33) == "heads"       # S > 32
    assert ops.chunk_attention_route(8, 8, 8) == "heads"         # MHA
    assert ops.chunk_attention_route(72, 8, 8) == "heads"        # (a shape neither kernel takes)


def test_grouped_scaled_rope_vs_fp64():
    """llama3 frequencies (kvquant_amd.rope) through the _rope twin against tests/rope_check.py's statement"""
    from kvquant_amd import ops
    from kvquant_amd.cache import chunk_kv
    bits, G, L0, S = 4, 4, 1000, 7
    kc, vc, k, v, ks, vs = rc.make(bits, HKV, L0, S, "llama3", device=DEV)
    assert ops.chunk_attention_route(HKV * G, HKV, S) == "grouped"
    q = cc.queries(HKV * G, S, DEV, 13)
    inv, af = kc.rope_table(L0 + S)
    out = chunk_kv(kc, vc, q, k, v)
    torch.cuda.synchronize()
    cc.check(out, rc.chunk_reference(kc, vc, q, L0, inv, af), "grouped llama3 " + _what(bits, False, 0, G, S, L0))
    # (the table matters: the theta rule's statement is far from this output)
    assert float((out.double() - cc.reference(kc, vc, q, L0)).abs().max()) > 1e-3 * float(out.abs().max())


def test_grouped_deterministic():
    a = _run(*CASES[1])[5]
    b = _run(*CASES[1])[5]
    assert torch.equal(a, b)


# ---- rollback ---------------------------------------------------------------------------------------------------------
K_ARRAYS = ("kcache", "outliers", "outlier_indices", "outliers_t", "outlier_indices_t")
V_ARRAYS = ("vcache", "lookup_table", "lookup_table2", "outliers", "outlier_indices")


def _assert_same_state(a, b):
    (ka, va), (kb, vb) = a, b
    assert ka.klen == kb.klen and va.vlen == vb.vlen and ka.klen == va.vlen
    for c1, c2, names in ((ka, kb, K_ARRAYS), (va, vb, V_ARRAYS)):
        for name in names:
            t1, t2 = getattr(c1, name), getattr(c2, name)
            assert (t1 is None) == (t2 is None), name
            if t1 is not None:
                assert torch.equal(t1, t2), name


@pytest.mark.parametrize("sinks", [0, 5])
def test_rollback_exact(sinks):
    """A: 8 draft tokens, 5 rejected, 6 others; B: the 3 kept tokens, the same 6 -- same caches, same last output"""
    from kvquant_amd.cache import chunk_kv
    L0, G, bits = 1000, 4, 2                      # (2 bit + Q-Norm: lookup_table2 is live in both caches)
    ks, vs = cc.sink_caches(HKV, sinks, DEV, 12) if sinks else (None, None)
    q8, q6 = cc.queries(HKV * G, 8, DEV, 13), cc.queries(HKV * G, 6, DEV, 14)
    twins, outs = [], []
    for first in (8, 3):
        kc, vc, scale, shift = cc.make_caches(bits, HKV, MAX_LEN, sinks=sinks, norm=True, device=DEV)
        kp, vp = cc.tokens(L0 + 14, HKV, scale, shift, DEV, seed=11)
        cc.fill(kc, vc, kp[:, :, :L0], vp[:, :, :L0])
        chunk_kv(kc, vc, q8[:, :first], kp[:, :, L0:L0 + first].contiguous(), vp[:, :, L0:L0 + first].contiguous(),
                 k_sink=ks, v_sink=vs)
        if first == 8:
            kc.truncate(5)
            vc.truncate(5)
        assert kc.klen == vc.vlen == sinks + L0 + 3
        outs.append(chunk_kv(kc, vc, q6, kp[:, :, L0 + 8:].contiguous(), vp[:, :, L0 + 8:].contiguous(),
                             k_sink=ks, v_sink=vs))
        twins.append((kc, vc))
    torch.cuda.synchronize()
    _assert_same_state(*twins)
    assert twins[0][0].klen == sinks + L0 + 9
    assert torch.equal(outs[0], outs[1])
    # everything behind the caches' length is as reset() leaves it
    kc, vc = twins[0]
    n = L0 + 9
    assert not kc.kcache[:, :, n:].any() and not kc.outliers_t[:, n:].any() and not kc.outlier_indices[n:].any()
    assert not vc.vcache[:, :, n:].any() and not vc.lookup_table[n:].any() and not vc.lookup_table2[n:].any()


def test_rollback_exact_compact():
    """compact=True caches (chunk_kv refuses them): decode_kv appends, states only"""
    from kvquant_amd.cache import QuantK, QuantV, decode_kv
    from tests import decode_check
    L0, bits, C = 1000, 4, HKV * 128
    quant, scale, shift = decode_check.quantizer(bits, seed=bits, C=C)
    q = cc.queries(HKV, 14, DEV, 13)
    twins = []
    for first in (8, 3):
        kw = dict(bits=bits, hidden_size=C, num_heads=HKV, max_position_embeddings=MAX_LEN, include_sparse=True,
                  sparsity_threshold=0.99, device=DEV, compact=True)
        kc, vc = QuantK(rope_theta=10000.0, **kw), QuantV(**kw)
        kc.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99)
        vc.load_lookup_table(quant, include_sparse=True, sparsity_threshold=0.99)
        kp, vp = cc.tokens(L0 + 14, HKV, scale.to(DEV), shift.to(DEV), DEV, seed=11)
        cc.fill(kc, vc, kp[:, :, :L0], vp[:, :, :L0])
        fed = list(range(first)) + list(range(8, 14))
        for n, i in enumerate(fed):
            if n == first and first == 8:
                kc.truncate(5)
                vc.truncate(5)
            decode_kv(kc, vc, q[:, i].contiguous(), kp[:, :, L0 + i].reshape(-1).contiguous(),
                      vp[:, :, L0 + i].reshape(-1).contiguous())
        twins.append((kc, vc))
    torch.cuda.synchronize()
    assert twins[0][0].outliers is None and twins[0][0].klen == L0 + 9
    _assert_same_state(*twins)


def test_truncate_error_paths():
    from kvquant_amd.cache import QuantK
    kc, vc, scale, shift = cc.make_caches(4, HKV, 256, sinks=5, device=DEV)
    kp, vp = cc.tokens(3, HKV, scale, shift, DEV, seed=11)
    cc.fill(kc, vc, kp, vp)
    for c in (kc, vc):
        with pytest.raises(ValueError):
            c.truncate(4)                          # into the 5 sink tokens
    kc, vc, scale, shift = cc.make_caches(4, HKV, 256, device=DEV)
    cc.fill(kc, vc, kp, vp)
    for c in (kc, vc):
        with pytest.raises(ValueError):
            c.truncate(4)                          # past zero
    assert kc.klen == vc.vlen == 3
    ko = QuantK(bits=4, hidden_size=HKV * 128, num_heads=HKV, max_position_embeddings=256, include_sparse=True,
                use_orig_sparse=True, device=DEV)
    ko.klen = 4
    with pytest.raises(NotImplementedError):
        ko.truncate(1)
