"""The parts of tests/census_check.py that need no GPU: the packer against gqa_check.unpack_codes, the count functions
against a double loop over rows and tokens, and the needle's precondition (softmax mass on the target >= 0.999 within
|q| <= 256) for ideal keys at 300 and 131584 columns."""
import math

import pytest
import torch

from tests import census_check as cen
from tests import gqa_check
from tests import tree_check as tc


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_pack_is_the_inverse_of_unpack(bits):
    g = torch.Generator().manual_seed(bits)
    codes = torch.randint(0, 2 ** bits, (3, 128, 70), generator=g)
    packed = cen.pack_codes(codes, bits)
    assert packed.dtype == torch.int32 and packed.shape == (3, 4 * bits, 70)
    assert torch.equal(gqa_check.unpack_codes(packed, bits), codes)
    # and the other way round on random words: pack(unpack(w)) == w, so no bit of a word is left unset or shared
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, (2, 4 * bits, 33), generator=g, dtype=torch.int64).to(torch.int32)
    assert torch.equal(cen.pack_codes(gqa_check.unpack_codes(words, bits), bits), words)
    # every code value at every position, one at a time
    for i in (0, 10, 21, 31, 127):
        one = torch.zeros(1, 128, 1, dtype=torch.int64)
        one[0, i, 0] = 2 ** bits - 1
        assert torch.equal(gqa_check.unpack_codes(cen.pack_codes(one, bits), bits), one)


def test_values_spell_the_token():
    ids = torch.tensor([0, 1, 7, 11, 77, 103, 104, 4100, 131583, cen.SINK_ID0 + 4])
    base = cen.base_values(ids)
    assert torch.equal(cen.decode_ids(base.double()), ids)
    assert base[:, 24:].sum(1).tolist() == [1] * len(ids)
    assert all(int(base[k, 24 + int(n) % 104]) == 1 for k, n in enumerate(ids))
    for Hkv in (1, 2, 4):
        vals = cen.values(ids, Hkv)
        idx, val = cen.outlier_entries(ids, Hkv)
        assert bool((idx[:, 0] <= idx[:, 1]).all()) and bool(((val == 0) | (val == 2)).all())
        assert bool(((val == 0) == (idx == 0)).all())
        extra = vals - base[None]
        assert bool((extra[:, :, :24] == 0).all())                           # the id channels carry no outlier
        for k, n in enumerate(ids.tolist()):
            n_entries = (n % 7 == 0) + (n % 11 == 0 and Hkv > 1)
            assert int(extra[:, k].sum()) == 2 * n_entries
            if n % 7 == 0:
                assert int(extra[(n // 7) % Hkv, k].sum()) >= 2
            if n % 11 == 0 and Hkv > 1:
                assert int(extra[(n // 11 + 1) % Hkv, k].sum()) >= 2


@pytest.mark.parametrize("sinks", [0, 3])
def test_counts_against_a_double_loop(sinks):
    Hkv = 2
    sv = cen.sink_values(sinks, "cpu") if sinks else None
    vals = cen.values(torch.arange(90), Hkv)
    for c0, S in ((0, 1), (0, 5), (7, 1), (60, 9), (81, 9)):
        got = cen.count_causal(vals, c0, S, sv)
        exp = cen.brute_counts(vals, cen.vis_causal(c0, S, 90).tolist(), sv)
        assert torch.equal(got[0], exp[0]) and torch.equal(got[1], exp[1]), (c0, S)
    # a window of 10 over a ring of 16 columns, two wraps and more (token space: the ring does not show), and the
    # stream's start, where the window is not yet full
    for n0, S in ((0, 4), (5, 7), (12, 7), (30, 7), (33, 1), (50, 6)):
        got = cen.count_window(vals, n0, S, 10, sv)
        exp = cen.brute_counts(vals, cen.vis_window(n0, S, 10, 90).tolist(), sv)
        assert torch.equal(got[0], exp[0]) and torch.equal(got[1], exp[1]), (n0, S)
        assert int(got[1].max()) <= 10 + sinks
    for name, shape in tc.SHAPES.items():
        for c0, S in ((0, 2), (5, 9), (58, 32)):
            parent = shape(S)
            got = cen.count_tree(vals, c0, parent, sv)
            exp = cen.brute_counts(vals, cen.vis_tree(c0, parent, 90).tolist(), sv)
            assert torch.equal(got[0], exp[0]) and torch.equal(got[1], exp[1]), (name, c0, S)


def test_ring_map_against_the_stream():
    """cache.ring_token on a tensor of columns: the token a column holds after N tokens went in one by one"""
    from kvquant_amd.cache import ring_token
    C = 16
    held = [-1] * C
    for n in range(50):
        held[n % C] = n
        res = min(n + 1, C)
        assert ring_token(torch.arange(res), n + 1, C).tolist() == held[:res]


def test_check_resolves_one_column():
    """one column too many or too few, at the longest length of the GPU cases, misses the bar by a factor above 5"""
    n = 131072 + 512
    count = torch.full((1, 1, 128), 3 * 2 ** 17, dtype=torch.int64)
    nv = torch.tensor([n])
    exact = (count.double() / n).float()
    cen.check(exact, count, nv, 1, "exact")
    for off in (-1, 1):
        with pytest.raises(AssertionError):
            cen.check(((count + off).double() / n).float(), count, nv, 1, "one column off")
    assert float(count.max()) * 2.0 ** -22 < 0.19


def test_split_plan_of_the_cases():
    """the nsplit the GPU tests' docstrings state"""
    plan = lambda *a, **k: cen.split_plan(*a, **k)[1:3]
    assert plan(2, 2, 2, 0) == (1, 1) and plan(2, 2, 65, 64) == (1, 3)
    assert plan(2, 1, 600, 4037) == (15, 5)
    assert plan(8, 2, 17, 2049) == (7, 5) and plan(8, 2, 32, 2049, grouped=True) == (7, 5)
    assert plan(8, 2, 33, 2049) == (7, 5)
    assert plan(2, 2, 9, 100, grouped=True) == (1, 2) and plan(8, 1, 32, 4090, grouped=True) == (13, 5)
    assert plan(8, 2, 93, 99, cols=192) == (1, 3) and plan(2, 1, 64, 1216, cols=640) == (2, 5)
    assert plan(8, 2, 512, 131072) == (32, 65) and plan(8, 2, 32, 131072, grouped=True) == (63, 33)


# ---- the needle's precondition for ideal keys ---------------------------------------------------------------------
def _inv(kind):
    if kind == "theta":
        return (10000.0 ** (-torch.arange(64, dtype=torch.float32) / 64)).float()
    from tests import rope_check as rc
    inv, af = rc.spec("llama3").table("cpu")
    return inv.float()


@pytest.mark.parametrize("L", [300, 131584])
@pytest.mark.parametrize("kind", ["theta", "llama3"])
@pytest.mark.parametrize("key", ["equal", "random"])
def test_needle_precondition_for_ideal_keys(L, kind, key):
    """a row that sees all L columns (the most competitors): the gain rule of the GPU fixture puts >= 0.999 of the fp64
    softmax mass on every target with |q| <= 256, the query rounded to fp16 as the fixture rounds it"""
    k = torch.ones(128) if key == "equal" else torch.randn(128, generator=torch.Generator().manual_seed(5)) + 0.5
    keys = cen.ideal_keys(k, _inv(kind), L)                                      # [128, L]
    tgt = torch.tensor(cen.ideal_targets(L))
    vis = torch.ones(len(tgt), L, dtype=torch.bool)
    q, gain = cen.needle_queries(keys[None], tgt, 1, vis, 0)
    assert float(q.abs().max()) <= cen.Q_MAX
    sc = (q[0].double() @ keys) / math.sqrt(128)
    mass = torch.softmax(sc, dim=-1).gather(1, tgt[:, None])
    print("%s %s L=%d: gain %.1f, min mass %.5f, peak score %.0f, |q| <= %.0f"
          % (kind, key, L, gain, float(mass.min()), float(sc.max()), float(q.abs().max())))
    assert float(mass.min()) >= cen.MASS
    assert bool((sc.argmax(dim=-1) == tgt).all())
