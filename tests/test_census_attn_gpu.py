"""The census (tests/census_check.py): WHICH columns a row of the matrix-core attention kernels sees, exactly, at any
length.  Every query is zero and every dequantised value a small integer that spells its token, so every score is 0,
every visible key weighs exactly 1, every partial sum is an integer below 2^24 and out * n_vis equals the sum of the
visible tokens' values up to the one rounding of the final division: |out * n_vis - count| <= max(count, 1) * 2^-22 for
EVERY row, head and channel, which resolves a single column wrongly masked or wrongly seen among 131584 (one column
moves a count by 1; the bar stays below 0.19).  The census proves nothing about K: a zero query makes the keys, their
outliers and their rotation irrelevant (tests/test_needle_attn_gpu.py is about those).

The chunk entries divide o / l (one IEEE division); the prefill kernel multiplies by 1 / l and writes fp16, hence its
own bar |out * n - count| <= count * 2^-10 + 2^-20 on the residue channels 24 .. 127, whose counts stay <= 6 at 600
rows (every asserted count is at most 128, so the bar is below 0.13)."""
import pytest
import torch

from tests import census_check as cen
from tests import tree_check as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS, GROUPED = "kvq_chunk_attention", "kvq_chunk_attention_grouped"

_fixtures = {}


@pytest.fixture(scope="module", autouse=True)
def _free_the_fixtures():
    """the caches (the 128K one among them) go back when the module is done"""
    yield
    _fixtures.clear()
    torch.cuda.empty_cache()


def _linear(bits, Hkv, L, sinks=0, norm=False):
    key = ("linear", bits, Hkv, L, sinks, norm)
    if key not in _fixtures:
        _fixtures[key] = cen.Linear(bits, Hkv, L, sinks=sinks, norm=norm, device=DEV, seed=3)
    return _fixtures[key]


def _zero_q(Hq, S):
    return torch.zeros(Hq, S, 128, dtype=torch.float16, device=DEV)


def _plain(fx, name, G, c0, S):
    """one chunk (c0, S) of the fixture through the named entry, every value asserted"""
    from kvquant_amd import ops
    Hq = fx.Hkv * G
    grouped = name == GROUPED
    nqb, nsplit, tps, nbytes = cen.split_plan(Hq, fx.Hkv, S, c0, grouped)
    assert getattr(ops._L(), name + "_workspace_bytes")(Hq, fx.Hkv, S, c0) == nbytes     # (the plan of the docstrings)
    out = ops._chunk_call("chunk_attention", name, fx.layer(), Hq, c0, _zero_q(Hq, S), None, fx.ks, fx.vs, None)
    count, n_vis = cen.count_causal(fx.vals, c0, S, fx.sink_vals)
    cen.check(out, count, n_vis, G, "%s nuq%d %d/%d sinks=%d c0=%d S=%d (%d splits of %d tiles)"
              % (name[4:], fx.bits, Hq, fx.Hkv, fx.sinks, c0, S, nsplit, tps))


# ---- per-head, grouped ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c0,S", [(0, 2), (0, 1), (1, 2), (1, 1)])
def test_census_empty_cache_and_single_tile(c0, S):
    """nuq4, 2 x 1, no sinks: an empty cache, one ragged tile, S = 1.  nsplit = 1."""
    _plain(_linear(4, 2, 192), HEADS, 1, c0, S)


@pytest.mark.parametrize("c0", [59, 63, 64])
@pytest.mark.parametrize("S", [5, 1, 65])
def test_census_tile_edges_with_sinks(c0, S):
    """nuq4, 2 x 1, 5 sinks (their tile rides in split 0): the chunk ends on the last column of a tile (59 + 5, 63 + 1),
    straddles a tile edge (59 / 63 + 65, 63 + 5) or starts on one (64).  nsplit = 1 (1 .. 3 tiles)."""
    _plain(_linear(4, 2, 192, sinks=5), HEADS, 1, c0, S)


def test_census_three_row_blocks():
    """nuq3, 1 x 2, 5 sinks, 4037 columns + 600 rows: three 256-row blocks whose column ranges end at 4293, 4549 and
    4637 (68, 72 and 73 tiles); 15 splits of 5 tiles, so split 14 (tiles 70 ..) is EMPTY for the first block -- the
    (-inf, 0) partial and the merge's skip -- and split 13 holds only three of its tiles."""
    fx = _linear(3, 1, 4037 + 600, sinks=5)
    assert cen.split_plan(2, 1, 600, 4037)[:3] == (3, 15, 5)
    _plain(fx, HEADS, 2, 4037, 600)


@pytest.mark.parametrize("name,S", [(HEADS, 17), (HEADS, 32), (HEADS, 33), (GROUPED, 17), (GROUPED, 32)])
def test_census_grouped_route_2bit_norm(name, S):
    """nuq2 with Q-Norm (p.V dequantises with lookup_table2; lookup_table holds 9.0), 2 x 4, 2049 columns: the grouped
    geometry up to its boundary of 32 rows (rows >= S are clamped duplicates), the per-head one on both sides of it.
    33 tiles, 7 splits of 5 tiles for every S here."""
    fx = _linear(2, 2, 2049 + 33, norm=True)
    assert fx.vc.mix_table() is fx.vc.lookup_table2
    assert cen.split_plan(8, 2, S, 2049, name == GROUPED)[1:3] == (7, 5)
    _plain(fx, name, 4, 2049, S)


@pytest.mark.parametrize("name,S", [(HEADS, 512), (GROUPED, 32)])
def test_census_128k(name, S):
    """nuq4, 2 x 4, 131072 columns.  Per-head, S = 512: two row blocks, 32 splits of 65 tiles (2056 and 2052 tiles).
    Grouped, S = 32: the 64-split cap -- 2049 tiles in 63 splits of 33."""
    fx = _linear(4, 2, 131072 + 512)
    assert cen.split_plan(8, 2, S, 131072, name == GROUPED)[1:3] == ((32, 65) if name == HEADS else (63, 33))
    _plain(fx, name, 4, 131072, S)


# ---- trees -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hkv,G", [(2, 1), (1, 8)])
@pytest.mark.parametrize("sinks", [0, 5])
def test_census_trees(Hkv, G, sinks):
    """nuq4, every shape of tree_check.SHAPES at S = 9 and 32, behind 100 columns (the chunk inside tile 1, or across
    the edge at 128: nsplit = 1) and behind 4090 (across the edge at 4096; 65 tiles, 13 splits of 5)."""
    from kvquant_amd import ops
    fx = _linear(4, Hkv, 4090 + 32, sinks=sinks)
    Hq = Hkv * G
    for c0, nsplit in ((100, 1), (4090, 13)):
        for S in (9, 32):
            assert cen.split_plan(Hq, Hkv, S, c0, True)[1] == nsplit
            assert ops._L().kvq_chunk_attention_tree_workspace_bytes(Hq, Hkv, S, c0) == cen.split_plan(Hq, Hkv, S, c0, True)[3]
            for name, shape in tc.SHAPES.items():
                parent = shape(S)
                out = ops.chunk_attention_tree(fx.layer(), Hq, c0, _zero_q(Hq, S), parent, k_sink=fx.ks, v_sink=fx.vs)
                count, n_vis = cen.count_tree(fx.vals, c0, parent, fx.sink_vals)
                cen.check(out, count, n_vis, G, "tree %s %d/%d sinks=%d c0=%d S=%d" % (name, Hq, Hkv, sinks, c0, S))


# ---- rings -------------------------------------------------------------------------------------------------------------
def _ring_case(fx, G, N, S, grouped):
    from kvquant_amd import ops
    Hq = fx.Hkv * G
    n0 = N - S
    fx.at(N)
    name = "kvq_chunk_attention_window" + ("_grouped" if grouped else "")
    plan = cen.split_plan(Hq, fx.Hkv, S, n0, grouped, cols=min(N, fx.C))
    assert getattr(ops._L(), name + "_workspace_bytes")(Hq, fx.Hkv, S, n0, fx.W, fx.C) == plan[3]
    out = ops.chunk_attention_window(fx.layer(), Hq, n0, fx.W, _zero_q(Hq, S), k_sink=fx.ks, v_sink=fx.vs, grouped=grouped)
    count, n_vis = cen.count_window(fx.vals, n0, S, fx.W, fx.sink_vals)
    cen.check(out, count, n_vis, G, "window nuq%d %d/%d sinks=%d C=%d W=%d N=%d S=%d %s"
              % (fx.bits, Hq, fx.Hkv, fx.sinks, fx.C, fx.W, N, S, "grouped" if grouped else "heads"))
    return plan


@pytest.mark.parametrize("bits", [4, 2])
@pytest.mark.parametrize("sinks", [0, 5])
def test_census_ring_two_wraps(bits, sinks):
    """2 x 4, ring C = 192, W = 100, both geometries (grouped up to 32 rows), at N = 192 (full, not wrapped), 228 and 450
    (two wraps) with S = 1, 17, 93 (= C - W + 1, the longest chunk): tiles masked whole, the tile that holds the
    newest column, the window's oldest token on the far side of it.  3 tiles: nsplit = 1."""
    fx = cen.Ring(bits, 2, 192, 100, sinks=sinks, device=DEV, seed=4)
    for N in (192, 228, 450):
        for S in (1, 17, 93):
            for grouped in ((False, True) if S <= 32 else (False,)):
                assert _ring_case(fx, 4, N, S, grouped)[1] == 1


@pytest.mark.parametrize("sinks", [0, 5])
def test_census_ring_masked_split(sinks):
    """nuq4, 1 x 2, ring C = 640 (10 tiles, 2 splits of 5), W = 300 at N = 1280: for S = 1 everything visible lies in
    split 1 and split 0 writes the (-inf, 0) partial (with sinks: the sink tokens' alone); S = 64 reaches back."""
    fx = cen.Ring(4, 1, 640, 300, sinks=sinks, device=DEV, seed=5)
    for S in (1, 64):
        for grouped in ((False, True) if S <= 32 else (False,)):
            assert _ring_case(fx, 2, 1280, S, grouped)[1:3] == (2, 5)


# ---- prefill -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,Hq,Hkv", [(1, 2, 2), (31, 3, 3), (33, 8, 2), (64, 2, 2), (65, 8, 2), (257, 4, 4), (600, 8, 2)])
def test_census_prefill(S, Hq, Hkv):
    """q = 0, random finite K, v in {0, 1} by the token rule; out = fp16(count / n).  Only the residue channels are
    asserted: their counts are at most ceil(600 / 104) = 6 <= 128, so count * 2^-10 + 2^-20 < 0.13 resolves one key."""
    from kvquant_amd import ops
    g = torch.Generator(device=DEV).manual_seed(S)
    k = (torch.randn(Hkv, S, 128, generator=g, device=DEV) * 2).half()
    vals = cen.base_values(torch.arange(S, device=DEV))[None].repeat(Hkv, 1, 1)
    out = ops.prefill_attention(_zero_q(Hq, S), k, vals.half().contiguous()).view(S, Hq, 128)
    count, n_vis = cen.count_causal(vals, 0, S)
    ch = slice(cen.ID_BITS, 128)
    assert int(count[..., ch].max()) <= 128
    cen.check(out, count, n_vis, Hq // Hkv, "prefill S=%d %d/%d" % (S, Hq, Hkv), channels=ch, bar=cen.prefill_bar)
