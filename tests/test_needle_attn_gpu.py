"""The needle (tests/census_check.py): at WHICH POSITION a column of the compressed cache is rotated.  The K cache holds
the same pre-RoPE token in every column (through parallel_pack: the real quantiser, the real outlier path), so a
column's rotated key depends on its position alone; V is the census, whose channels 0 .. 23 spell the token.  The query
of a row is gain x the dequantised key rotated at the position the STATEMENT gives a target token (sinks + token; a tree
node: sinks + c0 + depth), so the scores are the key's rotary autocorrelation and peak at the column that sits at that
position.  Asserted: the id spelled by out[row, h, 0:24] is the target's (a column rotated one position off, read from
the wrong ring slot, masked or -- a tree's sibling, same position, same key -- wrongly visible decodes another id or a
mixture), and chunk_check.check against the fp64 statement.

Precondition, asserted BEFORE the kernel's result is looked at and blamed on the fixture: the fp64 statement puts at
least 0.999 of the softmax mass on the target for every (row, target) pair, with |q| <= 256 (the gain is found per pair
by census_check.find_gains).  The needle proves nothing about accuracy under a diffuse softmax; the neighbouring tests
are about that.

Targets: the handful rows (first, last, middle, both sides of the 32- and 256-row block edges) take their first and
last visible column, their own column, c0 - 1 and c0, the first and last sink, on a ring the window's oldest token and
the columns around the newest one, in a tree the root and the parent; the columns on both sides of every tile edge and
split edge go to rows that see them (census_check.schedule).  A deliberate limit: a case of more than 80 tiles (the
128K one, 2048 tile edges for 32 rows) takes both sides of every SPLIT edge but of its tile edges only the first, the
last, those around c0 and one in the middle of every split (census_check.boundary_columns).  Every case runs with the
theta rule and with llama3 frequencies."""
import pytest
import torch

from tests import census_check as cen
from tests import chunk_check as cc
from tests import rope_check as rc
from tests import tree_check as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS, GROUPED = "kvq_chunk_attention", "kvq_chunk_attention_grouped"
ROPES = ["theta", "llama3"]

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _free_the_fixtures():
    """the caches and their fp64 dequantisations (0.5 GB per rope at 128K) go back when the module is done"""
    yield
    _cache.clear()
    torch.cuda.empty_cache()


def _linear(bits, Hkv, L, sinks, seed=3):
    key = (bits, Hkv, L, sinks, seed)
    if key not in _cache:
        _cache[key] = cen.Linear(bits, Hkv, L, sinks=sinks, same_key=True, device=DEV, seed=seed)
    return _cache[key]


def _table(rope):
    """the (inv_freq, attention factor) the entries take, None for the theta rule"""
    return None if rope == "theta" else rc.spec("llama3").table(DEV, 1 << 18)


def _dequant(fx, rope):
    """(keys rotated at sinks + column, Vhat, inv_freq) over all of the fixture's columns, once per fixture and rope"""
    key = (id(fx), rope)
    if key not in _cache:
        _cache[key] = cen.rotated(fx, fx.L, _table(rope))
    return _cache[key]


def _needle(what, G, keys, vals, vis, n_sink, personal, shared, run):
    """every launch of the schedule: precondition, decoded ids, chunk_check.check"""
    S = vis.shape[0]
    vis_key = torch.cat((torch.ones(S, n_sink, dtype=torch.bool, device=vis.device), vis), dim=1)
    targets = cen.schedule(personal, shared, vis_key, S).to(DEV)
    for r in range(targets.shape[0]):
        q, gain = cen.needle_queries(keys, targets[r], G, vis, n_sink)
        ref, p = cen.statement(q, keys, vals, vis, n_sink)
        mass = p.gather(2, targets[r][:, None, None].expand(S, p.shape[1], 1))
        assert float(q.abs().max()) <= cen.Q_MAX and float(mass.min()) >= cen.MASS, \
            "needle FIXTURE %s launch %d: the statement's mass on a target is %.5f" % (what, r, float(mass.min()))
        out = run(q)
        assert torch.isfinite(out).all()
        got, exp = cen.decode_ids(out), cen.expected_ids(targets[r], n_sink)[:, None].expand(S, out.shape[1])
        if not torch.equal(got, exp):
            i, h = [int(x) for x in (got != exp).nonzero()[0]]
            raise AssertionError("%s launch %d: row %d head %d attends to id %d, its target is id %d (ids from 2^20: sink "
                                 "tokens; gain %.1f, statement mass %.5f); %d of %d (row, head) pairs off"
                                 % (what, r, i, h, int(got[i, h]), int(exp[i, h]), gain, float(mass[i, h]),
                                    int((got != exp).sum()), got.numel()))
        cc.check(out, ref, "needle %s launch %d (gain <= %.1f, mass >= %.5f)" % (what, r, gain, float(mass.min())))
    return targets.shape[0]


def _personal(S, n_sink, vis, own, extra=lambda i: []):
    """{row: key-axis targets} of the handful rows, and every other row's own column"""
    out = {i: [n_sink + own(i)] for i in range(S)}
    visc = vis.cpu()
    for i in cen.handful(S):
        seen = visc[i].nonzero().flatten()
        out[i] += [n_sink + int(seen[0]), n_sink + int(seen[-1])] + [n_sink + t for t in extra(i)]
        if n_sink:
            out[i] += [0, n_sink - 1]
    return out


# ---- plain chunks: per-head and grouped -------------------------------------------------------------------------------
def _plain(fx, name, G, c0, S, rope):
    from kvquant_amd import ops
    Hq = fx.Hkv * G
    L = c0 + S
    kr, vh, inv = _dequant(fx, rope)
    keys, vals = cen.with_sinks(kr[:, :, :L], vh[:, :, :L], fx)
    vis = cen.vis_causal(c0, S, L, DEV)
    tps = cen.split_plan(Hq, fx.Hkv, S, c0, name == GROUPED)[2]
    personal = _personal(S, fx.sinks, vis, lambda i: c0 + i, lambda i: [c0 - 1, c0])
    shared = [fx.sinks + c for c in cen.boundary_columns(c0, S, tps, L)]
    table = _table(rope)
    run = lambda q: ops._chunk_call("chunk_attention", name, fx.layer(), Hq, c0, q, None, fx.ks, fx.vs, table)
    return _needle("%s nuq%d %d/%d sinks=%d c0=%d S=%d %s" % (name[4:], fx.bits, Hq, fx.Hkv, fx.sinks, c0, S, rope),
                   G, keys, vals, vis, fx.sinks, personal, shared, run)


@pytest.mark.parametrize("rope", ROPES)
def test_needle_tile_edges_with_sinks(rope):
    """nuq4, 2 x 1, 5 sinks (pos_offset = 5: dropped, every column decodes the id five further on), chunks (59 | 63 | 64)
    + (5 | 1 | 65): every column next to a tile edge is a target"""
    fx = _linear(4, 2, 192, 5)
    for c0 in (59, 63, 64):
        for S in (5, 1, 65):
            _plain(fx, HEADS, 1, c0, S, rope)


@pytest.mark.parametrize("rope", ROPES)
def test_needle_three_row_blocks(rope):
    """nuq3, 1 x 2, 5 sinks, 4037 + 600: both sides of all 72 tile edges and 14 split edges (15 splits of 5 tiles), of
    c0 and of the row-block edges"""
    _plain(_linear(3, 1, 4037 + 600, 5), HEADS, 2, 4037, 600, rope)


@pytest.mark.parametrize("rope", ROPES)
def test_needle_128k_grouped(rope):
    """nuq4, 2 x 4, 131072 + 32, grouped: both sides of all 62 split edges (63 splits of 33 tiles) and, of the 2048 tile
    edges, a deliberate sample: the first, the last, those around c0 and one in the middle of every split (all of them
    would be 128 launches of 32 rows)."""
    _plain(_linear(4, 2, 131072 + 32, 0), GROUPED, 4, 131072, 32, rope)


# ---- trees -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rope", ROPES)
@pytest.mark.parametrize("S", [9, 32])
@pytest.mark.parametrize("c0", [100, 4090])
@pytest.mark.parametrize("sinks", [0, 5])
@pytest.mark.parametrize("Hkv,G", [(2, 1), (1, 8)])
def test_needle_trees(Hkv, G, sinks, c0, S, rope):
    """the census table's tree row in full; every shape of tree_check.SHAPES: a row's targets are itself, its parent, the root and the columns before the
    chunk; a node's key sits at sinks + c0 + depth, so its siblings (and in a star every other draft node) carry the same
    key at the same position and only the mask tells them apart"""
    from kvquant_amd import ops
    fx = _linear(4, Hkv, 4090 + 32, sinks)
    Hq = Hkv * G
    L = c0 + S
    kr, vh, inv = _dequant(fx, rope)
    table = _table(rope)
    tps = cen.split_plan(Hq, Hkv, S, c0, True)[2]
    for name, shape in tc.SHAPES.items():
        parent = shape(S)
        keys, vals = cen.with_sinks(cen.tree_rotate(kr, c0, parent, sinks, inv), vh[:, :, :L], fx)
        vis = cen.vis_tree(c0, parent, L, DEV)
        personal = _personal(S, sinks, vis, lambda i: c0 + i, lambda i: [c0 - 1, c0, c0 + parent[i]])
        for i in range(S):                           # (every row: its parent, whose siblings share its position)
            personal[i].append(sinks + c0 + parent[i])
        shared = [sinks + c for c in cen.boundary_columns(c0, S, tps, c0)]
        run = lambda q: ops.chunk_attention_tree(fx.layer(), Hq, c0, q, parent, k_sink=fx.ks, v_sink=fx.vs, rope=table)
        _needle("tree %s %d/%d sinks=%d c0=%d S=%d %s" % (name, Hq, Hkv, sinks, c0, S, rope), G, keys, vals, vis, sinks,
                personal, shared, run)


# ---- rings -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rope", ROPES)
@pytest.mark.parametrize("sinks", [0, 5])
@pytest.mark.parametrize("bits", [4, 2])
def test_needle_ring_two_wraps(bits, sinks, rope):
    """2 x 4, ring C = 192, W = 100 at N = 192, 228, 450 with S = 1, 17, 93, both geometries: the ring column that holds
    token n must rotate at sinks + n.  The statement runs over a linear twin of N tokens (same quantiser, same token)."""
    from kvquant_amd import ops
    from kvquant_amd.cache import ring_token
    Hkv, G, C, W = 2, 4, 192, 100
    Hq = Hkv * G
    fx = cen.Ring(bits, Hkv, C, W, sinks=sinks, same_key=True, device=DEV, seed=4)
    table = _table(rope)
    for N in (192, 228, 450):
        fx.at(N)
        twin = _linear(bits, Hkv, N, sinks, seed=4)
        kr, vh, inv = _dequant(twin, rope)
        keys, vals = cen.with_sinks(kr, vh, twin)
        r = (N - 1) % C
        around = [ring_token(c % C, N, C) for c in (r - 1, r, r + 1)]
        edges = [ring_token(c, N, C) for c in (63, 64, 127, 128, 0, C - 1)]
        for S in (1, 17, 93):
            n0 = N - S
            vis = cen.vis_window(n0, S, W, N, DEV)
            personal = _personal(S, sinks, vis, lambda i: n0 + i, lambda i: [n0 + i - W + 1, n0 - 1, n0] + around)
            shared = [sinks + t for t in edges + around]
            for grouped in ((False, True) if S <= 32 else (False,)):
                run = lambda q: ops.chunk_attention_window(fx.layer(), Hq, n0, W, q, k_sink=fx.ks, v_sink=fx.vs,
                                                           rope=table, grouped=grouped)
                _needle("window nuq%d sinks=%d N=%d S=%d %s %s" % (bits, sinks, N, S, "grouped" if grouped else "heads", rope),
                        G, keys, vals, vis, sinks, personal, shared, run)


# ---- the helper's statement is the project's ----------------------------------------------------------------------------
def test_statement_is_the_projects():
    """census_check.statement over keys rotated by rope_check.dequant (and tree_rotate) against chunk_check.reference,
    tree_check.reference and window_check.reference on one small case each"""
    from tests import window_check as wc
    fx = _linear(4, 2, 192, 5)
    c0, S, G = 100, 9, 2
    q = cc.queries(fx.Hkv * G, S, DEV, 1)
    kr, vh, inv = _dequant(fx, "theta")
    L = c0 + S
    close = lambda a, b: float((a - b).abs().max()) < 1e-9 * float(b.abs().max())
    keys, vals = cen.with_sinks(kr[:, :, :L], vh[:, :, :L], fx)
    assert close(cen.statement(q, keys, vals, cen.vis_causal(c0, S, L, DEV), 5)[0], cc.reference(fx.kc, fx.vc, q, c0, fx.ks, fx.vs))
    assert close(cen.statement(q, keys, vals, cen.vis_window(c0, S, 40, L, DEV), 5)[0],
                 wc.reference(fx.kc, fx.vc, q, c0, 40, fx.ks, fx.vs))
    parent = tc.SHAPES["random"](S)
    keys, vals = cen.with_sinks(cen.tree_rotate(kr, c0, parent, 5, inv), vh[:, :, :L], fx)
    assert close(cen.statement(q, keys, vals, cen.vis_tree(c0, parent, L, DEV), 5)[0],
                 tc.reference(fx.kc, fx.vc, q, c0, parent, fx.ks, fx.vs))
