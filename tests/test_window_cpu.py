"""Host logic of the ring caches and the sliding-window routing (no GPU): the column -> token map against a
brute-force ring, the wrap split of a pack, the piece route of a long prompt, the truncate rule, config reading."""
import types

import pytest

from kvquant_amd import llama as kl
from kvquant_amd.attention import window_capacity, window_route
from kvquant_amd.cache import ring_check, ring_pieces, ring_token, ring_truncate_ok


@pytest.mark.parametrize("C", [64, 192])
def test_column_token_map_against_a_simulated_ring(C):
    ring = [None] * C
    for n in range(3 * C + 7):
        ring[n % C] = n
        N = n + 1
        for c in range(min(N, C)):
            assert ring_token(c, N, C) == ring[c], (c, N)
        # the closed form the kernel evaluates: base - (c > r ? C : 0)
        base, r = (N - 1) // C * C, (N - 1) % C
        assert all(ring_token(c, N, C) == c + base - (C if c > r else 0) for c in range(min(N, C)))


def test_visible_columns_are_the_window():
    """row i of a chunk n0 .. n0+S-1 sees exactly the tokens (n0 + i - W, n0 + i] under every valid call, and none of them
    has been overwritten by the chunk (W + S - 1 <= C)"""
    C, W = 192, 100
    for n0, S in [(0, 1), (99, 93), (191, 1), (192, 17), (300, 93), (383, 2)]:
        N = n0 + S
        held = {c: ring_token(c, N, C) for c in range(min(N, C))}
        assert sorted(held.values()) == list(range(max(N - C, 0), N))
        for i in (0, S - 1):
            want = set(range(max(n0 + i - W + 1, 0), n0 + i + 1))
            assert want <= set(held.values())


def test_pack_pieces():
    assert ring_pieces(0, 10, 192) == [(0, 0, 10)]
    assert ring_pieces(150, 42, 192) == [(150, 0, 42)]                   # ends at the last column
    assert ring_pieces(150, 60, 192) == [(150, 0, 42), (0, 42, 18)]      # crosses the wrap
    assert ring_pieces(192 * 3 + 191, 2, 192) == [(191, 0, 1), (0, 1, 1)]
    assert ring_pieces(384, 192, 192) == [(0, 0, 192)]
    assert ring_pieces(5, 0, 192) == []
    for n0, S in [(0, 192), (100, 192), (191, 190)]:
        cols = [(c + j) for c, _, n in ring_pieces(n0, S, 192) for j in range(n)]
        assert cols == [(n0 + i) % 192 for i in range(S)]
        offs = [o + j for _, o, n in ring_pieces(n0, S, 192) for j in range(n)]
        assert offs == list(range(S))
    with pytest.raises(ValueError):
        ring_pieces(0, 193, 192)


def test_ring_check_and_capacity():
    assert ring_check(100, 192) == 100 and ring_check(192, 192) == 192 and ring_check(1, 64) == 1
    for W, C in [(0, 192), (-1, 192), (193, 192), (100, 200), (100, 0)]:
        with pytest.raises(ValueError):
            ring_check(W, C)
    assert window_capacity(40, 88) == 128 and window_capacity(40, 89) == 192
    assert window_capacity(4096) == 4352 and window_capacity(32768) == 33024 and window_capacity(1, 0) == 64
    with pytest.raises(ValueError):
        window_capacity(0)


def test_route_of_a_long_prompt():
    C, W = 128, 40                           # pieces of C - W + 1 = 89 rows
    assert window_route(0, 300, 0, W, C) == [("prefill", 40), ("chunk", 89), ("chunk", 89), ("chunk", 82)]
    assert window_route(0, 300, 5, W, C) == [("prefill", 45), ("chunk", 89), ("chunk", 89), ("chunk", 77)]
    assert window_route(0, 30, 5, W, C) == [("prefill", 30)]
    assert window_route(0, 3, 5, W, C) == [("prefill", 3)]
    assert window_route(3, 4, 5, W, C) == [("token", 2), ("chunk", 2)]
    assert window_route(0, 1, 5, W, C) == [("token", 1)]
    assert window_route(0, 1, 0, W, C) == [("chunk", 1)]                 # (a first token on a ring: no decode route)
    assert window_route(500, 1, 5, W, C) == [("chunk", 1)]
    assert window_route(500, 90, 0, W, C) == [("chunk", 89), ("chunk", 1)]
    assert window_route(0, 5, 0, 1, 64) == [("chunk", 5)]                # (W = 1: no prefill piece of two rows)
    for klen, q_len, sinks in [(0, 1000, 0), (0, 1000, 5), (2, 77, 5), (640, 200, 5)]:
        route = window_route(klen, q_len, sinks, W, C)
        assert sum(n for _, n in route) == q_len
        assert all(n <= C - W + 1 for kind, n in route if kind == "chunk")


def test_truncate_rule():
    C, W = 192, 100
    assert ring_truncate_ok(150, 150, W, C, 150)                 # never wrapped: everything is still there
    assert ring_truncate_ok(192, 100, W, C, 192)
    assert ring_truncate_ok(400, 93, W, C, 400)                  # the slack: C - W + 1 tokens
    assert not ring_truncate_ok(400, 94, W, C, 400)
    assert not ring_truncate_ok(390, 84, W, C, 400)              # (an earlier rollback does not reset the high water)
    assert ring_truncate_ok(390, 83, W, C, 400)
    # a simulated ring: write tokens 0 .. hw-1 (token t into column t mod C), roll back to N, drop n more as truncate
    # does (the dropped tokens' columns are emptied), and ask whether the next token N - n still finds its W - 1
    # predecessors in the columns
    for C, W in ((192, 100), (64, 40), (64, 64)):
        for hw in (C - 3, C, C + 1, C + 57, 2 * C + 8):
            for N in range(max(hw - C, 1), hw + 1):
                ring = [None] * C
                for t in range(hw):
                    ring[t % C] = t
                for t in range(N, hw):
                    ring[t % C] = None
                for n in range(0, N):             # (at least one token stays: the next one has a predecessor to find)
                    if n:
                        ring[(N - n) % C] = None
                    held = set(x for x in ring if x is not None)
                    want = set(range(max(N - n - W + 1, 0), N - n))
                    assert ring_truncate_ok(N, n, W, C, hw) == (want <= held), (C, W, hw, N, n)


def _cfg(**kw):
    return types.SimpleNamespace(**kw)


def test_config_reading():
    assert kl.layer_windows(_cfg(), 2) == [None, None]
    assert kl.layer_windows(_cfg(sliding_window=None), 2) == [None, None]
    assert kl.layer_windows(_cfg(sliding_window=4096), 2) == [4096, 4096]
    assert kl.layer_windows(_cfg(sliding_window=4096, use_sliding_window=False), 2) == [None, None]
    assert kl.layer_windows(_cfg(sliding_window=4096, use_sliding_window=True), 2) == [4096, 4096]
    mixed = _cfg(sliding_window=512, layer_types=["sliding_attention", "full_attention", "sliding_attention"])
    assert kl.layer_windows(mixed, 3) == [512, None, 512]
    assert kl.layer_windows(mixed, 3, sliding_window=0) == [None, None, None]
    assert kl.layer_windows(mixed, 3, sliding_window=64) == [64, None, 64]
    assert kl.layer_windows(_cfg(sliding_window=4096), 2, sliding_window=0) == [None, None]
    assert kl.layer_windows(_cfg(), 2, sliding_window=40) == [40, 40]
    # an explicit window overrides use_sliding_window = False (the caller asked for it)
    assert kl.layer_windows(_cfg(sliding_window=4096, use_sliding_window=False), 1, sliding_window=40) == [40]
    with pytest.raises(ValueError):
        kl.layer_windows(_cfg(), 2, sliding_window=-1)


def test_config_reading_on_transformers_configs():
    from transformers import LlamaConfig, MistralConfig
    small = dict(vocab_size=64, hidden_size=256, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                 num_key_value_heads=1)
    assert kl.layer_windows(LlamaConfig(**small), 2) == [None, None]
    assert kl.layer_windows(MistralConfig(sliding_window=40, **small), 2) == [40, 40]
    assert kl.layer_windows(MistralConfig(sliding_window=None, **small), 2) == [None, None]
    assert kl.layer_windows(MistralConfig(sliding_window=40, **small), 2, sliding_window=0) == [None, None]
