"""The cache of captured training steps (avec_amd/nnet/captured.py: StepCache), with plain Python callables as entries: recency, eviction at `cache_size`
entries over both kinds, count / clear per kind, and the one warning at 2 * cache_size evictions.  No GPU."""
import warnings

import pytest

from avec_amd.nnet.captured import StepCache


def _key(kind, n, *extra):
    return (kind, ((2, n), "torch.float32"), "torch.bfloat16") + extra


def _fill(cache, keys, cache_size, who="graphed_train_step"):
    """get_or_make every key in order -> [made]"""
    made = []
    for k in keys:
        entry, m = cache.get_or_make(k, lambda k=k: (lambda: k), cache_size, who)
        assert entry() == k, "the entry of a key is the one made for it"
        made.append(m)
    return made


def test_a_hit_returns_the_same_entry_and_makes_it_most_recent():
    c = StepCache()
    a, b, d = _key("step", 1), _key("step", 2), _key("step", 3)
    assert _fill(c, [a, b, d], 3) == [True, True, True] and list(c.entries) == [a, b, d]
    first = c.entries[a]
    entry, made = c.get_or_make(a, _never, 3, "graphed_train_step")
    assert entry is first and not made
    assert list(c.entries) == [b, d, a], "a hit moves the entry to most-recent"
    assert c.evictions == 0


def _never():
    raise AssertionError("make() was called on a hit")


def test_a_new_key_beyond_cache_size_evicts_the_least_recent():
    c = StepCache()
    keys = [_key("step", n) for n in range(4)]
    assert _fill(c, keys[:3], 3) == [True] * 3 and c.count() == 3 and c.evictions == 0      # cache_size entries fit
    _fill(c, [keys[0]], 3)                                                                    # 0 is now the most recent, 1 the least
    assert _fill(c, [keys[3]], 3) == [True]
    assert list(c.entries) == [keys[2], keys[0], keys[3]] and c.evictions == 1
    assert _fill(c, [keys[1]], 3) == [True], "an evicted key is made again"
    assert list(c.entries) == [keys[0], keys[3], keys[1]] and c.evictions == 2


def test_make_that_raises_leaves_no_entry():
    c = StepCache()
    _fill(c, [_key("step", 0)], 2)

    def broken():
        raise RuntimeError("capture failed")
    with pytest.raises(RuntimeError, match="capture failed"):
        c.get_or_make(_key("step", 1), broken, 2, "graphed_train_step")
    assert list(c.entries) == [_key("step", 0)]


def test_count_and_clear_per_kind_and_one_bound_for_both():
    c = StepCache()
    steps, micros = [_key("step", n) for n in range(2)], [_key("micro", n, 3) for n in range(2)]
    _fill(c, steps + micros, 8)
    assert _key("micro", 0, 3) != _key("micro", 0, 2) and _key("micro", 0, 3)[1:3] == _key("step", 0)[1:], "same batch, other kind or other k: another key"
    assert (c.count(), c.count("step"), c.count("micro")) == (4, 2, 2)
    c.clear("micro")
    assert (c.count(), c.count("step"), c.count("micro")) == (2, 2, 0) and list(c.entries) == steps
    c.clear("micro")
    assert c.count() == 2
    _fill(c, micros, 8)
    c.clear("step")
    assert (c.count("step"), c.count("micro")) == (0, 2)
    c.clear()
    assert c.count() == 0 and c.entries == {}
    # cache_size bounds the cache as a whole: two of each kind in a cache of three
    _fill(c, [steps[0], micros[0], steps[1]], 3)
    _fill(c, [micros[1]], 3, who="graphed_micro_step")
    assert c.count() == 3 and list(c.entries) == [micros[0], steps[1], micros[1]] and c.evictions == 1


def test_the_warning_comes_once_at_twice_cache_size_evictions():
    c = StepCache()
    size = 2
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        _fill(c, [_key("micro", n, 1) for n in range(size)], size, who="graphed_micro_step")
        for n in range(size, size + 2 * size - 1):                # evictions 1 .. 2 * size - 1: silent
            _fill(c, [_key("micro", n, 1)], size, who="graphed_micro_step")
        assert c.evictions == 2 * size - 1 and seen == []
        _fill(c, [_key("micro", 100, 1)], size, who="graphed_micro_step")
        assert c.evictions == 2 * size and len(seen) == 1
        text = str(seen[0].message)
        assert text == ("graphed_micro_step: 4 captured steps evicted from a cache of 2 -- the batch shapes do not repeat; bucket the batches "
                        "(graph_bucket_frames / a length-bucketed sampler, nnet/samplers.py) or raise graph_cache_size")
        for n in range(200, 200 + 3 * size):                      # ... and never again
            _fill(c, [_key("micro", n, 1)], size, who="graphed_micro_step")
        c.clear()
        _fill(c, [_key("micro", n, 1) for n in range(300, 300 + 2 * size)], size, who="graphed_micro_step")
        assert len(seen) == 1 and c.evictions > 2 * size


def test_a_deep_copy_is_an_empty_cache():
    import copy
    c = StepCache()
    _fill(c, [_key("step", n) for n in range(3)], 2)
    d = copy.deepcopy({"steps": c})["steps"]
    assert isinstance(d, StepCache) and d is not c and d.count() == 0 and d.evictions == 0 and c.count() == 2 and c.evictions == 1
