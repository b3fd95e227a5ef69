"""The cached weight planes (genrl_amd/planes.py) while agents go away.  An entry of planes._wcache is dropped by a finalizer of its
parameter; an agent that went away is usually a reference cycle, so the finalizers run inside whatever allocation triggers the garbage
collector -- also one made while the cache is being walked.  A dictionary that changes size under its own iterator raises RuntimeError
('dictionary changed size during iteration'), which made a refresh after an optimiser step fail depending on how much garbage the tests
before it had left.  Here the finalizer is made to fire at a fixed point of the walk."""
import weakref

import torch

from genrl_amd import planes


class Gone:
    """a parameter-like object that can be weakly referenced and dropped at will"""


def entry(obj, epoch, stream):
    return [epoch, None, 0, weakref.ref(obj), stream]


def test_an_entry_dropped_during_the_walk_does_not_break_a_refresh(monkeypatch):
    cache = {}
    monkeypatch.setattr(planes, '_wcache', cache)
    objs = [Gone() for _ in range(4)]
    keys = [(id(o), False, 0, 4) for o in objs]

    class DropsAnother:
        """the stream field of the first entry: comparing it -- what the walk does per entry -- lets another entry's parameter die, as a
        collection at that point would"""
        def __eq__(self, other):
            cache.pop(keys[3], None)
            return False
    for i, (k, o) in enumerate(zip(keys, objs)):
        cache[k] = entry(o, -1, DropsAnother() if i == 0 else 'other stream')
    planes._refresh_stale('this stream')          # nothing is on this stream: no launch, but the whole cache is walked
    assert keys[3] not in cache and len(cache) == 3


def test_a_dead_weight_is_skipped_and_a_live_one_is_held():
    live, dead = Gone(), Gone()
    cache = {(1, False, 0, 4): entry(live, -1, 's'), (2, False, 0, 4): entry(dead, -1, 's')}
    del dead
    saved = planes._wcache
    planes._wcache = cache
    try:
        picked = planes._live(lambda key, ent: True)
    finally:
        planes._wcache = saved
    assert [key for key, _, _ in picked] == [(1, False, 0, 4)] and picked[0][2] is live


def test_invalidate_walks_copies():
    p = torch.nn.Parameter(torch.zeros(2, 2))
    saved = planes._wcache, planes._dcache

    class Cache(dict):
        def items(self):
            raise AssertionError('the cache itself was walked')
    planes._wcache, planes._dcache = Cache({(id(p), False, 0, 2): [3, None, 0, weakref.ref(p), 's']}), Cache({(id(p), 'tag'): [3, None, 0, weakref.ref(p), 's', None]})
    try:
        planes.invalidate([p])
        assert planes._wcache[(id(p), False, 0, 2)][0] == -1 and planes._dcache[(id(p), 'tag')][0] == -1
    finally:
        planes._wcache, planes._dcache = saved
