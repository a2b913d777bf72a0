"""``DeviceReplay.extend`` (the bulk load of IBRL's offline dataset into the ring) against repeated ``append``: the same head, count
and slot contents for every split of a stream of steps, across the wrap and past a full eviction.  CPU only."""
import numpy as np
import pytest
import torch

from dppo_amd.util.replay import DeviceReplay, ReturnsReplay

CAP, E, OD, AD = 5, 2, 3, 4


def stream(T, seed=0):
    rs = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32))
    return f(T, E, OD), f(T, E, OD), f(T, E, AD), f(T, E), torch.from_numpy((rs.uniform(size=(T, E)) < 0.3).astype(np.float32))


def same(a, b, whole=True):
    assert (a.head, a.steps, len(a)) == (b.head, b.steps, len(b))
    if whole:  # slot for slot
        for x, y in zip((a.obs, a.next_obs, a.actions, a.reward, a.terminated), (b.obs, b.next_obs, b.actions, b.reward, b.terminated)):
            assert torch.equal(x, y)
    inds = torch.arange(len(a))
    assert all(torch.equal(x, y) for x, y in zip(a.gather(inds), b.gather(inds)))  # ... and in the logical order


@pytest.mark.parametrize("chunks", [[3], [5], [2, 3], [4, 4], [1, 7, 2], [12], [3, 13, 1], [0, 6, 0, 5]])
def test_extend_equals_repeated_append(chunks):
    data = stream(sum(chunks))
    one, bulk = DeviceReplay(CAP, E, OD, AD, "cpu"), DeviceReplay(CAP, E, OD, AD, "cpu")
    t = 0
    for k in chunks:
        for i in range(t, t + k):
            one.append(*[x[i] for x in data])
        bulk.extend(*[x[t:t + k] for x in data])
        t += k
        same(one, bulk)
    if sum(chunks) > CAP:
        assert one.steps == CAP and one.head == sum(chunks) % CAP  # the oldest were evicted


def test_extend_mixes_with_append_and_takes_numpy():
    data = stream(9, seed=1)
    one, bulk = DeviceReplay(CAP, E, OD, AD, "cpu"), DeviceReplay(CAP, E, OD, AD, "cpu")
    for i in range(9):
        one.append(*[x[i] for x in data])
    bulk.append(*[x[0] for x in data])
    bulk.extend(*[x[1:7].numpy() for x in data])
    bulk.append(*[x[7] for x in data])
    bulk.extend(*[x[8:9] for x in data])
    same(one, bulk)


def test_extend_feeds_a_subclass_with_its_own_append_step_by_step():
    data = stream(4, seed=2)
    one, bulk = ReturnsReplay(CAP, E, OD, AD, "cpu"), ReturnsReplay(CAP, E, OD, AD, "cpu")
    for i in range(4):
        one.append(*[x[i] for x in data])
    bulk.extend(*data)
    same(one, bulk)
    assert bulk.open_slots == one.open_slots and len(bulk.open_slots[0]) == 4
