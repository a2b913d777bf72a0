"""``ReturnsReplay`` (dppo_amd/util/replay.py) on the CPU: a return lives in its own transition's slot, so it follows it through
wrap-around and eviction; only transitions of closed episodes are drawn; an episode longer than the ring is an error; and
``DeviceReplay`` is what it was for its present users."""
import numpy as np
import pytest
import torch

from dppo_amd.util.replay import DeviceReplay, ReturnsReplay


def put(rp, tag, n_envs=1):
    """One step whose every column carries ``tag`` (+ 0.1 e for env e): obs, next_obs = tag + 0.5, action = -tag, reward = 10 tag."""
    t = tag + 0.1 * np.arange(n_envs)
    rp.append(np.repeat(t[:, None], 2, 1), np.repeat(t[:, None] + 0.5, 2, 1), np.repeat(-t[:, None], 3, 1), 10 * t, np.zeros(n_envs))


def rows(rp, inds=None):
    inds = torch.arange(len(rp)) if inds is None else inds
    return [x.tolist() for x in rp.gather(inds)]


def test_device_replay_is_unchanged():
    rp = DeviceReplay(4, 1, 2, 3, "cpu")
    for t in range(6):
        put(rp, float(t))
    assert len(rp.gather(torch.arange(4))) == 5 and not hasattr(rp, "reward_to_go")
    assert rp.gather(torch.arange(4))[3].tolist() == [20.0, 30.0, 40.0, 50.0]


def test_returns_land_in_their_own_transitions_and_open_episodes_are_not_drawn():
    rp = ReturnsReplay(8, 1, 2, 3, "cpu")
    for t in range(3):
        put(rp, float(t))
    assert len(rp) == 3 and rp.n_closed() == 0 and rp.closed_indices().tolist() == []
    with pytest.raises(ValueError):  # nothing may be drawn while every stored transition belongs to the open episode
        rp.draw(1, 2)
    rp.close_episode([100.0, 101.0, 102.0])
    put(rp, 3.0)
    put(rp, 4.0)  # a second episode, still open
    assert rp.closed_indices().tolist() == [0, 1, 2] and rp.n_closed() == 3
    obs, nxt, act, rew, term, rtg = rows(rp)
    assert len(rp.gather(torch.arange(5))) == 6
    assert [o[0] for o in obs] == [0, 1, 2, 3, 4] and rtg[:3] == [100.0, 101.0, 102.0]
    np.random.seed(0)
    drawn = rp.draw(20, 4)
    assert drawn.shape == (20, 4) and set(drawn.reshape(-1).tolist()) == {0, 1, 2}
    with pytest.raises(ValueError, match="2 transitions"):
        rp.close_episode([1.0])  # one return for two transitions
    rp.close_episode([200.0, 201.0])
    assert rp.closed_indices().tolist() == [0, 1, 2, 3, 4] and rows(rp)[5] == [100.0, 101.0, 102.0, 200.0, 201.0]
    rp.close_episode([])  # no open episode: nothing to do


def test_returns_follow_their_transitions_through_wrap_around_and_eviction():
    """cap 5: episodes of 3, 2 and 3 steps.  The third wraps around and evicts the first; every surviving transition keeps the return
    written for it, and the logical order stays oldest first."""
    rp = ReturnsReplay(5, 1, 2, 3, "cpu")
    t = 0
    for length in (3, 2, 3):
        tags = []
        for _ in range(length):
            put(rp, float(t))
            tags.append(t)
            t += 1
        if length == 3 and t == 8:  # while the third episode is open its transitions are stored but not drawable
            assert [o[0] for o in rows(rp)[0]] == [3, 4, 5, 6, 7] and rp.closed_indices().tolist() == [0, 1]
        rp.close_episode([1000.0 + k for k in tags])
    assert rp.head == 3 and len(rp) == 5
    obs, _, _, rew, _, rtg = rows(rp)
    assert [o[0] for o in obs] == [3, 4, 5, 6, 7] and rtg == [1003.0, 1004.0, 1005.0, 1006.0, 1007.0]
    assert rew == [30.0, 40.0, 50.0, 60.0, 70.0]
    picked = torch.tensor([4, 0, 2])
    assert rows(rp, picked)[5] == [1007.0, 1003.0, 1005.0] and [o[0] for o in rows(rp, picked)[0]] == [7, 3, 5]
    # eviction of a closed transition by an open one makes that slot undrawable until its own episode closes
    put(rp, 8.0)
    assert [o[0] for o in rows(rp)[0]] == [4, 5, 6, 7, 8] and rp.closed_indices().tolist() == [0, 1, 2, 3]
    rp.close_episode([1008.0])
    assert rows(rp)[5] == [1004.0, 1005.0, 1006.0, 1007.0, 1008.0]


def test_an_episode_longer_than_the_ring_is_an_error():
    rp = ReturnsReplay(3, 1, 2, 3, "cpu")
    for t in range(3):
        put(rp, float(t))
    with pytest.raises(ValueError, match="longer than the replay ring"):
        put(rp, 3.0)
    rp.close_episode([1.0, 2.0, 3.0])
    put(rp, 3.0)  # a closed episode may be evicted
    assert [o[0] for o in rows(rp)[0]] == [1, 2, 3] and rp.closed_indices().tolist() == [0, 1]


def test_envs_close_their_episodes_independently():
    rp = ReturnsReplay(4, 2, 2, 3, "cpu")
    for t in range(3):
        put(rp, float(t), n_envs=2)
    rp.close_episode([5.0, 6.0, 7.0], env=1)
    assert rp.closed_indices().tolist() == [1, 3, 5]  # logical index = step * n_envs + env
    assert rows(rp, torch.tensor([1, 3, 5]))[5] == [5.0, 6.0, 7.0]
    put(rp, 3.0, n_envs=2)
    rp.close_episode([8.0], env=1)
    rp.close_episode([1.0, 2.0, 3.0, 4.0], env=0)
    assert rp.n_closed() == 8 and rows(rp)[5] == [1.0, 5.0, 2.0, 6.0, 3.0, 7.0, 4.0, 8.0]
