"""``StitchedSequenceQLearningDataset`` (reference agent/dataset/sequence.py:204-350), the offline transitions of RLPD / Cal-QL /
IBRL, on a hand-made five-episode file: which steps are samples (the last step of a TRUNCATED episode is not), ``next_state`` at
horizon 1 and 4, the ``cond_steps = 2`` padding at episode starts, and the discounted reward-to-go against a direct loop.  The
expectations are written out per sample the way the reference's ``__getitem__`` slices them."""
import numpy as np
import pytest
import torch

from dppo_amd.agent.dataset.sequence import StitchedSequenceQLearningDataset, Transition, TransitionWithReturn

LENGTHS = [5, 1, 7, 4, 6]
ENDS_TERMINAL = [True, True, False, False, True]  # episodes 2 and 3 are truncated: their last step has no next state in the file
OBS, ACT = 3, 2


@pytest.fixture(scope="module")
def npz(tmp_path_factory):
    total, rs = sum(LENGTHS), np.random.RandomState(5)
    states = (np.arange(total, dtype=np.float32)[:, None] * 10 + np.arange(OBS, dtype=np.float32)[None])  # row t reads 10 t + column
    actions = rs.uniform(-1, 1, size=(total, ACT)).astype(np.float32)
    rewards = rs.uniform(0, 2, size=total).astype(np.float32)
    terminals = np.zeros(total, dtype=bool)
    for end, term in zip(np.cumsum(LENGTHS), ENDS_TERMINAL):
        terminals[end - 1] = term
    path = tmp_path_factory.mktemp("rlpd") / "five_episodes.npz"
    np.savez(path, states=states, actions=actions, rewards=rewards, terminals=terminals, traj_lengths=np.array(LENGTHS))
    return str(path), dict(states=states, actions=actions, rewards=rewards, terminals=terminals)


def expected_index(horizon):
    """(start, steps since the episode began) of every sample, by the reference's rule."""
    out, cur = [], 0
    for n, term in zip(LENGTHS, ENDS_TERMINAL):
        max_start = cur + n - horizon - (0 if term else 1)
        out += [(i, i - cur) for i in range(cur, max_start + 1)]
        cur += n
    return out


@pytest.mark.parametrize("horizon", [1, 4])
@pytest.mark.parametrize("cond_steps", [1, 2])
def test_samples_next_states_and_padding(npz, horizon, cond_steps):
    path, raw = npz
    ds = StitchedSequenceQLearningDataset(path, horizon_steps=horizon, cond_steps=cond_steps, device="cpu")
    index = expected_index(horizon)
    assert len(ds) == len(index)
    if horizon == 1:  # every step but the two truncated episodes' last ones
        assert len(ds) == sum(LENGTHS) - 2
        starts = [s for s, _ in index]
        assert 5 + 1 + 7 - 1 not in starts and 5 + 1 + 7 + 4 - 1 not in starts and 5 - 1 in starts and 5 in starts
    batch = ds.gather(torch.arange(len(ds)))
    assert isinstance(batch, Transition) and batch.rewards.shape == (len(ds), 1) and batch.dones.shape == (len(ds), 1)
    assert batch.conditions["state"].shape == batch.conditions["next_state"].shape == (len(ds), cond_steps, OBS)
    for i, (start, before) in enumerate(index):
        assert np.array_equal(batch.actions[i].numpy(), raw["actions"][start:start + horizon])
        assert batch.rewards[i, 0].item() == raw["rewards"][start] and batch.dones[i, 0].item() == float(raw["terminals"][start])
        # the reference slices states[start - before : start + 1] and, horizon later, the same window; then picks max(before - t, 0)
        window = raw["states"][start - before:start + 1]
        want = np.stack([window[max(before - t, 0)] for t in reversed(range(cond_steps))])
        assert np.array_equal(batch.conditions["state"][i].numpy(), want), i
        if i < len(index) - horizon:
            window = raw["states"][start - before + horizon:start + 1 + horizon]
            want = np.stack([window[max(before - t, 0)] for t in reversed(range(cond_steps))])
        else:
            want = np.zeros_like(want)
        assert np.array_equal(batch.conditions["next_state"][i].numpy(), want), i
        item = ds[i]
        assert torch.equal(item.conditions["next_state"], batch.conditions["next_state"][i]) and torch.equal(item.actions, batch.actions[i])
    if cond_steps == 2:  # at an episode's first step both observations are the same one
        first = [i for i, (_, before) in enumerate(index) if before == 0]
        st = batch.conditions["state"][first]
        assert len(first) >= 3 and torch.equal(st[:, 0], st[:, 1])  # (horizon 4 leaves three episodes with a sample)
        later = [i for i, (_, before) in enumerate(index) if before > 0]
        st = batch.conditions["state"][later]
        assert torch.equal(st[:, 0] + 10, st[:, 1])


def test_reward_to_go_is_the_direct_loop(npz):
    path, raw = npz
    gamma = 0.9
    ds = StitchedSequenceQLearningDataset(path, horizon_steps=1, cond_steps=1, device="cpu", discount_factor=gamma, get_mc_return=True)
    want, cur = np.zeros(sum(LENGTHS), dtype=np.float32), 0
    for n in LENGTHS:
        for t in range(cur, cur + n):
            want[t] = np.float32(sum(float(raw["rewards"][k]) * gamma ** (k - t) for k in range(t, cur + n)))
        cur += n
    assert np.allclose(ds.reward_to_go.numpy(), want, rtol=1e-6, atol=0)
    assert ds.reward_to_go[4].item() == raw["rewards"][4] and ds.reward_to_go[5].item() == raw["rewards"][5]  # episode ends
    batch = ds.gather(torch.tensor([0, 3, 7]))
    assert isinstance(batch, TransitionWithReturn)
    starts = [s for s, _ in expected_index(1)]
    assert torch.equal(batch.reward_to_gos[:, 0], ds.reward_to_go[[starts[0], starts[3], starts[7]]])


def test_max_n_episodes_and_file_format(npz, tmp_path):
    path, raw = npz
    ds = StitchedSequenceQLearningDataset(path, horizon_steps=1, cond_steps=1, device="cpu", max_n_episodes=3)
    assert len(ds) == 5 + 1 + 7 - 1 and ds.rewards.numel() == 13 and ds.states.shape[0] == 13
    with pytest.raises(ValueError, match="npz"):
        StitchedSequenceQLearningDataset(str(tmp_path / "data.pkl"), device="cpu")
