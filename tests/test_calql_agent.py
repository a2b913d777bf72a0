"""The host loop of ``TrainCalQLAgent`` on the CPU: a scripted single env, tests/test_off_policy_agent.py's ``bare_agent`` and stub
model, a stub offline dataset whose rows carry their own index, and recorders in place of the optimisers.  Every expectation is read
off the reference's loop (agent/finetune/train_calql_agent.py, lines cited) and off the four deviations the agent's docstring
lists, not off the code under test.  Then: every shipped cfg resolves to the agent and its ``offline_dataset`` node builds."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dppo_amd.cfg.loader import get_class, instantiate, load_config
from dppo_amd.util.replay import ReturnsReplay
from tests.test_off_policy_agent import StubModel, StubSched, bare_agent

HERE = os.path.dirname(os.path.abspath(__file__))
SHIPPED = os.path.join(HERE, "golden", "shipped_calql_agent_cfgs.json")
OFFLINE_LEN, OFFLINE_BASE = 7, 1000.0
TRAIN_KEYS = {"itr", "step", "time", "train_episode_reward", "loss_actor", "loss_critic", "alpha"}
EVAL_KEYS = {"itr", "step", "time", "eval_success_rate", "eval_episode_reward", "eval_best_reward"}
GAMMA, SCALE = 0.9, 0.5


class ScriptedEnv:
    """One env whose observation is its step counter within the episode.  Episode i lasts LENGTHS[i % len] steps; odd episodes
    terminate, even ones truncate and hand over ``final_obs`` = 100 + t.  The k-th ``step`` call pays reward k (1, 2, ...)."""
    LENGTHS = (3, 1, 2, 4, 2)

    def __init__(self):
        self.t, self.k, self.ep = 0, 0, 0
        self.actions, self.log = [], []  # log: (k, episode, done) per step

    def _obs(self):
        return {"state": np.full((1, 1, 2), float(self.t), dtype=np.float32)}

    def reset_arg(self, options_list=None):
        self.t = 0
        return self._obs()

    def step(self, action):
        self.actions.append(np.array(action, copy=True))
        self.t += 1
        self.k += 1
        done = self.t >= self.LENGTHS[self.ep % len(self.LENGTHS)]
        terminated, truncated = np.array([done and self.ep % 2 == 1]), np.array([done and self.ep % 2 == 0])
        info = [{}]
        if truncated[0]:
            info[0]["final_obs"] = {"state": np.full((1, 2), 100.0 + self.t, dtype=np.float32)}
        self.log.append((self.k, self.ep, bool(done)))
        if done:
            self.t, self.ep = 0, self.ep + 1
        return self._obs(), np.array([float(self.k)]), terminated, truncated, info


class StubOffline:
    """Sample i: state OFFLINE_BASE + i, next state + 0.5, action -i, reward 10 i, done = i odd, reward-to-go 100 i."""

    def __len__(self):
        return OFFLINE_LEN

    def gather(self, idx):
        f, n = idx.double().float(), len(idx)
        cond = {"state": (OFFLINE_BASE + f).reshape(n, 1, 1).expand(n, 1, 2), "next_state": (OFFLINE_BASE + f + 0.5).reshape(n, 1, 1).expand(n, 1, 2)}
        return SimpleNamespace(actions=(-f).reshape(n, 1, 1).expand(n, 2, 3), conditions=cond, rewards=(10 * f).reshape(n, 1),
                               dones=(idx % 2).float().reshape(n, 1), reward_to_gos=(100 * f).reshape(n, 1))


class StubOptim:
    def __init__(self, events, name):
        self.events, self.name, self.param_groups = events, name, [{"lr": 0.1}]

    def step(self, grad):
        self.events.append((self.name, grad))


class StubCalQL(StubModel):
    """StubModel's sampler plus the three losses, each recording what it was given."""

    def __init__(self, events, agent):
        super().__init__()
        self.events, self.agent = events, agent
        self.grads, self.actor_grad = torch.zeros(3), torch.ones(2)
        self.network = SimpleNamespace(mark_updated=lambda: events.append(("actor_marked",)))
        self.critic = SimpleNamespace(flat_grads=lambda: self.grads, mark_updated=lambda: events.append(("critic_marked",)))
        self.last_loss_grad = None

    def loss_critic(self, obs, next_obs, actions, random_actions, rewards, returns, terminated, gamma, **kw):
        self.events.append(("loss_critic", dict(obs=obs["state"].clone(), next_obs=next_obs["state"].clone(), actions=actions.clone(),
                                                 random_actions=random_actions, rewards=rewards.clone(), returns=returns.clone(),
                                                 terminated=terminated.clone(), gamma=gamma, kw=kw, itr=self.agent.itr)))
        return torch.tensor(float(sum(1 for e in self.events if e[0] == "loss_critic")))

    def update_target_critic(self, tau):
        self.events.append(("polyak", tau))

    def loss_actor(self, obs, alpha, **kw):
        self.last_loss_grad = self.actor_grad
        self.events.append(("loss_actor", dict(obs=obs["state"].clone(), alpha=float(alpha), kw=kw)))
        return torch.tensor(-1.5)

    def loss_temperature(self, obs, log_alpha, target_entropy, **kw):
        self.events.append(("loss_temperature", dict(obs=obs["state"].clone(), target_entropy=target_entropy, kw=kw)))
        return (log_alpha * 2.0).sum()


def make_agent(tmp_path, **extra):
    from dppo_amd.agent.finetune.train_calql_agent import TrainCalQLAgent
    np.random.seed(0)
    events = []
    attrs = dict(device="cpu", n_cond_step=1, obs_dim=2, action_dim=3, act_steps=2, horizon_steps=2, n_envs=1, n_steps=1, n_train_itr=6,
                 val_freq=2, force_train=False, reset_at_iteration=False, batch_size=4, replay=ReturnsReplay(16, 1, 2, 6, "cpu"),
                 scale_reward_factor=SCALE, best_reward_threshold_for_success=3, log_freq=1, save_model_freq=100, use_wandb=False, itr=0,
                 venv=ScriptedEnv(), result_path=str(tmp_path / "result.pkl"), actor_lr_scheduler=StubSched(),
                 critic_lr_scheduler=StubSched(), n_explore_steps=1, n_eval_episode=2, n_episode_per_epoch=1, num_update=3,
                 train_online=True, automatic_entropy_tuning=True, target_ema_rate=0.25, gamma=GAMMA, target_entropy=-6.0,
                 dataset_offline=StubOffline(), log_alpha=torch.tensor(np.log(0.5), dtype=torch.float64, requires_grad=True),
                 actor_optimizer=StubOptim(events, "actor_step"), critic_optimizer=StubOptim(events, "critic_step"))
    attrs.update(extra)
    agent = bare_agent(TrainCalQLAgent, **attrs)
    agent.model = StubCalQL(events, agent)
    agent.log_alpha_optimizer = torch.optim.Adam([agent.log_alpha], lr=0.01)
    agent.save_model = lambda: events.append(("save", agent.itr))
    return agent, events


def returns_of(rewards, gamma=GAMMA):
    out, prev = [], 0.0
    for r in reversed(rewards):
        prev = r + gamma * prev
        out.append(prev)
    return out[::-1]


def ring(agent):
    rp = agent.replay
    return [x.tolist() for x in rp.gather(torch.arange(len(rp)))]


def test_online_run_follows_the_references_iteration(tmp_path):
    """n_explore_steps = 1, val_freq = 2: iteration 0 explores and trains nothing (:301), 1, 3 and 5 train, 2 and 4 evaluate (>=,
    :154-158).  A training rollout ends with its first finished episode (n_episode_per_epoch = 1, :240), an evaluation with its second
    (:238).  Episodes in the env's order: 0 (3 steps, itr 0), 1 (1 step, itr 1), 2 and 3 (eval), 4 (2 steps, itr 3), 5 and 6 (eval),
    7 (2 steps, itr 5)."""
    agent, events = make_agent(tmp_path)
    res = agent.run()
    m, venv = agent.model, agent.venv
    assert [ep for _, ep, _ in venv.log] == [0] * 3 + [1] + [2] * 2 + [3] * 4 + [4] * 2 + [5] * 3 + [6] + [7] * 2
    # exploration (:185-186): iteration 0's three actions are uniform draws, no model call; evaluations sample deterministically
    assert all(a.dtype == np.float32 and a.shape == (1, 2, 3) and np.abs(a).max() <= 1.0 for a in venv.actions[:3])
    assert [c[0] for c in m.calls] == [False] + [True] * 6 + [False] * 2 + [True] * 4 + [False] * 2
    assert [c[1] for c in m.calls] == [True] + [False] * 6 + [True] * 2 + [False] * 4 + [True] * 2  # model.train() / .eval() (:166)
    # the update count is the step count of the iteration's first finished episode (:314): 1, 2 and 2
    assert [e[1]["itr"] for e in events if e[0] == "loss_critic"] == [1] + [3] * 2 + [5] * 2
    assert len([e for e in events if e[0] == "loss_actor"]) == 5
    # records: one per iteration, logged from n_explore_steps on (>=, :462)
    assert agent.itr == 6 and [r["itr"] for r in res] == list(range(6)) and [r["step"] for r in res] == [6, 8, 8, 12, 12, 16]
    assert set(res[0]) == {"itr", "step"} and set(res[1]) == set(res[3]) == set(res[5]) == TRAIN_KEYS
    assert set(res[2]) == set(res[4]) == EVAL_KEYS
    assert res[1]["loss_critic"] == 1.0 and res[3]["loss_critic"] == 3.0 and res[5]["loss_actor"] == -1.5
    # a one-step episode is not counted in the episode statistics (end - start > 1, :250), like the reference
    assert res[1]["train_episode_reward"] == 0 and res[3]["train_episode_reward"] == 11 + 12 and res[5]["train_episode_reward"] == 17 + 18
    assert res[2]["eval_episode_reward"] == pytest.approx(((5 + 6) + (7 + 8 + 9 + 10)) / 2)
    with open(agent.result_path, "rb") as f:
        assert pickle.load(f) == res
    assert agent.actor_lr_scheduler.n == agent.critic_lr_scheduler.n == 6  # both schedules every iteration (:447-449)
    assert [e for e in events if e[0] == "save"] == [("save", 0), ("save", 5)]


def test_returns_stay_with_their_transitions(tmp_path):
    """Deviations 1, 2 and 4.  Only training episodes are stored: 0 (rewards 1, 2, 3), 1 (4), 4 (11, 12), 7 (17, 18); the evaluations in
    between wrote neither transitions nor returns.  The one-step episode 1 has its return.  Rewards are stored scaled by
    scale_reward_factor = 0.5, returns are formed from the UNSCALED rewards (the reference's arithmetic, :213, :226, :253-270)."""
    agent, _ = make_agent(tmp_path)
    agent.run()
    obs, nxt, act, rew, term, rtg = ring(agent)
    env_rewards = [[1, 2, 3], [4], [11, 12], [17, 18]]
    flat = [r for ep in env_rewards for r in ep]
    assert rew == [SCALE * r for r in flat]
    assert rtg == pytest.approx([x for ep in env_rewards for x in returns_of(ep)])
    assert agent.replay.n_closed() == len(agent.replay) == 8
    # a truncated episode's last next_obs is its final_obs (episodes 0 and 4 truncate at t = 3 and 2), a terminated one's (1 and 7) the reset
    assert [o[0] for o in obs] == [0, 1, 2, 0, 0, 1, 0, 1] and [o[0] for o in nxt] == [1, 2, 103, 0, 1, 102, 1, 0]
    assert term == [0, 0, 0, 1, 0, 0, 0, 1]


def test_update_draws_offline_then_online_and_runs_in_the_references_order(tmp_path, monkeypatch):
    """(:317-445) per update two ``np.random.choice`` draws with replacement, offline first, ``batch_size // 2`` each, from the
    global generator; the batch is [offline half | online half] with the returns; then the temperature's snapshot, critic loss
    (random_actions=None: the kernel draws them), critic step, mark, Polyak, actor loss on the same batch with the snapshot, actor
    step, temperature loss and step."""
    agent, events = make_agent(tmp_path)
    draws, real = [], np.random.choice

    def choice(a, size=None, *args, **kw):
        state = np.random.get_state()
        out = real(a, size, *args, **kw)
        draws.append((a, size, args, kw, state, np.array(out)))
        return out
    monkeypatch.setattr(np.random, "choice", choice)
    agent.run()
    monkeypatch.setattr(np.random, "choice", real)
    assert [(d[0], d[1], d[2], d[3]) for d in draws] == [(OFFLINE_LEN, 2, (), {}), (4, 2, (), {}), (OFFLINE_LEN, 2, (), {}), (6, 2, (), {}),
                                                         (OFFLINE_LEN, 2, (), {}), (6, 2, (), {}), (OFFLINE_LEN, 2, (), {}), (8, 2, (), {}),
                                                         (OFFLINE_LEN, 2, (), {}), (8, 2, (), {})]
    critic = [e[1] for e in events if e[0] == "loss_critic"]
    for i, c in enumerate(critic):
        off, on = draws[2 * i], draws[2 * i + 1]
        np.random.set_state(off[4])  # the same stream of the global generator gives the same indices
        assert np.array_equal(real(OFFLINE_LEN, 2), off[5])
        assert c["obs"].shape == (4, 2) and c["actions"].shape == (4, 6) and c["rewards"].shape == c["returns"].shape == c["terminated"].shape == (4,)
        assert c["obs"][:2, 0].tolist() == (OFFLINE_BASE + off[5]).tolist() and c["next_obs"][:2, 0].tolist() == (OFFLINE_BASE + off[5] + 0.5).tolist()
        assert c["actions"][:2, 0].tolist() == (-off[5]).tolist() and c["rewards"][:2].tolist() == (10.0 * off[5]).tolist()
        assert c["returns"][:2].tolist() == (100.0 * off[5]).tolist() and c["terminated"][:2].tolist() == (off[5] % 2).astype(float).tolist()
        assert c["gamma"] == GAMMA and c["random_actions"] is None and (c["obs"][2:] < OFFLINE_BASE).all()
        assert c["kw"] == dict(samples=None, noise=None)
        if c["itr"] == 5:  # (the ring no longer changes after iteration 5's rollout)
            want = agent.replay.gather(torch.from_numpy(on[5].astype(np.int64)))
            for k, x in zip(("obs", "next_obs", "actions", "rewards", "terminated", "returns"), want):
                assert torch.equal(c[k][2:], x.reshape(c[k][2:].shape)), k
    it3 = [e for e in events if e[0] != "save"][8:24]  # iteration 1 made one update (8 events), iteration 3 two
    one = ["loss_critic", "critic_step", "critic_marked", "polyak", "loss_actor", "actor_step", "actor_marked", "loss_temperature"]
    assert [e[0] for e in it3] == one * 2
    assert all(e[1] == 0.25 for e in it3 if e[0] == "polyak") and all(e[1] is agent.model.grads for e in it3 if e[0] == "critic_step")
    for u in (it3[:8], it3[8:]):
        assert torch.equal(u[4][1]["obs"], u[0][1]["obs"]) and torch.equal(u[7][1]["obs"], u[0][1]["obs"]) and u[7][1]["target_entropy"] == -6.0
        assert u[5][1] is agent.model.actor_grad
    # the snapshot is taken before the update's own temperature step: Adam moves log_alpha by 0.01 per update (d loss / d log_alpha = 2)
    alphas = [e[1]["alpha"] for e in events if e[0] == "loss_actor"]
    assert alphas == pytest.approx([0.5 * np.exp(-0.01 * i) for i in range(5)], rel=1e-6)
    assert float(agent.log_alpha.detach()) == pytest.approx(np.log(0.5) - 5 * 0.01, abs=1e-6)


def test_without_entropy_tuning_the_temperature_stays(tmp_path):
    agent, events = make_agent(tmp_path, automatic_entropy_tuning=False)
    agent.run()
    assert not [e for e in events if e[0] == "loss_temperature"] and float(agent.log_alpha.detach()) == pytest.approx(np.log(0.5))
    assert len([e for e in events if e[0] == "loss_actor"]) == 5


def test_no_update_when_no_episode_closed(tmp_path):
    """Deviation 3.  With n_episode_per_epoch = 0 a training rollout is one step (:240), so iterations 0 and 1 close no episode --
    the 3-step episode 0 stays open -- and make no update; its returns are written when it closes, over the transitions
    of all three iterations; nothing open is ever drawn."""
    agent, events = make_agent(tmp_path, n_episode_per_epoch=0, n_explore_steps=0, force_train=True, n_train_itr=4)
    seen = []
    inner = agent.draw_batch
    agent.draw_batch = lambda: seen.append((agent.itr, agent.replay.n_closed(), len(agent.replay))) or inner()
    agent.run()
    # iterations 0 and 1: episode 0 still open, no update; iteration 2 closes it (3 steps -> 3 updates); iteration 3 closes the
    # one-step episode 1 (1 update)
    assert [e[1]["itr"] for e in events if e[0] == "loss_critic"] == [2, 2, 2, 3]
    assert seen == [(2, 3, 3)] * 3 + [(3, 4, 4)]
    assert ring(agent)[5] == pytest.approx(returns_of([1, 2, 3]) + returns_of([4]))


def test_offline_mode_trains_on_the_dataset_alone(tmp_path, monkeypatch):
    """train_online = false (:160-165, :316-322): no training rollout, ``num_update`` updates per iteration on ``batch_size`` offline
    rows, one draw each; evaluations still run."""
    agent, events = make_agent(tmp_path, train_online=False, n_explore_steps=0, n_train_itr=4)
    del agent.n_episode_per_epoch  # (:82-84: read in online mode only)
    sizes, real = [], np.random.choice
    monkeypatch.setattr(np.random, "choice", lambda a, size=None, *args, **kw: sizes.append((a, size)) or real(a, size, *args, **kw))
    res = agent.run()
    monkeypatch.setattr(np.random, "choice", real)
    assert [e[1]["itr"] for e in events if e[0] == "loss_critic"] == [1] * 3 + [3] * 3 and sizes == [(OFFLINE_LEN, 4)] * 6
    assert len(agent.replay) == 0 and [r["step"] for r in res] == [0] * 4
    assert len(agent.venv.log) == (3 + 1) + (2 + 4)  # iterations 0 and 2 evaluate two episodes each
    c = next(e[1] for e in events if e[0] == "loss_critic")
    assert c["obs"].shape == (4, 2) and (c["obs"] >= OFFLINE_BASE).all() and c["returns"].tolist() == (10 * c["rewards"]).tolist()
    assert set(res[0]) == EVAL_KEYS and set(res[1]) == TRAIN_KEYS


def test_update_iteration_takes_given_draws(tmp_path):
    """``update_iteration`` with the batch and every draw injected calls the generator for nothing and returns device scalars."""
    agent, events = make_agent(tmp_path)
    b = dict(obs=torch.full((4, 2), 7.0), next_obs=torch.zeros(4, 2), actions=torch.zeros(4, 6), reward=torch.zeros(4),
             terminated=torch.zeros(4), returns=torch.arange(4.0))
    state = np.random.get_state()
    out = agent.update_iteration(batches=[b], samples="sm", sample_noise="sn", random_actions="ra", actor_noise="an", temp_noise="tn")
    assert all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))
    critic = next(e[1] for e in events if e[0] == "loss_critic")
    assert critic["kw"] == dict(samples="sm", noise="sn") and critic["random_actions"] == "ra" and critic["returns"].tolist() == [0, 1, 2, 3]
    actor, temp = next(e[1] for e in events if e[0] == "loss_actor"), next(e[1] for e in events if e[0] == "loss_temperature")
    assert actor["kw"] == dict(noise="an") and temp["kw"] == dict(noise="tn") and actor["obs"][0, 0] == 7.0
    assert [float(x) for x in out] == [1.0, -1.5, float(2 * np.log(0.5))] and not any(x.requires_grad for x in out)
    assert [float(x) for x in agent.update_iteration(batches=b)[:2]] == [2.0, -1.5]  # the batch itself is accepted too


# ------------------------------------------------------------------------------------------------------------------ the shipped cfgs
def write_offline(path, obs_dim, action_dim, n_traj=3, traj_len=6, seed=3):
    rs = np.random.RandomState(seed)
    total = n_traj * traj_len
    terminals = np.zeros(total, dtype=np.float32)
    terminals[traj_len - 1::traj_len] = 1
    np.savez(path, states=rs.uniform(-1, 1, (total, obs_dim)).astype(np.float32),
             actions=rs.uniform(-1, 1, (total, action_dim)).astype(np.float32), rewards=rs.uniform(0, 1, total).astype(np.float32),
             terminals=terminals, traj_lengths=np.full(n_traj, traj_len))
    return str(path)


def test_every_shipped_cfg_resolves_to_the_agent_and_builds_its_offline_dataset(tmp_path):
    from dppo_amd.agent.dataset.sequence import StitchedSequenceQLearningDataset
    from dppo_amd.agent.finetune.train_calql_agent import TrainCalQLAgent
    from dppo_amd.agent.finetune.train_off_policy_agent import OffPolicyAgent
    assert get_class("dppo.agent.finetune.train_calql_agent.TrainCalQLAgent") is TrainCalQLAgent and issubclass(TrainCalQLAgent, OffPolicyAgent)
    cfgs = load_config(SHIPPED)
    assert len(cfgs) == 16 and sum(bool(c.train.train_online) for c in cfgs.values()) == 8
    for name, cfg in cfgs.items():
        assert get_class(cfg._target_) is TrainCalQLAgent and cfg.env.n_envs == 1, name
        assert cfg.train.scale_reward_factor == 1.0, name  # (deviation 4 changes nothing on a shipped cfg)
        for key in ("train_online", "num_update", "n_random_actions", "n_eval_episode", "n_explore_steps", "init_temperature",
                    "automatic_entropy_tuning", "target_entropy", "target_ema_rate", "buffer_size", "actor_weight_decay",
                    "critic_weight_decay"):
            assert key in cfg.train, (name, key)
        assert ("n_episode_per_epoch" in cfg.train) or not cfg.train.train_online, name
        node = cfg.offline_dataset
        assert get_class(node._target_) is StitchedSequenceQLearningDataset and node.get_mc_return is True, name
        assert node.discount_factor == cfg.train.gamma, name
        ds = instantiate(node, dataset_path=write_offline(tmp_path / "offline.npz", cfg.obs_dim, cfg.action_dim), device="cpu")
        got = ds.gather(torch.tensor([0, 5]))
        assert got.reward_to_gos.shape == (2, 1) and got.conditions["state"].shape == (2, cfg.cond_steps, cfg.obs_dim), name
        assert got.actions.shape == (2, cfg.horizon_steps, cfg.action_dim) and "next_state" in got.conditions, name
