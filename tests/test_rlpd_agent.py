"""The host loop of ``TrainRLPDAgent`` on the CPU: tests/test_off_policy_agent.py's scripted vector env and ``bare_agent``, a stub
model that records the loss calls, and a stub offline dataset whose rows carry their own index.  Every expectation is read off the
reference's loop (agent/finetune/train_rlpd_agent.py, lines cited), not off the code under test."""
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dppo_amd.util.replay import DeviceReplay
from tests.test_off_policy_agent import E, ScriptedVecEnv, StubModel, StubSched, bare_agent, check_env_arrays_untouched

OFFLINE_LEN, OFFLINE_BASE = 7, 1000.0
TRAIN_KEYS = {"itr", "step", "time", "train_episode_reward", "loss_actor", "loss_critic", "alpha"}
EVAL_KEYS = {"itr", "step", "time", "eval_success_rate", "eval_episode_reward", "eval_best_reward"}


class StubOffline:
    """Sample i: state OFFLINE_BASE + i, next state OFFLINE_BASE + i + 0.5, action -i, reward 10 i, done = i odd."""

    def __len__(self):
        return OFFLINE_LEN

    def gather(self, idx):
        f = idx.double().float()
        n = len(idx)
        cond = {"state": (OFFLINE_BASE + f).reshape(n, 1, 1).expand(n, 1, 2), "next_state": (OFFLINE_BASE + f + 0.5).reshape(n, 1, 1).expand(n, 1, 2)}
        return SimpleNamespace(actions=(-f).reshape(n, 1, 1).expand(n, 2, 3), conditions=cond, rewards=(10 * f).reshape(n, 1),
                               dones=(idx % 2).float().reshape(n, 1))


class StubOptim:
    def __init__(self, events, name):
        self.events, self.name, self.param_groups = events, name, [{"lr": 0.1}]

    def step(self, grad):
        self.events.append((self.name, grad))


class StubRLPD(StubModel):
    """StubModel's sampler plus the three losses, each recording what it was given."""

    def __init__(self, events, agent):
        super().__init__()
        self.events, self.agent = events, agent
        self.network = SimpleNamespace(mark_updated=lambda: events.append(("actor_marked",)))
        self.flat_grads, self.last_loss_grad = torch.zeros(3), None

    def loss_critic(self, obs, next_obs, actions, rewards, terminated, gamma, alpha, **kw):
        rp = self.agent.replay
        ring = rp.gather(torch.arange(len(rp)))[1][:, 0].tolist()
        self.events.append(("loss_critic", dict(obs=obs["state"].clone(), next_obs=next_obs["state"].clone(), actions=actions.clone(),
                                                 rewards=rewards.clone(), terminated=terminated.clone(), gamma=gamma, alpha=float(alpha),
                                                 kw=kw, itr=self.agent.itr, ring_next=ring)))
        return torch.tensor(float(sum(1 for e in self.events if e[0] == "loss_critic")))

    def critic_flat_grads(self):
        return self.flat_grads

    def critics_updated(self):
        self.events.append(("critics_updated",))

    def update_target_critic(self, tau):
        self.events.append(("polyak", tau))

    def loss_actor(self, obs, alpha, **kw):
        self.last_loss_grad = torch.ones(2)
        self.events.append(("loss_actor", dict(obs=obs["state"].clone(), alpha=float(alpha), kw=kw)))
        return torch.tensor(-1.5)

    def loss_temperature(self, obs, log_alpha, target_entropy, **kw):
        self.events.append(("loss_temperature", dict(obs=obs["state"].clone(), target_entropy=target_entropy, kw=kw)))
        return (log_alpha * 2.0).sum()


def make_agent(tmp_path, **extra):
    from dppo_amd.agent.finetune.train_rlpd_agent import TrainRLPDAgent
    np.random.seed(0)
    events = []
    attrs = dict(device="cpu", n_cond_step=1, obs_dim=2, action_dim=3, act_steps=2, horizon_steps=2, n_envs=E, n_steps=2, n_train_itr=6,
                 val_freq=2, force_train=False, reset_at_iteration=False, batch_size=4, replay=DeviceReplay(4, E, 2, 6, "cpu"),
                 scale_reward_factor=0.5, best_reward_threshold_for_success=3, log_freq=1, save_model_freq=100, use_wandb=False, itr=0,
                 venv=ScriptedVecEnv(), result_path=str(tmp_path / "result.pkl"), actor_lr_scheduler=StubSched(),
                 critic_lr_scheduler=StubSched(), n_explore_steps=2, n_eval_episode=2, critic_num_update=3, target_ema_rate=0.25,
                 gamma=0.9, target_entropy=-6.0, dataset_offline=StubOffline(),
                 log_alpha=torch.tensor(np.log(0.5), dtype=torch.float64, requires_grad=True),
                 actor_optimizer=StubOptim(events, "actor_step"), critic_optimizer=StubOptim(events, "critic_step"))
    attrs.update(extra)
    agent = bare_agent(TrainRLPDAgent, **attrs)
    agent.model = StubRLPD(events, agent)
    agent.log_alpha_optimizer = torch.optim.Adam([agent.log_alpha], lr=0.01)
    agent.save_model = lambda: events.append(("save", agent.itr))
    return agent, events


def test_rlpd_run_follows_the_references_iteration(tmp_path):
    agent, events = make_agent(tmp_path)
    res = agent.run()
    m, venv = agent.model, agent.venv
    # exploration (:157-158) in iterations 0 and 1: four uniform draws, no model call
    explore = venv.actions[:4]
    assert all(a.dtype == np.float32 and a.shape == (E, 2, 3) and np.abs(a).max() <= 1.0 for a in explore)
    # eval_mode (:132-136) has >=: iteration 2 = n_explore_steps evaluates, and so does 4; each ends by its episode count (:206):
    # env 0 terminates and env 1 truncates at its third step
    assert len(venv.actions) == 4 * 2 + 2 * 3
    assert [c[0] for c in m.calls] == [True] * 3 + [False] * 2 + [True] * 3 + [False] * 2
    assert [c[1] for c in m.calls] == [False] * 3 + [True] * 2 + [False] * 3 + [True] * 2  # model.eval() / .train() (:140)
    # the update (:246) runs outside evaluation from n_explore_steps on: iterations 3 and 5, critic_num_update critic losses each
    assert [e[1]["itr"] for e in events if e[0] == "loss_critic"] == [3] * 3 + [5] * 3
    assert len([e for e in events if e[0] == "loss_actor"]) == 2
    # records (:358-403): one per iteration; time and what follows it only where itr % log_freq == 0 and itr > n_explore_steps, so
    # the evaluation of iteration 2 is not logged
    assert agent.itr == 6 and [r["itr"] for r in res] == list(range(6)) and [r["step"] for r in res] == [12, 24, 24, 36, 36, 48]
    assert all(set(res[i]) == {"itr", "step"} for i in (0, 1, 2))
    assert set(res[3]) == set(res[5]) == TRAIN_KEYS and set(res[4]) == EVAL_KEYS
    assert res[3]["loss_critic"] == 3.0 and res[5]["loss_critic"] == 6.0 and res[5]["loss_actor"] == -1.5
    assert res[3]["alpha"] == pytest.approx(float(agent.log_alpha.detach().exp()), rel=0.1) and res[3]["alpha"] != 0.5
    with open(agent.result_path, "rb") as f:
        assert pickle.load(f) == res
    # both schedules every iteration (:349-351); checkpoints at itr % save_model_freq == 0 and at the end (:354)
    assert agent.actor_lr_scheduler.n == agent.critic_lr_scheduler.n == 6
    assert [e for e in events if e[0] == "save"] == [("save", 0), ("save", 5)]
    check_env_arrays_untouched(venv)


def test_rlpd_final_obs_reaches_the_ring(tmp_path):
    """(:186-191) a truncated env's next observation is its pre-reset ``final_obs`` (dict or bare array); a terminated env's is what
    the env returned.  At the first update the ring holds iteration 1's and 3's steps; evaluations wrote nothing."""
    agent, events = make_agent(tmp_path)
    agent.run()
    first = next(e[1] for e in events if e[0] == "loss_critic")
    assert np.array(first["ring_next"]).reshape(4, E).tolist() == [[0, 103, 3], [1, 1, 104], [1, 1, 104], [2, 2, 1]]
    rp = agent.replay
    assert len(rp) == 4 * E and rp.gather(torch.arange(12))[1][:, 0].reshape(4, E).tolist() == [[1, 1, 104], [2, 2, 1]] * 2


def test_rlpd_update_draws_offline_then_online_and_updates_the_actor_once(tmp_path, monkeypatch):
    """(:249-347) per critic update two ``np.random.choice`` draws with replacement, offline first, ``batch_size // 2`` each, from the
    global generator; the batch is [offline half | online half]; each critic loss is followed by its step and the Polyak average;
    then ONE actor loss on the LAST batch with the last temperature snapshot, its step, and the temperature loss on that batch."""
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
    assert [(d[0], d[1], d[2], d[3]) for d in draws] == [(OFFLINE_LEN, 2, (), {}), (4 * E, 2, (), {})] * 6
    critic = [e[1] for e in events if e[0] == "loss_critic"]
    ring_rows = agent.replay.gather  # (the ring no longer changes between iteration 5's draws and the end of the run)
    for i, c in enumerate(critic):
        off, on = draws[2 * i], draws[2 * i + 1]
        np.random.set_state(off[4])  # the same stream of the global generator gives the same indices
        assert np.array_equal(real(OFFLINE_LEN, 2), off[5])
        assert c["obs"].shape == (4, 2) and c["actions"].shape == (4, 6) and c["rewards"].shape == (4,) and c["terminated"].shape == (4,)
        assert c["obs"][:2, 0].tolist() == (OFFLINE_BASE + off[5]).tolist() and c["next_obs"][:2, 0].tolist() == (OFFLINE_BASE + off[5] + 0.5).tolist()
        assert c["actions"][:2, 0].tolist() == (-off[5]).tolist() and c["rewards"][:2].tolist() == (10.0 * off[5]).tolist()
        assert c["terminated"][:2].tolist() == (off[5] % 2).astype(float).tolist()
        assert c["gamma"] == 0.9 and (c["obs"][2:] < OFFLINE_BASE).all()
        if c["itr"] == 5:
            want = ring_rows(torch.from_numpy(on[5].astype(np.int64)))
            assert torch.equal(c["obs"][2:], want[0]) and torch.equal(c["next_obs"][2:], want[1]) and torch.equal(c["actions"][2:], want[2])
            assert torch.equal(c["rewards"][2:], want[3]) and torch.equal(c["terminated"][2:], want[4])
    # the order of one iteration's update
    it5 = [e for e in events if e[0] != "save"][len([e for e in events if e[0] != "save"]) // 2:]
    assert [e[0] for e in it5] == ["loss_critic", "critic_step", "critics_updated", "polyak"] * 3 + [
        "loss_actor", "actor_step", "actor_marked", "loss_temperature"]
    assert all(e[1] == 0.25 for e in it5 if e[0] == "polyak")
    assert all(e[1] is agent.model.flat_grads for e in it5 if e[0] == "critic_step")
    actor, temp, last = it5[-4][1], it5[-1][1], it5[-8][1]
    assert torch.equal(actor["obs"], last["obs"]) and torch.equal(temp["obs"], last["obs"]) and temp["target_entropy"] == -6.0
    assert actor["alpha"] == last["alpha"]  # the snapshot of the last critic update (:313, :331-334)
    assert it5[-3][1] is agent.model.last_loss_grad
    # the temperature moved once per update iteration, by Adam on d loss / d log_alpha = 2
    assert float(agent.log_alpha.detach()) == pytest.approx(np.log(0.5) - 2 * 0.01, abs=1e-6)
    assert critic[0]["alpha"] == pytest.approx(0.5) and critic[3]["alpha"] == pytest.approx(0.5 * np.exp(-0.01), rel=1e-6)


def test_rlpd_update_iteration_takes_given_draws(tmp_path):
    """``update_iteration`` with every draw injected calls the generator for nothing and hands each repeat its own pair, sample and
    noise."""
    agent, events = make_agent(tmp_path, critic_num_update=2)
    b = [dict(obs=torch.full((4, 2), float(i)), next_obs=torch.zeros(4, 2), actions=torch.zeros(4, 6), reward=torch.zeros(4),
              terminated=torch.zeros(4)) for i in range(2)]
    state = np.random.get_state()
    out = agent.update_iteration(batches=b, pairs=[(0, 1), (2, 0)], next_actions=["na0", "na1"], next_logp=["nl0", "nl1"],
                                 actor_noise="an", temp_noise="tn")
    assert all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))
    critic = [e[1] for e in events if e[0] == "loss_critic"]
    assert [c["kw"] for c in critic] == [dict(next_actions="na0", next_logp="nl0", noise=None, pair=(0, 1)),
                                         dict(next_actions="na1", next_logp="nl1", noise=None, pair=(2, 0))]
    actor = next(e[1] for e in events if e[0] == "loss_actor")
    temp = next(e[1] for e in events if e[0] == "loss_temperature")
    assert actor["kw"] == dict(noise="an") and temp["kw"] == dict(noise="tn") and actor["obs"][0, 0] == 1.0
    assert [float(x) for x in out] == [2.0, -1.5, float(2 * np.log(0.5))] and not any(x.requires_grad for x in out)
