"""``TrainIBRLAgent``.  CPU: the host loop against the reference's (agent/finetune/train_ibrl_agent.py, lines cited) with
tests/test_off_policy_agent.py's ``bare_agent``, a scripted single env, a stub offline set whose rows carry their own index, and
recorders in place of the model's losses and the optimisers; every shipped cfg resolves to the agent.  GPU: one ``update_iteration``
with every draw given against the sequence the reference recorded (g32), a short ``run()`` on the synthetic env, and a checkpoint
loaded into a second agent bit for bit."""
import copy
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dppo_amd.cfg.loader import Cfg, get_class, load_config
from dppo_amd.util.replay import DeviceReplay
from tests.test_off_policy_agent import StubSched, bare_agent

HERE = os.path.dirname(os.path.abspath(__file__))
SHIPPED = os.path.join(HERE, "golden", "shipped_ibrl_cfgs.json")
CAN_CFG = "robomimic/finetune/can/ibrl_mlp.yaml"
DEV = "cuda:0"
OFFLINE_LEN, OFFLINE_BASE = 7, 1000.0
TRAIN_KEYS = {"itr", "step", "time", "train_episode_reward", "loss_actor", "loss_critic"}
EVAL_KEYS = {"itr", "step", "time", "eval_success_rate", "eval_episode_reward", "eval_best_reward"}


class OneEnv:
    """One env whose observation is its own step counter; it terminates at t == 3.  Reward: 1 + 0.5 k with k the number of ``step``
    calls."""

    def __init__(self):
        self.t, self.k, self.actions = 0, 0, []

    def _obs(self):
        return [{"state": np.full((1, 2), float(self.t), dtype=np.float32)}]

    def reset_arg(self, options_list=None):
        self.t = 0
        return self._obs()

    def step(self, action):
        self.actions.append(np.array(action, copy=True))
        self.t += 1
        self.k += 1
        terminated = np.array([self.t == 3])
        if terminated[0]:
            self.t = 0
        return self._obs(), np.array([1.0 + 0.5 * self.k]), terminated, np.zeros(1, dtype=bool), [{}]


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


class StubIBRL(torch.nn.Module):
    """The sampler (the first state coordinate, + 0.25 when deterministic) and the two losses, each recording what it was given."""

    def __init__(self, events, agent):
        super().__init__()
        self.events, self.agent, self.calls = events, agent, []
        self.network = SimpleNamespace(mark_updated=lambda: events.append(("actor_marked",)))
        self.flat_grads, self.last_loss_grad = torch.zeros(3), None

    def forward(self, cond, deterministic=False, **kw):
        self.calls.append((bool(deterministic), self.training, dict(kw)))
        s = cond["state"][:, 0, 0].float() + (0.25 if deterministic else 0.0)
        return s.reshape(-1, 1, 1).expand(-1, 2, 3).contiguous()

    def loss_critic(self, obs, next_obs, actions, rewards, terminated, gamma, inds=None, **kw):
        assert obs is self.agent.replay and next_obs is actions is rewards is terminated is None
        self.events.append(("loss_critic", dict(inds=inds.clone(), gamma=gamma, kw=kw, itr=self.agent.itr, ring_len=len(obs),
                                                 training=self.training)))
        return torch.tensor(float(sum(1 for e in self.events if e[0] == "loss_critic")))

    def critic_flat_grads(self):
        return self.flat_grads

    def critics_updated(self):
        self.events.append(("critics_updated",))

    def update_target_critic(self, tau):
        self.events.append(("polyak", tau))

    def loss_actor(self, obs, inds=None, **kw):
        assert obs is self.agent.replay
        self.last_loss_grad = torch.ones(2)
        self.events.append(("loss_actor", dict(inds=inds.clone(), kw=kw)))
        return torch.tensor(-1.5)

    def update_target_actor(self, tau):
        self.events.append(("polyak_actor", tau))


def make_agent(tmp_path, **extra):
    from dppo_amd.agent.finetune.train_ibrl_agent import TrainIBRLAgent
    np.random.seed(0)
    events = []
    attrs = dict(device="cpu", n_cond_step=1, obs_dim=2, action_dim=3, act_steps=2, horizon_steps=2, n_envs=1, n_steps=2, n_train_itr=8,
                 val_freq=3, force_train=False, reset_at_iteration=False, batch_size=4, replay=DeviceReplay(10, 1, 2, 6, "cpu"),
                 scale_reward_factor=0.5, best_reward_threshold_for_success=3, log_freq=1, save_model_freq=100, use_wandb=False, itr=0,
                 venv=OneEnv(), result_path=str(tmp_path / "result.pkl"), actor_lr_scheduler=StubSched(),
                 critic_lr_scheduler=StubSched(), n_explore_steps=2, n_eval_episode=2, critic_num_update=3, update_freq=2,
                 target_ema_rate=0.25, gamma=0.9, dataset_offline=StubOffline(),
                 actor_optimizer=StubOptim(events, "actor_step"), critic_optimizer=StubOptim(events, "critic_step"))
    attrs.update(extra)
    agent = bare_agent(TrainIBRLAgent, **attrs)
    agent.model = StubIBRL(events, agent)
    agent.save_model = lambda: events.append(("save", agent.itr))
    return agent, events


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_ibrl_preload_is_the_dataset_in_order_and_the_oldest_are_evicted(tmp_path):
    """(:91-105) the whole offline set goes into the buffer before the loop, in dataset order, rewards unscaled (scale_reward_factor
    is 0.5 here and must not touch them); a buffer smaller than the set keeps the newest (deque(maxlen))."""
    agent, _ = make_agent(tmp_path)
    agent.preload_offline()
    rp = agent.replay
    obs, nxt, act, rew, term = rp.gather(torch.arange(len(rp)))
    i = np.arange(OFFLINE_LEN, dtype=np.float32)
    assert len(rp) == OFFLINE_LEN and obs[:, 0].tolist() == (OFFLINE_BASE + i).tolist() and nxt[:, 0].tolist() == (OFFLINE_BASE + i + 0.5).tolist()
    assert act.shape == (OFFLINE_LEN, 6) and act[:, 0].tolist() == (-i).tolist() and rew.tolist() == (10 * i).tolist()
    assert term.tolist() == (i % 2).tolist()
    small, _ = make_agent(tmp_path, replay=DeviceReplay(4, 1, 2, 6, "cpu"))
    small.preload_offline()
    assert small.replay.gather(torch.arange(4))[0][:, 0].tolist() == (OFFLINE_BASE + i[3:]).tolist()


def test_ibrl_run_follows_the_references_iteration(tmp_path):
    agent, events = make_agent(tmp_path)
    res = agent.run()
    m, venv = agent.model, agent.venv
    # never a random action (:149-163): every env step's action is the model's, also in iterations 0..n_explore_steps
    assert len(m.calls) == len(venv.actions) and all(a.shape == (1, 2, 3) for a in venv.actions)
    # eval_mode (:125-129) has >: iteration 0 and iteration 2 = n_explore_steps do not evaluate (val_freq 3: 0, 3, 6 -> 3 and 6 do);
    # an evaluation ends by its episode count (:199): 2 episodes of 3 steps
    evals = [i for i in range(8) if i % 3 == 0 and i > 2]
    assert evals == [3, 6] and len(venv.actions) == 6 * 2 + 2 * 6
    det = [c[0] for c in m.calls]
    assert det == [False] * 6 + [True] * 6 + [False] * 4 + [True] * 6 + [False] * 2
    assert [c[1] for c in m.calls] == [not d for d in det]  # model.eval() / .train() (:133)
    # the update (:239-243): not in evaluation, itr > n_explore_steps and itr % update_freq == 0 -> iteration 4 alone (2 is not past
    # the exploration phase, 6 evaluates)
    assert [e[1]["itr"] for e in events if e[0] == "loss_critic"] == [4] * 3
    assert len([e for e in events if e[0] == "loss_actor"]) == 1
    assert all(e[1]["training"] for e in events if e[0] == "loss_critic")
    # records (:308-353): one per iteration; time and the rest only where itr > n_explore_steps.  Deviation: iteration 5 logs after
    # an update and carries both losses, iteration 3 is an evaluation, and a training iteration logged before any update (none in this
    # schedule but 7 below with update_freq 100) carries neither, where the reference's unbound names would raise
    assert agent.itr == 8 and [r["itr"] for r in res] == list(range(8))
    assert [r["step"] for r in res] == [4, 8, 12, 12, 16, 20, 20, 24]
    assert all(set(res[i]) == {"itr", "step"} for i in (0, 1, 2))
    assert set(res[3]) == set(res[6]) == EVAL_KEYS and set(res[4]) == set(res[5]) == set(res[7]) == TRAIN_KEYS
    assert res[4]["loss_critic"] == 3.0 and res[4]["loss_actor"] == -1.5 and res[7]["loss_critic"] == 3.0
    with open(agent.result_path, "rb") as f:
        assert pickle.load(f) == res
    # both schedules every iteration (:300-301); checkpoints at itr % save_model_freq == 0 and at the end (:304)
    assert agent.actor_lr_scheduler.n == agent.critic_lr_scheduler.n == 8
    assert [e for e in events if e[0] == "save"] == [("save", 0), ("save", 7)]
    # the ring: the offline set first, then the training steps with the reward scaled; evaluations wrote nothing; 10 slots keep the newest
    rp = agent.replay
    assert len(rp) == 10 and rp.gather(torch.arange(10))[3].tolist()[-1] == pytest.approx(0.5 * (1.0 + 0.5 * len(venv.actions)))


def test_ibrl_log_fields_are_left_out_until_an_update_has_run(tmp_path):
    agent, events = make_agent(tmp_path, update_freq=100, n_train_itr=5, val_freq=100)
    res = agent.run()
    assert not [e for e in events if e[0] == "loss_critic"]
    assert all(set(r) == {"itr", "step", "time", "train_episode_reward"} for r in res[3:]) and set(res[2]) == {"itr", "step"}


def test_ibrl_update_draws_from_the_one_ring_and_updates_the_actor_once(tmp_path, monkeypatch):
    """(:245-297) per critic update ONE ``np.random.choice(len(buffer), batch_size)`` with replacement from the global generator; each
    critic loss is followed by its step and the Polyak of the target members; then ONE actor loss on the LAST batch, its step, and the
    Polyak of the target actor."""
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
    critic = [e[1] for e in events if e[0] == "loss_critic"]
    # at iteration 4 the ring holds 7 offline rows + the steps of iterations 0, 1, 2 and 4: 15 > 10 slots -> full
    assert [(d[0], d[1], d[2], d[3]) for d in draws] == [(10, 4, (), {})] * 3 and all(c["ring_len"] == 10 for c in critic)
    for c, d in zip(critic, draws):
        np.random.set_state(d[4])
        assert np.array_equal(real(10, 4), d[5]) and c["inds"].tolist() == d[5].tolist() and c["inds"].dtype == torch.int64
        assert c["gamma"] == 0.9 and c["kw"] == dict(pair=None)
    upd = [e for e in events if e[0] != "save"]
    assert [e[0] for e in upd] == ["loss_critic", "critic_step", "critics_updated", "polyak"] * 3 + [
        "loss_actor", "actor_step", "actor_marked", "polyak_actor"]
    assert all(e[1] == 0.25 for e in upd if e[0] in ("polyak", "polyak_actor"))
    assert all(e[1] is agent.model.flat_grads for e in upd if e[0] == "critic_step")
    actor = upd[-4][1]
    assert actor["inds"].tolist() == critic[-1]["inds"].tolist() and actor["kw"] == dict(noise=None, mask=None)
    assert upd[-3][1] is agent.model.last_loss_grad


def test_ibrl_update_iteration_takes_given_draws(tmp_path):
    agent, events = make_agent(tmp_path, critic_num_update=2)
    agent.preload_offline()
    b = [torch.tensor([0, 1, 2, 3]), torch.tensor([4, 5, 6, 0])]
    state = np.random.get_state()
    out = agent.update_iteration(batches=b, pairs=[(0, 1), (2, 0)], critic_draws=[dict(noise_bc="b0", noise_rl="r0"), dict(mask_rl="m1")],
                                 actor_noise="an", actor_mask="am")
    assert all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))
    critic = [e[1] for e in events if e[0] == "loss_critic"]
    assert [c["kw"] for c in critic] == [dict(pair=(0, 1), noise_bc="b0", noise_rl="r0"), dict(pair=(2, 0), mask_rl="m1")]
    assert [c["inds"].tolist() for c in critic] == [[0, 1, 2, 3], [4, 5, 6, 0]]
    actor = next(e[1] for e in events if e[0] == "loss_actor")
    assert actor["kw"] == dict(noise="an", mask="am") and actor["inds"].tolist() == [4, 5, 6, 0]
    assert [float(x) for x in out] == [2.0, -1.5] and not any(x.requires_grad for x in out)


def test_every_shipped_cfg_resolves_to_the_agent():
    from dppo_amd.agent.finetune.train_ibrl_agent import TrainIBRLAgent
    from dppo_amd.agent.finetune.train_off_policy_agent import OffPolicyAgent
    assert get_class("dppo.agent.finetune.train_ibrl_agent.TrainIBRLAgent") is TrainIBRLAgent and issubclass(TrainIBRLAgent, OffPolicyAgent)
    assert TrainIBRLAgent.strictly_past_exploration == ("eval", "update", "log") and TrainIBRLAgent.explores_at_random is False
    cfgs = load_config(SHIPPED)
    assert len(cfgs) == 8
    for name, cfg in cfgs.items():
        assert get_class(cfg._target_) is TrainIBRLAgent and cfg.env.n_envs == 1, name
        for key in ("critic_num_update", "update_freq", "n_eval_episode", "n_explore_steps", "target_ema_rate", "buffer_size",
                    "scale_reward_factor", "actor_weight_decay", "critic_weight_decay", "actor_lr_scheduler", "critic_lr_scheduler"):
            assert key in cfg.train, (name, key)


# ------------------------------------------------------------------------------------------------------------------ GPU
def write_offline(path, obs_dim, action_dim, n_traj=4, traj_len=12, seed=3):
    rs = np.random.RandomState(seed)
    total = n_traj * traj_len
    terminals = np.zeros(total, dtype=np.float32)
    terminals[traj_len - 1::traj_len] = 1
    np.savez(path, states=rs.uniform(-1, 1, (total, obs_dim)).astype(np.float32),
             actions=rs.uniform(-1, 1, (total, action_dim)).astype(np.float32), rewards=rs.uniform(0, 1, total).astype(np.float32),
             terminals=terminals, traj_lengths=np.full(n_traj, traj_len))
    return str(path)


def agent_cfg(tmp_path, **train):
    cfg = copy.deepcopy(load_config(SHIPPED)[CAN_CFG])
    cfg.update(device=DEV, seed=42, logdir=str(tmp_path), env=Cfg(n_envs=1, name="synthetic", max_episode_steps=5, reset_at_iteration=False))
    cfg.model.update(device=DEV)
    cfg.model.pop("network_path", None)
    for node in (cfg.model.actor, cfg.model.critic):
        node["precision"] = "fp32"
        node["mlp_dims"] = [64, 64]
    cfg["offline_dataset"] = Cfg(_target_="dppo.agent.dataset.sequence.StitchedSequenceQLearningDataset", horizon_steps=cfg.horizon_steps,
                                 cond_steps=cfg.cond_steps, max_n_episodes=100, device=DEV,
                                 dataset_path=write_offline(tmp_path / "offline.npz", cfg.obs_dim, cfg.action_dim))
    cfg.train.update(dict(n_train_itr=8, n_explore_steps=1, batch_size=8, buffer_size=50, val_freq=100, save_model_freq=100, log_freq=1,
                          n_steps=2, update_freq=2, critic_num_update=2), **train)
    return cfg


@pytest.mark.gpu
def test_hip_ibrl_agent_update_is_the_recorded_sequence(tmp_path):
    """One fp32 ``update_iteration`` of a real agent on tiny, N = 77, straight off the ring with every draw given, against the
    sequence the reference recorded: two critic steps each with Polyak, one actor step, the target actor's Polyak."""
    from dppo_amd.agent.finetune.train_ibrl_agent import TrainIBRLAgent
    from dppo_amd.util.optim import FlatAdamW
    from tests.golden import make_golden_ibrl_actor_cases as A
    from tests.test_dql import check_stepped
    from tests.test_ibrl import make_model
    from tests.test_idql import check_grads_fp32
    from tests.test_rlpd_actor import member_rows
    from tests.test_sac import check_stepped_twice, named
    K = A.K
    g = np.load(os.path.join(HERE, "golden", "g32_ibrl_actor.npz"))
    case, n = A.SEQ_CASE, A.SEQ_N
    agent = TrainIBRLAgent(agent_cfg(tmp_path, n_train_itr=0))
    m = agent.model = make_model(case, "fp32", DEV)
    m.train()
    od, ta, da = K.shapes(case)
    agent.gamma, agent.target_ema_rate, agent.critic_num_update = K.GAMMA, A.SEQ_TAU, len(A.SEQ_PAIRS)
    agent.critic_optimizer = FlatAdamW(m.critic_flat_params(), lr=A.SEQ_LR, weight_decay=A.SEQ_WEIGHT_DECAY)
    agent.actor_optimizer = FlatAdamW(m.network.flat_params(), lr=A.SEQ_ACTOR_LR, weight_decay=A.SEQ_WEIGHT_DECAY)
    b = {k: v.to(DEV) for k, v in K.inputs(case, n).items()}
    rp = agent.replay = DeviceReplay(n + 5, 1, od, ta * da, DEV)
    rp.extend(torch.zeros(9, 1, od), torch.zeros(9, 1, od), torch.zeros(9, 1, ta * da), torch.zeros(9, 1), torch.zeros(9, 1))
    rp.extend(b["obs"].reshape(n, 1, -1), b["next_obs"].reshape(n, 1, -1), b["actions"].reshape(n, 1, -1), b["reward"].reshape(n, 1),
              b["terminated"].reshape(n, 1))
    assert rp.head != 0 and len(rp) == n + 5  # wrapped: the batch's rows start at logical index 5
    inds = torch.arange(5, n + 5, device=DEV)
    draws = dict(noise_bc=b["noise_bc"], noise_rl=b["noise_rl"], mask_bc=b["mask_bc"], mask_rl=b["mask_rl"])
    seen = []
    inner = m.loss_critic
    m.loss_critic = lambda *a, **kw: seen.append(inner(*a, **kw).detach().clone()) or seen[-1]
    lc, la = agent.update_iteration(batches=[inds, inds], pairs=list(A.SEQ_PAIRS), critic_draws=[draws, draws], actor_noise=b["noise_rl"],
                                    actor_mask=b["mask_rl"])
    print(f"seq: critic {float(lc)!r} ref {g['seq_c_losses'].tolist()!r}; actor {float(la)!r} ref {float(g['seq_a_loss'])!r}")
    assert len(seen) == 2 and float(seen[-1]) == float(lc)
    np.testing.assert_allclose([float(x) for x in seen] + [float(la)], list(g["seq_c_losses"]) + [float(g["seq_a_loss"])], rtol=2e-4, atol=2e-5)
    E = K.n_critics(case)
    check_grads_fp32(g, "seq_gq1", member_rows(m.critic_flat_grads(), E))
    check_grads_fp32(g, "seq_ga", named(m.network, m.last_loss_grad))
    actor = [(k, p) for k, p in m.network.named_parameters() if p.requires_grad]
    check_stepped(g, "seq_actor", actor, "seq_ga", A.SEQ_ACTOR_LR)
    target = [(k, p) for k, p in m.target_actor.named_parameters() if p.requires_grad]
    check_stepped(g, "seq_target_actor", target, "seq_ga", A.SEQ_ACTOR_LR * A.SEQ_TAU)
    # a member took two AdamW steps; its target two Polyak averages (tests/test_ibrl_actor.py's CPU test has the bound)
    check_stepped_twice(g, "seq_q", member_rows(m.critic_flat_params(), E), ("seq_gq0", "seq_gq1"), A.SEQ_LR)
    check_stepped_twice(g, "seq_target", member_rows(m.target_flat_params(), E), ("seq_gq0", "seq_gq1"), 2 * A.SEQ_LR * A.SEQ_TAU)


@pytest.mark.gpu
def test_hip_ibrl_agent_runs_and_its_checkpoint_loads_bit_for_bit(tmp_path):
    """The shipped can cfg shrunk (batch 8, hidden 64, a synthetic offline file and env).  The offline set is in the ring before the
    first step; iterations 2, 4 and 6 update; records carry the reference's keys; the actor, the members and all three targets moved
    and the imitation policy did not; a second agent loads the last checkpoint bit for bit."""
    from dppo_amd.agent.finetune.train_ibrl_agent import TrainIBRLAgent
    agent = TrainIBRLAgent(agent_cfg(tmp_path))
    m = agent.model
    assert len(agent.dataset_offline) == 4 * 12 and m.network.dropout == 0.5
    before = {k: f().clone() for k, f in (("actor", m.network.flat_params), ("target_actor", m.target_actor.flat_params),
                                           ("bc", m.bc_policy.flat_params), ("q", m.critic_flat_params), ("tq", m.target_flat_params))}
    calls = []
    inner = agent.update_iteration
    agent.update_iteration = lambda **kw: calls.append((agent.itr, len(agent.replay))) or inner(**kw)
    res = agent.run()
    # 48 offline rows and the 6 steps of iterations 0 to 2 met buffer_size = 50 before the first update: the oldest offline rows are gone
    assert [c[0] for c in calls] == [2, 4, 6] and calls[0][1] == 50 and len(agent.replay) == 50
    for r in res[2:]:
        assert set(r) == TRAIN_KEYS and np.isfinite([r["loss_actor"], r["loss_critic"]]).all()
    assert set(res[0]) == set(res[1]) == {"itr", "step"}
    now = dict(actor=m.network.flat_params(), target_actor=m.target_actor.flat_params(), bc=m.bc_policy.flat_params(),
               q=m.critic_flat_params(), tq=m.target_flat_params())
    for k in ("actor", "target_actor", "q", "tq"):
        assert not torch.equal(now[k], before[k]) and bool(torch.isfinite(now[k]).all()), k
    assert torch.equal(now["bc"], before["bc"])
    data = torch.load(os.path.join(str(tmp_path), "checkpoint", "state_7.pt"), weights_only=True)
    assert list(data["model"]) == list(m.state_dict())
    second = tmp_path / "second"
    second.mkdir()
    other = TrainIBRLAgent(agent_cfg(second))
    assert not torch.equal(other.model.network.flat_params(), m.network.flat_params())
    other.checkpoint_dir = agent.checkpoint_dir
    other.load(7)
    assert other.itr == 7
    om = other.model
    for a, b in ((om.network, m.network), (om.target_actor, m.target_actor), (om.bc_policy, m.bc_policy)):
        assert torch.equal(a.flat_params(), b.flat_params())
    assert torch.equal(om.critic_flat_params(), m.critic_flat_params()) and torch.equal(om.target_flat_params(), m.target_flat_params())
    # ... and acts like the first from there on: the kernel images follow the loaded weights
    cond = {"state": torch.zeros(4, 1, 23, device=DEV)}
    om.eval(), m.eval()
    noise = torch.zeros(4, 1, 7, device=DEV)
    kw = dict(deterministic=True, pair=(0, 1), noise_bc=noise, noise_rl=noise)
    assert torch.equal(om(cond, **kw), m(cond, **kw))
