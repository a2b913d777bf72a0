"""The host loops of the off-policy agents (IDQL, QSM, DQL, SAC) on the CPU: a scripted vector env, a stub model and recorders in
place of ``update_minibatch`` / ``save_model``.  ``FlatAdamW`` refuses CPU tensors, so the agents are not constructed: ``bare_agent``
makes an instance without ``__init__`` and sets what ``run()`` reads.  Every expected value below was recorded from the four
hand-copied ``run()`` bodies that preceded ``OffPolicyAgent``; the shared loop has to reproduce them.  Then the shared model
helpers (``off_policy.as_batch``, ``flat_views``, ``Workspace.get``) as far as they go without a device."""
import pickle

import numpy as np
import pytest
import torch

from dppo_amd import hip
from dppo_amd.util.replay import DeviceReplay

E = 3


class ScriptedVecEnv:
    """3 envs whose observation is their own step counter.  Env 0 terminates at t == 3; env e > 0 truncates at t >= e + 2 and
    hands over ``final_obs`` = 100 + t, as ``{"state": ...}`` for odd e and as a bare array for even e.  Reward: arange(E) + 0.5 k
    with k the number of ``step`` calls.  Observations come back as a list of dicts."""

    def __init__(self):
        self.t, self.k = np.zeros(E, dtype=np.int64), 0
        self.handed_out = []  # (array as returned, copy at that time)
        self.actions = []

    def _obs(self):
        out = [{"state": np.full((1, 2), float(self.t[e]), dtype=np.float32)} for e in range(E)]
        self.handed_out += [(o["state"], o["state"].copy()) for o in out]
        return out

    def reset_arg(self, options_list=None):
        self.t[:] = 0
        return self._obs()

    def step(self, action):
        self.actions.append(np.array(action, copy=True))
        self.t += 1
        self.k += 1
        terminated, truncated = np.zeros(E, dtype=bool), np.zeros(E, dtype=bool)
        info = [{} for _ in range(E)]
        terminated[0] = self.t[0] == 3
        for e in range(1, E):
            if self.t[e] >= e + 2:
                truncated[e] = True
                fin = np.full((1, 2), 100.0 + self.t[e], dtype=np.float32)
                self.handed_out.append((fin, fin.copy()))
                info[e]["final_obs"] = {"state": fin} if e % 2 else fin
        self.t[terminated | truncated] = 0
        return self._obs(), np.arange(E) + 0.5 * self.k, terminated, truncated, info


class StubModel(torch.nn.Module):
    """forward -> (E, 2, 3) filled with the first state coordinate, + 0.25 when deterministic."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, cond, deterministic=False, **kw):
        self.calls.append((bool(deterministic), self.training, dict(kw)))
        s = cond["state"][:, 0, 0].float() + (0.25 if deterministic else 0.0)
        return s.reshape(-1, 1, 1).expand(-1, 2, 3).contiguous()


class StubOpt:
    def __init__(self):
        self.param_groups = [{"lr": 0.1}]


class StubSched:
    def __init__(self):
        self.n = 0

    def step(self):
        self.n += 1


def bare_agent(cls, **attrs):
    """An agent without ``__init__`` (the only helper allowed to know how the agents are put together)."""
    a = object.__new__(cls)
    for k, v in attrs.items():
        setattr(a, k, v)
    return a


def make(cls, tmp_path, n_ret, **extra):
    np.random.seed(0)
    calls = []
    attrs = dict(device="cpu", n_cond_step=1, obs_dim=2, action_dim=3, act_steps=2, horizon_steps=2, n_envs=E, n_steps=5, n_train_itr=4,
                 val_freq=3, force_train=False, reset_at_iteration=False, batch_size=4, replay_ratio=1.0,
                 replay=DeviceReplay(4, E, 2, 6, "cpu"), scale_reward_factor=0.5, best_reward_threshold_for_success=3, log_freq=1,
                 save_model_freq=100, use_wandb=False, itr=0, venv=ScriptedVecEnv(), model=StubModel(),
                 result_path=str(tmp_path / "result.pkl"), actor_optimizer=StubOpt(), critic_optimizer=StubOpt(),
                 critic_q_optimizer=StubOpt(), critic_v_optimizer=StubOpt(), actor_lr_scheduler=StubSched(),
                 critic_lr_scheduler=StubSched(), critic_q_lr_scheduler=StubSched(), critic_v_lr_scheduler=StubSched(),
                 eval_deterministic=False, num_sample=2, use_expectile_exploration=True)
    attrs.update(extra)
    agent = bare_agent(cls, **attrs)
    agent.save_model = lambda: calls.append(("save", agent.itr))

    def update_minibatch(inds, **kw):
        calls.append(("mb", agent.itr, inds.clone(), kw))
        return tuple(torch.tensor(float(i + 1)) for i in range(n_ret))
    agent.update_minibatch = update_minibatch
    return agent, calls


def check_env_arrays_untouched(venv):
    assert venv.handed_out and all(np.array_equal(a, c) for a, c in venv.handed_out)


# ---- what the hand-copied run() bodies produced (IDQL, QSM and DQL alike) ---------------------------------------------------------
RR_INDS = {1: [[5, 0, 3, 11], [3, 7, 9, 3], [5, 2, 4, 7]], 2: [[6, 8, 8, 10], [1, 6, 7, 7], [8, 1, 5, 9]]}
RR_NEXT_OBS = [[0, 103, 1], [1, 1, 2], [1, 1, 3], [2, 2, 104]]
RR_REWARD = [[3.5, 4, 4.5], [3.75, 4.25, 4.75], [3, 3.5, 4], [3.25, 3.75, 4.25]]
RR_ACTIONS = [[2, 2, 0], [0, 0, 1], [0, 0, 2], [1, 1, 3]]
RR_OBS = [[2, 2, 0], [0, 0, 1], [0, 0, 2], [1, 1, 3]]


def replay_ratio_case(name):
    if name == "idql":
        from dppo_amd.agent.finetune.train_idql_diffusion_agent import TrainIDQLDiffusionAgent as cls
        return cls, 3, 12, dict(loss_actor=3.0, loss_critic=3.0, loss_critic_v=1.0, loss_critic_q=2.0, actor_lr=0.1, critic_lr=0.1)
    if name == "qsm":
        from dppo_amd.agent.finetune.train_qsm_diffusion_agent import TrainQSMDiffusionAgent as cls
    else:
        from dppo_amd.agent.finetune.train_dql_diffusion_agent import TrainDQLDiffusionAgent as cls
    return cls, 2, 8, dict(loss_actor=2.0, loss_critic=1.0, actor_lr=0.1, critic_lr=0.1)


@pytest.mark.parametrize("name", ["idql", "qsm", "dql"])
def test_replay_ratio_run_is_the_recorded_iteration(name, tmp_path):
    cls, n_ret, n_sched, metrics = replay_ratio_case(name)
    agent, calls = make(cls, tmp_path, n_ret)
    res = agent.run()
    # calls in order: save at 0; three minibatches (int(5 * 3 / 4 * 1)) in each of the train iterations 1 and 2; save at 3
    assert [c[:2] for c in calls] == [("save", 0)] + [("mb", 1)] * 3 + [("mb", 2)] * 3 + [("save", 3)]
    mbs = [c for c in calls if c[0] == "mb"]
    assert all(c[3] == {} for c in mbs)
    for itr in (1, 2):
        got = [c[2] for c in mbs if c[1] == itr]
        assert all(g.dtype == torch.int64 for g in got) and [g.tolist() for g in got] == RR_INDS[itr]
    scheds = [v for k, v in vars(agent).items() if k.endswith("_lr_scheduler")]
    used = [s.n for s in scheds if s.n]
    assert sum(used) == n_sched and set(used) == {4}
    # records
    assert agent.itr == 4 and [r["itr"] for r in res] == [0, 1, 2, 3] and [r["step"] for r in res] == [0, 30, 60, 60]
    assert all("time" in r for r in res)
    ev = lambda r: (r["eval_success_rate"], r["eval_episode_reward"], r["eval_best_reward"])
    np.testing.assert_allclose(ev(res[0]), (0.0, 22 / 3, 4 / 3), rtol=1e-12)
    np.testing.assert_allclose(ev(res[3]), (1.0, 97 / 3, 61 / 12), rtol=1e-12)
    assert set(res[0]) == set(res[3]) == {"itr", "step", "time", "eval_success_rate", "eval_episode_reward", "eval_best_reward"}
    np.testing.assert_allclose([res[1]["train_episode_reward"], res[2]["train_episode_reward"]], [47 / 3, 21.0], rtol=1e-12)
    for r in res[1:3]:
        assert set(r) == {"itr", "step", "time", "train_episode_reward"} | set(metrics)
        assert {k: r[k] for k in metrics} == metrics
    with open(agent.result_path, "rb") as f:
        on_disk = pickle.load(f)
    assert on_disk == res and len(on_disk) == 4
    # the sampler: train mode / eval mode of the module, deterministic flag, the subclass's keywords
    m = agent.model
    assert len(m.calls) == 20 and [c[1] for c in m.calls] == [False] * 5 + [True] * 10 + [False] * 5
    if name == "idql":
        assert all(c[0] is False and c[2] == {"num_sample": 2, "use_expectile_exploration": True} for c in m.calls)
    else:
        assert [c[0] for c in m.calls] == [True] * 5 + [False] * 10 + [True] * 5 and all(c[2] == {} for c in m.calls)
    # the env saw the first act_steps of the sample; eval iterations reset
    assert len(agent.venv.actions) == 20 and all(a.shape == (E, 2, 3) for a in agent.venv.actions)
    # the ring: 10 appends into 4 slots
    rp = agent.replay
    assert rp.steps == 4 and rp.head == 2
    assert rp.next_obs[:, :, 0].tolist() == RR_NEXT_OBS and torch.equal(rp.next_obs[:, :, 0], rp.next_obs[:, :, 1])
    assert rp.obs[:, :, 0].tolist() == RR_OBS
    term = torch.zeros(4, E)
    term[0, 0] = 1
    assert torch.equal(rp.terminated, term) and rp.terminated.dtype == torch.float32
    assert rp.reward.tolist() == RR_REWARD
    assert rp.actions[:, :, 0].tolist() == RR_ACTIONS and torch.equal(rp.actions, rp.actions[:, :, :1].expand(-1, -1, 6))
    check_env_arrays_untouched(agent.venv)


def test_idql_eval_deterministic_reaches_the_sampler_in_eval_only(tmp_path):
    cls, n_ret, _, _ = replay_ratio_case("idql")
    agent, _ = make(cls, tmp_path, n_ret, eval_deterministic=True)
    agent.run()
    assert [c[0] for c in agent.model.calls] == [True] * 5 + [False] * 10 + [True] * 5


def test_replay_ratio_run_resets_every_iteration_when_asked(tmp_path):
    """reset_at_iteration: every iteration starts from a reset, so every iteration sees the same episodes."""
    cls, n_ret, _, _ = replay_ratio_case("qsm")
    agent, _ = make(cls, tmp_path, n_ret, reset_at_iteration=True, force_train=True, n_train_itr=2)
    res = agent.run()
    assert [r["step"] for r in res] == [30, 60] and all("eval_success_rate" not in r for r in res)
    assert agent.replay.obs[:, :, 0].tolist() == [[0, 0, 3], [1, 1, 0], [1, 1, 1], [2, 2, 2]]
    assert agent.replay.next_obs[:, :, 0].tolist() == [[1, 1, 104], [2, 2, 1], [2, 2, 2], [0, 103, 3]]


# ---- SAC -------------------------------------------------------------------------------------------------------------------------
SAC_INDS = {2: [5, 1, 4, 9], 4: [4, 5, 0, 1], 5: [5, 7, 9, 1]}
SAC_NEXT_OBS = [[1, 1, 1], [1, 1, 2], [2, 2, 3], [0, 103, 104]]
SAC_OBS = [[0, 0, 0], [0, 0, 1], [1, 1, 2], [2, 2, 3]]
SAC_REWARD = [[7, 7.5, 8], [6.25, 6.75, 7.25], [6.5, 7, 7.5], [6.75, 7.25, 7.75]]
SAC_STEPS = [30, 60, 90, 90, 120, 150]
SAC_EVAL = (1.0, 27.0, 4.75)
SAC_TRAIN_REWARD = (22.5, 38.0, 140 / 3)


def test_sac_run_is_the_recorded_iteration(tmp_path):
    from dppo_amd.agent.finetune.train_sac_agent import TrainSACAgent
    agent, calls = make(TrainSACAgent, tmp_path, 3, n_explore_steps=1, n_eval_episode=2, n_train_itr=6, critic_update_freq=1,
                        actor_update_freq=2, log_alpha=torch.tensor(np.log(0.5), dtype=torch.float64))
    res = agent.run()
    # exploration in iteration 0 only (5 uniform draws, no model call); evaluation in iteration 3, ended by its episode count
    m, venv = agent.model, agent.venv
    explore = venv.actions[:5]
    assert all(a.dtype == np.float32 and a.shape == (E, 2, 3) and np.abs(a).max() <= 1.0 for a in explore)
    np.testing.assert_allclose(explore[0][0, 0], [0.09762701, 0.43037874, 0.20552675], rtol=1e-6)
    n_eval = len(venv.actions) - 25
    assert n_eval == 3 and len(m.calls) == 20 + n_eval
    assert [c[0] for c in m.calls] == [False] * 10 + [True] * n_eval + [False] * 10
    # updates: past the exploration phase, not in the evaluation; the actor every second iteration
    assert [c[:2] for c in calls] == [("save", 0), ("mb", 2), ("mb", 4), ("mb", 5), ("save", 5)]
    mbs = [c for c in calls if c[0] == "mb"]
    assert [c[3] for c in mbs] == [{"update_actor": True}, {"update_actor": True}, {"update_actor": False}]
    assert {c[1]: c[2].tolist() for c in mbs} == SAC_INDS and all(c[2].dtype == torch.int64 for c in mbs)
    # a record every iteration; time and what follows it only past the exploration phase
    assert agent.itr == 6 and [r["itr"] for r in res] == list(range(6)) and [r["step"] for r in res] == SAC_STEPS
    assert set(res[0]) == set(res[1]) == {"itr", "step"}
    assert set(res[3]) == {"itr", "step", "time", "eval_success_rate", "eval_episode_reward", "eval_best_reward"}
    np.testing.assert_allclose([res[3][k] for k in ("eval_success_rate", "eval_episode_reward", "eval_best_reward")],
                               SAC_EVAL, rtol=1e-12)
    for i in (2, 4, 5):
        assert set(res[i]) == {"itr", "step", "time", "train_episode_reward", "loss_critic", "alpha", "loss_actor"}
        assert res[i]["loss_critic"] == 1.0 and res[i]["loss_actor"] == 2.0 and res[i]["alpha"] == pytest.approx(0.5, rel=1e-15)
    np.testing.assert_allclose([res[i]["train_episode_reward"] for i in (2, 4, 5)], SAC_TRAIN_REWARD, rtol=1e-12)
    with open(agent.result_path, "rb") as f:
        assert pickle.load(f) == res
    rp = agent.replay
    assert rp.steps == 4 and rp.head == 1  # 25 appends into 4 slots
    assert rp.next_obs[:, :, 0].tolist() == SAC_NEXT_OBS and rp.obs[:, :, 0].tolist() == SAC_OBS
    assert rp.reward.tolist() == SAC_REWARD and rp.actions[:, :, 0].tolist() == SAC_OBS
    term = torch.zeros(4, E)
    term[3, 0] = 1
    assert torch.equal(rp.terminated, term)
    check_env_arrays_untouched(venv)



def test_sac_actor_loss_is_logged_only_after_an_actor_update(tmp_path):
    """The first update of this run skips the actor (actor_update_freq 3, first update at iteration 2): no loss_actor yet."""
    from dppo_amd.agent.finetune.train_sac_agent import TrainSACAgent
    agent, calls = make(TrainSACAgent, tmp_path, 3, n_explore_steps=1, n_eval_episode=2, n_train_itr=4, val_freq=100,
                        critic_update_freq=2, actor_update_freq=3, log_alpha=torch.tensor(0.0, dtype=torch.float64))

    def update_minibatch(inds, update_actor=True):
        calls.append(("mb", agent.itr, update_actor))
        return torch.tensor(1.0), (torch.tensor(2.0) if update_actor else None), None
    agent.update_minibatch = update_minibatch
    res = agent.run()
    assert [c for c in calls if c[0] == "mb"] == [("mb", 2, False)]
    assert "time" not in res[1] and set(res[2]) == set(res[3]) == {"itr", "step", "time", "train_episode_reward", "loss_critic", "alpha"}


# ---- the model helpers, as far as they go without a device -------------------------------------------------------------------------
def test_as_batch_refuses_cpu_tensors_and_describes_the_ring():
    from dppo_amd.model.common import off_policy
    obs = {"state": torch.zeros(5, 1, 2)}
    with pytest.raises(hip.DppoHipError, match="cpu"):
        off_policy.as_batch("QSM", obs, actions=torch.zeros(5, 2, 3))
    with pytest.raises(NotImplementedError, match="QSM is built for state observations only"):
        off_policy.as_batch("QSM", {"state": torch.zeros(5, 1, 2), "rgb": torch.zeros(5, 3, 4, 4)})
    rp = DeviceReplay(4, E, 2, 6, "cpu")
    for i in range(6):  # 6 appends into 4 slots: head 2
        rp.append(torch.full((E, 2), float(i)), torch.zeros(E, 2), torch.zeros(E, 6), np.zeros(E), np.zeros(E, dtype=np.float32))
    b, N, keep = off_policy.as_batch("QSM", rp)
    assert N == 12 and keep == (None,) and not b.inds
    assert (b.cap, b.n_envs, b.head, b.count) == (4, E, 2, 4) and b.obs == rp.obs.data_ptr() and b.next_obs == rp.next_obs.data_ptr()
    with pytest.raises(AssertionError):  # the index vector lives on the device
        off_policy.as_batch("QSM", rp, torch.tensor([0, 5, 7]))
    with pytest.raises(AssertionError):
        off_policy.as_batch("QSM", rp, torch.tensor([0, 5, 7], dtype=torch.int32))
    # the rows of a minibatch: one gather in the ring's logical order
    inds = torch.tensor([0, 5, 7, 11])
    assert torch.equal(off_policy.rows_of("QSM", rp, inds), rp.gather(inds)[0])
    assert torch.equal(off_policy.rows_of("QSM", rp, inds, nxt=True), rp.gather(inds)[1])
    assert torch.equal(off_policy.rows_of("QSM", rp, None), rp.gather(torch.arange(12))[0])
    assert off_policy.rows_of("QSM", obs, None) is obs["state"]


def test_flat_views_are_the_split_of_the_flat_gradient():
    from dppo_amd.model.diffusion.diffusion import flat_views
    params = [torch.zeros(3, 5), torch.zeros(5), torch.zeros(2, 1, 4), torch.zeros(())]
    grad = torch.arange(29, dtype=torch.float32)
    views = flat_views(grad, params)
    want = torch.split(grad, [p.numel() for p in params])
    assert len(views) == 4 and all(v.shape == p.shape and torch.equal(v.reshape(-1), w) for v, p, w in zip(views, params, want))
    assert all(v.data_ptr() == w.data_ptr() for v, w in zip(views, want))  # views, not copies


def test_workspace_get_raises_on_a_failed_size_query(monkeypatch):
    class Lib:
        @staticmethod
        def dppo_last_error():
            return b"N out of range"
    monkeypatch.setattr(hip, "load", lambda: Lib)
    with pytest.raises(hip.DppoHipError, match=r"^x_workspace_bytes failed \(rc=-1\): N out of range$"):
        hip.Workspace().get(-1, "cpu", "x_workspace_bytes")
    ws = hip.Workspace()
    buf = ws.get(300, "cpu", "x_workspace_bytes")
    assert buf.numel() == 300 and ws.get(10, "cpu") is buf
