"""The host loop of the four PPO fine-tuning agents on the CPU, after the pattern of tests/test_off_policy_agent.py: a scripted vector
env, a stub model, recorders in place of the update and of ``save_model`` (``gae_device`` and ``FlatAdamW`` need a device, so the
update itself is not run and the agents are made without ``__init__``).  ``observe`` runs one agent and turns everything the loop
did into plain lists.  Every constant below was recorded by running ``observe`` / ``observe_eval`` of this file against the two
hand-copied ``run()`` bodies (state and pixels) and the ``EvalAgent.run`` that stood before ``TrainAgent``; the one loop has to
reproduce them.  Nothing here was generated from the code that is under test now.

The run: 5 steps, 5 iterations, ``val_freq`` 3 (evaluation at 0 and 3, training at 1, 2 and 4, so that iteration 2 follows a
training iteration and ``reset_at_iteration: False`` carries ``done`` over), ``n_critic_warmup_itr`` 2."""
import pickle

import numpy as np
import pytest
import torch

from dppo_amd.model.diffusion.diffusion import Sample
from dppo_amd.util.rollout import GroupedVecEnv

E, S, TA, DA, ACT, KFT = 3, 5, 4, 3, 2, 2


class ScriptedVecEnv:
    """``n_envs`` envs whose observation is their own step counter (``state`` float32 (1, 2); with ``rgb`` also a uint8 (3, 4, 4)
    image of it).  Env 0 terminates at t == 3; env e > 0 truncates at t >= e + 2 + ``late``.  Reward: arange(E) + 0.5 k with k the
    number of ``step`` calls.  Observations come back as a list of dicts."""
    n_envs = E

    def __init__(self, rgb=False, late=0):
        self.t, self.k, self.rgb, self.late = np.zeros(E, dtype=np.int64), 0, rgb, late
        self.actions, self.resets = [], []

    def seed(self, seeds):
        pass

    def _obs(self):
        out = [{"state": np.full((1, 2), float(self.t[e]), dtype=np.float32)} for e in range(E)]
        if self.rgb:
            for e, o in enumerate(out):
                o["rgb"] = np.full((3, 4, 4), self.t[e], dtype=np.uint8)
        return out

    def reset_arg(self, options_list=None):
        self.resets.append(self.k)
        self.t[:] = 0
        return self._obs()

    def step(self, action):
        self.actions.append(np.array(action, copy=True))
        self.t += 1
        self.k += 1
        terminated, truncated = np.zeros(E, dtype=bool), np.zeros(E, dtype=bool)
        terminated[0] = self.t[0] == 3
        for e in range(1, E):
            truncated[e] = self.t[e] >= e + 2 + self.late
        self.t[terminated | truncated] = 0
        return self._obs(), np.arange(E) + 0.5 * self.k, terminated, truncated, [{} for _ in range(E)]


class StubModel(torch.nn.Module):
    """The action chunk (n, TA, DA) is the row's step counter + its image's value / 2 + 0.25 when deterministic + h / 16 at horizon
    step h.  ``chain``: returns a ``Sample`` whose chain entry k is the chunk - (KFT - k); otherwise the chunk."""
    horizon_steps = TA

    def __init__(self, chain):
        super().__init__()
        self.chain, self.calls, self.n_step, self.n_health = chain, [], 0, 0
        if chain:
            self.ft_denoising_steps = KFT

    def forward(self, cond, deterministic=False, return_chain=False):
        a = cond["state"][:, 0, 0].float() + (0.25 if deterministic else 0.0)
        if "rgb" in cond:
            assert cond["rgb"].dtype == torch.uint8
            a = a + cond["rgb"][:, 0, 0, 0].float() / 2
        self.calls.append((bool(deterministic), self.training, a.shape[0]))
        a = (a.reshape(-1, 1, 1) + torch.arange(TA).reshape(1, TA, 1) / 16).expand(-1, TA, DA).contiguous()
        if not self.chain:
            return a
        return Sample(a, torch.stack([a - (KFT - k) for k in range(KFT + 1)], dim=1))

    def step(self):
        self.n_step += 1

    def check_sampler_health(self):
        self.n_health += 1


class StubSched:
    def __init__(self):
        self.at = []

    def step(self):
        self.at.append(self.agent.itr)


class StubWandb:
    def __init__(self):
        self.logged = []

    def log(self, fields, step):
        self.logged.append((step, sorted(k for k in fields if k != "time")))


def agent_class(pixels, chain):
    if pixels and chain:
        from dppo_amd.agent.finetune.train_ppo_diffusion_img_agent import TrainPPOImgDiffusionAgent as cls
    elif pixels:
        from dppo_amd.agent.finetune.train_ppo_gaussian_img_agent import TrainPPOImgGaussianAgent as cls
    elif chain:
        from dppo_amd.agent.finetune.train_ppo_diffusion_agent import TrainPPODiffusionAgent as cls
    else:
        from dppo_amd.agent.finetune.train_ppo_gaussian_agent import TrainPPOGaussianAgent as cls
    return cls


def observe(tmp_path, pixels, chain, reset, groups=1, wandb=None):
    """Run one agent's loop and return what it did, as plain lists."""
    envs = [ScriptedVecEnv(rgb=pixels, late=g) for g in range(groups)]
    venv = envs[0] if groups == 1 else GroupedVecEnv(envs)
    n_envs = E * groups
    agent = object.__new__(agent_class(pixels, chain))  # no __init__: FlatAdamW and the models need a device
    attrs = dict(device="cpu", world=1, rank=0, n_cond_step=1, obs_dim=2, action_dim=DA, act_steps=ACT, horizon_steps=TA,
                 n_envs=n_envs, n_steps=S, n_train_itr=5, val_freq=3, force_train=False, reset_at_iteration=reset,
                 n_critic_warmup_itr=2, best_reward_threshold_for_success=3, log_freq=1, save_model_freq=2,
                 use_wandb=wandb is not None, _wandb=wandb, itr=0, venv=venv, model=StubModel(chain),
                 result_path=str(tmp_path / "result.pkl"), actor_lr_scheduler=StubSched(), critic_lr_scheduler=StubSched(),
                 obs_dims={"rgb": [3, 4, 4], "state": [2]})
    for k, v in attrs.items():
        setattr(agent, k, v)
    agent.actor_lr_scheduler.agent = agent.critic_lr_scheduler.agent = agent
    saves, updates = [], []
    agent.save_model = lambda: saves.append(agent.itr)

    def update(*args):
        """Whatever the hook's signature: the first two arguments are the observation buffer(s) and the chain buffer, the numpy
        arrays are reward, terminated and firsts in that order, and the dict of numpy arrays is the last observation."""
        obs, chains = args[0], args[1]
        reward, terminated, firsts = [a for a in args if isinstance(a, np.ndarray)]
        last = [a for a in args if isinstance(a, dict) and isinstance(a["state"], np.ndarray)][0]
        state = obs["state"] if isinstance(obs, dict) else obs
        assert state.dtype == torch.float32 and chains.dtype == torch.float32
        assert chains.shape == (S * n_envs, (KFT if chain else 0) + 1, TA * DA)
        assert torch.equal(chains, chains[:, :, :1].expand_as(chains) + (torch.arange(TA * DA) // DA / 16))
        u = {"itr": agent.itr, "firsts": ["".join(str(int(x)) for x in row) for row in firsts],
             "terminated": ["".join(str(int(x)) for x in row) for row in terminated], "reward": reward.tolist(),
             "obs": state.reshape(S * n_envs, -1)[:, 0].tolist(), "chain0": chains[:, 0, 0].tolist(),
             "chain_last": chains[:, -1, 0].tolist(), "last": last["state"][:, 0, 0].tolist()}
        assert state.reshape(S * n_envs, -1).shape[1] == 2
        if pixels:
            assert obs["rgb"].dtype == torch.uint8 and obs["rgb"].shape == (S * n_envs, 3, 4, 4) and last["rgb"].dtype == np.uint8
            u["rgb"] = obs["rgb"][:, 0, 0, 0].tolist()
            assert torch.equal(obs["rgb"], obs["rgb"][:, :1, :1, :1].expand_as(obs["rgb"]))
        updates.append(u)
        return {"loss": 1.5, "pg_loss": 0.5, "v_loss": 2.0, "approx_kl": 0.01 * agent.itr}
    agent._update = agent._update_img = update  # (_update_img: the pixel loop's hook in the code the constants were recorded from)
    res = agent.run()
    with open(agent.result_path, "rb") as f:
        assert pickle.load(f) == res
    assert all("time" in r for r in res)
    m = agent.model
    acts = [a for env in envs for a in env.actions]
    assert all(a.shape == (E, ACT, DA) and np.array_equal(a, a[:, :, :1].repeat(DA, axis=2)) for a in acts)
    assert all(np.allclose(a[:, 1, 0] - a[:, 0, 0], 1 / 16) for a in acts)  # the first ACT steps of the TA-step trajectory
    return {"updates": updates, "saves": saves, "records": [{k: v for k, v in r.items() if k != "time"} for r in res],
            "record_keys": [list(r) for r in res], "itr": agent.itr, "resets": [env.resets for env in envs],
            "actions": [[a[:, 0, 0].tolist() for a in env.actions] for env in envs],
            "actor_sched": agent.actor_lr_scheduler.at, "critic_sched": agent.critic_lr_scheduler.at,
            "model_calls": sorted(set(m.calls), key=m.calls.index), "n_model_calls": len(m.calls), "model_steps": m.n_step,
            "health_checks": m.n_health}


# ---- what the two hand-copied run() bodies produced ---------------------------------------------------------------------------------
# (chain and one-shot sample alike, but for the chain's first entry; keyed by (pixels, reset_at_iteration): the pixel stub adds half
# the image's value to the action)
RECORDED = {
    (False, False): {
        'actions': [[[0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 0.25, 3.25], [1.25, 1.25, 0.25], [0.0, 0.0,
          0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 0.0], [2.0, 2.0, 1.0], [0.0, 0.0, 2.0], [1.0, 1.0,
          3.0], [2.0, 2.0, 0.0], [0.0, 0.0, 1.0], [0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 0.25, 3.25],
          [1.25, 1.25, 0.25], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 0.0]]],
        'actor_sched': [2, 3, 4],
        'critic_sched': [0, 1, 2, 3, 4],
        'health_checks': 5,
        'itr': 5,
        'model_calls': [(True, False, 3), (False, True, 3)],
        'model_steps': 5,
        'n_model_calls': 25,
        'record_keys': [['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward', 'eval_best_reward'], ['itr', 'step',
          'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'train_episode_reward',
          'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward',
          'eval_best_reward'], ['itr', 'step', 'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl']],
        'records': [{'eval_best_reward': 1.3333333333333333, 'eval_episode_reward': 7.333333333333333, 'eval_success_rate': 0.0,
          'itr': 0, 'step': 0}, {'approx_kl': 0.01, 'itr': 1, 'loss': 1.5, 'pg_loss': 0.5, 'step': 30, 'train_episode_reward':
          15.666666666666666, 'v_loss': 2.0}, {'approx_kl': 0.02, 'itr': 2, 'loss': 1.5, 'pg_loss': 0.5, 'step': 60,
          'train_episode_reward': 21.0, 'v_loss': 2.0}, {'eval_best_reward': 5.083333333333333, 'eval_episode_reward':
          32.333333333333336, 'eval_success_rate': 1.0, 'itr': 3, 'step': 60}, {'approx_kl': 0.04, 'itr': 4, 'loss': 1.5, 'pg_loss':
          0.5, 'step': 90, 'train_episode_reward': 40.666666666666664, 'v_loss': 2.0}],
        'resets': [[0, 5, 15, 20]],
        'saves': [0, 2, 4],
        'updates': [
            {'chain_last': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'firsts': ['111', '000',
             '000', '110', '001', '000'], 'itr': 1, 'last': [2.0, 2.0, 1.0], 'obs': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0,
             0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'reward': [[3.0, 4.0, 5.0], [3.5, 4.5, 5.5], [4.0, 5.0, 6.0], [4.5, 5.5, 6.5], [5.0,
             6.0, 7.0]], 'terminated': ['000', '000', '100', '000', '000']},
            {'chain_last': [2.0, 2.0, 1.0, 0.0, 0.0, 2.0, 1.0, 1.0, 3.0, 2.0, 2.0, 0.0, 0.0, 0.0, 1.0], 'firsts': ['000', '110',
             '000', '001', '110', '000'], 'itr': 2, 'last': [1.0, 1.0, 2.0], 'obs': [2.0, 2.0, 1.0, 0.0, 0.0, 2.0, 1.0, 1.0, 3.0,
             2.0, 2.0, 0.0, 0.0, 0.0, 1.0], 'reward': [[5.5, 6.5, 7.5], [6.0, 7.0, 8.0], [6.5, 7.5, 8.5], [7.0, 8.0, 9.0], [7.5,
             8.5, 9.5]], 'terminated': ['100', '000', '000', '100', '000']},
            {'chain_last': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'firsts': ['111', '000',
             '000', '110', '001', '000'], 'itr': 4, 'last': [2.0, 2.0, 1.0], 'obs': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0,
             0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'reward': [[10.5, 11.5, 12.5], [11.0, 12.0, 13.0], [11.5, 12.5, 13.5], [12.0, 13.0,
             14.0], [12.5, 13.5, 14.5]], 'terminated': ['000', '000', '100', '000', '000']},
        ],
    },
    (False, True): {
        'actions': [[[0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 0.25, 3.25], [1.25, 1.25, 0.25], [0.0, 0.0,
          0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0,
          2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 0.0], [0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 0.25, 3.25],
          [1.25, 1.25, 0.25], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 0.0]]],
        'actor_sched': [2, 3, 4],
        'critic_sched': [0, 1, 2, 3, 4],
        'health_checks': 5,
        'itr': 5,
        'model_calls': [(True, False, 3), (False, True, 3)],
        'model_steps': 5,
        'n_model_calls': 25,
        'record_keys': [['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward', 'eval_best_reward'], ['itr', 'step',
          'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'train_episode_reward',
          'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward',
          'eval_best_reward'], ['itr', 'step', 'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl']],
        'records': [{'eval_best_reward': 1.3333333333333333, 'eval_episode_reward': 7.333333333333333, 'eval_success_rate': 0.0,
          'itr': 0, 'step': 0}, {'approx_kl': 0.01, 'itr': 1, 'loss': 1.5, 'pg_loss': 0.5, 'step': 30, 'train_episode_reward':
          15.666666666666666, 'v_loss': 2.0}, {'approx_kl': 0.02, 'itr': 2, 'loss': 1.5, 'pg_loss': 0.5, 'step': 60,
          'train_episode_reward': 24.0, 'v_loss': 2.0}, {'eval_best_reward': 5.083333333333333, 'eval_episode_reward':
          32.333333333333336, 'eval_success_rate': 1.0, 'itr': 3, 'step': 60}, {'approx_kl': 0.04, 'itr': 4, 'loss': 1.5, 'pg_loss':
          0.5, 'step': 90, 'train_episode_reward': 40.666666666666664, 'v_loss': 2.0}],
        'resets': [[0, 5, 10, 15, 20]],
        'saves': [0, 2, 4],
        'updates': [
            {'chain_last': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'firsts': ['111', '000',
             '000', '110', '001', '000'], 'itr': 1, 'last': [2.0, 2.0, 1.0], 'obs': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0,
             0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'reward': [[3.0, 4.0, 5.0], [3.5, 4.5, 5.5], [4.0, 5.0, 6.0], [4.5, 5.5, 6.5], [5.0,
             6.0, 7.0]], 'terminated': ['000', '000', '100', '000', '000']},
            {'chain_last': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'firsts': ['111', '000',
             '000', '110', '001', '000'], 'itr': 2, 'last': [2.0, 2.0, 1.0], 'obs': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0,
             0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'reward': [[5.5, 6.5, 7.5], [6.0, 7.0, 8.0], [6.5, 7.5, 8.5], [7.0, 8.0, 9.0], [7.5,
             8.5, 9.5]], 'terminated': ['000', '000', '100', '000', '000']},
            {'chain_last': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'firsts': ['111', '000',
             '000', '110', '001', '000'], 'itr': 4, 'last': [2.0, 2.0, 1.0], 'obs': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0,
             0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'reward': [[10.5, 11.5, 12.5], [11.0, 12.0, 13.0], [11.5, 12.5, 13.5], [12.0, 13.0,
             14.0], [12.5, 13.5, 14.5]], 'terminated': ['000', '000', '100', '000', '000']},
        ],
    },
    (True, False): {
        'actions': [[[0.25, 0.25, 0.25], [1.75, 1.75, 1.75], [3.25, 3.25, 3.25], [0.25, 0.25, 4.75], [1.75, 1.75, 0.25], [0.0, 0.0,
          0.0], [1.5, 1.5, 1.5], [3.0, 3.0, 3.0], [0.0, 0.0, 4.5], [1.5, 1.5, 0.0], [3.0, 3.0, 1.5], [0.0, 0.0, 3.0], [1.5, 1.5,
          4.5], [3.0, 3.0, 0.0], [0.0, 0.0, 1.5], [0.25, 0.25, 0.25], [1.75, 1.75, 1.75], [3.25, 3.25, 3.25], [0.25, 0.25, 4.75],
          [1.75, 1.75, 0.25], [0.0, 0.0, 0.0], [1.5, 1.5, 1.5], [3.0, 3.0, 3.0], [0.0, 0.0, 4.5], [1.5, 1.5, 0.0]]],
        'actor_sched': [2, 3, 4],
        'critic_sched': [0, 1, 2, 3, 4],
        'health_checks': 0,
        'itr': 5,
        'model_calls': [(True, False, 3), (False, True, 3)],
        'model_steps': 5,
        'n_model_calls': 25,
        'record_keys': [['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward', 'eval_best_reward'], ['itr', 'step',
          'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'train_episode_reward',
          'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward',
          'eval_best_reward'], ['itr', 'step', 'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl']],
        'records': [{'eval_best_reward': 1.3333333333333333, 'eval_episode_reward': 7.333333333333333, 'eval_success_rate': 0.0,
          'itr': 0, 'step': 0}, {'approx_kl': 0.01, 'itr': 1, 'loss': 1.5, 'pg_loss': 0.5, 'step': 30, 'train_episode_reward':
          15.666666666666666, 'v_loss': 2.0}, {'approx_kl': 0.02, 'itr': 2, 'loss': 1.5, 'pg_loss': 0.5, 'step': 60,
          'train_episode_reward': 21.0, 'v_loss': 2.0}, {'eval_best_reward': 5.083333333333333, 'eval_episode_reward':
          32.333333333333336, 'eval_success_rate': 1.0, 'itr': 3, 'step': 60}, {'approx_kl': 0.04, 'itr': 4, 'loss': 1.5, 'pg_loss':
          0.5, 'step': 90, 'train_episode_reward': 40.666666666666664, 'v_loss': 2.0}],
        'resets': [[0, 5, 15, 20]],
        'saves': [0, 2, 4],
        'updates': [
            {'chain_last': [0.0, 0.0, 0.0, 1.5, 1.5, 1.5, 3.0, 3.0, 3.0, 0.0, 0.0, 4.5, 1.5, 1.5, 0.0], 'firsts': ['111', '000',
             '000', '110', '001', '000'], 'itr': 1, 'last': [2.0, 2.0, 1.0], 'obs': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0,
             0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'reward': [[3.0, 4.0, 5.0], [3.5, 4.5, 5.5], [4.0, 5.0, 6.0], [4.5, 5.5, 6.5], [5.0,
             6.0, 7.0]], 'terminated': ['000', '000', '100', '000', '000']},
            {'chain_last': [3.0, 3.0, 1.5, 0.0, 0.0, 3.0, 1.5, 1.5, 4.5, 3.0, 3.0, 0.0, 0.0, 0.0, 1.5], 'firsts': ['000', '110',
             '000', '001', '110', '000'], 'itr': 2, 'last': [1.0, 1.0, 2.0], 'obs': [2.0, 2.0, 1.0, 0.0, 0.0, 2.0, 1.0, 1.0, 3.0,
             2.0, 2.0, 0.0, 0.0, 0.0, 1.0], 'reward': [[5.5, 6.5, 7.5], [6.0, 7.0, 8.0], [6.5, 7.5, 8.5], [7.0, 8.0, 9.0], [7.5,
             8.5, 9.5]], 'terminated': ['100', '000', '000', '100', '000']},
            {'chain_last': [0.0, 0.0, 0.0, 1.5, 1.5, 1.5, 3.0, 3.0, 3.0, 0.0, 0.0, 4.5, 1.5, 1.5, 0.0], 'firsts': ['111', '000',
             '000', '110', '001', '000'], 'itr': 4, 'last': [2.0, 2.0, 1.0], 'obs': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0,
             0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'reward': [[10.5, 11.5, 12.5], [11.0, 12.0, 13.0], [11.5, 12.5, 13.5], [12.0, 13.0,
             14.0], [12.5, 13.5, 14.5]], 'terminated': ['000', '000', '100', '000', '000']},
        ],
    },
    (True, True): {
        'actions': [[[0.25, 0.25, 0.25], [1.75, 1.75, 1.75], [3.25, 3.25, 3.25], [0.25, 0.25, 4.75], [1.75, 1.75, 0.25], [0.0, 0.0,
          0.0], [1.5, 1.5, 1.5], [3.0, 3.0, 3.0], [0.0, 0.0, 4.5], [1.5, 1.5, 0.0], [0.0, 0.0, 0.0], [1.5, 1.5, 1.5], [3.0, 3.0,
          3.0], [0.0, 0.0, 4.5], [1.5, 1.5, 0.0], [0.25, 0.25, 0.25], [1.75, 1.75, 1.75], [3.25, 3.25, 3.25], [0.25, 0.25, 4.75],
          [1.75, 1.75, 0.25], [0.0, 0.0, 0.0], [1.5, 1.5, 1.5], [3.0, 3.0, 3.0], [0.0, 0.0, 4.5], [1.5, 1.5, 0.0]]],
        'actor_sched': [2, 3, 4],
        'critic_sched': [0, 1, 2, 3, 4],
        'health_checks': 0,
        'itr': 5,
        'model_calls': [(True, False, 3), (False, True, 3)],
        'model_steps': 5,
        'n_model_calls': 25,
        'record_keys': [['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward', 'eval_best_reward'], ['itr', 'step',
          'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'train_episode_reward',
          'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward',
          'eval_best_reward'], ['itr', 'step', 'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl']],
        'records': [{'eval_best_reward': 1.3333333333333333, 'eval_episode_reward': 7.333333333333333, 'eval_success_rate': 0.0,
          'itr': 0, 'step': 0}, {'approx_kl': 0.01, 'itr': 1, 'loss': 1.5, 'pg_loss': 0.5, 'step': 30, 'train_episode_reward':
          15.666666666666666, 'v_loss': 2.0}, {'approx_kl': 0.02, 'itr': 2, 'loss': 1.5, 'pg_loss': 0.5, 'step': 60,
          'train_episode_reward': 24.0, 'v_loss': 2.0}, {'eval_best_reward': 5.083333333333333, 'eval_episode_reward':
          32.333333333333336, 'eval_success_rate': 1.0, 'itr': 3, 'step': 60}, {'approx_kl': 0.04, 'itr': 4, 'loss': 1.5, 'pg_loss':
          0.5, 'step': 90, 'train_episode_reward': 40.666666666666664, 'v_loss': 2.0}],
        'resets': [[0, 5, 10, 15, 20]],
        'saves': [0, 2, 4],
        'updates': [
            {'chain_last': [0.0, 0.0, 0.0, 1.5, 1.5, 1.5, 3.0, 3.0, 3.0, 0.0, 0.0, 4.5, 1.5, 1.5, 0.0], 'firsts': ['111', '000',
             '000', '110', '001', '000'], 'itr': 1, 'last': [2.0, 2.0, 1.0], 'obs': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0,
             0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'reward': [[3.0, 4.0, 5.0], [3.5, 4.5, 5.5], [4.0, 5.0, 6.0], [4.5, 5.5, 6.5], [5.0,
             6.0, 7.0]], 'terminated': ['000', '000', '100', '000', '000']},
            {'chain_last': [0.0, 0.0, 0.0, 1.5, 1.5, 1.5, 3.0, 3.0, 3.0, 0.0, 0.0, 4.5, 1.5, 1.5, 0.0], 'firsts': ['111', '000',
             '000', '110', '001', '000'], 'itr': 2, 'last': [2.0, 2.0, 1.0], 'obs': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0,
             0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'reward': [[5.5, 6.5, 7.5], [6.0, 7.0, 8.0], [6.5, 7.5, 8.5], [7.0, 8.0, 9.0], [7.5,
             8.5, 9.5]], 'terminated': ['000', '000', '100', '000', '000']},
            {'chain_last': [0.0, 0.0, 0.0, 1.5, 1.5, 1.5, 3.0, 3.0, 3.0, 0.0, 0.0, 4.5, 1.5, 1.5, 0.0], 'firsts': ['111', '000',
             '000', '110', '001', '000'], 'itr': 4, 'last': [2.0, 2.0, 1.0], 'obs': [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0,
             0.0, 0.0, 3.0, 1.0, 1.0, 0.0], 'reward': [[10.5, 11.5, 12.5], [11.0, 12.0, 13.0], [11.5, 12.5, 13.5], [12.0, 13.0,
             14.0], [12.5, 13.5, 14.5]], 'terminated': ['000', '000', '100', '000', '000']},
        ],
    },
}
RECORDED_GROUPED = {
    False: {
        'actions': [[[0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 0.25, 3.25], [1.25, 1.25, 0.25], [0.0, 0.0,
          0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 0.0], [2.0, 2.0, 1.0], [0.0, 0.0, 2.0], [1.0, 1.0,
          3.0], [2.0, 2.0, 0.0], [0.0, 0.0, 1.0], [0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 0.25, 3.25],
          [1.25, 1.25, 0.25], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 0.0]], [[0.25, 0.25,
          0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 3.25, 3.25], [1.25, 0.25, 4.25], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0],
          [2.0, 2.0, 2.0], [0.0, 3.0, 3.0], [1.0, 0.0, 4.0], [2.0, 1.0, 0.0], [0.0, 2.0, 1.0], [1.0, 3.0, 2.0], [2.0, 0.0, 3.0],
          [0.0, 1.0, 4.0], [0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 3.25, 3.25], [1.25, 0.25, 4.25], [0.0,
          0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 3.0, 3.0], [1.0, 0.0, 4.0]]],
        'actor_sched': [2, 3, 4],
        'critic_sched': [0, 1, 2, 3, 4],
        'health_checks': 5,
        'itr': 5,
        'model_calls': [(True, False, 3), (False, True, 3)],
        'model_steps': 5,
        'n_model_calls': 50,
        'record_keys': [['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward', 'eval_best_reward'], ['itr', 'step',
          'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'train_episode_reward',
          'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward',
          'eval_best_reward'], ['itr', 'step', 'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl']],
        'records': [{'eval_best_reward': 1.4166666666666667, 'eval_episode_reward': 8.583333333333334, 'eval_success_rate': 0.0,
          'itr': 0, 'step': 0}, {'approx_kl': 0.01, 'itr': 1, 'loss': 1.5, 'pg_loss': 0.5, 'step': 60, 'train_episode_reward':
          17.75, 'v_loss': 2.0}, {'approx_kl': 0.02, 'itr': 2, 'loss': 1.5, 'pg_loss': 0.5, 'step': 120, 'train_episode_reward':
          26.0, 'v_loss': 2.0}, {'eval_best_reward': 5.166666666666667, 'eval_episode_reward': 36.083333333333336,
          'eval_success_rate': 1.0, 'itr': 3, 'step': 120}, {'approx_kl': 0.04, 'itr': 4, 'loss': 1.5, 'pg_loss': 0.5, 'step': 180,
          'train_episode_reward': 45.25, 'v_loss': 2.0}],
        'resets': [[0, 5, 15, 20], [0, 5, 15, 20]],
        'saves': [0, 2, 4],
        'updates': [
            {'chain_last': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0,
             0.0, 3.0, 3.0, 1.0, 1.0, 0.0, 1.0, 0.0, 4.0], 'firsts': ['111111', '000000', '000000', '110100', '001010', '000001'],
             'itr': 1, 'last': [2.0, 2.0, 1.0, 2.0, 1.0, 0.0], 'obs': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0,
             2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0, 0.0, 3.0, 3.0, 1.0, 1.0, 0.0, 1.0, 0.0, 4.0], 'reward': [[3.0, 4.0, 5.0,
             3.0, 4.0, 5.0], [3.5, 4.5, 5.5, 3.5, 4.5, 5.5], [4.0, 5.0, 6.0, 4.0, 5.0, 6.0], [4.5, 5.5, 6.5, 4.5, 5.5, 6.5], [5.0,
             6.0, 7.0, 5.0, 6.0, 7.0]], 'terminated': ['000000', '000000', '100100', '000000', '000000']},
            {'chain_last': [2.0, 2.0, 1.0, 2.0, 1.0, 0.0, 0.0, 0.0, 2.0, 0.0, 2.0, 1.0, 1.0, 1.0, 3.0, 1.0, 3.0, 2.0, 2.0, 2.0, 0.0,
             2.0, 0.0, 3.0, 0.0, 0.0, 1.0, 0.0, 1.0, 4.0], 'firsts': ['000001', '110100', '000000', '001010', '110100', '000001'],
             'itr': 2, 'last': [1.0, 1.0, 2.0, 1.0, 2.0, 0.0], 'obs': [2.0, 2.0, 1.0, 2.0, 1.0, 0.0, 0.0, 0.0, 2.0, 0.0, 2.0, 1.0,
             1.0, 1.0, 3.0, 1.0, 3.0, 2.0, 2.0, 2.0, 0.0, 2.0, 0.0, 3.0, 0.0, 0.0, 1.0, 0.0, 1.0, 4.0], 'reward': [[5.5, 6.5, 7.5,
             5.5, 6.5, 7.5], [6.0, 7.0, 8.0, 6.0, 7.0, 8.0], [6.5, 7.5, 8.5, 6.5, 7.5, 8.5], [7.0, 8.0, 9.0, 7.0, 8.0, 9.0], [7.5,
             8.5, 9.5, 7.5, 8.5, 9.5]], 'terminated': ['100100', '000000', '000000', '100100', '000000']},
            {'chain_last': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0,
             0.0, 3.0, 3.0, 1.0, 1.0, 0.0, 1.0, 0.0, 4.0], 'firsts': ['111111', '000000', '000000', '110100', '001010', '000001'],
             'itr': 4, 'last': [2.0, 2.0, 1.0, 2.0, 1.0, 0.0], 'obs': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0,
             2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0, 0.0, 3.0, 3.0, 1.0, 1.0, 0.0, 1.0, 0.0, 4.0], 'reward': [[10.5, 11.5,
             12.5, 10.5, 11.5, 12.5], [11.0, 12.0, 13.0, 11.0, 12.0, 13.0], [11.5, 12.5, 13.5, 11.5, 12.5, 13.5], [12.0, 13.0, 14.0,
             12.0, 13.0, 14.0], [12.5, 13.5, 14.5, 12.5, 13.5, 14.5]], 'terminated': ['000000', '000000', '100100', '000000',
             '000000']},
        ],
    },
    True: {
        'actions': [[[0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 0.25, 3.25], [1.25, 1.25, 0.25], [0.0, 0.0,
          0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0,
          2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 0.0], [0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 0.25, 3.25],
          [1.25, 1.25, 0.25], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 0.0]], [[0.25, 0.25,
          0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 3.25, 3.25], [1.25, 0.25, 4.25], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0],
          [2.0, 2.0, 2.0], [0.0, 3.0, 3.0], [1.0, 0.0, 4.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 3.0, 3.0],
          [1.0, 0.0, 4.0], [0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [2.25, 2.25, 2.25], [0.25, 3.25, 3.25], [1.25, 0.25, 4.25], [0.0,
          0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 3.0, 3.0], [1.0, 0.0, 4.0]]],
        'actor_sched': [2, 3, 4],
        'critic_sched': [0, 1, 2, 3, 4],
        'health_checks': 5,
        'itr': 5,
        'model_calls': [(True, False, 3), (False, True, 3)],
        'model_steps': 5,
        'n_model_calls': 50,
        'record_keys': [['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward', 'eval_best_reward'], ['itr', 'step',
          'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'train_episode_reward',
          'loss', 'pg_loss', 'v_loss', 'approx_kl'], ['itr', 'step', 'time', 'eval_success_rate', 'eval_episode_reward',
          'eval_best_reward'], ['itr', 'step', 'time', 'train_episode_reward', 'loss', 'pg_loss', 'v_loss', 'approx_kl']],
        'records': [{'eval_best_reward': 1.4166666666666667, 'eval_episode_reward': 8.583333333333334, 'eval_success_rate': 0.0,
          'itr': 0, 'step': 0}, {'approx_kl': 0.01, 'itr': 1, 'loss': 1.5, 'pg_loss': 0.5, 'step': 60, 'train_episode_reward':
          17.75, 'v_loss': 2.0}, {'approx_kl': 0.02, 'itr': 2, 'loss': 1.5, 'pg_loss': 0.5, 'step': 120, 'train_episode_reward':
          26.916666666666668, 'v_loss': 2.0}, {'eval_best_reward': 5.166666666666667, 'eval_episode_reward': 36.083333333333336,
          'eval_success_rate': 1.0, 'itr': 3, 'step': 120}, {'approx_kl': 0.04, 'itr': 4, 'loss': 1.5, 'pg_loss': 0.5, 'step': 180,
          'train_episode_reward': 45.25, 'v_loss': 2.0}],
        'resets': [[0, 5, 10, 15, 20], [0, 5, 10, 15, 20]],
        'saves': [0, 2, 4],
        'updates': [
            {'chain_last': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0,
             0.0, 3.0, 3.0, 1.0, 1.0, 0.0, 1.0, 0.0, 4.0], 'firsts': ['111111', '000000', '000000', '110100', '001010', '000001'],
             'itr': 1, 'last': [2.0, 2.0, 1.0, 2.0, 1.0, 0.0], 'obs': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0,
             2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0, 0.0, 3.0, 3.0, 1.0, 1.0, 0.0, 1.0, 0.0, 4.0], 'reward': [[3.0, 4.0, 5.0,
             3.0, 4.0, 5.0], [3.5, 4.5, 5.5, 3.5, 4.5, 5.5], [4.0, 5.0, 6.0, 4.0, 5.0, 6.0], [4.5, 5.5, 6.5, 4.5, 5.5, 6.5], [5.0,
             6.0, 7.0, 5.0, 6.0, 7.0]], 'terminated': ['000000', '000000', '100100', '000000', '000000']},
            {'chain_last': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0,
             0.0, 3.0, 3.0, 1.0, 1.0, 0.0, 1.0, 0.0, 4.0], 'firsts': ['111111', '000000', '000000', '110100', '001010', '000001'],
             'itr': 2, 'last': [2.0, 2.0, 1.0, 2.0, 1.0, 0.0], 'obs': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0,
             2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0, 0.0, 3.0, 3.0, 1.0, 1.0, 0.0, 1.0, 0.0, 4.0], 'reward': [[5.5, 6.5, 7.5,
             5.5, 6.5, 7.5], [6.0, 7.0, 8.0, 6.0, 7.0, 8.0], [6.5, 7.5, 8.5, 6.5, 7.5, 8.5], [7.0, 8.0, 9.0, 7.0, 8.0, 9.0], [7.5,
             8.5, 9.5, 7.5, 8.5, 9.5]], 'terminated': ['000000', '000000', '100100', '000000', '000000']},
            {'chain_last': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0,
             0.0, 3.0, 3.0, 1.0, 1.0, 0.0, 1.0, 0.0, 4.0], 'firsts': ['111111', '000000', '000000', '110100', '001010', '000001'],
             'itr': 4, 'last': [2.0, 2.0, 1.0, 2.0, 1.0, 0.0], 'obs': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0,
             2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 3.0, 0.0, 3.0, 3.0, 1.0, 1.0, 0.0, 1.0, 0.0, 4.0], 'reward': [[10.5, 11.5,
             12.5, 10.5, 11.5, 12.5], [11.0, 12.0, 13.0, 11.0, 12.0, 13.0], [11.5, 12.5, 13.5, 11.5, 12.5, 13.5], [12.0, 13.0, 14.0,
             12.0, 13.0, 14.0], [12.5, 13.5, 14.5, 12.5, 13.5, 14.5]], 'terminated': ['000000', '000000', '100100', '000000',
             '000000']},
        ],
    },
}
RECORDED_WANDB = [(0, ['eval_best_reward', 'eval_episode_reward', 'eval_success_rate', 'step']), (1, ['approx_kl', 'loss',
                  'pg_loss', 'step', 'train_episode_reward', 'v_loss']), (2, ['approx_kl', 'loss', 'pg_loss', 'step',
                  'train_episode_reward', 'v_loss']), (3, ['eval_best_reward', 'eval_episode_reward', 'eval_success_rate', 'step']),
                  (4, ['approx_kl', 'loss', 'pg_loss', 'step', 'train_episode_reward', 'v_loss'])]
RECORDED_EVAL = {False: {'eval_best_reward': 2.3636363636363638, 'eval_episode_reward': 13.909090909090908, 'eval_success_rate':
                 0.36363636363636365, 'num_episode': 11}, True: {'eval_best_reward': 13.909090909090908, 'eval_episode_reward':
                 13.909090909090908, 'eval_success_rate': 1.0, 'num_episode': 11}}


def check(got, want, pixels, chain):
    ups = got.pop("updates")
    wups = want["updates"]
    assert got == {k: v for k, v in want.items() if k != "updates"}
    assert len(ups) == len(wups)
    for u, w in zip(ups, wups):
        if pixels:
            assert u.pop("rgb") == u["obs"]  # the image rows are the state rows' step counters
        chain0 = u.pop("chain0")
        # a chain's first entry is its last - KFT; a one-shot sample is a one-entry chain
        assert chain0 == [x - (KFT if chain else 0) for x in u["chain_last"]]
        assert u == w


@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("chain", [True, False])
@pytest.mark.parametrize("pixels", [False, True])
def test_ppo_run_is_the_recorded_iteration(tmp_path, pixels, chain, reset):
    got = observe(tmp_path, pixels, chain, reset)
    check(got, RECORDED[(pixels, reset)], pixels, chain)


@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("chain", [True, False])
def test_ppo_run_over_two_env_groups_is_the_recorded_iteration(tmp_path, chain, reset):
    got = observe(tmp_path, False, chain, reset, groups=2)
    check(got, RECORDED_GROUPED[reset], False, chain)


@pytest.mark.parametrize("pixels", [False, True])
def test_every_ppo_loop_logs_to_wandb(tmp_path, pixels):
    """The pixel loop had lost the wandb branch; it logs what the state loop logs."""
    w = StubWandb()
    observe(tmp_path, pixels, True, False, wandb=w)
    assert w.logged == RECORDED_WANDB


def observe_eval(tmp_path, sparse):
    from dppo_amd.agent.eval.eval_agent import EvalAgent
    agent = object.__new__(EvalAgent)
    for k, v in dict(device="cpu", n_envs=E, venv=ScriptedVecEnv(), act_steps=ACT, n_steps=12, model=StubModel(True),
                     furniture_sparse_reward=sparse, best_reward_threshold_for_success=3,
                     result_path=str(tmp_path / "result.npz")).items():
        setattr(agent, k, v)
    res = agent.run()
    saved = np.load(agent.result_path)
    assert {k: saved[k].item() for k in saved.files} == res and "time" in res
    assert set(agent.model.calls) == {(True, False, E)} and agent.venv.resets == [0]
    return {k: v for k, v in res.items() if k != "time"}


@pytest.mark.parametrize("sparse", [False, True])
def test_eval_run_is_the_recorded_result(tmp_path, sparse):
    got = observe_eval(tmp_path, sparse)
    assert list(got) == ["num_episode", "eval_success_rate", "eval_episode_reward", "eval_best_reward"]
    assert got == RECORDED_EVAL[sparse]
