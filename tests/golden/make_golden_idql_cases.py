"""Case tables and seeded recipes shared by make_golden_idql.py (generator, needs the reference) and tests/test_idql.py (no
reference needed): IDQL's twin-Q / expectile-V losses, best-of-N selection and one update sequence.

Nothing large is stored in g24_idql.npz: weights come from ``oracle.dppo_oracle.init_params``, inputs from the seeded numpy
recipes below; the fixture holds what only the reference can say (which candidate rows keep a margin from adv = 0, the shift of
V's output bias that balances the two signs, losses, statistics, gradients, chosen indices, actions)."""
import numpy as np
import torch

from oracle import dppo_oracle as O

# name -> (oracle spec name: obs / action shapes and the actor, residual_tyle, double_q)
IDQL_NETS = {
    "hopper": ("hopper", False, True),            # obs 11, act 4 x 3, plain Q (every shipped cfg: the ``residual_tyle`` typo)
    "can": ("can", False, True),                  # 23, 4 x 7 -- the shipped IDQL cfg's chunk, not the PPO cfg's 8 x 7
    "transport": ("transport", False, True),      # 59, 8 x 14: Q in_dim 171
    "hopper_res": ("hopper", True, True),         # residual_tyle=True
    "hopper_single": ("hopper", False, False),    # double_q=False
}
IDQL_HORIZON = {"can": 4}  # Ta where the IDQL cfg differs from the oracle's PPO spec
IDQL_SIZES = (77, 1000)    # a ragged tile; the shipped batch
IDQL_CASES = [(net, n) for net in IDQL_NETS for n in IDQL_SIZES]
SEED_Q1, SEED_Q2, SEED_V, SEED_ACTOR, SEED_TARGET = 241, 242, 243, 244, 245
WEIGHT_SCALE = 3.0         # of the critics' seeded weights: outputs of O(1), so that adv is not flat
TARGET_EPS = 0.05          # target = Q + TARGET_EPS * (a seeded draw of the same recipe)
EXPECTILE, GAMMA, REWARD_SCALE = 0.8, 0.99, 0.01
ADV_MARGIN, SIGN_SHARE = 0.1, 0.25
SAMPLING = [(8, 5, True), (8, 5, False), (40, 20, True), (40, 20, False)]  # (B, S, deterministic), hopper networks
SAMPLING_KW = dict(denoising_steps=20, randn_clip_value=3, min_sampling_denoising_std=0.1)
CRITIC_HYPERPARAM = 0.7
U_MARGIN, GAP_MARGIN = 1e-4, 1e-3
# the recorded update sequence (hopper, N = 77): AdamW(lr, betas (0.9, 0.999), eps 1e-8, weight_decay 0) steps, then Polyak
SEQ_LR, SEQ_TAU = 1e-3, 0.005


def shapes(net):
    """(obs_dim, Ta, Da) of a case's networks."""
    a, _ = O.named_specs(IDQL_NETS[net][0])
    return a.cond_dim, IDQL_HORIZON.get(net, a.horizon_steps), a.action_dim


def q_spec(net):
    od, ta, da = shapes(net)
    return O.NetSpec("critic", cond_dim=od + ta * da, mlp_dims=[256, 256, 256], activation="Mish", residual=IDQL_NETS[net][1])


def v_spec(net):
    return O.NetSpec("critic", cond_dim=shapes(net)[0], mlp_dims=[256, 256, 256], activation="Mish", residual=True)


def actor_spec(net):
    a, _ = O.named_specs(IDQL_NETS[net][0])
    return a


def twin_params(net, eps=0.0):
    """State dict of CriticObsAct: Q1 (and Q2) from distinct seeds; eps != 0 adds the target's perturbation."""
    spec, out = q_spec(net), {}
    for i, seed in enumerate((SEED_Q1, SEED_Q2)[:2 if IDQL_NETS[net][2] else 1]):
        p, d = O.init_params(spec, seed, WEIGHT_SCALE), O.init_params(spec, SEED_TARGET + 10 * i, WEIGHT_SCALE)
        for k in p:
            out[k.replace("Q1.", f"Q{i + 1}.")] = p[k] + np.float32(eps) * d[k] if eps else p[k]
    return out


def v_params(net, bias_shift=0.0):
    """State dict of the V critic; ``bias_shift`` (recorded per case in the fixture) is added to the output bias."""
    p = dict(O.init_params(v_spec(net), SEED_V, WEIGHT_SCALE))
    last = [k for k in p if k.endswith(".bias")][-1]
    p[last] = p[last] + np.float32(bias_shift)
    return p


def candidates(net, n):
    """The 4n seeded candidate transitions of case (net, n): obs, next_obs (4n, 1, Do), actions (4n, Ta, Da), reward scaled by
    REWARD_SCALE, terminated in {0, 1}.  The fixture's ``keep`` picks the n rows of the case."""
    od, ta, da = shapes(net)
    rs = np.random.RandomState(2400 + 7 * list(IDQL_NETS).index(net) + n)
    m = 4 * n
    f = lambda *s: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32))
    obs, nxt, act = f(m, 1, od), f(m, 1, od), f(m, ta, da)
    reward = torch.from_numpy((REWARD_SCALE * rs.uniform(0, 4, size=m)).astype(np.float32))
    terminated = torch.from_numpy((rs.uniform(size=m) < 0.3).astype(np.float32))
    return obs, nxt, act, reward, terminated


def sampling_inputs(B, S, seed):
    """state (B, 1, Do), noise (K + 1, S * B, Ta, Da), u (B,) of a hopper sampling case."""
    od, ta, da = shapes("hopper")
    rs = np.random.RandomState(seed)
    state = torch.from_numpy(rs.uniform(-1, 1, size=(B, 1, od)).astype(np.float32))
    noise = torch.from_numpy(rs.randn(SAMPLING_KW["denoising_steps"] + 1, S * B, ta, da).astype(np.float32))
    u = torch.from_numpy(rs.uniform(0.02, 0.98, size=B).astype(np.float32))
    return state, noise, u
