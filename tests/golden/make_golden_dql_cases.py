"""Case table, seeded recipes and a plain-torch restatement shared by make_golden_dql.py (generator, needs the reference) and
tests/test_dql.py (no reference needed): DQL's actor loss, differentiated through the K-step sampling chain.

Nets, seeds and the critics' weight scale are make_golden_qsm_cases.py's.  Nothing large is stored in g26_dql.npz: weights and
inputs come from seeds; the fixture holds what only the reference can say.  ``loss_actor`` below rebuilds every one of those
numbers from the oracle's forwards and ``torch.autograd.grad``; it can also be evaluated ON A GIVEN CHAIN (the values of every
step's input are the chain's, the gradient still flows from step to step) and WITH GIVEN CLAMP MASKS -- what a second
implementation of the same loss is compared against where an x0 lands on the other side of the clamp's edge."""
import numpy as np
import torch

from oracle import dppo_oracle as O
from tests.golden import make_golden_qsm_cases as Q

# case -> (net of make_golden_qsm_cases.QSM_NETS, K, model kwargs, which)
DQL_CASES = {
    "scratch": ("scratch", 10, {}, 0),          # AF = 3: below one 16-byte store
    "hopper": ("hopper", 20, {}, 0),            # ReLU
    "transport": ("transport", 20, {}, 0),      # Mish, AF = 112
    "hopper_noclip": ("hopper", 20, dict(denoised_clip_value=None), 0),   # no masks: a smooth function
    "hopper_final": ("hopper", 20, dict(final_action_clip_value=1.0), 0),
    "hopper_k1": ("hopper", 1, {}, 0),          # one step
    "hopper_q2": ("hopper", 20, {}, 1),         # the other side of the coin
}
CASES = [(c, 77) for c in DQL_CASES] + [("hopper", 1000)]  # a ragged tile (four 16-row tiles and 13 rows); the shipped batch
# cases whose chain g26 stores in full; the others' chains (0.7 MB for transport alone) are stored as flat[::61] + norm and rebuilt by
# the restatement, which test_dql.py pins to those entries
FULL_CHAINS = [("scratch", 77), ("hopper", 77), ("hopper_k1", 77)]
ETA = 1.0
SAMPLING_KW = Q.SAMPLING_KW
MIN_STD, RANDN_CLIP = SAMPLING_KW["min_sampling_denoising_std"], SAMPLING_KW["randn_clip_value"]
NEAR_TIE, NEAR_TIE_CAP = 1e-4, 1e-3
GAMMA = Q.GAMMA
SEQ_LR, SEQ_ACTOR_LR, SEQ_TAU = Q.SEQ_LR, Q.SEQ_ACTOR_LR, Q.SEQ_TAU


def net_of(case):
    return DQL_CASES[case][0]


def shapes(case):
    """(obs_dim, Ta, Da, K) of a case."""
    od, ta, da, _ = Q.shapes(net_of(case))
    return od, ta, da, DQL_CASES[case][1]


def model_kw(case):
    """denoised_clip_value (default 1.0) and final_action_clip_value (default None) of a case."""
    return dict(dict(denoised_clip_value=1.0, final_action_clip_value=None), **DQL_CASES[case][2])


def which(case):
    return DQL_CASES[case][3]


def inputs(case, n):
    """obs (n, 1, Do) in [-1, 1]; noise (K+1, n, Ta, Da): x_K, then the draw of every step; noise_bc (n, Ta, Da), t_bc (n,) in
    [0, K): the BC term's draws; and QSM's transitions for the recorded sequence's critic step."""
    od, ta, da, K = shapes(case)
    rs = np.random.RandomState(2600 + 11 * list(DQL_CASES).index(case) + n)
    obs = torch.from_numpy(rs.uniform(-1, 1, size=(n, 1, od)).astype(np.float32))
    noise = torch.from_numpy(rs.randn(K + 1, n, ta, da).astype(np.float32))
    noise_bc = torch.from_numpy(rs.randn(n, ta, da).astype(np.float32))
    t_bc = torch.from_numpy(rs.randint(0, K, size=n).astype(np.int64))
    return dict(obs=obs, noise=noise, noise_bc=noise_bc, t_bc=t_bc)


def near_ties(x0_raw, K, clip):
    """Flat indices into (n, K, AF) of the elements whose |x0_raw| is within NEAR_TIE * max(1, srm1[t]) of the clamp's edge:
    about 100 x the fp32 error of eps scaled by srm1 (406 at t = 19 of 20).  Position s of axis 1 is the step at t = K - 1 - s."""
    if clip is None:
        return np.zeros(0, dtype=np.int64)
    srm1 = O.ddpm_tables(K)["sqrt_recipm1_alphas_cumprod"].numpy()[::-1].astype(np.float64)
    tol = NEAR_TIE * np.maximum(1.0, srm1)[None, :, None]
    return np.flatnonzero(np.abs(np.abs(x0_raw.astype(np.float64)) - clip) < tol)


# ---- rounding of every Linear's operands to bf16 (the bf16 yardstick) --------------------------------------------------------
class _Bf16Linear(torch.autograd.Function):
    """F.linear with the weight and the input rounded to bf16 on the way in, forward and backward (the gradient arriving from
    above is an input of both backward products), products accumulated in fp32; bias and everything outside stay fp32."""

    @staticmethod
    def forward(ctx, x, w, b):
        r = lambda v: v.to(torch.bfloat16).float()
        xr, wr = r(x), r(w)
        ctx.save_for_backward(xr, wr)
        ctx.has_bias = b is not None
        y = xr @ wr.t()
        return y + b if b is not None else y

    @staticmethod
    def backward(ctx, g):
        xr, wr = ctx.saved_tensors
        gr = g.to(torch.bfloat16).float()
        gb = g.reshape(-1, g.shape[-1]).sum(0) if ctx.has_bias else None
        return gr @ wr, gr.reshape(-1, gr.shape[-1]).t() @ xr.reshape(-1, xr.shape[-1]), gb


class bf16_linears:
    """Context: every torch.nn.functional.linear call (the oracle's forwards use nothing else for their Linears) rounds its
    operands to bf16."""

    def __enter__(self):
        self.real = torch.nn.functional.linear
        torch.nn.functional.linear = lambda x, w, b=None: _Bf16Linear.apply(x, w, b)

    def __exit__(self, *a):
        torch.nn.functional.linear = self.real


# ---- ReLU gates near zero ---------------------------------------------------------------------------------------------------
# ReLU's derivative jumps at 0 as the x0 clamp's does at its edge.  A hidden pre-activation is a 512-term fp32 sum of O(0.2)
# (median |z| 0.16 at these weights): two correct implementations differ in it by about sqrt(512) * 2^-24 * 0.2 = 3e-7, so a
# unit with |z| below RELU_TIE = 1e-6 may stand on either side of 0 (9 of hopper N = 77's 1,655,808 pre-activations do).
RELU_TIE = 1e-6


class relu_gates:
    """Context: records every pre-activation the oracle's ReLU sees (``calls``, in call order) and forces the gate of the listed
    elements: force = {(call, flat index): open?}.  An open gate passes the value and the gradient, a closed one neither."""

    def __init__(self, force=None):
        self.force, self.calls = dict(force or {}), []

    def _act(self, x):
        c = len(self.calls)
        self.calls.append(x.detach())
        y = self.real(x)
        for (cc, idx), on in self.force.items():
            if cc == c:
                m = torch.zeros(x.numel(), dtype=torch.bool)
                m[idx] = True
                y = torch.where(m.reshape(x.shape), x if on else x * 0, y)
        return y

    def __enter__(self):
        self.real = O._ACT["ReLU"]
        O._ACT["ReLU"] = self._act
        return self

    def __exit__(self, *a):
        O._ACT["ReLU"] = self.real

    def near_zero(self):
        """[(|z|, (call, flat index), gate as computed)] of the recorded pre-activations below RELU_TIE, smallest first."""
        out = []
        for c, x in enumerate(self.calls):
            z = x.reshape(-1)
            for i in torch.nonzero(z.abs() < RELU_TIE).reshape(-1).tolist():
                out.append((abs(float(z[i])), (c, i), bool(z[i] > 0)))
        return sorted(out)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def loss_actor(actor_p, q_params, case, b, chains=None, masks=None, eta=ETA):
    """diffusion_dql.py:74-88 with forward_train :141-179, its draws replaced by ``b``'s.  ``actor_p``: leaf tensors.
    chains (n, K+1, Ta, Da) given: every step's input takes its VALUE from it.  masks (n, K, AF) given: the x0 clamp is
    where(mask, x0, sign(x0) * clip), gradient where mask.  Returns loss, stats {loss, bc, q_loss, mean q1, mean q2}, d_a, masks,
    x0_raw (n, K, AF), chain (n, K+1, AF) and grads (one per entry of actor_p, in its order)."""
    net = net_of(case)
    od, ta, da, K = shapes(case)
    kw, spec, n = model_kw(case), Q.actor_spec(net), len(b["obs"])
    clip, tabs = kw["denoised_clip_value"], O.ddpm_tables(K)
    col = lambda name, t: tabs[name][t].reshape(1, 1, 1)
    as_value = lambda x, i: x if chains is None else chains[:, i].reshape(x.shape).detach() + (x - x.detach())
    x = b["noise"][0]
    chain, x0s, ms = [], [], []
    for i, t in enumerate(reversed(range(K))):
        x = as_value(x, i)
        chain.append(x.detach())
        tb = torch.full((n,), t, dtype=torch.int64)
        eps = O.actor_forward(actor_p, spec, x, tb, b["obs"])
        x0 = col("sqrt_recip_alphas_cumprod", t) * x - col("sqrt_recipm1_alphas_cumprod", t) * eps
        x0s.append(x0.detach().reshape(n, -1))
        if clip is None:
            ms.append(torch.ones(n, ta * da, dtype=torch.bool))
        elif masks is None:
            ms.append(x0s[-1].abs() <= clip)
            x0 = x0.clamp(-clip, clip)
        else:
            m = torch.as_tensor(masks)[:, i].reshape(x0.shape).bool()
            ms.append(m.reshape(n, -1))
            x0 = torch.where(m, x0, (torch.sign(x0) * clip).detach())
        mu = col("ddpm_mu_coef1", t) * x0 + col("ddpm_mu_coef2", t) * x
        std = torch.clip(torch.exp(0.5 * col("ddpm_logvar_clipped", t)), min=MIN_STD)
        x = mu + std * b["noise"][i + 1].clamp(-RANDN_CLIP, RANDN_CLIP)
    if kw["final_action_clip_value"]:
        x = torch.clamp(x, -1, 1)
    a = as_value(x, K)
    chain.append(a.detach())
    q1, q2 = Q.twin_forward(q_params, net, b["obs"], a)
    x_noisy = O.q_sample(K, a, b["t_bc"], b["noise_bc"])
    bc = torch.nn.functional.mse_loss(O.actor_forward(actor_p, spec, x_noisy, b["t_bc"], b["obs"]), b["noise_bc"])
    qa, qb = (q1, q2) if which(case) == 0 else (q2, q1)
    q_loss = -qa.mean() / qb.abs().mean().detach()
    loss = bc + eta * q_loss
    grads = torch.autograd.grad(loss, [a] + list(actor_p.values()))
    stats = np.array([loss.item(), bc.item(), q_loss.item(), q1.detach().double().mean().item(), q2.detach().double().mean().item()])
    return dict(loss=loss.detach(), stats=stats, d_a=grads[0].reshape(n, -1), masks=torch.stack(ms, 1).numpy(),
                x0_raw=torch.stack(x0s, 1).numpy(), chain=torch.stack(chain, 1).reshape(n, K + 1, -1), grads=list(grads[1:]))


def critic_batch(n=77):
    """QSM's hopper transitions with the DQL hopper case's observations: the recorded sequence's minibatch."""
    b = dict(Q.inputs("hopper", n))
    b.update(inputs("hopper", n))
    return b


def restate_sequence(b):
    """One update on ``b`` in the reference agent's order (:232-260): critic loss and AdamW step, actor loss with the UPDATED
    critic and its step, Polyak.  Returns what make_golden_dql.update_sequence records."""
    q, tq, a = Q.leaf(Q.twin_params("hopper")), Q.twin_params("hopper", Q.TARGET_EPS), Q.leaf(Q.actor_params("hopper"))
    opt_c = torch.optim.AdamW(list(q.values()), lr=SEQ_LR, weight_decay=0)
    opt_a = torch.optim.AdamW(list(a.values()), lr=SEQ_ACTOR_LR, weight_decay=0)
    lc, _, _ = Q.critic_loss(q, tq, "hopper", b)
    lc.backward()
    gq = {k: v.grad.clone() for k, v in q.items()}
    opt_c.step()
    q2 = {k: v.detach() for k, v in q.items()}
    res = loss_actor(a, q2, "hopper", b)
    ga = dict(zip(a, res["grads"]))
    for k, v in a.items():
        v.grad = ga[k].clone()
    opt_a.step()
    t2 = {k: tq[k] * (1.0 - SEQ_TAU) + q2[k] * SEQ_TAU for k in tq}
    return dict(c_loss=lc.item(), a_loss=res["loss"].item(), gq=gq, ga=ga, q=q2, actor={k: v.detach() for k, v in a.items()}, target=t2)
