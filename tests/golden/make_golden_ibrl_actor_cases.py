"""Case table and plain-torch restatement of IBRL's actor loss through the ensemble's min (reference model/rl/gaussian_ibrl.py:115-128
on GaussianModel.forward, model/common/gaussian.py:85-120), shared by make_golden_ibrl_actor.py (generator, needs the reference),
tests/test_ibrl_actor.py and tests/test_ibrl_agent.py (no reference needed).

The networks, observations and draws of the first five cases are make_golden_ibrl_cases.py's (``K``, imported and not edited): the
online actor ``K.actor_params(case, "rl")``, the members ``K.member_params(case, e)``, ``K.inputs(case, n)["obs"]`` and the
``noise_rl`` / ``mask_rl`` draws.  A case may add SHIFT[case][e], a multiple of GRID = 2^-10, to member e's out-layer bias, which moves
q_e by exactly that and nothing else.  Measured once with measure(): K's members meet every condition below as they are (wins per
member: tiny_77 24 / 31 / 22, chunk_130 25 / 24 / 29 / 21 / 31, nodrop_64 36 / 28, can_256 30 / 172 / 35 / 3 / 16; smallest gaps 6.4e-3,
9.8e-2, 1.7e-2, 6.7e-3), so their shifts are 0; ``wide``'s sixteen seeded members are shifted by their negated float64 medians,
without which member 6 wins all three rows.  The conditions are asserted on the float64 restatement when the fixture is written
(check_conditions) and again by the tests.

  * outside ``twins`` the gap between a row's smallest and second-smallest Q is at least GAP (g31's band);
  * in every case with N >= 2 E every member wins at least one row;
  * the draws stay CLIP_BAND away from RANDN_CLIP (K's recipe) and, with N >= 3, at least one element is clamped on each side;
  * ReLU pre-activations below RELU_TIE are counted and reported (no gate is handed over anywhere).

``twins``: tiny's networks at N = 77 with member 2 a copy of member 1; the pair is the smallest on some rows, where d_a does not
depend on which of the two is picked and the library must name the lower index, 1.  ``wide``: E = 16 members of [1024, 1024] at
N = 3 under a [64, 64] actor, the top of the accepted range; it is restated only, no fixture holds it.

The restatement is written the way the reference writes it -- the clamped rsample, ``current_q.min(dim=0).values``, ``-mean`` -- takes a
dtype (float32 reproduces g32, float64 fed the same fp32 values is the yardstick of the GPU tests) and an optional ``sel`` handed in,
so that a second implementation (bf16) is compared on its own decisions.  It works under ``K.bf16_linears()``."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dppo_oracle as O
from tests.golden import make_golden_ibrl_cases as K

GRID = 2.0 ** -10
GAP = 1e-4
FIXED_STD, RANDN_CLIP, CLIP_BAND = K.FIXED_STD, K.RANDN_CLIP, K.CLIP_BAND
WIDE_NET = (11, 1, 3, [64, 64], "ReLU", 0.5, [1024, 1024], "ReLU", 16)
SEED_WIDE_ACTOR, SEED_WIDE_Q, SEED_WIDE_INPUTS = 3501, 3531, 3591
# (case, n) -> K's case whose recipes it borrows (None: its own)
ACTOR_CASES = {("tiny", 1): "tiny", ("tiny", 77): "tiny", ("chunk", 130): "chunk", ("nodrop", 64): "nodrop", ("can", 256): "can",
               ("twins", 77): "tiny", ("wide", 3): None}
CASES = [c for c in ACTOR_CASES if c[0] != "wide"]  # the fixture's
ALL_CASES = list(ACTOR_CASES)
TWIN_PAIR = (1, 2)
# out-layer bias shifts in units of GRID, per member (measure() prints the recipe's suggestion)
SHIFT = {
    "tiny": (0, 0, 0),
    "chunk": (0, 0, 0, 0, 0),
    "nodrop": (0, 0),
    "can": (0, 0, 0, 0, 0),
    "twins": (0, 0, 0),
    "wide": (-137, -99, 68, 73, -1304, -2209, 2497, 954, 1017, 966, 1514, 1328, -885, -743, 1480, -650),
}
# the recorded update sequence on tiny, N = 77: two critic AdamW steps, each with Polyak, one actor step, the target actor's Polyak
SEQ_CASE, SEQ_N = "tiny", 77
SEQ_PAIRS = ((2, 0), (0, 1))
SEQ_LR, SEQ_ACTOR_LR, SEQ_TAU, SEQ_WEIGHT_DECAY = 1e-3, 3e-4, 0.005, 0.0


def net_of(case):
    """(obs_dim, Ta, Da, actor widths, actor activation, dropout p, critic widths, critic activation, E)."""
    return WIDE_NET if case == "wide" else K.IBRL_NETS["tiny" if case == "twins" else case]


def n_critics(case):
    return net_of(case)[8]


def actor_spec(case):
    od, ta, da, dims, act = net_of(case)[:5]
    return O.NetSpec("gaussian", cond_dim=od, mlp_dims=list(dims), activation=act, residual=False, action_dim=da, horizon_steps=ta)


def q_spec(case):
    od, ta, da = net_of(case)[:3]
    return O.NetSpec("critic", cond_dim=od + ta * da, mlp_dims=list(net_of(case)[6]), activation=net_of(case)[7], residual=False,
                     use_layernorm=True)


def actor_params(case):
    """Trunk state dict of the online actor."""
    if case == "wide":
        return O.init_params(actor_spec(case), SEED_WIDE_ACTOR)
    return K.actor_params("tiny" if case == "twins" else case, "rl")


def actor_state_dict(case):
    sd = dict(actor_params(case))
    sd["logvar_min"] = torch.log(torch.tensor(0.01 ** 2))
    sd["logvar_max"] = torch.log(torch.tensor(1.0 ** 2))
    return sd


def out_bias_key(case):
    return f"Q1.moduleList.{len(net_of(case)[6])}.linear_1.bias"


def member_params(case, e, shifted=True):
    """State dict of online member e with its shift on the out-layer bias; ``twins``: member 2 is member 1."""
    if case == "wide":
        p = O.init_params(q_spec(case), SEED_WIDE_Q + e, K.Q_SCALE)
    else:
        src = TWIN_PAIR[0] if case == "twins" and e == TWIN_PAIR[1] else e
        p = K.member_params("tiny" if case == "twins" else case, src)
    if shifted:
        key = out_bias_key(case)
        p[key] = p[key] + np.float32(SHIFT[case][e] * GRID)
    return p


def members_of(case, shifted=True):
    return [member_params(case, e, shifted) for e in range(n_critics(case))]


@functools.lru_cache(maxsize=None)
def _inputs(case, n):
    if case != "wide":
        b = K.inputs("tiny" if case == "twins" else case, n)
        return dict(obs=b["obs"], noise=b["noise_rl"], mask=b["mask_rl"])
    od, ta, da, dims = WIDE_NET[:4]
    rs = np.random.RandomState(SEED_WIDE_INPUTS)
    obs = torch.from_numpy(rs.uniform(-1, 1, size=(n, 1, od)).astype(np.float32))
    z = np.clip(rs.standard_normal(size=(n, ta, da)), -2.5, 2.5).astype(np.float32)
    z[0, 0, 0], z[1, 0, 1] = 3.5, -3.75  # one element clamped on each side, on purpose
    mask = (rs.uniform(size=(len(dims), n, dims[0])) >= WIDE_NET[5]).astype(np.uint8)
    return dict(obs=obs, noise=torch.from_numpy(z), mask=torch.from_numpy(mask))


def inputs(case, n):
    """dict(obs (n, 1, Do), noise (n, Ta, Da), mask (L, n, H) uint8)."""
    return dict(_inputs(case, n))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def actor_pre(p, case, obs, mask, record=None):
    """The actor trunk's output before tanh, (n, Ta*Da): nn.Dropout (as x * (mask / (1 - p))) behind every hidden Linear, in front of
    the activation.  ``record``: a list that receives every ReLU pre-activation."""
    spec, pd = actor_spec(case), net_of(case)[5]
    fn = F.mish if spec.activation == "Mish" else O._ACT[spec.activation]
    x = obs.reshape(len(obs), -1)
    L = len(spec.mlp_dims)
    for i in range(L):
        x = F.linear(x, p[f"mlp_mean.moduleList.{i}.linear_1.weight"], p[f"mlp_mean.moduleList.{i}.linear_1.bias"])
        if mask is not None and pd > 0:
            x = x * (mask[i].to(x.dtype) / (1 - pd))
        if record is not None and spec.activation == "ReLU":
            record.append(x.detach())
        x = fn(x)
    return F.linear(x, p[f"mlp_mean.moduleList.{L}.linear_1.weight"], p[f"mlp_mean.moduleList.{L}.linear_1.bias"])


def q_forward(p, case, obs, act):
    x = torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=-1)
    return O.critic_forward(p, q_spec(case), x).reshape(-1)


def argmin_lowest(q):
    """The library's rule on (E, n): the smallest, a tie to the lowest member index."""
    best, sel = q[0].clone(), torch.zeros(q.shape[1], dtype=torch.int64)
    for e in range(1, q.shape[0]):
        lower = q[e] < best
        best, sel = torch.where(lower, q[e], best), torch.where(lower, torch.full_like(sel, e), sel)
    return sel


def loss_actor(actor_p, members, case, obs, noise, mask, dtype=torch.float32, sel=None, use_mask=True):
    """gaussian_ibrl.py:115-128 with rsample's draw and the dropout masks given.  ``actor_p``: leaf tensors of ``dtype``; ``members``:
    E plain dicts.  ``sel`` (n,) given: row n reads that member instead of ``min``.  Returns dict(loss, stats {loss, mean min q, mean
    over rows and members of q}, d_a, grads (one per entry of actor_p, in its order), a, mu, q (E, n), sel (own), qmin, relu_pre)."""
    obs = obs.to(dtype)
    pre = []
    loc = torch.tanh(actor_pre(actor_p, case, obs, mask if use_mask else None, pre))
    scale = torch.ones_like(loc) * FIXED_STD
    a = loc + noise.reshape(loc.shape).to(dtype) * scale
    a = torch.clamp(a, loc - RANDN_CLIP * scale, loc + RANDN_CLIP * scale)
    q = torch.stack([q_forward(K.cast(m, dtype), case, obs, a) for m in members])
    own = argmin_lowest(q.detach())
    if sel is None:
        qm = q.min(dim=0).values
    else:
        qm = q.gather(0, torch.as_tensor(np.asarray(sel)).reshape(1, -1).long())[0]
    loss = -torch.mean(qm)
    d_a = torch.autograd.grad(loss, a, retain_graph=True)[0]
    grads = torch.autograd.grad(loss, list(actor_p.values()))
    stats = np.array([loss.item(), qm.detach().double().mean().item(), q.detach().double().mean().item()])
    return dict(loss=loss.detach(), stats=stats, d_a=d_a.detach(), grads=list(grads), a=a.detach(), mu=loc.detach(), q=q.detach(),
                sel=own.numpy(), qmin=qm.detach(), relu_pre=pre)


def restate(case, n, dtype=torch.float64, sel=None, use_mask=True):
    """``loss_actor`` of one case on fresh leaves, with ``named`` = (state-dict name, gradient) in the state dict's order."""
    a, b = K.leaf(actor_params(case), dtype), inputs(case, n)
    res = loss_actor(a, members_of(case), case, b["obs"], b["noise"], b["mask"], dtype=dtype, sel=sel, use_mask=use_mask)
    res["named"] = list(zip(a, res["grads"]))
    return res


def conditions(case, n):
    """What the module docstring promises, measured on the float64 restatement: dict(gap, wins (E,), clamped (lo, hi), band_ok,
    relu_near)."""
    r, b = restate(case, n), inputs(case, n)
    q = r["q"]
    srt = torch.sort(q, dim=0).values
    gap = (srt[1] - srt[0]).min().item()
    wins = np.bincount(r["sel"], minlength=q.shape[0])
    z = b["noise"].double()
    edge = (z.abs() - RANDN_CLIP).abs()
    near = sum(int(((p.abs() < K.RELU_TIE) & (p != 0)).sum()) for p in r["relu_pre"])  # (a dropped unit is an exact 0: no tie)
    return dict(gap=gap, wins=wins, clamped=(int((z < -RANDN_CLIP).sum()), int((z > RANDN_CLIP).sum())),
                band_ok=bool((edge >= CLIP_BAND).all()), relu_near=near, q=q, sel=r["sel"])


def check_conditions(case, n):
    c = conditions(case, n)
    E = n_critics(case)
    if case == "twins":
        i, j = TWIN_PAIR
        assert torch.equal(c["q"][i], c["q"][j]) and c["wins"][i] >= 5 and c["wins"][j] == 0 and c["wins"][0] >= 5, c["wins"]
        rest = torch.stack([c["q"][e] for e in range(E) if e != j])
        srt = torch.sort(rest, dim=0).values
        assert (srt[1] - srt[0]).min().item() >= GAP
    else:
        assert c["gap"] >= GAP, (case, n, c["gap"])
        if n >= 2 * E:
            assert (c["wins"] >= 1).all(), (case, n, c["wins"])
    assert c["band_ok"], (case, n)
    if n >= 3:
        assert c["clamped"][0] >= 1 and c["clamped"][1] >= 1, (case, n, c["clamped"])
    return c


# ---- the recorded update sequence ---------------------------------------------------------------------------------------------------
def seq_members():
    return members_of(SEQ_CASE), [K.member_params(SEQ_CASE, e, K.TARGET_EPS) for e in range(n_critics(SEQ_CASE))]


def restate_sequence(dtype=torch.float32):
    """One ``update_iteration`` in the agent's order (reference train_ibrl_agent.py:245-297) on ONE batch, K.inputs(tiny, 77), used for
    both critic updates with the pairs SEQ_PAIRS: [critic loss, AdamW step, Polyak] x 2, the actor loss against the STEPPED members,
    its AdamW step, the target actor's Polyak.  ``gq``: one list of member gradients per critic update.  Returns what make_golden_ibrl_actor.update_sequence records."""
    case, n = SEQ_CASE, SEQ_N
    b = K.inputs(case, n)
    online, target = seq_members()
    members = [K.leaf(m, dtype) for m in online]
    targets = [K.cast(m, dtype) for m in target]
    actor = K.leaf(actor_params(case), dtype)
    tactor = K.cast(K.actor_params(case, "target"), dtype)
    flat = [t for m in members for t in m.values()]
    opt_c = torch.optim.AdamW(flat, lr=SEQ_LR, weight_decay=SEQ_WEIGHT_DECAY)
    opt_a = torch.optim.AdamW(list(actor.values()), lr=SEQ_ACTOR_LR, weight_decay=SEQ_WEIGHT_DECAY)
    c_losses, gq = [], []
    for pair in SEQ_PAIRS:
        rc = K.loss_critic(members, targets, case, b, pair, dtype=dtype)
        for m, gs in zip(members, rc["grads"]):
            for t, g in zip(m.values(), gs):
                t.grad = g.clone()
        gq.append([{k: t.grad.clone() for k, t in m.items()} for m in members])
        opt_c.step()
        targets = [{k: tq[k] * (1.0 - SEQ_TAU) + m[k].detach() * SEQ_TAU for k in tq} for tq, m in zip(targets, members)]
        c_losses.append(rc["loss"].item())
    stepped = [{k: t.detach().clone() for k, t in m.items()} for m in members]
    ra = loss_actor(actor, stepped, case, b["obs"], b["noise_rl"], b["mask_rl"], dtype=dtype)
    for t, g in zip(actor.values(), ra["grads"]):
        t.grad = g.clone()
    ga = {k: t.grad.clone() for k, t in actor.items()}
    opt_a.step()
    tactor = {k: tactor[k] * (1.0 - SEQ_TAU) + actor[k].detach() * SEQ_TAU for k in tactor}
    return dict(c_losses=c_losses, gq=gq, q=stepped, target=targets, a_loss=ra["loss"].item(), ga=ga,
                actor={k: v.detach() for k, v in actor.items()}, target_actor=tactor)


def measure():
    """Prints, per case, the float64 medians of the UNSHIFTED members' Q in units of GRID (negated: the recipe's shifts), and the
    conditions under the shifts in force."""
    for case, n in ALL_CASES:
        b = inputs(case, n)
        a = K.leaf(actor_params(case), torch.float64)
        r = loss_actor(a, members_of(case, shifted=False), case, b["obs"], b["noise"], b["mask"], dtype=torch.float64)
        med = r["q"].median(dim=1).values
        print(f"{case}_{n}: suggested shifts {[-int(round(m.item() / GRID)) for m in med]}")
        c = conditions(case, n)
        print(f"  in force: smallest gap {c['gap']:.3e}, wins {c['wins'].tolist()}, clamped (lo, hi) {c['clamped']}, band ok {c['band_ok']}, "
              f"ReLU pre-activations below {K.RELU_TIE:g}: {c['relu_near']}")


if __name__ == "__main__":
    measure()
