"""Generate the IDQL fixture by running the REFERENCE's IDQLDiffusion / CriticObsAct / CriticObs on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_idql.py <checkout of the reference (the directory holding dppo/)>

Writes tests/golden/g24_idql.npz.  Per loss case (make_golden_idql_cases.IDQL_CASES): which n of the 4n seeded candidate rows are
kept (|adv| >= ADV_MARGIN * max |adv|, each sign >= SIGN_SHARE of them: the expectile loss is discontinuous in sign(adv), and a
bf16 run must not flip one), the shift of V's output bias that centres adv, the reference's two losses, their statistics, the
per-row adv and every parameter gradient (large tensors as flat[::61] + norm + sum, like make_golden.py's put_grad).  Per
sampling case: the seed whose inputs keep the argmax and the inverse-CDF draw unambiguous, the chosen index and the actions.
One update sequence (V step, Q loss with the updated V, Q step, Polyak).  Weights and inputs are never stored: both sides
rebuild them from make_golden_idql_cases.py.
"""
import copy
import os
import sys
from contextlib import contextmanager

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import dppo_oracle as O  # noqa: E402  (seeded weight recipe + specs only)
from tests.golden import make_golden_idql_cases as K  # noqa: E402
from tests.golden.make_golden import recorded_noise  # noqa: E402
from tests.golden.make_golden_bc import put_grad, save  # noqa: E402

torch.set_num_threads(4)


def ref_model(net, v_bias=0.0, **kw):
    from dppo.model.common.critic import CriticObs, CriticObsAct
    from dppo.model.diffusion.diffusion_idql import IDQLDiffusion
    from dppo.model.diffusion.mlp_diffusion import DiffusionMLP
    od, ta, da = K.shapes(net)
    a = K.actor_spec(net)
    actor = DiffusionMLP(action_dim=da, horizon_steps=ta, cond_dim=od, time_dim=a.time_dim, mlp_dims=list(a.mlp_dims),
                         activation_type=a.activation, residual_style=True)
    if ta == a.horizon_steps:
        actor.load_state_dict(O.init_params(a, K.SEED_ACTOR), strict=True)
    _, residual, double_q = K.IDQL_NETS[net]
    q = CriticObsAct(cond_dim=od, mlp_dims=[256, 256, 256], action_dim=da, action_steps=ta, activation_type="Mish",
                     residual_tyle=residual, double_q=double_q, residual_style=True)  # (the last one is swallowed, as shipped)
    q.load_state_dict(K.twin_params(net), strict=True)
    v = CriticObs(cond_dim=od, mlp_dims=[256, 256, 256], activation_type="Mish", residual_style=True)
    v.load_state_dict(K.v_params(net, v_bias), strict=True)
    m = IDQLDiffusion(actor=actor, critic_q=q, critic_v=v, horizon_steps=ta, obs_dim=od, action_dim=da, device="cpu",
                      **dict(K.SAMPLING_KW, **kw))
    m.target_q.load_state_dict(K.twin_params(net, K.TARGET_EPS), strict=True)
    return m


def advantages(m, obs, act):
    """compute_advantages (the reference's own for a twin; with one trunk it unpacks a tensor, so q = q1 is spelled out)."""
    if hasattr(m.target_q, "Q2"):
        return m.compute_advantages({"state": obs}, act)
    with torch.no_grad():
        q = m.target_q({"state": obs}, act)
    return q - m.critic_v({"state": obs}).reshape(-1)


def loss_q(m, obs, nxt, act, reward, term):
    if hasattr(m.critic_q, "Q2"):
        return m.loss_critic_q({"state": obs}, {"state": nxt}, act, reward, term, K.GAMMA)
    q1 = m.critic_q({"state": obs}, act)
    with torch.no_grad():
        nv = m.critic_v({"state": nxt}).view(-1)
    return torch.mean((q1 - (reward + K.GAMMA * nv * (1 - term))) ** 2)


def put_grads(out, key, module):
    for k, p in module.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), (key, k)
        put_grad(out, f"{key}_{k}", p.grad)


def loss_case(out, net, n):
    from dppo.model.diffusion.diffusion_idql import expectile_loss
    name = f"{net}_{n}"
    obs, nxt, act, reward, term = K.candidates(net, n)
    with torch.no_grad():
        adv0 = advantages(ref_model(net), obs, act)
    shift = float(adv0.median())
    m = ref_model(net, shift)
    with torch.no_grad():
        adv = advantages(m, obs, act)
    keep = torch.nonzero(adv.abs() >= K.ADV_MARGIN * adv.abs().max()).reshape(-1)[:n]
    assert keep.numel() == n, (name, keep.numel())
    pos = float((adv[keep] > 0).float().mean())
    assert K.SIGN_SHARE <= pos <= 1 - K.SIGN_SHARE, (name, pos)
    obs, nxt, act, reward, term = (t[keep] for t in (obs, nxt, act, reward, term))
    assert 0 < term.sum() < n
    adv = advantages(m, obs, act)
    lv = expectile_loss(adv, K.EXPECTILE).mean()
    lv.backward()
    out.update({f"{name}_keep": keep.numpy().astype(np.int32), f"{name}_v_bias": np.float64(shift),
                f"{name}_adv": adv.detach().numpy(), f"{name}_v_loss": np.float64(lv.item()),
                f"{name}_adv_mean": np.float64(adv.double().mean().item()), f"{name}_adv_pos": np.float64(pos)})
    put_grads(out, f"{name}_gv", m.critic_v)
    lq = loss_q(m, obs, nxt, act, reward, term)
    lq.backward()
    with torch.no_grad():
        q1 = m.critic_q({"state": obs}, act)
        q1 = q1[0] if isinstance(q1, tuple) else q1
        tgt = reward + K.GAMMA * m.critic_v({"state": nxt}).view(-1) * (1 - term)
    out.update({f"{name}_q_loss": np.float64(lq.item()), f"{name}_q1_mean": np.float64(q1.double().mean().item()),
                f"{name}_target_mean": np.float64(tgt.double().mean().item())})
    put_grads(out, f"{name}_gq", m.critic_q)
    print(f"  {name}: v_loss {lv.item():.5f} q_loss {lq.item():.5f} adv>0 {pos:.3f} max|adv| {adv.abs().max():.3f} bias {shift:.4f}")
    return m, (obs, nxt, act, reward, term)


def update_sequence(out, m, batch):
    """hopper_77 continued: the V step, then the Q loss WITH THE UPDATED V and its step, then Polyak (reference agent :272-294)."""
    obs, nxt, act, reward, term = batch
    opt_v = torch.optim.AdamW(m.critic_v.parameters(), lr=K.SEQ_LR, weight_decay=0)
    opt_q = torch.optim.AdamW(m.critic_q.parameters(), lr=K.SEQ_LR, weight_decay=0)
    lv = m.loss_critic_v({"state": obs}, act)
    opt_v.zero_grad()
    lv.backward()
    opt_v.step()
    lq = m.loss_critic_q({"state": obs}, {"state": nxt}, act, reward, term, K.GAMMA)
    opt_q.zero_grad()
    lq.backward()
    opt_q.step()
    put_grads(out, "seq_gq", m.critic_q)
    m.update_target_critic(K.SEQ_TAU)
    out.update(seq_v_loss=np.float64(lv.item()), seq_q_loss=np.float64(lq.item()))
    for key, mod in (("seq_v", m.critic_v), ("seq_q", m.critic_q), ("seq_target", m.target_q)):
        for k, p in mod.named_parameters():  # the stepped weights, stored like the gradients (same entries of each tensor)
            put_grad(out, f"{key}_{k}", p)
    print(f"  seq: v_loss {lv.item():.5f} q_loss(updated V) {lq.item():.5f}")


@contextmanager
def inverse_cdf_multinomial(u):
    """torch.multinomial(weights (B, S), 1) as the inverse CDF of the supplied uniforms, in float64."""
    real = torch.multinomial

    def draw(w, k):
        cdf = torch.cumsum(w.double(), 1)
        return (u.double()[:, None] * cdf[:, -1:] >= cdf).sum(1, keepdim=True).clamp(max=w.shape[1] - 1)
    torch.multinomial = draw
    try:
        yield
    finally:
        torch.multinomial = real


def sampling_cases(out):
    from dppo.model.diffusion.diffusion_rwr import RWRDiffusion
    shift = None
    for B, S, det in K.SAMPLING:
        name = f"sample_B{B}_S{S}_{'det' if det else 'sto'}"
        for seed in range(2470, 2670):
            state, noise, u = K.sampling_inputs(B, S, seed)
            m = ref_model("hopper", shift or 0.0)
            rep = state[None].repeat(S, 1, 1, 1).view(S * B, *state.shape[1:])
            with recorded_noise(list(noise)):
                cand = RWRDiffusion.forward(m, {"state": rep}, deterministic=det)
            with torch.no_grad():
                q1, q2 = m.target_q({"state": rep}, cand)
                q = torch.min(q1, q2).view(S, B)
                v = m.critic_v({"state": rep}).view(S, B)
            if shift is None:  # centre adv of the sampled candidates once, for every sampling case
                shift = float((q - v).detach().median())
                v = v + shift
                m = ref_model("hopper", shift)
            top = torch.topk(q, 2, dim=0).values
            gap_ok = bool(((top[0] - top[1]) >= K.GAP_MARGIN * (q.max(0).values - q.min(0).values)).all())
            w = torch.where(q - v > 0, K.CRITIC_HYPERPARAM, 1 - K.CRITIC_HYPERPARAM).double()
            cdf = torch.cumsum(w, 0) / w.sum(0)
            u_ok = bool(((cdf - u.double()[None]).abs() >= K.U_MARGIN).all())
            adv_ok = bool(((q - v).abs() >= 1e-4).all())  # no weight of the draw hangs on a sign an fp32 run could flip
            if gap_ok and (det or (u_ok and adv_ok)):
                break
        else:
            raise AssertionError(name)
        with recorded_noise(list(noise)), inverse_cdf_multinomial(u):
            act = m(cond={"state": state}, deterministic=det, num_sample=S, critic_hyperparam=K.CRITIC_HYPERPARAM,
                    use_expectile_exploration=True)
        cv = cand.view(S, B, -1)
        idx = np.array([int(torch.nonzero((cv[:, b] == act[b].reshape(-1)).all(1))[0]) for b in range(B)], dtype=np.int32)
        if det:
            assert np.array_equal(idx, q.argmax(0).numpy())
        out.update({f"{name}_seed": np.int64(seed), f"{name}_idx": idx, f"{name}_actions": act.numpy()})
        print(f"  {name}: seed {seed} idx {idx[:8]} share adv>0 {float((q - v > 0).float().mean()):.2f}")
    out["sample_v_bias"] = np.float64(shift)


def main():
    out = {}
    for net, n in K.IDQL_CASES:
        m, batch = loss_case(out, net, n)
        if (net, n) == ("hopper", 77):
            update_sequence(out, copy.deepcopy(m), batch)
    sampling_cases(out)
    save("g24_idql", out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    main()
