"""QSM fine-tuning (reference model/diffusion/diffusion_qsm.py, agent/finetune/train_qsm_diffusion_agent.py): the 8 shipped QSM cfgs
resolve, ``QSMDiffusion`` carries the reference's state dict, both new C ABI entries check their arguments, and the plain-torch
restatement of tests/golden/make_golden_qsm_cases.py reproduces the g25 fixture the reference wrote (CPU); on the GPU the TD critic
loss and the actor loss on the critic's action gradient reproduce the reference's losses, statistics, g and every gradient,
``x_t`` is torch's ``q_sample`` bit for bit, repeated / gathered calls are bit-equal, the target call touches no parameter
gradient, and the agent runs the reference's update order.

bf16 bounds.  Measured (profiles/qsm_parity.json, written by tools/qsm_parity_report.py with this module's own helpers): per case,
against the REFERENCE golden, the loss error |loss - ref| / max(1, |ref|), the worst per-tensor gradient error ||g - g_ref|| /
||g_ref|| over the tensors carrying >= 1e-6 of the squared gradient norm, and the cosine of the whole gradient with the golden
over the stored entries -- for the critic loss, the actor loss and g (one tensor, no loss).  Each error bound is 2x the worst
recorded value over the cases; the cosine bound is the worst recorded value minus half its distance to 1 (the rule of
tests/test_idql.py::bf16_bounds).
"""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from dppo_amd.cfg.loader import Cfg, get_class, instantiate, load_config
from oracle import dppo_oracle as O
from tests.golden import make_golden_qsm_cases as K
from tests.test_idql import bf16_errors, check_grads_fp32

T = torch.from_numpy
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SHIPPED = os.path.join(HERE, "golden", "shipped_qsm_cfgs.json")
PARITY = os.path.join(os.path.dirname(HERE), "profiles", "qsm_parity.json")
HOPPER_CFG = "gym/finetune/hopper-v2/ft_qsm_diffusion_mlp.yaml"


def bf16_bounds():
    """From the committed record of the MI355X measurement (profiles/qsm_parity.json, "worst/<what>/bf16"): 2 x the worst loss /
    gradient error over the cases, worst cosine - (1 - worst cosine) / 2."""
    with open(PARITY) as f:
        rec = json.load(f)
    out = {}
    for which in ("critic", "actor", "g"):
        w = rec[f"worst/{which}/bf16"]
        out[which] = dict(loss=2 * w["loss"], grad=2 * w["grad"], cos=w["cos"] - 0.5 * (1 - w["cos"]))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_every_shipped_qsm_cfg_resolves():
    """All 8: agent / model / critic classes, act_steps == horizon_steps, plain Q descriptors of the right width, flat images
    that are what the C ABI counts, and both new workspace queries answer at the cfg's batch size in both precisions."""
    from dppo_amd import hip
    from dppo_amd.agent.finetune.train_qsm_diffusion_agent import TrainQSMDiffusionAgent
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.diffusion.diffusion_qsm import QSMDiffusion
    lib = hip.load()
    cfgs = load_config(SHIPPED)
    assert len(cfgs) == 8 and "gym/scratch/hopper-v2/qsm_diffusion_mlp.yaml" in cfgs
    assert sum(p.endswith("ft_qsm_diffusion_mlp.yaml") for p in cfgs) == 7
    for p in sorted(cfgs):
        cfg = cfgs[p]
        assert get_class(cfg._target_) is TrainQSMDiffusionAgent, p
        assert get_class(cfg.model._target_) is QSMDiffusion, p
        assert get_class(cfg.model.critic._target_) is CriticObsAct, p
        assert cfg.act_steps == cfg.horizon_steps, p
        assert cfg.train.q_grad_coeff > 0, p
        m = instantiate(cfg.model, network_path=None)
        assert type(m) is QSMDiffusion and m.actor is m.network and m.target_q is not m.critic_q, p
        q = m.critic_q
        dq = q.net_desc()
        od = cfg.obs_dim * cfg.cond_steps
        # the shipped ``residual_style: True`` is swallowed by **kwargs: PLAIN Q trunks [To*Do + Ta*Da, 256, 256, 256, 1]
        assert dq.plain == 1 and dq.n_blocks == 2 and dq.hidden == 256 and dq.in_dim == od + cfg.action_dim * cfg.act_steps, p
        assert q.double_q and q.cond_dim == od, p
        for t in q._trunks(bind=False):
            assert lib.dppo_net_param_count(C.byref(t.net_desc())) == sum(x.numel() for x in t.trunk_parameters()), p
        assert q.flat_params().numel() == 2 * lib.dppo_net_param_count(C.byref(dq)) == m.target_q.flat_params().numel(), p
        assert m.actor.flat_params().numel() == lib.dppo_net_param_count(C.byref(m.actor.net_desc())), p
        N = int(cfg.train.batch_size)
        for prec in (hip.PREC_F32, hip.PREC_BF16):
            assert lib.dppo_qsm_actor_target_workspace_bytes(C.byref(dq), prec, od, N) > 0, p
            assert lib.dppo_qsm_q_loss_workspace_bytes(C.byref(dq), prec, od, N) > 0, p


def make_q(net, prec="fp32", **kw):
    from dppo_amd.model.common.critic import CriticObsAct
    od, ta, da, _ = K.shapes(net)
    return CriticObsAct(**dict(dict(cond_dim=od, mlp_dims=[256, 256, 256], action_dim=da, action_steps=ta, activation_type="Mish",
                                    residual_tyle=K.QSM_NETS[net][4], residual_style=True, precision=prec), **kw))


def make_model(net, prec, device):
    from dppo_amd.model.diffusion.diffusion_qsm import QSMDiffusion
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    od, ta, da, steps = K.shapes(net)
    a = K.actor_spec(net)
    actor = DiffusionMLP(da, ta, od, time_dim=a.time_dim, mlp_dims=list(a.mlp_dims), activation_type=a.activation,
                         residual_style=True, precision=prec)
    actor.load_state_dict(K.actor_params(net), strict=True)
    q = make_q(net, prec)
    q.load_state_dict(K.twin_params(net), strict=True)
    m = QSMDiffusion(actor=actor, critic=q, horizon_steps=ta, obs_dim=od, action_dim=da, device=device, denoising_steps=steps,
                     **K.SAMPLING_KW)
    m.target_q.load_state_dict(K.twin_params(net, K.TARGET_EPS), strict=True)
    return m


def test_qsm_state_dict_is_the_references(golden):
    """Keys and shapes are what the reference's QSMDiffusion recorded (g25): network / actor aliases, critic_q, target_q."""
    g = golden("g25_qsm")
    sd = make_model("hopper", "fp32", "cpu").state_dict()
    assert list(sd) == [str(k) for k in g["state_dict_keys"]]
    assert [",".join(str(int(x)) for x in v.shape) for v in sd.values()] == [str(s) for s in g["state_dict_shapes"]]
    assert {k.split(".")[0] for k in sd} == {"network", "actor", "critic_q", "target_q"}


def test_qsm_entries_reject_bad_arguments_on_the_host():
    from dppo_amd import hip
    lib = hip.load()
    X = 4096  # a non-null address no call may touch: every refusal below comes before the first launch
    err = lambda: lib.dppo_last_error().decode()
    dq, dres = make_q("hopper").net_desc(), make_q("hopper_res").net_desc()
    assert dq.plain == 1 and dres.plain == 0
    N, F32 = 64, hip.PREC_F32
    batch = lambda **kw: C.byref(hip.IdqlBatch(**dict(dict(obs=X, next_obs=X, actions=X, reward=X, terminated=X, inds=None, cap=N,
                                                           n_envs=1, head=0, count=N), **kw)))
    wt = lib.dppo_qsm_actor_target_workspace_bytes(C.byref(dq), F32, 11, N)
    wq = lib.dppo_qsm_q_loss_workspace_bytes(C.byref(dq), F32, 11, N)
    assert wq > wt > 0  # two trained trunks and two inference ones > two forwards and a data-gradient chain
    assert lib.dppo_qsm_q_loss_workspace_bytes(C.byref(dres), F32, 11, N) > 0
    assert lib.dppo_qsm_actor_target_workspace_bytes(C.byref(dres), F32, 11, N) == -1 and "plain Q trunks" in err()
    for fn in (lib.dppo_qsm_actor_target_workspace_bytes, lib.dppo_qsm_q_loss_workspace_bytes):
        assert fn(C.byref(dq), F32, 11, 0) == -1 and "N out of range" in err()
        assert fn(C.byref(dq), F32, 23, N) == -1 and "does not pair" in err()
        assert fn(C.byref(dq), F32, 0, N) == -1 and "does not pair" in err()
        assert fn(C.byref(dq), 7, 11, N) == -1
        bad = hip.NetDesc.from_buffer_copy(dq)
        bad.out_dim = 2
        assert fn(C.byref(bad), F32, 11, N) == -1 and "out_dim 1" in err()
        bad = hip.NetDesc.from_buffer_copy(dq)
        bad.act = 5
        assert fn(C.byref(bad), F32, 11, N) == -1 and "activation" in err()

    def t_call(d=dq, qp=X, k2=X, b=None, od=11, N_=N, noise=X, t=X, sa=X, sb=X, steps=20, coeff=10.0, pairs=X, obs_out=X, wsb=wt):
        return lib.dppo_qsm_actor_target(C.byref(d), F32, qp, X, k2, b or batch(), od, N_, noise, t, sa, sb, steps, coeff, pairs,
                                         obs_out, None, X, wsb, None)

    def q_call(d=dq, qp=X, k2=X, tp=X, tk2=X, b=None, od=11, nact=X, N_=N, gamma=0.99, grad=X, stats=X, wsb=wq):
        return lib.dppo_qsm_q_loss_fwd_bwd(C.byref(d), F32, qp, X, k2, tp, X, tk2, b or batch(), od, nact, N_, gamma, grad, stats, X,
                                           wsb, None)
    for call in (t_call, q_call):
        assert call(qp=None) == -1 and "null pointer" in err()
        assert call(k2=None) == -1 and "null pointer" in err()  # always the twin
        assert call(N_=0) == -1 and "N out of range" in err()
        assert call(od=23) == -1 and "does not pair" in err()
        assert call(wsb=(wt if call is t_call else wq) - 256) == -1 and "workspace too small" in err()
        assert call(b=batch(obs=None)) == -1 and "null pointer in batch" in err()
        assert call(b=batch(head=N)) == -1 and "ring geometry" in err()
        assert call(b=batch(count=N + 1)) == -1 and "ring geometry" in err()
        assert call(b=batch(count=N - 1)) == -1 and "stored transitions" in err()
        bad = hip.NetDesc.from_buffer_copy(dq)
        bad.kind = 0
        assert call(d=bad) == -1
    assert t_call(d=dres) == -1 and "plain Q trunks" in err()
    for kw in (dict(noise=None), dict(t=None), dict(sa=None), dict(sb=None), dict(pairs=None), dict(obs_out=None)):
        assert t_call(**kw) == -1 and "null pointer" in err()
    for steps in (0, 1025):
        assert t_call(steps=steps) == -1 and "outside [1, 1024]" in err()
    for coeff in (-1.0, float("nan"), float("inf")):
        assert t_call(coeff=coeff) == -1 and "q_grad_coeff" in err()
    assert t_call(b=batch(reward=None, next_obs=None, terminated=None), wsb=0) == -1 and "workspace" in err()  # never reads them
    for kw in (dict(tp=None), dict(tk2=None), dict(nact=None), dict(grad=None), dict(stats=None)):
        assert q_call(**kw) == -1 and "null pointer" in err()
    assert q_call(b=batch(reward=None)) == -1 and "null pointer in batch" in err()
    for gamma in (-0.01, 1.01, float("nan")):
        assert q_call(gamma=gamma) == -1 and "outside [0, 1]" in err()
    assert q_call(d=dres, wsb=0) == -1 and "workspace too small" in err()  # a residual twin is accepted here


def test_qsm_model_refuses_what_the_reference_refuses():
    from dppo_amd import hip
    from dppo_amd.model.diffusion.diffusion_qsm import QSMDiffusion
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    mk = lambda critic=None, **kw: QSMDiffusion(actor=DiffusionMLP(3, 4, 11, mlp_dims=[512, 512, 512], residual_style=True),
                                                critic=critic or make_q("hopper"), horizon_steps=4, obs_dim=11, action_dim=3,
                                                device="cpu", denoising_steps=20, **kw)
    with pytest.raises(AssertionError, match="DDIM"):
        mk(use_ddim=True, ddim_steps=5)
    with pytest.raises(ValueError, match="twin critic"):
        mk(critic=make_q("hopper", double_q=False))
    m = mk()
    assert m.min_sampling_denoising_std == 0.1 and m.actor is m.network
    with pytest.raises(NotImplementedError, match="state observations"):
        m(cond={"state": torch.zeros(2, 1, 11), "rgb": torch.zeros(2, 1, 3, 8, 8)})
    with pytest.raises(NotImplementedError, match="state observations"):
        m.loss_actor({"state": torch.zeros(2, 1, 11), "rgb": torch.zeros(2, 1, 3, 8, 8)}, torch.zeros(2, 4, 3), 10.0)
    with pytest.raises(hip.DppoHipError):  # no CPU fallback
        m(cond={"state": torch.zeros(2, 1, 11)})
    with pytest.raises(hip.DppoHipError):
        m.loss_actor({"state": torch.zeros(2, 1, 11)}, torch.zeros(2, 4, 3), 10.0)


def close_to_fixture(g, key, x, what):
    """|x - g25| <= 1e-5 relative to the tensor's largest entry (DESIGN section 2's oracle bar); large tensors by their stored
    flat[::61] entries and their norm."""
    x = x.detach().double().cpu().numpy() if torch.is_tensor(x) else np.float64(x)
    if key in g:
        ref = g[key].astype(np.float64)
        assert np.abs(x.reshape(ref.shape) - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-30), (what, key)
    else:
        ref = g[key + "__sub"].astype(np.float64)
        assert np.abs(x.reshape(-1)[::61] - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-30), (what, key)
        assert np.linalg.norm(x) == pytest.approx(float(g[key + "__norm"]), rel=1e-5), (what, key)


def test_restatement_reproduces_the_reference_fixture(golden):
    """make_golden_qsm_cases.py's plain-torch QSM on the oracle's forwards against every value the reference recorded in g25:
    the fixture is pinned without a GPU and without the reference."""
    g = golden("g25_qsm")
    for net, n in K.CRITIC_CASES:
        name, b = f"{net}_{n}", K.inputs(net, n)
        q = K.leaf(K.twin_params(net))
        lc, q1m, ym = K.critic_loss(q, K.twin_params(net, K.TARGET_EPS), net, b)
        for key, v in ((f"{name}_c_loss", lc), (f"{name}_q1_mean", q1m), (f"{name}_y_mean", ym)):
            close_to_fixture(g, key, v, "critic")
        for (k, _), gr in zip(q.items(), torch.autograd.grad(lc, list(q.values()))):
            close_to_fixture(g, f"{name}_gq_{k}", gr, "critic gradient")
    for net, n in K.ACTOR_CASES:
        name, b = f"{net}_{n}", K.inputs(net, n)
        a = K.leaf(K.actor_params(net))
        la, gq = K.actor_loss(a, K.twin_params(net), net, b)
        close_to_fixture(g, f"{name}_a_loss", la, "actor")
        close_to_fixture(g, f"{name}_g", gq.reshape(n, -1), "g")
        for (k, _), gr in zip(a.items(), torch.autograd.grad(la, list(a.values()))):
            close_to_fixture(g, f"{name}_ga_{k}", gr, "actor gradient")
    seq = K.restate_sequence("hopper", K.inputs("hopper", 77))
    close_to_fixture(g, "seq_c_loss", seq["c_loss"], "seq")
    close_to_fixture(g, "seq_a_loss", seq["a_loss"], "seq")
    assert float(g["seq_a_loss"]) != float(g["hopper_77_a_loss"])  # the stepped critic moved g
    for key in ("gq", "ga", "q", "actor", "target"):
        for k, v in seq[key].items():
            close_to_fixture(g, f"seq_{key}_{k}", v, "seq")


# ---------------------------------------------------------------------------------------------------------------- GPU
def dev_batch(net, n):
    return {k: v.to(DEV) for k, v in K.inputs(net, n).items()}


def named_grads(module, flat):
    out, off = [], 0
    for (k, p), q in zip(module.named_parameters(), module.trunk_parameters()):
        assert p is q, k  # the flat image is the parameters in this order
        out.append((k, flat[off:off + p.numel()].view(p.shape)))
        off += p.numel()
    assert off == flat.numel()
    return out


def run_critic(m, b, inds=None, replay=None, rows=slice(None), **kw):
    src = replay if replay is not None else {"state": b["obs"][rows]}
    loss = m.loss_critic(src, {"state": b["next_obs"][rows]}, b["actions"][rows], b["reward"][rows], b["terminated"][rows], K.GAMMA,
                         inds=inds, **dict(dict(next_actions=b["next_actions"][rows]), **kw))
    return dict(c_loss=loss.detach().clone(), c_stats=m.last_stats.clone(), gq=m.critic_q.flat_grads().clone())


def run_actor(m, net, b, inds=None, replay=None, rows=slice(None)):
    src = replay if replay is not None else {"state": b["obs"][rows]}
    loss = m.loss_actor(src, b["actions"][rows], K.coeff(net), inds=inds, noise=b["noise"][rows], t=b["t"][rows], want_grad=True)
    return dict(a_loss=loss.detach().clone(), g=m.last_q_grad.clone(), pairs=m.last_pairs.clone(), ga=m.last_loss_grad.clone())


def ring_of(b, n, E=5):
    """The n rows of ``b`` scattered into a ring of E envs with more steps than they need, its oldest step in slot 3
    (test_hip_idql_losses_fp32's construction) -> (DeviceReplay, inds)."""
    from dppo_amd.util.replay import DeviceReplay
    cap = (n + E - 1) // E + 3
    rp = DeviceReplay(cap, E, b["obs"][0].numel(), b["actions"][0].numel(), device=DEV)
    rp.head, rp.steps = 3, cap - 1
    inds = T(np.random.RandomState(n).permutation(rp.steps * E)[:n].astype(np.int64)).to(DEV)
    rows = rp.slot_of(inds)
    for dst, key in ((rp.obs, "obs"), (rp.next_obs, "next_obs"), (rp.actions, "actions"), (rp.reward, "reward"),
                     (rp.terminated, "terminated")):
        dst.view(cap * E, -1)[rows] = b[key].reshape(n, -1)
    return rp, inds


@pytest.mark.gpu
@pytest.mark.parametrize("net,n", K.CRITIC_CASES, ids=[f"{a}_{b}" for a, b in K.CRITIC_CASES])
def test_hip_qsm_losses_fp32(golden, net, n):
    """loss_critic and (plain twins) loss_actor against the reference on every g25 case: losses, statistics, g and every
    gradient; pairs[:, 0] is torch's q_sample and pairs[:, 1] is -(float)coeff * g, bit for bit; two calls are bit-equal; a
    gathered call (indices into a ring with head != 0) equals the contiguous one bit for bit."""
    g, name = golden("g25_qsm"), f"{net}_{n}"
    m, b = make_model(net, "fp32", DEV), dev_batch(net, n)
    res = run_critic(m, b)
    got = np.array([float(res["c_loss"])] + res["c_stats"].tolist())
    want = np.array([g[f"{name}_c_loss"], g[f"{name}_c_loss"], g[f"{name}_q1_mean"], g[f"{name}_y_mean"]], dtype=np.float64)
    print(f"{name}: critic {got} ref {want}")
    np.testing.assert_allclose(got, want, rtol=2e-4, atol=2e-5)
    check_grads_fp32(g, f"{name}_gq", named_grads(m.critic_q, res["gq"]))
    assert all(torch.equal(res[k], v) for k, v in run_critic(m, b).items())
    rp, inds = ring_of(b, n)
    ring = run_critic(m, b, inds=inds, replay=rp)
    assert all(torch.equal(res[k], ring[k]) for k in res), [k for k in res if not torch.equal(res[k], ring[k])]
    if (net, n) not in K.ACTOR_CASES:
        return
    act = run_actor(m, net, b)
    gref = g[f"{name}_g"] if f"{name}_g" in g else None
    print(f"{name}: actor loss {float(act['a_loss'])!r} ref {float(g[name + '_a_loss'])!r}" +
          (f" max |g - ref| {np.abs(act['g'].cpu().numpy() - gref).max():.3e}" if gref is not None else ""))
    np.testing.assert_allclose(float(act["a_loss"]), float(g[f"{name}_a_loss"]), rtol=2e-4, atol=2e-5)
    check_grads_fp32(g, name, [("g", act["g"])])
    check_grads_fp32(g, f"{name}_ga", named_grads(m.actor, act["ga"]))
    cpu = K.inputs(net, n)
    x_t = make_model(net, "fp32", "cpu").q_sample(cpu["actions"], cpu["t"], cpu["noise"])
    assert torch.equal(act["pairs"][:, 0].cpu(), x_t.reshape(n, -1))
    assert np.array_equal(act["pairs"][:, 1].cpu().numpy(), -np.float32(K.coeff(net)) * act["g"].cpu().numpy())
    assert all(torch.equal(act[k], v) for k, v in run_actor(m, net, b).items())
    ring = run_actor(m, net, b, inds=inds, replay=rp)
    assert all(torch.equal(act[k], ring[k]) for k in act), [k for k in act if not torch.equal(act[k], ring[k])]


@pytest.mark.gpu
@pytest.mark.parametrize("net", ["hopper", "transport", "hopper_res"])
def test_hip_qsm_half_batches_add_up(net):
    """g is per row: rows 0..37 and 38..76 computed in two calls equal the 77-row call's rows at the fp32 gradient rule (a tail-row
    or tile-boundary error shows here).  The critic's flat gradient: mean over 77 = (38 * first + 39 * rest) / 77, tensor by tensor
    at test_hip_idql_half_batches_add_up's rule (rtol 1e-5, atol 1e-5 of the tensor's rms)."""
    m, b = make_model(net, "fp32", DEV), dev_batch(net, 77)
    lo, hi = slice(0, 38), slice(38, 77)
    if net != "hopper_res":  # (no action gradient of a residual twin)
        whole = run_actor(m, net, b)["g"].cpu().numpy()
        parts = np.concatenate([run_actor(m, net, b, rows=lo)["g"].cpu().numpy(), run_actor(m, net, b, rows=hi)["g"].cpu().numpy()])
        atol = 2e-4 * float(np.linalg.norm(whole)) / np.sqrt(whole.size) + 1e-7
        print(f"g halves: max |diff| {np.abs(parts - whole).max():.3e} (atol {atol:.3e})")
        np.testing.assert_allclose(parts, whole, rtol=2e-3, atol=atol)
    whole = run_critic(m, b)["gq"]
    both = (38.0 * run_critic(m, b, rows=lo)["gq"].double() + 39.0 * run_critic(m, b, rows=hi)["gq"].double()) / 77.0
    for (name, x), (_, w) in zip(named_grads(m.critic_q, both), named_grads(m.critic_q, whole)):
        x, w = x.cpu().numpy(), w.double().cpu().numpy()
        rms = float(np.sqrt(np.mean(w * w)))
        assert rms > 0, name
        np.testing.assert_allclose(x, w, rtol=1e-5, atol=1e-5 * rms, err_msg=name)


@pytest.mark.gpu
def test_hip_qsm_target_call_touches_no_parameter_gradient():
    m, b = make_model("hopper", "fp32", DEV), dev_batch("hopper", 77)
    m.critic_q.flat_grads().fill_(7.0)
    m.target_q.flat_grads().fill_(7.0)
    loss = m.loss_actor({"state": b["obs"]}, b["actions"], 10.0, noise=b["noise"], t=b["t"])
    assert np.isfinite(float(loss.detach()))
    assert bool((m.critic_q.flat_grads() == 7.0).all()) and bool((m.target_q.flat_grads() == 7.0).all())
    # and with its own draws the loss is a different, finite number
    assert np.isfinite(float(m.loss_actor({"state": b["obs"]}, b["actions"], 10.0).detach())) and m.last_q_grad is None


@pytest.mark.gpu
def test_hip_qsm_loss_critic_samples_next_actions_with_forward():
    """next_actions=None: a' = forward({"state": gathered next_obs}) -- with the sampler's noise given, bit-equal to passing it."""
    net, n = "hopper", 77
    m, b = make_model(net, "fp32", DEV), dev_batch(net, n)
    noise = torch.randn(K.shapes(net)[3] + 1, n, 4, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    nact = m.forward({"state": b["next_obs"]}, noise=noise)
    assert nact.shape == (n, 4, 3) and torch.equal(nact, m(cond={"state": b["next_obs"]}, deterministic=False, noise=noise))
    want = run_critic(m, b, next_actions=nact)
    got = run_critic(m, b, next_actions=None, noise=noise)
    assert all(torch.equal(want[k], got[k]) for k in want)
    rp, inds = ring_of(b, n)
    ring = run_critic(m, b, inds=inds, replay=rp, next_actions=None, noise=noise)
    assert all(torch.equal(want[k], ring[k]) for k in want)
    assert not torch.equal(want["c_loss"], run_critic(m, b)["c_loss"])  # (the recipe's next_actions are other actions)


def qsm_errors(g, net, n, m, crit, act):
    """{"critic": ..., "actor": ..., "g": ...} of one run against g25, in bf16_errors' terms."""
    name = f"{net}_{n}"
    out = {"critic": bf16_errors(g, f"{name}_gq", named_grads(m.critic_q, crit["gq"]), float(crit["c_loss"]), float(g[f"{name}_c_loss"]))}
    if act is not None:
        out["actor"] = bf16_errors(g, f"{name}_ga", named_grads(m.actor, act["ga"]), float(act["a_loss"]), float(g[f"{name}_a_loss"]))
        out["g"] = bf16_errors(g, name, [("g", act["g"])], 0.0, 0.0)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("net,n", K.CRITIC_CASES, ids=[f"{a}_{b}" for a, b in K.CRITIC_CASES])
def test_hip_qsm_losses_bf16(golden, net, n):
    g = golden("g25_qsm")
    m, b = make_model(net, "bf16", DEV), dev_batch(net, n)
    crit = run_critic(m, b)
    act = run_actor(m, net, b) if (net, n) in K.ACTOR_CASES else None
    errs = qsm_errors(g, net, n, m, crit, act)
    print(f"{net}_{n} bf16: {errs}")
    bounds = bf16_bounds()
    for which, e in errs.items():
        bd = bounds[which]
        assert e["loss"] <= bd["loss"] and e["grad"] <= bd["grad"] and e["cos"] >= bd["cos"], (which, e, bd)


def agent_cfg(tmp_path, **train):
    cfg = copy.deepcopy(load_config(SHIPPED)[HOPPER_CFG])
    cfg.update(device=DEV, seed=42, logdir=str(tmp_path), env=Cfg(n_envs=8, name="synthetic", max_episode_steps=5, reset_at_iteration=False))
    cfg.pop("wandb", None)
    cfg.model.update(device=DEV, network_path=None)
    for node in (cfg.model.actor, cfg.model.critic):
        node["precision"] = "fp32"
    cfg.train.update(dict(n_train_itr=3, n_critic_warmup_itr=1, n_steps=4, batch_size=16, replay_ratio=2, buffer_size=3, val_freq=100,
                          force_train=True, save_model_freq=100), **train)
    return cfg


@pytest.mark.gpu
def test_hip_qsm_agent_runs_the_reference_update_order(tmp_path):
    """hopper cfg shrunk (8 envs, 4 steps, batch 16, replay_ratio 2, ring of 3 steps, 3 iterations, 1 warm-up): the run completes;
    during the warm-up iteration the actor's loss and gradient are computed but its parameters do not move, afterwards they do;
    after every minibatch the target is the Polyak recurrence of its previous value and the freshly stepped critic; a checkpoint
    round-trips."""
    from dppo_amd.agent.finetune.train_qsm_diffusion_agent import TrainQSMDiffusionAgent
    agent = TrainQSMDiffusionAgent(agent_cfg(tmp_path))
    m = agent.model
    assert agent.replay.cap == 3 and m.critic_q.net_desc().plain == 1 and agent.q_grad_coeff == 10
    actor0, critic0 = m.actor.flat_params().clone(), m.critic_q.flat_params().clone()
    actor_after, polyak_ok, warm = {}, [], []
    inner = agent.update_minibatch

    def spy(inds, **kw):
        before, a_before = m.target_q.flat_params().clone(), m.actor.flat_params().clone()
        out = inner(inds, **kw)
        tau = agent.critic_tau
        want = before.cpu() * (1.0 - tau) + m.critic_q.flat_params().cpu() * tau
        polyak_ok.append(torch.equal(m.target_q.flat_params().cpu(), want))
        actor_after[agent.itr] = m.actor.flat_params().clone()
        if agent.itr < agent.n_critic_warmup_itr:  # the loss and its gradient exist, the step was not taken
            warm.append(bool(torch.isfinite(out[1])) and bool(m.last_loss_grad.abs().sum() > 0) and
                        torch.equal(m.actor.flat_params(), a_before))
        return out
    agent.update_minibatch = spy
    res = agent.run()
    assert [r["itr"] for r in res] == [0, 1, 2] and all(np.isfinite(r["loss_actor"]) and np.isfinite(r["loss_critic"]) for r in res)
    assert len(polyak_ok) == 3 * int(4 * 8 / 16 * 2) and all(polyak_ok)
    assert len(warm) == 4 and all(warm)
    assert torch.equal(actor_after[0], actor0) and not torch.equal(actor_after[1], actor0)
    assert not torch.equal(m.critic_q.flat_params(), critic0)
    assert agent.replay.steps == 3 and agent.replay.head == (3 * 4) % 3
    assert not torch.equal(m.target_q.flat_params(), m.critic_q.flat_params())
    data = torch.load(os.path.join(str(tmp_path), "checkpoint", "state_2.pt"), weights_only=True)
    assert set(data) == {"itr", "model"} and data["itr"] == 2
    assert {k.split(".")[0] for k in data["model"]} == {"network", "actor", "critic_q", "target_q"}
    assert "critic_q.Q2.moduleList.3.linear_1.bias" in data["model"]
    other = TrainQSMDiffusionAgent(agent_cfg(tmp_path, n_train_itr=0))
    other.load(2)
    for a, b in ((other.model.actor, m.actor), (other.model.critic_q, m.critic_q), (other.model.target_q, m.target_q)):
        assert torch.equal(a.flat_params(), b.flat_params())
    st, nz = torch.zeros(8, 1, 11, device=DEV), torch.randn(21, 8, 4, 3, device=DEV)
    assert torch.equal(other.model(cond={"state": st}, noise=nz), m(cond={"state": st}, noise=nz))


@pytest.mark.gpu
def test_hip_qsm_agent_minibatch_is_the_recorded_sequence(golden, tmp_path):
    """One fp32 ``update_minibatch`` on the hopper_77 rows against the sequence the reference recorded: critic loss and AdamW step,
    then the actor loss WITH THE UPDATED critic (its value differs from the stand-alone case's), the actor's step, and the
    Polyak average of the stepped critic -- at test_hip_idql_agent_minibatch_is_the_recorded_sequence's tolerances."""
    from dppo_amd.agent.finetune.train_qsm_diffusion_agent import TrainQSMDiffusionAgent
    from dppo_amd.util.optim import FlatAdamW
    from dppo_amd.util.replay import DeviceReplay
    g = golden("g25_qsm")
    agent = TrainQSMDiffusionAgent(agent_cfg(tmp_path, n_train_itr=0, n_critic_warmup_itr=0, critic_tau=K.SEQ_TAU))
    m = agent.model = make_model("hopper", "fp32", DEV)
    agent.gamma, agent.q_grad_coeff, agent.max_grad_norm = K.GAMMA, K.coeff("hopper"), None
    agent.critic_optimizer = FlatAdamW(m.critic_q.flat_params(), lr=K.SEQ_LR, weight_decay=0)
    agent.actor_optimizer = FlatAdamW(m.actor.flat_params(), lr=K.SEQ_ACTOR_LR, weight_decay=0)
    b = dev_batch("hopper", 77)
    rp = agent.replay = DeviceReplay(77, 1, 11, 12, device=DEV)
    for dst, key in ((rp.obs, "obs"), (rp.next_obs, "next_obs"), (rp.actions, "actions"), (rp.reward, "reward"),
                     (rp.terminated, "terminated")):
        dst.copy_(b[key].reshape(dst.shape))
    rp.steps = 77
    lc, la = agent.update_minibatch(torch.arange(77, device=DEV), next_actions=b["next_actions"], noise=b["noise"], t=b["t"])
    print(f"seq: critic {float(lc)!r} ref {float(g['seq_c_loss'])!r}; actor {float(la)!r} ref {float(g['seq_a_loss'])!r}")
    assert float(g["seq_a_loss"]) != float(g["hopper_77_a_loss"])  # the stepped critic moved g
    np.testing.assert_allclose([float(lc), float(la)], [float(g["seq_c_loss"]), float(g["seq_a_loss"])], rtol=2e-4, atol=2e-5)
    check_grads_fp32(g, "seq_gq", named_grads(m.critic_q, m.critic_q.flat_grads()))
    check_grads_fp32(g, "seq_ga", named_grads(m.actor, m.last_loss_grad))
    # AdamW's first step is lr * g / (|g| + eps): an entry whose gradient is off by dg moves off by lr * dg / (|g| + eps), with dg
    # from the gradient rule above (rtol 2e-3, the tensor's atol) -- and by at most 2 lr whatever the gradient; the target moves
    # by tau times the critic's step.  Plus one ulp-class term for the weight itself.
    for key, net, gkey, step in (("seq_q", m.critic_q, "seq_gq", K.SEQ_LR), ("seq_actor", m.actor, "seq_ga", K.SEQ_ACTOR_LR),
                                 ("seq_target", m.target_q, "seq_gq", K.SEQ_LR * K.SEQ_TAU)):
        for k, p in net.named_parameters():
            x = p.detach().cpu().numpy()
            if f"{key}_{k}" in g:
                ref, xs, gref = g[f"{key}_{k}"], x, g[f"{gkey}_{k}"]
                gn = float(np.linalg.norm(gref))
            else:
                ref, xs, gref, gn = g[f"{key}_{k}__sub"], x.reshape(-1)[::61], g[f"{gkey}_{k}__sub"], float(g[f"{gkey}_{k}__norm"])
            atol_g = 2e-4 * max(gn, 1e-8) / np.sqrt(x.size) + 1e-7
            tol = step * np.minimum(2.0, 2e-3 + atol_g / (np.abs(gref) + 1e-8)) + 1e-6 * np.abs(ref) + 1e-7
            assert (np.abs(xs - ref) <= tol).all(), (key, k, float(np.abs(xs - ref).max()))
            assert (np.abs(xs - ref) <= step * 1e-2 + 1e-6 * np.abs(ref) + 1e-7).mean() > 0.99, (key, k)  # and nearly all are tight
