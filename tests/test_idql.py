"""IDQL fine-tuning (reference model/diffusion/diffusion_idql.py, model/common/critic.py:57-113,
agent/finetune/train_idql_diffusion_agent.py): the 7 shipped ft_idql_diffusion_mlp cfgs resolve, ``CriticObsAct`` carries the
reference's state dict (``residual_tyle`` typo included), every new C ABI entry checks its arguments and ``DeviceReplay`` maps
indices like the reference's deques (CPU); on the GPU the twin-Q / expectile-V losses reproduce the reference's losses,
statistics, per-row advantages and every gradient (g24 fixture, tests/golden/make_golden_idql.py), the Polyak average is the
torch expression bit for bit, the selection kernel picks what a numpy restatement picks, ``IDQLDiffusion.forward`` returns the
golden candidate, and the agent runs the reference's update order.

bf16 bounds.  The project had no number for these losses in bf16, so they are measured (profiles/idql_parity.json, written by
tools/idql_parity_report.py with this module's own helpers): per case, against the REFERENCE golden, the loss error
|loss - ref| / max(1, |ref|), the worst per-tensor gradient error ||g - g_ref|| / ||g_ref|| over the tensors carrying >= 1e-6 of
the squared gradient norm, and the cosine of the whole gradient with the golden over the stored entries.  Each error bound is
2x the worst recorded value over the cases; the cosine bound is the worst recorded value minus half its distance to 1 (the rule
of tests/test_pretrain_gaussian.py).  Before any of them, sign(adv) must agree with the reference on EVERY row: the fixture
keeps a margin of 10 % of max |adv| for exactly that.
"""
import collections
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from dppo_amd.cfg.loader import Cfg, get_class, instantiate, load_config
from oracle import dppo_oracle as O
from tests.golden import make_golden_idql_cases as K

T = torch.from_numpy
DEV = "cuda:0"
SHIPPED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shipped_idql_cfgs.json")

PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "idql_parity.json")


def bf16_bounds():
    """From the committed record of the MI355X measurement (profiles/idql_parity.json, "worst/<loss>/bf16"), by the rule above:
    2 x the worst loss / gradient error over the ten cases, worst cosine - (1 - worst cosine) / 2."""
    import json
    with open(PARITY) as f:
        rec = json.load(f)
    out = {}
    for which in ("v", "q"):
        w = rec[f"worst/{which}/bf16"]
        out[which] = dict(loss=2 * w["loss"], grad=2 * w["grad"], cos=w["cos"] - 0.5 * (1 - w["cos"]))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_every_shipped_idql_cfg_resolves():
    """All 7: agent / model / critic classes, the flat image of every trunk is what the C ABI counts, and the three workspace
    queries answer at the cfg's batch size (and the sampling query at n_envs * eval_sample_num) in both precisions."""
    from dppo_amd import hip
    from dppo_amd.agent.finetune.train_idql_diffusion_agent import TrainIDQLDiffusionAgent
    from dppo_amd.model.common.critic import CriticObs, CriticObsAct
    from dppo_amd.model.diffusion.diffusion_idql import IDQLDiffusion
    lib = hip.load()
    cfgs = load_config(SHIPPED)
    assert len(cfgs) == 7
    for p in sorted(cfgs):
        cfg = cfgs[p]
        assert get_class(cfg._target_) is TrainIDQLDiffusionAgent, p
        assert get_class(cfg.model._target_) is IDQLDiffusion, p
        assert get_class(cfg.model.critic_q._target_) is CriticObsAct and get_class(cfg.model.critic_v._target_) is CriticObs, p
        assert cfg.act_steps == cfg.horizon_steps, p
        m = instantiate(cfg.model, network_path=None)
        assert type(m) is IDQLDiffusion and m.actor is m.network and m.target_q is not m.critic_q, p
        q, v = m.critic_q, m.critic_v
        dq, dv = q.net_desc(), v.net_desc()
        # the shipped ``residual_style: True`` is swallowed by **kwargs: PLAIN Q trunks [To*Do + Ta*Da, 256, 256, 256, 1]
        assert dq.plain == 1 and dq.n_blocks == 2 and dq.in_dim == cfg.obs_dim * cfg.cond_steps + cfg.action_dim * cfg.act_steps, p
        assert dv.plain == 0 and dv.in_dim == cfg.obs_dim * cfg.cond_steps, p
        for t in q._trunks(bind=False):
            assert lib.dppo_net_param_count(C.byref(t.net_desc())) == sum(x.numel() for x in t.trunk_parameters()), p
        assert q.flat_params().numel() == 2 * lib.dppo_net_param_count(C.byref(dq)) == m.target_q.flat_params().numel(), p
        assert v.flat_params().numel() == lib.dppo_net_param_count(C.byref(dv)), p
        assert m.actor.flat_params().numel() == lib.dppo_net_param_count(C.byref(m.actor.net_desc())), p
        N, rows = int(cfg.train.batch_size), int(cfg.env.n_envs) * int(cfg.train.eval_sample_num)
        for prec in (hip.PREC_F32, hip.PREC_BF16):
            assert lib.dppo_idql_v_loss_workspace_bytes(C.byref(dq), C.byref(dv), prec, N, 1) > 0, p
            assert lib.dppo_idql_q_loss_workspace_bytes(C.byref(dq), C.byref(dv), prec, N, 1) > 0, p
            assert lib.dppo_idql_q_forward_workspace_bytes(C.byref(dq), prec, rows, 1) > 0, p


def make_q(net, prec="fp32"):
    from dppo_amd.model.common.critic import CriticObsAct
    od, ta, da = K.shapes(net)
    _, residual, double_q = K.IDQL_NETS[net]
    return CriticObsAct(cond_dim=od, mlp_dims=[256, 256, 256], action_dim=da, action_steps=ta, activation_type="Mish",
                        residual_tyle=residual, double_q=double_q, residual_style=True, precision=prec)


@pytest.mark.parametrize("net", ["hopper", "hopper_res", "hopper_single"])
def test_critic_obs_act_state_dict_is_the_references(golden, net):
    """Keys = the parameter names the reference module recorded its gradients under (g24), shapes = the trunk's; a deep copy
    is an independent target."""
    g = golden("g24_idql")
    q = make_q(net)
    sd = q.state_dict()
    names = list(dict.fromkeys(k[len(f"{net}_77_gq_"):].split("__")[0] for k in g if k.startswith(f"{net}_77_gq_")))
    assert list(sd) == names
    shapes = {n.replace("Q1.", pre): s for pre in ("Q1.", "Q2.") for n, s, _ in O.param_shapes(K.q_spec(net))}
    assert all(tuple(sd[k].shape) == shapes[k] for k in sd)
    plain = not K.IDQL_NETS[net][1]
    assert ("Q1.moduleList.0.linear_1.weight" in sd) == plain and ("Q1.layers.0.weight" in sd) == (not plain)
    assert ("Q2.moduleList.0.linear_1.weight" in sd) == (net == "hopper")
    q.load_state_dict(K.twin_params(net), strict=True)
    t = copy.deepcopy(q)
    assert torch.equal(t.flat_params(), q.flat_params()) and t.flat_params().data_ptr() != q.flat_params().data_ptr()
    t.flat_params().add_(1.0)
    assert not torch.equal(t.state_dict()[names[0]], q.state_dict()[names[0]])
    assert all(a._flat.data_ptr() != b._flat.data_ptr() for a, b in zip(t._trunks(), q._trunks()))


def test_idql_entries_reject_bad_arguments_on_the_host():
    from dppo_amd import hip
    lib = hip.load()
    X = 4096  # a non-null address no call may touch: every refusal below comes before the first launch
    err = lambda: lib.dppo_last_error().decode()
    q = make_q("hopper")
    dq = q.net_desc()
    dv = hip.NetDesc(kind=1, in_dim=11, hidden=256, n_blocks=1, out_dim=1, act=hip.ACT_MISH, time_dim=0, act_flat=0, cond_dim=11,
                     cond_hidden=0, cond_out=0)
    N, F32 = 64, hip.PREC_F32
    batch = lambda **kw: C.byref(hip.IdqlBatch(**dict(dict(obs=X, next_obs=X, actions=X, reward=X, terminated=X, inds=None, cap=N,
                                                           n_envs=1, head=0, count=N), **kw)))
    wv = lib.dppo_idql_v_loss_workspace_bytes(C.byref(dq), C.byref(dv), F32, N, 1)
    wq = lib.dppo_idql_q_loss_workspace_bytes(C.byref(dq), C.byref(dv), F32, N, 1)
    wf = lib.dppo_idql_q_forward_workspace_bytes(C.byref(dq), F32, N, 1)
    assert wq > wv > wf > 0  # two trained trunks > one > none
    assert lib.dppo_idql_v_loss_workspace_bytes(C.byref(dq), C.byref(dv), F32, N, 0) < wv
    for fn in (lib.dppo_idql_v_loss_workspace_bytes, lib.dppo_idql_q_loss_workspace_bytes):
        assert fn(C.byref(dq), C.byref(dv), F32, 0, 1) == -1 and "N out of range" in err()
        assert fn(C.byref(dv), C.byref(dv), F32, N, 1) == -1 and "do not pair" in err()
        assert fn(C.byref(dq), C.byref(dv), 7, N, 1) == -1
    assert lib.dppo_idql_q_forward_workspace_bytes(C.byref(dq), F32, 0, 1) == -1 and "N out of range" in err()

    def v_call(dq_=dq, dv_=dv, tp=X, k2=X, b=None, N_=N, tau=0.8, grad=X, stats=X, wsb=wv, twin=1):
        return lib.dppo_idql_v_loss_fwd_bwd(C.byref(dq_), C.byref(dv_), F32, tp, X, k2, X, X, b or batch(), N_, tau, twin, grad, None,
                                            stats, X, wsb, None)

    def q_call(dq_=dq, dv_=dv, qp=X, k2=X, b=None, N_=N, gamma=0.99, grad=X, stats=X, wsb=wq, twin=1):
        return lib.dppo_idql_q_loss_fwd_bwd(C.byref(dq_), C.byref(dv_), F32, qp, X, k2, X, X, b or batch(), N_, gamma, twin, grad,
                                            stats, X, wsb, None)
    for call in (v_call, q_call):
        assert call(**{("tp" if call is v_call else "qp"): None}) == -1 and "null pointer" in err()
        assert call(k2=None) == -1 and "null pointer" in err()  # a twin needs the second image ...
        assert call(grad=None) == -1 and "null pointer" in err()
        assert call(stats=None) == -1 and "null pointer" in err()
        assert call(N_=0) == -1 and "N out of range" in err()
        assert call(wsb=(wv if call is v_call else wq) - 256) == -1 and "workspace too small" in err()
        assert call(dq_=dv) == -1 and "do not pair" in err()
        bad = hip.NetDesc.from_buffer_copy(dv)
        bad.out_dim = 2
        assert call(dv_=bad) == -1 and "out_dim 1" in err()
        assert call(b=batch(obs=None)) == -1 and "null pointer in batch" in err()
        assert call(b=batch(head=N)) == -1 and "ring geometry" in err()
        assert call(b=batch(count=N + 1)) == -1 and "ring geometry" in err()
        assert call(b=batch(count=N - 1)) == -1 and "stored transitions" in err()  # identity order over fewer rows than N
        assert call(b=batch(count=N - 1, inds=X), wsb=0) == -1 and "workspace too small" in err()  # (gathered: passes that check)
    assert q_call(b=batch(reward=None)) == -1 and "null pointer in batch" in err()
    assert v_call(b=batch(reward=None, next_obs=None, terminated=None), wsb=0) == -1 and "workspace" in err()  # V never reads them
    for tau in (-0.01, 1.01, float("nan")):
        assert v_call(tau=tau) == -1 and "outside [0, 1]" in err()
        assert q_call(gamma=tau) == -1 and "outside [0, 1]" in err()
        assert lib.dppo_polyak(X, X, tau, 8, None) == -1 and "outside [0, 1]" in err()
        assert lib.dppo_idql_select(X, X, X, 0, X, X, 8, 4, 12, 1, tau, 0, X, X, None) == -1 and "outside [0, 1]" in err()
    assert lib.dppo_polyak(None, X, 0.5, 8, None) == -1 and "null pointer" in err()
    assert lib.dppo_polyak(X, None, 0.5, 8, None) == -1 and "null pointer" in err()
    assert lib.dppo_polyak(X, X, 0.5, 0, None) == -1 and "n out of range" in err()

    def f_call(d=dq, qp=X, k2=X, od=11, rows=N, N_=N, q2=X, wsb=wf):
        return lib.dppo_idql_q_forward(C.byref(d), F32, qp, X, k2, X, od, rows, X, N_, 1, X, q2, X, wsb, None)
    assert f_call(qp=None) == -1 and "null pointer" in err()
    assert f_call(q2=None) == -1 and "null pointer" in err()
    assert f_call(N_=0) == -1 and "N out of range" in err()
    assert f_call(rows=0) == -1 and "obs_rows" in err()
    assert f_call(rows=N + 1) == -1 and "obs_rows" in err()
    assert f_call(od=23) == -1 and "does not pair" in err()
    assert f_call(od=0) == -1 and "does not pair" in err()
    assert f_call(wsb=wf - 256) == -1 and "workspace too small" in err()
    sel = lambda q1=X, cand=X, v=X, out=X, B=8, S=4, w=12, mode=1: lib.dppo_idql_select(q1, X, v, 0, cand, X, B, S, w, mode, 0.7, 0,
                                                                                         out, X, None)
    assert sel(q1=None) == -1 and "null pointer" in err()
    assert sel(cand=None) == -1 and "null pointer" in err()
    assert sel(out=None) == -1 and "null pointer" in err()
    assert sel(v=None) == -1 and "needs v" in err()
    assert sel(mode=2) == -1 and "mode" in err()
    for kw in (dict(B=0), dict(S=0), dict(w=0), dict(B=2 ** 30, S=4)):
        assert sel(**kw) == -1 and "out of range" in err()


def test_device_replay_maps_indices_like_the_reference_deques():
    """``append`` x 11 into a ring of 4 (two wrap-arounds and a partial fill on the way): ``len``, eviction and the logical order
    are those of five ``deque(maxlen=4)`` flattened "s e ... -> (s e) ..." (reference agent :101-105, 233-253).  CPU tensors:
    this checks the index mapping the row builder restates, not the kernels."""
    import einops
    from dppo_amd.util.replay import DeviceReplay
    cap, E, od, ad = 4, 3, 5, 6
    rp = DeviceReplay(cap, E, od, ad, device="cpu")
    dq = [collections.deque(maxlen=cap) for _ in range(5)]
    rs = np.random.RandomState(0)
    for step in range(11):
        items = (rs.randn(E, 1, od).astype(np.float32), rs.randn(E, 1, od).astype(np.float32), rs.randn(E, 2, 3).astype(np.float32),
                 rs.randn(E), rs.rand(E) < 0.5)
        rp.append(T(items[0]), items[1], T(items[2]), items[3], items[4].astype(np.float32))
        for d, x in zip(dq, items):
            d.append(x)
        assert len(rp) == min(step + 1, cap) * E == len(dq[0]) * E
        assert rp.head == max(0, step + 1 - cap) % cap
        ref = [einops.rearrange(np.array(dq[i]), "s e h d -> (s e) (h d)") for i in range(3)] + [
            np.array(dq[3]).reshape(-1).astype(np.float32), np.array(dq[4]).reshape(-1).astype(np.float32)]
        inds = T(rs.permutation(len(rp)).astype(np.int64))
        for got, want in zip(rp.gather(inds), ref):
            assert np.array_equal(got.numpy(), want[inds.numpy()])
        b = rp.batch(None)
        assert (b.cap, b.n_envs, b.head, b.count) == (cap, E, rp.head, min(step + 1, cap)) and b.inds is None
    np.random.seed(3)
    a = rp.draw(5, 7)
    np.random.seed(3)
    want = np.stack([np.random.choice(len(rp), 7) for _ in range(5)])  # one draw for the iteration = the reference's per-minibatch draws
    assert a.dtype == torch.int64 and np.array_equal(a.numpy(), want)


def test_idql_model_refuses_what_the_reference_refuses():
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.diffusion.diffusion_idql import IDQLDiffusion
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    mk = lambda **kw: IDQLDiffusion(actor=DiffusionMLP(3, 4, 11, mlp_dims=[512, 512, 512], residual_style=True), critic_q=make_q("hopper"),
                                    critic_v=CriticObs(11, [256, 256, 256], residual_style=True), horizon_steps=4, obs_dim=11,
                                    action_dim=3, device="cpu", denoising_steps=20, **kw)
    with pytest.raises(AssertionError, match="DDIM"):
        mk(use_ddim=True, ddim_steps=5)
    m = mk()
    assert m.min_sampling_denoising_std == 0.1 and m.actor is m.network
    assert {k.split(".")[0] for k in m.state_dict()} == {"network", "actor", "critic_q", "target_q", "critic_v"}
    with pytest.raises(NotImplementedError, match="state observations"):
        m(cond={"state": torch.zeros(2, 1, 11), "rgb": torch.zeros(2, 1, 3, 8, 8)})
    from dppo_amd import hip
    with pytest.raises(hip.DppoHipError):  # no CPU fallback
        m(cond={"state": torch.zeros(2, 1, 11)})


# ---------------------------------------------------------------------------------------------------------------- GPU
def build_model(net, prec, v_bias=0.0):
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.diffusion.diffusion_idql import IDQLDiffusion
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    od, ta, da = K.shapes(net)
    a = K.actor_spec(net)
    actor = DiffusionMLP(da, ta, od, time_dim=a.time_dim, mlp_dims=list(a.mlp_dims), activation_type=a.activation,
                         residual_style=True, precision=prec)
    if ta == a.horizon_steps:
        actor.load_state_dict(O.init_params(a, K.SEED_ACTOR), strict=True)
    q = make_q(net, prec)
    q.load_state_dict(K.twin_params(net), strict=True)
    v = CriticObs(od, [256, 256, 256], activation_type="Mish", residual_style=True, precision=prec)
    v.load_state_dict(K.v_params(net, v_bias), strict=True)
    m = IDQLDiffusion(actor=actor, critic_q=q, critic_v=v, horizon_steps=ta, obs_dim=od, action_dim=da, device=DEV, **K.SAMPLING_KW)
    m.target_q.load_state_dict(K.twin_params(net, K.TARGET_EPS), strict=True)
    return m


def case_batch(g, net, n):
    keep = T(g[f"{net}_{n}_keep"].astype(np.int64))
    return tuple(t[keep].to(DEV) for t in K.candidates(net, n))


def run_losses(m, batch, inds=None, replay=None):
    """Both losses on one batch -> dict of loss values, statistics, the V epilogue's per-row adv and the two flat gradients (clones)."""
    obs, nxt, act, reward, term = batch
    src = replay if replay is not None else {"state": obs}
    lv = m.loss_critic_v(src, act, inds=inds, expectile=K.EXPECTILE, want_adv=True)
    adv, sv, gv = m.last_adv.clone(), m.last_stats.clone(), m.critic_v.flat_grads().clone()
    lq = m.loss_critic_q(src, {"state": nxt}, act, reward, term, K.GAMMA, inds=inds)
    sq, gq = m.last_stats.clone(), m.critic_q.flat_grads().clone()
    return dict(adv=adv, v_loss=lv.detach().clone(), v_stats=sv, gv=gv, q_loss=lq.detach().clone(), q_stats=sq, gq=gq)


def named_grads(module, flat):
    out, off = [], 0
    for (k, _), p in zip(module.named_parameters(), module.trunk_parameters()):
        out.append((k, flat[off:off + p.numel()].view(p.shape)))
        off += p.numel()
    assert off == flat.numel()
    return out


def check_grads_fp32(g, prefix, named):
    """tests/test_hip_parity.py:177-187's rule."""
    for k, grad in named:
        grad = grad.cpu().numpy()
        key = f"{prefix}_{k}"
        ref_n = float(g[key + "__norm"]) if key not in g else float(np.linalg.norm(g[key]))
        atol = 2e-4 * max(ref_n, 1e-8) / np.sqrt(grad.size) + 1e-7
        if key in g:
            np.testing.assert_allclose(grad, g[key], rtol=2e-3, atol=atol, err_msg=key)
        else:
            np.testing.assert_allclose(grad.reshape(-1)[::61], g[key + "__sub"], rtol=2e-3, atol=atol, err_msg=key)
            assert np.linalg.norm(grad.astype(np.float64)) == pytest.approx(ref_n, rel=2e-4), key


def bf16_errors(g, prefix, named, loss, ref_loss):
    per, n_ref, num, a2, b2 = [], 0.0, 0.0, 0.0, 0.0
    for k, grad in named:
        x = grad.double().cpu().numpy().reshape(-1)
        key = f"{prefix}_{k}"
        if key in g:
            r, xs = g[key].astype(np.float64).reshape(-1), x
            nr = float(r @ r)
        else:
            r, xs, nr = g[key + "__sub"].astype(np.float64), x[::61], float(g[key + "__norm"]) ** 2
        per.append((k, nr, float(np.linalg.norm(xs - r) / (np.linalg.norm(r) + 1e-30))))
        n_ref += nr
        num, a2, b2 = num + float(xs @ r), a2 + float(xs @ xs), b2 + float(r @ r)
    worst = max((e, k) for k, nr, e in per if nr >= 1e-6 * n_ref)
    return dict(loss=abs(loss - ref_loss) / max(1.0, abs(ref_loss)), grad=worst[0], grad_tensor=worst[1], cos=num / np.sqrt(a2 * b2))


def case_errors(g, net, n, m, res):
    """{"v": ..., "q": ...} of one bf16 (or fp32) run, and whether sign(adv) agrees with the reference on every row."""
    name = f"{net}_{n}"
    sign_ok = bool(np.array_equal(res["adv"].cpu().numpy() > 0, g[f"{name}_adv"] > 0))
    return sign_ok, {
        "v": bf16_errors(g, f"{name}_gv", named_grads(m.critic_v, res["gv"]), float(res["v_loss"]), float(g[f"{name}_v_loss"])),
        "q": bf16_errors(g, f"{name}_gq", named_grads(m.critic_q, res["gq"]), float(res["q_loss"]), float(g[f"{name}_q_loss"]))}


@pytest.mark.gpu
@pytest.mark.parametrize("net,n", K.IDQL_CASES, ids=[f"{a}_{b}" for a, b in K.IDQL_CASES])
def test_hip_idql_losses_fp32(golden, net, n):
    """loss_critic_v / loss_critic_q against the reference on every g24 case: losses and statistics, per-row adv, every
    gradient; two calls are bit-equal; a gathered call (indices into a ring with head != 0) equals the contiguous one bit for
    bit."""
    from dppo_amd.util.replay import DeviceReplay
    g, name = golden("g24_idql"), f"{net}_{n}"
    m = build_model(net, "fp32", float(g[f"{name}_v_bias"]))
    batch = case_batch(g, net, n)
    res = run_losses(m, batch)
    got_v = np.array([float(res["v_loss"])] + res["v_stats"].tolist())
    got_q = np.array([float(res["q_loss"])] + res["q_stats"].tolist())
    want_v = np.array([g[f"{name}_v_loss"], g[f"{name}_v_loss"], g[f"{name}_adv_mean"], g[f"{name}_adv_pos"]], dtype=np.float64)
    want_q = np.array([g[f"{name}_q_loss"], g[f"{name}_q_loss"], g[f"{name}_q1_mean"], g[f"{name}_target_mean"]], dtype=np.float64)
    print(f"{name}: v {got_v} ref {want_v}\n  q {got_q} ref {want_q}\n  max |adv - ref| {np.abs(res['adv'].cpu().numpy() - g[name + '_adv']).max():.3e}")
    np.testing.assert_allclose(got_v, want_v, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(got_q, want_q, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(res["adv"].cpu().numpy(), g[f"{name}_adv"], rtol=0, atol=2e-5)
    check_grads_fp32(g, f"{name}_gv", named_grads(m.critic_v, res["gv"]))
    check_grads_fp32(g, f"{name}_gq", named_grads(m.critic_q, res["gq"]))
    again = run_losses(m, batch)
    assert all(torch.equal(res[k], again[k]) for k in res)
    # compute_advantages is forward only: the same numbers (inference forwards), and no gradient buffer is written
    m.critic_v.flat_grads().fill_(7.0)
    fwd = m.compute_advantages({"state": batch[0]}, batch[2])
    assert bool((m.critic_v.flat_grads() == 7.0).all())
    np.testing.assert_allclose(fwd.cpu().numpy(), g[f"{name}_adv"], rtol=0, atol=2e-5)
    # the same rows out of a ring: 5 envs, more steps than rows need, written so that the oldest step sits in slot 3
    obs, nxt, act, reward, term = batch
    E, cap = 5, (n + 4) // 5 + 3
    rp = DeviceReplay(cap, E, obs[0].numel(), act[0].numel(), device=DEV)
    rp.head, rp.steps = 3, cap - 1
    inds = torch.from_numpy(np.random.RandomState(n).permutation(rp.steps * E)[:n].astype(np.int64)).to(DEV)
    rows = rp.slot_of(inds)
    for dst, src in ((rp.obs, obs), (rp.next_obs, nxt), (rp.actions, act), (rp.reward, reward), (rp.terminated, term)):
        dst.view(cap * E, -1)[rows] = src.reshape(n, -1)
    ring = run_losses(m, batch, inds=inds, replay=rp)
    assert all(torch.equal(res[k], ring[k]) for k in res), [k for k in res if not torch.equal(res[k], ring[k])]
    assert torch.equal(m.compute_advantages(rp, None, inds=inds), fwd)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_hip_plain_trunk_inference_forward_never_runs_a_layer_in_place(prec):
    """The inference forward (no activations kept) of a plain trunk with TWO hidden-to-hidden layers, the shipped Q trunk's
    shape: 1000 rows (several row tiles, four column tiles per layer) against the oracle, and bit-equal from call to call.  With
    one buffer for consecutive layers' activations the second layer's GEMM ran in place and its output changed from run to
    run by O(0.1)."""
    from dppo_amd.model.common.critic import CriticObs
    spec = O.NetSpec("critic", cond_dim=23, mlp_dims=[256, 256, 256], activation="Mish", residual=False)
    params = O.init_params(spec, 77, 3.0)
    c = CriticObs(23, [256, 256, 256], activation_type="Mish", residual_style=False, precision=prec).to(DEV)
    c.load_state_dict(params, strict=True)
    assert c.net_desc().plain == 1 and c.net_desc().n_blocks == 2
    state = T(np.random.RandomState(1).uniform(-1, 1, size=(1000, 1, 23)).astype(np.float32))
    want = O.critic_forward(params, spec, state).reshape(-1).numpy()
    outs = [c({"state": state.to(DEV)}).reshape(-1).clone() for _ in range(6)]
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    err = float(np.abs(outs[0].cpu().numpy() - want).max())
    print(f"plain inference forward {prec}: max |v - oracle| {err:.3e}, max |oracle| {np.abs(want).max():.3f}")
    # fp32: the class of tests/test_plain_mlp.py's forward check.  bf16: both operands of each of the four layers are rounded
    # to 2^-9 relative, at worst 2^-8 of a layer's output scale per layer and adding up linearly: 4 * 2^-8 = 1.6e-2
    assert err <= (1e-4 if prec == "fp32" else 1.6e-2) * max(1.0, float(np.abs(want).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("net", ["hopper", "hopper_res"])
def test_hip_idql_half_batches_add_up(golden, net):
    """mean over 77 rows = (38 * mean over the first 38 + 39 * mean over the rest) / 77, for both flat gradients, tensor by tensor at
    rtol 1e-5.  The absolute term is tied to each tensor's own scale: 1e-5 of its rms.  An entry is a sum over the rows of
    products whose size is set by the tensor's rms, not by the entry: where the sum cancels to far below the rms its fp32
    rounding (the two runs add the rows in different orders and round 1 / N differently, ~1e-7 of the products) does not
    shrink with it, so rtol alone would hold such entries to fewer digits than fp32 carries.  An error in a tail row or in a
    1 / N factor of one layer moves that tensor's entries by a fraction of its rms, three or more orders above this term."""
    g = golden("g24_idql")
    m = build_model(net, "fp32", float(g[f"{net}_77_v_bias"]))
    batch = case_batch(g, net, 77)
    whole = run_losses(m, batch)
    a, b = run_losses(m, tuple(t[:38] for t in batch)), run_losses(m, tuple(t[38:] for t in batch))
    for k, mod in (("gv", m.critic_v), ("gq", m.critic_q)):
        both = (38.0 * a[k].double() + 39.0 * b[k].double()) / 77.0
        for (name, x), (_, w) in zip(named_grads(mod, both), named_grads(mod, whole[k])):
            x, w = x.cpu().numpy(), w.double().cpu().numpy()
            rms = float(np.sqrt(np.mean(w * w)))
            assert rms > 0, name
            print(f"{net} {k} {name}: rms {rms:.3e} worst |diff| / (1e-5 |w| + 1e-5 rms) {float((np.abs(x - w) / (1e-5 * np.abs(w) + 1e-5 * rms)).max()):.3f}")
            np.testing.assert_allclose(x, w, rtol=1e-5, atol=1e-5 * rms, err_msg=f"{k} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 134913])
def test_hip_polyak_is_the_torch_expression_bit_for_bit(n):
    """target * (1 - tau) + source * tau evaluated by torch on the CPU (fp32 tensors, Python-float scalars), with the source
    offset by one float from a 16-byte boundary (the scalar path) and aligned (the 16-byte path with an odd tail)."""
    from dppo_amd import hip
    rs = np.random.RandomState(n)
    for tau in (0.005, 0.001, 1.0 / 3.0):
        for off in (1, 0):
            t0, s0 = T(rs.randn(n).astype(np.float32)), T(rs.randn(n + 1).astype(np.float32))
            want = t0 * (1.0 - tau) + s0[off:off + n] * tau
            t, s = t0.to(DEV), s0.to(DEV)
            assert t.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
            src = s[off:off + n]
            hip.check(hip.load().dppo_polyak(t.data_ptr(), src.data_ptr(), tau, n, hip.stream()), "dppo_polyak")
            assert torch.equal(t.cpu(), want), (n, tau, off)


def select_ref(q1, q2, v, cand, u, S, B, mode, h):
    """numpy restatement of the selection: float64 throughout (the crafted inputs keep every decision away from rounding)."""
    q = (np.minimum(q1, q2) if q2 is not None else q1).astype(np.float64).reshape(S, B)
    if mode == 0:
        idx = q.argmax(0)  # first index on ties
    else:
        w = np.where(q - v.astype(np.float64).reshape(-1, B) > 0, h, 1 - h)
        cdf = np.cumsum(w, 0) / w.sum(0)
        idx = (u.astype(np.float64)[None] >= cdf).sum(0).clip(max=S - 1)
    return idx.astype(np.int32), cand.reshape(S, B, -1)[idx, np.arange(B)]


def run_select(q1, q2, v, cand, u, S, B, mode, h, v_per_env=0, seed=0):
    from dppo_amd import hip
    d = lambda x: None if x is None else T(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    tq1, tq2, tv, tc, tu = d(q1), d(q2), d(v), d(cand), d(u)
    AF = cand.shape[-1]
    act = torch.empty(B, AF, device=DEV)
    idx = torch.empty(B, dtype=torch.int32, device=DEV)
    hip.check(hip.load().dppo_idql_select(tq1.data_ptr(), hip.ptr(tq2), hip.ptr(tv), v_per_env, tc.data_ptr(), hip.ptr(tu), B, S, AF,
                                          mode, h, seed, act.data_ptr(), idx.data_ptr(), hip.stream()), "dppo_idql_select")
    return idx.cpu().numpy(), act.cpu().numpy()


@pytest.mark.gpu
def test_hip_idql_select_on_crafted_arrays():
    rs = np.random.RandomState(5)
    for B, S, AF in ((1, 1, 1), (37, 5, 12), (300, 20, 28), (16, 3, 112)):
        cand = rs.randn(S * B, AF).astype(np.float32)
        # argmax: integer-valued q with ties (first index wins), min over the twin decides
        q1, q2 = rs.randint(0, 3, size=S * B).astype(np.float32), rs.randint(0, 3, size=S * B).astype(np.float32)
        for two in (q2, None):
            idx, act = run_select(q1, two, None, cand, None, S, B, 0, 0.7)
            ridx, ract = select_ref(q1, two, None, cand, None, S, B, 0, 0.7)
            assert np.array_equal(idx, ridx) and np.array_equal(act, ract)
        assert S == 1 or (np.sort(np.minimum(q1, q2).reshape(S, B), 0)[-1] == np.sort(np.minimum(q1, q2).reshape(S, B), 0)[-2]).any()
        # inverse CDF: adv = +-1 exactly, u kept >= 1e-4 from every boundary (float64 boundaries)
        v = rs.randn(S * B).astype(np.float32)
        sign = np.where(rs.rand(S * B) < 0.5, 1.0, -1.0).astype(np.float32)
        q1 = v + sign
        q2 = q1 + rs.randint(0, 2, size=S * B).astype(np.float32) * 4.0  # q2 >= q1: the min is q1
        for h in (0.7, 0.2, 0.5):
            w = np.where(sign.reshape(S, B) > 0, h, 1 - h).astype(np.float64)
            cdf = np.cumsum(w, 0) / w.sum(0)
            u = rs.uniform(0, 1, size=B)
            for _ in range(50):
                bad = (np.abs(cdf - u[None]) < 1e-4).any(0) | (u >= 1 - 1e-4)
                if not bad.any():
                    break
                u[bad] = rs.uniform(0, 1, size=int(bad.sum()))
            assert not bad.any()
            idx, act = run_select(q1, q2, v, cand, u, S, B, 1, h)
            ridx, ract = select_ref(q1, q2, v, cand, u, S, B, 1, h)
            assert np.array_equal(idx, ridx) and np.array_equal(act, ract), (B, S, h)
        # v given once per env
        ve = rs.randn(B).astype(np.float32)
        q1 = (np.tile(ve, S) + sign).astype(np.float32)
        idx, _ = run_select(q1, None, ve, cand, u, S, B, 1, 0.7, v_per_env=1)
        assert np.array_equal(idx, select_ref(q1, None, np.tile(ve, S), cand, u, S, B, 1, 0.7)[0])


@pytest.mark.gpu
def test_hip_idql_select_in_kernel_generator_draws_the_weights():
    """B = 8192 envs with the same adv pattern (+, -, -, +) and h = 0.7: weights (0.7, 0.3, 0.3, 0.7) / 2.  Each index is drawn
    within 5 standard errors of its probability, two seeds differ, one seed repeats."""
    B, S, h = 8192, 4, 0.7
    sign = np.array([1, -1, -1, 1], dtype=np.float32)
    q1 = np.repeat(sign, B)
    v = np.zeros(S * B, dtype=np.float32)
    cand = np.repeat(np.arange(S, dtype=np.float32), B).reshape(S * B, 1)
    p = np.where(sign > 0, h, 1 - h) / np.where(sign > 0, h, 1 - h).sum()
    a, act = run_select(q1, None, v, cand, None, S, B, 1, h, seed=1234567891234)
    b, _ = run_select(q1, None, v, cand, None, S, B, 1, h, seed=99)
    a2, _ = run_select(q1, None, v, cand, None, S, B, 1, h, seed=1234567891234)
    assert np.array_equal(a, a2) and not np.array_equal(a, b) and np.array_equal(act.reshape(-1), a.astype(np.float32))
    for idx in (a, b):
        freq = np.bincount(idx, minlength=S) / B
        assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / B)).all(), (freq, p)


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,det", K.SAMPLING, ids=[f"B{b}_S{s}_{'det' if d else 'sto'}" for b, s, d in K.SAMPLING])
def test_hip_idql_forward_returns_the_golden_candidate(golden, B, S, det):
    """fp32 with the recorded noise (and uniforms): the chosen index is the reference's, the action within the chain tolerance;
    in both precisions the returned row is bit-equal to the candidate the model's own sampler, target twin and V give that
    index."""
    g = golden("g24_idql")
    name = f"sample_B{B}_S{S}_{'det' if det else 'sto'}"
    state, noise, u = K.sampling_inputs(B, S, int(g[f"{name}_seed"]))
    for prec in ("fp32", "bf16"):
        m = build_model("hopper", prec, float(g["sample_v_bias"]))
        kw = dict(deterministic=det, num_sample=S, critic_hyperparam=K.CRITIC_HYPERPARAM, noise=noise.to(DEV), u=u.to(DEV))
        act, idx, cand, q1, q2, v = m(cond={"state": state.to(DEV)}, return_all=True, **kw)
        assert act.shape == (B, 4, 3) and cand.shape == (S * B, 4, 3)
        ridx, ract = select_ref(q1.cpu().numpy(), q2.cpu().numpy(), None if v is None else np.tile(v.cpu().numpy(), S),
                                cand.cpu().numpy().reshape(S * B, -1), u.numpy(), S, B, 0 if det else 1, K.CRITIC_HYPERPARAM)
        if prec == "fp32":
            print(f"{name}: idx {idx.cpu().numpy()} golden {g[name + '_idx']} max |a - ref| {np.abs(act.cpu().numpy() - g[name + '_actions']).max():.3e}")
            assert np.array_equal(idx.cpu().numpy(), g[f"{name}_idx"])
            np.testing.assert_allclose(act.cpu().numpy(), g[f"{name}_actions"], rtol=0, atol=1e-4)
            assert np.array_equal(idx.cpu().numpy(), ridx)
        else:
            # bf16: the choice against the restatement on the model's OWN q1 / q2 / v.  The argmax is exact (same fp32 values,
            # first index on ties).  The draw's weights follow the signs of this precision's adv, so the fixture's margin of u
            # from the CDF boundaries does not carry over: an environment whose u lies within 1e-5 of a float64 boundary (the
            # kernel sums S <= 20 weights in fp32, error ~1e-6) is left out, and nearly all must remain.
            clear = np.ones(B, dtype=bool)
            if not det:
                q = np.minimum(q1.cpu().numpy(), q2.cpu().numpy()).astype(np.float64).reshape(S, B)
                w = np.where(q - v.cpu().numpy().astype(np.float64)[None] > 0, K.CRITIC_HYPERPARAM, 1 - K.CRITIC_HYPERPARAM)
                clear = (np.abs(np.cumsum(w, 0) / w.sum(0) - u.numpy().astype(np.float64)[None]) >= 1e-5).all(0)
            assert clear.mean() >= 0.9 and np.array_equal(idx.cpu().numpy()[clear], ridx[clear])
        pick = cand.view(S, B, -1)[idx.long(), torch.arange(B, device=DEV)]
        assert torch.equal(act.reshape(B, -1), pick)
        assert torch.equal(m(cond={"state": state.to(DEV)}, **kw), act)  # and the plain call returns the same rows
        assert (v is None) == det


@pytest.mark.gpu
@pytest.mark.parametrize("net,n", K.IDQL_CASES, ids=[f"{a}_{b}" for a, b in K.IDQL_CASES])
def test_hip_idql_losses_bf16(golden, net, n):
    g = golden("g24_idql")
    m = build_model(net, "bf16", float(g[f"{net}_{n}_v_bias"]))
    res = run_losses(m, case_batch(g, net, n))
    sign_ok, errs = case_errors(g, net, n, m, res)
    print(f"{net}_{n} bf16: sign(adv) agrees {sign_ok}; {errs}")
    assert sign_ok, "sign(adv) differs from the reference on some row: the fixture's margin is wrong (fix the generator)"
    for which, e in errs.items():
        b = bf16_bounds()[which]
        assert e["loss"] <= b["loss"] and e["grad"] <= b["grad"] and e["cos"] >= b["cos"], (which, e, b)


def agent_cfg(tmp_path, **train):
    cfgs = load_config(SHIPPED)
    cfg = copy.deepcopy(cfgs["gym/finetune/hopper-v2/ft_idql_diffusion_mlp.yaml"])
    cfg.update(device=DEV, seed=42, logdir=str(tmp_path), env=Cfg(n_envs=4, name="synthetic", max_episode_steps=5, reset_at_iteration=False))
    cfg.pop("wandb", None)
    cfg.model.update(device=DEV, network_path=None)
    for node in (cfg.model.actor, cfg.model.critic_q, cfg.model.critic_v):
        node["precision"] = "fp32"
    cfg.train.update(dict(n_train_itr=3, n_critic_warmup_itr=1, n_steps=6, batch_size=16, replay_ratio=4, buffer_size=4, val_freq=100,
                          force_train=True, save_model_freq=100, eval_sample_num=3), **train)
    return cfg


@pytest.mark.gpu
def test_hip_idql_agent_runs_the_reference_update_order(tmp_path):
    """hopper cfg shrunk (4 envs, 6 steps, batch 16, replay_ratio 4, ring of 4 steps, 3 iterations, 1 warm-up): the run completes;
    the actor is untouched during the warm-up iteration and moves afterwards; the ring evicts; after every minibatch the target
    is the Polyak recurrence of its previous value and the freshly stepped Q; a checkpoint round-trips."""
    from dppo_amd.agent.finetune.train_idql_diffusion_agent import TrainIDQLDiffusionAgent
    agent = TrainIDQLDiffusionAgent(agent_cfg(tmp_path))
    m = agent.model
    assert agent.replay.cap == 4 and m.critic_q.net_desc().plain == 1
    actor0 = m.actor.flat_params().clone()
    actor_after, polyak_ok, lens = {}, [], []
    inner = agent.update_minibatch

    def spy(inds, **kw):
        before = m.target_q.flat_params().clone()
        out = inner(inds, **kw)
        tau = agent.critic_tau
        want = before.cpu() * (1.0 - tau) + m.critic_q.flat_params().cpu() * tau
        polyak_ok.append(torch.equal(m.target_q.flat_params().cpu(), want))
        actor_after[agent.itr] = m.actor.flat_params().clone()
        lens.append(len(agent.replay))
        return out
    agent.update_minibatch = spy
    res = agent.run()
    assert [r["itr"] for r in res] == [0, 1, 2] and all(np.isfinite(r["loss_actor"]) and np.isfinite(r["loss_critic"]) for r in res)
    assert len(polyak_ok) == 3 * int(6 * 4 / 16 * 4) and all(polyak_ok)
    assert torch.equal(actor_after[0], actor0) and not torch.equal(actor_after[1], actor0)
    assert set(lens) == {16} and agent.replay.steps == 4 and agent.replay.head == (3 * 6) % 4  # 18 appends into 4 slots
    assert not torch.equal(m.target_q.flat_params(), m.critic_q.flat_params())
    path = os.path.join(str(tmp_path), "checkpoint", "state_2.pt")
    data = torch.load(path, weights_only=True)
    assert set(data) == {"itr", "model"} and data["itr"] == 2
    assert {k.split(".")[0] for k in data["model"]} == {"network", "actor", "critic_q", "target_q", "critic_v"}
    assert "critic_q.Q2.moduleList.3.linear_1.bias" in data["model"] and "critic_v.Q1.layers.2.weight" in data["model"]
    other = TrainIDQLDiffusionAgent(agent_cfg(tmp_path, n_train_itr=0))
    other.load(2)
    for a, b in ((other.model.actor, m.actor), (other.model.critic_q, m.critic_q), (other.model.target_q, m.target_q),
                 (other.model.critic_v, m.critic_v)):
        assert torch.equal(a.flat_params(), b.flat_params())
    st = torch.zeros(4, 1, 11, device=DEV)
    nz, u = torch.randn(21, 12, 4, 3, device=DEV), torch.full((4,), 0.5, device=DEV)
    assert torch.equal(other.model(cond={"state": st}, num_sample=3, noise=nz, u=u), m(cond={"state": st}, num_sample=3, noise=nz, u=u))


@pytest.mark.gpu
def test_hip_idql_agent_minibatch_is_the_recorded_sequence(golden, tmp_path):
    """One fp32 minibatch of ``update_minibatch`` on the hopper_77 rows against the sequence the reference recorded: V loss and
    AdamW step, then the Q loss WITH THE UPDATED V (its value and gradient differ from the stand-alone case's), the Q step, and
    the Polyak average of the stepped Q."""
    from dppo_amd.agent.finetune.train_idql_diffusion_agent import TrainIDQLDiffusionAgent
    from dppo_amd.util.optim import FlatAdamW
    from dppo_amd.util.replay import DeviceReplay
    g = golden("g24_idql")
    agent = TrainIDQLDiffusionAgent(agent_cfg(tmp_path, n_train_itr=0, critic_tau=K.SEQ_TAU))
    m = agent.model = build_model("hopper", "fp32", float(g["hopper_77_v_bias"]))
    agent.gamma = K.GAMMA
    agent.critic_v_optimizer = FlatAdamW(m.critic_v.flat_params(), lr=K.SEQ_LR, weight_decay=0)
    agent.critic_q_optimizer = FlatAdamW(m.critic_q.flat_params(), lr=K.SEQ_LR, weight_decay=0)
    agent.actor_optimizer = FlatAdamW(m.actor.flat_params(), lr=1e-4, weight_decay=0)
    obs, nxt, act, reward, term = case_batch(g, "hopper", 77)
    rp = agent.replay = DeviceReplay(77, 1, 11, 12, device=DEV)
    for dst, src in ((rp.obs, obs), (rp.next_obs, nxt), (rp.actions, act), (rp.reward, reward), (rp.terminated, term)):
        dst.copy_(src.reshape(dst.shape))
    rp.steps = 77
    inds = torch.arange(77, device=DEV)
    lv, lq, la = agent.update_minibatch(inds, noise=torch.randn(77, 4, 3, device=DEV), t=torch.randint(0, 20, (77,), device=DEV))
    print(f"seq: v_loss {float(lv)!r} ref {float(g['seq_v_loss'])!r}; q_loss {float(lq)!r} ref {float(g['seq_q_loss'])!r}")
    assert float(g["seq_q_loss"]) != float(g["hopper_77_q_loss"])  # the updated V moved the target
    np.testing.assert_allclose([float(lv), float(lq)], [float(g["seq_v_loss"]), float(g["seq_q_loss"])], rtol=2e-4, atol=2e-5)
    check_grads_fp32(g, "seq_gq", named_grads(m.critic_q, m.critic_q.flat_grads()))
    # AdamW's first step is lr * g / (|g| + eps): an entry whose gradient is off by dg moves off by lr * dg / (|g| + eps), with dg
    # from the gradient rule above (rtol 2e-3, the tensor's atol) -- and by at most 2 lr whatever the gradient; the target moves
    # by tau times Q's step.  Plus one ulp-class term for the weight itself.
    for key, net, gkey, step in (("seq_v", m.critic_v, "hopper_77_gv", K.SEQ_LR), ("seq_q", m.critic_q, "seq_gq", K.SEQ_LR),
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
    assert np.isfinite(float(la)) and agent.itr == 0  # warm-up: the actor's loss is computed, its step is not taken
