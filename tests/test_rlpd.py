"""LayerNorm in a plain Q trunk (reference model/common/mlp.py:46-74 with ``use_layernorm``: ``norm_1 = nn.LayerNorm(o_dim)``, eps
1e-5, behind every Linear but the last and in front of the activation), the critic of every RLPD / Cal-QL / IBRL cfg the reference
ships.  ``CriticObsAct(use_layernorm=True, double_q=False)`` carries the reference's state dict, the C ABI lays the flat image out in
that order, the entries that are not taught LayerNorm refuse such a descriptor (CPU), and on the GPU every member's Q through
``dppo_idql_q_forward`` is held to the restatement of tests/golden/make_golden_rlpd_cases.py in FLOAT64 fed the same fp32 values.
``RLPD_Gaussian`` (reference model/rl/gaussian_rlpd.py) keeps the ensemble in one flat [E][P] image under the reference's names; its
``loss_critic`` (``dppo_rlpd_q_loss_fwd_bwd``) is held the same way: statistics by stats_close, every gradient tensor of every member
(``norm_1.weight`` / ``norm_1.bias`` among them) by grad_violations' rule, ReLU gates within RELU_TIE handed over as
tests/test_sac.py::check_on_own_sel does.

fp32.  stats_close's rule (tests/test_dql.py) on every row: |q - q64| <= 1e-5 max(1, |q64|).  The ``tiny_flat`` member (variance 0,
rstd = 1 / sqrt(eps)) is held by the same rule: with xhat = 0 exactly, z = beta and nothing is amplified.

bf16.  No tolerance is fixed: the yardstick is the restatement with every Linear's operands rounded to bf16 (bf16_linears) and
LayerNorm left in fp32; with e_y its error against the fp32 restatement (relative l2 over all members' rows), the call may be off
from the fp32 restatement by at most 2 e_y.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dppo_amd import hip
from tests.golden import make_golden_rlpd_cases as K
from tests.test_dql import grad_violations, rel_errors, stats_close
from tests.test_qsm import ring_of

DEV = "cuda:0"
IDS = [f"{c}_{n}" for c, n in K.CASES]
D64 = torch.float64


def make_q(case, prec="fp32", **kw):
    from dppo_amd.model.common.critic import CriticObsAct
    od, ta, da, dims, act, _ = K.RLPD_NETS[case]
    return CriticObsAct(**dict(dict(cond_dim=od, mlp_dims=dims, action_dim=da, action_steps=ta, activation_type=act,
                                    use_layernorm=True, double_q=False, precision=prec), **kw))


def ln_desc(case):
    return make_q(case).net_desc()


@functools.lru_cache(maxsize=None)
def restated(case, n, dtype=D64, bf16=False):
    """Every member's Q, [E][n]: computed once, shared, never modified."""
    b = K.inputs(case, n)
    out = []
    with torch.no_grad():
        for e in range(K.n_critics(case)):
            p = K.cast(K.member_params(case, e), dtype)
            if bf16:
                with K.bf16_linears():
                    out.append(K.q_forward(p, case, b["obs"].to(dtype), b["actions"].to(dtype)))
            else:
                out.append(K.q_forward(p, case, b["obs"].to(dtype), b["actions"].to(dtype)))
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case", list(K.RLPD_NETS))
def test_layernorm_trunk_carries_the_references_state_dict(case):
    """Names and order are the reference's (linear_1.weight, linear_1.bias, norm_1.weight, norm_1.bias per hidden layer, the last
    layer the Linear alone); the flat image is those tensors back to back and as long as the C ABI says."""
    q, p = make_q(case), K.member_params(case, 0)
    dims = K.RLPD_NETS[case][3]
    want = [f"Q1.moduleList.{i}.{m}.{w}" for i in range(len(dims) + 1) for m in (("linear_1", "norm_1") if i < len(dims) else ("linear_1",))
            for w in ("weight", "bias")]
    assert list(q.state_dict()) == want == list(p)
    assert q.Q1.moduleList[0].norm_1.eps == 1e-5
    q.load_state_dict(p, strict=True)
    flat, d = q.flat_params(), q.net_desc()
    assert d.plain == 1 and d.use_layernorm == 1 and d.kind == 1 and d.n_blocks == len(dims) - 1
    assert torch.equal(flat, torch.cat([v.reshape(-1) for v in p.values()]))
    assert flat.numel() == hip.load().dppo_net_param_count(C.byref(d))
    off = 0
    for t in q.parameters():  # views of the flat image, in state-dict order
        assert t.data_ptr() == flat.data_ptr() + 4 * off
        off += t.numel()
    for prec in (hip.PREC_F32, hip.PREC_BF16):  # LayerNorm adds nothing to the kernel image: gamma / beta are read from the fp32 one
        plain = hip.NetDesc.from_buffer_copy(d)
        plain.use_layernorm = 0
        assert hip.load().dppo_packed_bytes(C.byref(d), prec, 0) == hip.load().dppo_packed_bytes(C.byref(plain), prec, 0) > 0


def test_entries_not_taught_layernorm_refuse_it():
    lib, d = hip.load(), ln_desc("tiny")
    err = lambda: lib.dppo_last_error()
    # one member's Q is read through dppo_idql_q_forward with double_q = 0; a twin of LayerNorm trunks is not built
    assert lib.dppo_idql_q_forward_workspace_bytes(C.byref(d), hip.PREC_F32, 77, 0) > 0
    assert lib.dppo_idql_q_forward_workspace_bytes(C.byref(d), hip.PREC_F32, 77, 1) == -1 and b"LayerNorm" in err()
    assert b"dppo_idql_q_forward" in err()
    # the training entries of IDQL / QSM / SAC and the state-value forward
    v = hip.NetDesc.from_buffer_copy(d)
    v.use_layernorm, v.in_dim, v.cond_dim = 0, 11, 11
    for dq in (0, 1):
        assert lib.dppo_idql_q_loss_workspace_bytes(C.byref(d), C.byref(v), hip.PREC_F32, 77, dq) == -1 and b"LayerNorm" in err()
        assert lib.dppo_idql_v_loss_workspace_bytes(C.byref(d), C.byref(v), hip.PREC_F32, 77, dq) == -1 and b"LayerNorm" in err()
    assert lib.dppo_mlp_forward_workspace_bytes(C.byref(d), hip.PREC_F32, 77) == -1 and b"LayerNorm" in err()
    # what a plain trunk refused before, it refuses still: and a denoiser's message still says ``plain``
    bad = hip.NetDesc.from_buffer_copy(d)
    bad.hidden = 96
    assert lib.dppo_net_param_count(C.byref(bad)) == -1 and b"multiple of 64" in err()
    bad = hip.NetDesc.from_buffer_copy(d)
    bad.use_layernorm = 2
    assert lib.dppo_net_param_count(C.byref(bad)) == -1 and b"use_layernorm" in err()
    a = hip.NetDesc(kind=0, in_dim=12 + 16 + 11, hidden=64, n_blocks=1, out_dim=12, act=hip.ACT_RELU, time_dim=16, act_flat=12,
                    cond_dim=11, cond_hidden=0, cond_out=0, use_layernorm=1, plain=1)
    assert lib.dppo_net_param_count(C.byref(a)) == -1 and b"plain" in err()
    a.use_layernorm = 0
    assert lib.dppo_net_param_count(C.byref(a)) > 0


def test_twin_entries_refuse_a_layernorm_trunk():
    """QSM / DQL / SAC read the critic as a twin [Q1 | Q2]: their workspace queries (the same host checks as the calls) refuse."""
    lib, d = hip.load(), ln_desc("tiny")
    a = hip.NetDesc(kind=1, in_dim=11, hidden=64, n_blocks=1, out_dim=6, act=hip.ACT_RELU, time_dim=0, act_flat=0, cond_dim=11,
                    cond_hidden=0, cond_out=0, use_layernorm=0, plain=1)
    q, f32 = C.byref(d), hip.PREC_F32
    for name, call in (("qsm_actor_target", lambda: lib.dppo_qsm_actor_target_workspace_bytes(q, f32, 11, 77)),
                       ("qsm_q_loss", lambda: lib.dppo_qsm_q_loss_workspace_bytes(q, f32, 11, 77)),
                       ("sac_q_loss", lambda: lib.dppo_sac_q_loss_workspace_bytes(q, f32, 11, 77)),
                       ("sac_actor", lambda: lib.dppo_sac_actor_workspace_bytes(C.byref(a), q, f32, 11, 77))):
        assert call() == -1, name
        assert b"LayerNorm" in lib.dppo_last_error(), (name, lib.dppo_last_error())


def test_owners_that_cannot_run_a_layernorm_trunk_refuse_it():
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.common.mlp import MLP
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.common.mlp_gmm import GMM_MLP
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    for build in (lambda: CriticObs(11, [64, 64], use_layernorm=True, residual_style=False),
                  lambda: make_q("tiny", double_q=True),
                  lambda: GMM_MLP(3, 1, 11, mlp_dims=[64, 64], fixed_std=0.1, use_layernorm=True, residual_style=False),
                  lambda: Gaussian_MLP(3, 1, 11, mlp_dims=[64, 64], fixed_std=None, tanh_output=False, use_layernorm=True),
                  lambda: DiffusionMLP(3, 4, 11, mlp_dims=[64, 64], residual_style=False, use_layernorm=True),
                  lambda: MLP([14, 64, 64, 1], activation_type="ReLU", use_layernorm=True, use_layernorm_final=True),
                  lambda: MLP([14, 64, 64, 1], activation_type="ReLU", use_layernorm=True, dropout=0.1),
                  lambda: MLP([14, 64, 64, 1], activation_type="ReLU", use_layernorm=True, append_dim=2)):
        with pytest.raises(NotImplementedError):
            build()
    assert sorted(dict(MLP([14, 64, 64, 1], activation_type="ReLU").named_parameters())) == sorted(
        f"moduleList.{i}.linear_1.{w}" for i in range(3) for w in ("weight", "bias"))


@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_inputs_keep_their_guard_bands(case, n):
    """On the float64 restatement fed the fp32 values: outside ``tiny_flat`` every row's pre-LayerNorm variance exceeds VAR_FLOOR, so
    no row sits where eps decides; in it the flattened member's layer-0 variance is exactly 0 (in fp32 too) and its Q is finite."""
    b = K.inputs(case, n)
    for e in range(K.n_critics(case)):
        var = K.pre_ln_variances(K.cast(K.member_params(case, e), D64), case, b["obs"].double(), b["actions"].double())
        flat = case == "tiny_flat" and e == K.FLAT_MEMBER
        for i, v in enumerate(var):
            if flat and i == 0:
                assert (v == 0).all()
                v32 = K.pre_ln_variances(K.member_params(case, e), case, b["obs"], b["actions"])[0]
                assert (v32 == 0).all()
            else:
                assert v.min().item() > K.VAR_FLOOR, (e, i, v.min().item())
    assert torch.isfinite(restated(case, n)).all()


def test_no_cpu_fallback():
    q = make_q("tiny")
    with pytest.raises(hip.DppoHipError):
        q({"state": torch.zeros(2, 1, 11)}, torch.zeros(2, 1, 3))


# ------------------------------------------------------------------------------------------------------------------ GPU
def run_members(case, n, prec):
    b, out = K.inputs(case, n), []
    for e in range(K.n_critics(case)):
        q = make_q(case, prec)
        q.load_state_dict(K.member_params(case, e), strict=True)
        q = q.to(DEV)
        out.append(q({"state": b["obs"].to(DEV)}, b["actions"].to(DEV)).cpu())
    return torch.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_layernorm_q_fp32(case, n):
    got, ref = run_members(case, n, "fp32"), restated(case, n)
    assert got.shape == ref.shape
    for e in range(len(ref)):
        stats_close(got[e].numpy(), ref[e].numpy(), f"{case}_{n} member {e}")
    again = run_members(case, n, "fp32")
    assert torch.equal(got, again)  # the same inputs give the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_layernorm_q_bf16_within_twice_the_rounding_yardstick(case, n):
    fp32, yard = restated(case, n, torch.float32).double(), restated(case, n, torch.float32, True).double()
    got = run_members(case, n, "bf16").double()
    err = lambda x: float((x - fp32).norm() / fp32.norm())
    e_y, e_c = err(yard), err(got)
    print(f"{case}_{n} bf16 Q: yardstick {e_y:.3e} call {e_c:.3e}")
    assert e_c <= 2 * e_y, (e_c, e_y)


@pytest.mark.gpu
def test_hip_layernorm_q_scores_repeated_observations():
    """obs_repeat (best-of-N scoring): row n is scored against observation n % B, through LayerNorm too."""
    case, n = "chunk", 77
    b, q = K.inputs(case, n), make_q(case)
    q.load_state_dict(K.member_params(case, 2), strict=True)
    q = q.to(DEV)
    act = torch.cat([b["actions"], b["actions"].flip(0)]).to(DEV)
    got = q({"state": b["obs"].to(DEV)}, act, obs_repeat=2).cpu()
    p = K.cast(K.member_params(case, 2), D64)
    with torch.no_grad():
        ref = K.q_forward(p, case, torch.cat([b["obs"], b["obs"]]).double(), act.cpu().double())
    stats_close(got.numpy(), ref.numpy(), "obs_repeat")


# ================================================================================================ the ensemble: RLPD_Gaussian
def make_model(case, prec, device, backup=True):
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_rlpd import RLPD_Gaussian
    od, ta, da, dims, act, E = K.RLPD_NETS[case]
    actor = Gaussian_MLP(da, ta, od, mlp_dims=dims[:2], activation_type=act, tanh_output=False, fixed_std=None, std_min=0.0067,
                         std_max=7.3891, precision=prec)
    m = RLPD_Gaussian(actor=actor, critic=make_q(case, prec), n_critics=E, backup_entropy=backup, horizon_steps=ta, device=device,
                      randn_clip_value=3.0, tanh_output=True)
    for e in range(E):
        m.critic_networks[e].load_state_dict(K.member_params(case, e), strict=True)
        m.target_networks[e].load_state_dict(K.member_params(case, e, K.TARGET_EPS), strict=True)
    return m


def restate_critic(case, n, dtype=D64, bf16=False, gates=None):
    E = K.n_critics(case)
    members = [K.leaf(K.member_params(case, e), dtype) for e in range(E)]
    targets = [K.member_params(case, e, K.TARGET_EPS) for e in range(E)]
    args = (members, targets, case, K.inputs(case, n), K.pair_of(case, n), K.backup_entropy(case, n))
    with gates if gates is not None else K.relu_gates() as rg:
        if bf16:
            with K.bf16_linears():
                res = K.loss_critic(*args, dtype=dtype)
        else:
            res = K.loss_critic(*args, dtype=dtype)
    res["named"] = [(f"{e}.{k}", g) for e, (p, gs) in enumerate(zip(members, res["grads"])) for k, g in zip(p, gs)]
    res["near_zero"] = rg.near_zero()
    return res


@functools.lru_cache(maxsize=None)
def restated_critic(case, n):
    """The float64 restatement of one case: computed once, shared, never modified."""
    return restate_critic(case, n)


def named_grads(m):
    """(member.name, slice of the [E][P] gradient) in the flat image's order."""
    g, out, off = m.critic_flat_grads(), [], 0
    for e, q in enumerate(m.critic_networks):
        names = {id(p): k for k, p in q.named_parameters()}
        for p in q.trunk_parameters():
            out.append((f"{e}.{names[id(p)]}", g[off:off + p.numel()].view(p.shape).clone()))
            off += p.numel()
    assert off == g.numel()
    return out


def check_with_gates(case, n, got, what):
    """Every gradient of a run against the float64 restatement by grad_violations' rule on EVERY entry.  Where that misses and the
    networks are ReLU ones, the yardstick's gates below RELU_TIE are tried on their other side, nearest to zero first, each kept if
    it lowers the count of entries outside the rule (tests/test_dql.py::check_on_own_chain)."""
    ref = restated_critic(case, n)
    bad = grad_violations(ref["named"], got)
    if not bad or K.RLPD_NETS[case][4] != "ReLU":
        assert not bad, (what, bad)
        return
    count = lambda b: sum(x[1] + int(x[3]) for x in b)
    print(f"{what}: {count(bad)} entries outside the rule {bad}; {len(ref['near_zero'])} ReLU gates below {K.RELU_TIE:g}")
    force = {}
    for z, where, gate in ref["near_zero"]:
        trial = dict(force)
        trial[where] = not gate
        now = grad_violations(restate_critic(case, n, gates=K.relu_gates(trial))["named"], got)
        if count(now) < count(bad):
            force, bad = trial, now
        if not bad:
            return
    assert not bad, (what, bad, force)


def run_critic(m, case, n, replay=None, inds=None):
    b = {k: v.to(DEV) for k, v in K.inputs(case, n).items()}
    kw = dict(next_actions=b["next_actions"], next_logp=b["next_logp"], pair=K.pair_of(case, n))
    if replay is not None:
        loss = m.loss_critic(replay, None, None, None, None, K.GAMMA, K.ALPHA, inds=inds, **kw)
    else:
        loss = m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], K.GAMMA,
                             K.ALPHA, **kw)
    return dict(loss=loss.detach(), stats=m.last_stats.cpu().numpy().copy(), grads=m.critic_flat_grads().clone())


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_every_shipped_rlpd_model_builds():
    """All nine rlpd_mlp*.yaml of the reference (tests/golden/shipped_rlpd_cfgs.json, settings only): the model target resolves to
    RLPD_Gaussian and builds (eight of them: the lift cfg omits the actor's action_dim, as shipped), its critic is a plain LayerNorm trunk with double_q off, the state-dict keys are the reference's
    (network.*, critic_networks.{e}.*, target_networks.{e}.*; the reference adds base_model.*, ignored on load), the C ABI counts one
    member's parameters, the flat image is [E][P] and the loss's workspace query accepts the shape.  The agent target
    (TrainRLPDAgent) is recorded in the fixture and not built."""
    import os
    from dppo_amd.cfg.loader import get_class, instantiate, load_config
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.rl.gaussian_rlpd import RLPD_Gaussian
    cfgs = load_config(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shipped_rlpd_cfgs.json"))
    assert len(cfgs) == 9 and all(os.path.basename(k).startswith("rlpd_mlp") for k in cfgs)
    lib, seen = hip.load(), set()
    for name, cfg in cfgs.items():
        assert cfg._target_.endswith("train_rlpd_agent.TrainRLPDAgent"), name
        assert get_class(cfg.model._target_) is RLPD_Gaussian and get_class(cfg.model.critic._target_) is CriticObsAct, name
        assert cfg.model.critic.use_layernorm is True and cfg.model.critic.double_q is False and cfg.model.tanh_output is True, name
        if "action_dim" not in cfg.model.actor:  # robomimic/finetune/lift: the shipped cfg leaves it out, and Gaussian_MLP
            assert "lift" in name                # requires it in the reference too: it cannot be built there either
            with pytest.raises(TypeError, match="action_dim"):
                instantiate(cfg.model)
            continue
        m = instantiate(cfg.model)
        E, dims = int(cfg.model.n_critics), list(cfg.model.critic.mlp_dims)
        seen.add((E, len(dims)))
        member = [f"Q1.moduleList.{i}.{mod}.{w}" for i in range(len(dims) + 1)
                  for mod in (("linear_1", "norm_1") if i < len(dims) else ("linear_1",)) for w in ("weight", "bias")]
        keys = [k for k in m.state_dict() if not k.startswith("network.")]
        assert keys == [f"{box}.{e}.{k}" for box in ("critic_networks", "target_networks") for e in range(E) for k in member], name
        dq = m.critic_networks[0].net_desc()
        od, af = cfg.obs_dim * cfg.cond_steps, cfg.action_dim * cfg.horizon_steps
        assert (dq.kind, dq.plain, dq.use_layernorm, dq.in_dim, dq.hidden, dq.n_blocks) == (1, 1, 1, od + af, dims[0], len(dims) - 1), name
        P = lib.dppo_net_param_count(C.byref(dq))
        assert P == sum(p.numel() for p in m.critic_networks[0].parameters()) and m.critic_flat_params().numel() == E * P, name
        assert m.backup_entropy == bool(cfg.model.get("backup_entropy", False))
        for prec in (hip.PREC_F32, hip.PREC_BF16):
            assert lib.dppo_rlpd_q_loss_workspace_bytes(C.byref(dq), prec, od, int(cfg.train.batch_size), E) > 0, lib.dppo_last_error()
    assert (10, 2) in seen and (5, 3) in seen


def test_rlpd_state_dict_is_the_references():
    """network.*, critic_networks.{e}.*, target_networks.{e}.* under the reference's names; ``base_model.*`` keys of a reference
    checkpoint are accepted and ignored; the ensemble is ONE flat [E][P] image with the parameters as views in state-dict order."""
    case = "tiny"
    m, E = make_model(case, "fp32", "cpu"), K.n_critics(case)
    member = list(K.member_params(case, 0))
    keys = list(m.state_dict())
    want = [f"{box}.{e}.{k}" for box in ("critic_networks", "target_networks") for e in range(E) for k in member]
    assert [k for k in keys if not k.startswith("network.")] == want and keys[0].startswith("network.")
    sd = dict(m.state_dict())
    sd.update({f"base_model.{k}": torch.empty(v.shape, device="meta") for k, v in K.member_params(case, 0).items()})
    m.load_state_dict(sd, strict=True)
    flat = m.critic_flat_params()
    P = hip.load().dppo_net_param_count(C.byref(m.critic_networks[0].net_desc()))
    assert flat.numel() == E * P
    off = 0
    for e in range(E):
        for k, t in m.critic_networks[e].named_parameters():
            assert t.data_ptr() == flat.data_ptr() + 4 * off and torch.equal(t, K.member_params(case, e)[k]), (e, k)
            off += t.numel()
    assert torch.equal(m.target_flat_params()[P:2 * P], torch.cat([v.reshape(-1) for v in K.member_params(case, 1, K.TARGET_EPS).values()]))
    with torch.no_grad():  # an in-place step on the flat image is a step on every member
        flat.add_(1.0)
    assert torch.equal(m.critic_networks[2].Q1.moduleList[0].norm_1.weight, K.member_params(case, 2)["Q1.moduleList.0.norm_1.weight"] + 1.0)
    pair = m.get_random_indices()
    assert len(pair) == 2 and pair[0] != pair[1] and pair.device.type == "cpu" and int(pair.max()) < E


def test_rlpd_model_refuses_what_it_cannot_run():
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_rlpd import RLPD_Gaussian
    from tests.test_sac import make_q as twin_q
    actor = Gaussian_MLP(3, 1, 11, mlp_dims=[64, 64], activation_type="ReLU", tanh_output=False, fixed_std=None)
    kw = dict(horizon_steps=1, device="cpu", tanh_output=True)
    with pytest.raises(ValueError, match="double_q"):
        RLPD_Gaussian(actor=actor, critic=twin_q("tiny"), n_critics=3, **kw)
    with pytest.raises(ValueError, match="two critics"):
        RLPD_Gaussian(actor=actor, critic=make_q("tiny"), n_critics=1, **kw)
    fixed = Gaussian_MLP(3, 1, 11, mlp_dims=[256, 256, 256], fixed_std=0.1, residual_style=True)
    with pytest.raises(NotImplementedError, match="state-dependent"):
        RLPD_Gaussian(actor=fixed, critic=make_q("tiny"), n_critics=3, **kw)
    m = RLPD_Gaussian(actor=actor, critic=make_q("tiny"), n_critics=3, **kw)
    with pytest.raises(NotImplementedError, match="not built"):
        m.loss_actor({"state": torch.zeros(2, 1, 11)}, 0.7)


def test_rlpd_entry_rejects_bad_arguments_on_the_host():
    """Every refusal leaves its reason in dppo_last_error(); nothing here touches a device (the pointers are never read)."""
    lib, d = hip.load(), ln_desc("tiny")
    err = lambda: lib.dppo_last_error()
    ws_bytes = lambda desc, E=3, N=77, od=11, prec=hip.PREC_F32: lib.dppo_rlpd_q_loss_workspace_bytes(C.byref(desc), prec, od, N, E)
    assert ws_bytes(d) > 0
    for E in (1, 0, 17):
        assert ws_bytes(d, E=E) == -1 and b"members" in err()
    assert ws_bytes(d, prec=7) == -1 and b"prec" in err()
    assert ws_bytes(d, N=0) == -1 and b"N out of range" in err()
    assert ws_bytes(d, od=14) == -1 and b"obs_dim" in err()
    plain = hip.NetDesc.from_buffer_copy(d)
    plain.use_layernorm = 0
    assert ws_bytes(plain) == -1 and b"LayerNorm" in err()
    res = hip.NetDesc(kind=1, in_dim=14, hidden=256, n_blocks=1, out_dim=1, act=hip.ACT_RELU, time_dim=0, act_flat=0, cond_dim=14,
                      cond_hidden=0, cond_out=0, use_layernorm=1, plain=0)
    assert ws_bytes(res) == -1 and b"plain" in err()
    wide = hip.NetDesc.from_buffer_copy(d)
    wide.hidden = 2048
    assert ws_bytes(wide) == -1 and b"hidden" in err()
    one = C.c_double(0)  # stands in for every pointer: refusals come before anything is read
    ptr = C.addressof(one)
    imgs = (C.c_void_p * 3)(ptr, ptr, ptr)
    batch = hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 0, 77)

    def call(E=3, pair=(0, 1), q_params=ptr, images=imgs, timgs=imgs, logp=ptr, alpha=ptr, N=77, gamma=0.99, prec=hip.PREC_F32, desc=d):
        return lib.dppo_rlpd_q_loss_fwd_bwd(C.byref(desc), prec, E, q_params, images, ptr, timgs, pair[0], pair[1], C.byref(batch), 11,
                                            ptr, logp, alpha, N, gamma, ptr, ptr, ptr, 1 << 40, None)
    for pair in ((0, 0), (3, 0), (0, -1), (1, 7)):
        assert call(pair=pair) == -1 and b"pair" in err(), pair
    assert call(E=1) == -1 and b"members" in err()
    assert call(q_params=None) == -1 and b"null pointer" in err()
    assert call(logp=None) == -1 and b"go together" in err()
    assert call(alpha=None) == -1 and b"go together" in err()
    assert call(images=(C.c_void_p * 3)(ptr, None, ptr)) == -1 and b"member 1" in err()
    assert call(timgs=(C.c_void_p * 3)(None, ptr, ptr)) == -1 and b"target member" in err()
    assert call(prec=5) == -1 and b"prec" in err()
    assert call(N=0) == -1 and b"N out of range" in err()
    assert call(gamma=1.5) == -1 and b"gamma" in err()
    assert call(desc=plain) == -1 and b"LayerNorm" in err()
    assert lib.dppo_version() == 1


@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_target_pairs_keep_their_guard_band(case, n):
    """On the float64 restatement: every |tq_i - tq_j| is at least ten times the fp32 ceiling Q_CEIL, so both implementations take
    the same member's value in every row."""
    r = restated_critic(case, n)
    gap = (r["tq"][0] - r["tq"][1]).abs().min().item()
    assert gap >= 10 * K.Q_CEIL, gap
    assert len({K.pair_of(c, k) for c, k in K.CASES}) >= 4 and not K.backup_entropy(*K.NO_BACKUP)


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_rlpd_loss_critic_fp32(case, n):
    """Statistics and every member's every gradient against float64; two calls are bit-equal; a gathered call (indices into a ring
    with head != 0) equals the contiguous one bit for bit; a member outside the pair trains."""
    m, ref = make_model(case, "fp32", DEV, K.backup_entropy(case, n)), restated_critic(case, n)
    res = run_critic(m, case, n)
    stats_close(res["stats"], ref["stats"], f"{case}_{n} critic")
    assert float(res["loss"]) == np.float32(res["stats"][0])
    got = named_grads(m)
    check_with_gates(case, n, got, f"{case}_{n}")
    E, P = K.n_critics(case), res["grads"].numel() // K.n_critics(case)
    for e in set(range(E)) - set(K.pair_of(case, n)):
        assert res["grads"][e * P:(e + 1) * P].abs().sum().item() > 0, e
    again = run_critic(m, case, n)
    assert torch.equal(res["grads"], again["grads"]) and np.array_equal(res["stats"], again["stats"])
    rp, inds = ring_of({k: v.to(DEV) for k, v in K.inputs(case, n).items()}, n)
    ring = run_critic(m, case, n, replay=rp, inds=inds)
    assert torch.equal(res["grads"], ring["grads"]) and np.array_equal(res["stats"], ring["stats"])
    loss = m.loss_critic(rp, None, None, None, None, K.GAMMA, K.ALPHA, inds=inds, next_actions=K.inputs(case, n)["next_actions"].to(DEV),
                         next_logp=K.inputs(case, n)["next_logp"].to(DEV), pair=K.pair_of(case, n))
    loss.backward()  # .backward() hands every parameter of every member its slice
    w = m.critic_networks[E - 1].Q1.moduleList[0].norm_1.weight
    assert torch.equal(w.grad, dict(got)[f"{E - 1}.Q1.moduleList.0.norm_1.weight"])


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_rlpd_loss_critic_bf16_within_twice_the_rounding_yardstick(case, n):
    """No tolerance is fixed: with e_y the error of the bf16-Linear restatement (LayerNorm in fp32) against the fp32 restatement,
    the call may be off by at most 2 e_y on the loss, per tensor and on 1 - cosine."""
    m = make_model(case, "bf16", DEV, K.backup_entropy(case, n))
    res = run_critic(m, case, n)
    fp32, yard = restate_critic(case, n, torch.float32), restate_critic(case, n, torch.float32, bf16=True)
    z = torch.zeros(1)
    for r in (fp32, yard):
        r["d_a"] = z
    call = dict(loss=res["stats"][0], d_a=z, named=named_grads(m))
    e_y, e_c = rel_errors(fp32, yard), rel_errors(fp32, call)
    worst = max(e_c["per"], key=lambda k: e_c["per"][k] / (e_y["per"][k] + 1e-30))
    print(f"{case}_{n} bf16: yardstick loss {e_y['loss']:.3e} 1-cos {e_y['one_minus_cos']:.3e}; call loss {e_c['loss']:.3e} 1-cos "
          f"{e_c['one_minus_cos']:.3e}; worst tensor {worst}: {e_c['per'][worst]:.3e} against {e_y['per'][worst]:.3e}")
    assert e_c["loss"] <= 2 * e_y["loss"] and e_c["one_minus_cos"] <= 2 * e_y["one_minus_cos"]
    for k in e_c["per"]:
        assert e_c["per"][k] <= 2 * e_y["per"][k], (k, e_c["per"][k], e_y["per"][k])


@pytest.mark.gpu
def test_hip_rlpd_polyak_moves_the_whole_target_ensemble():
    case = "tiny"
    m = make_model(case, "fp32", DEV)
    t0, s0 = m.target_flat_params().clone(), m.critic_flat_params().clone()
    m.update_target_critic(0.005)
    want = t0 * np.float32(1 - 0.005) + s0 * np.float32(0.005)
    assert torch.equal(m.target_flat_params(), want)
    assert torch.equal(m.target_networks[2].Q1.moduleList[1].norm_1.bias.reshape(-1), want.view(3, -1)[2][-(64 + 1 + 64):-(64 + 1)])
