"""Cal-QL's conservative critic loss (reference model/rl/gaussian_calql.py:56-171) on the twin of LayerNorm Q trunks every shipped
calql_mlp_*.yaml configures: ``CriticObsAct(use_layernorm=True, double_q=True, twin_layernorm=True)`` and ``CalQL_Gaussian.loss_critic``
(``dppo_calql_q_loss_fwd_bwd``, csrc/calql.hip).

CPU.  The plain-torch restatement of tests/golden/make_golden_calql_cases.py -- written with the two scalars L, L' in place of the
reference's (N, N) broadcast -- reproduces in float32 what the reference itself computed (g29_calql.npz): that licenses it as the
yardstick, also for ``per_row_logpi=True``, which the reference cannot run.  The constructed returns and clips keep their guard bands.
Every shipped Cal-QL model builds through ``instantiate`` with its text unchanged; the host checks refuse with a message.

GPU, fp32.  Both modes, every case: ``last_stats`` and ``last_y`` by stats_close (tests/test_dql.py: 1e-5 max(1, |ref|)) against the
restatement in FLOAT64 fed the same fp32 values (the policy's samples are the fp32 restatement's, handed over as ``samples``), every
gradient tensor of both trunks by grad_violations' rule, ReLU gates within RELU_TIE handed over as tests/test_rlpd.py does.
GPU, bf16.  No tolerance is fixed: with e_y the error of the bf16-Linear restatement against the fp32 one, the call may be off by at
most 2 e_y on every statistic, per gradient tensor (relative l2) and on 1 - cosine.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from dppo_amd import hip
from tests.golden import make_golden_calql_cases as K
from tests.test_dql import grad_violations, rel_errors, stats_close
from tests.test_idql import check_grads_fp32

DEV = "cuda:0"
IDS = [f"{c}_{n}" for c, n in K.CASES]
MODES = [False, True]
D64 = torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def g29():
    return np.load(os.path.join(HERE, "golden", "g29_calql.npz"))


def make_q(case, prec="fp32", **kw):
    from dppo_amd.model.common.critic import CriticObsAct
    od, ta, da, dims, act, _, _ = K.CALQL_NETS[case]
    return CriticObsAct(**dict(dict(cond_dim=od, mlp_dims=dims, action_dim=da, action_steps=ta, activation_type=act, use_layernorm=True,
                                    double_q=True, twin_layernorm=True, precision=prec), **kw))


def make_model(case, n, prec, device, per_row=False):
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_calql import CalQL_Gaussian
    od, ta, da, dims, act, R, S = K.CALQL_NETS[case]
    actor = Gaussian_MLP(da, ta, od, mlp_dims=dims, activation_type=act, tanh_output=False, fixed_std=None, std_min=K.S.STD_MIN,
                         std_max=K.S.STD_MAX, precision=prec)
    actor.load_state_dict(K.actor_params(case), strict=True)
    lo, hi = K.clips_of(case, n, per_row)
    m = CalQL_Gaussian(actor=actor, critic=make_q(case, prec), cql_clip_diff_min=lo, cql_clip_diff_max=hi,
                       cql_min_q_weight=K.MIN_Q_WEIGHT, cql_n_actions=S, per_row_logpi=per_row, horizon_steps=ta, device=device,
                       randn_clip_value=K.S.RANDN_CLIP, tanh_output=True)
    m.critic.load_state_dict(K.twin_params(case), strict=True)
    m.target_critic.load_state_dict(K.twin_params(case, K.TARGET_EPS), strict=True)
    return m


def restate(case, n, per_row=False, dtype=D64, bf16=False, gates=None):
    q = K.RL.leaf(K.twin_params(case), dtype)
    args = (q, K.twin_params(case, K.TARGET_EPS), case, K.inputs(case, n), K.samples(case, n), K.returns_of(case, n, per_row))
    kw = dict(per_row=per_row, clips=K.clips_of(case, n, per_row), dtype=dtype)
    with gates if gates is not None else K.relu_gates() as rg:
        if bf16:
            with K.bf16_linears():
                res = K.loss_critic(*args, **kw)
        else:
            res = K.loss_critic(*args, **kw)
    res["named"] = list(zip(q, res["grads"]))
    res["near_zero"] = rg.near_zero()
    return res


@functools.lru_cache(maxsize=None)
def restated(case, n, per_row=False):
    """The float64 restatement of one case in one mode: computed once, shared, never modified."""
    return restate(case, n, per_row)


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_restatement_reproduces_the_reference_in_float32(g29, case, n):
    """Reference mode: the loss to 1e-6 relative, the other statistics by the same rule, every gradient of both trunks by the
    gradient rule on the fixture's stored form.  (The reference forms the (N, R + 2 N) matrix; the restatement the R + 2 columns.)"""
    r, name = restate(case, n, dtype=torch.float32), f"{case}_{n}"
    ref = g29[f"{name}_stats"]
    print(f"{name}: restated {r['stats']} reference {ref}")
    assert abs(r["stats"][0] - ref[0]) <= 1e-6 * abs(ref[0])
    np.testing.assert_allclose(r["stats"], ref, rtol=1e-6, atol=1e-6)
    check_grads_fp32(g29, f"{name}_gq", r["named"])


def test_per_row_mode_is_another_loss():
    """The broadcast matters: the paper's per-row weights give a different loss on the same inputs."""
    a, b = restated("tiny", 77, False), restate("tiny", 77, True)
    b_same = K.loss_critic(K.RL.leaf(K.twin_params("tiny"), D64), K.twin_params("tiny", K.TARGET_EPS), "tiny", K.inputs("tiny", 77),
                           K.samples("tiny", 77), K.returns_of("tiny", 77, False), per_row=True, dtype=D64)
    assert abs(a["stats"][0] - b_same["stats"][0]) > 1.0 and abs(a["stats"][1] - b["stats"][1]) < 1e-12


@pytest.mark.parametrize("per_row", MODES)
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_constructed_inputs_keep_their_guard_bands(case, n, per_row):
    """On the float64 restatement: every one of the 4 N calibration comparisons, and every clamp comparison of tiny_clip, is at least
    GUARD from its threshold; outside N = 1 at least a quarter of the calibration comparisons bind and a quarter do not; tiny_clip
    has rows clipped on each side and rows that pass; no pre-LayerNorm row sits where eps decides."""
    r, ret = restated(case, n, per_row), K.returns_of(case, n, per_row).double()
    assert K.GUARD == 8 * K.BF16_Q_ERR
    q4 = torch.stack([r["rows"][0][2], r["rows"][1][2], r["rows"][0][3], r["rows"][1][3]], dim=1)
    assert (q4 - ret[:, None]).abs().min().item() >= K.GUARD
    bind = (q4 < ret[:, None]).double().mean().item()
    if n > 1:
        assert 0.25 <= bind <= 0.75, bind
    lo, hi = K.clips_of(case, n, per_row)
    d = torch.stack(r["diffs"])
    if case == "tiny_clip":
        assert math.isfinite(lo) and math.isfinite(hi) and np.float32(lo) == lo and np.float32(hi) == hi
        assert min((d - lo).abs().min().item(), (d - hi).abs().min().item()) >= K.GUARD
        assert (d < lo).any() and (d > hi).any() and ((d > lo) & (d < hi)).any()
    else:
        assert lo == -math.inf and hi == math.inf
    b, sm = K.inputs(case, n), K.samples(case, n)
    for i in (1, 2):
        p = K.RL.cast(K.trunk(K.twin_params(case), i), D64)
        with K._lent(case) as key:
            var = K.RL.pre_ln_variances(p, key, b["obs"].double(), sm["pi_actions"].double())
        assert min(v.min().item() for v in var) > K.VAR_FLOOR
    assert all((v.abs() <= 1).all() for k, v in sm.items() if k.endswith("actions"))


def test_twin_layernorm_critic_is_opt_in_and_carries_the_references_state_dict(g29):
    from dppo_amd.model.common.critic import CriticObsAct
    with pytest.raises(NotImplementedError):  # the bare combination stays refused
        CriticObsAct(cond_dim=11, mlp_dims=[64, 64], action_dim=3, use_layernorm=True, double_q=True)
    q = make_q("kitchen")
    assert q.twin_layernorm and q.double_q
    keys = [k[len("critic."):] for k in g29["state_dict_keys"] if k.startswith("critic.")]
    assert list(q.state_dict()) == keys == list(K.twin_params("kitchen"))
    assert not make_q("tiny", use_layernorm=False).twin_layernorm  # the keyword alone turns nothing on
    q.load_state_dict(K.twin_params("kitchen"), strict=True)
    flat, d = q.flat_params(), q.net_desc()
    P = hip.load().dppo_net_param_count(C.byref(d))
    assert (d.plain, d.use_layernorm, d.kind) == (1, 1, 1) and flat.numel() == 2 * P == q._abi_param_count()
    assert torch.equal(flat, torch.cat([v.reshape(-1) for v in K.twin_params("kitchen").values()]))
    # the double_q = 1 forward query on a LayerNorm descriptor stays refused: the twin's forward runs one trunk per call
    assert hip.load().dppo_idql_q_forward_workspace_bytes(C.byref(d), hip.PREC_F32, 77, 1) == -1


def test_every_shipped_calql_model_builds():
    """All 16 calql_mlp_*.yaml of the reference (tests/golden/shipped_calql_cfgs.json, settings only, text unchanged): the model
    target resolves to CalQL_Gaussian and builds through ``instantiate`` (a finetune cfg's checkpoint path is set aside: there is no
    such file), its critic is the LayerNorm twin, the state-dict keys are the fixture's, the C ABI counts one trunk's parameters, the
    flat image is 2 P and the workspace query accepts (batch_size, n_random_actions, cql_n_actions) in both precisions."""
    from dppo_amd.cfg.loader import get_class, instantiate, load_config
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.rl.gaussian_calql import CalQL_Gaussian
    cfgs = load_config(os.path.join(HERE, "golden", "shipped_calql_cfgs.json"))
    assert len(cfgs) == 16 and all(os.path.basename(k).startswith("calql_mlp_") for k in cfgs)
    lib, seen = hip.load(), set()
    for name, cfg in cfgs.items():
        assert cfg._target_.endswith("train_calql_agent.TrainCalQLAgent"), name
        assert get_class(cfg.model._target_) is CalQL_Gaussian and get_class(cfg.model.critic._target_) is CriticObsAct, name
        assert cfg.model.critic.use_layernorm is True and cfg.model.critic.double_q is True and "twin_layernorm" not in cfg.model.critic
        m = instantiate(cfg.model, network_path=None)
        q, dims = m.critic, list(cfg.model.critic.mlp_dims)
        assert q.twin_layernorm and m.target_critic.twin_layernorm and m.target_critic is not q, name
        trunk = [f"moduleList.{i}.{mod}.{w}" for i in range(len(dims) + 1)
                 for mod in (("linear_1", "norm_1") if i < len(dims) else ("linear_1",)) for w in ("weight", "bias")]
        keys = [k for k in m.state_dict() if not k.startswith("network.")]
        assert keys == [f"{box}.Q{i}.{k}" for box in ("critic", "target_critic") for i in (1, 2) for k in trunk], name
        dq = q.net_desc()
        od, af = cfg.obs_dim * cfg.cond_steps, cfg.action_dim * cfg.horizon_steps
        assert (dq.kind, dq.plain, dq.use_layernorm, dq.in_dim, dq.hidden, dq.n_blocks) == (1, 1, 1, od + af, dims[0], len(dims) - 1), name
        P = lib.dppo_net_param_count(C.byref(dq))
        assert P == sum(p.numel() for p in q.Q1.parameters()) and q.flat_params().numel() == 2 * P, name
        assert m.cql_min_q_weight == float(cfg.model.cql_min_q_weight) and m.cql_n_actions == 10 and not m.per_row_logpi
        assert m.cql_clip_diff_min == -math.inf and m.cql_clip_diff_max == math.inf
        seen.add((od, af, len(dims), int(cfg.train.n_random_actions)))
        for prec in (hip.PREC_F32, hip.PREC_BF16):
            assert lib.dppo_calql_q_loss_workspace_bytes(C.byref(dq), prec, od, int(cfg.train.batch_size), int(cfg.train.n_random_actions),
                                                         m.cql_n_actions) > 0, lib.dppo_last_error()
    assert (60, 9, 3, 10) in seen and (17, 6, 2, 4) in seen


def test_instantiate_merges_declared_child_defaults_only_where_asked():
    """A class that declares nothing behaves as before; a key the node already has wins over the default."""
    from dppo_amd.cfg.loader import instantiate
    node = {"_target_": "dppo.model.common.critic.CriticObsAct", "cond_dim": 11, "mlp_dims": [64, 64], "action_dim": 3,
            "use_layernorm": True, "double_q": True}
    with pytest.raises(NotImplementedError):
        instantiate(node)
    actor = {"_target_": "dppo.model.common.mlp_gaussian.Gaussian_MLP", "action_dim": 3, "horizon_steps": 1, "cond_dim": 11,
             "mlp_dims": [64, 64], "activation_type": "ReLU", "tanh_output": False}
    model = {"_target_": "dppo.model.rl.gaussian_calql.CalQL_Gaussian", "actor": actor, "critic": dict(node), "horizon_steps": 1,
             "device": "cpu", "tanh_output": True}
    assert instantiate(model).critic.twin_layernorm and "twin_layernorm" not in model["critic"]
    model["critic"]["twin_layernorm"] = False
    with pytest.raises(NotImplementedError):
        instantiate(model)


def test_calql_model_loads_actor_critic_and_target_from_network_path(tmp_path):
    m = make_model("tiny", 77, "fp32", "cpu")
    sd = {k: v + 1.0 for k, v in m.state_dict().items()}
    torch.save({"model": sd}, tmp_path / "state.pt")
    from dppo_amd.model.rl.gaussian_calql import CalQL_Gaussian
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    actor = Gaussian_MLP(3, 1, 11, mlp_dims=[64, 64], activation_type="ReLU", tanh_output=False, fixed_std=None, std_min=K.S.STD_MIN,
                         std_max=K.S.STD_MAX)
    m2 = CalQL_Gaussian(actor=actor, critic=make_q("tiny"), network_path=str(tmp_path / "state.pt"), horizon_steps=1, device="cpu",
                        tanh_output=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(ValueError, match="twin"):
        from tests.test_sac import make_q as plain_twin
        CalQL_Gaussian(actor=actor, critic=plain_twin("tiny"), horizon_steps=1, device="cpu", tanh_output=True)


def test_calql_entry_rejects_bad_arguments_on_the_host():
    """Every refusal leaves its reason in dppo_last_error(); nothing here touches a device (the pointers are never read)."""
    lib, d = hip.load(), make_q("tiny").net_desc()
    err = lambda: lib.dppo_last_error()
    ws_bytes = lambda desc=d, N=77, od=11, R=4, S=3, prec=hip.PREC_F32: lib.dppo_calql_q_loss_workspace_bytes(C.byref(desc), prec, od, N, R, S)
    assert ws_bytes() > 0 and ws_bytes(R=64, S=64) > 0 and ws_bytes(R=1, S=1) > 0
    for R in (0, 65, -1):
        assert ws_bytes(R=R) == -1 and b"n_random" in err()
    for S in (0, 65):
        assert ws_bytes(S=S) == -1 and b"n_next" in err()
    assert ws_bytes(prec=7) == -1 and b"prec" in err()
    assert ws_bytes(N=0) == -1 and b"N out of range" in err()
    assert ws_bytes(N=1 << 30) == -1 and b"N out of range" in err()
    assert ws_bytes(od=14) == -1 and b"obs_dim" in err()
    plain = hip.NetDesc.from_buffer_copy(d)
    plain.use_layernorm = 0
    assert ws_bytes(plain) == -1 and b"LayerNorm" in err()
    res = hip.NetDesc(kind=1, in_dim=14, hidden=256, n_blocks=1, out_dim=1, act=hip.ACT_RELU, time_dim=0, act_flat=0, cond_dim=14,
                      cond_hidden=0, cond_out=0, use_layernorm=1, plain=0)
    assert ws_bytes(res) == -1 and b"plain" in err()
    den = hip.NetDesc(kind=0, in_dim=3 + 16 + 11, hidden=64, n_blocks=1, out_dim=3, act=hip.ACT_RELU, time_dim=16, act_flat=3,
                      cond_dim=11, cond_hidden=0, cond_out=0, use_layernorm=0, plain=1)
    assert ws_bytes(den) == -1 and b"kind-1" in err()
    one = C.c_double(0)  # stands in for every pointer: refusals come before anything is read
    ptr = C.addressof(one)
    batch = hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 0, 77)
    names = ("q_params", "q1", "q2", "t_params", "t1", "t2", "returns", "next_a", "pi_a", "lp", "pi_na", "lpn", "q_grad", "stats", "ws")

    def call(desc=d, prec=hip.PREC_F32, N=77, gamma=0.99, wsb=1 << 40, cfg=None, null=None, **c):
        if cfg is None:
            cfg = hip.CalqlCfg(**dict(dict(n_random=4, n_next=3, per_row_logpi=0, min_q_weight=5.0, clip_diff_min=-math.inf,
                                           clip_diff_max=math.inf, log_rand_pi=0.125), **c))
        p = {k: (None if k == null else ptr) for k in names}
        return lib.dppo_calql_q_loss_fwd_bwd(C.byref(desc), prec, p["q_params"], p["q1"], p["q2"], p["t_params"], p["t1"], p["t2"],
                                             C.byref(cfg), C.byref(batch), 11, p["returns"], p["next_a"], p["pi_a"], p["lp"],
                                             p["pi_na"], p["lpn"], None, N, gamma, p["q_grad"], p["stats"], None, None, p["ws"], wsb, None)
    assert call(n_random=0) == -1 and b"n_random" in err()
    assert call(n_random=65) == -1 and b"n_random" in err()
    assert call(n_next=0) == -1 and b"n_next" in err()
    assert call(clip_diff_min=1.0, clip_diff_max=0.5) == -1 and b"clip_diff_min" in err()
    assert call(clip_diff_min=math.nan) == -1 and b"clip_diff_min" in err()
    assert call(min_q_weight=-1.0) == -1 and b"min_q_weight" in err()
    for k in names:
        assert call(null=k) == -1 and b"null pointer" in err(), k
    assert call(prec=5) == -1 and b"prec" in err()
    assert call(N=0) == -1 and b"N out of range" in err()
    assert call(gamma=1.5) == -1 and b"gamma" in err()
    assert call(desc=plain) == -1 and b"LayerNorm" in err()
    assert call(desc=res) == -1 and b"plain" in err()
    assert call(desc=den) == -1 and b"kind-1" in err()
    assert call(wsb=1024) == -1 and b"workspace too small" in err()
    assert lib.dppo_version() == 1


def test_loss_actor_is_the_follow_up_and_there_is_no_cpu_fallback():
    m = make_model("tiny", 77, "fp32", "cpu")
    with pytest.raises(NotImplementedError, match="follow-up"):
        m.loss_actor({"state": torch.zeros(2, 1, 11)}, 0.7)
    b, sm = K.inputs("tiny", 77), K.samples("tiny", 77)
    with pytest.raises(hip.DppoHipError):
        m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], b["random_actions"], b["reward"],
                      K.returns_of("tiny", 77), b["terminated"], K.GAMMA, samples=sm)
    with pytest.raises(hip.DppoHipError):
        m.critic({"state": b["obs"]}, b["actions"])


# ------------------------------------------------------------------------------------------------------------------ GPU
def named_grads(m):
    """(name, slice of the [2][P] gradient) in the flat image's order."""
    q, out, off = m.critic, [], 0
    g, names = q.flat_grads(), {id(p): k for k, p in m.critic.named_parameters()}
    for p in q.trunk_parameters():
        out.append((names[id(p)], g[off:off + p.numel()].view(p.shape).clone()))
        off += p.numel()
    assert off == g.numel()
    return out


def run_critic(m, case, n, per_row, replay=None, inds=None, random_actions="given", **kw):
    b = {k: v.to(DEV) for k, v in K.inputs(case, n).items()}
    sm = {k: v.to(DEV) for k, v in K.samples(case, n).items()}
    ra = b["random_actions"] if isinstance(random_actions, str) else random_actions
    ret = K.returns_of(case, n, per_row).to(DEV)
    kw = dict(dict(samples=sm), **kw)
    if replay is not None:
        loss = m.loss_critic(replay, None, None, ra, None, ret, None, K.GAMMA, inds=inds, **kw)
    else:
        loss = m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], ra, b["reward"], ret, b["terminated"], K.GAMMA, **kw)
    return dict(loss=loss.detach(), stats=m.last_stats.cpu().numpy().copy(), y=m.last_y.cpu().clone(), grads=m.critic.flat_grads().clone())


def check_with_gates(case, n, per_row, got, what):
    """tests/test_rlpd.py::check_with_gates on this file's restatement."""
    ref = restated(case, n, per_row)
    bad = grad_violations(ref["named"], got)
    if not bad or K.CALQL_NETS[case][4] != "ReLU":
        assert not bad, (what, bad)
        return
    count = lambda b: sum(x[1] + int(x[3]) for x in b)
    print(f"{what}: {count(bad)} entries outside the rule {bad}; {len(ref['near_zero'])} ReLU gates below {K.RELU_TIE:g}")
    force = {}
    for z, where, gate in ref["near_zero"]:
        trial = dict(force)
        trial[where] = not gate
        now = grad_violations(restate(case, n, per_row, gates=K.relu_gates(trial))["named"], got)
        if count(now) < count(bad):
            force, bad = trial, now
        if not bad:
            return
    assert not bad, (what, bad, force)


@pytest.mark.gpu
@pytest.mark.parametrize("per_row", MODES, ids=["reference", "per_row"])
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_calql_loss_critic_fp32(case, n, per_row):
    m, ref = make_model(case, n, "fp32", DEV, per_row), restated(case, n, per_row)
    res = run_critic(m, case, n, per_row)
    stats_close(res["stats"], ref["stats"], f"{case}_{n} per_row={per_row}")
    stats_close(res["y"].numpy(), ref["y"].numpy(), f"{case}_{n} y")
    assert float(res["loss"]) == np.float32(res["stats"][0])
    check_with_gates(case, n, per_row, named_grads(m), f"{case}_{n} per_row={per_row}")
    again = run_critic(m, case, n, per_row)
    assert torch.equal(res["grads"], again["grads"]) and np.array_equal(res["stats"], again["stats"]) and torch.equal(res["y"], again["y"])


@pytest.mark.gpu
@pytest.mark.parametrize("per_row", MODES, ids=["reference", "per_row"])
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_calql_loss_critic_bf16_within_twice_the_rounding_yardstick(case, n, per_row):
    """e_c <= 2 e_y on the loss, on 1 - cosine and per tensor, as tests/test_rlpd.py.  The six statistics are held the same way plus
    the floor n 2^-24: a statistic is a mean over n rows that the fp32 restatement, from which both errors are measured, sums in fp32
    (worst case n ulps of 2^-24) and the call in double.  Without the floor a statistic that bf16 cannot move -- tiny_clip's mean
    difference where a trunk's rows are pinned to the clip values: e_y = 0 exactly, the call 3.8e-8 off -- would ask for the
    restatement's own summation order."""
    m = make_model(case, n, "bf16", DEV, per_row)
    res = run_critic(m, case, n, per_row)
    fp32, yard = restate(case, n, per_row, torch.float32), restate(case, n, per_row, torch.float32, bf16=True)
    z = torch.zeros(1)
    for r in (fp32, yard):
        r["d_a"] = z
    call = dict(loss=res["stats"][0], d_a=z, named=named_grads(m))
    e_y, e_c = rel_errors(fp32, yard), rel_errors(fp32, call)
    worst = max(e_c["per"], key=lambda k: e_c["per"][k] / (e_y["per"][k] + 1e-30))
    s_err = lambda s: np.abs(np.asarray(s, dtype=np.float64) - np.asarray(fp32["stats"])) / np.maximum(1.0, np.abs(fp32["stats"]))
    s_y, s_c = s_err(yard["stats"]), s_err(res["stats"])
    print(f"{case}_{n} per_row={per_row} bf16: yardstick loss {e_y['loss']:.3e} 1-cos {e_y['one_minus_cos']:.3e}; call loss {e_c['loss']:.3e} "
          f"1-cos {e_c['one_minus_cos']:.3e}; worst tensor {worst}: {e_c['per'][worst]:.3e} against {e_y['per'][worst]:.3e}; "
          f"stats yardstick {s_y} call {s_c}")
    assert e_c["loss"] <= 2 * e_y["loss"] and e_c["one_minus_cos"] <= 2 * e_y["one_minus_cos"]
    assert (s_c <= 2 * s_y + n * 2.0 ** -24).all(), (s_c, s_y)
    for k in e_c["per"]:
        assert e_c["per"][k] <= 2 * e_y["per"][k], (k, e_c["per"][k], e_y["per"][k])


@pytest.mark.gpu
def test_hip_twin_layernorm_forward():
    """Both trunks' Q through one dppo_idql_q_forward each against the float64 restatement, and with obs_repeat."""
    case, n = "chunk", 77
    b, q = K.inputs(case, n), make_q(case)
    q.load_state_dict(K.twin_params(case), strict=True)
    q = q.to(DEV)
    act = torch.cat([b["actions"], b["actions"].flip(0)])
    got = [q({"state": b["obs"].to(DEV)}, b["actions"].to(DEV)), q({"state": b["obs"].to(DEV)}, act.to(DEV), obs_repeat=2)]
    for i in (1, 2):
        p = K.RL.cast(K.trunk(K.twin_params(case), i), D64)
        with torch.no_grad():
            ref = K.q_forward(p, case, b["obs"].double(), b["actions"].double())
            ref2 = K.q_forward(p, case, torch.cat([b["obs"], b["obs"]]).double(), act.double())
        stats_close(got[0][i - 1].cpu().numpy(), ref.numpy(), f"Q{i}")
        stats_close(got[1][i - 1].cpu().numpy(), ref2.numpy(), f"Q{i} obs_repeat")


@pytest.mark.gpu
def test_hip_calql_in_kernel_random_actions():
    """random_actions=None: uniform draws in [-1, 1) keyed by the CPU generator's seed, left in last_random_actions; handing them
    back gives the same bits."""
    case, n = "chunk", 77
    m = make_model(case, n, "fp32", DEV)
    R, (od, ta, da) = 10, K.shapes(case)
    m.n_random_actions = R
    torch.manual_seed(5)
    a = run_critic(m, case, n, False, random_actions=None)
    ra = m.last_random_actions.clone()
    assert ra.shape == (n, R, ta, da) and ra.dtype == torch.float32
    assert float(ra.min()) >= -1.0 and float(ra.max()) < 1.0
    assert abs(float(ra.double().mean())) <= 4.0 / math.sqrt(3.0 * n * R * ta * da)
    assert ra.unique().numel() > 0.99 * ra.numel()
    torch.manual_seed(6)
    run_critic(m, case, n, False, random_actions=None)
    assert not torch.equal(ra, m.last_random_actions)
    back = run_critic(m, case, n, False, random_actions=ra)
    assert m.last_random_actions is None
    assert torch.equal(a["grads"], back["grads"]) and np.array_equal(a["stats"], back["stats"])
    torch.manual_seed(5)
    run_critic(m, case, n, False, random_actions=None)
    assert torch.equal(ra, m.last_random_actions)  # the same seed, the same draws


@pytest.mark.gpu
def test_hip_calql_ring_equals_arrays_and_backward_hands_out_the_slices():
    from tests.test_qsm import ring_of
    case, n = "tiny", 77
    m = make_model(case, n, "fp32", DEV)
    res = run_critic(m, case, n, False)
    got = dict(named_grads(m))
    rp, inds = ring_of({k: v.to(DEV) for k, v in K.inputs(case, n).items()}, n)
    ring = run_critic(m, case, n, False, replay=rp, inds=inds)
    assert torch.equal(res["grads"], ring["grads"]) and np.array_equal(res["stats"], ring["stats"]) and torch.equal(res["y"], ring["y"])
    b = {k: v.to(DEV) for k, v in K.inputs(case, n).items()}
    loss = m.loss_critic(rp, None, None, b["random_actions"], None, K.returns_of(case, n).to(DEV), None, K.GAMMA, inds=inds,
                         samples={k: v.to(DEV) for k, v in K.samples(case, n).items()})
    loss.backward()
    w = m.critic.Q2.moduleList[0].norm_1.weight
    assert torch.equal(w.grad, got["Q2.moduleList.0.norm_1.weight"])


@pytest.mark.gpu
def test_hip_calql_samples_come_from_one_forward():
    """Without ``samples`` the three policy samples are ONE forward over N (S + 2) stacked rows [next_obs x S | obs | next_obs] with
    ``noise`` as its draws; the loss is bit for bit the one of the same samples handed over."""
    case, n = "tiny", 77
    m = make_model(case, n, "fp32", DEV)
    b, (R, S) = {k: v.to(DEV) for k, v in K.inputs(case, n).items()}, K.n_samples(case)
    calls, real = [], m.forward

    def forward(cond, **kw):
        out = real(cond, **kw)
        calls.append((cond["state"].clone(), out))
        return out
    object.__setattr__(m, "forward", forward)
    a = run_critic(m, case, n, False, samples=None, noise=b["noise"])
    assert len(calls) == 1 and calls[0][0].shape[0] == n * (S + 2)
    cur, nxt = b["obs"].reshape(n, -1), b["next_obs"].reshape(n, -1)
    assert torch.equal(calls[0][0], torch.cat([nxt.repeat_interleave(S, dim=0), cur, nxt]))
    act, lp = calls[0][1]
    act = act.reshape(n * (S + 2), -1)
    sm = dict(next_actions=act[:n * S], pi_actions=act[n * S:n * S + n], log_pi=lp[n * S:n * S + n], pi_next_actions=act[n * S + n:],
              log_pi_next=lp[n * S + n:])
    back = run_critic(m, case, n, False, samples=sm)
    assert len(calls) == 1
    assert torch.equal(a["grads"], back["grads"]) and np.array_equal(a["stats"], back["stats"])


@pytest.mark.gpu
def test_hip_calql_polyak_moves_the_whole_target_twin():
    m = make_model("tiny", 77, "fp32", DEV)
    t0, s0 = m.target_critic.flat_params().clone(), m.critic.flat_params().clone()
    m.update_target_critic(0.005)
    want = t0 * np.float32(1 - 0.005) + s0 * np.float32(0.005)
    assert torch.equal(m.target_critic.flat_params(), want)
    P = want.numel() // 2
    assert torch.equal(m.target_critic.Q2.moduleList[1].norm_1.bias.reshape(-1), want[P:][-(64 + 1 + 64):-(64 + 1)])
    assert not torch.equal(want[P:], t0[P:]) and not torch.equal(want[:P], t0[:P])
