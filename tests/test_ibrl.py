"""IBRL's model (reference model/rl/gaussian_ibrl.py): the dropout actor on a plain fixed-std trunk, the Q-guided choice between the
imitation policy's proposal and the online actor's (``dppo_ibrl_act``), and the ensemble's TD loss whose target bootstraps from the
better of the two proposals (``dppo_ibrl_q_loss_fwd_bwd``).

CPU.  The plain-torch restatement of tests/golden/make_golden_ibrl_cases.py reproduces the reference (tests/golden/g31_ibrl.npz,
written by make_golden_ibrl.py from the reference's own classes) in float32: the loss to 1e-6 relative, every member's gradient by
check_grads_fp32, took_bc equal and the chosen actions bit for bit.  The constructed inputs keep their guard bands on the float64
restatement, so that no choice hangs on an fp32 rounding.  Every shipped cfg builds with its text unchanged, the state dict is the
reference's, and everything the model, the actor and the three library entries cannot run is refused with a message.

GPU, fp32.  Held to the restatement in FLOAT64 fed the same fp32 values: the actor's mean and sample under a given mask within 2e-5
(tests/test_sac.py's bound for SAC's sample), Q values and statistics by stats_close, every member's gradient by grad_violations
under tests/test_rlpd.py's check_with_gates (its code, run on this file's restatement), took_bc against the fixture and against the
rule applied to the call's own Q values, the action against the chosen proposal bit for bit.

GPU, bf16.  No tolerance is fixed: errors are measured against the fp32 restatement and stay within twice those of the restatement
with every Linear's operands rounded to bf16, on the loss, on 1 - cosine and per tensor; the statistics get tests/test_calql.py's
floor n 2^-24; took_bc is held only to the rule on the call's own Q values.
"""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest
import torch

from dppo_amd import hip
from tests import test_rlpd as R
from tests.golden import make_golden_ibrl_cases as K
from tests.test_dql import grad_violations, rel_errors, stats_close
from tests.test_idql import check_grads_fp32
from tests.test_qsm import ring_of

DEV = "cuda:0"
IDS = [f"{c}_{n}" for c, n in K.CASES]
D64 = torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE_TOL = 2e-5  # tests/test_sac.py::test_hip_sac_sample_fp32's bound on an action


@pytest.fixture(scope="module")
def g31():
    return np.load(os.path.join(HERE, "golden", "g31_ibrl.npz"))


def make_actor(case, prec="fp32", **kw):
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    od, ta, da, dims, act, p = K.IBRL_NETS[case][:6]
    return Gaussian_MLP(**dict(dict(action_dim=da, horizon_steps=ta, cond_dim=od, mlp_dims=list(dims), activation_type=act, dropout=p,
                                    fixed_std=K.FIXED_STD, precision=prec, plain_fixed_std=True), **kw))


def make_q(case, prec="fp32", **kw):
    from dppo_amd.model.common.critic import CriticObsAct
    od, ta, da = K.shapes(case)
    return CriticObsAct(**dict(dict(cond_dim=od, mlp_dims=list(K.IBRL_NETS[case][6]), action_dim=da, action_steps=ta,
                                    activation_type=K.IBRL_NETS[case][7], use_layernorm=True, double_q=False, precision=prec), **kw))


def make_model(case, prec, device, soft=False):
    from dppo_amd.model.rl.gaussian_ibrl import IBRL_Gaussian
    m = IBRL_Gaussian(actor=make_actor(case, prec), critic=make_q(case, prec), n_critics=K.n_critics(case), soft_action_sample=soft,
                      soft_action_sample_beta=K.BETA, horizon_steps=K.shapes(case)[1], device=device, randn_clip_value=K.RANDN_CLIP)
    for name, net in (("bc", m.bc_policy), ("rl", m.network), ("target", m.target_actor)):
        net.load_state_dict(K.actor_state_dict(case, name), strict=True)
    for e in range(K.n_critics(case)):
        m.critic_networks[e].load_state_dict(K.member_params(case, e), strict=True)
        m.target_networks[e].load_state_dict(K.member_params(case, e, K.TARGET_EPS), strict=True)
    return m


def restate_critic(case, n, dtype=D64, bf16=False, gates=None):
    E = K.n_critics(case)
    members = [K.leaf(K.member_params(case, e), dtype) for e in range(E)]
    targets = [K.member_params(case, e, K.TARGET_EPS) for e in range(E)]
    args = (members, targets, case, K.inputs(case, n), K.pair_of(case))
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


@functools.lru_cache(maxsize=None)
def restated_forward(case, n, soft, dtype=D64, bf16=False):
    if bf16:
        with K.bf16_linears():
            return K.forward(case, K.forward_inputs(case, n), K.pair_of(case), soft, dtype=dtype)
    return K.forward(case, K.forward_inputs(case, n), K.pair_of(case), soft, dtype=dtype)


# tests/test_rlpd.py's check_with_gates, its own code object, run against this file's restatement: the function reads
# ``restated_critic``, ``restate_critic`` and the cases module ``K`` from its globals, which are rebound here and nowhere else
_gate_globals = dict(R.__dict__)
_gate_globals.update(restated_critic=restated_critic, restate_critic=restate_critic,
                     K=types.SimpleNamespace(RLPD_NETS={c: (None,) * 4 + (v[7],) for c, v in K.IBRL_NETS.items()}, RELU_TIE=K.RELU_TIE,
                                             relu_gates=K.relu_gates))
check_with_gates = types.FunctionType(R.check_with_gates.__code__, _gate_globals, "check_with_gates")
named_grads = R.named_grads


def dev_inputs(b):
    return {k: v.to(DEV) for k, v in b.items()}


def member_flats(case, r):
    """One flat vector per member from a restatement's gradient lists: the fixture's form."""
    return [(str(e), torch.cat([g.reshape(-1) for g in gs])) for e, gs in enumerate(r["grads"])]


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_restatement_reproduces_the_reference_in_float32(g31, case, n):
    """tests/test_calql.py's rule: the loss to 1e-6 relative, the statistics likewise, y per row by stats_close, every member's gradient by
    check_grads_fp32 on the fixture's stored form; ``forward``, greedy and soft: took_bc equal (the row where both weights overflow,
    stored as 2 because the reference raises there, takes the greedy rule) and the chosen actions bit for bit."""
    r, name = restate_critic(case, n, dtype=torch.float32), f"{case}_{n}"
    ref = g31[f"{name}_stats"]
    print(f"{name}: restated {r['stats']} reference {ref}")
    assert abs(r["stats"][0] - float(g31[f"{name}_c_loss"])) <= 1e-6 * abs(float(g31[f"{name}_c_loss"]))
    np.testing.assert_allclose(r["stats"], ref, rtol=1e-6, atol=1e-6)
    stats_close(r["y"].numpy(), g31[f"{name}_y"], f"{name} y")  # per row: two fp32 evaluations of a trunk, the QSM / DQL tests' rule
    assert r["bc_share"] == float(g31[f"{name}_bc_share"])
    check_grads_fp32(g31, f"{name}_gq", member_flats(case, r))
    for soft in (False, True):
        f, key = restated_forward(case, n, soft, torch.float32), f"{name}_{'soft' if soft else 'greedy'}"
        took = g31[f"{key}_took_bc"]
        mine = f["took_bc"].numpy().astype(np.uint8)
        assert np.array_equal(mine[took != 2], took[took != 2]), key
        if soft:
            assert np.array_equal(np.nonzero(took == 2)[0], np.nonzero(f["nan_rows"].numpy())[0]), key
            greedy = restated_forward(case, n, False, torch.float32)
            assert np.array_equal(mine[took == 2], (greedy["q_bc"] > greedy["q_rl"]).numpy().astype(np.uint8)[took == 2])
        keep = took != 2
        assert np.array_equal(f["action"].numpy()[keep], g31[f"{key}_action"][keep]), key
    g = restated_forward(case, n, False, torch.float32)
    assert np.array_equal(g["a_bc"].numpy(), g31[f"{name}_a_bc"]) and np.array_equal(g["a_rl"].numpy(), g31[f"{name}_a_rl"])


@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_constructed_inputs_keep_their_guard_bands(case, n):
    """On the float64 restatement (DESIGN 18's rule for ``sel``: ten times the fp32 ceiling Q_CEIL): every non-tie |mb - mr| of the
    target and every non-tie |min q_bc - min q_rl| of greedy ``forward``; every |u - p_bc| at least U_BAND; every ||z| - randn_clip|
    at least CLIP_BAND.  The tie row's proposals are equal and its two Q are equal; on the overflow row both beta q clear fp32's exp
    range by more than ten ceilings of beta q, and on no other row either does."""
    tie, ovf = K.special_rows(n)
    rest = torch.ones(n, dtype=torch.bool)
    if tie is not None:
        rest[tie] = False
    r = restated_critic(case, n)
    assert ((r["mb"] - r["mr"]).abs()[rest] >= 10 * K.Q_CEIL).all()
    g, s = restated_forward(case, n, False), restated_forward(case, n, True)
    assert ((g["q_bc"] - g["q_rl"]).abs()[rest] >= 10 * K.Q_CEIL).all()
    fb = K.forward_inputs(case, n)
    ok = ~s["nan_rows"]
    assert ((fb["u"].double() - s["p_bc"])[ok].abs() >= K.U_BAND).all()
    for b in (fb, K.inputs(case, n)):
        for z in (b["noise_bc"], b["noise_rl"]):
            assert ((z.abs() - K.RANDN_CLIP).abs() >= K.CLIP_BAND).all()
        assert (b["noise_rl"].abs() > K.RANDN_CLIP).any() or n == 1
    if tie is not None:
        assert torch.equal(g["a_bc"][tie], g["a_rl"][tie]) and g["q_bc"][tie] == g["q_rl"][tie] and not g["took_bc"][tie]
        assert torch.equal(r["a_bc"][tie], r["a_rl"][tie]) and r["mb"][tie] == r["mr"][tie]
        margin = 10 * K.BETA * K.Q_CEIL * 20  # |q| up to 20
        for q in (s["q_bc"], s["q_rl"]):
            assert q[ovf] * K.BETA > K.EXP_OVERFLOW + margin
            others = torch.ones(n, dtype=torch.bool)
            others[ovf] = False
            assert (q[others] * K.BETA < K.EXP_OVERFLOW - margin).all()
        assert s["nan_rows"][ovf] and int(s["nan_rows"].sum()) == 1
        assert 0 < int(g["took_bc"].sum()) < n - 1 and 0 < r["bc_share"] < 1
        assert ((s["p_bc"][ok] - 0.5).abs() < 0.49).sum() >= 5 and (s["took_bc"] != g["took_bc"]).any()  # the soft draw is no greedy pick
    print(f"{case}_{n}: {len(r['near_zero'])} ReLU gates below {K.RELU_TIE:g} in the critic restatement")


def test_every_shipped_ibrl_model_builds():
    """All eight ibrl_mlp*.yaml of the reference (tests/golden/shipped_ibrl_cfgs.json, settings only, text unchanged): the model target
    resolves to IBRL_Gaussian and builds through ``instantiate`` (the checkpoint path is set aside: there is no such file), the actor
    is the plain fixed-std trunk with the cfg's dropout, the critic a plain LayerNorm trunk with double_q off, the C ABI counts the
    parameters, and the workspace queries accept B = 1 and the cfg's batch size in both precisions."""
    from dppo_amd.cfg.loader import get_class, instantiate, load_config
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_ibrl import IBRL_Gaussian
    cfgs = load_config(os.path.join(HERE, "golden", "shipped_ibrl_cfgs.json"))
    assert len(cfgs) == 8 and all(os.path.basename(k).startswith("ibrl_mlp") for k in cfgs)
    lib, seen = hip.load(), set()
    for name, cfg in cfgs.items():
        assert cfg._target_.endswith("train_ibrl_agent.TrainIBRLAgent"), name
        assert get_class(cfg.model._target_) is IBRL_Gaussian and get_class(cfg.model.critic._target_) is CriticObsAct, name
        assert get_class(cfg.model.actor._target_) is Gaussian_MLP and "plain_fixed_std" not in cfg.model.actor, name
        assert cfg.model.critic.use_layernorm is True and cfg.model.critic.double_q is False and cfg.env.n_envs == 1, name
        m = instantiate(cfg.model, network_path=None)
        a, dims, E = m.network, list(cfg.model.actor.mlp_dims), int(cfg.model.n_critics)
        p = float(cfg.model.actor.get("dropout", 0.0))
        assert a.plain_fixed_std and a.dropout == p and a.fixed_std == 0.1 and a.tanh_output is True and m.tanh_output is False, name
        assert m.soft_action_sample == bool(cfg.model.soft_action_sample) and m.soft_action_sample_beta == 10.0, name
        assert m.bc_policy is not a and m.target_actor is not a and not any(t.requires_grad for t in m.bc_policy.parameters())
        assert sum(isinstance(x, torch.nn.Dropout) for x in a.modules()) == (len(dims) if p else 0)
        da, dq = a.net_desc(), m.critic_networks[0].net_desc()
        od, af = cfg.obs_dim * cfg.cond_steps, cfg.action_dim * cfg.horizon_steps
        assert (da.kind, da.plain, da.use_layernorm, da.in_dim, da.hidden, da.n_blocks, da.out_dim) == (1, 1, 0, od, dims[0], len(dims) - 1, af)
        assert (dq.kind, dq.plain, dq.use_layernorm, dq.in_dim) == (1, 1, 1, od + af), name
        assert lib.dppo_net_param_count(C.byref(da)) == a.flat_params().numel()
        assert m.critic_flat_params().numel() == E * lib.dppo_net_param_count(C.byref(dq))
        seen.add((od, af, p, E))
        for prec in (hip.PREC_F32, hip.PREC_BF16):
            assert lib.dppo_ibrl_act_workspace_bytes(C.byref(da), C.byref(dq), prec, 1) > 0, lib.dppo_last_error()
            assert lib.dppo_ibrl_q_loss_workspace_bytes(C.byref(dq), prec, od, int(cfg.train.batch_size), E) > 0, lib.dppo_last_error()
            assert lib.dppo_gaussian_workspace_bytes(C.byref(da), None, prec, int(cfg.train.batch_size)) > 0
    assert (23, 7, 0.5, 5) in seen and (17, 6, 0.0, 5) in seen and (60, 9, 0.5, 5) in seen


def test_ibrl_state_dict_is_the_references(g31, tmp_path):
    """Keys and shapes are the fixture's (the reference's base_model.* aside: accepted and ignored on load); ``network_path`` loads
    into ``network`` before ``bc_policy`` and ``target_actor`` are copied from it."""
    from dppo_amd.model.rl.gaussian_ibrl import IBRL_Gaussian
    m = make_model("tiny", "fp32", "cpu")
    ref = {k: s for k, s in zip(g31["state_dict_keys"].tolist(), g31["state_dict_shapes"].tolist())}
    mine = {k: ",".join(str(s) for s in v.shape) for k, v in m.state_dict().items()}
    assert [k for k in ref if not k.startswith("base_model.")] == list(mine) and any(k.startswith("base_model.") for k in ref)
    assert all(ref[k] == mine[k] for k in mine)
    sd = dict(m.state_dict())
    sd.update({f"base_model.{k}": torch.empty(v.shape, device="meta") for k, v in K.member_params("tiny", 0).items()})
    m.load_state_dict(sd, strict=True)
    flat, P = m.critic_flat_params(), hip.load().dppo_net_param_count(C.byref(m.critic_networks[0].net_desc()))
    assert flat.numel() == 3 * P and torch.equal(flat[P:2 * P], torch.cat([v.reshape(-1) for v in K.member_params("tiny", 1).values()]))
    pair = m.get_random_indices()
    assert len(pair) == 2 and pair[0] != pair[1] and pair.device.type == "cpu" and int(pair.max()) < 3
    actor_sd = {f"network.{k}": v + 1.0 for k, v in K.actor_state_dict("tiny", "bc").items()}
    torch.save({"model": actor_sd}, tmp_path / "state.pt")
    m2 = IBRL_Gaussian(actor=make_actor("tiny"), critic=make_q("tiny"), n_critics=3, network_path=str(tmp_path / "state.pt"),
                       horizon_steps=1, device="cpu")
    for box in ("network", "bc_policy", "target_actor"):
        for k, v in getattr(m2, box).state_dict().items():
            assert torch.equal(v, actor_sd[f"network.{k}"]), (box, k)


def test_what_cannot_run_is_refused():
    from dppo_amd.model.common.gaussian import GaussianModel
    from dppo_amd.model.common.mlp import MLP
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_ibrl import IBRL_Gaussian
    from dppo_amd.model.rl.gaussian_ppo import PPO_Gaussian
    from tests.test_sac import make_q as twin_q
    with pytest.raises(NotImplementedError):  # the bare combination still raises (tests/test_sac.py asserts it too)
        Gaussian_MLP(3, 1, 11, mlp_dims=[64, 64], fixed_std=0.1, residual_style=False)
    with pytest.raises(NotImplementedError):
        MLP([14, 64, 64, 1], activation_type="ReLU", use_layernorm=True, dropout=0.1)
    with pytest.raises(NotImplementedError):
        MLP([14, 64, 64, 1], activation_type="ReLU", dropout=0.1, use_drop_final=True)
    for kw in (dict(use_layernorm=True), dict(learn_fixed_std=True), dict(residual_style=True), dict(fixed_std=None)):
        with pytest.raises(NotImplementedError):
            make_actor("tiny", **kw)
    kw = dict(horizon_steps=1, device="cpu")
    with pytest.raises(ValueError, match="double_q"):
        IBRL_Gaussian(actor=make_actor("tiny"), critic=twin_q("tiny"), n_critics=3, **kw)
    for E in (1, hip.RLPD_MAX_E + 1):
        with pytest.raises(ValueError, match="n_critics"):
            IBRL_Gaussian(actor=make_actor("tiny"), critic=make_q("tiny"), n_critics=E, **kw)
    with pytest.raises(ValueError, match="LayerNorm"):
        IBRL_Gaussian(actor=make_actor("tiny"), critic=make_q("tiny", use_layernorm=False), n_critics=3, **kw)
    residual = Gaussian_MLP(3, 1, 11, mlp_dims=[256, 256, 256], fixed_std=0.1, residual_style=True)
    with pytest.raises(ValueError, match="plain_fixed_std"):
        IBRL_Gaussian(actor=residual, critic=make_q("tiny"), n_critics=3, **kw)
    m = make_model("tiny", "fp32", "cpu")
    with pytest.raises(NotImplementedError, match="follow-up"):
        m.loss_actor({"state": torch.zeros(2, 1, 11)})
    with pytest.raises(NotImplementedError, match="not built"):
        GaussianModel.loss(m, torch.zeros(2, 1, 3), {"state": torch.zeros(2, 1, 11)}, 0.0)
    from dppo_amd.model.common.critic import CriticObs
    with pytest.raises(NotImplementedError, match="not built"):
        PPO_Gaussian(clip_ploss_coef=0.1, actor=make_actor("tiny"), critic=CriticObs(11, [256, 256, 256], residual_style=True),
                     horizon_steps=1, device="cpu")
    b, fb = K.inputs("tiny", 77), K.forward_inputs("tiny", 77)
    with pytest.raises(hip.DppoHipError):  # no CPU fallback
        m({"state": fb["obs"]})
    with pytest.raises(hip.DppoHipError):
        m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], K.GAMMA)
    with pytest.raises(hip.DppoHipError):
        m._sample(m.network, {"state": fb["obs"]}, False)


def test_ibrl_entries_reject_bad_arguments_on_the_host():
    """Every refusal leaves its reason in dppo_last_error(); nothing here touches a device (the pointers are never read)."""
    lib = hip.load()
    da, dq = make_actor("tiny").net_desc(), make_q("tiny").net_desc()
    err = lambda: lib.dppo_last_error()
    one = C.c_double(0)
    ptr = C.addressof(one)
    imgs = (C.c_void_p * 3)(ptr, ptr, ptr)
    cfg = make_actor("tiny").gaussian_cfg(randn_clip=3.0)
    drop = lambda p=0.5: hip.Dropout(p=p, seed_lo=1, seed_hi=2, pad=0, mask=None, mask_out=None)
    ln = hip.NetDesc.from_buffer_copy(da)
    ln.use_layernorm = 1
    residual = hip.NetDesc(kind=1, in_dim=11, hidden=256, n_blocks=1, out_dim=3, act=hip.ACT_RELU, time_dim=0, act_flat=0, cond_dim=11,
                           cond_hidden=0, cond_out=0, use_layernorm=0, plain=0)

    # dppo_gaussian_sample_drop
    def sample(desc=da, d=None, params=ptr, B=4, prec=hip.PREC_F32, wsb=1 << 40, null_drop=False):
        d = d if d is not None else drop()
        return lib.dppo_gaussian_sample_drop(C.byref(desc), prec, params, ptr, C.byref(cfg), None, ptr, None, B, ptr, None,
                                             None if null_drop else C.byref(d), ptr, wsb, None)
    for p in (1.0, -0.1, 1.5, float("nan")):
        assert sample(d=drop(p)) == -1 and b"outside [0, 1)" in err(), p
    assert sample(null_drop=True) == -1 and b"dropout struct" in err()
    assert sample(params=None) == -1 and b"null pointer" in err()
    assert sample(desc=ln) == -1 and b"LayerNorm" in err()
    assert sample(desc=residual) == -1 and b"plain" in err()
    assert sample(B=0) == -1 and b"B out of range" in err()
    assert sample(prec=7) == -1 and b"prec" in err()
    assert sample(wsb=64) == -1 and b"workspace too small" in err()

    # dppo_ibrl_act
    ws_act = lambda a=da, q=dq, B=4, prec=hip.PREC_F32: lib.dppo_ibrl_act_workspace_bytes(C.byref(a), C.byref(q), prec, B)
    assert ws_act() > 0
    assert ws_act(a=ln) == -1 and b"LayerNorm" in err()
    assert ws_act(a=residual) == -1 and b"plain" in err()
    assert ws_act(B=0) == -1 and b"B out of range" in err()
    assert ws_act(prec=7) == -1 and b"prec" in err()
    plain_q = hip.NetDesc.from_buffer_copy(dq)
    plain_q.use_layernorm = 0
    assert ws_act(q=plain_q) == -1 and b"LayerNorm" in err()
    wide_q = hip.NetDesc.from_buffer_copy(dq)
    wide_q.in_dim = wide_q.cond_dim = 15
    assert ws_act(q=wide_q) == -1 and b"pair with the actor" in err()

    def act(E=3, pair=(2, 0), a=da, q=dq, bc=ptr, images=imgs, d_bc=None, B=4, prec=hip.PREC_F32, wsb=1 << 40, beta=10.0, obs=ptr):
        return lib.dppo_ibrl_act(C.byref(a), C.byref(q), prec, E, bc, ptr, ptr, ptr, C.byref(cfg), C.byref(cfg),
                                 C.byref(d_bc) if d_bc is not None else None, None, ptr, images, pair[0], pair[1], obs, None, None, B, 1,
                                 beta, None, 1, 2, ptr, None, None, None, None, None, ptr, wsb, None)
    for pair in ((0, 0), (3, 0), (0, -1), (1, 7)):
        assert act(pair=pair) == -1 and b"pair" in err(), pair
    for E in (1, 0, 17):
        assert act(E=E) == -1 and b"members" in err(), E
    assert act(bc=None) == -1 and b"null pointer" in err()
    assert act(obs=None) == -1 and b"null pointer" in err()
    assert act(images=(C.c_void_p * 3)(None, ptr, ptr)) == -1 and b"member of the pair" in err()
    assert act(d_bc=drop(1.0)) == -1 and b"outside [0, 1)" in err()
    assert act(a=ln) == -1 and b"LayerNorm" in err()
    assert act(B=0) == -1 and b"B out of range" in err()
    assert act(prec=5) == -1 and b"prec" in err()
    assert act(beta=float("nan")) == -1 and b"beta" in err()
    assert act(wsb=64) == -1 and b"workspace too small" in err()

    # dppo_ibrl_q_loss_fwd_bwd
    ws_q = lambda desc=dq, E=3, N=77, od=11, prec=hip.PREC_F32: lib.dppo_ibrl_q_loss_workspace_bytes(C.byref(desc), prec, od, N, E)
    assert ws_q() > ws_q(N=38) > 0
    for E in (1, 0, 17):
        assert ws_q(E=E) == -1 and b"members" in err()
    assert ws_q(prec=7) == -1 and b"prec" in err()
    assert ws_q(N=0) == -1 and b"N out of range" in err()
    assert ws_q(od=14) == -1 and b"obs_dim" in err()
    assert ws_q(desc=plain_q) == -1 and b"LayerNorm" in err()
    batch = hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 0, 77)

    def loss(E=3, pair=(2, 0), q_params=ptr, images=imgs, timgs=imgs, nbc=ptr, nrl=ptr, N=77, gamma=0.99, prec=hip.PREC_F32, desc=dq,
             wsb=1 << 40):
        return lib.dppo_ibrl_q_loss_fwd_bwd(C.byref(desc), prec, E, q_params, images, ptr, timgs, pair[0], pair[1], C.byref(batch), 11,
                                            nbc, nrl, N, gamma, ptr, ptr, None, None, ptr, wsb, None)
    for pair in ((0, 0), (3, 0), (0, -1), (1, 7)):
        assert loss(pair=pair) == -1 and b"pair" in err(), pair
    assert loss(E=1) == -1 and b"members" in err()
    assert loss(q_params=None) == -1 and b"null pointer" in err()
    assert loss(nbc=None) == -1 and b"null pointer" in err()
    assert loss(nrl=None) == -1 and b"null pointer" in err()
    assert loss(images=(C.c_void_p * 3)(ptr, None, ptr)) == -1 and b"member 1" in err()
    assert loss(timgs=(C.c_void_p * 3)(None, ptr, ptr)) == -1 and b"target member" in err()
    assert loss(prec=5) == -1 and b"prec" in err()
    assert loss(N=0) == -1 and b"N out of range" in err()
    assert loss(gamma=1.5) == -1 and b"gamma" in err()
    assert loss(desc=plain_q) == -1 and b"LayerNorm" in err()
    assert loss(wsb=64) == -1 and b"workspace too small" in err()
    assert lib.dppo_version() == 1


# ------------------------------------------------------------------------------------------------------------------ GPU
def run_forward(m, case, n, deterministic=False):
    fb = dev_inputs(K.forward_inputs(case, n))
    drop = K.dropout(case) > 0
    a = m({"state": fb["obs"]}, deterministic=deterministic, pair=K.pair_of(case), noise_bc=fb["noise_bc"], noise_rl=fb["noise_rl"],
          mask_bc=fb["mask_bc"] if drop else None, mask_rl=fb["mask_rl"] if drop else None, u=fb["u"])
    return dict(action=a.reshape(n, -1).clone(), q_bc=m.last_q_bc.clone(), q_rl=m.last_q_rl.clone(), took=m.last_took_bc.clone(),
                a_bc=m.last_a_bc.clone(), a_rl=m.last_a_rl.clone())


def own_rule(res, soft, u):
    """The select rule applied to the call's own Q values, in fp32 on the device's numbers."""
    qb, qr = res["q_bc"].cpu(), res["q_rl"].cpu()
    took = qb > qr
    if soft:
        d = torch.exp(qr * np.float32(K.BETA)) - torch.exp(qb * np.float32(K.BETA))
        p_bc = 1 / (1 + torch.exp(d))
        sure = (u - p_bc).abs() > 1e-5  # (a draw this close to the call's own p_bc may fall on either side of the device's exp)
        return torch.where(torch.isnan(d), took, u < p_bc), sure | torch.isnan(d)
    return took, torch.ones_like(took)


def run_critic(m, case, n, replay=None, inds=None):
    b = dev_inputs(K.inputs(case, n))
    drop = K.dropout(case) > 0
    kw = dict(pair=K.pair_of(case), noise_bc=b["noise_bc"], noise_rl=b["noise_rl"], mask_bc=b["mask_bc"] if drop else None,
              mask_rl=b["mask_rl"] if drop else None)
    if replay is not None:
        loss = m.loss_critic(replay, None, None, None, None, K.GAMMA, inds=inds, **kw)
    else:
        loss = m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], K.GAMMA, **kw)
    return dict(loss=loss.detach(), stats=m.last_stats.cpu().numpy().copy(), grads=m.critic_flat_grads().clone(), y=m.last_y.clone(),
                share=float(m.last_bc_share))


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_ibrl_actor_mean_and_sample_fp32(case, n):
    """The three actors' mean and sample under the given masks within 2e-5 of float64; ``eval()`` ignores the mask's dropout."""
    m, b = make_model(case, "fp32", DEV), K.forward_inputs(case, n)
    db, drop = dev_inputs(b), K.dropout(case) > 0
    for which, net, std, det in (("bc", m.bc_policy, K.BC_STD, True), ("rl", m.network, K.FIXED_STD, False)):
        mask = b[f"mask_{which}"]
        want, mean = K.sample(K.cast(K.actor_params(case, which), D64), case, b["obs"].double(), mask, b[f"noise_{which}"], std)
        a, mu = m._sample(net, {"state": db["obs"]}, det, db[f"noise_{which}"], want_mean=True,
                          drop_mask=db[f"mask_{which}"] if drop else None)
        ea, em = (a.reshape(n, -1).double().cpu() - want).abs().max().item(), (mu.double().cpu() - mean).abs().max().item()
        print(f"{case}_{n} {which}: sample off by {ea:.2e}, mean by {em:.2e}")
        assert ea <= SAMPLE_TOL and em <= SAMPLE_TOL
    if drop:
        m.network.eval()
        _, mu = m._sample(m.network, {"state": db["obs"]}, False, db["noise_rl"], want_mean=True)
        _, mean = K.sample(K.cast(K.actor_params(case, "rl"), D64), case, b["obs"].double(), None, b["noise_rl"], K.FIXED_STD)
        assert (mu.double().cpu() - mean).abs().max().item() <= SAMPLE_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("soft", [False, True], ids=["greedy", "soft"])
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_ibrl_forward_fp32(g31, case, n, soft):
    m, ref = make_model(case, "fp32", DEV, soft), restated_forward(case, n, soft)
    res = run_forward(m, case, n)
    stats_close(res["q_bc"].cpu().numpy(), ref["q_bc"].numpy(), f"{case}_{n} q_bc")
    stats_close(res["q_rl"].cpu().numpy(), ref["q_rl"].numpy(), f"{case}_{n} q_rl")
    assert (res["a_bc"].double().cpu() - ref["a_bc"]).abs().max() <= SAMPLE_TOL and (res["a_rl"].double().cpu() - ref["a_rl"]).abs().max() <= SAMPLE_TOL
    took = res["took"].cpu()
    fix = g31[f"{case}_{n}_{'soft' if soft else 'greedy'}_took_bc"]
    assert np.array_equal(took.numpy().astype(np.uint8)[fix != 2], fix[fix != 2])
    assert torch.equal(took, ref["took_bc"])  # (the overflow row included: the greedy rule decides it)
    mine, sure = own_rule(res, soft, K.forward_inputs(case, n)["u"])
    assert torch.equal(took[sure], mine[sure]) and sure.float().mean() > 0.95
    assert torch.equal(res["action"], torch.where(res["took"][:, None], res["a_bc"], res["a_rl"]))
    tie, ovf = K.special_rows(n)
    if tie is not None:
        assert torch.equal(res["a_bc"][tie], res["a_rl"][tie]) and res["q_bc"][tie] == res["q_rl"][tie] and (soft or not took[tie])
        if soft:
            w = torch.exp(res["q_bc"][ovf] * np.float32(K.BETA)), torch.exp(res["q_rl"][ovf] * np.float32(K.BETA))
            assert torch.isinf(w[0]) and torch.isinf(w[1]) and bool(took[ovf]) == bool(res["q_bc"][ovf] > res["q_rl"][ovf])
    again = run_forward(m, case, n)
    assert all(torch.equal(res[k], again[k]) for k in res)
    if soft:  # deterministic: greedy whatever the model's setting, and the RL proposal at sigma 1e-4
        det, dref = run_forward(m, case, n, deterministic=True), K.forward(case, K.forward_inputs(case, n), K.pair_of(case), True, True, dtype=D64)
        stats_close(det["q_rl"].cpu().numpy(), dref["q_rl"].numpy(), f"{case}_{n} deterministic q_rl")
        assert torch.equal(det["took"].cpu(), det["q_bc"].cpu() > det["q_rl"].cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_ibrl_loss_critic_fp32(case, n):
    """Statistics, y and every member's every gradient against float64; the returned loss is the statistic; two calls are bit-equal;
    a gathered call (indices into a ring with head != 0) equals the contiguous one bit for bit; ``.backward()`` hands out the slices."""
    m, ref = make_model(case, "fp32", DEV), restated_critic(case, n)
    res = run_critic(m, case, n)
    stats_close(res["stats"], ref["stats"], f"{case}_{n} critic")
    stats_close(res["y"].cpu().numpy(), ref["y"].numpy(), f"{case}_{n} y")
    assert float(res["loss"]) == np.float32(res["stats"][0])
    assert res["share"] == ref["bc_share"] and m.last_pair == K.pair_of(case)
    got = named_grads(m)
    check_with_gates(case, n, got, f"{case}_{n}")
    again = run_critic(m, case, n)
    assert torch.equal(res["grads"], again["grads"]) and np.array_equal(res["stats"], again["stats"]) and torch.equal(res["y"], again["y"])
    if case != "can":
        rp, inds = ring_of(dev_inputs(K.inputs(case, n)), n)
        ring = run_critic(m, case, n, replay=rp, inds=inds)
        assert torch.equal(res["grads"], ring["grads"]) and np.array_equal(res["stats"], ring["stats"]) and torch.equal(res["y"], ring["y"])
        loss = m.loss_critic(rp, None, None, None, None, K.GAMMA, inds=inds, pair=K.pair_of(case), next_actions_bc=ref["a_bc"].float().to(DEV),
                             next_actions_rl=ref["a_rl"].float().to(DEV))
        loss.backward()
        E = K.n_critics(case)
        w = m.critic_networks[E - 1].Q1.moduleList[0].norm_1.weight
        assert w.grad is not None and torch.equal(w.grad, dict(named_grads(m))[f"{E - 1}.Q1.moduleList.0.norm_1.weight"])


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_ibrl_loss_critic_bf16_within_twice_the_rounding_yardstick(case, n):
    """e_c <= 2 e_y on the loss, on 1 - cosine and per tensor, the statistics with the floor n 2^-24, as tests/test_calql.py.

    Measured on MI355X, worst tensor against the yardstick: tiny_1 1.98e-3 / 1.49e-3 (1.33 x), tiny_77 3.367e-2 / 3.365e-2, chunk_130
    3.55e-3 / 3.12e-3, nodrop_64 1.29e-3 / 1.23e-3, can_256 1.22e-2 / 1.20e-2.  tiny_1 is the case that shows why the members'
    backward hands LayerNorm's backward its input in fp32 here (csrc/ibrl.h): with that row rounded to bf16 first, as RLPD's call
    does, member 0's second hidden bias came out at 3.165e-3, 2.13 x the yardstick -- a figure that the three roundings of that path
    (the loss gradient, the row in front of LayerNorm's backward, the row behind it) reproduce on the CPU to four digits, and that
    drops to 1.982e-3 without the middle one, which is what the call now measures."""
    m = make_model(case, "bf16", DEV)
    res = run_critic(m, case, n)
    fp32, yard = restate_critic(case, n, torch.float32), restate_critic(case, n, torch.float32, bf16=True)
    z = torch.zeros(1)
    for r in (fp32, yard):
        r["d_a"] = z
    call = dict(loss=res["stats"][0], d_a=z, named=named_grads(m))
    e_y, e_c = rel_errors(fp32, yard), rel_errors(fp32, call)
    worst = max(e_c["per"], key=lambda k: e_c["per"][k] / (e_y["per"][k] + 1e-30))
    s_err = lambda s: np.abs(np.asarray(s, dtype=np.float64) - np.asarray(fp32["stats"])) / np.maximum(1.0, np.abs(fp32["stats"]))
    s_y, s_c = s_err(yard["stats"]), s_err(res["stats"])
    print(f"{case}_{n} bf16: yardstick loss {e_y['loss']:.3e} 1-cos {e_y['one_minus_cos']:.3e}; call loss {e_c['loss']:.3e} 1-cos "
          f"{e_c['one_minus_cos']:.3e}; worst tensor {worst}: {e_c['per'][worst]:.3e} against {e_y['per'][worst]:.3e}; "
          f"stats yardstick {s_y} call {s_c}; bc share call {res['share']:.4f} yardstick {yard['bc_share']:.4f} fp32 {fp32['bc_share']:.4f}")
    assert e_c["loss"] <= 2 * e_y["loss"] and e_c["one_minus_cos"] <= 2 * e_y["one_minus_cos"]
    assert (s_c <= 2 * s_y + n * 2.0 ** -24).all(), (s_c, s_y)
    for k in e_c["per"]:
        assert e_c["per"][k] <= 2 * e_y["per"][k], (k, e_c["per"][k], e_y["per"][k])


@pytest.mark.gpu
@pytest.mark.parametrize("soft", [False, True], ids=["greedy", "soft"])
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_ibrl_forward_bf16_within_twice_the_rounding_yardstick(case, n, soft):
    """Both Q vectors, relative l2 against the fp32 restatement, within twice the bf16-Linear yardstick's; took_bc by the rule on the
    call's own Q values; the action is the chosen proposal bit for bit."""
    m = make_model(case, "bf16", DEV, soft)
    res = run_forward(m, case, n)
    fp32, yard = restated_forward(case, n, soft, torch.float32), restated_forward(case, n, soft, torch.float32, True)
    err = lambda r, x: float(np.linalg.norm(x - r) / (np.linalg.norm(r) + 1e-30))
    for k in ("q_bc", "q_rl"):
        r = fp32[k].double().numpy()
        e_y, e_c = err(r, yard[k].double().numpy()), err(r, res[k].double().cpu().numpy())
        print(f"{case}_{n} bf16 {k}: yardstick {e_y:.3e} call {e_c:.3e}")
        assert e_c <= 2 * e_y + n * 2.0 ** -24
    mine, sure = own_rule(res, soft, K.forward_inputs(case, n)["u"])
    assert torch.equal(res["took"].cpu()[sure], mine[sure])
    assert torch.equal(res["action"], torch.where(res["took"][:, None], res["a_bc"], res["a_rl"]))


@pytest.mark.gpu
def test_hip_ibrl_targets_move_as_whole_images():
    case = "tiny"
    m = make_model(case, "fp32", DEV)
    t0, s0 = m.target_flat_params().clone(), m.critic_flat_params().clone()
    m.update_target_critic(0.01)
    assert torch.equal(m.target_flat_params(), t0 * np.float32(1 - 0.01) + s0 * np.float32(0.01))
    a0, n0 = m.target_actor.flat_params().clone(), m.network.flat_params().clone()
    before = m.target_actor.packed(m.prec, 0).clone()
    m.update_target_actor(0.01)
    want = a0 * np.float32(1 - 0.01) + n0 * np.float32(0.01)
    assert torch.equal(m.target_actor.flat_params(), want) and not torch.equal(a0, want)
    assert torch.equal(torch.cat([p.reshape(-1) for p in m.target_actor.mlp_mean.parameters()]), want)
    assert not torch.equal(m.target_actor.packed(m.prec, 0), before)  # the kernel image is rebuilt
    assert torch.equal(m.bc_policy.flat_params(), torch.cat([v.reshape(-1) for v in K.actor_params(case, "bc").values()]).to(DEV))


@pytest.mark.gpu
def test_hip_ibrl_sequence_equals_the_restated_sequence():
    """Critic loss, AdamW on ``critic_flat_params()``, Polyak of both targets, then ``forward``: against the same sequence on the
    float64 restatement, the Q values by stats_close and the choice equal wherever the restated gap keeps its guard band."""
    case, n, lr, tau = "tiny", 77, 1e-3, 0.01
    m = make_model(case, "fp32", DEV)
    opt = torch.optim.AdamW([m.critic_flat_params()], lr=lr, weight_decay=0)
    res = run_critic(m, case, n)
    m.critic_flat_params().grad = m.critic_flat_grads()
    opt.step()
    m.critics_updated()
    m.update_target_critic(tau)
    m.update_target_actor(tau)
    fwd = run_forward(m, case, n)
    E = K.n_critics(case)
    members = [K.leaf(K.member_params(case, e), D64) for e in range(E)]
    targets = [K.member_params(case, e, K.TARGET_EPS) for e in range(E)]
    ropt = torch.optim.AdamW([t for p in members for t in p.values()], lr=lr, weight_decay=0)
    r = K.loss_critic(members, targets, case, K.inputs(case, n), K.pair_of(case), dtype=D64)
    for p, gs in zip(members, r["grads"]):
        for t, g in zip(p.values(), gs):
            t.grad = g
    ropt.step()
    stepped = [{k: v.detach() for k, v in p.items()} for p in members]
    ref = K.forward(case, K.forward_inputs(case, n), K.pair_of(case), False, dtype=D64, members=stepped)
    stats_close(res["stats"], r["stats"], "sequence critic")
    stats_close(fwd["q_bc"].cpu().numpy(), ref["q_bc"].numpy(), "sequence q_bc")
    stats_close(fwd["q_rl"].cpu().numpy(), ref["q_rl"].numpy(), "sequence q_rl")
    banded = (ref["q_bc"] - ref["q_rl"]).abs() >= 10 * K.Q_CEIL
    assert torch.equal(fwd["took"].cpu()[banded], ref["took_bc"][banded]) and banded.float().mean() > 0.9
    want_t = torch.cat([torch.cat([(t * (1 - tau) + s[k] * tau).reshape(-1) for k, t in K.cast(targets[e], D64).items()]) for e, s in enumerate(stepped)])
    assert (m.target_flat_params().double().cpu() - want_t).abs().max() <= 1e-6 + 2 * lr * tau
