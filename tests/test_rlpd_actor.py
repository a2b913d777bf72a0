"""RLPD's actor loss through the mean of the ensemble's Q (reference model/rl/gaussian_rlpd.py:100-112) and ``TrainRLPDAgent``
(reference agent/finetune/train_rlpd_agent.py).

CPU: the fp32 restatement of tests/golden/make_golden_rlpd_actor_cases.py reproduces the g28 fixture the reference wrote
(``loss_actor``, ``loss_critic``, one update sequence); the inputs keep their guard bands on the float64 restatement; the analytic
route the kernels take (g = the members' mean dq_e/da through ``S.head_backward``) is autograd's in float64; both new C ABI entries
check their arguments; every shipped cfg resolves to the agent.

GPU, fp32: ``dppo_rlpd_actor_fwd_bwd`` on all ten cases and on ``wide`` (E = 16, hidden 1024: the top of the accepted range) is held
to the restatement in FLOAT64 fed the same fp32 values: statistics by stats_close, d_a and every actor gradient by grad_violations'
rule on every entry, ReLU gates within RELU_TIE handed over as tests/test_sac.py::check_on_own_sel does (ReLU cases only; it prints
how many it tried).  bf16: no tolerance is fixed; the yardstick is the restatement with every Linear's operands rounded to bf16 and
LayerNorm left in fp32, and the call may be off from the fp32 restatement by at most twice the yardstick's own error.
"""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from dppo_amd import hip
from dppo_amd.cfg.loader import Cfg, get_class, load_config
from tests.golden import make_golden_rlpd_actor_cases as A
from tests.golden import make_golden_rlpd_cases as K
from tests.golden import make_golden_sac_cases as S
from tests.test_dql import check_stepped, grad_violations, rel_errors, stats_close
from tests.test_idql import check_grads_fp32
from tests.test_qsm import close_to_fixture, ring_of
from tests.test_sac import by_name, check_stepped_twice, named, rel_close

DEV = "cuda:0"
D64 = torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))
SHIPPED = os.path.join(HERE, "golden", "shipped_rlpd_cfgs.json")
CHEETAH_CFG = "gym/scratch/halfcheetah-v2/rlpd_mlp.yaml"
IDS = [f"{c}_{n}" for c, n in A.CASES]
ALL_IDS = [f"{c}_{n}" for c, n in A.ALL_CASES]


def actor_dims(case):
    return list(A.WIDE_ACTOR_DIMS) if case == "wide" else S.dims(A.sac_case(case))


def make_q(case, prec="fp32"):
    from dppo_amd.model.common.critic import CriticObsAct
    od, ta, da, dims, act, _ = A.net_of(case)
    return CriticObsAct(cond_dim=od, mlp_dims=list(dims), action_dim=da, action_steps=ta, activation_type=act, use_layernorm=True,
                        double_q=False, precision=prec)


def make_model(case, prec, device, backup=True):
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_rlpd import RLPD_Gaussian
    od, ta, da, dims, act, E = A.net_of(case)
    actor = Gaussian_MLP(da, ta, od, mlp_dims=actor_dims(case), activation_type=act, tanh_output=False, fixed_std=None,
                         std_min=S.STD_MIN, std_max=S.STD_MAX, precision=prec)
    actor.load_state_dict(A.actor_params(case), strict=True)
    m = RLPD_Gaussian(actor=actor, critic=make_q(case, prec), n_critics=E, backup_entropy=backup, horizon_steps=ta, device=device,
                      randn_clip_value=A.RANDN_CLIP, tanh_output=True)
    for e in range(E):
        m.critic_networks[e].load_state_dict(A.member_params(case, e), strict=True)
        if case != "wide":
            m.target_networks[e].load_state_dict(K.member_params(case, e, K.TARGET_EPS), strict=True)
    return m


def restate(case, n, dtype=D64, bf16=False, gates=None):
    with gates if gates is not None else K.relu_gates() as rg:
        if bf16:
            with K.bf16_linears():
                res = A.restate(case, n, dtype)
        else:
            res = A.restate(case, n, dtype)
    res["near_zero"], res["calls"] = rg.near_zero(), len(rg.calls)
    return res


@functools.lru_cache(maxsize=None)
def restated(case, n, dtype=D64):
    """The restatement of one case: computed once, shared, never modified."""
    return restate(case, n, dtype)


def member_rows(flat, E):
    """(member index as text, its row of a flat [E][P] image): the fixture's names."""
    return [(str(e), row) for e, row in enumerate(flat.detach().reshape(E, -1))]


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case,n", A.CASES, ids=IDS)
def test_restatement_reproduces_the_reference_fixture(golden, case, n):
    """The fp32 restatement against g28: the losses and d_a by close_to_fixture's rule, gradients by check_grads_fp32's; a member's
    gradients are one flat vector in the fixture (its row of the [E][P] image)."""
    g, name, r = golden("g28_rlpd"), f"{case}_{n}", restated(case, n, torch.float32)
    close_to_fixture(g, f"{name}_a_loss", r["loss"], name)
    close_to_fixture(g, f"{name}_d_a", r["d_a"], name)
    check_grads_fp32(g, f"{name}_ga", r["named"])
    E = K.n_critics(case)
    members = [K.leaf(K.member_params(case, e)) for e in range(E)]
    targets = [K.member_params(case, e, K.TARGET_EPS) for e in range(E)]
    rc = K.loss_critic(members, targets, case, K.inputs(case, n), K.pair_of(case, n), K.backup_entropy(case, n))
    close_to_fixture(g, f"{name}_c_loss", rc["loss"], name)
    check_grads_fp32(g, f"{name}_gq", [(str(e), torch.cat([t.reshape(-1) for t in gs])) for e, gs in enumerate(rc["grads"])])


def test_restatement_reproduces_the_recorded_sequence(golden):
    """Two critic AdamW steps with Polyak, one actor step, one temperature step on cheetah, N = 77.  A member took two steps
    (check_stepped_twice); its target is (1 - tau)^2 t0 + tau (1 - tau) q1 + tau q2, so it is off by at most tau times the sum of the
    one-step and the two-step bound, which 2 tau times the two-step bound covers."""
    g, seq = golden("g28_rlpd"), A.restate_sequence()
    first = f"{A.SEQ_CASE}_{A.SEQ_N}"
    assert float(g["seq_c_loss"][0]) == float(g[f"{first}_c_loss"]) and float(g["seq_c_loss"][1]) != float(g["seq_c_loss"][0])
    rel_close(seq["c_loss"], g["seq_c_loss"], 1e-5, "seq critic")
    rel_close([seq["a_loss"], seq["t_loss"]], [g["seq_a_loss"], g["seq_t_loss"]], 1e-5, "seq actor, temperature")
    rel_close([seq["log_alpha"]], [g["seq_log_alpha"]], 1e-6, "seq log_alpha")
    assert float(g["seq_a_loss"]) != float(g[f"{first}_a_loss"])  # the stepped members moved the actor's loss
    flat = lambda ps: [(str(e), torch.cat([t.reshape(-1) for t in p.values()])) for e, p in enumerate(ps)]
    check_grads_fp32(g, f"{first}_gq", flat(seq["gq"][0]))
    check_grads_fp32(g, "seq_gq1", flat(seq["gq"][1]))
    check_grads_fp32(g, "seq_ga", list(seq["ga"].items()))
    check_stepped_twice(g, "seq_q", flat(seq["q"]), (f"{first}_gq", "seq_gq1"), A.SEQ_LR)
    check_stepped_twice(g, "seq_target", flat(seq["target"]), (f"{first}_gq", "seq_gq1"), 2 * A.SEQ_LR * A.SEQ_TAU)
    check_stepped(g, "seq_actor", [(k, seq["actor"][k]) for k in S.grad_names(seq["actor"])], "seq_ga", A.SEQ_ACTOR_LR)


def test_state_dict_keys_are_the_references(golden):
    """g28's keys of the reference's RLPD_Gaussian on ``tiny``: ours, plus the reference's stateless ``base_model.*``."""
    from tests.test_rlpd import make_model as tiny_model
    want = [str(k) for k in golden("g28_rlpd")["state_dict_keys"]]
    assert [k for k in want if not k.startswith("base_model.")] == list(tiny_model("tiny", "fp32", "cpu").state_dict())
    assert any(k.startswith("base_model.") for k in want)


@pytest.mark.parametrize("case,n", A.ALL_CASES, ids=ALL_IDS)
def test_inputs_keep_their_guard_bands(case, n):
    """On the float64 restatement: |u| <= U_MAX, every draw inside NOISE_CAP, and at the SAMPLED actions every row's pre-LayerNorm
    variance exceeds VAR_FLOOR -- but in tiny_flat's flattened layer, where it is exactly 0."""
    r, b = restated(case, n), A.inputs(case, n)
    assert r["u"].abs().max() <= S.U_MAX, r["u"].abs().max()
    assert b["noise"].abs().max() <= S.NOISE_CAP
    for e in range(A.n_critics(case)):
        var = A.pre_ln_variances(K.cast(A.member_params(case, e), D64), case, b["obs"].double(), r["a"])
        for i, v in enumerate(var):
            if case == "tiny_flat" and e == K.FLAT_MEMBER and i == 0:
                assert (v == 0).all()
            else:
                assert v.min().item() > K.VAR_FLOOR, (e, i, v.min().item())
    assert torch.isfinite(r["q"]).all() and r["d_a"].abs().amax(dim=1).min() > 0


def test_relu_gates_near_zero_are_few():
    """What the gate-flipping fallback of the GPU test may touch: over the ten cases of K.CASES one ReLU pre-activation of the
    float64 restatement lies below RELU_TIE (cheetah, N = 256); ``wide`` is counted on its own."""
    counts = {f"{c}_{n}": len(restated(c, n)["near_zero"]) for c, n in A.ALL_CASES}
    print(f"ReLU gates below {K.RELU_TIE:g}: {counts}")
    assert sum(v for k, v in counts.items() if not k.startswith("wide")) <= 1, counts
    assert all(restated(c, n)["calls"] > 0 for c, n in A.ALL_CASES if A.net_of(c)[4] == "ReLU")


@pytest.mark.parametrize("case,n", [("cheetah", 77), ("chunk", 77), ("tiny_flat", 77), A.WIDE])
def test_analytic_route_is_autograds(case, n):
    """g = the members' mean dq_e/da through the head's backward as the kernels implement it (sac.h) against autograd on the
    float64 restatement; d_a = -g / N."""
    b, p = A.inputs(case, n), S.leaf(A.actor_params(case), D64)
    members = [K.cast(A.member_params(case, e), D64) for e in range(A.n_critics(case))]
    s = S.sample(p, A.sac_case(case), b["obs"].double(), b["noise"])
    qs = torch.stack([A.q_forward(m, case, b["obs"].double(), s["a"]) for m in members])
    loss = (-qs.mean(dim=0) + A.ALPHA * s["logp"]).mean()
    g = torch.stack([torch.autograd.grad(q.sum(), s["a"], retain_graph=True)[0] for q in qs]).mean(dim=0)
    dmean, draw = torch.autograd.grad(loss, [s["mean"], s["raw"]])
    zc = b["noise"].double().reshape(n, -1).clamp(-A.RANDN_CLIP, A.RANDN_CLIP)
    du, dr = S.head_backward({k: v.detach() for k, v in s.items()}, g, zc, A.ALPHA, n, p["logvar_min"].detach(), p["logvar_max"].detach())
    for got, want in ((du, dmean), (dr, draw)):
        assert (got - want).abs().max() <= 1e-9 * want.abs().max() + 1e-15, ((got - want).abs().max(), want.abs().max())
    ref = restated(case, n)
    assert (ref["d_a"] + g / n).abs().max() <= 1e-12 * g.abs().max()
    if case == "tiny_flat":
        assert (ref["g_members"][K.FLAT_MEMBER] == 0).all() and (ref["g_members"][0] != 0).any()


def descs(case):
    m = make_model(case, "fp32", "cpu")
    return m.network.net_desc(), m.critic_networks[0].net_desc()


def test_rlpd_actor_entries_reject_bad_arguments_on_the_host():
    """Every refusal of both new entries leaves its reason in dppo_last_error(); nothing here touches a device."""
    lib = hip.load()
    err = lambda: lib.dppo_last_error()
    da, dq = descs("tiny")
    f32 = hip.PREC_F32

    def ws(a=da, q=dq, prec=f32, od=11, N=77, E=3):
        return lib.dppo_rlpd_actor_workspace_bytes(C.byref(a) if a is not None else None, C.byref(q) if q is not None else None, prec,
                                                   od, N, E)
    need = ws()
    assert need > 0
    assert ws(a=None) == -1 and b"null" in err()
    assert ws(q=None) == -1 and b"null" in err()
    for E in (1, 0, 17):
        assert ws(E=E) == -1 and b"members" in err(), E
    assert ws(prec=7) == -1 and b"prec" in err()
    assert ws(N=0) == -1 and b"N out of range" in err()
    plain = hip.NetDesc.from_buffer_copy(dq)
    plain.use_layernorm = 0
    assert ws(q=plain) == -1 and b"LayerNorm" in err()
    twin = hip.NetDesc.from_buffer_copy(dq)
    twin.out_dim = 2
    assert ws(q=twin) == -1 and b"out_dim 1" in err()
    wide = hip.NetDesc.from_buffer_copy(dq)
    wide.hidden = 2048
    assert ws(q=wide) == -1 and b"hidden" in err()
    other_q = descs("chunk")[1]
    assert ws(q=other_q, od=22) == -1 and b"do not pair" in err()  # tiny's actor against chunk's members
    assert ws(od=12) == -1 and b"do not pair" in err()
    odd = hip.NetDesc.from_buffer_copy(da)
    odd.out_dim = 7
    assert ws(a=odd) == -1 and b"SAC actor" in err()
    one = C.c_double(0)  # stands in for every pointer: refusals come before anything is read
    ptr = C.addressof(one)
    imgs = (C.c_void_p * 3)(ptr, ptr, ptr)
    cfg = make_model("tiny", "fp32", "cpu")._cfg(False, torch.zeros(1))

    def call(a=da, q=dq, E=3, actor_params=ptr, images=imgs, cfg=cfg, batch=hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 0, 77),
             N=77, alpha=ptr, grad=ptr, stats=ptr, wsp=ptr, wsb=1 << 40, prec=f32, od=11):
        return lib.dppo_rlpd_actor_fwd_bwd(C.byref(a), C.byref(q), prec, E, actor_params, ptr, ptr, images, C.byref(cfg),
                                           C.byref(batch) if batch is not None else None, od, N, None, alpha, grad, stats, None, None,
                                           None, wsp, wsb, None)
    for kw in (dict(actor_params=None), dict(alpha=None), dict(grad=None), dict(stats=None), dict(wsp=None), dict(images=None)):
        assert call(**kw) == -1 and b"null pointer" in err(), kw
    assert call(images=(C.c_void_p * 3)(ptr, None, ptr)) == -1 and b"member 1" in err()
    assert call(batch=None) == -1 and b"null batch" in err()
    for E in (1, 17):
        assert call(E=E) == -1 and b"members" in err()
    assert call(q=plain) == -1 and b"LayerNorm" in err()
    assert call(q=twin) == -1 and b"out_dim 1" in err()
    assert call(od=12) == -1 and b"do not pair" in err()
    assert call(prec=5) == -1 and b"prec" in err()
    assert call(N=0) == -1 and b"N out of range" in err()
    det = type(cfg).from_buffer_copy(cfg)
    det.deterministic = 1
    assert call(cfg=det) == -1 and b"deterministic" in err()
    for bad in (hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 77, 77), hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 0, 78),
                hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 0, 1, 0, 0), hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 0, 0, 77)):
        assert call(batch=bad) == -1 and b"ring geometry" in err()
    assert call(batch=hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 0, 76)) == -1 and b"exceeds" in err()
    assert call(batch=hip.IdqlBatch(None, ptr, ptr, ptr, ptr, None, 77, 1, 0, 77)) == -1 and b"null pointer in batch" in err()
    assert call(wsb=need - 1) == -1 and b"workspace too small" in err()


def test_workspace_query_accepts_every_shipped_cfg_and_the_widest_shape():
    from dppo_amd.cfg.loader import instantiate
    lib, seen = hip.load(), 0
    for name, cfg in load_config(SHIPPED).items():
        assert get_class(cfg._target_).__name__ == "TrainRLPDAgent", name
        if "action_dim" not in cfg.model.actor:  # robomimic/finetune/lift, as shipped: it cannot be built in the reference either
            continue
        m = instantiate(cfg.model)
        da, dq = m.network.net_desc(), m.critic_networks[0].net_desc()
        od = cfg.obs_dim * cfg.cond_steps
        for prec in (hip.PREC_F32, hip.PREC_BF16):
            assert lib.dppo_rlpd_actor_workspace_bytes(C.byref(da), C.byref(dq), prec, od, int(cfg.train.batch_size),
                                                       int(cfg.model.n_critics)) > 0, (name, lib.dppo_last_error())
        seen += 1
    assert seen == 8
    da, dq = descs("wide")
    assert dq.hidden == 1024 and A.n_critics("wide") == 16
    for prec in (hip.PREC_F32, hip.PREC_BF16):
        for N in (3, 256):
            assert lib.dppo_rlpd_actor_workspace_bytes(C.byref(da), C.byref(dq), prec, 11, N, 16) > 0, lib.dppo_last_error()


def test_every_shipped_cfg_targets_the_agent():
    from dppo_amd.agent.finetune.train_off_policy_agent import OffPolicyAgent
    from dppo_amd.agent.finetune.train_rlpd_agent import TrainRLPDAgent
    cfgs = load_config(SHIPPED)
    assert len(cfgs) == 9 and all(get_class(c._target_) is TrainRLPDAgent for c in cfgs.values())
    assert issubclass(TrainRLPDAgent, OffPolicyAgent)


# ------------------------------------------------------------------------------------------------------------------ GPU
def dev_inputs(case, n):
    return {k: v.to(DEV) for k, v in A.inputs(case, n).items()}


def alpha_dev(x=A.ALPHA):
    return torch.full((1,), float(x), dtype=torch.float64, device=DEV)


def run_actor(m, b, replay=None, inds=None):
    src = replay if replay is not None else {"state": b["obs"]}
    loss = m.loss_actor(src, alpha_dev(), inds=inds, noise=b["noise"])
    return dict(loss=loss.detach().clone(), stats=m.last_stats.clone(), ga=m.last_loss_grad.clone(), d_a=m.last_d_a.clone(),
                logp=m.last_logp.clone(), a=m.last_actions.clone())


def check_with_gates(case, n, got_named, d_a, what):
    """d_a and every gradient of a run against the float64 restatement by grad_violations' rule on EVERY entry.  Where that misses
    and the networks are ReLU ones, the yardstick's gates below RELU_TIE are tried on their other side, nearest to zero first, each
    kept if it lowers the count of entries outside the rule (tests/test_sac.py::check_on_own_sel).  Returns the gates tried."""
    ref = restated(case, n)
    order = [k for k, _ in ref["named"]]
    got = [("d_a", d_a)] + by_name(got_named, order)
    bad = grad_violations([("d_a", ref["d_a"])] + ref["named"], got)
    if not bad or A.net_of(case)[4] != "ReLU":
        assert not bad, (what, bad)
        return 0
    count = lambda b: sum(x[1] + int(x[3]) for x in b)
    print(f"{what}: {count(bad)} entries outside the rule {bad}; {len(ref['near_zero'])} ReLU gates below {K.RELU_TIE:g}")
    force, tried = {}, 0
    for z, where, gate in ref["near_zero"]:
        trial = dict(force)
        trial[where] = not gate
        tried += 1
        res = restate(case, n, gates=K.relu_gates(trial))
        now = grad_violations([("d_a", res["d_a"])] + res["named"], got)
        if count(now) < count(bad):
            force, bad = trial, now
        if not bad:
            break
    print(f"{what}: tried {tried} gates, kept {force}")
    assert not bad, (what, bad, force)
    return tried


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", A.ALL_CASES, ids=ALL_IDS)
def test_hip_rlpd_loss_actor_fp32(case, n):
    """Statistics, the sample, d_a and every actor gradient against float64; the critics are only read; two calls are bit-equal; a
    gathered call (indices into a ring with head != 0) equals the contiguous one bit for bit."""
    name = f"{case}_{n}"
    m, b, ref = make_model(case, "fp32", DEV), dev_inputs(case, n), restated(case, n)
    af = A.net_of(case)[1] * A.net_of(case)[2]
    m.critic_flat_grads().fill_(7.0)
    q0 = m.critic_flat_params().clone()
    ra = run_actor(m, b)
    stats_close(ra["stats"].cpu().numpy(), ref["stats"], f"{name} actor")
    assert float(ra["loss"]) == float(ra["stats"][0].float())
    assert (ra["a"].double().cpu() - ref["a"]).abs().max() <= 2e-5
    assert (ra["logp"].double().cpu() - ref["logp"]).abs().max() <= 2e-4 * af
    tried = check_with_gates(case, n, named(m.network, ra["ga"]), ra["d_a"], name)
    assert tried <= (1 if case != "wide" else len(ref["near_zero"]))  # (test_relu_gates_near_zero_are_few counts them)
    assert bool((m.critic_flat_grads() == 7.0).all()) and torch.equal(m.critic_flat_params(), q0)  # the members are only read
    again = run_actor(m, b)
    assert all(torch.equal(ra[k], again[k]) for k in ra), [k for k in ra if not torch.equal(ra[k], again[k])]
    z = torch.zeros(n, device=DEV)
    rp, inds = ring_of(dict(obs=b["obs"], next_obs=b["obs"], actions=torch.zeros(n, af, device=DEV), reward=z, terminated=z), n)
    assert rp.head != 0
    ring = run_actor(m, b, replay=rp, inds=inds)
    assert all(torch.equal(ra[k], ring[k]) for k in ra), [k for k in ra if not torch.equal(ra[k], ring[k])]
    loss = m.loss_actor({"state": b["obs"]}, alpha_dev(), noise=b["noise"])
    loss.backward()  # .backward() hands every actor parameter its slice
    w = m.network.mlp_mean.moduleList[0].linear_1.weight
    assert torch.equal(w.grad, dict(named(m.network, ra["ga"]))["mlp_mean.moduleList.0.linear_1.weight"])


@pytest.mark.gpu
def test_hip_rlpd_rows_do_not_depend_on_the_batch():
    """Rows 0..38 of a 39-row call against the same rows of the 77-row call: sample and log-probability bit-equal; d_a carries
    1 / N, so N d_a agrees to fp32 rounding of that one division."""
    m, b = make_model("chunk", "fp32", DEV), dev_inputs("chunk", 77)
    whole = run_actor(m, b)
    part = run_actor(m, {k: v[:39] for k, v in b.items()})
    for k in ("a", "logp"):
        assert torch.equal(part[k], whole[k][:39]), k
    x, y = 39.0 * part["d_a"].double(), 77.0 * whole["d_a"][:39].double()
    assert (x - y).abs().max() <= 1e-6 * y.abs().max()


@pytest.mark.gpu
def test_hip_rlpd_flattened_member_adds_nothing_to_g():
    """tiny_flat: the flattened member's W0 is 0, so whatever stands behind its layer 0 its share of g is exactly 0: with its upper
    layers doubled d_a and every actor gradient keep their bits (its Q, and with it the loss, moves), and all of it is finite."""
    case, n = "tiny_flat", 77
    m, b = make_model(case, "fp32", DEV), dev_inputs(case, n)
    ra = run_actor(m, b)
    assert all(bool(torch.isfinite(v).all()) for v in ra.values())
    flat = m.critic_networks[K.FLAT_MEMBER]
    with torch.no_grad():
        for k, p in flat.named_parameters():
            if not k.startswith("Q1.moduleList.0.linear_1"):
                p.mul_(2.0)
    m.critics_updated()
    rb = run_actor(m, b)
    assert torch.equal(ra["d_a"], rb["d_a"]) and torch.equal(ra["ga"], rb["ga"]) and torch.equal(ra["a"], rb["a"])
    assert not torch.equal(ra["stats"][:2], rb["stats"][:2]) and ra["d_a"].abs().max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", A.CASES, ids=IDS)
def test_hip_rlpd_loss_actor_bf16_within_twice_the_rounding_yardstick(case, n):
    """No tolerance is fixed: with e_y the error of the bf16-Linear restatement (LayerNorm in fp32) against the fp32 restatement,
    the call may be off by at most 2 e_y on the loss, on d_a, per tensor and on 1 - cosine."""
    m, b = make_model(case, "bf16", DEV), dev_inputs(case, n)
    res = run_actor(m, b)
    fp32, yard = restate(case, n, torch.float32), restate(case, n, torch.float32, bf16=True)
    order = [k for k, _ in fp32["named"]]
    call = dict(loss=res["loss"], d_a=res["d_a"], named=by_name(named(m.network, res["ga"]), order))
    e_y, e_c = rel_errors(fp32, yard), rel_errors(fp32, call)
    worst = max(e_c["per"], key=lambda k: e_c["per"][k] / (e_y["per"][k] + 1e-30))
    print(f"{case}_{n} bf16: yardstick loss {e_y['loss']:.3e} d_a {e_y['d_a']:.3e} 1-cos {e_y['one_minus_cos']:.3e}; call loss "
          f"{e_c['loss']:.3e} d_a {e_c['d_a']:.3e} 1-cos {e_c['one_minus_cos']:.3e}; worst tensor {worst}: {e_c['per'][worst]:.3e} "
          f"against {e_y['per'][worst]:.3e}")
    assert e_c["loss"] <= 2 * e_y["loss"] and e_c["d_a"] <= 2 * e_y["d_a"] and e_c["one_minus_cos"] <= 2 * e_y["one_minus_cos"]
    for k in e_c["per"]:
        assert e_c["per"][k] <= 2 * e_y["per"][k], (k, e_c["per"][k], e_y["per"][k])


# ------------------------------------------------------------------------------------------------------------------ the agent
def write_offline(path, obs_dim, action_dim, n_traj=4, traj_len=12, seed=3):
    rs = np.random.RandomState(seed)
    total = n_traj * traj_len
    terminals = np.zeros(total, dtype=np.float32)
    terminals[traj_len - 1::traj_len] = 1
    np.savez(path, states=rs.uniform(-1, 1, (total, obs_dim)).astype(np.float32),
             actions=rs.uniform(-1, 1, (total, action_dim)).astype(np.float32), rewards=rs.uniform(0, 1, total).astype(np.float32),
             terminals=terminals, traj_lengths=np.full(n_traj, traj_len))
    return str(path)


def agent_cfg(tmp_path, **train):
    cfg = copy.deepcopy(load_config(SHIPPED)[CHEETAH_CFG])
    cfg.update(device=DEV, seed=42, logdir=str(tmp_path), env=Cfg(n_envs=4, name="synthetic", max_episode_steps=5, reset_at_iteration=False))
    cfg.pop("wandb", None)
    cfg.model.update(device=DEV, n_critics=3)
    for node in (cfg.model.actor, cfg.model.critic):
        node["precision"] = "fp32"
        node["mlp_dims"] = [64, 64]
    cfg["offline_dataset"] = Cfg(_target_="dppo.agent.dataset.sequence.StitchedSequenceQLearningDataset",
                                 dataset_path=write_offline(tmp_path / "offline.npz", cfg.obs_dim, cfg.action_dim),
                                 horizon_steps=cfg.horizon_steps, cond_steps=cfg.cond_steps, device=DEV)
    cfg.train.update(dict(n_train_itr=6, n_explore_steps=2, n_steps=1, batch_size=8, critic_num_update=3, buffer_size=64, val_freq=100,
                          save_model_freq=100, log_freq=1), **train)
    return cfg


@pytest.mark.gpu
def test_hip_rlpd_agent_update_is_the_recorded_sequence(golden, tmp_path):
    """One fp32 ``update_iteration`` on cheetah, N = 77, with every draw given, against the sequence the reference recorded: two
    critic steps with Polyak, one actor step, one temperature step, ``log_alpha`` included."""
    from dppo_amd.agent.finetune.train_rlpd_agent import TrainRLPDAgent
    from dppo_amd.util.optim import FlatAdamW
    g, case, n = golden("g28_rlpd"), A.SEQ_CASE, A.SEQ_N
    agent = TrainRLPDAgent(agent_cfg(tmp_path, n_train_itr=0))
    m = agent.model = make_model(case, "fp32", DEV, K.backup_entropy(case, n))
    E = K.n_critics(case)
    agent.gamma, agent.target_entropy, agent.critic_num_update = K.GAMMA, S.target_entropy(case), A.SEQ_CRITIC_UPDATES
    agent.target_ema_rate = A.SEQ_TAU
    agent.critic_optimizer = FlatAdamW(m.critic_flat_params(), lr=A.SEQ_LR, weight_decay=A.SEQ_WEIGHT_DECAY)
    agent.actor_optimizer = FlatAdamW(m.network.flat_params(), lr=A.SEQ_ACTOR_LR, weight_decay=A.SEQ_WEIGHT_DECAY)
    agent.log_alpha = torch.tensor(A.SEQ_LOG_ALPHA, dtype=torch.float64, device=DEV, requires_grad=True)
    agent.log_alpha_optimizer = torch.optim.Adam([agent.log_alpha], lr=A.SEQ_LR)
    b = {k: v.to(DEV) for k, v in K.inputs(case, n).items()}
    sb = {k: v.to(DEV) for k, v in S.inputs(case, n).items()}
    batch = dict(obs=b["obs"].reshape(n, -1), next_obs=b["next_obs"].reshape(n, -1), actions=b["actions"].reshape(n, -1),
                 reward=b["reward"], terminated=b["terminated"])
    k = A.SEQ_CRITIC_UPDATES
    seen = []
    inner = m.loss_critic
    m.loss_critic = lambda *a, **kw: seen.append(inner(*a, **kw).detach().clone()) or seen[-1]
    lc, la, lt = agent.update_iteration(batches=[batch] * k, pairs=[K.pair_of(case, n)] * k, next_actions=[b["next_actions"]] * k,
                                        next_logp=[b["next_logp"]] * k, actor_noise=sb["noise"], temp_noise=sb["noise_t"])
    print(f"seq: critic {[float(x) for x in seen]} ref {g['seq_c_loss']}; actor {float(la)!r} ref {float(g['seq_a_loss'])!r}; temperature "
          f"{float(lt)!r} ref {float(g['seq_t_loss'])!r}; log_alpha {float(agent.log_alpha.detach())!r} ref {float(g['seq_log_alpha'])!r}")
    assert len(seen) == k and float(seen[-1]) == float(lc)
    np.testing.assert_allclose([float(x) for x in seen] + [float(la), float(lt)],
                               list(g["seq_c_loss"]) + [float(g["seq_a_loss"]), float(g["seq_t_loss"])], rtol=2e-4, atol=2e-5)
    assert abs(float(agent.log_alpha.detach()) - float(g["seq_log_alpha"])) <= 1e-6
    check_grads_fp32(g, "seq_gq1", member_rows(m.critic_flat_grads(), E))
    check_grads_fp32(g, "seq_ga", named(m.network, m.last_loss_grad))
    first = f"{case}_{n}_gq"
    check_stepped_twice(g, "seq_q", member_rows(m.critic_flat_params(), E), (first, "seq_gq1"), A.SEQ_LR)
    # the target after two Polyak averages: test_restatement_reproduces_the_recorded_sequence has the bound
    check_stepped_twice(g, "seq_target", member_rows(m.target_flat_params(), E), (first, "seq_gq1"), 2 * A.SEQ_LR * A.SEQ_TAU)
    check_stepped(g, "seq_actor", [(k, p) for k, p in m.network.named_parameters() if p.requires_grad], "seq_ga", A.SEQ_ACTOR_LR)


@pytest.mark.gpu
def test_hip_rlpd_agent_runs(tmp_path):
    """The shipped cfg shrunk (4 envs, batch 8, E = 3, hidden 64, 2 exploration iterations, 6 iterations, a synthetic offline file):
    iterations 2..5 update; records carry the reference's keys; every network moved, the targets by Polyak; a checkpoint round-trips
    bit for bit."""
    from dppo_amd.agent.finetune.train_rlpd_agent import TrainRLPDAgent
    agent = TrainRLPDAgent(agent_cfg(tmp_path))
    m = agent.model
    assert (agent.critic_num_update, agent.n_explore_steps, m.n_critics) == (3, 2, 3) and len(agent.dataset_offline) == 4 * 12
    assert agent.target_entropy == -6 and float(agent.log_alpha.detach()) == 0.0
    actor0, critic0, target0 = m.network.flat_params().clone(), m.critic_flat_params().clone(), m.target_flat_params().clone()
    calls = []
    inner = agent.update_iteration
    agent.update_iteration = lambda **kw: calls.append(agent.itr) or inner(**kw)
    res = agent.run()
    assert calls == [2, 3, 4, 5]
    assert [r["itr"] for r in res] == list(range(6)) and res[-1]["step"] == 6 * 4
    assert all(set(r) == {"itr", "step"} for r in res[:3])
    for r in res[3:]:
        assert set(r) == {"itr", "step", "time", "train_episode_reward", "loss_actor", "loss_critic", "alpha"}
        assert np.isfinite([r["loss_actor"], r["loss_critic"], r["alpha"]]).all()
    for now, before in ((m.network.flat_params(), actor0), (m.critic_flat_params(), critic0), (m.target_flat_params(), target0)):
        assert not torch.equal(now, before) and bool(torch.isfinite(now).all())
    moved = (m.target_flat_params() - target0).abs().max() / (m.critic_flat_params() - critic0).abs().max()
    assert 0 < float(moved) < 0.5  # Polyak at 0.005 over 12 updates: the targets trail the members
    assert float(agent.log_alpha.detach()) != 0.0
    data = torch.load(os.path.join(str(tmp_path), "checkpoint", "state_5.pt"), weights_only=True)
    assert list(data["model"]) == list(m.state_dict())
    other = TrainRLPDAgent(agent_cfg(tmp_path, n_train_itr=0))
    other.load(5)
    for a, b in ((other.model.network.flat_params(), m.network.flat_params()), (other.model.critic_flat_params(), m.critic_flat_params()),
                 (other.model.target_flat_params(), m.target_flat_params())):
        assert torch.equal(a, b)
    loss = other.model.loss_actor({"state": torch.zeros(4, 1, 17, device=DEV)}, 0.5, noise=torch.zeros(4, 1, 6, device=DEV))
    same = m.loss_actor({"state": torch.zeros(4, 1, 17, device=DEV)}, 0.5, noise=torch.zeros(4, 1, 6, device=DEV))
    assert torch.equal(loss.detach(), same.detach())  # the loaded kernel images are the saved weights'
