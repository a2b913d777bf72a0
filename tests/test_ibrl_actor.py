"""IBRL's actor loss through the ensemble's min (reference model/rl/gaussian_ibrl.py:115-128): ``IBRL_Gaussian.loss_actor`` =
``dppo_ibrl_actor_fwd_bwd`` (csrc/ibrl.h).

CPU: the fp32 restatement of tests/golden/make_golden_ibrl_actor_cases.py reproduces the g32 fixture the reference wrote (the loss,
d_a, every actor gradient, the selected members, one update sequence); the cases keep their conditions (gaps, wins per member, clamped
draws); the route the kernels take (the selected member's dq/da, d_u = d_a (1 - mu^2), d/dz = d/dz' keep s) is autograd's in float64;
both new C ABI entries check their arguments.

GPU, fp32: every case, ``twins`` and ``wide`` included, against the restatement in FLOAT64 fed the same fp32 values: statistics by
stats_close, ``sel`` equal on every row, d_a and every actor gradient by grad_violations' rule on every entry with no ReLU gate handed
over.  Bit identity: two calls; ring and contiguous; a 39-row call against the first 39 rows of the 77-row one; the mask drawn in the
kernel, written out and fed back; p = 0 and eval() against the null struct.  bf16: no tolerance is fixed; the yardstick is the
restatement with every Linear's operands rounded to bf16, both restated on the call's own ``sel``, and the call may be off from the fp32
restatement by at most twice the yardstick's own error.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from dppo_amd import hip
from tests.golden import make_golden_ibrl_actor_cases as A
from tests.test_dql import check_stepped, grad_violations, rel_errors, stats_close
from tests.test_idql import check_grads_fp32
from tests.test_qsm import close_to_fixture, ring_of
from tests.test_sac import by_name, check_stepped_twice, named, rel_close

K = A.K
DEV = "cuda:0"
D64 = torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))
IDS = [f"{c}_{n}" for c, n in A.ALL_CASES]
FIX_IDS = [f"{c}_{n}" for c, n in A.CASES]


@pytest.fixture(scope="module")
def g32():
    return np.load(os.path.join(HERE, "golden", "g32_ibrl_actor.npz"))


def make_model(case, prec, device):
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_ibrl import IBRL_Gaussian
    od, ta, da, dims, act, p, qdims, qact, E = A.net_of(case)
    actor = Gaussian_MLP(action_dim=da, horizon_steps=ta, cond_dim=od, mlp_dims=list(dims), activation_type=act, dropout=p,
                         fixed_std=A.FIXED_STD, precision=prec, plain_fixed_std=True)
    q = CriticObsAct(cond_dim=od, mlp_dims=list(qdims), action_dim=da, action_steps=ta, activation_type=qact, use_layernorm=True,
                     double_q=False, precision=prec)
    m = IBRL_Gaussian(actor=actor, critic=q, n_critics=E, horizon_steps=ta, device=device, randn_clip_value=A.RANDN_CLIP)
    m.network.load_state_dict(A.actor_state_dict(case), strict=True)
    for e in range(E):
        m.critic_networks[e].load_state_dict(A.member_params(case, e), strict=True)
    m.train()  # as the reference's agent leaves it: dropout is live
    return m


def restate(case, n, dtype=D64, bf16=False, sel=None):
    if bf16:
        with K.bf16_linears():
            return A.restate(case, n, dtype, sel=sel)
    return A.restate(case, n, dtype, sel=sel)


@functools.lru_cache(maxsize=None)
def restated(case, n, dtype=D64):
    """The restatement of one case on its own selection: computed once, shared, never modified."""
    return restate(case, n, dtype)


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case,n", A.CASES, ids=FIX_IDS)
def test_restatement_reproduces_the_reference_fixture(g32, case, n):
    r, name = restated(case, n, torch.float32), f"{case}_{n}"
    close_to_fixture(g32, f"{name}_a_loss", r["loss"], name)
    close_to_fixture(g32, f"{name}_d_a", r["d_a"], name)
    check_grads_fp32(g32, f"{name}_ga", r["named"])
    # the selected member per row, as the generator recomputed it in float64 from the reference's own modules
    assert np.array_equal(g32[f"{name}_sel"], restated(case, n)["sel"])


def test_restatement_reproduces_the_recorded_sequence(g32):
    """Two critic AdamW steps each with Polyak, one actor step, the target actor's Polyak, on tiny N = 77."""
    seq = A.restate_sequence()
    rel_close(seq["c_losses"] + [seq["a_loss"]], list(g32["seq_c_losses"]) + [float(g32["seq_a_loss"])], 1e-5, "seq losses")
    assert float(g32["seq_a_loss"]) != float(g32["tiny_77_a_loss"])  # the actor met the stepped members
    flat = lambda ps: [(str(e), torch.cat([t.reshape(-1) for t in p.values()])) for e, p in enumerate(ps)]
    for i in range(2):
        check_grads_fp32(g32, f"seq_gq{i}", flat(seq["gq"][i]))
    # a member took two steps; its target is (1 - tau)^2 t0 + tau (1 - tau) q1 + tau q2: off by at most tau times the sum of the
    # one-step and the two-step bound, which 2 tau times the two-step bound covers (tests/test_rlpd_actor.py's rule)
    check_stepped_twice(g32, "seq_q", flat(seq["q"]), ("seq_gq0", "seq_gq1"), A.SEQ_LR)
    check_stepped_twice(g32, "seq_target", flat(seq["target"]), ("seq_gq0", "seq_gq1"), 2 * A.SEQ_LR * A.SEQ_TAU)
    check_grads_fp32(g32, "seq_ga", list(seq["ga"].items()))
    check_stepped(g32, "seq_actor", list(seq["actor"].items()), "seq_ga", A.SEQ_ACTOR_LR)
    check_stepped(g32, "seq_target_actor", list(seq["target_actor"].items()), "seq_ga", A.SEQ_ACTOR_LR * A.SEQ_TAU)


@pytest.mark.parametrize("case,n", A.ALL_CASES, ids=IDS)
def test_cases_keep_their_conditions(case, n):
    c = A.check_conditions(case, n)
    print(f"{case}_{n}: smallest gap {c['gap']:.3e}, wins {c['wins'].tolist()}, clamped (lo, hi) {c['clamped']}, ReLU pre-activations "
          f"below {K.RELU_TIE:g}: {c['relu_near']}")
    assert len(restated(case, n)["sel"]) == n  # no row is left out of any comparison


def test_twins_d_a_does_not_depend_on_the_pick():
    r = restated("twins", 77)
    i, j = A.TWIN_PAIR
    other = np.where(r["sel"] == i, j, r["sel"])
    assert (r["sel"] == i).sum() >= 5 and not (r["sel"] == j).any()
    forced = restate("twins", 77, sel=other)
    assert torch.equal(forced["d_a"], r["d_a"]) and all(torch.equal(a, b) for a, b in zip(forced["grads"], r["grads"]))


@pytest.mark.parametrize("case,n", [("tiny", 77), ("chunk", 130), ("wide", 3)])
def test_analytic_route_is_autograds(case, n):
    """What the kernels compute, spelled out in float64: g = the selected member's dq/da, d_a = -g / N, d_u = d_a (1 - mu^2), and
    through every hidden layer d/dz = (upstream . W) act'(z') keep s with the mask applied explicitly."""
    b, ref = A.inputs(case, n), restated(case, n)
    p = K.cast(A.actor_params(case), D64)
    a = ref["a"].clone().requires_grad_(True)
    q = torch.stack([A.q_forward(K.cast(m, D64), case, b["obs"].double(), a) for m in A.members_of(case)])
    g = torch.autograd.grad(q.gather(0, torch.as_tensor(ref["sel"])[None])[0].sum(), a)[0]
    d_a = -g / n
    assert (d_a - ref["d_a"]).abs().max() <= 1e-12 * ref["d_a"].abs().max()
    pd, L = A.net_of(case)[5], len(A.net_of(case)[3])
    s = 1.0 / (1.0 - pd)
    act = A.net_of(case)[4]
    x, zs, hs = b["obs"].double().reshape(n, -1), [], []
    for i in range(L):
        z = torch.nn.functional.linear(x, p[f"mlp_mean.moduleList.{i}.linear_1.weight"], p[f"mlp_mean.moduleList.{i}.linear_1.bias"])
        z = z * b["mask"][i].double() * s if pd > 0 else z
        zs.append(z)
        hs.append(x)
        x = torch.nn.functional.mish(z) if act == "Mish" else torch.relu(z)

    def dact(z):
        if act == "ReLU":
            return (z > 0).double()
        zz = z.clone().requires_grad_(True)
        return torch.autograd.grad(torch.nn.functional.mish(zz).sum(), zz)[0]
    d = d_a * (1 - ref["mu"] ** 2)
    grads = {f"mlp_mean.moduleList.{L}.linear_1.weight": d.t() @ x, f"mlp_mean.moduleList.{L}.linear_1.bias": d.sum(0)}
    up = d @ p[f"mlp_mean.moduleList.{L}.linear_1.weight"]
    for i in reversed(range(L)):
        dz = up * dact(zs[i])
        if pd > 0:
            dz = dz * b["mask"][i].double() * s
        grads[f"mlp_mean.moduleList.{i}.linear_1.weight"], grads[f"mlp_mean.moduleList.{i}.linear_1.bias"] = dz.t() @ hs[i], dz.sum(0)
        up = dz @ p[f"mlp_mean.moduleList.{i}.linear_1.weight"]
    for k, want in ref["named"]:
        assert (grads[k] - want).abs().max() <= 1e-9 * want.abs().max() + 1e-15, k


def descs(case):
    m = make_model(case, "fp32", "cpu")
    return m.network.net_desc(), m.critic_networks[0].net_desc()


def test_ibrl_actor_entries_reject_bad_arguments_on_the_host():
    """Every refusal of both new entries leaves its reason in dppo_last_error(); nothing here touches a device."""
    lib = hip.load()
    err = lambda: lib.dppo_last_error()
    da, dq = descs("tiny")
    f32 = hip.PREC_F32

    def ws(a=da, q=dq, prec=f32, od=11, N=77, E=3):
        return lib.dppo_ibrl_actor_workspace_bytes(C.byref(a) if a is not None else None, C.byref(q) if q is not None else None, prec,
                                                   od, N, E)
    need = ws()
    assert need > 0
    assert ws(a=None) == -1 and b"null" in err()
    assert ws(q=None) == -1 and b"null" in err()
    assert ws(prec=7) == -1 and b"prec" in err()
    assert ws(N=0) == -1 and b"N out of range" in err()
    for E in (1, hip.RLPD_MAX_E + 1):
        assert ws(E=E) == -1 and b"members out of" in err()
    plain = hip.NetDesc.from_buffer_copy(dq)
    plain.use_layernorm = 0
    assert ws(q=plain) == -1 and b"LayerNorm" in err()
    two = hip.NetDesc.from_buffer_copy(dq)
    two.out_dim = 2
    assert ws(q=two) == -1 and b"out_dim 1" in err()  # a two-output member
    ln = hip.NetDesc.from_buffer_copy(da)
    ln.use_layernorm = 1
    assert ws(a=ln) == -1 and b"LayerNorm" in err()
    residual = hip.NetDesc(kind=1, in_dim=11, hidden=256, n_blocks=1, out_dim=3, act=hip.ACT_RELU, time_dim=0, act_flat=0, cond_dim=11,
                           cond_hidden=0, cond_out=0, use_layernorm=0, plain=0)
    assert ws(a=residual) == -1 and b"dropout runs in a plain" in err()
    assert ws(q=descs("chunk")[1]) == -1 and b"does not pair" in err()  # tiny's actor against chunk's members
    assert ws(od=12) == -1 and b"do not pair" in err()
    wa, wq = descs("wide")
    for prec in (hip.PREC_F32, hip.PREC_BF16):  # the top of the accepted range
        assert ws(a=wa, q=wq, prec=prec, N=3, E=16) > 0, err()
    one = C.c_double(0)  # stands in for every pointer: refusals come before anything is read
    ptr = C.addressof(one)
    imgs = (C.c_void_p * 3)(ptr, ptr, ptr)
    cfg = make_model("tiny", "fp32", "cpu").network.gaussian_cfg(randn_clip=3.0)
    drop = lambda p=0.5: hip.Dropout(p=p, seed_lo=1, seed_hi=2, pad=0, mask=None, mask_out=None)

    def call(a=da, q=dq, E=3, actor_params=ptr, packed=ptr, q_params=ptr, images=imgs, cfg=cfg, d=None,
             batch=hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 0, 77), N=77, grad=ptr, stats=ptr, wsp=ptr, wsb=1 << 40, prec=f32,
             od=11):
        return lib.dppo_ibrl_actor_fwd_bwd(C.byref(a), C.byref(q), prec, E, actor_params, packed, q_params, images,
                                           C.byref(cfg) if cfg is not None else None, C.byref(d) if d is not None else None,
                                           C.byref(batch) if batch is not None else None, od, N, None, grad, stats, None, None, None,
                                           None, wsp, wsb, None)
    for kw in (dict(actor_params=None), dict(packed=None), dict(q_params=None), dict(images=None), dict(grad=None), dict(stats=None),
               dict(wsp=None)):
        assert call(**kw) == -1 and b"null pointer" in err(), kw
    assert call(images=(C.c_void_p * 3)(ptr, None, ptr)) == -1 and b"kernel image of member 1" in err()
    assert call(cfg=None) == -1 and b"null" in err()
    assert call(batch=None) == -1 and b"null batch" in err()
    assert call(q=plain) == -1 and b"LayerNorm" in err()
    assert call(a=ln) == -1 and b"LayerNorm" in err()
    assert call(a=residual) == -1 and b"dropout runs in a plain" in err()
    assert call(od=12) == -1 and b"do not pair" in err()
    assert call(prec=5) == -1 and b"prec" in err()
    assert call(N=0) == -1 and b"N out of range" in err()
    assert call(E=1) == -1 and b"members out of" in err()
    det = type(cfg).from_buffer_copy(cfg)
    det.deterministic = 1
    assert call(cfg=det) == -1 and b"deterministic" in err()
    learned = type(cfg).from_buffer_copy(cfg)
    learned.std_mode = 1
    assert call(cfg=learned) == -1 and b"std" in err()
    assert call(d=drop(1.0)) == -1 and b"dropout p" in err()
    assert call(d=drop(-0.1)) == -1 and b"dropout p" in err()
    for bad in (hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 77, 77), hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 0, 78),
                hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 0, 1, 0, 0), hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 0, 0, 77)):
        assert call(batch=bad) == -1 and b"ring geometry" in err()
    assert call(batch=hip.IdqlBatch(ptr, ptr, ptr, ptr, ptr, None, 77, 1, 0, 76)) == -1 and b"exceeds" in err()
    assert call(batch=hip.IdqlBatch(None, ptr, ptr, ptr, ptr, None, 77, 1, 0, 77)) == -1 and b"null pointer in batch" in err()
    assert call(wsb=need - 1) == -1 and b"workspace too small" in err()


def test_workspace_query_accepts_every_shipped_cfg():
    from dppo_amd.cfg.loader import instantiate, load_config
    lib, cfgs = hip.load(), load_config(os.path.join(HERE, "golden", "shipped_ibrl_cfgs.json"))
    assert len(cfgs) == 8
    for name, cfg in cfgs.items():
        m = instantiate(cfg.model, network_path=None)
        da, dq = m.network.net_desc(), m.critic_networks[0].net_desc()
        for prec in (hip.PREC_F32, hip.PREC_BF16):
            assert lib.dppo_ibrl_actor_workspace_bytes(C.byref(da), C.byref(dq), prec, cfg.obs_dim * cfg.cond_steps,
                                                       int(cfg.train.batch_size), m.n_critics) > 0, (name, lib.dppo_last_error())


# ------------------------------------------------------------------------------------------------------------------ GPU
def dev_inputs(case, n):
    return {k: v.to(DEV) for k, v in A.inputs(case, n).items()}


OUT = ("loss", "stats", "ga", "d_a", "a", "qmin", "sel")


def run_actor(m, b, replay=None, inds=None, noise=True, mask=True):
    src = replay if replay is not None else {"state": b["obs"]}
    use_mask = mask and m.network.training and m.network.dropout > 0
    loss = m.loss_actor(src, inds, noise=b["noise"] if noise else None, mask=b["mask"] if use_mask else None, want_mask=True)
    return dict(loss=loss.detach().clone(), stats=m.last_stats.clone(), ga=m.last_loss_grad.clone(), d_a=m.last_d_a.clone(),
                a=m.last_actions.clone(), qmin=m.last_qmin.clone(), sel=m.last_sel.clone(),
                mask=None if m.last_drop_mask is None else m.last_drop_mask.clone())


def same_bits(x, y, keys=OUT):
    return [k for k in keys if not torch.equal(x[k], y[k])]


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", A.ALL_CASES, ids=IDS)
def test_hip_ibrl_loss_actor_fp32(g32, case, n):
    """Statistics, the sample, the selection, d_a and every actor gradient against float64 (no ReLU gate is handed over); close to the
    fixture; the members are only read and their gradient buffer untouched; two calls are bit-equal; a gathered call (indices into a
    ring with head != 0) equals the contiguous one bit for bit; ``backward()`` hands the slices out."""
    m, b, ref = make_model(case, "fp32", DEV), dev_inputs(case, n), restated(case, n)
    af = A.net_of(case)[1] * A.net_of(case)[2]
    m.critic_flat_grads().fill_(7.0)
    q0 = m.critic_flat_params().clone()
    img0 = [t.clone() for t in m._ens.images(m.prec)[1]]
    ra = run_actor(m, b)
    stats_close(ra["stats"].cpu().numpy(), ref["stats"], f"{case}_{n} actor")
    assert float(ra["loss"]) == float(ra["stats"][0].float())
    assert (ra["a"].double().cpu() - ref["a"]).abs().max() <= 2e-5
    assert (ra["qmin"].double().cpu() - ref["qmin"]).abs().max() <= 1e-5 * max(1.0, float(ref["qmin"].abs().max()))
    assert np.array_equal(ra["sel"].cpu().numpy(), ref["sel"]), np.flatnonzero(ra["sel"].cpu().numpy() != ref["sel"])
    if case == "twins":
        assert not (ra["sel"] == A.TWIN_PAIR[1]).any() and int((ra["sel"] == A.TWIN_PAIR[0]).sum()) >= 5  # the lower index
    order = [k for k, _ in ref["named"]]
    got = [("d_a", ra["d_a"])] + by_name(named(m.network, ra["ga"]), order)
    bad = grad_violations([("d_a", ref["d_a"])] + ref["named"], got)
    assert not bad, (case, n, bad)
    if (case, n) in A.CASES:
        name = f"{case}_{n}"
        assert abs(float(ra["loss"]) - float(g32[f"{name}_a_loss"])) <= 1e-5 * max(1.0, abs(float(g32[f"{name}_a_loss"])))
        check_grads_fp32(g32, f"{name}_ga", named(m.network, ra["ga"]))
    assert bool((m.critic_flat_grads() == 7.0).all()) and torch.equal(m.critic_flat_params(), q0)  # the members are only read
    assert all(torch.equal(x, y) for x, y in zip(img0, m._ens.images(m.prec)[1]))  # ... and so are their kernel images
    again = run_actor(m, b)
    assert not same_bits(ra, again), same_bits(ra, again)
    z = torch.zeros(n, device=DEV)
    rp, inds = ring_of(dict(obs=b["obs"], next_obs=b["obs"], actions=torch.zeros(n, af, device=DEV), reward=z, terminated=z), n)
    assert rp.head != 0
    ring = run_actor(m, b, replay=rp, inds=inds)
    assert not same_bits(ra, ring), same_bits(ra, ring)
    loss = m.loss_actor({"state": b["obs"]}, noise=b["noise"], mask=b["mask"] if m.network.dropout > 0 else None)
    assert m.last_drop_mask is None  # written out only where asked for
    loss.backward()  # .backward() hands every actor parameter its slice
    w = m.network.mlp_mean.moduleList[0].linear_1.weight
    assert torch.equal(w.grad, dict(named(m.network, ra["ga"]))["mlp_mean.moduleList.0.linear_1.weight"])
    assert all(p.grad is None for net in m.critic_networks for p in net.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_hip_ibrl_rows_depend_on_their_own_row_alone(prec):
    """Rows 0..38 of a 39-row call equal those of the 77-row call in the sample's, the min's and the gradient rows' bits."""
    case = "tiny"
    m, b = make_model(case, prec, DEV), dev_inputs(case, 77)
    full = run_actor(m, b)
    head = dict(obs=b["obs"][:39].contiguous(), noise=b["noise"][:39].contiguous(), mask=b["mask"][:, :39].contiguous())
    part = run_actor(m, head)
    for k in ("a", "qmin", "sel"):
        assert torch.equal(part[k], full[k][:39]), k
    # d_a = -g / N: the same g, divided by another N
    g_part, g_full = part["d_a"].double() * 39, full["d_a"][:39].double() * 77
    assert (g_part - g_full).abs().max() <= 2.0 ** -22 * g_full.abs().max()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case,n", [("tiny", 77), ("chunk", 130)])
def test_hip_ibrl_drawn_mask_fed_back_reproduces_every_bit(case, n, prec):
    """The mask drawn in the kernel is written out; fed back as a given mask it reproduces every output bit for bit; its keep share
    is 1 - p within five standard deviations."""
    m, b = make_model(case, prec, DEV), dev_inputs(case, n)
    torch.manual_seed(5)
    drawn = run_actor(m, b, mask=False)
    p = A.net_of(case)[5]
    assert drawn["mask"] is not None and set(drawn["mask"].unique().tolist()) <= {0, 1}
    share, cnt = float(drawn["mask"].float().mean()), drawn["mask"].numel()
    assert abs(share - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / cnt), share
    fed = run_actor(m, dict(b, mask=drawn["mask"]))
    assert not same_bits(drawn, fed), same_bits(drawn, fed)
    assert torch.equal(fed["mask"], drawn["mask"])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_hip_ibrl_no_dropout_is_the_null_struct_path(prec):
    """eval() and p = 0 equal the null-struct call bit for bit, and with eval() the result is the restatement without masks."""
    case, n = "tiny", 77
    m, b = make_model(case, prec, DEV), dev_inputs(case, n)
    m.network.eval()
    ev = run_actor(m, b)
    assert ev["mask"] is None
    m.network.train()
    m.network.dropout = 0.0  # live iff training and dropout > 0: the null struct again
    p0 = run_actor(m, b)
    assert not same_bits(ev, p0), same_bits(ev, p0)
    # p = 0 through a struct: the library's own rule (a struct with p = 0 and no mask is the path without dropout)
    lib, net, q = hip.load(), m.network, m.critic_networks[0]
    da, dq = net.net_desc(), q.net_desc()
    cfg = net.gaussian_cfg(deterministic=False, randn_clip=m.randn_clip_value)
    drop = hip.Dropout(p=0.0, seed_lo=3, seed_hi=4, pad=0, mask=None, mask_out=None)
    obs, noise = b["obs"].reshape(n, -1).contiguous(), b["noise"].reshape(n, -1).contiguous()
    batch = hip.IdqlBatch(obs.data_ptr(), None, None, None, None, None, n, 1, 0, n)
    wsb = lib.dppo_ibrl_actor_workspace_bytes(C.byref(da), C.byref(dq), m.prec, 11, n, 3)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    grad, stats = torch.empty_like(net.flat_params()), torch.empty(3, dtype=torch.float64, device=DEV)
    d_a = torch.empty(n, 3, device=DEV)
    hip.check(lib.dppo_ibrl_actor_fwd_bwd(C.byref(da), C.byref(dq), m.prec, 3, net.flat_params().data_ptr(),
                                          net.packed(m.prec, 0).data_ptr(), m.critic_flat_params().data_ptr(), m._ens.images(m.prec)[0],
                                          C.byref(cfg), C.byref(drop), C.byref(batch), 11, n, noise.data_ptr(), grad.data_ptr(),
                                          stats.data_ptr(), d_a.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(), hip.stream()),
              "dppo_ibrl_actor_fwd_bwd")
    assert torch.equal(grad, ev["ga"]) and torch.equal(stats, ev["stats"]) and torch.equal(d_a, ev["d_a"])
    if prec == "fp32":
        ref = A.restate(case, n, use_mask=False)
        stats_close(ev["stats"].cpu().numpy(), ref["stats"], "eval()")
        bad = grad_violations([("d_a", ref["d_a"])] + ref["named"],
                              [("d_a", ev["d_a"])] + by_name(named(m.network, ev["ga"]), [k for k, _ in ref["named"]]))
        assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", A.CASES, ids=FIX_IDS)
def test_hip_ibrl_loss_actor_bf16_within_twice_the_rounding_yardstick(case, n):
    """No tolerance is fixed: with e_y the error of the bf16-Linear restatement against the fp32 restatement, both on the call's own
    selection, the call may be off by at most 2 e_y on the loss, on d_a, per tensor and on 1 - cosine.  The call's ``sel`` must be the
    float64 one on every row whose float64 gap exceeds twice the yardstick's own Q error.
    Measured on MI355X, call against yardstick: d_a 1.89 x (tiny_1: one row, nothing averages, and the error is the members' chain's
    in front of the tail), 1.00 x (tiny_77), 1.11 x (chunk_130), 1.00 x (nodrop_64, can_256, twins_77); worst tensor 1.94 x (tiny_1: the out
    bias, which at N = 1 is d_out itself: 4.06e-3 against 2.09e-3), 1.01 x, 1.15 x, 1.01 x, 1.00 x, 1.10 x; 1 - cosine at most 1.24 x
    (chunk_130); rows within twice the bf16 Q error: 0, 2, 3, 1, 9, 2, none of them decided differently from float64."""
    m, b = make_model(case, "bf16", DEV), dev_inputs(case, n)
    res = run_actor(m, b)
    r64 = restated(case, n)
    sel = res["sel"].cpu().numpy().astype(np.int64)
    fp32, yard = restate(case, n, torch.float32, sel=sel), restate(case, n, torch.float32, bf16=True, sel=sel)
    q_err = float((yard["q"].double() - r64["q"]).abs().max())
    srt = torch.sort(r64["q"], dim=0).values
    if case == "twins":
        keep = [e for e in range(r64["q"].shape[0]) if e != A.TWIN_PAIR[1]]
        srt = torch.sort(r64["q"][keep], dim=0).values
        assert not (sel == A.TWIN_PAIR[1]).any()
    sure = ((srt[1] - srt[0]) > 2 * q_err).numpy() if srt.shape[0] > 1 else np.ones(n, dtype=bool)
    assert np.array_equal(sel[sure], r64["sel"][sure]), (case, np.flatnonzero(sel != r64["sel"]))
    order = [k for k, _ in fp32["named"]]
    call = dict(loss=res["loss"], d_a=res["d_a"], named=by_name(named(m.network, res["ga"]), order))
    e_y, e_c = rel_errors(fp32, yard), rel_errors(fp32, call)
    worst = max(e_c["per"], key=lambda k: e_c["per"][k] / (e_y["per"][k] + 1e-30))
    print(f"{case}_{n} bf16: {int((~sure).sum())} of {n} rows within twice the bf16 Q error {q_err:.3e}, {int((sel != r64['sel']).sum())} "
          f"decided differently; yardstick loss {e_y['loss']:.3e} d_a {e_y['d_a']:.3e} 1-cos {e_y['one_minus_cos']:.3e}; call loss "
          f"{e_c['loss']:.3e} d_a {e_c['d_a']:.3e} 1-cos {e_c['one_minus_cos']:.3e}; worst tensor {worst}: {e_c['per'][worst]:.3e} "
          f"against {e_y['per'][worst]:.3e} ({e_c['per'][worst] / (e_y['per'][worst] + 1e-30):.2f} x)")
    assert e_c["loss"] <= 2 * e_y["loss"] and e_c["d_a"] <= 2 * e_y["d_a"] and e_c["one_minus_cos"] <= 2 * e_y["one_minus_cos"]
    for k in e_c["per"]:
        assert e_c["per"][k] <= 2 * e_y["per"][k], (k, e_c["per"][k], e_y["per"][k])
