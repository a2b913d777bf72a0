"""CPU-side pins of the training driver's host decisions (no GPU: the library's host code runs without one).

* every ``dppo_*_workspace_bytes`` export returns what tests/golden/workspace_bytes.json records.  The table was written
  by the library built from commit fa6215e ("Add IDQL fine-tuning ..."), the last one in which every entry point sized its
  own buffers and re-derived the backward's route: it pins the carve order and every size (38 KB, 1,594 short lines);
* ``dppo_backward_route`` reports the path the fused backward takes, against a table read off the predicates
  (tests/test_hip_parity.py::_one_block_ab states the same in prose).

``python -m tests.test_route --write`` rewrites the golden table from whatever library DPPO_HIP_LIB names."""
import ctypes as C
import json
import os
import sys

import pytest

from dppo_amd import hip
from oracle import dppo_oracle as O
from tests.test_hip_parity import HIP_SUPPORTED

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")
PRECS = {"fp32": hip.PREC_F32, "bf16": hip.PREC_BF16}
SIZES = (64, 1300, 6500, 50000)
KFT = 10


def descs(sname):
    """(actor, critic) descriptors of a named spec, built the way tests/test_hip_parity.py::build_model builds its networks."""
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    a, c = O.named_specs(sname)
    actor = DiffusionMLP(action_dim=a.action_dim, horizon_steps=a.horizon_steps, cond_dim=a.cond_dim, time_dim=a.time_dim,
                         mlp_dims=list(a.mlp_dims), activation_type=a.activation, cond_mlp_dims=a.cond_mlp_dims,
                         residual_style=True, use_layernorm=a.use_layernorm)
    critic = CriticObs(cond_dim=c.cond_dim, mlp_dims=list(c.mlp_dims), activation_type=c.activation, residual_style=True,
                       use_layernorm=c.use_layernorm)
    return actor.net_desc(), critic.net_desc()


def trunk(like, **kw):
    d = hip.NetDesc.from_buffer_copy(like)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def workspace_row(lib, sname, prec, N):
    """Every MLP workspace export at one (spec, precision, N); the Gaussian / mixture / Q trunks are the critic's trunk with
    the actor's action width (kind 1: what those entry points take)."""
    a, c = descs(sname)
    R = C.byref
    gauss = trunk(c, out_dim=a.act_flat)
    mean, wts = trunk(c, out_dim=5 * a.act_flat), trunk(c, out_dim=5)
    q = trunk(c, in_dim=c.in_dim + a.act_flat, cond_dim=c.in_dim + a.act_flat)
    return {
        "mlp_forward_actor": lib.dppo_mlp_forward_workspace_bytes(R(a), prec, N),
        "mlp_forward_critic": lib.dppo_mlp_forward_workspace_bytes(R(c), prec, N),
        "sample_chain": lib.dppo_sample_chain_workspace_bytes(R(a), prec, N),
        "chain_logprob": lib.dppo_chain_logprob_workspace_bytes(R(a), prec, N, KFT),
        "bc_loss": lib.dppo_bc_loss_workspace_bytes(R(a), prec, N, KFT),
        "denoise_mse": lib.dppo_denoise_mse_workspace_bytes(R(a), prec, N),
        "ppo": lib.dppo_ppo_workspace_bytes(R(a), R(c), prec, N),
        "gaussian": lib.dppo_gaussian_workspace_bytes(R(gauss), R(c), prec, N),
        "gaussian_infer": lib.dppo_gaussian_workspace_bytes(R(gauss), None, prec, N),
        "gaussian_bc": lib.dppo_gaussian_bc_workspace_bytes(R(gauss), prec, N),
        "gmm": lib.dppo_gmm_workspace_bytes(R(mean), R(wts), R(c), prec, N),
        "gmm_infer": lib.dppo_gmm_workspace_bytes(R(mean), R(wts), None, prec, N),
        "gmm_bc": lib.dppo_gmm_bc_workspace_bytes(R(mean), R(wts), prec, N),
        "idql_v_loss": lib.dppo_idql_v_loss_workspace_bytes(R(q), R(c), prec, N, 1),
        "idql_q_loss": lib.dppo_idql_q_loss_workspace_bytes(R(q), R(c), prec, N, 1),
        "idql_q_loss_single": lib.dppo_idql_q_loss_workspace_bytes(R(q), R(c), prec, N, 0),
        "idql_q_forward": lib.dppo_idql_q_forward_workspace_bytes(R(q), prec, N, 1),
    }


def other_rows(lib, prec, N):
    """The exports that take no residual-MLP actor: a plain trunk's sampler, the conv denoiser, the visual encoder."""
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    R = C.byref
    plain = DiffusionMLP(3, 4, 11, mlp_dims=[256, 256, 256], activation_type="ReLU", residual_style=False).net_desc()
    _, critic = descs("can")
    u = hip.UnetDesc(action_dim=7, cond_dim=23, horizon_steps=4, time_dim=16, dim=64, n_levels=2, mults=(C.c_int32 * 4)(1, 2, 0, 0),
                     kernel_size=5, n_groups=8, larger_encoder=1, cond_predict_scale=1, act=hip.ACT_MISH, groupnorm_eps=1e-5)
    v = hip.VisDesc(in_ch=3, img_h=96, img_w=96, embed_dim=128, num_heads=4, depth=1, embed_norm=0, prop_dim=9, spatial_emb=128,
                    num_img=1)
    return {
        "plain_sample": lib.dppo_plain_sample_workspace_bytes(R(plain), prec, N),
        "unet": lib.dppo_unet_workspace_bytes(R(u), prec, N),
        "unet_sample": lib.dppo_unet_sample_workspace_bytes(R(u), prec, N, 1),
        "unet_ppo": lib.dppo_unet_ppo_workspace_bytes(R(u), R(critic), prec, N),
        "unet_denoise_mse": lib.dppo_unet_denoise_mse_workspace_bytes(R(u), prec, N),
        "vis_train": lib.dppo_vis_workspace_bytes(R(v), prec, min(N, 6500), 1),
        "vis_infer": lib.dppo_vis_workspace_bytes(R(v), prec, min(N, 6500), 0),
    }


def workspace_table(lib):
    t = {}
    for pname, prec in PRECS.items():
        for N in SIZES:
            for sname in sorted(HIP_SUPPORTED):
                t[f"{sname}/{pname}/{N}"] = workspace_row(lib, sname, prec, N)
            t[f"other/{pname}/{N}"] = other_rows(lib, prec, N)
    return t


def test_every_workspace_size_equals_the_recorded_table():
    want = json.load(open(GOLDEN))
    got = workspace_table(hip.load())
    assert sorted(got) == sorted(want)
    assert len(want) == 2 * len(SIZES) * (len(HIP_SUPPORTED) + 1)
    for key in want:
        assert got[key] == want[key], key
    # no export refused its descriptor (-1); only the sampler, with no encoder and no split kernel, needs no workspace at all
    assert all(v > 0 or (v == 0 and name == "sample_chain") for row in want.values() for name, v in row.items())


# ---- dppo_backward_route ------------------------------------------------------------------------------------------------
BITS = ("fused", "one_block", "lowrank", "merged", "onehot", "dw0", "dw0_nhot", "dw0_round", "need_aux", "side_tail",
        "tail_post", "post_one")
ZEROED, DOBS, SIDE = 1, 2, 4
PPO_ACTOR, PPO_CRITIC = ZEROED | SIDE, ZEROED


def route(d, prec, N, flags, Kft=KFT):
    mask = C.c_int(-1)
    rc = hip.load().dppo_backward_route(C.byref(d), PRECS[prec], N, Kft, flags, C.byref(mask))
    assert rc == 0, hip.load().dppo_last_error()
    assert 0 <= mask.value < 1 << len(BITS)
    return {b for i, b in enumerate(BITS) if mask.value >> i & 1}


ONE = {"fused", "one_block", "lowrank", "merged"}  # a one-block network on its own kernels, N >= 100 out_dim
HOPPER_ACTOR = ONE | {"onehot", "dw0", "dw0_nhot", "dw0_round", "side_tail", "tail_post", "post_one"}
CRITIC = ONE | {"dw0", "post_one"}  # (no time embedding: no one-hot, nothing for a side tail)


def test_route_of_the_headline_networks():
    """hopper at the headline minibatch: everything on -- 12 action + 11 observation columns leave room for 9 of the 10
    one-hot columns, the tenth is rebuilt (dw0_round)."""
    a, c = descs("hopper")
    assert route(a, "bf16", 50000, PPO_ACTOR) == HOPPER_ACTOR
    assert route(c, "bf16", 50000, PPO_CRITIC) == CRITIC
    # 5 fine-tuned steps: every one-hot column fits, none is rebuilt
    assert route(a, "bf16", 6500, PPO_ACTOR, Kft=5) == HOPPER_ACTOR - {"dw0_round"}


@pytest.mark.parametrize("sname,cols", [("halfcheetah", 41), ("can", 79)])
def test_wide_actors_keep_dh0_but_their_critics_do_not(sname, cols):
    a, c = descs(sname)
    assert a.act_flat + a.cond_dim == cols > 32  # informative input columns: more than the 32 the in-kernel product holds
    # (the time-embedding gradient then stays behind the GEMMs, in the one post-reduce launch)
    assert route(a, "bf16", 50000, PPO_ACTOR) == ONE | {"onehot", "post_one"}
    assert route(c, "bf16", 50000, PPO_CRITIC) == CRITIC


@pytest.mark.parametrize("sname", ["hopper", "halfcheetah", "can"])
def test_fp32_never_takes_the_in_kernel_first_layer_gradient(sname):
    a, c = descs(sname)
    ra, rc = route(a, "fp32", 50000, PPO_ACTOR), route(c, "fp32", 50000, PPO_CRITIC)
    assert not (ra | rc) & {"dw0", "dw0_nhot", "dw0_round", "side_tail", "tail_post"}
    assert {"fused", "one_block", "lowrank", "onehot", "post_one"} <= ra and {"fused", "one_block", "lowrank", "post_one"} <= rc
    # the merged forward's fp32 LDS image fits the 256-wide critics, not a 512-wide actor (fused_can_merge, knob 22)
    assert "merged" not in ra and "merged" in rc


def test_small_minibatches_leave_the_one_block_route():
    a, c = descs("hopper")
    assert 100 * a.out_dim == 1200
    r = route(a, "bf16", 1199, PPO_ACTOR)
    assert not r & {"one_block", "lowrank", "dw0", "side_tail", "tail_post"} and {"fused", "onehot", "post_one"} <= r
    assert {"one_block", "lowrank", "dw0"} <= route(a, "bf16", 1200, PPO_ACTOR)
    assert not route(c, "bf16", 99, PPO_CRITIC) & {"one_block", "lowrank", "dw0"}
    assert {"one_block", "lowrank", "dw0"} <= route(c, "bf16", 100, PPO_CRITIC)


def test_callers_that_bring_less_get_less():
    """Behaviour cloning and the denoising loss zero no arrival counters: no in-kernel dW0, and the time-embedding gradient
    goes through the separate launches (post_one off).  Outside PPO no critic-like trunk takes the in-kernel dW0 either.  A
    caller that wants d loss / d observation needs dh_0 in memory."""
    a, c = descs("hopper")
    assert route(a, "bf16", 50000, SIDE) == ONE | {"onehot"}
    assert route(c, "bf16", 50000, 0, Kft=0) == ONE | {"post_one"}
    assert route(a, "bf16", 50000, PPO_ACTOR | DOBS) == ONE | {"onehot", "post_one"}
    assert route(c, "bf16", 50000, PPO_CRITIC | DOBS) == ONE | {"post_one"}
    assert route(a, "bf16", 50000, ZEROED) == HOPPER_ACTOR - {"side_tail", "tail_post"}  # no side stream to put a tail on
    # no denoising steps told (Kft = 0): no one-hot columns, the time-embedding gradient is a pass of its own
    assert route(a, "bf16", 50000, 0, Kft=0) == ONE | {"need_aux", "post_one"}


@pytest.mark.parametrize("knob,cleared", [(37, {"dw0", "dw0_nhot", "dw0_round", "side_tail", "tail_post"}),
                                          (38, {"side_tail", "tail_post"}), (41, {"tail_post"}),
                                          (18, {"dw0", "dw0_nhot", "dw0_round", "side_tail", "tail_post", "post_one"}),
                                          (16, {"lowrank", "one_block", "dw0", "dw0_nhot", "dw0_round", "side_tail", "tail_post"}),
                                          (11, {"onehot", "dw0", "dw0_nhot", "dw0_round", "side_tail", "tail_post"})])
def test_a_knob_clears_its_own_bit_and_what_depends_on_it(knob, cleared):
    lib = hip.load()
    a, _ = descs("hopper")
    try:
        assert lib.dppo_tune_set(knob, 0) == 0
        r = route(a, "bf16", 50000, PPO_ACTOR)
    finally:
        lib.dppo_tune_set(knob, 1)
    extra = {"need_aux"} if knob == 11 else set()  # without the one-hot columns the gradient needs its own pass
    assert r == (HOPPER_ACTOR - cleared) | extra
    assert route(a, "bf16", 50000, PPO_ACTOR) == HOPPER_ACTOR


def test_layered_path_and_refused_knob_combination():
    lib = hip.load()
    a, _ = descs("hopper")
    mask = C.c_int(0)
    try:
        assert lib.dppo_tune_set(1, 0) == 0
        assert "fused" not in route(a, "bf16", 50000, PPO_ACTOR)
    finally:
        lib.dppo_tune_set(1, 1)
    try:  # knob 8's "no dh_0 store" experiments have nothing to switch off once dh_0 never exists
        for v in (1, 32):
            assert lib.dppo_tune_set(8, v) == 0
            assert lib.dppo_backward_route(C.byref(a), hip.PREC_BF16, 50000, KFT, PPO_ACTOR, C.byref(mask)) != 0
            assert b"knob 37" in lib.dppo_last_error()
            assert lib.dppo_tune_set(37, 0) == 0
            assert lib.dppo_backward_route(C.byref(a), hip.PREC_BF16, 50000, KFT, PPO_ACTOR, C.byref(mask)) == 0
            assert lib.dppo_tune_set(37, 1) == 0
    finally:
        lib.dppo_tune_set(8, 0)
        lib.dppo_tune_set(37, 1)
    assert lib.dppo_backward_route(C.byref(a), hip.PREC_BF16, 0, KFT, 0, C.byref(mask)) != 0
    assert lib.dppo_backward_route(C.byref(a), hip.PREC_BF16, 64, KFT, 8, C.byref(mask)) != 0
    assert lib.dppo_backward_route(C.byref(a), hip.PREC_BF16, 64, KFT, 0, None) != 0


if __name__ == "__main__" and "--write" in sys.argv:
    hip.SYMBOLS.pop("dppo_backward_route")  # (a library from before the export has no such symbol)
    with open(GOLDEN, "w") as f:
        json.dump(workspace_table(hip.load()), f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN} from {hip.LIB_PATH}")
