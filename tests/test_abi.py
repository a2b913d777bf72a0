"""CPU-side checks of the drop-in boundary: the shared library loads, exports every symbol the header declares,
argument validation works without a GPU, and the product path refuses to run on CPU (no silent fallback)."""
import ctypes as C
import os
import re

import pytest
import torch

from dppo_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "dppo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dppo_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = hip.load()
    names = header_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"libdppo_hip.so does not export {n}"
    assert sorted(hip.SYMBOLS) == names, "ctypes table and header disagree"
    assert lib.dppo_version() == 1


def hopper_desc():
    return hip.NetDesc(kind=0, in_dim=39, hidden=512, n_blocks=1, out_dim=12, act=hip.ACT_RELU, time_dim=16,
                       act_flat=12, cond_dim=11, cond_hidden=0, cond_out=0)


def test_param_count_matches_reference_sizes():
    lib = hip.load()
    assert lib.dppo_net_param_count(C.byref(hopper_desc())) == 553020
    critic = hip.NetDesc(kind=1, in_dim=11, hidden=256, n_blocks=1, out_dim=1, act=hip.ACT_MISH, time_dim=0,
                         act_flat=0, cond_dim=11, cond_hidden=0, cond_out=0)
    assert lib.dppo_net_param_count(C.byref(critic)) == 134913
    for prec in (hip.PREC_F32, hip.PREC_BF16):
        assert lib.dppo_packed_bytes(C.byref(hopper_desc()), prec, 20) > 553020
        assert lib.dppo_ppo_workspace_bytes(C.byref(hopper_desc()), C.byref(critic), prec, 50000) > 0


def test_bad_arguments_are_rejected_with_a_message():
    lib = hip.load()
    d = hopper_desc()
    d.hidden = 100
    assert lib.dppo_net_param_count(C.byref(d)) == -1
    assert b"hidden" in lib.dppo_last_error()
    d = hopper_desc()
    d.in_dim = 40
    assert lib.dppo_packed_bytes(C.byref(d), hip.PREC_BF16, 20) == -1
    assert lib.dppo_packed_bytes(C.byref(hopper_desc()), 7, 20) == -1
    assert lib.dppo_gae(None, None, None, None, 1, 1, 0.99, 0.95, 1.0, None, None, None, None, None) == -1
    # tuning knobs: a retired or unknown number is an error that names it, never a silent no-op
    for knob in (9, 10, 31, 32, 33, 34, 35, 39, 40):
        assert lib.dppo_tune_set(knob, 1) != 0
        msg = lib.dppo_last_error()
        assert str(knob).encode() in msg and b"retired" in msg
    assert lib.dppo_tune_set(99, 1) != 0
    assert b"99" in lib.dppo_last_error() and b"unknown" in lib.dppo_last_error()
    assert lib.dppo_tune_set(2, 1) == 0  # a live knob set to its default


def test_python_layout_matches_c_abi_and_reference_names():
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    a = DiffusionMLP(3, 4, 11, mlp_dims=[512, 512, 512], activation_type="ReLU", residual_style=True)
    c = CriticObs(11, [256, 256, 256], residual_style=True)
    assert list(dict(a.named_parameters())) == [
        "time_embedding.1.weight", "time_embedding.1.bias", "time_embedding.3.weight", "time_embedding.3.bias",
        "mlp_mean.layers.0.weight", "mlp_mean.layers.0.bias", "mlp_mean.layers.1.l1.weight",
        "mlp_mean.layers.1.l1.bias", "mlp_mean.layers.1.l2.weight", "mlp_mean.layers.1.l2.bias",
        "mlp_mean.layers.2.weight", "mlp_mean.layers.2.bias"]
    assert list(dict(c.named_parameters()))[:2] == ["Q1.layers.0.weight", "Q1.layers.0.bias"]
    lib = hip.load()
    assert a.flat_params().numel() == lib.dppo_net_param_count(C.byref(a.net_desc()))
    assert c.flat_params().numel() == lib.dppo_net_param_count(C.byref(c.net_desc()))
    # parameters are views of the flat image, in state-dict order
    f = a.flat_params()
    off = 0
    for p in a.parameters():
        assert p.data_ptr() == f.data_ptr() + 4 * off
        off += p.numel()


def test_no_cpu_fallback():
    from dppo_amd.model.common.critic import CriticObs
    c = CriticObs(11, [256, 256, 256], residual_style=True)
    with pytest.raises(hip.DppoHipError):
        c({"state": torch.zeros(2, 1, 11)})


def test_unsupported_variants_fail_loudly():
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    with pytest.raises(NotImplementedError):  # LayerNorm blocks exist only on the fused kernels' widths
        DiffusionMLP(3, 4, 11, mlp_dims=[384, 384, 384], residual_style=True, use_layernorm=True)
    with pytest.raises(NotImplementedError):  # plain trunks: one hidden width, no LayerNorm / cond_mlp
        DiffusionMLP(3, 4, 11, mlp_dims=[512, 512, 512], residual_style=False, use_layernorm=True)
    with pytest.raises(NotImplementedError):
        DiffusionMLP(3, 4, 11, mlp_dims=[512, 256], residual_style=False)
    d = hopper_desc()
    d.use_layernorm, d.hidden = 1, 384
    assert hip.load().dppo_net_param_count(C.byref(d)) < 0


def test_plain_mlp_layout_matches_reference_names():
    """residual_style=False: moduleList.{i}.linear_1 names (reference mlp.py:46-74) and the C ABI's flat size."""
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    a = DiffusionMLP(3, 4, 11, mlp_dims=[64, 64], residual_style=False)
    names = [n for n in dict(a.named_parameters()) if n.startswith("mlp_mean.")]
    assert names == [f"mlp_mean.moduleList.{i}.linear_1.{w}" for i in range(3) for w in ("weight", "bias")]
    d = a.net_desc()
    assert d.plain == 1 and d.n_blocks == 1 and d.hidden == 64
    assert a.flat_params().numel() == hip.load().dppo_net_param_count(C.byref(d))
    c = CriticObs(cond_dim=11, mlp_dims=[64, 64], residual_style=False)
    assert c.flat_params().numel() == hip.load().dppo_net_param_count(C.byref(c.net_desc())) == 11 * 64 + 64 + 64 * 64 + 64 + 64 + 1


def test_layernorm_layout_matches_reference_names():
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    a = DiffusionMLP(3, 4, 11, mlp_dims=[512, 512, 512], residual_style=True, use_layernorm=True)
    names = [n for n in dict(a.named_parameters()) if n.startswith("mlp_mean.layers.1.")]
    assert names == [f"mlp_mean.layers.1.{m}.{w}" for m in ("l1", "l2", "norm1", "norm2") for w in ("weight", "bias")]
    assert a.flat_params().numel() == hip.load().dppo_net_param_count(C.byref(a.net_desc())) == 553020 + 4 * 512


def test_cond_mlp_layout_matches_reference_names():
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    a = DiffusionMLP(9, 4, 60, mlp_dims=[256, 256, 256], residual_style=True, cond_mlp_dims=[128, 32])
    names = list(dict(a.named_parameters()))
    assert names[4:8] == ["cond_mlp.moduleList.0.linear_1.weight", "cond_mlp.moduleList.0.linear_1.bias",
                          "cond_mlp.moduleList.1.linear_1.weight", "cond_mlp.moduleList.1.linear_1.bias"]
    assert names[8] == "mlp_mean.layers.0.weight" and tuple(a.mlp_mean.layers[0].weight.shape) == (256, 36 + 16 + 32)
    lib = hip.load()
    assert a.flat_params().numel() == lib.dppo_net_param_count(C.byref(a.net_desc()))


def test_new_entry_points_reject_bad_descriptors_with_a_message():
    """Argument validation of the round-2 entries runs on the host (no GPU needed): every refusal leaves its reason in
    dppo_last_error()."""
    lib = hip.load()
    v = hip.VisDesc(in_ch=3, img_h=96, img_w=96, embed_dim=128, num_heads=4, depth=1, embed_norm=0, prop_dim=9, spatial_emb=128,
                    num_img=1)
    assert lib.dppo_vis_param_count(C.byref(v)) == 419712
    for field, value, word in (("img_h", 97, b"image"), ("embed_dim", 100, b"embed_dim"), ("num_heads", 3, b"num_heads"),
                               ("depth", 9, b"depth"), ("num_img", 3, b"num_img"), ("embed_norm", 1, b"embed_norm"),
                               ("img_w", 512, b"patches")):
        bad = hip.VisDesc.from_buffer_copy(v)
        setattr(bad, field, value)
        assert lib.dppo_vis_param_count(C.byref(bad)) == -1, field
        assert word in lib.dppo_last_error(), (field, lib.dppo_last_error())
    assert lib.dppo_vis_workspace_bytes(C.byref(v), hip.PREC_BF16, 0, 1) == -1
    # plain trunks: multiples of 64, no LayerNorm / cond_mlp; wide outputs only off the denoiser
    d = hopper_desc()
    d.plain, d.hidden, d.in_dim = 1, 64, 39
    assert lib.dppo_net_param_count(C.byref(d)) == 2 * 16 * 16 + 2 * 16 + 2 * 16 * 16 + 16 + 39 * 64 + 64 + 64 * 64 + 64 + 12 * 64 + 12
    d.use_layernorm = 1
    assert lib.dppo_net_param_count(C.byref(d)) == -1 and b"plain" in lib.dppo_last_error()
    d = hopper_desc()
    d.out_dim = d.act_flat = 140
    d.in_dim = 140 + 16 + 11
    assert lib.dppo_net_param_count(C.byref(d)) == -1 and b"out_dim" in lib.dppo_last_error()
    wide = hip.NetDesc(kind=1, in_dim=23, hidden=512, n_blocks=1, out_dim=140, act=hip.ACT_MISH, time_dim=0, act_flat=0,
                       cond_dim=23, cond_hidden=0, cond_out=0)
    assert lib.dppo_net_param_count(C.byref(wide)) == 23 * 512 + 512 + 2 * (512 * 512 + 512) + 140 * 512 + 140
    assert lib.dppo_sample_chain_workspace_bytes(C.byref(d), hip.PREC_BF16, 16) == -1
    # GMM: the two trunks must agree with the cfg
    wts = hip.NetDesc(kind=1, in_dim=23, hidden=512, n_blocks=1, out_dim=5, act=hip.ACT_MISH, time_dim=0, act_flat=0, cond_dim=23,
                      cond_hidden=0, cond_out=0)
    crit = hip.NetDesc(kind=1, in_dim=23, hidden=256, n_blocks=1, out_dim=1, act=hip.ACT_MISH, time_dim=0, act_flat=0, cond_dim=23,
                       cond_hidden=0, cond_out=0)
    assert lib.dppo_gmm_workspace_bytes(C.byref(wide), C.byref(wts), C.byref(crit), hip.PREC_BF16, 64) > 0
    cfg = hip.GmmCfg(horizon_steps=4, action_dim=7, num_modes=4, std_mode=0, fixed_std=0.1)
    assert lib.dppo_gmm_logprob(C.byref(wide), C.byref(wts), hip.PREC_BF16, None, None, None, None, C.byref(cfg), None, None, None,
                                4, None, None, 0, None) == -1
    assert b"out_dim" in lib.dppo_last_error()


def test_unet_descriptors_are_rejected_with_a_message():
    """check_desc of the conv denoiser: a network the reference cannot run is refused by name, not run over the wrong width."""
    lib = hip.load()

    def desc(mults=(1, 2), **kw):
        f = dict(action_dim=7, cond_dim=23, horizon_steps=4, time_dim=16, dim=64, n_levels=len(mults),
                 mults=(C.c_int32 * 4)(*(list(mults) + [0] * (4 - len(mults)))), kernel_size=5, n_groups=8, larger_encoder=1,
                 cond_predict_scale=1, act=hip.ACT_MISH, groupnorm_eps=1e-5)
        f.update(kw)
        return C.byref(hip.UnetDesc(**f))
    assert lib.dppo_unet_param_count(desc()) > 0
    assert lib.dppo_unet_param_count(desc(mults=(1, 2, 1))) > 0  # decreasing multipliers are the reference's to run
    # final_conv is Conv1dBlock(dim, dim) on a map of dim * dim_mults[0] channels: the reference raises unless dim_mults[0] == 1
    for mults in ((3,), (2, 4), (2, 1)):
        for call in (lambda d: lib.dppo_unet_param_count(d), lambda d: lib.dppo_unet_packed_bytes(d, hip.PREC_BF16, 20),
                     lambda d: lib.dppo_unet_workspace_bytes(d, hip.PREC_F32, 4)):
            assert call(desc(mults=mults)) == -1, mults
            assert b"final_conv" in lib.dppo_last_error() and b"dim_mults[0]" in lib.dppo_last_error(), lib.dppo_last_error()
    for kw, word in ((dict(mults=(1, 2, 4, 8, 16)[:4], n_levels=5), b"n_levels"), (dict(dim=36), b"dim"), (dict(n_groups=33), b"n_groups"),
                     (dict(n_groups=7), b"n_groups"), (dict(horizon_steps=6, mults=(1, 2, 4)), b"horizon_steps"),
                     (dict(horizon_steps=65), b"horizon_steps"), (dict(action_dim=65), b"action_dim"), (dict(time_dim=130), b"time_dim"),
                     (dict(cond_dim=1025), b"cond_dim"), (dict(kernel_size=4), b"kernel_size"), (dict(mults=(1, 17)), b"channel")):
        assert lib.dppo_unet_param_count(desc(**kw)) == -1, kw
        assert word in lib.dppo_last_error(), (kw, lib.dppo_last_error())


def test_gemm_test_entries_validate_their_arguments_on_the_host():
    """dppo_gemm_nt_desc_raw / dppo_gemm_tn_group_raw / dppo_gemm_tn_job_raw / dppo_gemm_tn_raw refuse a bad call with -1
    and a message before anything is launched (the pointers below are never dereferenced: no GPU here)."""
    lib = hip.load()
    p = 0x1000  # non-null, never read
    err = lib.dppo_last_error

    def nt(**kw):
        f = dict(X=p, W=p, bias=None, M=100, N=40, Kp=64, ldx=64, ldw=64, dsrc=None, dsrc_kind=0, dsrc_ld=0, dact=0, ldres=0,
                 res=None, add=None, out_f32=p, out_pre=None, out_act=None, ldadd=0, ldo32=48, ldo=0, act=0)
        f.update(kw)
        return C.byref(hip.GemmNTDesc(**f))
    B16 = hip.PREC_BF16
    assert lib.dppo_gemm_nt_desc_raw(B16, None, None) == -1 and b"null" in err()
    for kw, word in ((dict(X=None), b"null"), (dict(W=None), b"null"), (dict(out_f32=None), b"null"), (dict(M=0), b"M"),
                     (dict(N=0), b"N"), (dict(Kp=72, ldx=72, ldw=72), b"Kp"), (dict(Kp=0), b"Kp"), (dict(ldx=56), b"ldx"),
                     (dict(ldx=68), b"ldx"), (dict(ldw=70), b"ldw"), (dict(ldw=32), b"ldw"), (dict(ldo32=40), b"ldo32"),
                     (dict(ldo32=50), b"ldo32"), (dict(out_pre=p, ldo=47), b"ldo"), (dict(out_act=p, ldo=0), b"ldo"),
                     (dict(dsrc_kind=3), b"dsrc_kind"), (dict(dsrc_kind=1), b"dsrc"), (dict(dsrc_kind=2, dsrc=p, dsrc_ld=44), b"dsrc_ld"),
                     (dict(res=p, ldres=40), b"ldres"), (dict(add=p, ldadd=16), b"ldadd"), (dict(act=3), b"act"),
                     (dict(dact=-1), b"act")):
        assert lib.dppo_gemm_nt_desc_raw(B16, nt(**kw), None) == -1, kw
        assert word in err(), (kw, err())
    assert lib.dppo_gemm_nt_desc_raw(7, nt(), None) == -1
    assert lib.dppo_gemm_nt_desc_raw(hip.PREC_F32, nt(Kp=48, ldx=48, ldw=48), None) == -1 and b"Kp" in err()  # fp32: 32 per k-tile
    assert lib.dppo_gemm_nt_desc_raw(hip.PREC_F32, nt(ldx=66), None) == -1 and b"ldx" in err()                # fp32: 4 per 16 bytes

    def job(**kw):
        f = dict(A=p, B=p, slab=p, M=1000, lda=512, N1=512, ldb=64, N2=40, rows_per_split=256, ncol_a=0, ncol_b=0, pad=0)
        f.update(kw)
        return hip.GemmTNJob(**f)
    out = (C.c_void_p * 9)(*([p] * 9))
    bad_jobs = ((dict(A=None), b"null"), (dict(B=None), b"null"), (dict(slab=None), b"null"), (dict(M=0), b"M"),
                (dict(N1=0), b"N1"), (dict(rows_per_split=100), b"rows_per_split"), (dict(rows_per_split=0), b"rows_per_split"),
                (dict(lda=516), b"lda"), (dict(ldb=60), b"ldb"), (dict(lda=504), b"lda"), (dict(ldb=32), b"ldb"),
                (dict(ncol_a=500), b"ncol_a"), (dict(lda=64, ncol_a=256), b"ncol_a"), (dict(ldb=8, ncol_b=24), b"ncol_b"))
    for kw, word in bad_jobs:
        assert lib.dppo_gemm_tn_job_raw(B16, C.byref(job(**kw)), p, None) == -1, kw
        assert word in err(), (kw, err())
        jobs = (hip.GemmTNJob * 2)(job(), job(**kw))  # the second job of a group is checked like the first
        assert lib.dppo_gemm_tn_group_raw(B16, jobs, 2, out, None) == -1, kw
        assert word in err(), (kw, err())
    assert lib.dppo_gemm_tn_job_raw(B16, None, p, None) == -1 and b"null" in err()
    assert lib.dppo_gemm_tn_job_raw(B16, C.byref(job()), None, None) == -1 and b"null" in err()
    jobs = (hip.GemmTNJob * 9)(*[job() for _ in range(9)])
    for n in (0, -1, 9):
        assert lib.dppo_gemm_tn_group_raw(B16, jobs, n, out, None) == -1 and b"1..8" in err()
    assert lib.dppo_gemm_tn_group_raw(B16, None, 1, out, None) == -1 and b"null" in err()
    assert lib.dppo_gemm_tn_group_raw(B16, jobs, 1, None, None) == -1 and b"null" in err()
    out[1] = None
    assert lib.dppo_gemm_tn_group_raw(B16, jobs, 2, out, None) == -1 and b"C_out[1]" in err()
    assert lib.dppo_gemm_tn_group_raw(7, jobs, 1, out, None) == -1
    assert lib.dppo_gemm_tn_job_raw(hip.PREC_F32, C.byref(job(lda=514)), p, None) == -1 and b"lda" in err()  # fp32: multiples of 4
    # dppo_gemm_tn_raw: the same leading-dimension rules
    for lda, ldb in ((504, 64), (512, 32), (516, 64), (512, 60)):
        assert lib.dppo_gemm_tn_raw(B16, p, lda, 512, p, ldb, 40, 1000, 256, p, p, None) == -1, (lda, ldb)
        assert b"lda" in err()
    assert lib.dppo_gemm_tn_raw(B16, p, 512, 512, p, 64, 40, 1000, 100, p, p, None) == -1 and b"rows_per_split" in err()
    assert lib.dppo_gemm_tn_raw(B16, None, 512, 512, p, 64, 40, 1000, 256, p, p, None) == -1
