// C ABI of libdppo_hip.so (include/dppo_hip.h): argument checks, layouts, workspace carving and the
// launch sequences.  No allocation, no synchronisation, no global mutable state.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "fused.h"
#include "gemm.h"
#include "ppo.h"
#include "gaussian.h"
#include "gmm.h"
#include "idql.h"
#include "qsm.h"
#include "dql.h"
#include "sac.h"
#include "rlpd.h"
#include "calql.h"
#include "ibrl.h"
#include "unet.h"
#include "sampler.h"

using namespace dppo;

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
namespace dppo {
void set_vis_mfma_attn(int v);  // vision.hip
}
namespace dppo {  // the same two helpers for the other translation units that export entry points (unet.hip)
int api_fail(int code, const char* msg) { return fail(code, "%s", msg); }
int api_check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail((int)e, "HIP launch failed: %s", hipGetErrorString(e));
  return 0;
}
}  // namespace dppo
// A fused kernel refused a shape that fused_ok() admitted: the packed image then holds no layered operands to fall back
// on, so the call must fail (reported by the check_launch() that ends every entry point).
static int g_fused_fault = 0;
static int check_launch() {
  if (g_fused_fault) {
    const int rc = g_fused_fault;
    g_fused_fault = 0;
    return fail(-1, "fused MLP kernel refused the launch (code %d): shape admitted by the packer but not by the kernel", rc);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail((int)e, "HIP launch failed: %s", hipGetErrorString(e));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// layouts
// ------------------------------------------------------------------------------------------------
struct ParamLayout {  // float offsets into the flat fp32 parameter / gradient buffer (state-dict order)
  int64_t te1_w, te1_b, te2_w, te2_b, c1w, c1b, c2w, c2b, W0, b0, l1w[MAX_BLOCKS], l1b[MAX_BLOCKS], l2w[MAX_BLOCKS], l2b[MAX_BLOCKS],
      n1w[MAX_BLOCKS], n1b[MAX_BLOCKS], n2w[MAX_BLOCKS], n2b[MAX_BLOCKS], Wout, bout, total;
  int64_t n0w, n0b;  // plain trunk with LayerNorm: layer 0's norm_1 (the hidden layers' are n1w / n1b)
};
static ParamLayout param_layout(const dppo_net_desc& d) {
  ParamLayout L;
  memset(&L, 0, sizeof(L));
  int64_t o = 0;
  const int td = d.time_dim, H = d.hidden;
  if (d.kind == 0) {
    L.te1_w = o, o += 2 * td * td;
    L.te1_b = o, o += 2 * td;
    L.te2_w = o, o += td * 2 * td;
    L.te2_b = o, o += td;
    if (d.cond_hidden > 0) {
      L.c1w = o, o += (int64_t)d.cond_hidden * d.cond_dim;
      L.c1b = o, o += d.cond_hidden;
      L.c2w = o, o += (int64_t)d.cond_out * d.cond_hidden;
      L.c2b = o, o += d.cond_out;
    }
  }
  L.W0 = o, o += (int64_t)H * d.in_dim;
  L.b0 = o, o += H;
  const bool plain_ln = d.plain && d.use_layernorm;  // linear_1.weight, linear_1.bias, norm_1.weight, norm_1.bias per hidden layer
  if (plain_ln) {
    L.n0w = o, o += H;
    L.n0b = o, o += H;
  }
  for (int b = 0; b < d.n_blocks; ++b) {
    L.l1w[b] = o, o += (int64_t)H * H;
    L.l1b[b] = o, o += H;
    if (plain_ln) {
      L.n1w[b] = o, o += H;
      L.n1b[b] = o, o += H;
    }
    if (d.plain) continue;  // a plain MLP's hidden layers are single Linear(H, H) modules (mlp.py:46-74)
    L.l2w[b] = o, o += (int64_t)H * H;
    L.l2b[b] = o, o += H;
    if (d.use_layernorm) {
      L.n1w[b] = o, o += H;
      L.n1b[b] = o, o += H;
      L.n2w[b] = o, o += H;
      L.n2b[b] = o, o += H;
    }
  }
  L.Wout = o, o += (int64_t)d.out_dim * H;
  L.bout = o, o += d.out_dim;
  L.total = o;
  return L;
}

struct PackLayout {  // byte offsets into the packed image
  // every offset depends on (net, prec) only; the time table sits last so that only `total` grows with n_time
  size_t W0, W1[MAX_BLOCKS], W2[MAX_BLOCKS], Wout, W1T[MAX_BLOCKS], W2T[MAX_BLOCKS], WoutT, W0tT, sstream, ostream,
      bstream, wcomp, ostream2, cbias, w0comp, ostream0, cbias2, Wc1, Wc2, Wc2T, W0eT, temb, total;
  int Kp0, Kpo, tdp;
  int Kp0s, CNT0;  // one-block networks: padded K of the first-layer composite Wout . W0 and its out-stream k-steps per wave
  int Kpc, C1p, Ep;  // cond_mlp: padded K of the encoder layers (cond, hidden) and padded encoder width
};
static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
// Width of a network's input rows x (and of the row-major first-layer operand): in_dim padded to 64 -- and, for a denoiser,
// with at least 24 spare columns behind in_dim: the one-hot of the row's denoising step lives there (plan_route()), and
// without room for it the time-embedding gradient costs a gemm_nt over all rows, a segmented sum and two more launches
// (halfcheetah: in_dim 57, 7 spare of 64: +40 us per update until the rows became 128 wide).
static int row_kp0(const dppo_net_desc& d) {
  int k = round_up(d.in_dim, 64);
  if (d.kind == 0 && k - d.in_dim < 24) k += 64;
  return k;
}
template <class P>
static PackLayout pack_layout(const dppo_net_desc& d, int n_time) {
  PackLayout L;
  memset(&L, 0, sizeof(L));
  const size_t ES = P::ESIZE;
  const int H = d.hidden;
  L.Kp0 = row_kp0(d);
  L.Kpo = round_up(d.out_dim, 64);
  L.tdp = round_up(d.time_dim > 0 ? d.time_dim : 1, 16);
  size_t o = 0;
  L.W0 = o, o = al256(o + (size_t)H * L.Kp0 * ES);
  for (int b = 0; b < d.n_blocks; ++b) {
    L.W1[b] = o, o = al256(o + (size_t)H * H * ES);
    L.W2[b] = o, o = al256(o + (size_t)H * H * ES);
    L.W1T[b] = o, o = al256(o + (size_t)H * H * ES);
    L.W2T[b] = o, o = al256(o + (size_t)H * H * ES);
  }
  L.Wout = o, o = al256(o + (size_t)d.out_dim * H * ES);
  L.WoutT = o, o = al256(o + (size_t)H * L.Kpo * ES);
  if (d.kind == 0) L.W0tT = o, o = al256(o + (size_t)d.time_dim * H * ES);
  if (!d.plain && d.out_dim <= 128) {  // per-wave fragment streams: forward (sampler + fused forward), out layer, backward
    const SamplerGeom g = sampler_geom<P>(d);
    const FusedGeom fg = fused_geom<P>(d);
    L.sstream = o, o = al256(o + (size_t)SAMPLER_WAVES * g.hidden_frags_per_wave * 64 * 16);
    L.ostream = o, o = al256(o + (size_t)SAMPLER_WAVES * g.out_frags_per_wave * 64 * 16);
    L.bstream = o, o = al256(o + (size_t)SAMPLER_WAVES * fg.frags_per_wave * 64 * 16);
    L.wcomp = o, o = al256(o + (size_t)d.out_dim * H * 4);  // fp32 Wout . W2 of the top block (source of its composite layer)
    // merged out layer (inference): out = Wout . h_in + (Wout . W2) . act(z1) + cbias, cbias = bout + Wout . b2
    L.ostream2 = o, o = al256(o + (size_t)SAMPLER_WAVES * g.out_frags_per_wave * 64 * 16);
    L.cbias = o, o = al256(o + (size_t)round_up(d.out_dim, 16) * 4);
    if (d.n_blocks == 1) {  // the fused forward's merged out layer (FusedFwdArgs::merge_top)
      L.Kp0s = g.Kp0, L.CNT0 = (g.KS0 + SAMPLER_WAVES - 1) / SAMPLER_WAVES;
      L.w0comp = o, o = al256(o + (size_t)d.out_dim * L.Kp0s * 4);
      L.ostream0 = o, o = al256(o + (size_t)SAMPLER_WAVES * L.CNT0 * g.OT * 64 * 16);
      L.cbias2 = o, o = al256(o + (size_t)round_up(d.out_dim, 16) * 4);
    }
  }
  L.Kpc = round_up(d.cond_dim > 0 ? d.cond_dim : 1, 64);
  if (d.cond_hidden > 0) {  // observation encoder: row-major GEMM operands (small), W2^T and the encoder columns of W0
    L.C1p = round_up(d.cond_hidden, 64), L.Ep = round_up(d.cond_out, 64);
    L.Wc1 = o, o = al256(o + (size_t)d.cond_hidden * L.Kpc * ES);
    L.Wc2 = o, o = al256(o + (size_t)d.cond_out * L.C1p * ES);
    L.Wc2T = o, o = al256(o + (size_t)d.cond_hidden * L.Ep * ES);
    L.W0eT = o, o = al256(o + (size_t)d.cond_out * H * ES);
  }
  L.temb = o, o = al256(o + (size_t)n_time * (d.time_dim > 0 ? d.time_dim : 0) * 4);
  L.total = o;
  return L;
}

// ln_plain: the caller reads a plain kind-1 trunk with LayerNorm (rlpd.h); every other entry refuses one
static int check_net(const dppo_net_desc* d, bool ln_plain = false) {
  if (!d) return fail(-1, "null net descriptor");
  if (d->kind != 0 && d->kind != 1) return fail(-1, "net.kind must be 0 (actor) or 1 (critic)");
  if (d->plain != 0 && d->plain != 1) return fail(-1, "plain must be 0 or 1");
  if (d->plain) {  // non-residual MLP trunk (model/common/mlp.py:27-81): layered GEMM path only
    if (d->hidden < 64 || d->hidden % 64) return fail(-1, "plain MLP: hidden=%d must be a positive multiple of 64", d->hidden);
    if (d->n_blocks < 1) return fail(-1, "plain MLP: at least two hidden widths (n_blocks = hidden-to-hidden layers >= 1)");
    if (d->cond_hidden || d->cond_out) return fail(-1, "plain MLP: cond_mlp is not built");
    if (d->use_layernorm == 1 && d->kind == 0) return fail(-1, "plain MLP: LayerNorm is built for kind-1 (critic) trunks only");
    if (d->use_layernorm == 1 && !ln_plain)
      return fail(-1, "plain MLP with LayerNorm: this entry is not taught it; dppo_idql_q_forward with double_q = 0, dppo_rlpd_q_loss_fwd_bwd and dppo_calql_q_loss_fwd_bwd read such a trunk");
    if (d->use_layernorm == 1 && d->hidden > LN_MAX_H) return fail(-1, "plain MLP with LayerNorm: hidden=%d above %d", d->hidden, LN_MAX_H);
  } else if (d->hidden < 128 || d->hidden % 128) return fail(-1, "hidden=%d must be a positive multiple of 128", d->hidden);
  if (d->n_blocks < 0 || d->n_blocks > MAX_BLOCKS) return fail(-1, "n_blocks=%d out of [0,%d]", d->n_blocks, MAX_BLOCKS);
  if (d->act != DPPO_ACT_RELU && d->act != DPPO_ACT_MISH) return fail(-1, "activation %d unsupported", d->act);
  // (out_dim > 128 -- the mixture-of-Gaussians head, Ta*Da*num_modes outputs -- runs on the layered GEMM path only: no
  // fragment streams are packed, and such a descriptor is refused by the K-step sampler)
  if (d->out_dim < 1 || d->out_dim > 1024) return fail(-1, "out_dim=%d out of [1,1024]", d->out_dim);
  if (d->out_dim > 128 && d->kind == 0) return fail(-1, "a denoiser's out_dim = Ta*Da must be <= 128");
  if (d->kind == 0) {
    if (d->time_dim < 4 || d->time_dim % 2) return fail(-1, "time_dim=%d must be even and >= 4", d->time_dim);
    if (d->act_flat != d->out_dim) return fail(-1, "actor out_dim must equal act_flat");
    if ((d->cond_hidden > 0) != (d->cond_out > 0)) return fail(-1, "cond_hidden / cond_out must both be set or both 0");
    if (d->cond_hidden < 0 || d->cond_hidden > 1024 || d->cond_out > 256) return fail(-1, "cond_mlp dims out of range");
    if (d->cond_out > 0 && (d->act_flat + d->time_dim) % 4) return fail(-1, "cond_mlp needs Ta*Da + time_dim to be a multiple of 4");
    if (d->in_dim != d->act_flat + d->time_dim + (d->cond_out > 0 ? d->cond_out : d->cond_dim))
      return fail(-1, "actor in_dim mismatch");
  } else {
    if (d->in_dim != d->cond_dim) return fail(-1, "critic in_dim must equal cond_dim");
    if (d->cond_hidden || d->cond_out) return fail(-1, "critic has no cond_mlp");
  }
  if (d->in_dim < 1 || d->in_dim > 1024) return fail(-1, "in_dim=%d out of [1,1024]", d->in_dim);
  if (d->use_layernorm != 0 && d->use_layernorm != 1) return fail(-1, "use_layernorm must be 0 or 1");
  if (d->use_layernorm && !d->plain && !(d->hidden == 256 || d->hidden == 512 || d->hidden == 1024))
    return fail(-1, "LayerNorm blocks need hidden in {256, 512, 1024} (fused kernels only), got %d", d->hidden);
  return 0;
}
static int check_prec(int prec) {
  if (prec != DPPO_PREC_F32 && prec != DPPO_PREC_BF16) return fail(-1, "prec must be DPPO_PREC_F32 or DPPO_PREC_BF16");
  return 0;
}
#define DPPO_DISPATCH(prec, CALL)        \
  ((prec) == DPPO_PREC_F32 ? CALL(F32) : CALL(BF16))

static int g_use_fused = 1;  // tuning knob 1: 1 = fused row-tile kernels where the shape is covered, 0 = layered GEMMs

template <class P>
static bool fused_ok(const dppo_net_desc& d) {
  // the input tile (width round_up(in_dim, .)) and the d_out tile share an H-wide LDS image with the activations
  if (d.plain) return false;
  return (g_use_fused || d.use_layernorm) && fused_rows_per_tile<P>(d) > 0 && d.out_dim <= 128 && d.hidden <= 1024 &&
         sampler_geom<P>(d).Kp0 <= d.hidden && fused_geom<P>(d).KpB0 <= d.hidden;
}

// ------------------------------------------------------------------------------------------------
// pack
// ------------------------------------------------------------------------------------------------
static int g_pack_one = 1;  // tuning knob 13: one launch per network for all of its kernel-ready images
template <class P>
static int pack_impl(const dppo_net_desc& d, int n_time, const float* prm, char* pk, hipStream_t s,
                     PackNet* defer_pn = nullptr, ComposeJob* defer_cj = nullptr, bool* deferred = nullptr) {
  // defer_pn / defer_cj: the caller launches the one-launch pack (and the composite) itself, batched with another
  // network's (dppo_pack_nets); *deferred tells whether this network's could be deferred
  const ParamLayout pl = param_layout(d);
  const PackLayout L = pack_layout<P>(d, n_time);
  const int H = d.hidden;
  if (deferred) *deferred = false;
  if (d.plain) {  // row-major operands of the layered path only
    if (d.kind == 0) {
      launch_time_table(prm + pl.te1_w, prm + pl.te1_b, prm + pl.te2_w, prm + pl.te2_b, d.time_dim, n_time, (float*)(pk + L.temb), s);
      launch_transpose_cast<P>(prm + pl.W0, H, d.time_dim, d.in_dim, d.act_flat, pk + L.W0tT, H, s);
    }
    launch_cast_pad<P>(prm + pl.W0, H, d.in_dim, d.in_dim, pk + L.W0, L.Kp0, s);
    for (int b = 0; b < d.n_blocks; ++b) {
      launch_cast_pad<P>(prm + pl.l1w[b], H, H, H, pk + L.W1[b], H, s);
      launch_transpose_cast<P>(prm + pl.l1w[b], H, H, H, 0, pk + L.W1T[b], H, s);
    }
    launch_cast_pad<P>(prm + pl.Wout, d.out_dim, H, H, pk + L.Wout, H, s);
    launch_transpose_cast<P>(prm + pl.Wout, d.out_dim, H, H, 0, pk + L.WoutT, L.Kpo, s);
    return check_launch();
  }
  const bool one_launch = fused_ok<P>(d) && g_pack_one && pack_net_supports(d.time_dim);
  if (d.kind == 0 && !one_launch)
    launch_time_table(prm + pl.te1_w, prm + pl.te1_b, prm + pl.te2_w, prm + pl.te2_b, d.time_dim, n_time,
                      (float*)(pk + L.temb), s);
  if (!fused_ok<P>(d)) {  // row-major operand copies of the layer-by-layer gemm_nt path (unused by the fused kernels)
    launch_cast_pad<P>(prm + pl.W0, H, d.in_dim, d.in_dim, pk + L.W0, L.Kp0, s);
    for (int b = 0; b < d.n_blocks; ++b) {
      launch_cast_pad<P>(prm + pl.l1w[b], H, H, H, pk + L.W1[b], H, s);
      launch_cast_pad<P>(prm + pl.l2w[b], H, H, H, pk + L.W2[b], H, s);
      launch_transpose_cast<P>(prm + pl.l1w[b], H, H, H, 0, pk + L.W1T[b], H, s);
      launch_transpose_cast<P>(prm + pl.l2w[b], H, H, H, 0, pk + L.W2T[b], H, s);
    }
    launch_cast_pad<P>(prm + pl.Wout, d.out_dim, H, H, pk + L.Wout, H, s);
    // WoutT[h][o] = Wout[o][h] : src rows = out_dim, cols = H  -> dst [H][Kpo]
    launch_transpose_cast<P>(prm + pl.Wout, d.out_dim, H, H, 0, pk + L.WoutT, L.Kpo, s);
  }
  // W0tT[j][h] = W0[h][act_flat + j]
  if (d.kind == 0 && !one_launch)
    launch_transpose_cast<P>(prm + pl.W0, H, d.time_dim, d.in_dim, d.act_flat, pk + L.W0tT, H, s);
  if (d.cond_hidden > 0) {
    launch_cast_pad<P>(prm + pl.c1w, d.cond_hidden, d.cond_dim, d.cond_dim, pk + L.Wc1, L.Kpc, s);
    launch_cast_pad<P>(prm + pl.c2w, d.cond_out, d.cond_hidden, d.cond_hidden, pk + L.Wc2, L.C1p, s);
    // Wc2T[c][e] = Wc2[e][c] -> [cond_hidden][Ep] ; W0eT[e][h] = W0[h][act_flat + td + e] -> [cond_out][H]
    launch_transpose_cast<P>(prm + pl.c2w, d.cond_out, d.cond_hidden, d.cond_hidden, 0, pk + L.Wc2T, L.Ep, s);
    launch_transpose_cast<P>(prm + pl.W0, H, d.cond_out, d.in_dim, d.act_flat + d.time_dim, pk + L.W0eT, H, s);
  }
  if (d.out_dim > 128) return check_launch();  // layered path only (fused_ok() is false: the row-major operands above are it)
  {
    const SamplerGeom g = sampler_geom<P>(d);
    const FusedGeom fg = fused_geom<P>(d);
    // forward stream [L0][b: l1, l2]... and backward stream, top down: [dh = d_out . Wout][b = nb-1..0: W2^T, W1^T]
    // ("feature f, contraction index k" of a transposed layer is W[k][f] = W[k*H + f]); all in one launch
    PackNet pn;
    memset(&pn, 0, sizeof(pn));
    PackStream& ps = pn.ps;
    ps.TPW = g.TPW;
    u32x4* fwd = (u32x4*)(pk + L.sstream);
    u32x4* bwd = (u32x4*)(pk + L.bstream);
    ps.layer[ps.n_layers++] = pack_layer(prm + pl.W0, d.in_dim, 1, d.in_dim, g.KS0, 0, fwd, g.total_pos);
    for (int b = 0; b < d.n_blocks; ++b) {
      ps.layer[ps.n_layers++] = pack_layer(prm + pl.l1w[b], H, 1, H, g.KSH, g.KS0 + 2 * b * g.KSH, fwd, g.total_pos);
      ps.layer[ps.n_layers++] = pack_layer(prm + pl.l2w[b], H, 1, H, g.KSH, g.KS0 + (2 * b + 1) * g.KSH, fwd, g.total_pos);
    }
    ps.layer[ps.n_layers++] = pack_layer(prm + pl.Wout, 1, H, d.out_dim, fg.KSB0, 0, bwd, fg.total_pos);
    for (int b = d.n_blocks - 1, pos = fg.KSB0; b >= 0; --b) {
      if (b == d.n_blocks - 1) {  // top block: the composite (Wout . W2)^T, laid out like the Wout^T layer
        float* wc = (float*)(pk + L.wcomp);
        ComposeJobs cq;
        cq.n = 1;
        memset(&cq.j[0], 0, sizeof(cq.j[0]));
        cq.j[0].Wout = prm + pl.Wout, cq.j[0].W2 = prm + pl.l2w[b], cq.j[0].b2 = prm + pl.l2b[b], cq.j[0].bout = prm + pl.bout;
        cq.j[0].Wc = wc, cq.j[0].cbias = (float*)(pk + L.cbias), cq.j[0].H = H, cq.j[0].out_dim = d.out_dim;
        if (d.n_blocks == 1) {
          cq.j[0].W0 = prm + pl.W0, cq.j[0].b0 = prm + pl.b0, cq.j[0].W0c = (float*)(pk + L.w0comp);
          cq.j[0].cbias2 = (float*)(pk + L.cbias2), cq.j[0].in_dim = d.in_dim, cq.j[0].Kp0s = L.Kp0s;
        }
        if (one_launch && defer_cj != nullptr)
          *defer_cj = cq.j[0];
        else
          launch_compose(cq, s);
        ps.layer[ps.n_layers++] = pack_layer(wc, 1, H, d.out_dim, fg.KSB0, pos, bwd, fg.total_pos);
        pos += fg.KSB0;
      } else {
        ps.layer[ps.n_layers++] = pack_layer(prm + pl.l2w[b], 1, H, H, g.KSH, pos, bwd, fg.total_pos);
        pos += g.KSH;
      }
      ps.layer[ps.n_layers++] = pack_layer(prm + pl.l1w[b], 1, H, H, g.KSH, pos, bwd, fg.total_pos);
      pos += g.KSH;
    }
    if (one_launch) {  // + out-layer stream, time-embedding table and W0tT, all in the same launch
      int maxks = 0;
      for (int l = 0; l < ps.n_layers; ++l) maxks = ps.layer[l].KS > maxks ? ps.layer[l].KS : maxks;
      pn.ps_x = SAMPLER_WAVES * maxks * ps.TPW;
      pn.Wout = prm + pl.Wout, pn.out_dim = d.out_dim, pn.H = H, pn.OT = g.OT, pn.CNT = g.CNT;
      pn.ostream = (u32x4*)(pk + L.ostream);
      if (d.n_blocks >= 1) pn.Wc = (const float*)(pk + L.wcomp), pn.ostream2 = (u32x4*)(pk + L.ostream2);
      if (d.n_blocks == 1)
        pn.W0c = (const float*)(pk + L.w0comp), pn.ostream0 = (u32x4*)(pk + L.ostream0), pn.Kp0s = L.Kp0s, pn.CNT0 = L.CNT0;
      if (d.kind == 0) {
        pn.te_w1 = prm + pl.te1_w, pn.te_b1 = prm + pl.te1_b, pn.te_w2 = prm + pl.te2_w, pn.te_b2 = prm + pl.te2_b;
        pn.td = d.time_dim, pn.n_time = n_time, pn.temb = (float*)(pk + L.temb);
        pn.tsrc = prm + pl.W0, pn.t_rows = H, pn.t_cols = d.time_dim, pn.t_lds = d.in_dim, pn.t_coff = d.act_flat;
        pn.t_ldd = H, pn.tdst = pk + L.W0tT;
      }
      if (defer_pn != nullptr && (d.n_blocks == 0 || defer_cj != nullptr)) {
        *defer_pn = pn;
        if (deferred) *deferred = true;
      } else {
        launch_pack_net<P>(pn, s);
      }
    } else {
      launch_pack_stream<P>(ps, s);
      launch_pack_out<P>(prm + pl.Wout, d.out_dim, H, g.OT, g.CNT, (u32x4*)(pk + L.ostream), s);
      if (d.n_blocks >= 1)
        launch_pack_out<P>((const float*)(pk + L.wcomp), d.out_dim, H, g.OT, g.CNT, (u32x4*)(pk + L.ostream2), s);
      if (d.n_blocks == 1)
        launch_pack_out<P>((const float*)(pk + L.w0comp), d.out_dim, L.Kp0s, g.OT, L.CNT0, (u32x4*)(pk + L.ostream0), s);
    }
  }
  return check_launch();
}

// ------------------------------------------------------------------------------------------------
// MLP forward / backward drivers on the GEMM path
// ------------------------------------------------------------------------------------------------
struct Carver {
  char* base;
  size_t off, cap;
  void* take(size_t bytes) {
    off = al256(off);
    void* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  }
};
// a *_workspace_bytes export: carve(c, P{}) runs one of the carve_* functions against a null base, in the call's precision
template <class F>
static int64_t ws_bytes(int prec, F carve) {
  Carver c{nullptr, 0, 0};
  return (int64_t)(prec == DPPO_PREC_F32 ? carve(c, F32{}) : carve(c, BF16{}));
}
// ... and its counterpart at the head of the driver: carve(c) runs the same carve_* function against the caller's buffer and fills
// the driver's workspace struct; a short buffer (need_ws: or none) is refused
template <class F>
static int carve_ws(void* ws, int64_t wsb, F carve, bool need_ws = false) {
  Carver c{(char*)ws, 0, (size_t)wsb};
  const size_t need = carve(c);
  if ((need_ws && !ws) || (int64_t)need > wsb) return fail(-1, "workspace too small: need %zu bytes, got %lld", need, (long long)wsb);
  return 0;
}
// the row count of a call: one int's worth
static int check_rows(int64_t N) {
  if (N < 1 || N > 0x7fffffff) return fail(-1, "N out of range");
  return 0;
}

// Which kernels one network's fused backward launches, and on which streams: decided once per network per call (its shape step
// at the head of carve_mlp, plan_route() right behind the carve) and only READ from there on -- by carve_mlp, the row builders' callers,
// mlp_forward and the backward's stages.  dppo_backward_route() exports it: every field is described at its DPPO_ROUTE_* bit
// in include/dppo_hip.h.
struct BwdRoute {
  bool fused, one_block, lowrank, merged;
  int onehot_col;  // column of the input rows where the one-hot of the row's denoising step starts, -1 = none
  bool dw0;
  int dw0_nhot;  // one-hot columns among the 32 of the in-kernel dW0
  bool dw0_round, need_aux, side_tail, tail_post, post_one;
  bool aux_side;  // (not exported) need_aux's pass runs on side stream TAIL_SIDE: the caller has one
};

template <class P>
struct MlpBufs {  // activations of one network for M rows
  void* in;                    // [M][Kp0] elem
  float* h[MAX_BLOCKS + 1];    // [M][H] f32 residual stream (h[0] = layer-0 output)
  void* a1[MAX_BLOCKS];        // act(h[b])
  void* z1[MAX_BLOCKS];        // l1 pre-activation (elem)
  void* a2[MAX_BLOCKS];        // act(z1)
  void* hpre[MAX_BLOCKS + 1];  // elem(h[b]); hpre[nb] = hE (out-layer input)
  void* hE;                    // elem(h[nb])
  float* out;                  // [M][ldout] f32
  int ldout;
  // backward
  void* d_out;  // [M][Kpo] elem
  void* dh;     // [M][H] elem
  void* dz1;    // [M][H] elem
  float* dtemb; // [M][tdp] f32 (actor)
  // cond_mlp (observation encoder) activations / gradients
  void* cin;     // [M][Kpc] elem : [obs | 0]
  void* ca;      // [M][C1p] act(z_c)
  void* cz;      // [M][C1p] z_c (Mish')
  void* d_enc;   // [M][Ep]
  void* d_cz;    // [M][C1p]
  void* dh_all[MAX_BLOCKS + 1];  // fused backward: dh[b] = d loss / d h_b, elem [M][H]
  void* dz1_all[MAX_BLOCKS];
  float* ln_stats;               // [nb][2][M][2] LayerNorm row statistics (training); a plain trunk uses [nb + 1][M][2] of it
  float* ln_part;                // plain trunk with LayerNorm, backward: [ln_bwd_blocks(M)][2][H] partial parameter sums
  float* ln_dz32[2];             // plain trunk with LayerNorm, backward, or null (carve_mlp leaves them null): [M][H] fp32 each; the data
                                 // GEMMs then hand LayerNorm's backward its input unrounded (ibrl.h)
  const void* dh0_final;         // where the last backward left d loss / d h_0
  void* w0T;                     // [cond_dim][H] elem: layer 0's observation columns, transposed (obs_grad)
  float* dobs;                   // [M][round_up(cond_dim, 16)]: obs_grad's GEMM output (the epilogue stores 16-column groups)
  float* tile_colsum;            // [(2nb+1)][tiles][H]
  int tiles;
  float* slab;  // split-M partial weight gradients: a pool, one sub-slab per pending weight-gradient GEMM
  size_t slab_used;   // floats handed out since the last flush
  SlabJobs slab_jobs; // reductions pending on the pool (flush_slabs)
  GemmTNGroup tn_group;  // weight-gradient GEMMs pending on the pool: launched together by flush_slabs
  BwdRoute route;
  // side streams to join into the flushing stream right behind the GEMM launch: the barrier packets (~10 us each even when
  // the event fired long ago) are then processed while the GEMMs run instead of at the end of the call
  hipStream_t join_s[2];
  int join_idx[2], n_join;
  float* part;  // column-sum / segment-sum partials
  float* lowrank;  // [out_dim][H] T = d_out^T . act(z1) of the top block (see lowrank_dw_kernel)
  float* lowrank_u;  // [out_dim][Kp0] U = d_out^T . x (merged-top networks: dWout is rebuilt from U and T, see PostReduce)
  double* post_counter;  // 8 zeroed bytes: arrival counter of post_reduce_kernel (zeroed by the row builder, left zero)
  unsigned* tail_counter;  // the 8 bytes right behind it (zeroed with it): arrival counter of tail_post_kernel's thin reductions
  size_t slab_floats, part_floats;
};

constexpr int REDUCE_BLOCKS = 256;
constexpr int POST_COUNTER_DOUBLES = 2;  // post_counter and tail_counter: one row-builder zero array

static bool lowrank_top(const dppo_net_desc& d, int64_t M);
template <class P>
static int plan_route(const dppo_net_desc& d, int64_t M, int Kft, int flags, MlpBufs<P>& B);

static int g_dbg = 0;  // tuning knob 8: timing experiments on the fused kernels (results are wrong while it is set)
template <class P>
static void carve_mlp(Carver& c, const dppo_net_desc& d, int64_t M, bool keep, bool bwd, MlpBufs<P>& B) {
  const size_t ES = P::ESIZE;
  const int H = d.hidden, nb = d.n_blocks;
  const int Kp0 = row_kp0(d), Kpo = round_up(d.out_dim, 64);
  memset(&B, 0, sizeof(B));
  // The route's shape step: what (network, rows, knobs) alone decide.  The per-tile column sums below are sized by it; the rest
  // (plan_route) needs what this carve produces.
  BwdRoute& R = B.route;
  R.onehot_col = -1, R.lowrank = lowrank_top(d, M);
  R.one_block = fused_bwd_one_block<P>(d) && d.out_dim <= 128 && R.lowrank;  // (its kernel writes no dh_nb: it needs the low-rank dW2)
  R.merged = fused_ok<P>(d) && fused_can_merge<P>(d);
  R.fused = fused_ok<P>(d) && M > 0 && fused_rows_per_tile<P>(d, R.one_block) > 0;
  B.in = c.take((size_t)M * Kp0 * ES);
  const int nh = keep ? nb + 1 : (nb > 0 ? 2 : 1);
  float* hbuf[MAX_BLOCKS + 1];
  for (int i = 0; i < nh; ++i) hbuf[i] = (float*)c.take((size_t)M * H * 4);
  for (int b = 0; b <= nb; ++b) B.h[b] = keep ? hbuf[b] : hbuf[b & 1];
  void* a1s = nullptr;
  void* a2s = nullptr;
  for (int b = 0; b < nb; ++b) {
    if (keep || b == 0) {
      a1s = c.take((size_t)M * H * ES);
      a2s = c.take((size_t)M * H * ES);
    } else if (d.plain) {
      // a plain layer reads a2[b - 1] and writes a2[b]: two buffers in turn, never one GEMM in place (its workgroups would read
      // rows that the others' column tiles are overwriting)
      a2s = b == 1 ? c.take((size_t)M * H * ES) : B.a2[b - 2];
    }
    B.a1[b] = a1s;
    B.a2[b] = a2s;
    B.z1[b] = keep ? c.take((size_t)M * H * ES) : nullptr;
  }
  if (d.cond_hidden > 0) {
    const int Kpc = round_up(d.cond_dim, 64), C1p = round_up(d.cond_hidden, 64), Ep = round_up(d.cond_out, 64);
    B.cin = c.take((size_t)M * Kpc * ES);
    B.ca = c.take((size_t)M * C1p * ES);
    B.cz = keep ? c.take((size_t)M * C1p * ES) : nullptr;
    if (bwd) {
      B.d_enc = c.take((size_t)M * Ep * ES);
      B.d_cz = c.take((size_t)M * C1p * ES);
    }
  }
  if (d.use_layernorm && keep) B.ln_stats = (float*)c.take((size_t)nb * 2 * M * 2 * 4);
  B.hE = c.take((size_t)M * H * ES);
  for (int b = 0; b <= nb; ++b) B.hpre[b] = b == nb ? B.hE : (keep ? c.take((size_t)M * H * ES) : nullptr);
  B.ldout = round_up(d.out_dim, 16);
  B.out = (float*)c.take((size_t)M * B.ldout * 4);
  if (bwd) {
    B.d_out = c.take((size_t)M * Kpo * ES);
    B.dh = c.take((size_t)M * H * ES);
    B.dz1 = c.take((size_t)M * H * ES);
    B.dh_all[nb] = B.dh;
    for (int b = 0; b < nb; ++b) {
      B.dh_all[b] = c.take((size_t)M * H * ES);
      B.dz1_all[b] = b == 0 ? B.dz1 : c.take((size_t)M * H * ES);
    }
    const int mt = d.plain || d.out_dim > 128 ? 0 : fused_rows_per_tile<P>(d, R.one_block);
    B.tiles = mt > 0 ? (int)((M + mt - 1) / mt) : 0;
    B.tile_colsum = (float*)c.take((size_t)(2 * nb + 2 + (d.use_layernorm ? 4 * nb : 0)) * (B.tiles > 0 ? B.tiles : 1) * H * 4);
    const int tdp = round_up(d.time_dim > 0 ? d.time_dim : 1, 16);
    B.dtemb = d.kind == 0 ? (float*)c.take((size_t)M * tdp * 4) : nullptr;
    // largest slab: H x max(H, Kp0) with up to 64 splits of a <=4-tile output, or 16+ splits of H x H
    const size_t tiles_hh = (size_t)((H + 127) / 128) * ((H + 127) / 128);
    size_t splits_hh = (512 + tiles_hh - 1) / tiles_hh;
    const size_t alt = (size_t)128 * H * (size_t)(Kp0 > 128 ? Kp0 : 128);  // thin outputs, up to 128 splits
    // a pool for all of one backward's GEMMs (2 per block + first and out layer), reduced together at the end
    B.slab_floats = (size_t)2 * (nb > 0 ? nb : 1) * splits_hh * (size_t)H * H + 2 * alt;
    B.slab = (float*)c.take(B.slab_floats * 4);
    B.slab_used = 0, B.slab_jobs.n = 0, B.tn_group.n = 0, B.n_join = 0;
    B.part_floats = (size_t)REDUCE_BLOCKS * (H > 1024 ? H : 1024);
    B.part = (float*)c.take(B.part_floats * 4);
    B.lowrank = (float*)c.take((size_t)round_up(d.out_dim, 16) * H * 4);
    B.lowrank_u = (float*)c.take((size_t)round_up(d.out_dim, 16) * Kp0 * 4);
    B.post_counter = (double*)c.take(POST_COUNTER_DOUBLES * 8);
    B.tail_counter = (unsigned*)(B.post_counter + 1);
    B.w0T = c.take((size_t)round_up(d.cond_dim > 0 ? d.cond_dim : 1, 16) * H * ES);
    B.dobs = (float*)c.take((size_t)M * round_up(d.cond_dim > 0 ? d.cond_dim : 1, 16) * 4);
    if (d.plain && d.use_layernorm) B.ln_part = (float*)c.take((size_t)ln_bwd_blocks(M) * 2 * H * 4);
    // the route of a caller that has nothing to add (no denoising steps, no zeroed counters, no side stream); the entry points
    // that do (BC, denoise-MSE, PPO) plan again with their own inputs before they build their rows
    plan_route<P>(d, M, 0, 0, B);
  }
}

static void fill_bias_off(const dppo_net_desc& d, const ParamLayout& pl, int* off) {
  off[0] = (int)pl.b0;
  for (int b = 0; b < d.n_blocks; ++b) off[1 + 2 * b] = (int)pl.l1b[b], off[2 + 2 * b] = (int)pl.l2b[b];
  off[1 + 2 * d.n_blocks] = (int)pl.bout;
}
static void fill_ln_off(const dppo_net_desc& d, const ParamLayout& pl, int* off) {
  for (int b = 0; b < d.n_blocks; ++b)
    off[4 * b] = (int)pl.n1w[b], off[4 * b + 1] = (int)pl.n1b[b], off[4 * b + 2] = (int)pl.n2w[b], off[4 * b + 3] = (int)pl.n2b[b];
}

// cond_mlp (mlp_diffusion.py:201-207,240-241): enc = Linear2(act(Linear1(obs))), written as elem straight into the
// encoder columns [act_flat + time_dim, +cond_out) of the trunk's input rows `in` (ld Kp0).  cin: [M][Kpc] elem obs.
template <class P>
static void cond_encode(const dppo_net_desc& d, const float* prm, const char* pk, const PackLayout& L, int64_t M,
                        const void* cin, MlpBufs<P>& B, void* in, float* enc_f32, int ld_enc, bool keep, hipStream_t s) {
  const ParamLayout pl = param_layout(d);
  GemmNT g;
  memset(&g, 0, sizeof(g));
  g.M = (int)M, g.N = d.cond_hidden, g.Kp = L.Kpc, g.ldx = L.Kpc, g.ldw = L.Kpc, g.ldo = L.C1p, g.act = d.act;
  g.X = cin, g.W = pk + L.Wc1, g.bias = prm + pl.c1b, g.out_act = B.ca, g.out_pre = keep ? B.cz : nullptr;
  launch_gemm_nt<P>(g, s);
  if (L.C1p > round_up(d.cond_hidden, 16)) launch_zero_cols<P>(B.ca, (int)M, round_up(d.cond_hidden, 16), L.C1p, L.C1p, s);
  memset(&g, 0, sizeof(g));
  g.M = (int)M, g.N = d.cond_out, g.Kp = L.C1p, g.ldx = L.C1p, g.ldw = L.C1p;
  g.X = B.ca, g.W = pk + L.Wc2, g.bias = prm + pl.c2b;
  if (in != nullptr) g.out_pre = (char*)in + (size_t)(d.act_flat + d.time_dim) * P::ESIZE, g.ldo = L.Kp0;
  if (enc_f32 != nullptr) g.out_f32 = enc_f32, g.ldo32 = ld_enc;
  launch_gemm_nt<P>(g, s);
}

template <class P>
static void mlp_forward(const dppo_net_desc& d, const float* prm, const char* pk, const PackLayout& L, int64_t M,
                        MlpBufs<P>& B, bool keep, hipStream_t s, const LossArgs* fuse_loss = nullptr, bool layered = false,
                        const dppo_dropout* drop = nullptr) {
  // fuse_loss: the policy half of the PPO loss in the forward kernel's epilogue (fuse_loss_ok() held: the merged fused kernel runs)
  // layered: the GEMM path even where the fused kernels cover the shape (the caller's backward reads the layered path's
  // derivative sources: dql_impl)
  // drop: dropout behind every hidden layer of a plain trunk without LayerNorm (ibrl.h; the entry checked the descriptor); null, or
  // p = 0 without a given mask, is the path without it, launch for launch
  const ParamLayout pl = param_layout(d);
  const int H = d.hidden, nb = d.n_blocks;
  if (fuse_loss != nullptr && !(fused_ok<P>(d) && B.route.merged)) {
    g_fused_fault = -8;  // (fuse_loss_ok() and this function disagree)
    return;
  }
  if (!layered && fused_ok<P>(d)) {
    FusedFwdArgs f;
    memset(&f, 0, sizeof(f));
    f.wstream = (const u32x4*)(pk + L.sstream), f.ostream = (const u32x4*)(pk + L.ostream), f.params = prm;
    fill_bias_off(d, pl, f.bias_off);
    f.in = B.in, f.ld_in = L.Kp0, f.M = (int)M, f.Kp0 = sampler_geom<P>(d).Kp0, f.nb = nb, f.act = d.act;
    f.out_dim = d.out_dim, f.out = B.out, f.ldout = B.ldout, f.in_valid = d.in_dim;
    f.use_ln = d.use_layernorm;
    if (d.use_layernorm) fill_ln_off(d, pl, f.ln_off);
    if (keep) {
      for (int b = 0; b < nb; ++b) {
        f.a1[b] = B.a1[b], f.a2[b] = B.a2[b];
        // derivative sources: Mish' itself, ReLU sign words, or (LayerNorm) the pre-LayerNorm tensors
        f.z1[b] = B.z1[b], f.hpre[b] = B.hpre[b];
      }
      f.hpre[nb] = B.hE;
      f.ln_stats = d.use_layernorm ? B.ln_stats : nullptr;
    }
    if (B.route.merged) {  // the block's second layer folded into the out layer: h_nb is never formed (fused_forward_merged_kernel)
      f.merge_top = 1, f.ks0v = (d.in_dim + P::KB - 1) / P::KB, f.hpre[nb] = nullptr;
      if (g_dbg & 64) f.hpre[0] = nullptr;   // timing experiments: the forward does not store act'(h_0) ...
      if (g_dbg & 128) f.a2[0] = nullptr;    // ... / act(z1)
      if (g_dbg & 256) f.z1[0] = nullptr;    // ... / act'(z1)
      f.ostream0 = (const u32x4*)(pk + L.ostream0), f.ostream2 = (const u32x4*)(pk + L.ostream2);
      f.cbias2 = (const float*)(pk + L.cbias2);
    }
    g_fused_fault = launch_fused_forward<P>(d, f, s, fuse_loss);
    return;
  }
  if (d.plain) {  // x -> act(W0 x) -> act(W_b .) ... -> Wout .   (pre-activations kept for the backward: hpre[0], z1[b])
    GemmNT q;
    memset(&q, 0, sizeof(q));
    q.M = (int)M, q.X = B.in, q.ldx = L.Kp0, q.W = pk + L.W0, q.ldw = L.Kp0, q.Kp = L.Kp0, q.N = H, q.bias = prm + pl.b0;
    q.ldo = H, q.act = d.act, q.out_act = B.a1[0], q.out_pre = keep ? B.hpre[0] : nullptr;
    // LayerNorm (rlpd.h): the GEMM leaves its bias-added row in fp32 (B.h[.], carved for every trunk and unused by a plain one
    // without LayerNorm), the row kernel writes act(z) and, kept, z where the GEMM's own epilogue would have
    LnRows ln;
    memset(&ln, 0, sizeof(ln));
    ln.M = M, ln.H = H, ln.act = d.act, ln.ldx = H, ln.ldo = H;
    if (d.use_layernorm) {
      ln.x = B.h[0], ln.gamma = prm + pl.n0w, ln.beta = prm + pl.n0b, ln.out_act = q.out_act, ln.out_z = q.out_pre;
      ln.stats = keep ? B.ln_stats : nullptr;
      q.out_act = q.out_pre = nullptr, q.out_f32 = B.h[0], q.ldo32 = H;
    }
    // dropout (ibrl.h) takes the same route: the unrounded row in B.h[.], then the row kernel in the epilogue's place
    const bool dropping = drop != nullptr && !d.use_layernorm && (drop->p > 0.f || drop->mask != nullptr);
    DropRows dr;
    memset(&dr, 0, sizeof(dr));
    if (dropping) {
      dr.M = M, dr.H = H, dr.act = d.act, dr.ldx = H, dr.ldo = H, dr.p = drop->p, dr.scale = 1.f / (1.f - drop->p);
      dr.k0 = drop->seed_lo, dr.k1 = drop->seed_hi, dr.mask = drop->mask, dr.mask_out = drop->mask_out;
      dr.x = B.h[0], dr.layer = 0, dr.out_act = q.out_act, dr.out_z = q.out_pre;
      q.out_act = q.out_pre = nullptr, q.out_f32 = B.h[0], q.ldo32 = H;
    }
    launch_gemm_nt<P>(q, s);
    if (d.use_layernorm) launch_ln_rows<P>(ln, s);
    if (dropping) launch_drop_rows<P>(dr, s);
    for (int b = 0; b < nb; ++b) {
      memset(&q, 0, sizeof(q));
      q.M = (int)M, q.N = H, q.Kp = H, q.ldx = H, q.ldw = H, q.ldo = H, q.act = d.act;
      q.X = b == 0 ? B.a1[0] : B.a2[b - 1], q.W = pk + L.W1[b], q.bias = prm + pl.l1b[b];
      q.out_pre = keep ? B.z1[b] : nullptr, q.out_act = B.a2[b];
      if (d.use_layernorm) {
        ln.x = B.h[b + 1], ln.gamma = prm + pl.n1w[b], ln.beta = prm + pl.n1b[b], ln.out_act = q.out_act, ln.out_z = q.out_pre;
        ln.stats = keep ? B.ln_stats + (size_t)(b + 1) * M * 2 : nullptr;
        q.out_act = q.out_pre = nullptr, q.out_f32 = B.h[b + 1], q.ldo32 = H;
      }
      if (dropping) {
        dr.x = B.h[b + 1], dr.layer = b + 1, dr.out_act = q.out_act, dr.out_z = q.out_pre;
        q.out_act = q.out_pre = nullptr, q.out_f32 = B.h[b + 1], q.ldo32 = H;
      }
      launch_gemm_nt<P>(q, s);
      if (d.use_layernorm) launch_ln_rows<P>(ln, s);
      if (dropping) launch_drop_rows<P>(dr, s);
    }
    memset(&q, 0, sizeof(q));
    q.M = (int)M, q.N = d.out_dim, q.Kp = H, q.ldx = H, q.ldw = H;
    q.X = B.a2[nb - 1], q.W = pk + L.Wout, q.bias = prm + pl.bout, q.out_f32 = B.out, q.ldo32 = B.ldout;
    launch_gemm_nt<P>(q, s);
    return;
  }
  GemmNT g;
  memset(&g, 0, sizeof(g));
  g.M = (int)M;
  // layer 0
  g.X = B.in, g.ldx = L.Kp0, g.W = pk + L.W0, g.ldw = L.Kp0, g.Kp = L.Kp0, g.N = H, g.bias = prm + pl.b0;
  g.out_f32 = B.h[0], g.ldo32 = H, g.ldo = H, g.act = d.act;
  g.out_act = nb > 0 ? B.a1[0] : nullptr;
  g.out_pre = nb > 0 ? nullptr : B.hE;
  launch_gemm_nt<P>(g, s);
  for (int b = 0; b < nb; ++b) {
    memset(&g, 0, sizeof(g));
    g.M = (int)M, g.N = H, g.Kp = H, g.ldx = H, g.ldw = H, g.ldo = H, g.ldo32 = H, g.act = d.act;
    g.X = B.a1[b], g.W = pk + L.W1[b], g.bias = prm + pl.l1b[b];
    g.out_pre = keep ? B.z1[b] : nullptr, g.out_act = B.a2[b];
    launch_gemm_nt<P>(g, s);
    g.X = B.a2[b], g.W = pk + L.W2[b], g.bias = prm + pl.l2b[b];
    g.res = B.h[b], g.ldres = H;
    g.out_f32 = B.h[b + 1];
    g.out_act = b + 1 < nb ? B.a1[b + 1] : nullptr;
    g.out_pre = b + 1 < nb ? nullptr : B.hE;
    launch_gemm_nt<P>(g, s);
  }
  memset(&g, 0, sizeof(g));
  g.M = (int)M, g.N = d.out_dim, g.Kp = H, g.ldx = H, g.ldw = H;
  g.X = B.hE, g.W = pk + L.Wout, g.bias = prm + pl.bout, g.out_f32 = B.out, g.ldo32 = B.ldout;
  launch_gemm_nt<P>(g, s);
}

// ---- side streams ----------------------------------------------------------------------------------------
// Independent parts of one call run on side streams so that their kernels fill each other's gaps (the persistent
// row-tile kernels leave CUs idle in their last round of tiles; the small reductions are latency-bound).  Fork / join
// through events: legal under stream capture too.  Tuning knob 2 turns it off (one stream, for per-kernel timing).
//   side 0: the critic pipeline of a PPO update;  side 1: the bias / time-embedding gradient tail of the actor
static int g_overlap = 1;
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  bool ok = false;
};
static SideStream* side_stream(int idx) {
  static SideStream tab[16][3];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  SideStream& t = tab[dev][idx];
  if (!t.ok) {
    if (hipStreamCreateWithFlags(&t.s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&t.fork, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&t.join, hipEventDisableTiming) != hipSuccess) return nullptr;
    t.ok = true;
  }
  return &t;
}
static bool side_stream_on(int idx) { return (((g_overlap == 1 ? 7 : g_overlap >> 1) >> idx) & 1) != 0; }
static hipStream_t fork_side(hipStream_t main, int idx = 0) {  // returns the stream the independent part should use
  // g_overlap: 0 = none, 1 = every side stream, other values = bit mask over the side-stream indices, shifted by one
  // (e.g. 2 = the critic pipeline's only)
  SideStream* t = side_stream_on(idx) ? side_stream(idx) : nullptr;
  if (t == nullptr) return main;
  (void)hipEventRecord(t->fork, main);
  (void)hipStreamWaitEvent(t->s, t->fork, 0);
  return t->s;
}
static void join_side(hipStream_t main, hipStream_t sidestream, int idx = 0) {
  if (sidestream == main) return;
  SideStream* t = side_stream(idx);
  (void)hipEventRecord(t->join, sidestream);
  (void)hipStreamWaitEvent(main, t->join, 0);
}

static int g_post_one = 1;         // tuning knob 18: low-rank dW2 + time-embedding gradient in one launch after the slab reduce
static int g_merge_top = 1;        // tuning knob 17: sampler merges the top block's second layer into the out layer
static int g_lowrank_top = 1;      // tuning knob 16: top block's dW2 from the rank-out_dim factorisation (no H x H GEMM, no dh store)
static int g_early_join = 1;       // tuning knob 14: side streams joined right behind the weight-gradient GEMM launch
static int g_tn_group = 1;         // tuning knob 12: one launch for all weight-gradient GEMMs of a backward pass
static int g_tn_target = 256;      // tuning knob 3: workgroups a weight-gradient GEMM aims for (tiles x row splits)
static int g_tn_max_splits = 128;  // tuning knob 4: cap on its row splits (each split costs one fp32 slab of the output)
// (the out_dim-deep product costs H^2 out_dim scalar MACs against the M H^2 MFMA MACs it saves: on for M >= 100 out_dim;
// measured a loss at out_dim = 112, M = 10,000 -- ratio 89 -- and wins at out_dim 56, M = 7,500 -- ratio 134, BASELINE
// configs[2], where it also admits the one-block backward; tuning knob 30 moves the ratio)
static int g_lowrank_ratio = 100;
static bool lowrank_top(const dppo_net_desc& d, int64_t M) {
  return g_lowrank_top && d.n_blocks >= 1 && M >= (int64_t)g_lowrank_ratio * d.out_dim;
}
static int g_mom_rider = 0;  // tuning knob 36: the minibatch's advantage moments as riders of the row builder (1: always, 2: never) or a launch
                              // of their own.  0 (default): riders for minibatches of at most MOM_RIDER_MAX_N samples -- at N = 50,000 the
                              // launch already hides under the critic's forward on the side stream (the riders save 3.5 us only in the
                              // serial order, profiles/r03_moments_rider_ab.txt); at BASELINE configs[2]'s 7,500 the step is a chain of
                              // launches and one fewer is 0.186 -> 0.180 ms
constexpr int64_t MOM_RIDER_MAX_N = 16384;
static bool mom_rider_on(int64_t N, bool has_gmom) { return !has_gmom && (g_mom_rider == 1 || (g_mom_rider == 0 && N <= MOM_RIDER_MAX_N)); }
// Time-embedding gradient through the first layer's weight-gradient GEMM: with a one-hot of the row's denoising step k in
// the K padding of the input rows, dW0's extra columns are S[h][k] = sum over the rows of step k of dh0[row][h], and
// d loss / d temb[k] = W0[:, temb columns]^T S[:, k] -- no second pass over dh0, no segmented reduction (tuning knob 11).
static int g_temb_onehot = 1;
// In-kernel first-layer weight gradient (tuning knob 37; fused.h, FusedBwdArgs::dw0_slab).  dh_0 -- a third of the bytes the
// weight-gradient GEMMs read, for a 512 x 64 output -- is then neither stored nor read back: the one-block backward multiplies each
// tile of it with the tile's input rows while both are on chip and keeps the partial product in LDS.  The 64 KB that has room for
// is [H][32]: the network's informative input columns must fit 32.  A denoiser's rows are [x_k | temb(t_k) | obs | one-hot(k)]:
// the temb columns are a function of k alone (their gradient is rebuilt from the one-hot sums, PostReduce::dW0t; the kernel
// skips them when it reads the row tile: act_flat and time_dim must be multiples of 4), and of the Kft one-hot columns the last
// may be left out (every row carries exactly one: PostReduce::S_rest, with the bias gradient taken of the rounded dh_0) --
// hopper: 12 + 11 + 9 = 32.  (What else it needs: plan_route().)
static int g_dw0 = 1;
// Tuning knob 38: with the in-kernel dW0 everything the time-embedding gradient needs -- the one-hot sums, the first layer's bias
// gradient, then G = W0_temb^T . S and the time MLP's backward (a chain of dependent steps: 11 of post_reduce's 16 us) -- comes out
// of the backward KERNEL, not out of the weight-gradient GEMMs: that reduction and that part of post_reduce run on a side stream
// under the GEMM launch, with the bias sums and the loss statistics, and only the GEMMs' own slabs, the low-rank dW2 and dWout
// stay behind the GEMMs on the caller's stream.
static int g_side_tail = 1;
// Tuning knob 41: with knob 38, what is left behind the actor's GEMMs -- their slab reductions, then the low-rank dW2 / dWout / db2,
// which read only the two THIN products -- is ONE launch (tail_post_kernel: the thin products' reduce blocks first, the dependent
// blocks poll their arrival, the big slabs are reduced beside them) instead of two.
static int g_tail_post = 1;
// The rest of the route: what needs the carve (tiles, part_floats, slab_floats), the denoising steps and the caller.  flags
// (DPPO_ROUTE_IN_*): the caller's row builder zeroes post_counter and tail_counter in this call; somebody asks for
// d loss / d observation; the tail may use side stream TAIL_SIDE.  Runs before the rows are built: they carry the one-hot columns.
template <class P>
static int plan_route(const dppo_net_desc& d, int64_t M, int Kft, int flags, MlpBufs<P>& B) {
  BwdRoute& R = B.route;
  const bool zeroed = flags & DPPO_ROUTE_IN_ZEROED, wants_dobs = flags & DPPO_ROUTE_IN_DOBS;
  const int Kp0 = row_kp0(d);
  const bool side = flags & DPPO_ROUTE_IN_SIDE;
  // (the encoder's epilogue zero-fills up to a multiple of 16 columns; S[H][Kft] and G[td][Kft] live in B.part)
  const bool oh = g_temb_onehot && d.kind == 0 && fused_ok<P>(d) && Kft >= 1 && !(d.cond_out > 0 && d.cond_out % 16) &&
                  Kp0 - d.in_dim >= Kft && (size_t)(d.hidden + d.time_dim) * Kft <= B.part_floats;
  R.onehot_col = oh ? d.in_dim : -1;
  const int room = 32 - (d.kind == 0 ? d.act_flat + d.cond_dim : d.in_dim);  // one-hot columns that fit behind the data columns
  const int nhot = d.kind != 0 ? 0 : (room >= Kft ? Kft : room);
  R.dw0 = g_dw0 && P::ESIZE == 2 && zeroed && !wants_dobs && d.cond_hidden <= 0 && g_tn_group && g_post_one && R.fused &&
          R.one_block && fused_dw0_shape(d) && Kp0 >= 64 &&
          (size_t)fused_bwd_one_grid<P>(d, M) * d.hidden * 32 <= B.slab_floats / 2;  // a slab per workgroup in the pool
  if (d.kind == 0)
    R.dw0 = R.dw0 && oh && d.in_dim == d.act_flat + d.time_dim + d.cond_dim && d.act_flat % 4 == 0 && d.time_dim % 4 == 0 &&
            32 + d.time_dim <= 64 && nhot >= Kft - 1;
  else
    R.dw0 = R.dw0 && d.in_dim <= 32;
  if (R.dw0 && (g_dbg & 33))
    return fail(-1, "tuning knob 8, bits 0 and 5 (values 1 and 32: no dh_0 store) cannot run with the in-kernel dW0: set knob 37 to 0 first");
  R.dw0_nhot = R.dw0 ? nhot : 0;
  R.dw0_round = R.dw0 && d.kind == 0 && nhot < Kft;  // (the last one-hot column is rebuilt from the bias gradient)
  R.need_aux = d.kind == 0 && !oh;
  R.aux_side = R.need_aux && side;
  R.side_tail = R.dw0 && d.kind == 0 && side && g_side_tail && g_early_join && zeroed && !(g_dbg & 28);
  R.tail_post = R.side_tail && g_tail_post;  // (dw0 implies the one-block backward: there is always a post-reduce part)
  // its arrival counter (zeroed by the row builder) is only needed by the time-embedding part
  R.post_one = g_post_one && (!oh || zeroed) && (R.lowrank || oh || R.merged || R.one_block);
  return 0;
}
template <class P>
static void flush_slabs(MlpBufs<P>& B, hipStream_t s, const SlotOuts* slots = nullptr, int slot_width = 0,
                        const LossArgs* fin = nullptr, bool defer_reduce = false) {
  // defer_reduce: launch the GEMMs (and join the side streams) but leave the slab jobs to the caller (tail_post_kernel)
  // slots / fin: the fused backward's per-tile column sums and the loss statistics ride in the reduction launch (see
  // tail_reduce_kernel)
  if (B.tn_group.n > 0) {
    GemmTNGroup& gr = B.tn_group;
    gemm_tn_group_order(gr);  // longest row ranges first, base[]
    launch_gemm_tn_group<P>(gr, s);
    gr.n = 0;
  }
  // One wait on the caller's stream however many side streams there are: the earlier ones are joined into the LAST one (their
  // waits cost nothing there) and only that one into s -- a satisfied event wait is still a barrier packet between the GEMM
  // launch and the reduction behind it, ~6 us each on the update's critical path (profiles/r03_dw0_ab.txt, knob 38).
  for (int i = 0; i + 1 < B.n_join; ++i) join_side(B.join_s[B.n_join - 1], B.join_s[i], B.join_idx[i]);
  if (B.n_join > 0) join_side(s, B.join_s[B.n_join - 1], B.join_idx[B.n_join - 1]);
  B.n_join = 0;
  if (defer_reduce) return;
  if (slots != nullptr || fin != nullptr) {
    TailReduce t;
    memset(&t, 0, sizeof(t));
    t.jobs = B.slab_jobs;
    if (slots != nullptr) t.colsum = B.tile_colsum, t.tiles = B.tiles, t.width = slot_width, t.slots = *slots;
    if (g_dbg & 4) t.jobs.n = 0;          // timing experiments (knob 8; results are wrong while set): no slab reductions,
    if (g_dbg & 8) t.slots.n_slots = 0;   // no bias sums,
    if (g_dbg & 16) fin = nullptr;        // no loss statistics
    launch_tail_reduce(t, fin, s);
  } else {
    launch_slab_reduce_batch(B.slab_jobs, s);
  }
  B.slab_jobs.n = 0, B.slab_used = 0;
}
// gw[N1][N2] (ld ldgw) = A[M][N1]^T . B[M][N2].  A thin N1 (the out layer) is computed transposed, B^T . A, so that the
// 512 x 64 block shape of gemm_tn covers it in one output tile; the slab reduce transposes back.
template <class P>
static void weight_grad(const void* A, int lda, int N1, const void* Bm, int ldb, int N2, int64_t M, MlpBufs<P>& B,
                        float* gw, int ldgw, hipStream_t s, bool defer = false, int n2a = -1, float* gw2 = nullptr,
                        int ldgw2 = 0) {  // n2a >= 0: columns [n2a, N2) of the result go to gw2 instead (never with a thin N1)
  const bool swap = N1 <= 64 && N2 > 64;
  if (swap) {
    const void* tp = A;
    A = Bm, Bm = tp;
    int ti = lda;
    lda = ldb, ldb = ti;
    ti = N1, N1 = N2, N2 = ti;
  }
  const bool group = defer && g_tn_group;  // launched with the caller's other GEMMs, 128 x 128 tiles throughout
  const bool thin = !group && gemm_tn_thin(N1, N2);
  const size_t N1s = (size_t)round_up(N1, 4);  // (every sub-slab of the pool starts on a 16-byte boundary)
  const size_t tiles = thin ? (size_t)((N1 + 511) / 512) : (size_t)((N1 + 127) / 128) * ((N2 + 127) / 128);
  int64_t splits = (g_tn_target + tiles - 1) / tiles;
  const int64_t max_splits = (M + 63) / 64;
  if (splits > max_splits) splits = max_splits;
  if (splits > g_tn_max_splits) splits = g_tn_max_splits;
  if ((size_t)splits * N1s * N2 > B.slab_floats - B.slab_used || B.slab_jobs.n + 2 > MAX_SLAB_JOBS ||
      B.tn_group.n >= MAX_TN_JOBS)
    flush_slabs(B, s);
  while (splits > 1 && (size_t)splits * N1s * N2 > B.slab_floats) --splits;
  if (splits >= 8) splits = splits / 8 * 8;  // a multiple of the XCD count keeps one split's tiles on one XCD
  int64_t rps = (M + splits - 1) / splits;
  rps = (rps + 63) / 64 * 64;
  const int64_t need = (M + rps - 1) / rps;
  if (need < splits) splits = need >= 8 ? (need + 7) / 8 * 8 : need;  // surplus splits see no rows and store zeros
  GemmTN t;
  memset(&t, 0, sizeof(t));
  t.A = A, t.B = Bm, t.M = (int)M, t.N1 = N1, t.N2 = N2, t.lda = lda, t.ldb = ldb;
  float* sub = B.slab + B.slab_used;
  B.slab_used += (size_t)splits * N1s * N2;
  t.slab = sub, t.ldc = N2, t.splits = (int)splits, t.rows_per_split = (int)rps;
  if (group)
    B.tn_group.j[B.tn_group.n++] = t;
  else
    launch_gemm_tn<P>(t, s);
  SlabJob& j = B.slab_jobs.j[B.slab_jobs.n++];
  j.slab = sub, j.out = gw, j.splits = (int)splits, j.rows = N1, j.cols = N2, j.lds = N2, j.ldo = ldgw, j.transpose = swap ? 1 : 0;
  j.c0 = 0, j.wide = 0;
  if (n2a >= 0 && !swap) {
    j.cols = n2a;
    SlabJob& j2 = B.slab_jobs.j[B.slab_jobs.n++];
    j2 = j;
    j2.out = gw2, j2.ldo = ldgw2, j2.c0 = n2a, j2.cols = N2 - n2a;
  }
  if (!defer) flush_slabs(B, s);  // deferred: the caller flushes once after its last GEMM (same stream)
}

// d temb = dh0 . W0[:, temb columns]; summed per fine-tuned step; back through the tiny time MLP
template <class P>
static void time_embedding_grad(const dppo_net_desc& d, const float* prm, const char* pk, const PackLayout& L, int64_t M,
                                MlpBufs<P>& B, const void* dh0, float* grad, const int32_t* krow, const dppo_step* ksteps,
                                int Kft, hipStream_t s) {
  const ParamLayout pl = param_layout(d);
  const int H = d.hidden, td = d.time_dim;
  GemmNT g;
  memset(&g, 0, sizeof(g));
  g.M = (int)M, g.N = td, g.Kp = H, g.ldx = H, g.ldw = H;
  g.X = dh0, g.W = pk + L.W0tT, g.out_f32 = B.dtemb, g.ldo32 = L.tdp;
  launch_gemm_nt<P>(g, s);
  int sblocks = (int)(B.part_floats / ((size_t)Kft * td)) - 1;  // partial[sblocks][Kft*td] + G[Kft*td] must fit
  sblocks = sblocks > REDUCE_BLOCKS ? REDUCE_BLOCKS : (sblocks < 1 ? 1 : sblocks);
  launch_temb_segsum(B.dtemb, L.tdp, krow, M, Kft, td, B.part, sblocks, s);
  float* G = B.part + (size_t)sblocks * Kft * td;
  launch_slab_reduce(B.part, sblocks, (size_t)Kft * td, G, 1.f, s);
  launch_time_backward(prm + pl.te1_w, prm + pl.te1_b, prm + pl.te2_w, G, ksteps, Kft, td, grad + pl.te1_w,
                       grad + pl.te1_b, grad + pl.te2_w, grad + pl.te2_b, s);
}

// gradients of the encoder from dh0 (= d loss / d h_0 of the trunk)
template <class P>
static void cond_backward(const dppo_net_desc& d, const float* prm, const char* pk, const PackLayout& L, int64_t M,
                          MlpBufs<P>& B, const void* dh0, const void* cin, float* grad, hipStream_t s) {
  const ParamLayout pl = param_layout(d);
  const int H = d.hidden;
  GemmNT g;
  memset(&g, 0, sizeof(g));  // d_enc = dh0 . W0[:, enc columns]
  g.M = (int)M, g.N = d.cond_out, g.Kp = H, g.ldx = H, g.ldw = H, g.ldo = L.Ep;
  g.X = dh0, g.W = pk + L.W0eT, g.out_pre = B.d_enc;
  launch_gemm_nt<P>(g, s);
  if (L.Ep > round_up(d.cond_out, 16))  // columns the epilogue does not store must be zero: they are the next GEMM's K padding
    launch_zero_cols<P>(B.d_enc, (int)M, round_up(d.cond_out, 16), L.Ep, L.Ep, s);
  weight_grad<P>(B.d_enc, L.Ep, d.cond_out, B.ca, L.C1p, d.cond_hidden, M, B, grad + pl.c2w, d.cond_hidden, s);
  launch_colsum<P>(B.d_enc, (int)M, d.cond_out, L.Ep, B.part, REDUCE_BLOCKS, grad + pl.c2b, 1.f, s);
  memset(&g, 0, sizeof(g));  // d_zc = (d_enc . Wc2) * act'(z_c)
  g.M = (int)M, g.N = d.cond_hidden, g.Kp = L.Ep, g.ldx = L.Ep, g.ldw = L.Ep, g.ldo = L.C1p;
  g.X = B.d_enc, g.W = pk + L.Wc2T, g.out_pre = B.d_cz, g.dsrc_kind = 2, g.dsrc_ld = L.C1p, g.dact = d.act;
  g.dsrc = d.act == DPPO_ACT_RELU ? B.ca : B.cz;
  launch_gemm_nt<P>(g, s);
  weight_grad<P>(B.d_cz, L.C1p, d.cond_hidden, cin, L.Kpc, d.cond_dim, M, B, grad + pl.c1w, d.cond_dim, s);
  launch_colsum<P>(B.d_cz, (int)M, d.cond_hidden, L.C1p, B.part, REDUCE_BLOCKS, grad + pl.c1b, 1.f, s);
}

// ---- the fused backward, stage by stage.  Every stage READS B.route; none decides routing. ---------------------------
constexpr int TAIL_SIDE = 1;  // side-stream index of the actor's bias / time-embedding gradient tail
// one kernel produces every data gradient (dh[nb..0], dz1[..]) and their per-tile column sums; returns its refusal code
template <class P>
static int launch_backward_kernel(const dppo_net_desc& d, const float* prm, const char* pk, const PackLayout& L, int64_t M,
                                  MlpBufs<P>& B, hipStream_t s, float*& dw0_slab) {
  const BwdRoute& R = B.route;
  const ParamLayout pl = param_layout(d);
  const int H = d.hidden, nb = d.n_blocks;
  FusedBwdArgs f;
  memset(&f, 0, sizeof(f));
  f.bstream = (const u32x4*)(pk + L.bstream), f.d_out = B.d_out, f.ld_dout = L.Kpo, f.M = (int)M, f.KpB0 = fused_geom<P>(d).KpB0;
  f.nb = nb, f.act = d.act, f.colsum = B.tile_colsum, f.out_valid = d.out_dim;
  f.dout_slot = 2 * nb + 1 + (d.use_layernorm ? 4 * nb : 0);
  f.params = prm, f.use_ln = d.use_layernorm, f.ln_stats = B.ln_stats;
  if (d.use_layernorm) fill_ln_off(d, pl, f.ln_off);
  for (int b = 0; b < nb; ++b)  // the forward left the derivative sources in z1 / hpre (see emit())
    f.m1[b] = B.z1[b], f.m0[b] = B.hpre[b], f.dz1[b] = B.dz1_all[b];
  for (int b = 0; b <= nb; ++b) f.dh[b] = B.dh_all[b];
  if (R.lowrank) f.dh[nb] = nullptr;  // only dW2 of the top block read it: see lowrank_dw_kernel
  f.one_block = R.one_block ? 1 : 0;
  if (g_dbg & 1)  // timing experiment: no gradient stores (the weight-gradient GEMMs then read stale buffers)
    for (int b = 0; b <= nb; ++b) f.dh[b] = nullptr, f.dz1[b < nb ? b : 0] = nullptr;
  if (g_dbg & 32) f.dh[0] = nullptr;  // timing experiment: dh_0 is not stored (bound of the in-kernel dW0)
  if (g_dbg & 2)  // timing experiment: no derivative-source fetch
    for (int b = 0; b < nb; ++b) f.m1[b] = f.m0[b] = nullptr;
  dw0_slab = nullptr;
  if (R.dw0) {  // in-kernel dW0: a slab per workgroup out of the pool, reduced with the GEMMs' slabs
    const size_t need = (size_t)fused_bwd_one_grid<P>(d, M) * H * 32;
    if (need > B.slab_floats - B.slab_used) flush_slabs(B, s);
    dw0_slab = B.slab + B.slab_used;
    B.slab_used += need;
    f.dh[0] = nullptr, f.dw0_slab = dw0_slab, f.xc = B.in, f.ld_xc = L.Kp0;
    f.xc_af = d.kind == 0 ? d.act_flat : 64, f.xc_skip = d.kind == 0 ? d.time_dim : 0;
    f.dw0_round = R.dw0_round ? 1 : 0;
  }
  return launch_fused_backward<P>(d, f, s);
}
// bias gradients = column sums, reduced over tiles in one launch; slot order: dh[nb..0], then dz1[nb-1..0]
static SlotOuts bias_slots(const dppo_net_desc& d, const ParamLayout& pl, const BwdRoute& R, float* grad) {
  const int H = d.hidden, nb = d.n_blocks;
  SlotOuts so;
  memset(&so, 0, sizeof(so));
  so.n_slots = 2 * nb + 1;
  for (int b = nb - 1; b >= 0; --b) {
    so.out[nb - (b + 1)] = grad + pl.l2b[b];
    so.out[(nb + 1) + (nb - 1 - b)] = grad + pl.l1b[b];
  }
  so.out[nb] = grad + pl.b0;
  if (d.use_layernorm) {  // 4 more slots per block, top block first: d gamma1, d beta1, d gamma2, d beta2
    for (int b = nb - 1; b >= 0; --b) {
      const int ls = (2 * nb + 1) + 4 * (nb - 1 - b);
      so.out[ls] = grad + pl.n1w[b], so.out[ls + 1] = grad + pl.n1b[b];
      so.out[ls + 2] = grad + pl.n2w[b], so.out[ls + 3] = grad + pl.n2b[b];
    }
    so.n_slots += 4 * nb;
  }
  for (int i = 0; i < so.n_slots; ++i) so.n[i] = H;
  if (R.one_block) so.n[0] = 0;  // colsum(dh_nb) is not formed by the one-block kernel: db2 comes from PostReduce::db2
  so.out[so.n_slots] = grad + pl.bout, so.n[so.n_slots] = d.out_dim, ++so.n_slots;  // the d_out slot: the out layer's bias gradient
  return so;
}
// the weight-gradient products, queued for one grouped launch (flush_slabs); the in-kernel dW0's slab jobs go to `side`
// when the side tail reduces them
template <class P>
static void queue_weight_grads(const dppo_net_desc& d, const ParamLayout& pl, const PackLayout& L, int64_t M, MlpBufs<P>& B,
                               float* grad, int Kft, hipStream_t s, float* dw0_slab, SlabJobs& side) {
  const BwdRoute& R = B.route;
  const int H = d.hidden, nb = d.n_blocks;
  // merged top (the forward never formed h_nb): dWout = d_out^T . h_nb is rebuilt behind the slab reduce from
  // U = d_out^T . x and T = d_out^T . act(z1) (PostReduce::U); T is then needed whether or not dW2 uses it
  if (R.merged)
    weight_grad<P>(B.d_out, L.Kpo, d.out_dim, B.in, L.Kp0, d.in_dim, M, B, B.lowrank_u, L.Kp0, s, true);
  else
    weight_grad<P>(B.d_out, L.Kpo, d.out_dim, B.hE, H, H, M, B, grad + pl.Wout, H, s, true);
  for (int b = nb - 1; b >= 0; --b) {
    if ((R.lowrank || R.merged) && b == nb - 1)  // T = d_out^T . act(z1), [out_dim][H]; dW2 = Wout^T . T after the slab reduce
      weight_grad<P>(B.d_out, L.Kpo, d.out_dim, B.a2[b], H, H, M, B, B.lowrank, H, s, true);
    if (!(R.lowrank && b == nb - 1))
      weight_grad<P>(B.dh_all[b + 1], H, H, B.a2[b], H, H, M, B, grad + pl.l2w[b], H, s, true);
    weight_grad<P>(B.dz1_all[b], H, H, B.a1[b], H, H, M, B, grad + pl.l1w[b], H, s, true);
  }
  if (R.dw0) {  // the kernel's per-workgroup partials [grid][H][32]: data columns -> dW0, one-hot columns -> S[h][k] (B.part)
    const int grid = fused_bwd_one_grid<P>(d, M);
    auto job = [&](int c0, int cols, float* out, int ldo) {
      SlabJob& j = R.side_tail ? side.j[side.n++] : B.slab_jobs.j[B.slab_jobs.n++];
      j.slab = dw0_slab, j.out = out, j.splits = grid, j.rows = H, j.cols = cols, j.lds = 32, j.ldo = ldo, j.transpose = 0;
      j.c0 = c0, j.wide = grid >= 32 ? 1 : 0;  // (a slab per workgroup: slab_job_block_wide)
    };
    if (d.kind == 0) {
      job(0, d.act_flat, grad + pl.W0, d.in_dim);
      job(d.act_flat, d.cond_dim, grad + pl.W0 + d.act_flat + d.time_dim, d.in_dim);
      job(d.act_flat + d.cond_dim, R.dw0_nhot, B.part, Kft);
    } else {
      job(0, d.in_dim, grad + pl.W0, d.in_dim);
    }
  } else if (g_dbg & 32) {  // timing experiment: no dW0 product in the group
  } else if (R.onehot_col >= 0)  // + Kft one-hot columns: their block of the result is S[h][k] (B.part), see plan_route()
    weight_grad<P>(B.dh_all[0], H, H, B.in, L.Kp0, d.in_dim + Kft, M, B, grad + pl.W0, d.in_dim, s, true, d.in_dim, B.part, Kft);
  else
    weight_grad<P>(B.dh_all[0], H, H, B.in, L.Kp0, d.in_dim, M, B, grad + pl.W0, d.in_dim, s, true);
}
// the time-embedding half of a PostReduce: G = W0_temb^T . S from the one-hot sums S (B.part), then the time MLP's backward
template <class P>
static void fill_time_post(PostReduce& q, const dppo_net_desc& d, const ParamLayout& pl, const float* prm, const char* pk,
                           const PackLayout& L, const MlpBufs<P>& B, float* grad, const dppo_step* ksteps, int Kft) {
  q.S = B.part, q.W0 = prm + pl.W0, q.ldw0 = d.in_dim, q.AF = d.act_flat, q.Kft = Kft, q.td = d.time_dim;
  q.G = B.part + (size_t)d.hidden * Kft, q.w1 = prm + pl.te1_w, q.b1 = prm + pl.te1_b, q.w2 = prm + pl.te2_w;
  q.ksteps = ksteps, q.gw1 = grad + pl.te1_w, q.gb1 = grad + pl.te1_b, q.gw2 = grad + pl.te2_w, q.gb2 = grad + pl.te2_b;
  if (B.route.dw0) {  // the time-embedding columns of dW0 from the one-hot sums, the last of which may have to be rebuilt
    // (without room for it the first layer's bias gradient is the column sums of the rounded dh_0)
    q.S_rest = B.route.dw0_round ? grad + pl.b0 : nullptr, q.dW0t = grad + pl.W0;
    q.temb = (const float*)(pk + L.temb), q.temb_bf16 = P::ESIZE == 2 ? 1 : 0;
  }
}
// Side tail (knob 38): what the backward kernel alone feeds -- its dW0 slabs, the bias sums, the loss statistics, then the
// time-embedding gradient -- queued on the side stream BEHIND the kernel and BESIDE the GEMM launch that follows on s
template <class P>
static void launch_side_tail(const dppo_net_desc& d, const ParamLayout& pl, const float* prm, const char* pk, const PackLayout& L,
                             MlpBufs<P>& B, float* grad, const dppo_step* ksteps, int Kft, hipStream_t s, const SlotOuts& so,
                             const SlabJobs& jobs, const LossArgs* fin) {
  hipStream_t st = fork_side(s, TAIL_SIDE);
  TailReduce t;
  memset(&t, 0, sizeof(t));
  t.jobs = jobs, t.colsum = B.tile_colsum, t.tiles = B.tiles, t.width = d.hidden, t.slots = so;
  launch_tail_reduce(t, fin, st);
  PostReduce q;
  memset(&q, 0, sizeof(q));
  q.H = d.hidden, q.out_dim = d.out_dim;
  fill_time_post<P>(q, d, pl, prm, pk, L, B, grad, ksteps, Kft);
  q.counter = (unsigned*)B.post_counter;
  launch_post_reduce(q, st);
  B.join_s[B.n_join] = st, B.join_idx[B.n_join++] = TAIL_SIDE;  // (joined right behind the GEMM launch: flush_slabs)
}
// what follows the slab reduction on s: the low-rank dW2, dWout / db2 of a merged / one-block network, the time-embedding
// gradient from the one-hot sums (unless the side tail took it) -- one launch (knob 18; with knob 41 the slab reduction too)
template <class P>
static void launch_post(const dppo_net_desc& d, const ParamLayout& pl, const float* prm, const char* pk, const PackLayout& L,
                        MlpBufs<P>& B, float* grad, const dppo_step* ksteps, int Kft, hipStream_t s) {
  const BwdRoute& R = B.route;
  const int H = d.hidden, nb = d.n_blocks;
  const bool oh = R.onehot_col >= 0;
  PostReduce q;
  memset(&q, 0, sizeof(q));
  q.H = H, q.out_dim = d.out_dim, q.T = B.lowrank;
  if (R.merged) {  // (cs = column sums of d_out = the out-layer bias gradient, reduced on the aux stream joined above)
    q.U = B.lowrank_u, q.ldu = L.Kp0, q.in_dim = d.in_dim, q.W0 = prm + pl.W0, q.ldw0 = d.in_dim, q.W2 = prm + pl.l2w[nb - 1];
    q.b0 = prm + pl.b0, q.b2 = prm + pl.l2b[nb - 1], q.cs = grad + pl.bout, q.dWout = grad + pl.Wout;
  }
  if (R.one_block) q.db2 = grad + pl.l2b[0], q.Wout_b = prm + pl.Wout, q.cs = grad + pl.bout;
  if (!R.post_one) {
    launch_wout_grad(q, s);  // (merged top and / or one-block backward; nothing otherwise)
    if (R.lowrank) launch_lowrank_dw(prm + pl.Wout, B.lowrank, d.out_dim, H, grad + pl.l2w[nb - 1], s);
    if (oh) {
      PostReduce t = {};
      fill_time_post<P>(t, d, pl, prm, pk, L, B, grad, ksteps, Kft);
      launch_time_backward_from_sums(t.w1, t.b1, t.w2, t.S, t.W0, t.ldw0, t.AF, H, t.G, ksteps, Kft, t.td, t.gw1, t.gb1, t.gw2, t.gb2, s);
    }
    return;
  }
  if (R.lowrank) q.Wout = prm + pl.Wout, q.dW = grad + pl.l2w[nb - 1];
  if (oh && !R.side_tail) fill_time_post<P>(q, d, pl, prm, pk, L, B, grad, ksteps, Kft);
  q.counter = (unsigned*)B.post_counter;
  if (!R.tail_post) {
    launch_post_reduce(q, s);
    return;
  }
  TailPost tp;  // (no time-embedding part here: it went to the side stream)
  memset(&tp, 0, sizeof(tp));
  for (int pass = 0; pass < 2; ++pass)  // the thin products' jobs first
    for (int i = 0; i < B.slab_jobs.n; ++i) {
      const SlabJob& j = B.slab_jobs.j[i];
      const bool thin = j.out == B.lowrank || j.out == B.lowrank_u;
      if (thin == (pass == 0)) tp.jobs.j[tp.jobs.n++] = j;
      if (thin && pass == 0) ++tp.n_first_jobs;
    }
  tp.q = q;
  tp.q.wait_cnt = B.tail_counter;  // (zeroed by the row builder: DPPO_ROUTE_IN_ZEROED)
  launch_tail_post(tp, s);
  B.slab_jobs.n = 0, B.slab_used = 0;
}
template <class P>
static void backward_fused(const dppo_net_desc& d, const float* prm, const char* pk, const PackLayout& L, int64_t M,
                           MlpBufs<P>& B, float* grad, const int32_t* krow, const dppo_step* ksteps, int Kft,
                           hipStream_t s, const LossArgs* fin) {
  const BwdRoute& R = B.route;
  const ParamLayout pl = param_layout(d);
  float* dw0_slab;
  g_fused_fault = launch_backward_kernel<P>(d, prm, pk, L, M, B, s, dw0_slab);
  if (g_fused_fault != 0) return;
  const SlotOuts so = bias_slots(d, pl, R, grad);
  // The bias sums and the loss statistics ride in the slab-reduction launch behind the GEMMs (tail_reduce_kernel).
  // Only the rare time-embedding gradient WITHOUT the one-hot columns (a gemm_nt + segmented sum over all rows) still runs
  // beside the GEMMs on a side stream (it shares B.part with nothing on s).
  hipStream_t aux = R.aux_side ? fork_side(s, TAIL_SIDE) : s;
  if (R.need_aux) time_embedding_grad<P>(d, prm, pk, L, M, B, B.dh_all[0], grad, krow, ksteps, Kft, aux);
  SlabJobs side_jobs = {};
  queue_weight_grads<P>(d, pl, L, M, B, grad, Kft, s, dw0_slab, side_jobs);
  if (R.side_tail) launch_side_tail<P>(d, pl, prm, pk, L, B, grad, ksteps, Kft, s, so, side_jobs, fin);
  if (aux != s && g_early_join) B.join_s[B.n_join] = aux, B.join_idx[B.n_join++] = TAIL_SIDE;
  if (R.tail_post)
    flush_slabs(B, s, nullptr, 0, nullptr, true);  // the GEMMs; their slabs are reduced with the post-reduce parts below
  else if (R.side_tail)
    flush_slabs(B, s);  // the GEMMs' own slabs
  else
    flush_slabs(B, s, &so, d.hidden, fin);  // every slab of this backward, its bias sums and the loss statistics: one launch
  if (aux != s && !g_early_join) join_side(s, aux, TAIL_SIDE);
  launch_post<P>(d, pl, prm, pk, L, B, grad, ksteps, Kft, s);
  B.dh0_final = R.dw0 ? nullptr : B.dh_all[0];  // (in-kernel dW0: no dh_0 exists; plan_route() made sure nobody asks)
}
// a plain MLP's backward, layer by layer
template <class P>
static void backward_plain(const dppo_net_desc& d, const float* prm, const char* pk, const PackLayout& L, int64_t M,
                           MlpBufs<P>& B, float* grad, const int32_t* krow, const dppo_step* ksteps, int Kft, hipStream_t s,
                           const DropBwd* drop = nullptr) {
  // drop (mask, scale): the forward ran with dropout (ibrl.h); the kept pre-activations are z', and each hidden layer's d/dz' becomes
  // d/dz in place where LayerNorm's backward sits in a LayerNorm trunk.  Null: every caller from before runs launch for launch.
  const ParamLayout pl = param_layout(d);
  const int H = d.hidden, nb = d.n_blocks;
  weight_grad<P>(B.d_out, L.Kpo, d.out_dim, B.a2[nb - 1], H, H, M, B, grad + pl.Wout, H, s);
  launch_colsum<P>(B.d_out, (int)M, d.out_dim, L.Kpo, B.part, REDUCE_BLOCKS, grad + pl.bout, 1.f, s);
  GemmNT q;  // dz = (upstream . W) * act'(z): starts from d_out . Wout at the last hidden layer's pre-activation
  memset(&q, 0, sizeof(q));
  q.M = (int)M, q.N = H, q.Kp = L.Kpo, q.ldx = L.Kpo, q.ldw = L.Kpo, q.ldo = H;
  q.X = B.d_out, q.W = pk + L.WoutT, q.dsrc = B.z1[nb - 1], q.dsrc_kind = 2, q.dsrc_ld = H, q.dact = d.act, q.out_pre = B.dh;
  // wide: upstream (.) act'(z) reaches LayerNorm's backward in fp32 (ibrl.h); its in-place output is the elem row either way
  const bool wide = d.use_layernorm && B.ln_dz32[0] != nullptr;
  float* dz32 = B.ln_dz32[0];
  float* other32 = B.ln_dz32[1];
  if (wide) q.out_pre = nullptr, q.out_f32 = dz32, q.ldo32 = H;
  launch_gemm_nt<P>(q, s);
  void* dz = B.dh;
  void* other = B.dz1;
  // LayerNorm (rlpd.h): dz is d loss / d z here; in place it becomes d loss / d (the Linear's output), what the steps below read
  LnBwd ln;
  memset(&ln, 0, sizeof(ln));
  ln.ld = H, ln.ldx = H, ln.M = M, ln.H = H, ln.partial = B.ln_part;
  DropBwd db;
  memset(&db, 0, sizeof(db));
  if (drop != nullptr) db = *drop, db.ld = H, db.M = M, db.H = H;
  for (int b = nb - 1; b >= 0; --b) {
    if (drop != nullptr) {
      db.dz = dz, db.layer = b + 1;
      launch_drop_bwd<P>(db, s);
    }
    if (d.use_layernorm) {
      ln.dz = dz, ln.dz32 = wide ? dz32 : nullptr, ln.x = B.h[b + 1], ln.stats = B.ln_stats + (size_t)(b + 1) * M * 2, ln.gamma = prm + pl.n1w[b];
      ln.dgamma = grad + pl.n1w[b], ln.dbeta = grad + pl.n1b[b];
      launch_ln_bwd<P>(ln, s);
    }
    weight_grad<P>(dz, H, H, b == 0 ? B.a1[0] : B.a2[b - 1], H, H, M, B, grad + pl.l1w[b], H, s);
    launch_colsum<P>(dz, (int)M, H, H, B.part, REDUCE_BLOCKS, grad + pl.l1b[b], 1.f, s);
    memset(&q, 0, sizeof(q));
    q.M = (int)M, q.N = H, q.Kp = H, q.ldx = H, q.ldw = H, q.ldo = H;
    q.X = dz, q.W = pk + L.W1T[b], q.dsrc = b == 0 ? B.hpre[0] : B.z1[b - 1], q.dsrc_kind = 2, q.dsrc_ld = H, q.dact = d.act;
    q.out_pre = other;
    if (wide) q.out_pre = nullptr, q.out_f32 = other32, q.ldo32 = H;
    launch_gemm_nt<P>(q, s);
    void* t = dz;
    dz = other, other = t;
    float* t32 = dz32;
    dz32 = other32, other32 = t32;
  }
  if (d.use_layernorm) {
    ln.dz = dz, ln.dz32 = wide ? dz32 : nullptr, ln.x = B.h[0], ln.stats = B.ln_stats, ln.gamma = prm + pl.n0w, ln.dgamma = grad + pl.n0w, ln.dbeta = grad + pl.n0b;
    launch_ln_bwd<P>(ln, s);
  }
  if (drop != nullptr) {
    db.dz = dz, db.layer = 0;
    launch_drop_bwd<P>(db, s);
  }
  weight_grad<P>(dz, H, H, B.in, L.Kp0, d.in_dim, M, B, grad + pl.W0, d.in_dim, s);
  launch_colsum<P>(dz, (int)M, H, H, B.part, REDUCE_BLOCKS, grad + pl.b0, 1.f, s);
  if (d.kind == 0) time_embedding_grad<P>(d, prm, pk, L, M, B, dz, grad, krow, ksteps, Kft, s);
  B.dh0_final = dz;
}
// the residual trunk's backward on the layered GEMM path
template <class P>
static void backward_layered(const dppo_net_desc& d, const float* prm, const char* pk, const PackLayout& L, int64_t M,
                             MlpBufs<P>& B, float* grad, const int32_t* krow, const dppo_step* ksteps, int Kft, hipStream_t s) {
  const ParamLayout pl = param_layout(d);
  const int H = d.hidden, nb = d.n_blocks;
  // output layer parameters
  weight_grad<P>(B.d_out, L.Kpo, d.out_dim, B.hE, H, H, M, B, grad + pl.Wout, H, s);
  launch_colsum<P>(B.d_out, (int)M, d.out_dim, L.Kpo, B.part, REDUCE_BLOCKS, grad + pl.bout, 1.f, s);
  // dh = d_out . Wout
  GemmNT g;
  memset(&g, 0, sizeof(g));
  g.M = (int)M, g.N = H, g.Kp = L.Kpo, g.ldx = L.Kpo, g.ldw = L.Kpo, g.ldo = H;
  g.X = B.d_out, g.W = pk + L.WoutT, g.out_pre = B.dh;
  launch_gemm_nt<P>(g, s);
  for (int b = nb - 1; b >= 0; --b) {
    // l2: dz2 = dh
    weight_grad<P>(B.dh, H, H, B.a2[b], H, H, M, B, grad + pl.l2w[b], H, s);
    launch_colsum<P>(B.dh, (int)M, H, H, B.part, REDUCE_BLOCKS, grad + pl.l2b[b], 1.f, s);
    // dz1 = (dh . W2) * act'(z1)
    memset(&g, 0, sizeof(g));
    g.M = (int)M, g.N = H, g.Kp = H, g.ldx = H, g.ldw = H, g.ldo = H;
    g.X = B.dh, g.W = pk + L.W2T[b], g.dsrc = B.z1[b], g.dsrc_kind = 2, g.dsrc_ld = H, g.dact = d.act;
    g.out_pre = B.dz1;
    launch_gemm_nt<P>(g, s);
    weight_grad<P>(B.dz1, H, H, B.a1[b], H, H, M, B, grad + pl.l1w[b], H, s);
    launch_colsum<P>(B.dz1, (int)M, H, H, B.part, REDUCE_BLOCKS, grad + pl.l1b[b], 1.f, s);
    // dh <- dh + (dz1 . W1) * act'(h[b])      (in place: each element is read then written by one lane)
    memset(&g, 0, sizeof(g));
    g.M = (int)M, g.N = H, g.Kp = H, g.ldx = H, g.ldw = H, g.ldo = H;
    g.X = B.dz1, g.W = pk + L.W1T[b], g.dsrc = B.h[b], g.dsrc_kind = 1, g.dsrc_ld = H, g.dact = d.act;
    g.add = B.dh, g.ldadd = H, g.out_pre = B.dh;
    launch_gemm_nt<P>(g, s);
  }
  // layer 0: dW0[h][c] = sum_m dh[m][h] in[m][c]
  weight_grad<P>(B.dh, H, H, B.in, L.Kp0, d.in_dim, M, B, grad + pl.W0, d.in_dim, s);
  launch_colsum<P>(B.dh, (int)M, H, H, B.part, REDUCE_BLOCKS, grad + pl.b0, 1.f, s);
  if (d.kind == 0) time_embedding_grad<P>(d, prm, pk, L, M, B, B.dh, grad, krow, ksteps, Kft, s);
  B.dh0_final = B.dh;
}

// d_out (B.d_out, [M][Kpo] elem) -> gradients of every parameter of the network into `grad`
// fin: the loss's statistics are finalised off the critical path (on the tail stream, or after the GEMMs)
template <class P>
static void mlp_backward(const dppo_net_desc& d, const float* prm, const char* pk, const PackLayout& L, int64_t M,
                         MlpBufs<P>& B, float* grad, const int32_t* krow, const dppo_step* ksteps, int Kft,
                         hipStream_t s, const LossArgs* fin = nullptr, const DropBwd* drop = nullptr) {
  if (B.route.fused) return backward_fused<P>(d, prm, pk, L, M, B, grad, krow, ksteps, Kft, s, fin);
  if (fin) launch_loss_finalize(*fin, s);  // (the fused backward finalises them in one of its reduction launches)
  if (d.plain) return backward_plain<P>(d, prm, pk, L, M, B, grad, krow, ksteps, Kft, s, drop);
  backward_layered<P>(d, prm, pk, L, M, B, grad, krow, ksteps, Kft, s);
}

// d loss / d observation of a trunk WITHOUT an observation encoder: d_obs[m][c] = sum_h dh0[m][h] W0[h][col0 + c], where the
// observation sits in layer 0's input at columns col0 = act_flat + time_dim (actor: cat[x, temb, obs]) or 0 (critic).  What a
// visual encoder in front of the trunk (vision.hip) back-propagates from.  One transposing pack of cond_dim x H weights
// + one gemm_nt.
template <class P>
static void obs_grad(const dppo_net_desc& d, const float* prm, int64_t M, MlpBufs<P>& B, float* d_obs, hipStream_t s) {
  const ParamLayout pl = param_layout(d);
  const int H = d.hidden, col0 = d.kind == 0 ? d.act_flat + d.time_dim : 0;
  launch_transpose_cast<P>(prm + pl.W0, H, d.cond_dim, d.in_dim, col0, B.w0T, H, s);
  GemmNT g;
  memset(&g, 0, sizeof(g));
  g.M = (int)M, g.N = d.cond_dim, g.Kp = H, g.ldx = H, g.ldw = H, g.X = B.dh0_final, g.W = B.w0T;
  g.out_f32 = B.dobs, g.ldo32 = round_up(d.cond_dim, 16);
  launch_gemm_nt<P>(g, s);
  launch_copy_cols(B.dobs, g.ldo32, 0, d.cond_dim, M, d_obs, s);
}

// ------------------------------------------------------------------------------------------------
// exported functions
// ------------------------------------------------------------------------------------------------
// Exported functions take C linkage from their declarations in include/dppo_hip.h.

int dppo_version(void) { return 1; }
const char* dppo_last_error(void) { return g_err; }

int64_t dppo_net_param_count(const dppo_net_desc* net) {
  if (check_net(net, true)) return -1;
  return param_layout(*net).total;
}

int64_t dppo_packed_bytes(const dppo_net_desc* net, int prec, int n_time) {
  if (check_net(net, true) || check_prec(prec)) return -1;
  if (n_time < 0) return fail(-1, "n_time < 0");
#define CALL(P) (int64_t) pack_layout<P>(*net, n_time).total
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

template <class P>
static int pack_two_impl(const dppo_net_desc& d0, int t0, const float* p0, char* k0, const dppo_net_desc& d1, int t1,
                         const float* p1, char* k1, hipStream_t s) {
  PackNets q;
  ComposeJobs cq;
  memset(&q, 0, sizeof(q));
  memset(&cq, 0, sizeof(cq));
  bool def0 = false, def1 = false;
  ComposeJob c0, c1;
  memset(&c0, 0, sizeof(c0));
  memset(&c1, 0, sizeof(c1));
  if (int e = pack_impl<P>(d0, t0, p0, k0, s, &q.n[0], &c0, &def0)) return e;
  if (int e = pack_impl<P>(d1, t1, p1, k1, s, &q.n[1], &c1, &def1)) return e;
  if (def0 && c0.Wout) cq.j[cq.n++] = c0;
  if (def1 && c1.Wout) cq.j[cq.n++] = c1;
  launch_compose(cq, s);  // both composites in one launch, then both networks' images in one launch
  if (def0 && def1)
    launch_pack_nets<P>(q, s);
  else if (def0)
    launch_pack_net<P>(q.n[0], s);
  else if (def1)
    launch_pack_net<P>(q.n[1], s);
  return check_launch();
}

int dppo_pack_nets(const dppo_net_desc* net0, int n_time0, const float* params0, void* packed0,
                   const dppo_net_desc* net1, int n_time1, const float* params1, void* packed1, int prec,
                   dppo_stream_t stream) {
  if (int e = check_net(net0, true)) return e;
  if (int e = check_net(net1, true)) return e;
  if (int e = check_prec(prec)) return e;
  if (!params0 || !packed0 || !params1 || !packed1) return fail(-1, "null pointer");
  if ((net0->kind == 0 && n_time0 < 1) || (net1->kind == 0 && n_time1 < 1)) return fail(-1, "actor needs n_time >= 1");
#define CALL(P)                                                                                                  \
  pack_two_impl<P>(*net0, n_time0, params0, (char*)packed0, *net1, n_time1, params1, (char*)packed1, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

int dppo_pack_net(const dppo_net_desc* net, int prec, int n_time, const float* params, void* packed,
                  dppo_stream_t stream) {
  if (int e = check_net(net, true)) return e;
  if (int e = check_prec(prec)) return e;
  if (!params || !packed) return fail(-1, "null pointer");
  if (net->kind == 0 && n_time < 1) return fail(-1, "actor needs n_time >= 1");
#define CALL(P) pack_impl<P>(*net, n_time, params, (char*)packed, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- forwards --------------------------------------------------------------------------------------
int64_t dppo_mlp_forward_workspace_bytes(const dppo_net_desc* net, int prec, int64_t rows) {
  if (check_net(net) || check_prec(prec)) return -1;
  if (rows < 0 || rows > 0x7fffffff) return fail(-1, "rows out of range");
  return ws_bytes(prec, [&](Carver& c, auto p) {
    MlpBufs<decltype(p)> B;
    carve_mlp<decltype(p)>(c, *net, rows, false, false, B);
    return al256(c.off);
  });
}

template <class P>
static int net_forward_impl(const dppo_net_desc& d, const float* prm, const char* pk, const float* x,
                            const int64_t* t, const float* state, int64_t M, float* out, void* ws, int64_t wsb,
                            hipStream_t s) {
  Carver c{(char*)ws, 0, (size_t)wsb};
  MlpBufs<P> B;
  carve_mlp<P>(c, d, M, false, false, B);
  if ((int64_t)c.off > wsb) return fail(-1, "workspace too small: need %zu bytes, got %lld", c.off, (long long)wsb);
  const PackLayout L = pack_layout<P>(d, 0);
  if (d.cond_hidden > 0) {  // [x | temb | 0] rows, then the encoder writes its columns
    launch_build_direct<P>(x, t, nullptr, (const float*)(pk + L.temb), d.act_flat, d.time_dim, 0, M, B.in, L.Kp0, s);
    launch_build_direct<P>(nullptr, nullptr, state, nullptr, 0, 0, d.cond_dim, M, B.cin, L.Kpc, s);
    cond_encode<P>(d, prm, pk, L, M, B.cin, B, B.in, nullptr, 0, false, s);
  } else {
    launch_build_direct<P>(x, t, state, (const float*)(pk + L.temb), d.act_flat, d.time_dim, d.cond_dim, M, B.in,
                           L.Kp0, s);
  }
  mlp_forward<P>(d, prm, pk, L, M, B, false, s);
  launch_slab_reduce_2d(B.out, 1, (int)M, d.out_dim, B.ldout, out, d.out_dim, 1.f, s);
  return check_launch();
}

int dppo_actor_forward(const dppo_net_desc* net, int prec, const float* params, const void* packed, const float* x,
                       const int64_t* t, const float* state, int64_t rows, float* eps, void* workspace,
                       int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_net(net)) return e;
  if (int e = check_prec(prec)) return e;
  if (net->kind != 0) return fail(-1, "dppo_actor_forward needs an actor descriptor");
  if (!params || !packed || !x || !t || !state || !eps || !workspace) return fail(-1, "null pointer");
  if (rows <= 0 || rows > 0x7fffffff) return fail(-1, "rows out of range");
#define CALL(P) \
  net_forward_impl<P>(*net, params, (const char*)packed, x, t, state, rows, eps, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

int dppo_critic_forward(const dppo_net_desc* net, int prec, const float* params, const void* packed,
                        const float* state, int64_t rows, float* values, void* workspace, int64_t workspace_bytes,
                        dppo_stream_t stream) {
  if (int e = check_net(net)) return e;
  if (int e = check_prec(prec)) return e;
  if (net->kind != 1) return fail(-1, "dppo_critic_forward needs a critic descriptor");
  if (!params || !packed || !state || !values || !workspace) return fail(-1, "null pointer");
  if (rows <= 0 || rows > 0x7fffffff) return fail(-1, "rows out of range");
#define CALL(P)                                                                                                    \
  net_forward_impl<P>(*net, params, (const char*)packed, nullptr, nullptr, state, rows, values, workspace, workspace_bytes, \
                      (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- sampler -----------------------------------------------------------------------------------------
template <class P>
static bool sample_split(const dppo_net_desc& d, int64_t B) {
  return sampler_split_ok(d, P::ESIZE == 2, B, g_merge_top && d.n_blocks >= 1);
}
template <class P>
static size_t sample_carve(Carver& c, const dppo_net_desc& d, int64_t B, MlpBufs<P>& Bz, float*& enc, void** xch = nullptr) {
  memset(&Bz, 0, sizeof(Bz));
  enc = nullptr;
  if (sample_split<P>(d, B)) {  // the split sampler's exchange block: first, so that its memset starts at the allocation
    void* x = c.take(sampler_split_xch_bytes(d, B));
    if (xch) *xch = x;
  }
  if (d.cond_hidden <= 0) return al256(c.off);
  const size_t ES = P::ESIZE;
  Bz.cin = c.take((size_t)B * round_up(d.cond_dim, 64) * ES);
  Bz.ca = c.take((size_t)B * round_up(d.cond_hidden, 64) * ES);
  enc = (float*)c.take((size_t)2 * B * round_up(d.cond_out, 16) * 4);
  return al256(c.off);
}
template <class P>
static size_t sample_ws(const dppo_net_desc& d, int64_t B) {
  Carver c{nullptr, 0, 0};
  MlpBufs<P> Bz;
  float* enc;
  return sample_carve<P>(c, d, B, Bz, enc);
}

template <class P>
static int sample_impl(const dppo_net_desc& d, const float* pb, const char* kb, const float* pf, const char* kf,
                       const dppo_diffusion_cfg& cfg, const dppo_step* sched, int n_steps, const float* obs,
                       const float* noise, int64_t B, float* traj, float* chains, int chain_len, int init_slot, void* ws,
                       int64_t wsb, hipStream_t s) {
  const SamplerGeom g = sampler_geom<P>(d);
  const PackLayout L = pack_layout<P>(d, 0);
  const ParamLayout pl = param_layout(d);
  SampleArgs a;
  memset(&a, 0, sizeof(a));
  a.wstream[0] = (const u32x4*)(kb + L.sstream), a.wstream[1] = (const u32x4*)(kf + L.sstream);
  a.ostream[0] = (const u32x4*)(kb + L.ostream), a.ostream[1] = (const u32x4*)(kf + L.ostream);
  a.ostream2[0] = (const u32x4*)(kb + L.ostream2), a.ostream2[1] = (const u32x4*)(kf + L.ostream2);
  a.cbias[0] = (const float*)(kb + L.cbias), a.cbias[1] = (const float*)(kf + L.cbias);
  a.merge_top = g_merge_top && d.n_blocks >= 1 ? 1 : 0;
  a.params[0] = pb, a.params[1] = pf;
  a.temb[0] = (const float*)(kb + L.temb), a.temb[1] = (const float*)(kf + L.temb);
  fill_bias_off(d, pl, a.bias_off);
  a.use_ln = d.use_layernorm;
  if (d.use_layernorm) fill_ln_off(d, pl, a.ln_off);
  a.obs[0] = a.obs[1] = obs, a.cond = d.cond_dim, a.ld_obs = d.cond_dim;
  void* xch = nullptr;
  const bool split = sample_split<P>(d, B);
  if (d.cond_hidden > 0 || split) {
    MlpBufs<P> Bz;
    float* enc = nullptr;
    if (!ws || (int64_t)sample_ws<P>(d, B) > wsb)
      return fail(-1, "sampler workspace too small: need %zu bytes (dppo_sample_chain_workspace_bytes)", sample_ws<P>(d, B));
    Carver c{(char*)ws, 0, (size_t)wsb};
    sample_carve<P>(c, d, B, Bz, enc, &xch);
    if (d.cond_hidden > 0) {  // per-network encoded observation, computed once per call (constant over the K steps)
      const int lde = round_up(d.cond_out, 16);
      launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, d.cond_dim, B, Bz.cin, L.Kpc, s);
      cond_encode<P>(d, pb, kb, L, B, Bz.cin, Bz, nullptr, enc, lde, false, s);
      cond_encode<P>(d, pf, kf, L, B, Bz.cin, Bz, nullptr, enc + (size_t)B * lde, lde, false, s);
      a.obs[0] = enc, a.obs[1] = enc + (size_t)B * lde, a.cond = d.cond_out, a.ld_obs = lde;
    }
  }
  a.noise = noise, a.seed_lo = cfg.seed_lo, a.seed_hi = cfg.seed_hi, a.traj = traj, a.chains = chains, a.sched = sched;
  a.B = (int)B, a.AF = d.act_flat, a.td = d.time_dim, a.Kp0 = g.Kp0, a.nb = d.n_blocks;
  a.n_steps = n_steps, a.chain_len = chain_len, a.init_slot = init_slot, a.act = d.act, a.use_ddim = cfg.use_ddim;
  a.has_dclip = cfg.has_denoised_clip, a.has_eclip = cfg.has_eps_clip, a.has_fclip = cfg.has_final_clip;
  a.dclip = cfg.denoised_clip, a.eclip = cfg.eps_clip, a.rclip = cfg.randn_clip, a.fclip = cfg.final_clip;
  if (split) {
    const int rs = launch_sample_chain_split(g, a, xch, sampler_split_xch_bytes(d, B), s);
    if (rs == 0) return check_launch();
    if (rs != -1) return fail(-1, "split sampler: launch failed (%d)", rs);
  }
  const int rc = launch_sample_chain<P>(g, a, s);
  if (rc == -1) return fail(-1, "sampler: hidden=%d / out_dim=%d not instantiated (hidden in {256,512,768,1024}, out_dim <= 128)", d.hidden, d.out_dim);
  if (rc == -2) return fail(-1, "sampler: LDS image exceeds 160 KiB for hidden=%d at this precision", d.hidden);
  return check_launch();
}

// ---- plain (non-residual) trunks: the K-step loop on the host, one layered forward + one posterior kernel per step -------
template <class P>
static size_t carve_plain_sample(Carver& c, const dppo_net_desc& d, int64_t B, MlpBufs<P>& Bz, float*& x) {
  carve_mlp<P>(c, d, B, false, false, Bz);
  x = (float*)c.take((size_t)B * d.act_flat * 4);
  return al256(c.off);
}
int64_t dppo_plain_sample_workspace_bytes(const dppo_net_desc* actor, int prec, int64_t B) {
  if (check_net(actor) || check_prec(prec)) return -1;
  if (actor->kind != 0 || !actor->plain) return fail(-1, "dppo_plain_sample_chain needs a plain actor descriptor");
  if (B < 1 || B > 0x7fffffff) return fail(-1, "B out of range");
  return ws_bytes(prec, [&](Carver& c, auto p) {
    MlpBufs<decltype(p)> Bz;
    float* x;
    return carve_plain_sample<decltype(p)>(c, *actor, B, Bz, x);
  });
}
template <class P>
static int plain_sample_impl(const dppo_net_desc& d, const float* pb, const char* kb, const float* pf, const char* kf,
                             const dppo_diffusion_cfg& cfg, const dppo_step* sched, int n_steps, const float* obs,
                             const float* noise, int64_t B, float* traj, float* chains, int chain_len, int init_slot, void* ws,
                             int64_t wsb, hipStream_t s) {
  Carver c{(char*)ws, 0, (size_t)wsb};
  MlpBufs<P> Bz;
  float* x;
  const size_t need = carve_plain_sample<P>(c, d, B, Bz, x);
  if ((int64_t)need > wsb) return fail(-1, "workspace too small: need %zu bytes, got %lld", need, (long long)wsb);
  const PackLayout L = pack_layout<P>(d, 0);
  const int AF = d.act_flat;
  const int64_t n = B * AF;
  launch_chain_init(noise, cfg.seed_lo, cfg.seed_hi, n, AF, x, chains, chain_len, init_slot, s);
  for (int i = 0; i < n_steps; ++i) {
    const dppo_step& st = sched[i];
    const float* prm = st.net ? pf : pb;
    const char* pk = st.net ? kf : kb;
    // rows [x | temb(t) | obs]: the table pointer is offset to row t, so every row reads its row 0
    launch_build_direct<P>(x, nullptr, obs, (const float*)(pk + L.temb) + (size_t)st.t * d.time_dim, AF, d.time_dim, d.cond_dim, B,
                           Bz.in, L.Kp0, s);
    mlp_forward<P>(d, prm, pk, L, B, Bz, false, s);
    launch_chain_step(cfg, st, x, Bz.out, Bz.ldout, noise, (size_t)(i + 1) * n, n, AF, chain_len, i + 1 == n_steps, chains, traj, s);
  }
  return check_launch();
}
int dppo_plain_sample_chain(const dppo_net_desc* actor, int prec, const float* params_base, const void* packed_base,
                            const float* params_ft, const void* packed_ft, const dppo_diffusion_cfg* cfg,
                            const dppo_step* sched_host, int n_steps, const float* obs, const float* noise, int64_t B,
                            float* traj, float* chains, int chain_len, int init_slot, void* workspace,
                            int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_net(actor)) return e;
  if (int e = check_prec(prec)) return e;
  if (actor->kind != 0 || !actor->plain) return fail(-1, "dppo_plain_sample_chain needs a plain actor descriptor");
  if (!params_base || !packed_base || !params_ft || !packed_ft || !cfg || !sched_host || !obs || !traj || !workspace)
    return fail(-1, "null pointer");
  if (B < 1 || B > 0x7fffffff || n_steps < 1) return fail(-1, "B / n_steps out of range");
  if (chains != nullptr && chain_len < 1) return fail(-1, "chain_len must be >= 1 when chains are requested");
#define CALL(P)                                                                                                             \
  plain_sample_impl<P>(*actor, params_base, (const char*)packed_base, params_ft, (const char*)packed_ft, *cfg, sched_host, n_steps, \
                       obs, noise, B, traj, chains, chain_len, init_slot, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

int64_t dppo_sample_chain_workspace_bytes(const dppo_net_desc* actor, int prec, int64_t B) {
  if (check_net(actor) || check_prec(prec)) return -1;
  if (actor->plain) return fail(-1, "plain MLP trunks sample through dppo_plain_sample_chain (dppo_plain_sample_workspace_bytes)");
  if (B < 1) return fail(-1, "B out of range");
#define CALL(P) (int64_t) sample_ws<P>(*actor, B)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

int64_t dppo_sample_chain_exchange_bytes(const dppo_net_desc* actor, int prec, int64_t B) {
  if (check_net(actor) || check_prec(prec)) return -1;
  if (actor->plain || B < 1) return 0;
  const bool split = prec == DPPO_PREC_F32 ? sample_split<F32>(*actor, B) : sample_split<BF16>(*actor, B);
  return split ? (int64_t)sampler_split_xch_bytes(*actor, B) : 0;
}

int dppo_sample_chain(const dppo_net_desc* actor, int prec, const float* params_base, const void* packed_base,
                      const float* params_ft, const void* packed_ft, const dppo_diffusion_cfg* cfg,
                      const dppo_step* sched, int n_steps, const float* obs, const float* noise, int64_t B, float* traj,
                      float* chains, int chain_len, int init_slot, void* workspace, int64_t workspace_bytes,
                      dppo_stream_t stream) {
  if (int e = check_net(actor)) return e;
  if (int e = check_prec(prec)) return e;
  if (actor->plain) return fail(-1, "plain MLP trunks sample through dppo_plain_sample_chain (host-looped steps)");
  if (actor->kind != 0) return fail(-1, "dppo_sample_chain needs an actor descriptor");
  if (!params_base || !packed_base || !params_ft || !packed_ft || !cfg || !sched || !obs || !traj)  // noise may be NULL
    return fail(-1, "null pointer");
  if (n_steps < 1) return fail(-1, "n_steps must be >= 1");
  if (B < 1 || B > (1 << 24)) return fail(-1, "B out of range");
  if (chain_len < 0 || (chain_len > 0 && !chains)) return fail(-1, "chains buffer missing");
  if (init_slot >= chain_len) return fail(-1, "init_slot outside the chain");
#define CALL(P)                                                                                                   \
  sample_impl<P>(*actor, params_base, (const char*)packed_base, params_ft, (const char*)packed_ft, *cfg, sched, n_steps, obs, \
                 noise, B, traj, chains, chain_len, init_slot, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- chain log-probs ---------------------------------------------------------------------------------
int64_t dppo_chain_logprob_workspace_bytes(const dppo_net_desc* actor, int prec, int64_t B, int Kft) {
  if (check_net(actor) || check_prec(prec)) return -1;
  if (B < 0 || Kft < 1 || B * Kft > 0x7fffffff) return fail(-1, "B*Kft out of range");
  return ws_bytes(prec, [&](Carver& c, auto p) {  // the network's buffers, then brow and krow
    MlpBufs<decltype(p)> W;
    carve_mlp<decltype(p)>(c, *actor, B * Kft, false, false, W);
    c.take((size_t)B * Kft * 4), c.take((size_t)B * Kft * 4);
    return al256(c.off);
  });
}

template <class P>
static int logprob_impl(const dppo_net_desc& d, const float* prm, const char* pk, const dppo_diffusion_cfg& cfg,
                        const dppo_step* ksteps, int Kft, const float* obs, const float* chains, int64_t Bn, float* logp,
                        void* ws, int64_t wsb, hipStream_t s) {
  const int64_t M = Bn * Kft;
  Carver c{(char*)ws, 0, (size_t)wsb};
  MlpBufs<P> B;
  carve_mlp<P>(c, d, M, false, false, B);
  int32_t* brow = (int32_t*)c.take((size_t)M * 4);
  int32_t* krow = (int32_t*)c.take((size_t)M * 4);
  if ((int64_t)c.off > wsb) return fail(-1, "workspace too small: need %zu bytes, got %lld", c.off, (long long)wsb);
  const PackLayout L = pack_layout<P>(d, 0);
  BuildRows br;
  memset(&br, 0, sizeof(br));
  br.chains = chains, br.obs = obs, br.temb = (const float*)(pk + L.temb), br.ksteps = ksteps;
  br.Kft = Kft, br.AF = d.act_flat, br.td = d.time_dim, br.cond = d.cond_dim, br.M = M, br.obs_in_a = 1;
  br.inA = B.in, br.KpA = L.Kp0, br.brow = brow, br.krow = krow, br.onehot0 = -1;
  if (d.cond_hidden > 0) br.obs_in_a = 0, br.inC = B.cin, br.KpC = L.Kpc;
  launch_build_rows<P>(br, s);
  if (d.cond_hidden > 0) cond_encode<P>(d, prm, pk, L, M, B.cin, B, B.in, nullptr, 0, false, s);
  mlp_forward<P>(d, prm, pk, L, M, B, false, s);
  LogprobArgs la;
  la.eps = B.out, la.lde = B.ldout, la.chains = chains, la.ksteps = ksteps, la.cfg = cfg, la.Kft = Kft;
  la.AF = d.act_flat, la.M = M, la.logp = logp;
  launch_logprob(la, s);
  return check_launch();
}

int dppo_chain_logprob(const dppo_net_desc* actor, int prec, const float* params, const void* packed,
                       const dppo_diffusion_cfg* cfg, const dppo_step* ksteps, int Kft, const float* obs,
                       const float* chains, int64_t B, float* logprobs, void* workspace, int64_t workspace_bytes,
                       dppo_stream_t stream) {
  if (int e = check_net(actor)) return e;
  if (int e = check_prec(prec)) return e;
  if (actor->kind != 0) return fail(-1, "dppo_chain_logprob needs an actor descriptor");
  if (!params || !packed || !cfg || !ksteps || !obs || !chains || !logprobs || !workspace) return fail(-1, "null pointer");
  if (B < 1 || Kft < 1 || B * Kft > 0x7fffffff) return fail(-1, "B*Kft out of range");
#define CALL(P)                                                                                                 \
  logprob_impl<P>(*actor, params, (const char*)packed, *cfg, ksteps, Kft, obs, chains, B, logprobs, workspace, workspace_bytes, \
                  (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- behaviour-cloning term ----------------------------------------------------------------------------
template <class P>
static size_t carve_bc(Carver& c, const dppo_net_desc& d, int64_t M, MlpBufs<P>& B, int32_t*& brow, int32_t*& krow,
                       double** partial = nullptr) {
  carve_mlp<P>(c, d, M, true, true, B);
  brow = (int32_t*)c.take((size_t)M * 4);
  krow = (int32_t*)c.take((size_t)M * 4);
  double* pp = (double*)c.take((size_t)(bc_loss_blocks(M, pack_layout<P>(d, 0).Kpo) + 1) * sizeof(double));
  if (partial) *partial = pp;
  return al256(c.off);
}
int64_t dppo_bc_loss_workspace_bytes(const dppo_net_desc* actor, int prec, int64_t B, int Kft) {
  if (check_net(actor) || check_prec(prec)) return -1;
  if (B < 1 || Kft < 1 || B * Kft > 0x7fffffff) return fail(-1, "B*Kft out of range");
  if (Kft > 1024 || (int64_t)Kft * actor->time_dim > 65536 ||
      time_backward_lds_bytes(Kft, actor->time_dim) > 156 * 1024)
    return fail(-1, "Kft * time_dim = %d too large for the time-embedding backward (LDS)", Kft * actor->time_dim);
  return ws_bytes(prec, [&](Carver& c, auto p) {
    MlpBufs<decltype(p)> W;
    int32_t *br, *kr;
    return carve_bc<decltype(p)>(c, *actor, B * Kft, W, br, kr);
  });
}
// Behaviour cloning and the supervised denoising loss are one pipeline: rows -> cond_encode -> forward -> loss -> backward ->
// cond_backward (-> obs_grad).  `br` arrives with the caller's row sources (chains or pairs / kinds, obs); loss(B, L, partial)
// launches the caller's loss, from B.out into B.d_out.
template <class P, class Loss>
static int denoise_train(const dppo_net_desc& d, const float* prm, const char* pk, BuildRows br, const dppo_step* steps, int Kft,
                         int64_t M, float* grad, float* d_obs, void* ws, int64_t wsb, hipStream_t s, Loss loss) {
  Carver c{(char*)ws, 0, (size_t)wsb};
  MlpBufs<P> B;
  int32_t *brow, *krow;
  double* partial;
  const size_t need = carve_bc<P>(c, d, M, B, brow, krow, &partial);
  if ((int64_t)need > wsb) return fail(-1, "workspace too small: need %zu bytes, got %lld", need, (long long)wsb);
  if (int e = plan_route<P>(d, M, Kft, DPPO_ROUTE_IN_SIDE | (d_obs ? DPPO_ROUTE_IN_DOBS : 0), B)) return e;
  const PackLayout L = pack_layout<P>(d, 0);
  br.temb = (const float*)(pk + L.temb), br.ksteps = steps;
  br.Kft = Kft, br.AF = d.act_flat, br.td = d.time_dim, br.cond = d.cond_dim, br.M = M, br.obs_in_a = 1;
  br.inA = B.in, br.KpA = L.Kp0, br.brow = brow, br.krow = krow, br.onehot0 = B.route.onehot_col;
  if (d.cond_hidden > 0) br.obs_in_a = 0, br.inC = B.cin, br.KpC = L.Kpc;
  launch_build_rows<P>(br, s);
  if (d.cond_hidden > 0) cond_encode<P>(d, prm, pk, L, M, B.cin, B, B.in, nullptr, 0, true, s);
  mlp_forward<P>(d, prm, pk, L, M, B, true, s);
  loss(B, L, partial);
  mlp_backward<P>(d, prm, pk, L, M, B, grad, krow, steps, Kft, s);
  if (d.cond_hidden > 0) cond_backward<P>(d, prm, pk, L, M, B, B.dh0_final, B.cin, grad, s);
  if (d_obs) obs_grad<P>(d, prm, M, B, d_obs, s);
  return check_launch();
}
template <class P>
static int bc_impl(const dppo_net_desc& d, const float* prm, const char* pk, const dppo_diffusion_cfg& cfg,
                   const dppo_step* ksteps, int Kft, const float* obs, const float* chains, int64_t Bn, float* grad,
                   double* loss, void* ws, int64_t wsb, hipStream_t s) {
  const int64_t M = Bn * Kft;
  BuildRows br;
  memset(&br, 0, sizeof(br));
  br.chains = chains, br.obs = obs;
  return denoise_train<P>(d, prm, pk, br, ksteps, Kft, M, grad, nullptr, ws, wsb, s,
                          [&](MlpBufs<P>& B, const PackLayout& L, double* partial) {
                            BcArgs ba;
                            ba.eps = B.out, ba.lde = B.ldout, ba.chains = chains, ba.ksteps = ksteps, ba.cfg = cfg, ba.Kft = Kft;
                            ba.AF = d.act_flat, ba.M = M, ba.d_eps = B.d_out, ba.ldde = L.Kpo, ba.loss = loss, ba.partial = partial;
                            launch_bc_loss<P>(ba, s);
                          });
}
int dppo_bc_loss_fwd_bwd(const dppo_net_desc* actor, int prec, const float* params, const void* packed,
                         const dppo_diffusion_cfg* cfg, const dppo_step* ksteps, int Kft, const float* obs,
                         const float* chains, int64_t B, float* grad, double* loss, void* workspace,
                         int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_net(actor)) return e;
  if (int e = check_prec(prec)) return e;
  if (actor->kind != 0) return fail(-1, "dppo_bc_loss_fwd_bwd needs an actor descriptor");
  if (!params || !packed || !cfg || !ksteps || !obs || !chains || !grad || !loss || !workspace) return fail(-1, "null pointer");
  if (B < 1 || Kft < 1 || B * Kft > 0x7fffffff) return fail(-1, "B*Kft out of range");
  if (Kft > 1024) return fail(-1, "Kft out of range");
  if ((int64_t)Kft * actor->time_dim > 65536 || time_backward_lds_bytes(Kft, actor->time_dim) > 156 * 1024)
    return fail(-1, "Kft * time_dim = %d too large for the time-embedding backward (LDS)", Kft * actor->time_dim);
#define CALL(P)                                                                                                       \
  bc_impl<P>(*actor, params, (const char*)packed, *cfg, ksteps, Kft, obs, chains, B, grad, loss, workspace, workspace_bytes, \
             (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
int dppo_axpy(float* y, const float* x, double alpha, int64_t n, dppo_stream_t stream) {
  if (!y || !x || n < 0) return fail(-1, "bad argument");
  launch_axpy(y, x, (float)alpha, n, (hipStream_t)stream);
  return check_launch();
}

// ---- supervised denoising loss (pre-training) ------------------------------------------------------------
int64_t dppo_denoise_mse_workspace_bytes(const dppo_net_desc* actor, int prec, int64_t N) {
  return dppo_bc_loss_workspace_bytes(actor, prec, N, 1);
}
template <class P>
static int mse_impl(const dppo_net_desc& d, const float* prm, const char* pk, const dppo_step* tsteps, int n_time,
                    const float* obs, const float* pairs, const int64_t* kinds, int64_t M, float* grad, double* loss,
                    void* ws, int64_t wsb, hipStream_t s, float* d_obs = nullptr) {
  BuildRows br;  // gathered mode: row n = (pairs[n][0], temb(tsteps[kinds[n]].t), obs[n])
  memset(&br, 0, sizeof(br));
  br.kinds = kinds, br.chains = pairs, br.obs = obs;
  return denoise_train<P>(d, prm, pk, br, tsteps, n_time, M, grad, d_obs, ws, wsb, s,
                          [&](MlpBufs<P>& B, const PackLayout& L, double* partial) {
                            MseArgs ma;
                            ma.eps = B.out, ma.lde = B.ldout, ma.pairs = pairs, ma.AF = d.act_flat, ma.M = M, ma.d_eps = B.d_out;
                            ma.ldde = L.Kpo, ma.loss = loss, ma.partial = partial;
                            launch_mse_loss<P>(ma, s);
                          });
}
static int mse_entry(const dppo_net_desc* actor, int prec, const float* params, const void* packed,
                             const dppo_step* tsteps, int n_time, const float* obs, const float* pairs,
                             const int64_t* kinds, int64_t N, float* grad, double* loss, void* workspace,
                             int64_t workspace_bytes, dppo_stream_t stream, float* d_obs) {
  if (int e = check_net(actor)) return e;
  if (int e = check_prec(prec)) return e;
  if (actor->kind != 0) return fail(-1, "dppo_denoise_mse_fwd_bwd needs an actor descriptor");
  if (d_obs && actor->cond_hidden > 0) return fail(-1, "d_obs with a cond_mlp actor is not built");
  if (!params || !packed || !tsteps || !obs || !pairs || !kinds || !grad || !loss || !workspace)
    return fail(-1, "null pointer");
  if (N < 1 || N > 0x7fffffff || n_time < 1 || n_time > 1024) return fail(-1, "N / n_time out of range");
  if (time_backward_lds_bytes(n_time, actor->time_dim) > 156 * 1024)
    return fail(-1, "n_time * time_dim = %d too large for the time-embedding backward (LDS)", n_time * actor->time_dim);
#define CALL(P)                                                                                                        \
  mse_impl<P>(*actor, params, (const char*)packed, tsteps, n_time, obs, pairs, kinds, N, grad, loss, workspace, \
              workspace_bytes, (hipStream_t)stream, d_obs)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
int dppo_denoise_mse_fwd_bwd(const dppo_net_desc* actor, int prec, const float* params, const void* packed,
                             const dppo_step* tsteps, int n_time, const float* obs, const float* pairs,
                             const int64_t* kinds, int64_t N, float* grad, double* loss, void* workspace,
                             int64_t workspace_bytes, dppo_stream_t stream) {
  return mse_entry(actor, prec, params, packed, tsteps, n_time, obs, pairs, kinds, N, grad, loss, workspace, workspace_bytes,
                   stream, nullptr);
}
int dppo_denoise_mse_fwd_bwd_obs(const dppo_net_desc* actor, int prec, const float* params, const void* packed,
                                 const dppo_step* tsteps, int n_time, const float* obs, const float* pairs,
                                 const int64_t* kinds, int64_t N, float* grad, double* loss, void* workspace,
                                 int64_t workspace_bytes, dppo_stream_t stream, float* d_obs) {
  if (!d_obs) return fail(-1, "null pointer");
  return mse_entry(actor, prec, params, packed, tsteps, n_time, obs, pairs, kinds, N, grad, loss, workspace, workspace_bytes,
                   stream, d_obs);
}

// ---- GAE ---------------------------------------------------------------------------------------------
int dppo_gae(const double* reward, const float* values, const float* terminated, const float* last_values, int n_steps,
             int n_envs, double gamma, double gae_lambda, double reward_scale_const, double* adv64, double* ret64,
             float* adv32, float* ret32, dppo_stream_t stream) {
  if (!reward || !values || !terminated || !last_values) return fail(-1, "null pointer");
  if (n_steps < 1 || n_envs < 1) return fail(-1, "empty rollout");
  launch_gae(reward, values, terminated, last_values, n_steps, n_envs, gamma, gae_lambda, reward_scale_const, adv64,
             ret64, adv32, ret32, (hipStream_t)stream);
  return check_launch();
}

// ---- PPO update --------------------------------------------------------------------------------------
template <class P>
struct PpoWs {
  MlpBufs<P> A, C;
  int32_t *brow, *krow;
  int32_t* brow_c;  // the critic pipeline's own copy of brow (it builds its rows on its own stream)
  double* moments;
  float* loss_tab;  // [2 Kft], Kft <= 1024
  double* loss_partial;
  double* loss_partial_v;  // the value half's, when it runs on the critic's stream
};
template <class P>
static size_t carve_ppo(Carver& c, const dppo_net_desc& a, const dppo_net_desc& cr, int64_t N, PpoWs<P>& W) {
  W.moments = (double*)c.take((8 + 2 * ADV_MOMENT_BLOCKS) * sizeof(double));
  W.loss_tab = (float*)c.take(2 * 1024 * sizeof(float));
  W.loss_partial = (double*)c.take((size_t)loss_blocks(N) * 8 * sizeof(double));
  W.loss_partial_v = (double*)c.take((size_t)loss_blocks(N) * 8 * sizeof(double));
  W.brow = (int32_t*)c.take((size_t)N * 4);
  W.brow_c = (int32_t*)c.take((size_t)N * 4);
  W.krow = (int32_t*)c.take((size_t)N * 4);
  carve_mlp<P>(c, a, N, true, true, W.A);
  carve_mlp<P>(c, cr, N, true, true, W.C);
  return al256(c.off);
}
int64_t dppo_ppo_workspace_bytes(const dppo_net_desc* actor, const dppo_net_desc* critic, int prec, int64_t N) {
  if (check_net(actor) || check_net(critic) || check_prec(prec)) return -1;
  if (N < 2 || N > 0x7fffffff) return fail(-1, "N out of range");
  return ws_bytes(prec, [&](Carver& c, auto p) {
    PpoWs<decltype(p)> W;
    return carve_ppo<decltype(p)>(c, *actor, *critic, N, W);
  });
}

// Tuning knob 42: the policy half of the PPO loss in the epilogue of the actor's fused forward, spread over the workgroup
// (loss_dev.h; fused.hip, LOSSF): no loss launch between the actor's forward and backward, the forward's eps tile never goes to
// HBM.  What takes it (everything else keeps the separate launch): bf16; the merged one-block forward with one out tile and
// 64-row tiles (hidden 512, a head of at most 16 outputs = the action chunk, so cnt <= 16); the value half on the critic's own
// stream; no advantage-moment riders (their partial sums are added by the loss launch's block 0).  The per-step tables in LDS
// bound Kft at 64.  dppo_ppo_loss_route() exports the answer.
static int g_fuse_loss = 1;
template <class P>
static bool fuse_loss_ok(const dppo_net_desc& d, int64_t N, bool has_gmom, bool two_streams, int Kft) {
  if (!g_fuse_loss || P::ESIZE != 2 || !two_streams || mom_rider_on(N, has_gmom)) return false;
  if (!fused_ok<P>(d) || !fused_can_merge<P>(d) || !fused_loss_shape(d, Kft)) return false;
  return d.kind == 0 && d.out_dim == d.act_flat && d.act_flat <= 16 && pack_layout<P>(d, 0).Kpo % 8 == 0;
}

template <class P>
static int ppo_impl(const dppo_net_desc& a, const dppo_net_desc& cr, const float* ap, const char* ak, const float* cp,
                    const char* ck, const dppo_diffusion_cfg& dcfg, const dppo_ppo_cfg& pcfg, const dppo_step* ksteps,
                    const float* obs_k, const float* chains_k, const float* returns_k, const float* values_k,
                    const float* adv_k, const float* logprobs_k, const int64_t* inds, const int64_t* kinds, int64_t N,
                    const double* gmom, float* agrad, float* cgrad, double* stats, void* ws, int64_t wsb, hipStream_t s,
                    const dppo_obs_io* oio = nullptr, const dppo_dp_hook* hook = nullptr) {
  Carver c{(char*)ws, 0, (size_t)wsb};
  PpoWs<P> W;
  const size_t need = carve_ppo<P>(c, a, cr, N, W);
  if ((int64_t)need > wsb) return fail(-1, "workspace too small: need %zu bytes, got %lld", need, (long long)wsb);
  const PackLayout LA = pack_layout<P>(a, 0), LC = pack_layout<P>(cr, 0);
  const int Kft = pcfg.ft_denoising_steps;
  // (the row builders below zero both networks' counters; only the actor's tail has a side stream)
  const int dobs_a = oio && oio->d_obs_actor ? DPPO_ROUTE_IN_DOBS : 0, dobs_c = oio && oio->d_obs_critic ? DPPO_ROUTE_IN_DOBS : 0;
  if (int e = plan_route<P>(a, N, Kft, DPPO_ROUTE_IN_ZEROED | DPPO_ROUTE_IN_SIDE | dobs_a, W.A)) return e;
  if (int e = plan_route<P>(cr, N, Kft, DPPO_ROUTE_IN_ZEROED | dobs_c, W.C)) return e;
  // The critic pipeline (rows -> forward -> value loss -> backward -> weight gradients) and the actor pipeline (rows ->
  // advantage moments -> forward -> policy loss -> ...) share nothing but the call's inputs: one fork at entry, one join
  // at the end.  A cross-stream event hop costs 10-17 us of device idle time; at entry it hides behind the actor's row
  // builder, and the loss is evaluated as two launches rather than joining the streams in the middle of the call.
  // (With a cond_mlp the actor's encoder reads the critic's observation rows: the row builder then stays one launch.)
  const bool own_rows = a.cond_hidden == 0;
  hipStream_t s2 = own_rows ? fork_side(s) : s;
  BuildRows br;
  memset(&br, 0, sizeof(br));
  br.zero_b = W.moments, br.n_zero_b = 32;  // zeroed by the row builder (every statistic has one owner launch that writes it)
  // post_reduce_kernel's arrival counter and, behind it, tail_post_kernel's (both networks')
  br.zero_a = W.A.post_counter, br.n_zero_a = POST_COUNTER_DOUBLES;
  br.zero_c = W.C.post_counter, br.n_zero_c = POST_COUNTER_DOUBLES;
  if (Kft <= 1024) br.loss_tab = W.loss_tab, br.pcfg = pcfg;
  br.inds = inds, br.kinds = kinds, br.chains = chains_k, br.obs = obs_k, br.temb = (const float*)(ak + LA.temb);
  br.ksteps = ksteps;
  br.Kft = Kft, br.AF = a.act_flat, br.td = a.time_dim, br.cond = a.cond_dim, br.M = N;
  br.inA = W.A.in, br.KpA = LA.Kp0, br.inC = W.C.in, br.KpC = LC.Kp0, br.brow = W.brow, br.krow = W.krow;
  br.obs_in_a = a.cond_hidden > 0 ? 0 : 1;  // with cond_mlp the encoder fills the state columns (from the critic's obs rows)
  br.onehot0 = W.A.route.onehot_col;
  // advantage moments as riders of the actor's row builder (knob 36): no launch between the rows and the actor's forward
  const bool mom_rider = mom_rider_on(N, gmom != nullptr);
  if (mom_rider) br.mom_adv = adv_k, br.mom_out = W.moments, br.n_zero_b = 8;  // (block 0 must not zero the riders' slots, [8, ...))
  const float* obs_c = oio && oio->obs_critic ? oio->obs_critic : nullptr;  // the critic's own observation rows (pixel nets)
  const bool split = s2 != s || obs_c != nullptr;
  if (split) {
    BuildRows bc = br;  // critic rows only, on the critic's stream
    bc.zero_a = bc.zero_b = nullptr, bc.n_zero_a = bc.n_zero_b = 0, bc.loss_tab = nullptr, bc.mom_adv = nullptr;
    br.zero_c = nullptr, br.n_zero_c = 0;  // (the critic's row builder zeroes the critic's counters: its own stream's order)
    bc.inA = nullptr, bc.brow = W.brow_c, bc.krow = nullptr;
    if (obs_c) bc.obs = obs_c;
    bc.cond = cr.cond_dim;
    launch_build_rows<P>(bc, s2);
    br.inC = nullptr;
  }
  launch_build_rows<P>(br, s);
  if (a.cond_hidden > 0) cond_encode<P>(a, ap, ak, LA, N, W.C.in, W.A, W.A.in, nullptr, 0, true, s);
  if (gmom == nullptr && !mom_rider) launch_adv_moments(adv_k, W.brow, N, W.moments, s);
  if (!own_rows) s2 = fork_side(s);
  LossArgs la;
  memset(&la, 0, sizeof(la));
  la.eps = W.A.out, la.lde = W.A.ldout, la.vnew = W.C.out, la.ldv = W.C.ldout, la.brow = W.brow, la.krow = W.krow;
  la.gathered = kinds != nullptr;
  la.chains = chains_k, la.logprobs_k = logprobs_k, la.returns_k = returns_k, la.values_k = values_k, la.adv_k = adv_k;
  la.ksteps = ksteps, la.dcfg = dcfg, la.pcfg = pcfg, la.AF = a.act_flat, la.N = N;
  la.moments = gmom ? gmom : W.moments;
  if (mom_rider) la.mom_blocks = ADV_RIDER_BLOCKS, la.moments_out = W.moments;
  la.tab = Kft <= 1024 ? W.loss_tab : nullptr;
  la.d_eps = W.A.d_out, la.ldde = LA.Kpo, la.d_v = W.C.d_out, la.lddv = LC.Kpo, la.stats = stats;
  const bool two_streams = s2 != s;
  // the policy half of the loss in the actor forward's epilogue (knob 42): its arguments as the policy launch would get them
  LossArgs lpol = la;
  lpol.part = 1, lpol.partial = W.loss_partial;
  const bool fuse_loss = fuse_loss_ok<P>(a, N, gmom != nullptr, two_streams, Kft);
  // critic half
  mlp_forward<P>(cr, cp, ck, LC, N, W.C, true, s2);
  if (two_streams) {
    la.part = 2, la.partial = W.loss_partial_v;
    if (split) la.brow = W.brow_c;
    if (gmom == nullptr) la.n_count = (double)N;  // = what adv_moments leaves in moments[2], without waiting for it
    launch_ppo_loss<P>(la, s2);
    const LossArgs lv = la;
    la.brow = W.brow, la.n_count = 0;
    // (no tail stream of its own: a fork from a forked stream crashes hipGraph capture on ROCm 7.0 at capture end, and
    // the critic's tail is one 10-us reduction)
    mlp_backward<P>(cr, cp, ck, LC, N, W.C, cgrad, nullptr, nullptr, 0, s2, &lv);
    if (oio && oio->d_obs_critic) obs_grad<P>(cr, cp, N, W.C, oio->d_obs_critic, s2);
    // data parallel: everything that writes critic_grad is enqueued on s2 -- the caller queues the critic slice's
    // all-reduce behind it THERE, so that it runs while the actor's forward / backward still occupy the main stream
    if (hook && hook->critic_grads_enqueued) hook->critic_grads_enqueued(hook->user, (dppo_stream_t)s2);
  }
  // actor half
  mlp_forward<P>(a, ap, ak, LA, N, W.A, true, s, fuse_loss ? &lpol : nullptr);
  la.part = two_streams ? 1 : 3, la.partial = W.loss_partial;
  if (!fuse_loss) launch_ppo_loss<P>(la, s);
  if (!two_streams) {
    mlp_backward<P>(cr, cp, ck, LC, N, W.C, cgrad, nullptr, nullptr, 0, s);
    if (oio && oio->d_obs_critic) obs_grad<P>(cr, cp, N, W.C, oio->d_obs_critic, s);
    if (hook && hook->critic_grads_enqueued) hook->critic_grads_enqueued(hook->user, (dppo_stream_t)s);
  }
  if (two_streams && g_early_join) W.A.join_s[W.A.n_join] = s2, W.A.join_idx[W.A.n_join++] = 0;
  mlp_backward<P>(a, ap, ak, LA, N, W.A, agrad, W.krow, ksteps, Kft, s, &la);
  if (a.cond_hidden > 0) cond_backward<P>(a, ap, ak, LA, N, W.A, W.A.dh0_final, W.C.in, agrad, s);
  if (oio && oio->d_obs_actor) obs_grad<P>(a, ap, N, W.A, oio->d_obs_actor, s);
  if (!(two_streams && g_early_join) || W.A.n_join > 0) join_side(s, s2);  // (n_join > 0: the backward never flushed)
  W.A.n_join = 0;
  return check_launch();
}

static bool hipStreamIsCapturing_safe(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}
static int check_obs_io(const dppo_obs_io* io, const int64_t* kinds, bool actor_has_encoder) {
  if (!io) return 0;
  if (kinds == nullptr) return fail(-1, "the _obs entries take pre-gathered samples (kinds), one observation row per sample");
  if (actor_has_encoder && (io->obs_critic || io->d_obs_actor)) return fail(-1, "d_obs / obs_critic with a cond_mlp actor is not built");
  return 0;
}
static int ppo_entry(const dppo_net_desc* actor, const dppo_net_desc* critic, int prec, const float* actor_params,
                          const void* actor_packed, const float* critic_params, const void* critic_packed,
                          const dppo_diffusion_cfg* dcfg, const dppo_ppo_cfg* pcfg, const dppo_step* ksteps,
                          const float* obs_k, const float* chains_k, const float* returns_k, const float* values_k,
                          const float* adv_k, const float* logprobs_k, const int64_t* inds, const int64_t* kinds,
                          int64_t N, const double* global_moments, float* actor_grad, float* critic_grad,
                          double* stats, void* workspace, int64_t workspace_bytes, dppo_stream_t stream, const dppo_obs_io* io,
                          const dppo_dp_hook* hook = nullptr) {
  if (int e = check_net(actor)) return e;
  if (int e = check_net(critic)) return e;
  if (int e = check_prec(prec)) return e;
  if (actor->kind != 0 || critic->kind != 1 || critic->out_dim != 1)
    return fail(-1, "descriptor kinds must be (actor, critic with out_dim 1)");
  if (actor->cond_dim != critic->cond_dim && !(io && io->obs_critic))
    return fail(-1, "actor and critic observe different cond_dim");
  if (!actor_params || !actor_packed || !critic_params || !critic_packed || !dcfg || !pcfg || !ksteps || !obs_k ||
      !chains_k || !returns_k || !values_k || !adv_k || !logprobs_k || !actor_grad || !critic_grad || !stats ||
      !workspace)
    return fail(-1, "null pointer");
  if (int e = check_obs_io(io, kinds, actor->cond_hidden > 0)) return e;
  if ((inds == nullptr) == (kinds == nullptr)) return fail(-1, "pass exactly one of inds (rollout mode) / kinds (gathered mode)");
  if (N < 2 || N > 0x7fffffff) return fail(-1, "N out of range");
  if (pcfg->ft_denoising_steps < 1 || pcfg->ft_denoising_steps > 1024) return fail(-1, "Kft out of range");
  if ((int64_t)pcfg->ft_denoising_steps * actor->time_dim > 65536 ||
      time_backward_lds_bytes(pcfg->ft_denoising_steps, actor->time_dim) > 156 * 1024)
    return fail(-1, "Kft * time_dim too large");
  if (pcfg->horizon_steps * pcfg->action_dim != actor->act_flat) return fail(-1, "Ta*Da != act_flat");
  if (pcfg->reward_horizon < 1) return fail(-1, "reward_horizon must be >= 1");
#define CALL(P)                                                                                                        \
  ppo_impl<P>(*actor, *critic, actor_params, (const char*)actor_packed, critic_params, (const char*)critic_packed, *dcfg,     \
              *pcfg, ksteps, obs_k, chains_k, returns_k, values_k, adv_k, logprobs_k, inds, kinds, N, global_moments, actor_grad, critic_grad, stats, \
              workspace, workspace_bytes, (hipStream_t)stream, io, hook)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
int dppo_ppo_loss_fwd_bwd_dp(const dppo_net_desc* actor, const dppo_net_desc* critic, int prec, const float* actor_params,
                             const void* actor_packed, const float* critic_params, const void* critic_packed,
                             const dppo_diffusion_cfg* dcfg, const dppo_ppo_cfg* pcfg, const dppo_step* ksteps,
                             const float* obs_k, const float* chains_k, const float* returns_k, const float* values_k,
                             const float* adv_k, const float* logprobs_k, const int64_t* inds, const int64_t* kinds,
                             int64_t N, const double* global_moments, float* actor_grad, float* critic_grad,
                             double* stats, void* workspace, int64_t workspace_bytes, dppo_stream_t stream,
                             const dppo_dp_hook* hook) {
  if (hipStreamIsCapturing_safe((hipStream_t)stream) && hook && hook->critic_grads_enqueued)
    return fail(-1, "dppo_ppo_loss_fwd_bwd_dp: a collective cannot be queued from inside a stream capture");
  return ppo_entry(actor, critic, prec, actor_params, actor_packed, critic_params, critic_packed, dcfg, pcfg, ksteps, obs_k,
                   chains_k, returns_k, values_k, adv_k, logprobs_k, inds, kinds, N, global_moments, actor_grad, critic_grad,
                   stats, workspace, workspace_bytes, stream, nullptr, hook);
}
int dppo_ppo_loss_fwd_bwd(const dppo_net_desc* actor, const dppo_net_desc* critic, int prec, const float* actor_params,
                          const void* actor_packed, const float* critic_params, const void* critic_packed,
                          const dppo_diffusion_cfg* dcfg, const dppo_ppo_cfg* pcfg, const dppo_step* ksteps,
                          const float* obs_k, const float* chains_k, const float* returns_k, const float* values_k,
                          const float* adv_k, const float* logprobs_k, const int64_t* inds, const int64_t* kinds,
                          int64_t N, const double* global_moments, float* actor_grad, float* critic_grad,
                          double* stats, void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  return ppo_entry(actor, critic, prec, actor_params, actor_packed, critic_params, critic_packed, dcfg, pcfg, ksteps, obs_k,
                   chains_k, returns_k, values_k, adv_k, logprobs_k, inds, kinds, N, global_moments, actor_grad, critic_grad,
                   stats, workspace, workspace_bytes, stream, nullptr);
}
int dppo_ppo_loss_fwd_bwd_obs(const dppo_net_desc* actor, const dppo_net_desc* critic, int prec, const float* actor_params,
                              const void* actor_packed, const float* critic_params, const void* critic_packed,
                              const dppo_diffusion_cfg* dcfg, const dppo_ppo_cfg* pcfg, const dppo_step* ksteps,
                              const float* obs_k, const float* chains_k, const float* returns_k, const float* values_k,
                              const float* adv_k, const float* logprobs_k, const int64_t* kinds, int64_t N,
                              const double* global_moments, float* actor_grad, float* critic_grad, double* stats,
                              void* workspace, int64_t workspace_bytes, dppo_stream_t stream, const dppo_obs_io* io) {
  if (!io) return fail(-1, "null pointer");
  return ppo_entry(actor, critic, prec, actor_params, actor_packed, critic_params, critic_packed, dcfg, pcfg, ksteps, obs_k,
                   chains_k, returns_k, values_k, adv_k, logprobs_k, nullptr, kinds, N, global_moments, actor_grad, critic_grad,
                   stats, workspace, workspace_bytes, stream, io);
}

// ---- Gaussian-policy PPO (gaussian.hip) ----------------------------------------------------------------------
static int check_gauss(const dppo_net_desc* actor, const dppo_gaussian_cfg* cfg, const float* logvar) {
  if (int e = check_net(actor)) return e;
  if (actor->kind != 1) return fail(-1, "the Gaussian actor is a kind-1 (observation trunk) descriptor");
  if (!cfg) return fail(-1, "null cfg");
  if (cfg->horizon_steps * cfg->action_dim != actor->out_dim) return fail(-1, "Ta*Da != actor out_dim");
  if (cfg->std_mode != 0 && cfg->std_mode != 1) return fail(-1, "std_mode must be 0 (fixed) or 1 (learned per dimension)");
  if (cfg->std_mode == 1 && !logvar) return fail(-1, "std_mode 1 needs logvar");
  if (cfg->std_mode == 0 && !(cfg->fixed_std > 0)) return fail(-1, "fixed_std must be positive");
  return 0;
}
// what the two training entries (PPO, behaviour cloning) refuse on top of check_gauss(); the inference entries take any Ta*Da
static int check_gauss_train(const dppo_net_desc* actor, const dppo_gaussian_cfg* cfg, const float* logvar_grad) {
  if (cfg->std_mode == 1 && !logvar_grad) return fail(-1, "std_mode 1 needs logvar_grad");
  if (cfg->std_mode == 1 && actor->out_dim > 768)
    return fail(-1, "Ta * Da above 768 with a learned std (the logvar terms of one block live in shared memory)");
  return 0;
}
template <class P>
static size_t carve_gauss(Carver& c, const dppo_net_desc& a, const dppo_net_desc* cr, int64_t N, bool train, MlpBufs<P>& A,
                          MlpBufs<P>& Cb, double*& moments, double*& scratch, double*& partial) {
  moments = (double*)c.take(4 * sizeof(double));
  scratch = (double*)c.take(2 * 64 * sizeof(double));
  partial = (double*)c.take((size_t)gauss_blocks(N) * (8 + a.out_dim) * sizeof(double));
  carve_mlp<P>(c, a, N, train, train, A);
  if (cr) carve_mlp<P>(c, *cr, N, train, train, Cb);
  return al256(c.off);
}
int64_t dppo_gaussian_workspace_bytes(const dppo_net_desc* actor, const dppo_net_desc* critic, int prec, int64_t N) {
  if (check_net(actor) || (critic && check_net(critic)) || check_prec(prec)) return -1;
  if (int e = check_rows(N)) return e;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    MlpBufs<decltype(p)> A, Cb;
    double *m, *sc, *pa;
    return carve_gauss<decltype(p)>(c, *actor, critic, N, critic != nullptr, A, Cb, m, sc, pa);
  });
}
template <class P>
static int gauss_infer_impl(const dppo_net_desc& d, const float* prm, const char* pk, const dppo_gaussian_cfg& cfg,
                            const float* logvar, const float* obs, const float* noise, const float* actions, int64_t N,
                            float* out_actions, float* out_mean, float* out_logp, void* ws, int64_t wsb, hipStream_t s,
                            const dppo_dropout* drop = nullptr) {
  MlpBufs<P> A, Cb;
  double *m, *sc, *pa;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_gauss<P>(c, d, nullptr, N, false, A, Cb, m, sc, pa); }, true)) return e;
  const PackLayout L = pack_layout<P>(d, 0);
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, d.cond_dim, N, A.in, L.Kp0, s);
  mlp_forward<P>(d, prm, pk, L, N, A, false, s, nullptr, false, drop);
  GaussArgs g;
  memset(&g, 0, sizeof(g));
  g.cfg = cfg, g.mean_pre = A.out, g.ldm = A.ldout, g.logvar = logvar, g.N = N, g.AF = d.out_dim;
  if (out_actions) {
    g.noise = noise, g.out_actions = out_actions, g.out_mean = out_mean;
    launch_gauss_sample(g, s);
  } else {
    g.actions = actions, g.out_logp = out_logp;
    launch_gauss_logprob(g, s);
  }
  return check_launch();
}
int dppo_gaussian_sample(const dppo_net_desc* actor, int prec, const float* params, const void* packed,
                         const dppo_gaussian_cfg* cfg, const float* logvar, const float* obs, const float* noise,
                         int64_t B, float* actions, float* mean_out, void* workspace, int64_t workspace_bytes,
                         dppo_stream_t stream) {
  if (int e = check_gauss(actor, cfg, logvar)) return e;
  if (int e = check_prec(prec)) return e;
  if (!params || !packed || !obs || !actions) return fail(-1, "null pointer");
  if (B < 1 || B > 0x7fffffff) return fail(-1, "B out of range");
#define CALL(P)                                                                                                        \
  gauss_infer_impl<P>(*actor, params, (const char*)packed, *cfg, logvar, obs, noise, nullptr, B, actions, mean_out, nullptr, \
                      workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
// ---- dropout in a plain trunk's forward (ibrl.h) ---------------------------------------------------------------------------------
static int check_drop_actor(const dppo_net_desc* actor) {
  if (int e = check_net(actor)) return e;
  if (actor->kind != 1 || !actor->plain || actor->use_layernorm)
    return fail(-1, "dropout runs in a plain kind-1 trunk without LayerNorm only (kind = 1, plain = 1, use_layernorm = 0)");
  return 0;
}
static int check_dropout(const dppo_dropout* drop) {
  if (!drop) return fail(-1, "null pointer: the dropout struct");
  if (!(drop->p >= 0.f && drop->p < 1.f)) return fail(-1, "dropout p=%g outside [0, 1)", (double)drop->p);
  return 0;
}
int dppo_gaussian_sample_drop(const dppo_net_desc* actor, int prec, const float* params, const void* packed,
                              const dppo_gaussian_cfg* cfg, const float* logvar, const float* obs, const float* noise, int64_t B,
                              float* actions, float* mean_out, const dppo_dropout* drop, void* workspace, int64_t workspace_bytes,
                              dppo_stream_t stream) {
  if (int e = check_drop_actor(actor)) return e;
  if (int e = check_gauss(actor, cfg, logvar)) return e;
  if (int e = check_prec(prec)) return e;
  if (int e = check_dropout(drop)) return e;
  if (!params || !packed || !obs || !actions) return fail(-1, "null pointer");
  if (B < 1 || B > 0x7fffffff) return fail(-1, "B out of range");
#define CALL(P)                                                                                                        \
  gauss_infer_impl<P>(*actor, params, (const char*)packed, *cfg, logvar, obs, noise, nullptr, B, actions, mean_out, nullptr, \
                      workspace, workspace_bytes, (hipStream_t)stream, drop)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
int dppo_gaussian_logprob(const dppo_net_desc* actor, int prec, const float* params, const void* packed,
                          const dppo_gaussian_cfg* cfg, const float* logvar, const float* obs, const float* actions,
                          int64_t N, float* logp, void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_gauss(actor, cfg, logvar)) return e;
  if (int e = check_prec(prec)) return e;
  if (!params || !packed || !obs || !actions || !logp) return fail(-1, "null pointer");
  if (int e = check_rows(N)) return e;
#define CALL(P)                                                                                                        \
  gauss_infer_impl<P>(*actor, params, (const char*)packed, *cfg, logvar, obs, nullptr, actions, N, nullptr, nullptr, logp, \
                      workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
template <class P>
static int gauss_ppo_impl(const dppo_net_desc& a, const dppo_net_desc& cr, const float* ap, const char* ak, const float* cp,
                          const char* ck, const dppo_gaussian_cfg& cfg, const float* logvar, const float* obs,
                          const float* actions, const float* returns, const float* oldvalues, const float* adv,
                          const float* oldlogp, int64_t N, const double* gmom, float* agrad, float* cgrad, float* lvgrad,
                          double* stats, void* ws, int64_t wsb, hipStream_t s, const dppo_obs_io* oio = nullptr) {
  MlpBufs<P> A, Cb;
  double *moments, *scratch, *partial;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_gauss<P>(c, a, &cr, N, true, A, Cb, moments, scratch, partial); }))
    return e;
  const PackLayout LA = pack_layout<P>(a, 0), LC = pack_layout<P>(cr, 0);
  // the critic pipeline on the side stream beside the actor's forward (one fork here, one join at the end)
  hipStream_t s2 = fork_side(s);
  launch_build_direct<P>(nullptr, nullptr, oio && oio->obs_critic ? oio->obs_critic : obs, nullptr, 0, 0, cr.cond_dim, N, Cb.in,
                         LC.Kp0, s2);
  mlp_forward<P>(cr, cp, ck, LC, N, Cb, true, s2);
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, a.cond_dim, N, A.in, LA.Kp0, s);
  if (gmom == nullptr) launch_gauss_moments(adv, N, moments, scratch, s);
  mlp_forward<P>(a, ap, ak, LA, N, A, true, s);
  if (s2 != s) join_side(s, s2);  // the loss reads both outputs
  GaussArgs g;
  memset(&g, 0, sizeof(g));
  g.cfg = cfg, g.mean_pre = A.out, g.ldm = A.ldout, g.logvar = logvar, g.actions = actions, g.N = N, g.AF = a.out_dim;
  g.vnew = Cb.out, g.ldv = Cb.ldout, g.returns = returns, g.oldvalues = oldvalues, g.adv = adv, g.oldlogp = oldlogp;
  g.moments = gmom ? gmom : moments, g.d_mean = A.d_out, g.lddm = LA.Kpo, g.d_v = Cb.d_out, g.lddv = LC.Kpo;
  g.partial = partial, g.stats = stats, g.logvar_grad = lvgrad;
  launch_gauss_loss<P>(g, s);
  s2 = fork_side(s);
  mlp_backward<P>(cr, cp, ck, LC, N, Cb, cgrad, nullptr, nullptr, 0, s2);
  if (oio && oio->d_obs_critic) obs_grad<P>(cr, cp, N, Cb, oio->d_obs_critic, s2);
  mlp_backward<P>(a, ap, ak, LA, N, A, agrad, nullptr, nullptr, 0, s);
  if (oio && oio->d_obs_actor) obs_grad<P>(a, ap, N, A, oio->d_obs_actor, s);
  if (s2 != s) join_side(s, s2);
  return check_launch();
}
static int gauss_ppo_entry(const dppo_net_desc* actor, const dppo_net_desc* critic, int prec,
                                   const float* actor_params, const void* actor_packed, const float* critic_params,
                                   const void* critic_packed, const dppo_gaussian_cfg* cfg, const float* logvar,
                                   const float* obs, const float* actions, const float* returns,
                                   const float* oldvalues, const float* adv, const float* oldlogp, int64_t N,
                                   const double* global_moments, float* actor_grad, float* critic_grad,
                                   float* logvar_grad, double* stats, void* workspace, int64_t workspace_bytes,
                                   dppo_stream_t stream, const dppo_obs_io* io) {
  if (int e = check_gauss(actor, cfg, logvar)) return e;
  if (int e = check_net(critic)) return e;
  if (int e = check_prec(prec)) return e;
  if (critic->kind != 1 || critic->out_dim != 1) return fail(-1, "critic descriptor must be kind 1 with out_dim 1");
  if (actor->cond_dim != critic->cond_dim && !(io && io->obs_critic))
    return fail(-1, "actor and critic observe different cond_dim");
  if (!actor_params || !actor_packed || !critic_params || !critic_packed || !obs || !actions || !returns || !oldvalues ||
      !adv || !oldlogp || !actor_grad || !critic_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_gauss_train(actor, cfg, logvar_grad)) return e;
  if (N < 2 || N > 0x7fffffff) return fail(-1, "N out of range");
#define CALL(P)                                                                                                          \
  gauss_ppo_impl<P>(*actor, *critic, actor_params, (const char*)actor_packed, critic_params, (const char*)critic_packed, *cfg, \
                    logvar, obs, actions, returns, oldvalues, adv, oldlogp, N, global_moments, actor_grad, critic_grad,       \
                    logvar_grad, stats, workspace, workspace_bytes, (hipStream_t)stream, io)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
int dppo_gaussian_ppo_loss_fwd_bwd(const dppo_net_desc* actor, const dppo_net_desc* critic, int prec,
                                   const float* actor_params, const void* actor_packed, const float* critic_params,
                                   const void* critic_packed, const dppo_gaussian_cfg* cfg, const float* logvar,
                                   const float* obs, const float* actions, const float* returns,
                                   const float* oldvalues, const float* adv, const float* oldlogp, int64_t N,
                                   const double* global_moments, float* actor_grad, float* critic_grad,
                                   float* logvar_grad, double* stats, void* workspace, int64_t workspace_bytes,
                                   dppo_stream_t stream) {
  return gauss_ppo_entry(actor, critic, prec, actor_params, actor_packed, critic_params, critic_packed, cfg, logvar, obs, actions,
                         returns, oldvalues, adv, oldlogp, N, global_moments, actor_grad, critic_grad, logvar_grad, stats,
                         workspace, workspace_bytes, stream, nullptr);
}
int dppo_gaussian_ppo_loss_fwd_bwd_obs(const dppo_net_desc* actor, const dppo_net_desc* critic, int prec,
                                       const float* actor_params, const void* actor_packed, const float* critic_params,
                                       const void* critic_packed, const dppo_gaussian_cfg* cfg, const float* logvar,
                                       const float* obs, const float* actions, const float* returns,
                                       const float* oldvalues, const float* adv, const float* oldlogp, int64_t N,
                                       const double* global_moments, float* actor_grad, float* critic_grad,
                                       float* logvar_grad, double* stats, void* workspace, int64_t workspace_bytes,
                                       dppo_stream_t stream, const dppo_obs_io* io) {
  if (!io) return fail(-1, "null pointer");
  return gauss_ppo_entry(actor, critic, prec, actor_params, actor_packed, critic_params, critic_packed, cfg, logvar, obs, actions,
                         returns, oldvalues, adv, oldlogp, N, global_moments, actor_grad, critic_grad, logvar_grad, stats,
                         workspace, workspace_bytes, stream, io);
}

// ---- Gaussian behaviour cloning (GaussianModel.loss): the training buffers of one trunk, no critic ----------------------------
int64_t dppo_gaussian_bc_workspace_bytes(const dppo_net_desc* actor, int prec, int64_t N) {
  if (check_net(actor) || check_prec(prec)) return -1;
  if (int e = check_rows(N)) return e;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    MlpBufs<decltype(p)> A, Cb;
    double *m, *sc, *pa;
    return carve_gauss<decltype(p)>(c, *actor, nullptr, N, true, A, Cb, m, sc, pa);
  });
}
template <class P>
static int gauss_bc_impl(const dppo_net_desc& a, const float* ap, const char* ak, const dppo_gaussian_cfg& cfg,
                         const float* logvar, const float* obs, const float* actions, int64_t N, double ent_coef, float* agrad,
                         float* lvgrad, double* out, void* ws, int64_t wsb, hipStream_t s) {
  MlpBufs<P> A, Cb;
  double *moments, *scratch, *partial;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_gauss<P>(c, a, nullptr, N, true, A, Cb, moments, scratch, partial); }))
    return e;
  const PackLayout LA = pack_layout<P>(a, 0);
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, a.cond_dim, N, A.in, LA.Kp0, s);
  mlp_forward<P>(a, ap, ak, LA, N, A, true, s);
  GaussArgs g;
  memset(&g, 0, sizeof(g));
  g.cfg = cfg, g.mean_pre = A.out, g.ldm = A.ldout, g.logvar = logvar, g.actions = actions, g.N = N, g.AF = a.out_dim;
  g.d_mean = A.d_out, g.lddm = LA.Kpo, g.partial = partial, g.logvar_grad = lvgrad, g.ent_coef = ent_coef, g.bc_out = out;
  launch_gauss_nll<P>(g, s);
  mlp_backward<P>(a, ap, ak, LA, N, A, agrad, nullptr, nullptr, 0, s);
  return check_launch();
}
int dppo_gaussian_bc_loss_fwd_bwd(const dppo_net_desc* actor, int prec, const float* params, const void* packed,
                                  const dppo_gaussian_cfg* cfg, const float* logvar, const float* obs, const float* actions,
                                  int64_t N, double ent_coef, float* grad, float* logvar_grad, double* loss_entropy,
                                  void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_gauss(actor, cfg, logvar)) return e;
  if (int e = check_prec(prec)) return e;
  if (!params || !packed || !obs || !actions || !grad || !loss_entropy || !workspace) return fail(-1, "null pointer");
  if (int e = check_gauss_train(actor, cfg, logvar_grad)) return e;
  if (cfg->deterministic) return fail(-1, "the behaviour-cloning loss is not defined for deterministic = 1");
  if (int e = check_rows(N)) return e;
#define CALL(P)                                                                                                              \
  gauss_bc_impl<P>(*actor, params, (const char*)packed, *cfg, logvar, obs, actions, N, ent_coef, grad, logvar_grad, loss_entropy, \
                   workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- mixture-of-Gaussians policy PPO (gmm.hip) ---------------------------------------------------------------------------
static int check_gmm(const dppo_net_desc* mean, const dppo_net_desc* wts, const dppo_gmm_cfg* cfg, const float* logvar) {
  if (int e = check_net(mean)) return e;
  if (int e = check_net(wts)) return e;
  if (!cfg) return fail(-1, "null cfg");
  if (mean->kind != 1 || wts->kind != 1) return fail(-1, "GMM trunks are kind-1 descriptors on the observation");
  if (cfg->num_modes < 1 || cfg->num_modes > GMM_MAX_MODES) return fail(-1, "num_modes out of [1, %d]", GMM_MAX_MODES);
  if (cfg->horizon_steps < 1 || cfg->action_dim < 1) return fail(-1, "bad Ta / Da");
  if (mean->out_dim != cfg->num_modes * cfg->horizon_steps * cfg->action_dim) return fail(-1, "mean trunk out_dim != num_modes * Ta * Da");
  if (wts->out_dim != cfg->num_modes) return fail(-1, "weights trunk out_dim != num_modes");
  if (mean->cond_dim != wts->cond_dim) return fail(-1, "the two trunks observe different cond_dim");
  if (cfg->std_mode != 0 && cfg->std_mode != 1) return fail(-1, "std_mode must be 0 or 1");
  if (cfg->std_mode == 1 && !logvar) return fail(-1, "std_mode 1 needs logvar");
  return 0;
}
// what the two training entries (PPO, behaviour cloning) refuse on top of check_gmm(): carve_gmm() reserves GMM_MAX_MODES x 64
// logvar columns per block of partials, and the loss kernels keep num_modes * Ta * Da floats per sample in shared memory
// (action_dim <= 64 is conservative: the carve holds any num_modes * action_dim <= GMM_MAX_MODES * 64)
static int check_gmm_train(const dppo_gmm_cfg* cfg, const float* logvar_grad) {
  if (cfg->std_mode == 1 && !logvar_grad) return fail(-1, "std_mode 1 needs logvar_grad");
  if (cfg->action_dim > 64) return fail(-1, "action_dim above 64 (the logvar partials hold %d x 64 columns)", GMM_MAX_MODES);
  if ((int64_t)cfg->num_modes * cfg->horizon_steps * cfg->action_dim > 3072)
    return fail(-1, "num_modes * Ta * Da above 3072 (the logvar terms of one block live in shared memory)");
  return 0;
}
template <class P>
static size_t carve_gmm(Carver& c, const dppo_net_desc& am, const dppo_net_desc& aw, const dppo_net_desc* cr, int64_t N, int K,
                        bool train, MlpBufs<P>& Am, MlpBufs<P>& Aw, MlpBufs<P>& Cb, double*& moments, double*& scratch,
                        double*& partial) {
  moments = (double*)c.take(4 * sizeof(double));
  scratch = (double*)c.take(2 * 64 * sizeof(double));
  partial = (double*)c.take((size_t)gmm_blocks(N) * (8 + K) * sizeof(double));
  carve_mlp<P>(c, am, N, train, train, Am);
  carve_mlp<P>(c, aw, N, train, train, Aw);
  if (cr) carve_mlp<P>(c, *cr, N, train, train, Cb);
  return al256(c.off);
}
int64_t dppo_gmm_workspace_bytes(const dppo_net_desc* mean, const dppo_net_desc* weights, const dppo_net_desc* critic, int prec,
                                 int64_t N) {
  if (check_net(mean) || check_net(weights) || (critic && check_net(critic)) || check_prec(prec)) return -1;
  if (int e = check_rows(N)) return e;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    MlpBufs<decltype(p)> Am, Aw, Cb;
    double *m, *sc, *pa;
    return carve_gmm<decltype(p)>(c, *mean, *weights, critic, N, GMM_MAX_MODES * 64, critic != nullptr, Am, Aw, Cb, m, sc, pa);
  });
}
template <class P>
static int gmm_infer_impl(const dppo_net_desc& am, const dppo_net_desc& aw, const float* mp, const char* mk, const float* wp,
                          const char* wk, const dppo_gmm_cfg& cfg, const float* logvar, const float* obs, const int64_t* modes,
                          const float* noise, const float* actions, int64_t N, float* out_actions, float* out_logp, void* ws,
                          int64_t wsb, hipStream_t s) {
  MlpBufs<P> Am, Aw, Cb;
  double *moments, *scratch, *partial;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_gmm<P>(c, am, aw, nullptr, N, GMM_MAX_MODES * 64, false, Am, Aw, Cb, moments, scratch, partial); }))
    return e;
  const PackLayout LM = pack_layout<P>(am, 0), LW = pack_layout<P>(aw, 0);
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, am.cond_dim, N, Am.in, LM.Kp0, s);
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, aw.cond_dim, N, Aw.in, LW.Kp0, s);
  mlp_forward<P>(am, mp, mk, LM, N, Am, false, s);
  mlp_forward<P>(aw, wp, wk, LW, N, Aw, false, s);
  GmmArgs g;
  memset(&g, 0, sizeof(g));
  g.cfg = cfg, g.mean_pre = Am.out, g.ldm = Am.ldout, g.logits = Aw.out, g.ldl = Aw.ldout, g.logvar = logvar, g.N = N;
  g.AF = cfg.horizon_steps * cfg.action_dim, g.modes_in = modes, g.noise = noise, g.actions = actions;
  g.out_actions = out_actions, g.out_logp = out_logp;
  if (out_actions) launch_gmm_sample(g, s);
  else launch_gmm_logprob(g, s);
  return check_launch();
}
int dppo_gmm_sample(const dppo_net_desc* mean, const dppo_net_desc* weights, int prec, const float* mean_params,
                    const void* mean_packed, const float* weights_params, const void* weights_packed, const dppo_gmm_cfg* cfg,
                    const float* logvar, const float* obs, const int64_t* modes, const float* noise, int64_t B, float* actions,
                    void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_gmm(mean, weights, cfg, logvar)) return e;
  if (int e = check_prec(prec)) return e;
  if (!mean_params || !mean_packed || !weights_params || !weights_packed || !obs || !actions || !workspace) return fail(-1, "null pointer");
  if (B < 1 || B > 0x7fffffff) return fail(-1, "B out of range");
#define CALL(P)                                                                                                                \
  gmm_infer_impl<P>(*mean, *weights, mean_params, (const char*)mean_packed, weights_params, (const char*)weights_packed, *cfg, logvar, \
                    obs, modes, noise, nullptr, B, actions, nullptr, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
int dppo_gmm_logprob(const dppo_net_desc* mean, const dppo_net_desc* weights, int prec, const float* mean_params,
                     const void* mean_packed, const float* weights_params, const void* weights_packed, const dppo_gmm_cfg* cfg,
                     const float* logvar, const float* obs, const float* actions, int64_t N, float* logp, void* workspace,
                     int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_gmm(mean, weights, cfg, logvar)) return e;
  if (int e = check_prec(prec)) return e;
  if (!mean_params || !mean_packed || !weights_params || !weights_packed || !obs || !actions || !logp || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_rows(N)) return e;
#define CALL(P)                                                                                                                \
  gmm_infer_impl<P>(*mean, *weights, mean_params, (const char*)mean_packed, weights_params, (const char*)weights_packed, *cfg, logvar, \
                    obs, nullptr, nullptr, actions, N, nullptr, logp, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
template <class P>
static int gmm_ppo_impl(const dppo_net_desc& am, const dppo_net_desc& aw, const dppo_net_desc& cr, const float* mp, const char* mk,
                        const float* wp, const char* wk, const float* cp, const char* ck, const dppo_gmm_cfg& cfg,
                        const float* logvar, const float* obs, const float* actions, const float* returns, const float* oldvalues,
                        const float* adv, const float* oldlogp, int64_t N, const double* gmom, float* mgrad, float* wgrad,
                        float* cgrad, float* lvgrad, double* stats, void* ws, int64_t wsb, hipStream_t s) {
  MlpBufs<P> Am, Aw, Cb;
  double *moments, *scratch, *partial;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_gmm<P>(c, am, aw, &cr, N, GMM_MAX_MODES * 64, true, Am, Aw, Cb, moments, scratch, partial); }))
    return e;
  const PackLayout LM = pack_layout<P>(am, 0), LW = pack_layout<P>(aw, 0), LC = pack_layout<P>(cr, 0);
  hipStream_t s2 = fork_side(s);  // the critic pipeline beside the two actor trunks
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, cr.cond_dim, N, Cb.in, LC.Kp0, s2);
  mlp_forward<P>(cr, cp, ck, LC, N, Cb, true, s2);
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, am.cond_dim, N, Am.in, LM.Kp0, s);
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, aw.cond_dim, N, Aw.in, LW.Kp0, s);
  if (gmom == nullptr) launch_gauss_moments(adv, N, moments, scratch, s);
  mlp_forward<P>(am, mp, mk, LM, N, Am, true, s);
  mlp_forward<P>(aw, wp, wk, LW, N, Aw, true, s);
  if (s2 != s) join_side(s, s2);
  GmmArgs g;
  memset(&g, 0, sizeof(g));
  g.cfg = cfg, g.mean_pre = Am.out, g.ldm = Am.ldout, g.logits = Aw.out, g.ldl = Aw.ldout, g.logvar = logvar, g.actions = actions;
  g.N = N, g.AF = cfg.horizon_steps * cfg.action_dim, g.vnew = Cb.out, g.ldv = Cb.ldout, g.returns = returns;
  g.oldvalues = oldvalues, g.adv = adv, g.oldlogp = oldlogp, g.moments = gmom ? gmom : moments;
  g.d_mean = Am.d_out, g.lddm = LM.Kpo, g.d_logits = Aw.d_out, g.lddl = LW.Kpo, g.d_v = Cb.d_out, g.lddv = LC.Kpo;
  g.partial = partial, g.stats = stats, g.logvar_grad = lvgrad;
  launch_gmm_loss<P>(g, s);
  s2 = fork_side(s);
  mlp_backward<P>(cr, cp, ck, LC, N, Cb, cgrad, nullptr, nullptr, 0, s2);
  mlp_backward<P>(am, mp, mk, LM, N, Am, mgrad, nullptr, nullptr, 0, s);
  mlp_backward<P>(aw, wp, wk, LW, N, Aw, wgrad, nullptr, nullptr, 0, s);
  if (s2 != s) join_side(s, s2);
  return check_launch();
}
int dppo_gmm_ppo_loss_fwd_bwd(const dppo_net_desc* mean, const dppo_net_desc* weights, const dppo_net_desc* critic, int prec,
                              const float* mean_params, const void* mean_packed, const float* weights_params,
                              const void* weights_packed, const float* critic_params, const void* critic_packed,
                              const dppo_gmm_cfg* cfg, const float* logvar, const float* obs, const float* actions,
                              const float* returns, const float* oldvalues, const float* adv, const float* oldlogp, int64_t N,
                              const double* global_moments, float* mean_grad, float* weights_grad, float* critic_grad,
                              float* logvar_grad, double* stats, void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_gmm(mean, weights, cfg, logvar)) return e;
  if (int e = check_net(critic)) return e;
  if (int e = check_prec(prec)) return e;
  if (critic->kind != 1 || critic->out_dim != 1) return fail(-1, "critic descriptor must be kind 1 with out_dim 1");
  if (mean->cond_dim != critic->cond_dim) return fail(-1, "actor and critic observe different cond_dim");
  if (!mean_params || !mean_packed || !weights_params || !weights_packed || !critic_params || !critic_packed || !obs || !actions ||
      !returns || !oldvalues || !adv || !oldlogp || !mean_grad || !weights_grad || !critic_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_gmm_train(cfg, logvar_grad)) return e;
  if (N < 2 || N > 0x7fffffff) return fail(-1, "N out of range");
#define CALL(P)                                                                                                                  \
  gmm_ppo_impl<P>(*mean, *weights, *critic, mean_params, (const char*)mean_packed, weights_params, (const char*)weights_packed,        \
                  critic_params, (const char*)critic_packed, *cfg, logvar, obs, actions, returns, oldvalues, adv, oldlogp, N,          \
                  global_moments, mean_grad, weights_grad, critic_grad, logvar_grad, stats, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- GMM behaviour cloning (GMMModel.loss): the training buffers of the two trunks, no critic -----------------------------------
int64_t dppo_gmm_bc_workspace_bytes(const dppo_net_desc* mean, const dppo_net_desc* weights, int prec, int64_t N) {
  if (check_net(mean) || check_net(weights) || check_prec(prec)) return -1;
  if (int e = check_rows(N)) return e;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    MlpBufs<decltype(p)> Am, Aw, Cb;
    double *m, *sc, *pa;
    return carve_gmm<decltype(p)>(c, *mean, *weights, nullptr, N, GMM_MAX_MODES * 64, true, Am, Aw, Cb, m, sc, pa);
  });
}
template <class P>
static int gmm_bc_impl(const dppo_net_desc& am, const dppo_net_desc& aw, const float* mp, const char* mk, const float* wp,
                       const char* wk, const dppo_gmm_cfg& cfg, const float* logvar, const float* obs, const float* actions,
                       int64_t N, float* mgrad, float* wgrad, float* lvgrad, double* out, void* ws, int64_t wsb, hipStream_t s) {
  MlpBufs<P> Am, Aw, Cb;
  double *moments, *scratch, *partial;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_gmm<P>(c, am, aw, nullptr, N, GMM_MAX_MODES * 64, true, Am, Aw, Cb, moments, scratch, partial); }))
    return e;
  const PackLayout LM = pack_layout<P>(am, 0), LW = pack_layout<P>(aw, 0);
  hipStream_t s2 = fork_side(s);  // the weights trunk beside the mean trunk, forward and backward
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, aw.cond_dim, N, Aw.in, LW.Kp0, s2);
  mlp_forward<P>(aw, wp, wk, LW, N, Aw, true, s2);
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, am.cond_dim, N, Am.in, LM.Kp0, s);
  mlp_forward<P>(am, mp, mk, LM, N, Am, true, s);
  if (s2 != s) join_side(s, s2);  // the loss reads both outputs
  GmmArgs g;
  memset(&g, 0, sizeof(g));
  g.cfg = cfg, g.mean_pre = Am.out, g.ldm = Am.ldout, g.logits = Aw.out, g.ldl = Aw.ldout, g.logvar = logvar, g.actions = actions;
  g.N = N, g.AF = cfg.horizon_steps * cfg.action_dim, g.d_mean = Am.d_out, g.lddm = LM.Kpo, g.d_logits = Aw.d_out, g.lddl = LW.Kpo;
  g.partial = partial, g.logvar_grad = lvgrad, g.bc_out = out;
  launch_gmm_nll<P>(g, s);
  s2 = fork_side(s);
  mlp_backward<P>(aw, wp, wk, LW, N, Aw, wgrad, nullptr, nullptr, 0, s2);
  mlp_backward<P>(am, mp, mk, LM, N, Am, mgrad, nullptr, nullptr, 0, s);
  if (s2 != s) join_side(s, s2);
  return check_launch();
}
int dppo_gmm_bc_loss_fwd_bwd(const dppo_net_desc* mean, const dppo_net_desc* weights, int prec, const float* mean_params,
                             const void* mean_packed, const float* weights_params, const void* weights_packed,
                             const dppo_gmm_cfg* cfg, const float* logvar, const float* obs, const float* actions, int64_t N,
                             float* mean_grad, float* weights_grad, float* logvar_grad, double* loss_entropy, void* workspace,
                             int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_gmm(mean, weights, cfg, logvar)) return e;
  if (int e = check_prec(prec)) return e;
  if (!mean_params || !mean_packed || !weights_params || !weights_packed || !obs || !actions || !mean_grad || !weights_grad ||
      !loss_entropy || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_gmm_train(cfg, logvar_grad)) return e;
  if (cfg->std_mode == 0 && !(cfg->fixed_std > 0)) return fail(-1, "fixed_std must be positive");
  if (cfg->deterministic) return fail(-1, "the behaviour-cloning loss is not defined for deterministic = 1");
  if (int e = check_rows(N)) return e;
#define CALL(P)                                                                                                                   \
  gmm_bc_impl<P>(*mean, *weights, mean_params, (const char*)mean_packed, weights_params, (const char*)weights_packed, *cfg, logvar, \
                 obs, actions, N, mean_grad, weights_grad, logvar_grad, loss_entropy, workspace, workspace_bytes,                 \
                 (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- conv denoiser: PPO update and supervised loss (unet.hip does the network, this file the loss and the critic) -------
template <class P>
struct UnetPpoWs {
  double *moments, *loss_partial;
  float* loss_tab;
  int32_t *brow, *krow;
  MlpBufs<P> C;
  void* d_eps;
  void* uws;
  size_t ubytes;
  int ldde;
};
template <class P>
static size_t carve_unet_ppo(Carver& c, const dppo_unet_desc& u, const dppo_net_desc* cr, int64_t N, UnetPpoWs<P>& W) {
  W.moments = (double*)c.take((8 + 2 * ADV_MOMENT_BLOCKS) * sizeof(double));
  W.loss_tab = (float*)c.take(2 * 1024 * sizeof(float));
  W.ldde = round_up(u.horizon_steps * u.action_dim, 64);
  const int64_t lb = loss_blocks(N), mb = bc_loss_blocks(N, W.ldde) + 1;
  W.loss_partial = (double*)c.take((size_t)(lb * 8 > mb ? lb * 8 : mb) * sizeof(double));
  W.brow = (int32_t*)c.take((size_t)N * 4);
  W.krow = (int32_t*)c.take((size_t)N * 4);
  if (cr) carve_mlp<P>(c, *cr, N, true, true, W.C);
  W.d_eps = c.take((size_t)N * W.ldde * P::ESIZE);
  W.ubytes = unet_trainer_bytes<P>(u, N);
  W.uws = c.take(W.ubytes);
  return al256(c.off);
}
int64_t dppo_unet_ppo_workspace_bytes(const dppo_unet_desc* actor, const dppo_net_desc* critic, int prec, int64_t N) {
  if (unet_check_desc(actor) || check_net(critic) || check_prec(prec)) return -1;
  if (N < 2 || N > (1 << 24)) return fail(-1, "N out of range");
  return ws_bytes(prec, [&](Carver& c, auto p) {
    UnetPpoWs<decltype(p)> W;
    return carve_unet_ppo<decltype(p)>(c, *actor, critic, N, W);
  });
}
template <class P>
static int unet_ppo_impl(const dppo_unet_desc& u, const dppo_net_desc& cr, const float* ap, const char* ak, const float* cp,
                         const char* ck, const dppo_diffusion_cfg& dcfg, const dppo_ppo_cfg& pcfg, const dppo_step* ksteps,
                         const float* obs_k, const float* chains_k, const float* returns_k, const float* values_k,
                         const float* adv_k, const float* logprobs_k, const int64_t* inds, const int64_t* kinds, int64_t N,
                         const double* gmom, float* agrad, float* cgrad, double* stats, void* ws, int64_t wsb, hipStream_t s,
                         const dppo_obs_io* oio = nullptr) {
  UnetPpoWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_unet_ppo<P>(c, u, &cr, N, W); })) return e;
  const PackLayout LC = pack_layout<P>(cr, 0);
  const int Kft = pcfg.ft_denoising_steps, AF = u.horizon_steps * u.action_dim;
  BuildRows br;  // critic rows + the zeroing / loss table side jobs; the conv actor builds its own input images
  memset(&br, 0, sizeof(br));
  br.zero_b = W.moments, br.n_zero_b = 32;
  if (Kft <= 1024) br.loss_tab = W.loss_tab, br.pcfg = pcfg;
  br.inds = inds, br.kinds = kinds, br.chains = chains_k, br.ksteps = ksteps, br.Kft = Kft, br.AF = AF;
  br.obs = oio && oio->obs_critic ? oio->obs_critic : obs_k;  // (pixel nets: the critic encodes the images itself)
  br.cond = cr.cond_dim, br.M = N, br.inC = W.C.in, br.KpC = LC.Kp0, br.brow = W.brow, br.onehot0 = -1;
  launch_build_rows<P>(br, s);
  launch_unet_index(inds, kinds, Kft, N, W.brow, W.krow, s);
  if (gmom == nullptr) launch_adv_moments(adv_k, W.brow, N, W.moments, s);
  // critic pipeline beside the actor's forward
  hipStream_t s2 = fork_side(s);
  mlp_forward<P>(cr, cp, ck, LC, N, W.C, true, s2);
  UnetTrainer<P>* T = unet_trainer_new<P>(u, ap, ak, N, W.uws, W.ubytes, s);
  UnetTrainIO io;
  memset(&io, 0, sizeof(io));
  io.chains = chains_k, io.obs = obs_k, io.brow = W.brow, io.krow = W.krow, io.ksteps = ksteps, io.Kft = Kft;
  io.gathered = kinds != nullptr;
  const float* eps = unet_trainer_forward<P>(T, io);
  if (s2 != s) join_side(s, s2);
  LossArgs la;
  memset(&la, 0, sizeof(la));
  la.eps = eps, la.lde = AF, la.vnew = W.C.out, la.ldv = W.C.ldout, la.brow = W.brow, la.krow = W.krow;
  la.gathered = kinds != nullptr;
  la.chains = chains_k, la.logprobs_k = logprobs_k, la.returns_k = returns_k, la.values_k = values_k, la.adv_k = adv_k;
  la.ksteps = ksteps, la.dcfg = dcfg, la.pcfg = pcfg, la.AF = AF, la.N = N;
  la.moments = gmom ? gmom : W.moments;
  la.tab = Kft <= 1024 ? W.loss_tab : nullptr;
  la.d_eps = W.d_eps, la.ldde = W.ldde, la.d_v = W.C.d_out, la.lddv = LC.Kpo, la.stats = stats;
  la.part = 3, la.partial = W.loss_partial;
  launch_ppo_loss<P>(la, s);
  s2 = fork_side(s);
  mlp_backward<P>(cr, cp, ck, LC, N, W.C, cgrad, nullptr, nullptr, 0, s2, &la);
  if (oio && oio->d_obs_critic) obs_grad<P>(cr, cp, N, W.C, oio->d_obs_critic, s2);
  unet_trainer_backward<P>(T, W.d_eps, W.ldde, agrad, oio ? oio->d_obs_actor : nullptr);
  unet_trainer_free<P>(T);
  if (s2 != s) join_side(s, s2);
  return check_launch();
}
static int unet_ppo_entry(const dppo_unet_desc* actor, const dppo_net_desc* critic, int prec, const float* actor_params,
                               const void* actor_packed, const float* critic_params, const void* critic_packed,
                               const dppo_diffusion_cfg* dcfg, const dppo_ppo_cfg* pcfg, const dppo_step* ksteps,
                               const float* obs_k, const float* chains_k, const float* returns_k, const float* values_k,
                               const float* adv_k, const float* logprobs_k, const int64_t* inds, const int64_t* kinds,
                               int64_t N, const double* global_moments, float* actor_grad, float* critic_grad,
                               double* stats, void* workspace, int64_t workspace_bytes, dppo_stream_t stream,
                               const dppo_obs_io* io) {
  if (int e = unet_check_desc(actor)) return e;
  if (int e = check_net(critic)) return e;
  if (int e = check_prec(prec)) return e;
  if (critic->kind != 1 || critic->out_dim != 1) return fail(-1, "critic descriptor must be kind 1 with out_dim 1");
  if (actor->cond_dim != critic->cond_dim && !(io && io->obs_critic))
    return fail(-1, "actor and critic observe different cond_dim");
  if (!actor_params || !actor_packed || !critic_params || !critic_packed || !dcfg || !pcfg || !ksteps || !obs_k ||
      !chains_k || !returns_k || !values_k || !adv_k || !logprobs_k || !actor_grad || !critic_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_obs_io(io, kinds, false)) return e;
  if ((inds == nullptr) == (kinds == nullptr)) return fail(-1, "pass exactly one of inds (rollout mode) / kinds (gathered mode)");
  if (N < 2 || N > (1 << 24)) return fail(-1, "N out of range");
  if (pcfg->ft_denoising_steps < 1 || pcfg->ft_denoising_steps > 1024) return fail(-1, "Kft out of range");
  if ((int64_t)pcfg->ft_denoising_steps * actor->time_dim > 16384)  // (its LDS tables go in chunks of steps: no limit from them)
    return fail(-1, "Kft * time_dim above 16384 (the per-step gradient table of the time MLP's backward)");
  if (pcfg->horizon_steps != actor->horizon_steps || pcfg->action_dim != actor->action_dim) return fail(-1, "Ta / Da mismatch");
  if (pcfg->reward_horizon < 1) return fail(-1, "reward_horizon must be >= 1");
#define CALL(P)                                                                                                          \
  unet_ppo_impl<P>(*actor, *critic, actor_params, (const char*)actor_packed, critic_params, (const char*)critic_packed, *dcfg, \
                   *pcfg, ksteps, obs_k, chains_k, returns_k, values_k, adv_k, logprobs_k, inds, kinds, N, global_moments,     \
                   actor_grad, critic_grad, stats, workspace, workspace_bytes, (hipStream_t)stream, io)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
int dppo_unet_ppo_loss_fwd_bwd(const dppo_unet_desc* actor, const dppo_net_desc* critic, int prec, const float* actor_params,
                               const void* actor_packed, const float* critic_params, const void* critic_packed,
                               const dppo_diffusion_cfg* dcfg, const dppo_ppo_cfg* pcfg, const dppo_step* ksteps,
                               const float* obs_k, const float* chains_k, const float* returns_k, const float* values_k,
                               const float* adv_k, const float* logprobs_k, const int64_t* inds, const int64_t* kinds,
                               int64_t N, const double* global_moments, float* actor_grad, float* critic_grad,
                               double* stats, void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  return unet_ppo_entry(actor, critic, prec, actor_params, actor_packed, critic_params, critic_packed, dcfg, pcfg, ksteps, obs_k,
                        chains_k, returns_k, values_k, adv_k, logprobs_k, inds, kinds, N, global_moments, actor_grad,
                        critic_grad, stats, workspace, workspace_bytes, stream, nullptr);
}
int dppo_unet_ppo_loss_fwd_bwd_obs(const dppo_unet_desc* actor, const dppo_net_desc* critic, int prec, const float* actor_params,
                                   const void* actor_packed, const float* critic_params, const void* critic_packed,
                                   const dppo_diffusion_cfg* dcfg, const dppo_ppo_cfg* pcfg, const dppo_step* ksteps,
                                   const float* obs_k, const float* chains_k, const float* returns_k, const float* values_k,
                                   const float* adv_k, const float* logprobs_k, const int64_t* kinds, int64_t N,
                                   const double* global_moments, float* actor_grad, float* critic_grad, double* stats,
                                   void* workspace, int64_t workspace_bytes, dppo_stream_t stream, const dppo_obs_io* io) {
  if (!io) return fail(-1, "null pointer");
  return unet_ppo_entry(actor, critic, prec, actor_params, actor_packed, critic_params, critic_packed, dcfg, pcfg, ksteps, obs_k,
                        chains_k, returns_k, values_k, adv_k, logprobs_k, nullptr, kinds, N, global_moments, actor_grad,
                        critic_grad, stats, workspace, workspace_bytes, stream, io);
}
int64_t dppo_unet_denoise_mse_workspace_bytes(const dppo_unet_desc* net, int prec, int64_t N) {
  if (unet_check_desc(net) || check_prec(prec)) return -1;
  if (N < 1 || N > (1 << 24)) return fail(-1, "N out of range");
  return ws_bytes(prec, [&](Carver& c, auto p) {
    UnetPpoWs<decltype(p)> W;
    return carve_unet_ppo<decltype(p)>(c, *net, nullptr, N, W);
  });
}
template <class P>
static int unet_mse_impl(const dppo_unet_desc& u, const float* prm, const char* pk, const dppo_step* tsteps, int n_time,
                         const float* obs, const float* pairs, const int64_t* kinds, int64_t N, float* grad, double* loss,
                         void* ws, int64_t wsb, hipStream_t s, float* d_obs = nullptr) {
  UnetPpoWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_unet_ppo<P>(c, u, nullptr, N, W); })) return e;
  const int AF = u.horizon_steps * u.action_dim;
  launch_unet_index(nullptr, kinds, n_time, N, W.brow, W.krow, s);
  UnetTrainer<P>* T = unet_trainer_new<P>(u, prm, pk, N, W.uws, W.ubytes, s);
  UnetTrainIO io;
  memset(&io, 0, sizeof(io));
  io.chains = pairs, io.obs = obs, io.brow = W.brow, io.krow = W.krow, io.ksteps = tsteps, io.Kft = n_time, io.gathered = 1;
  const float* eps = unet_trainer_forward<P>(T, io);
  MseArgs ma;
  ma.eps = eps, ma.lde = AF, ma.pairs = pairs, ma.AF = AF, ma.M = N, ma.d_eps = W.d_eps, ma.ldde = W.ldde, ma.loss = loss;
  ma.partial = W.loss_partial;
  launch_mse_loss<P>(ma, s);
  unet_trainer_backward<P>(T, W.d_eps, W.ldde, grad, d_obs);
  unet_trainer_free<P>(T);
  return check_launch();
}
static int unet_mse_entry(const dppo_unet_desc* net, int prec, const float* params, const void* packed,
                                  const dppo_step* tsteps, int n_time, const float* obs, const float* pairs,
                                  const int64_t* kinds, int64_t N, float* grad, double* loss, void* workspace,
                                  int64_t workspace_bytes, dppo_stream_t stream, float* d_obs) {
  if (int e = unet_check_desc(net)) return e;
  if (int e = check_prec(prec)) return e;
  if (!params || !packed || !tsteps || !obs || !pairs || !kinds || !grad || !loss || !workspace) return fail(-1, "null pointer");
  if (N < 1 || N > (1 << 24) || n_time < 1 || n_time > 1024) return fail(-1, "N / n_time out of range");
  if ((int64_t)n_time * net->time_dim > 16384)  // (its LDS tables go in chunks of steps: no limit from them)
    return fail(-1, "n_time * time_dim above 16384 (the per-step gradient table of the time MLP's backward)");
#define CALL(P)                                                                                                          \
  unet_mse_impl<P>(*net, params, (const char*)packed, tsteps, n_time, obs, pairs, kinds, N, grad, loss, workspace, workspace_bytes, \
                   (hipStream_t)stream, d_obs)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
int dppo_unet_denoise_mse_fwd_bwd(const dppo_unet_desc* net, int prec, const float* params, const void* packed,
                                  const dppo_step* tsteps, int n_time, const float* obs, const float* pairs,
                                  const int64_t* kinds, int64_t N, float* grad, double* loss, void* workspace,
                                  int64_t workspace_bytes, dppo_stream_t stream) {
  return unet_mse_entry(net, prec, params, packed, tsteps, n_time, obs, pairs, kinds, N, grad, loss, workspace, workspace_bytes,
                        stream, nullptr);
}
int dppo_unet_denoise_mse_fwd_bwd_obs(const dppo_unet_desc* net, int prec, const float* params, const void* packed,
                                      const dppo_step* tsteps, int n_time, const float* obs, const float* pairs,
                                      const int64_t* kinds, int64_t N, float* grad, double* loss, void* workspace,
                                      int64_t workspace_bytes, dppo_stream_t stream, float* d_obs) {
  if (!d_obs) return fail(-1, "null pointer");
  return unet_mse_entry(net, prec, params, packed, tsteps, n_time, obs, pairs, kinds, N, grad, loss, workspace, workspace_bytes,
                        stream, d_obs);
}

// ---- IDQL (idql.hip): twin-Q critics, expectile V, best-of-N selection, Polyak target -----------------------------------------
static int check_idql_q(const dppo_net_desc* q, bool ln_plain = false) {
  if (int e = check_net(q, ln_plain)) return e;
  if (q->kind != 1 || q->out_dim != 1) return fail(-1, "a Q trunk is a kind-1 descriptor with out_dim 1");
  return 0;
}
static int check_idql_pair(const dppo_net_desc* q, const dppo_net_desc* v) {
  if (int e = check_idql_q(q)) return e;
  if (int e = check_net(v)) return e;
  if (v->kind != 1 || v->out_dim != 1) return fail(-1, "the V critic is a kind-1 descriptor with out_dim 1");
  if (q->in_dim <= v->cond_dim)
    return fail(-1, "Q / V descriptors do not pair: Q in_dim=%d must be V cond_dim=%d + the action width", q->in_dim, v->cond_dim);
  return 0;
}
// what of the ring an entry reads, and so what must be non-null: the observations (an actor loss), the stored actions too, or the
// whole transition (a TD loss)
enum RingNeed { RING_OBS, RING_ACTIONS, RING_TRANSITION };
static int check_idql_batch(const dppo_idql_batch* b, int64_t N, RingNeed need) {
  if (!b) return fail(-1, "null batch");
  if (!b->obs || (need >= RING_ACTIONS && !b->actions) || (need == RING_TRANSITION && (!b->next_obs || !b->reward || !b->terminated)))
    return fail(-1, "null pointer in batch");
  if (b->cap < 1 || b->n_envs < 1 || b->count < 1 || b->count > b->cap || b->head < 0 || b->head >= b->cap)
    return fail(-1, "batch ring geometry: need 1 <= count <= cap, n_envs >= 1, 0 <= head < cap");
  if (!b->inds && N > b->count * b->n_envs) return fail(-1, "N=%lld exceeds the %lld stored transitions", (long long)N,
                                                         (long long)(b->count * b->n_envs));
  return 0;
}
template <class P>
struct IdqlWs {
  MlpBufs<P> Q1, Q2, V;
  double* partial;
  float *r, *term;
};
// train_q: the Q trunks keep their activations and get backward buffers (Q loss); otherwise V does (V loss)
template <class P>
static size_t carve_idql(Carver& c, const dppo_net_desc& q, const dppo_net_desc* v, int64_t N, bool twin, bool train_q, bool train_v,
                         IdqlWs<P>& W) {
  W.partial = (double*)c.take((size_t)idql_blocks(N) * 4 * sizeof(double));
  W.r = (float*)c.take((size_t)N * 4);
  W.term = (float*)c.take((size_t)N * 4);
  carve_mlp<P>(c, q, N, train_q, train_q, W.Q1);
  if (twin) carve_mlp<P>(c, q, N, train_q, train_q, W.Q2);
  if (v) carve_mlp<P>(c, *v, N, train_v, train_v, W.V);
  return al256(c.off);
}
static int64_t idql_ws_bytes(const dppo_net_desc* q, const dppo_net_desc* v, int prec, int64_t N, int double_q, bool train_q,
                             bool train_v) {
  // (no V, no training: dppo_idql_q_forward, which reads one LayerNorm trunk -- a twin of them is not built)
  if ((v ? check_idql_pair(q, v) : check_idql_q(q, !double_q && !train_q)) || check_prec(prec)) return -1;
  if (int e = check_rows(N)) return e;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    IdqlWs<decltype(p)> W;
    return carve_idql<decltype(p)>(c, *q, v, N, double_q != 0, train_q, train_v, W);
  });
}
int64_t dppo_idql_v_loss_workspace_bytes(const dppo_net_desc* q, const dppo_net_desc* v, int prec, int64_t N, int double_q) {
  return idql_ws_bytes(q, v, prec, N, double_q, false, true);
}
int64_t dppo_idql_q_loss_workspace_bytes(const dppo_net_desc* q, const dppo_net_desc* v, int prec, int64_t N, int double_q) {
  return idql_ws_bytes(q, v, prec, N, double_q, true, false);
}
int64_t dppo_idql_q_forward_workspace_bytes(const dppo_net_desc* q, int prec, int64_t N, int double_q) {
  return idql_ws_bytes(q, nullptr, prec, N, double_q, false, false);
}
static IdqlRows idql_rows_of(const dppo_idql_batch& b, int64_t N, int OD, int AD) {
  IdqlRows r;
  memset(&r, 0, sizeof(r));
  r.obs = b.obs, r.next_obs = b.next_obs, r.actions = b.actions, r.reward = b.reward, r.terminated = b.terminated, r.inds = b.inds;
  r.cap = b.cap, r.E = b.n_envs, r.head = b.head, r.count = b.count, r.N = N, r.OD = OD, r.AD = AD;
  return r;
}
template <class P>
static int idql_v_impl(const dppo_net_desc& q, const dppo_net_desc& v, const float* tp, const char* tk1, const char* tk2,
                       const float* vp, const char* vk, const dppo_idql_batch& b, int64_t N, double tau, bool twin, float* vgrad,
                       float* adv, double* stats, void* ws, int64_t wsb, hipStream_t s) {
  IdqlWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_idql<P>(c, q, &v, N, twin, false, true, W); })) return e;
  const PackLayout LQ = pack_layout<P>(q, 0), LV = pack_layout<P>(v, 0);
  IdqlRows r = idql_rows_of(b, N, v.cond_dim, q.in_dim - v.cond_dim);
  r.q1in = W.Q1.in, r.q2in = twin ? W.Q2.in : nullptr, r.vin = W.V.in, r.KpQ = LQ.Kp0, r.KpV = LV.Kp0;
  launch_idql_rows<P>(r, s);
  // the two target trunks on side streams beside V's forward; the loss reads all three outputs
  hipStream_t s1 = fork_side(s, 0);
  mlp_forward<P>(q, tp, tk1, LQ, N, W.Q1, false, s1);
  hipStream_t s2 = s;
  if (twin) {
    s2 = fork_side(s, 2);
    mlp_forward<P>(q, tp + param_layout(q).total, tk2, LQ, N, W.Q2, false, s2);
  }
  mlp_forward<P>(v, vp, vk, LV, N, W.V, true, s);
  if (s1 != s) join_side(s, s1, 0);
  if (s2 != s) join_side(s, s2, 2);
  IdqlLoss l;
  memset(&l, 0, sizeof(l));
  l.q1 = W.Q1.out, l.q2 = twin ? W.Q2.out : nullptr, l.ldq = W.Q1.ldout, l.v = W.V.out, l.ldv = W.V.ldout, l.N = N;
  l.tau = (float)tau, l.d_a = W.V.d_out, l.ldd = LV.Kpo, l.adv_out = adv, l.partial = W.partial, l.stats = stats;
  launch_idql_v_loss<P>(l, s);
  mlp_backward<P>(v, vp, vk, LV, N, W.V, vgrad, nullptr, nullptr, 0, s);
  return check_launch();
}
int dppo_idql_v_loss_fwd_bwd(const dppo_net_desc* q, const dppo_net_desc* v, int prec, const float* target_q_params,
                             const void* target_q1_packed, const void* target_q2_packed, const float* v_params,
                             const void* v_packed, const dppo_idql_batch* batch, int64_t N, double expectile, int double_q,
                             float* v_grad, float* adv_out, double* stats, void* workspace, int64_t workspace_bytes,
                             dppo_stream_t stream) {
  if (int e = check_idql_pair(q, v)) return e;
  if (int e = check_prec(prec)) return e;
  if (!target_q_params || !target_q1_packed || (double_q && !target_q2_packed) || !v_params || !v_packed || !v_grad || !stats ||
      !workspace)
    return fail(-1, "null pointer");
  if (int e = check_rows(N)) return e;
  if (int e = check_idql_batch(batch, N, RING_ACTIONS)) return e;
  if (!(expectile >= 0.0 && expectile <= 1.0)) return fail(-1, "expectile tau=%g outside [0, 1]", expectile);
#define CALL(P)                                                                                                                \
  idql_v_impl<P>(*q, *v, target_q_params, (const char*)target_q1_packed, (const char*)target_q2_packed, v_params,              \
                 (const char*)v_packed, *batch, N, expectile, double_q != 0, v_grad, adv_out, stats, workspace, workspace_bytes, \
                 (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
template <class P>
static int idql_q_impl(const dppo_net_desc& q, const dppo_net_desc& v, const float* qp, const char* qk1, const char* qk2,
                       const float* vp, const char* vk, const dppo_idql_batch& b, int64_t N, double gamma, bool twin, float* qgrad,
                       double* stats, void* ws, int64_t wsb, hipStream_t s) {
  IdqlWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_idql<P>(c, q, &v, N, twin, true, false, W); })) return e;
  const PackLayout LQ = pack_layout<P>(q, 0), LV = pack_layout<P>(v, 0);
  const int64_t nq = param_layout(q).total;
  IdqlRows r = idql_rows_of(b, N, v.cond_dim, q.in_dim - v.cond_dim);
  r.q1in = W.Q1.in, r.q2in = twin ? W.Q2.in : nullptr, r.nvin = W.V.in, r.KpQ = LQ.Kp0, r.KpV = LV.Kp0;
  r.r_out = W.r, r.term_out = W.term;
  launch_idql_rows<P>(r, s);
  // Q2 on side stream 0 and V(next_obs) on side stream 2 beside Q1; one join before the loss, one after the backward
  hipStream_t s2 = twin ? fork_side(s, 0) : s;
  if (twin) mlp_forward<P>(q, qp + nq, qk2, LQ, N, W.Q2, true, s2);
  hipStream_t s3 = fork_side(s, 2);
  mlp_forward<P>(v, vp, vk, LV, N, W.V, false, s3);
  mlp_forward<P>(q, qp, qk1, LQ, N, W.Q1, true, s);
  if (s2 != s) join_side(s, s2, 0);
  if (s3 != s) join_side(s, s3, 2);
  IdqlLoss l;
  memset(&l, 0, sizeof(l));
  l.q1 = W.Q1.out, l.q2 = twin ? W.Q2.out : nullptr, l.ldq = W.Q1.ldout, l.v = W.V.out, l.ldv = W.V.ldout, l.N = N;
  l.reward = W.r, l.terminated = W.term, l.gamma = (float)gamma, l.d_a = W.Q1.d_out, l.d_b = twin ? W.Q2.d_out : nullptr;
  l.ldd = LQ.Kpo, l.partial = W.partial, l.stats = stats;
  launch_idql_q_loss<P>(l, s);
  if (twin) {
    s2 = fork_side(s, 0);
    mlp_backward<P>(q, qp + nq, qk2, LQ, N, W.Q2, qgrad + nq, nullptr, nullptr, 0, s2);
  }
  mlp_backward<P>(q, qp, qk1, LQ, N, W.Q1, qgrad, nullptr, nullptr, 0, s);
  if (s2 != s) join_side(s, s2, 0);
  return check_launch();
}
int dppo_idql_q_loss_fwd_bwd(const dppo_net_desc* q, const dppo_net_desc* v, int prec, const float* q_params,
                             const void* q1_packed, const void* q2_packed, const float* v_params, const void* v_packed,
                             const dppo_idql_batch* batch, int64_t N, double gamma, int double_q, float* q_grad, double* stats,
                             void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_idql_pair(q, v)) return e;
  if (int e = check_prec(prec)) return e;
  if (!q_params || !q1_packed || (double_q && !q2_packed) || !v_params || !v_packed || !q_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_rows(N)) return e;
  if (int e = check_idql_batch(batch, N, RING_TRANSITION)) return e;
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(-1, "discount gamma=%g outside [0, 1]", gamma);
#define CALL(P)                                                                                                                  \
  idql_q_impl<P>(*q, *v, q_params, (const char*)q1_packed, (const char*)q2_packed, v_params, (const char*)v_packed, *batch, N, gamma, \
                 double_q != 0, q_grad, stats, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
template <class P>
static int idql_fwd_impl(const dppo_net_desc& q, const float* qp, const char* qk1, const char* qk2, const float* obs, int OD,
                         int64_t obs_rows, const float* actions, int64_t N, bool twin, float* q1o, float* q2o, void* ws,
                         int64_t wsb, hipStream_t s) {
  IdqlWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_idql<P>(c, q, nullptr, N, twin, false, false, W); })) return e;
  const PackLayout LQ = pack_layout<P>(q, 0);
  IdqlRows r;
  memset(&r, 0, sizeof(r));
  r.obs = obs, r.actions = actions, r.obs_mod = obs_rows, r.N = N, r.OD = OD, r.AD = q.in_dim - OD;
  r.q1in = W.Q1.in, r.q2in = twin ? W.Q2.in : nullptr, r.KpQ = LQ.Kp0;
  launch_idql_rows<P>(r, s);
  hipStream_t s2 = twin ? fork_side(s, 0) : s;
  if (twin) {
    mlp_forward<P>(q, qp + param_layout(q).total, qk2, LQ, N, W.Q2, false, s2);
    launch_copy_cols(W.Q2.out, W.Q2.ldout, 0, 1, N, q2o, s2);
  }
  mlp_forward<P>(q, qp, qk1, LQ, N, W.Q1, false, s);
  launch_copy_cols(W.Q1.out, W.Q1.ldout, 0, 1, N, q1o, s);
  if (s2 != s) join_side(s, s2, 0);
  return check_launch();
}
int dppo_idql_q_forward(const dppo_net_desc* q, int prec, const float* q_params, const void* q1_packed, const void* q2_packed,
                        const float* obs, int obs_dim, int64_t obs_rows, const float* actions, int64_t N, int double_q,
                        float* q1_out, float* q2_out, void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_idql_q(q, !double_q)) return e;
  if (int e = check_prec(prec)) return e;
  if (!q_params || !q1_packed || !obs || !actions || !q1_out || !workspace || (double_q && (!q2_packed || !q2_out)))
    return fail(-1, "null pointer");
  if (int e = check_rows(N)) return e;
  if (obs_rows < 1 || obs_rows > N) return fail(-1, "obs_rows out of [1, N]");
  if (obs_dim < 1 || obs_dim >= q->in_dim)
    return fail(-1, "Q descriptor does not pair with obs_dim=%d: in_dim=%d must be obs_dim + the action width", obs_dim, q->in_dim);
#define CALL(P)                                                                                                                  \
  idql_fwd_impl<P>(*q, q_params, (const char*)q1_packed, (const char*)q2_packed, obs, obs_dim, obs_rows, actions, N, double_q != 0, \
                   q1_out, q2_out, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
int dppo_idql_select(const float* q1, const float* q2, const float* v, int v_per_env, const float* candidates, const float* u,
                     int64_t B, int S, int width, int mode, double h, uint64_t seed, float* actions, int32_t* idx,
                     dppo_stream_t stream) {
  if (!q1 || !candidates || !actions) return fail(-1, "null pointer");
  if (mode != 0 && mode != 1) return fail(-1, "mode must be 0 (argmax) or 1 (expectile exploration)");
  if (mode == 1 && !v) return fail(-1, "mode 1 needs v");
  if (B < 1 || S < 1 || width < 1 || B * (int64_t)S > 0x7fffffff) return fail(-1, "B, S, width out of range");
  if (!(h >= 0.0 && h <= 1.0)) return fail(-1, "critic_hyperparam tau=%g outside [0, 1]", h);
  IdqlSelect a;
  memset(&a, 0, sizeof(a));
  a.q1 = q1, a.q2 = q2, a.v = v, a.cand = candidates, a.u = u, a.B = B, a.S = S, a.AF = width, a.mode = mode;
  a.v_per_env = v_per_env ? 1 : 0, a.h = (float)h, a.seed_lo = (uint32_t)seed, a.seed_hi = (uint32_t)(seed >> 32);
  a.actions = actions, a.idx = idx;
  launch_idql_select(a, (hipStream_t)stream);
  return check_launch();
}
int dppo_polyak(float* target, const float* source, double tau, int64_t n, dppo_stream_t stream) {
  if (!target || !source) return fail(-1, "null pointer");
  if (n < 1) return fail(-1, "n out of range");
  if (!(tau >= 0.0 && tau <= 1.0)) return fail(-1, "tau=%g outside [0, 1]", tau);
  launch_polyak(target, source, (float)(1.0 - tau), (float)tau, n, (hipStream_t)stream);
  return check_launch();
}

// ---- QSM (qsm.hip): the twin critic's action gradient as the actor's regression target, and the TD loss on the target twin ----
static int check_qsm_q(const dppo_net_desc* q, int obs_dim) {
  if (int e = check_idql_q(q)) return e;
  if (obs_dim < 1 || obs_dim >= q->in_dim)
    return fail(-1, "Q descriptor does not pair with obs_dim=%d: in_dim=%d must be obs_dim + the action width", obs_dim, q->in_dim);
  return 0;
}
static int check_qsm_plain(const dppo_net_desc* q) {
  if (!q->plain)
    return fail(-1, "the action gradient dQ/da is built for plain Q trunks (a residual trunk, residual_tyle=True, is not; no shipped cfg has one)");
  if (qsm_tail_rows(2 * q->hidden) < 1) return fail(-1, "hidden=%d too wide for the action-gradient tail", q->hidden);
  return 0;
}
// M Q trunks' forward buffers with the pre-activations kept, and what their action-gradient chains need: nothing of a parameter
// backward (no slab, no column-sum partials).  QSM's target: M = 2; the actor losses' workspace (QActorWs) builds on it.
template <class P>
struct QChainWs {
  MlpBufs<P> Q[RLPD_MAX_E];
  void *dza[RLPD_MAX_E], *dzb[RLPD_MAX_E];  // trunk i's two alternating [N][H] chain buffers; dza[i] takes the seed
  void* dhcat;                              // [N][M H] elem: trunk i's dh_0 in columns [i H, (i + 1) H)
  void* w0a;                                // [AF][M H] elem: the action columns of the M W0, stacked along K
};
template <class P>
static size_t carve_q_chains(Carver& c, const dppo_net_desc& q, int AF, int64_t N, int M, QChainWs<P>& W) {
  const size_t ES = P::ESIZE;
  for (int i = 0; i < M; ++i) {
    carve_mlp<P>(c, q, N, true, false, W.Q[i]);
    W.dza[i] = c.take((size_t)N * q.hidden * ES);
    W.dzb[i] = c.take((size_t)N * q.hidden * ES);
  }
  W.dhcat = c.take((size_t)N * M * q.hidden * ES);
  W.w0a = c.take((size_t)AF * M * q.hidden * ES);
  return al256(c.off);
}
int64_t dppo_qsm_actor_target_workspace_bytes(const dppo_net_desc* q, int prec, int obs_dim, int64_t N) {
  if (check_qsm_q(q, obs_dim) || check_qsm_plain(q) || check_prec(prec)) return -1;
  if (int e = check_rows(N)) return e;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    QChainWs<decltype(p)> W;
    return carve_q_chains<decltype(p)>(c, *q, q->in_dim - obs_dim, N, 2, W);
  });
}
// d q / d (layer 0's Linear output) of one plain trunk, into its columns of dhcat (row stride ldh), from a seed d q / d z_L that is
// already in dza: data gradients only.  Per hidden layer from the top, the data GEMM with the act' epilogue (backward_plain's step
// without its dW / db); a LayerNorm trunk runs the LayerNorm backward without parameter sums in front of each, and once more, in
// place, on dh_0.  (Seeds: Wout (.) act'(z_L) by q_seeded_chain; the twin's choice per row by sac_select_kernel / calql_select_kernel.)
template <class P>
static void q_chain_from_seed(const dppo_net_desc& q, const float* prm, const char* pk, const PackLayout& L, int64_t N, MlpBufs<P>& B,
                              void* dza, void* dzb, void* dh0, int ldh, hipStream_t s) {
  const ParamLayout pl = param_layout(q);
  const int H = q.hidden, nb = q.n_blocks;
  LnBwd ln;
  memset(&ln, 0, sizeof(ln));
  ln.ld = H, ln.ldx = H, ln.M = N, ln.H = H;  // (partial stays null: a data-gradient chain)
  void* dz = dza;
  void* other = dzb;
  for (int b = nb - 1; b >= 0; --b) {
    if (q.use_layernorm) {
      ln.dz = dz, ln.x = B.h[b + 1], ln.stats = B.ln_stats + (size_t)(b + 1) * N * 2, ln.gamma = prm + pl.n1w[b];
      launch_ln_bwd<P>(ln, s);
    }
    GemmNT g;
    memset(&g, 0, sizeof(g));
    g.M = (int)N, g.N = H, g.Kp = H, g.ldx = H, g.ldw = H;
    g.X = dz, g.W = pk + L.W1T[b], g.dsrc = b == 0 ? B.hpre[0] : B.z1[b - 1], g.dsrc_kind = 2, g.dsrc_ld = H, g.dact = q.act;
    g.out_pre = b == 0 ? dh0 : other, g.ldo = b == 0 ? ldh : H;
    launch_gemm_nt<P>(g, s);
    void* t = dz;
    dz = other, other = t;
  }
  if (q.use_layernorm) {
    ln.dz = dh0, ln.ld = ldh, ln.x = B.h[0], ln.stats = B.ln_stats, ln.gamma = prm + pl.n0w;
    launch_ln_bwd<P>(ln, s);
  }
}
// ... with the seed of the trunk's own Q in front (out_dim is 1, so Wout is broadcast): d q / d x of one trunk
template <class P>
static void q_seeded_chain(const dppo_net_desc& q, const float* prm, const char* pk, const PackLayout& L, int64_t N, MlpBufs<P>& B,
                           void* dza, void* dzb, void* dh0, int ldh, hipStream_t s) {
  launch_qsm_seed<P>(pk + L.Wout, B.z1[q.n_blocks - 1], N, q.hidden, q.act, dza, s);
  q_chain_from_seed<P>(q, prm, pk, L, N, B, dza, dzb, dh0, ldh, s);
}
template <class P>
static int qsm_target_impl(const dppo_net_desc& q, const float* qp, const char* qk1, const char* qk2, const dppo_idql_batch& b,
                           int OD, int64_t N, const float* noise, const int64_t* t, const float* sa, const float* sb, int K,
                           double coeff, float* pairs, float* obs_out, float* g_out, void* ws, int64_t wsb, hipStream_t s) {
  QChainWs<P> W;
  const int AD = q.in_dim - OD, H = q.hidden;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_q_chains<P>(c, q, AD, N, 2, W); })) return e;
  const PackLayout L = pack_layout<P>(q, 0);
  const ParamLayout pl = param_layout(q);
  QsmRows r;
  memset(&r, 0, sizeof(r));
  r.ring = idql_rows_of(b, N, OD, AD);
  r.noise = noise, r.t = t, r.sa = sa, r.sb = sb, r.K = K, r.pairs = pairs, r.obs_out = obs_out;
  r.q1in = W.Q[0].in, r.q2in = W.Q[1].in, r.KpQ = L.Kp0;
  launch_qsm_rows<P>(r, s);
  // Q2's forward and chain on side stream 0 beside Q1's; the packing of the tail's weight operand rides in front of Q1's
  hipStream_t s2 = fork_side(s, 0);
  mlp_forward<P>(q, qp + pl.total, qk2, L, N, W.Q[1], true, s2);
  q_seeded_chain<P>(q, qp + pl.total, qk2, L, N, W.Q[1], W.dza[1], W.dzb[1], (char*)W.dhcat + (size_t)H * P::ESIZE, 2 * H, s2);
  launch_pack_w0a<P>(qp, pl.total, pl.W0, q.in_dim, OD, AD, H, 2, W.w0a, s);
  mlp_forward<P>(q, qp, qk1, L, N, W.Q[0], true, s);
  q_seeded_chain<P>(q, qp, qk1, L, N, W.Q[0], W.dza[0], W.dzb[0], W.dhcat, 2 * H, s);
  if (s2 != s) join_side(s, s2, 0);
  QsmTail tl;
  memset(&tl, 0, sizeof(tl));
  tl.dh = W.dhcat, tl.wa = W.w0a, tl.N = N, tl.H2 = 2 * H, tl.AD = AD, tl.rows = qsm_tail_rows(2 * H), tl.coeff = (float)coeff;
  tl.pairs = pairs, tl.g_out = g_out;
  launch_qsm_tail<P>(tl, s);
  return check_launch();
}
int dppo_qsm_actor_target(const dppo_net_desc* q, int prec, const float* q_params, const void* q1_packed, const void* q2_packed,
                          const dppo_idql_batch* batch, int obs_dim, int64_t N, const float* noise, const int64_t* t,
                          const float* sqrt_alphas_cumprod, const float* sqrt_one_minus_alphas_cumprod, int K, double coeff,
                          float* pairs, float* obs_out, float* g_out, void* workspace, int64_t workspace_bytes,
                          dppo_stream_t stream) {
  if (int e = check_qsm_q(q, obs_dim)) return e;
  if (int e = check_qsm_plain(q)) return e;
  if (int e = check_prec(prec)) return e;
  if (!q_params || !q1_packed || !q2_packed || !noise || !t || !sqrt_alphas_cumprod || !sqrt_one_minus_alphas_cumprod || !pairs ||
      !obs_out || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_rows(N)) return e;
  if (int e = check_idql_batch(batch, N, RING_ACTIONS)) return e;
  if (K < 1 || K > 1024) return fail(-1, "K=%d denoising steps outside [1, 1024]", K);
  if (!(coeff >= 0.0 && coeff <= 3.0e38)) return fail(-1, "q_grad_coeff=%g must be finite and >= 0", coeff);
#define CALL(P)                                                                                                              \
  qsm_target_impl<P>(*q, q_params, (const char*)q1_packed, (const char*)q2_packed, *batch, obs_dim, N, noise, t,             \
                     sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, K, coeff, pairs, obs_out, g_out, workspace,         \
                     workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

template <class P>
struct QsmTdWs {
  MlpBufs<P> Q1, Q2, T1, T2;
  double* partial;
  float *r, *term;
};
template <class P>
static size_t carve_qsm_td(Carver& c, const dppo_net_desc& q, int64_t N, QsmTdWs<P>& W) {
  W.partial = (double*)c.take((size_t)idql_blocks(N) * 4 * sizeof(double));
  W.r = (float*)c.take((size_t)N * 4);
  W.term = (float*)c.take((size_t)N * 4);
  carve_mlp<P>(c, q, N, true, true, W.Q1);
  carve_mlp<P>(c, q, N, true, true, W.Q2);
  carve_mlp<P>(c, q, N, false, false, W.T1);
  carve_mlp<P>(c, q, N, false, false, W.T2);
  return al256(c.off);
}
int64_t dppo_qsm_q_loss_workspace_bytes(const dppo_net_desc* q, int prec, int obs_dim, int64_t N) {
  if (check_qsm_q(q, obs_dim) || check_prec(prec)) return -1;
  if (int e = check_rows(N)) return e;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    QsmTdWs<decltype(p)> W;
    return carve_qsm_td<decltype(p)>(c, *q, N, W);
  });
}
template <class P>
static int twin_td_impl(const dppo_net_desc& q, const float* qp, const char* qk1, const char* qk2, const float* tp, const char* tk1,
                        const char* tk2, const dppo_idql_batch& b, int OD, const float* next_actions, const float* next_logp,
                        const double* alpha, int64_t N, double gamma, float* qgrad, double* stats, void* ws, int64_t wsb,
                        hipStream_t s) {
  QsmTdWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_qsm_td<P>(c, q, N, W); })) return e;
  const PackLayout L = pack_layout<P>(q, 0);
  const int64_t nq = param_layout(q).total;
  QsmTdRows r;
  memset(&r, 0, sizeof(r));
  r.ring = idql_rows_of(b, N, OD, q.in_dim - OD);
  r.next_actions = next_actions, r.q1in = W.Q1.in, r.q2in = W.Q2.in, r.t1in = W.T1.in, r.t2in = W.T2.in, r.KpQ = L.Kp0;
  r.r_out = W.r, r.term_out = W.term;
  launch_qsm_td_rows<P>(r, s);
  // Q2 and the two target trunks on the three side streams beside Q1; the side streams are joined into the last one, so the
  // caller's stream waits once before the loss (flush_slabs() has the reason)
  hipStream_t s2 = fork_side(s, 0), s3 = fork_side(s, 1), s4 = fork_side(s, 2);
  mlp_forward<P>(q, qp + nq, qk2, L, N, W.Q2, true, s2);
  mlp_forward<P>(q, tp, tk1, L, N, W.T1, false, s3);
  mlp_forward<P>(q, tp + nq, tk2, L, N, W.T2, false, s4);
  mlp_forward<P>(q, qp, qk1, L, N, W.Q1, true, s);
  if (s4 != s) {
    if (s2 != s) join_side(s4, s2, 0);
    if (s3 != s) join_side(s4, s3, 1);
    join_side(s, s4, 2);
  } else {
    if (s2 != s) join_side(s, s2, 0);
    if (s3 != s) join_side(s, s3, 1);
  }
  IdqlLoss l;
  memset(&l, 0, sizeof(l));
  l.q1 = W.Q1.out, l.q2 = W.Q2.out, l.ldq = W.Q1.ldout, l.v = W.T1.out, l.v2 = W.T2.out, l.ldv = W.T1.ldout, l.N = N;
  l.reward = W.r, l.terminated = W.term, l.gamma = (float)gamma, l.d_a = W.Q1.d_out, l.d_b = W.Q2.d_out;
  l.ldd = L.Kpo, l.partial = W.partial, l.stats = stats;
  l.next_logp = next_logp, l.alpha = alpha;  // SAC's entropy term of the bootstrap; both null (QSM, DQL): none
  launch_idql_q_loss<P>(l, s);
  s2 = fork_side(s, 0);
  mlp_backward<P>(q, qp + nq, qk2, L, N, W.Q2, qgrad + nq, nullptr, nullptr, 0, s2);
  mlp_backward<P>(q, qp, qk1, L, N, W.Q1, qgrad, nullptr, nullptr, 0, s);
  if (s2 != s) join_side(s, s2, 0);
  return check_launch();
}
int dppo_qsm_q_loss_fwd_bwd(const dppo_net_desc* q, int prec, const float* q_params, const void* q1_packed, const void* q2_packed,
                            const float* target_q_params, const void* target_q1_packed, const void* target_q2_packed,
                            const dppo_idql_batch* batch, int obs_dim, const float* next_actions, int64_t N, double gamma,
                            float* q_grad, double* stats, void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_qsm_q(q, obs_dim)) return e;
  if (int e = check_prec(prec)) return e;
  if (!q_params || !q1_packed || !q2_packed || !target_q_params || !target_q1_packed || !target_q2_packed || !next_actions ||
      !q_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_rows(N)) return e;
  if (int e = check_idql_batch(batch, N, RING_TRANSITION)) return e;
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(-1, "discount gamma=%g outside [0, 1]", gamma);
#define CALL(P)                                                                                                                \
  twin_td_impl<P>(*q, q_params, (const char*)q1_packed, (const char*)q2_packed, target_q_params, (const char*)target_q1_packed, \
                  (const char*)target_q2_packed, *batch, obs_dim, next_actions, nullptr, nullptr, N, gamma, q_grad, stats,      \
                  workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- RLPD (rlpd.hip): the TD loss of an ensemble of LayerNorm Q trunks -----------------------------------------------------------
// A plain LayerNorm Q trunk that pairs with obs_dim (RLPD's and IBRL's members, Cal-QL's twin); not_ln: the caller's own message
static int check_ln_q(const dppo_net_desc* q, int obs_dim, const char* not_ln) {
  if (int e = check_idql_q(q, true)) return e;
  if (!q->plain || !q->use_layernorm) return fail(-1, "%s", not_ln);
  if (obs_dim < 1 || obs_dim >= q->in_dim)
    return fail(-1, "Q descriptor does not pair with obs_dim=%d: in_dim=%d must be obs_dim + the action width", obs_dim, q->in_dim);
  return 0;
}
static int check_rlpd_q(const dppo_net_desc* q, int obs_dim, int E) {
  if (int e = check_ln_q(q, obs_dim, "the ensemble's members are plain trunks with LayerNorm (plain = 1, use_layernorm = 1)")) return e;
  if (E < 2 || E > RLPD_MAX_E) return fail(-1, "E=%d members out of [2, %d]", E, RLPD_MAX_E);
  return 0;
}
static int check_member_pair(int pair0, int pair1, int E) {
  if (pair0 < 0 || pair0 >= E || pair1 < 0 || pair1 >= E || pair0 == pair1)
    return fail(-1, "pair (%d, %d): two different members of [0, %d) are needed", pair0, pair1, E);
  return 0;
}
static int check_member_images(const void* const* packed, int E) {
  for (int e = 0; e < E; ++e)
    if (!packed[e]) return fail(-1, "null pointer: kernel image of member %d", e);
  return 0;
}
// What the ensemble's TD target bootstraps from.  RLPD: the smaller target Q at one next action per row, with the entropy term
// where next_logp and alpha are set.  IBRL (next_bc set): the better of the two proposals' smaller target Q (ibrl.h's target kernel).
struct EnsembleBootstrap {
  const float *next_actions, *next_logp;  // RLPD
  const double* alpha;
  const float *next_bc, *next_rl;  // IBRL
  float* y_out;
  double* bc_share;
};
template <class P>
struct EnsembleTdWs {
  MlpBufs<P> Q[RLPD_MAX_E], T[2];
  double* partial;
  float *r, *term;
  float* tq;  // IBRL only, as the next two
  uint32_t* won;
  double* share;
};
template <class P>
static size_t carve_ensemble_td(Carver& c, const dppo_net_desc& q, int64_t N, int E, bool ibrl, EnsembleTdWs<P>& W) {
  W.partial = (double*)c.take((size_t)E * rlpd_blocks(N) * 4 * sizeof(double));
  W.r = (float*)c.take((size_t)N * 4);
  W.term = (float*)c.take((size_t)N * 4);
  W.tq = ibrl ? (float*)c.take((size_t)N * 4) : nullptr;
  W.won = ibrl ? (uint32_t*)c.take((size_t)ibrl_target_blocks(N) * 4) : nullptr;
  W.share = ibrl ? (double*)c.take(sizeof(double)) : nullptr;
  for (int e = 0; e < E; ++e) {
    carve_mlp<P>(c, q, N, true, true, W.Q[e]);
    // IBRL in bf16: the rows that enter LayerNorm's backward stay in fp32 (ibrl.h); in fp32 the elem rows are that already
    if (ibrl && P::ESIZE == 2)
      for (int i = 0; i < 2; ++i) W.Q[e].ln_dz32[i] = (float*)c.take((size_t)N * q.hidden * 4);
  }
  for (int i = 0; i < 2; ++i) carve_mlp<P>(c, q, ibrl ? 2 * N : N, false, false, W.T[i]);  // IBRL: both proposals' rows
  return al256(c.off);
}
static int64_t ensemble_td_ws_bytes(const dppo_net_desc* q, int prec, int obs_dim, int64_t N, int E, bool ibrl) {
  if (check_rlpd_q(q, obs_dim, E) || check_prec(prec)) return -1;
  if (N < 1 || N > (ibrl ? 0x3fffffff : 0x7fffffff)) return fail(-1, "N out of range");
  return ws_bytes(prec, [&](Carver& c, auto p) {
    EnsembleTdWs<decltype(p)> W;
    return carve_ensemble_td<decltype(p)>(c, *q, N, E, ibrl, W);
  });
}
int64_t dppo_rlpd_q_loss_workspace_bytes(const dppo_net_desc* q, int prec, int obs_dim, int64_t N, int E) {
  return ensemble_td_ws_bytes(q, prec, obs_dim, N, E, false);
}
int64_t dppo_ibrl_q_loss_workspace_bytes(const dppo_net_desc* q, int prec, int obs_dim, int64_t N, int E) {
  return ensemble_td_ws_bytes(q, prec, obs_dim, N, E, true);
}
// The TD loss of the E members against the pair (p0, p1) of target members.  RLPD and IBRL differ in four places: the rows, the
// targets' row count, IBRL's target step in front of the loss, and (in the carve) IBRL's fp32 LayerNorm rows in bf16.
template <class P>
static int ensemble_td_impl(const dppo_net_desc& q, int E, const float* qp, const void* const* qk, const float* tp,
                            const void* const* tk, int p0, int p1, const dppo_idql_batch& b, int OD, const EnsembleBootstrap& bs,
                            int64_t N, double gamma, float* qgrad, double* stats, void* ws, int64_t wsb, hipStream_t s) {
  const bool ibrl = bs.next_bc != nullptr;
  EnsembleTdWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_ensemble_td<P>(c, q, N, E, ibrl, W); })) return e;
  // every member's buffers sit at one stride: the loss kernel reaches member e's from member 0's
  const int64_t q_stride = W.Q[1].out - W.Q[0].out, d_stride = (char*)W.Q[1].d_out - (char*)W.Q[0].d_out;
  bool even = true;
  for (int e = 1; e < E; ++e) even = even && W.Q[e].out - W.Q[0].out == e * q_stride && (char*)W.Q[e].d_out - (char*)W.Q[0].d_out == e * d_stride;
  if (!even) return fail(-1, "members' workspaces are not evenly spaced");
  const PackLayout L = pack_layout<P>(q, 0);
  const int64_t nq = param_layout(q).total;
  // every member reads the same rows [obs | a | 0], both targets the same [next_obs | next_a | 0] (IBRL: for a_bc, then for a_rl):
  // one image each
  if (ibrl) {
    IbrlRows r;
    memset(&r, 0, sizeof(r));
    r.ring = idql_rows_of(b, N, OD, q.in_dim - OD);
    r.a_bc = bs.next_bc, r.a_rl = bs.next_rl, r.qin = W.Q[0].in, r.tin = W.T[0].in, r.Kp = L.Kp0, r.r_out = W.r, r.term_out = W.term;
    launch_ibrl_rows<P>(r, s);
  } else {
    QsmTdRows r;
    memset(&r, 0, sizeof(r));
    r.ring = idql_rows_of(b, N, OD, q.in_dim - OD);
    r.next_actions = bs.next_actions, r.q1in = r.q2in = W.Q[0].in, r.t1in = r.t2in = W.T[0].in, r.KpQ = L.Kp0;
    r.r_out = W.r, r.term_out = W.term;
    launch_qsm_td_rows<P>(r, s);
  }
  for (int e = 1; e < E; ++e) W.Q[e].in = W.Q[0].in;
  W.T[1].in = W.T[0].in;
  // the trunks take turns on the caller's stream and the three side streams
  const int64_t NT = ibrl ? 2 * N : N;
  hipStream_t st[4] = {s, fork_side(s, 0), fork_side(s, 1), fork_side(s, 2)};
  mlp_forward<P>(q, tp + p0 * nq, (const char*)tk[p0], L, NT, W.T[0], false, st[1]);
  mlp_forward<P>(q, tp + p1 * nq, (const char*)tk[p1], L, NT, W.T[1], false, st[2]);
  for (int e = 0; e < E; ++e) mlp_forward<P>(q, qp + e * nq, (const char*)qk[e], L, N, W.Q[e], true, st[(e + 3) & 3]);
  for (int i = 1; i < 4; ++i) join_side(s, st[i], i - 1);
  RlpdLoss l;
  memset(&l, 0, sizeof(l));
  l.q = W.Q[0].out, l.q_stride = q_stride, l.ldq = W.Q[0].ldout, l.t1 = W.T[0].out, l.t2 = W.T[1].out, l.ldt = W.T[0].ldout;
  l.reward = W.r, l.terminated = W.term, l.next_logp = bs.next_logp, l.alpha = bs.alpha, l.gamma = (float)gamma, l.N = N, l.E = E;
  l.d_out = W.Q[0].d_out, l.d_stride = d_stride, l.ldd = L.Kpo, l.partial = W.partial, l.stats = stats;
  if (ibrl) {  // the better proposal's smaller target Q per row, which the loss then reads as both of its targets
    IbrlTarget t;
    memset(&t, 0, sizeof(t));
    t.t1 = W.T[0].out, t.t2 = W.T[1].out, t.ldt = W.T[0].ldout, t.N = N, t.tq = W.tq, t.reward = W.r, t.terminated = W.term;
    t.gamma = (float)gamma, t.y_out = bs.y_out, t.partial = W.won, t.share = bs.bc_share ? bs.bc_share : W.share;
    launch_ibrl_target(t, s);
    l.t1 = l.t2 = W.tq, l.ldt = 1;
  }
  launch_rlpd_loss<P>(l, s);
  for (int i = 1; i < 4; ++i) st[i] = fork_side(s, i - 1);
  for (int e = 0; e < E; ++e)
    mlp_backward<P>(q, qp + e * nq, (const char*)qk[e], L, N, W.Q[e], qgrad + e * nq, nullptr, nullptr, 0, st[e & 3]);
  for (int i = 1; i < 4; ++i) join_side(s, st[i], i - 1);
  launch_rlpd_out_bias(W.partial, N, E, qgrad, nq, param_layout(q).bout, s);
  return check_launch();
}
// The checks both entries share behind their own null-pointer test
static int check_ensemble_td(const void* const* q_packed, const void* const* target_q_packed, int pair0, int pair1, int E,
                             const dppo_idql_batch* batch, int64_t N, int64_t n_max, double gamma) {
  if (int e = check_member_pair(pair0, pair1, E)) return e;
  if (int e = check_member_images(q_packed, E)) return e;
  if (!target_q_packed[pair0] || !target_q_packed[pair1]) return fail(-1, "null pointer: kernel image of a target member of the pair");
  if (N < 1 || N > n_max) return fail(-1, "N out of range");
  if (int e = check_idql_batch(batch, N, RING_TRANSITION)) return e;
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(-1, "discount gamma=%g outside [0, 1]", gamma);
  return 0;
}
int dppo_rlpd_q_loss_fwd_bwd(const dppo_net_desc* q, int prec, int E, const float* q_params, const void* const* q_packed,
                             const float* target_q_params, const void* const* target_q_packed, int pair0, int pair1,
                             const dppo_idql_batch* batch, int obs_dim, const float* next_actions, const float* next_logp,
                             const double* alpha, int64_t N, double gamma, float* q_grad, double* stats, void* workspace,
                             int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_rlpd_q(q, obs_dim, E)) return e;
  if (int e = check_prec(prec)) return e;
  if (!q_params || !q_packed || !target_q_params || !target_q_packed || !next_actions || !q_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if ((next_logp == nullptr) != (alpha == nullptr)) return fail(-1, "null pointer: next_logp and alpha go together (both null: no entropy backup)");
  if (int e = check_ensemble_td(q_packed, target_q_packed, pair0, pair1, E, batch, N, 0x7fffffff, gamma)) return e;
  EnsembleBootstrap bs;
  memset(&bs, 0, sizeof(bs));
  bs.next_actions = next_actions, bs.next_logp = next_logp, bs.alpha = alpha;
#define CALL(P)                                                                                                                   \
  ensemble_td_impl<P>(*q, E, q_params, q_packed, target_q_params, target_q_packed, pair0, pair1, *batch, obs_dim, bs, N, gamma, q_grad, \
                      stats, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- IBRL (ibrl.hip): acting through two proposals, and the ensemble's TD loss with the better of them as bootstrap ----------------
template <class P>
struct IbrlActWs {
  MlpBufs<P> A[2], Q[2];  // the BC and the RL actor over B rows, the pair's members over 2B
  float *a_bc, *a_rl, *q_bc, *q_rl;
  uint8_t* took;
};
template <class P>
static size_t carve_ibrl_act(Carver& c, const dppo_net_desc& a, const dppo_net_desc& q, int64_t B, IbrlActWs<P>& W) {
  W.a_bc = (float*)c.take((size_t)B * a.out_dim * 4);
  W.a_rl = (float*)c.take((size_t)B * a.out_dim * 4);
  W.q_bc = (float*)c.take((size_t)B * 4);
  W.q_rl = (float*)c.take((size_t)B * 4);
  W.took = (uint8_t*)c.take((size_t)B);
  for (int i = 0; i < 2; ++i) carve_mlp<P>(c, a, B, false, false, W.A[i]);
  for (int i = 0; i < 2; ++i) carve_mlp<P>(c, q, 2 * B, false, false, W.Q[i]);
  return al256(c.off);
}
static int check_ibrl_act_nets(const dppo_net_desc* actor, const dppo_net_desc* q, int E) {
  if (int e = check_drop_actor(actor)) return e;
  if (int e = check_rlpd_q(q, actor ? actor->cond_dim : 0, E)) return e;
  if (q->in_dim != actor->cond_dim + actor->out_dim)
    return fail(-1, "Q descriptor does not pair with the actor: in_dim=%d must be cond_dim=%d + Ta*Da=%d", q->in_dim, actor->cond_dim,
                actor->out_dim);
  return 0;
}
int64_t dppo_ibrl_act_workspace_bytes(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, int64_t B) {
  if (check_ibrl_act_nets(actor, q, 2) || check_prec(prec)) return -1;
  if (B < 1 || B > 0x3fffffff) return fail(-1, "B out of range");
  return ws_bytes(prec, [&](Carver& c, auto p) {
    IbrlActWs<decltype(p)> W;
    return carve_ibrl_act<decltype(p)>(c, *actor, *q, B, W);
  });
}
template <class P>
static int ibrl_act_impl(const dppo_net_desc& a, const dppo_net_desc& q, const float* bcp, const char* bck, const float* rlp,
                         const char* rlk, dppo_gaussian_cfg cfg_bc, const dppo_gaussian_cfg& cfg_rl, const dppo_dropout* drop_bc,
                         const dppo_dropout* drop_rl, const float* qp0, const char* qk0, const float* qp1, const char* qk1,
                         const float* obs, const float* noise_bc, const float* noise_rl, int64_t B, const IbrlSelect& sel_in,
                         float* a_bc_out, float* a_rl_out, float* q_bc_out, float* q_rl_out, uint8_t* took_out, void* ws, int64_t wsb,
                         hipStream_t s) {
  IbrlActWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_ibrl_act<P>(c, a, q, B, W); })) return e;
  const PackLayout LA = pack_layout<P>(a, 0), LQ = pack_layout<P>(q, 0);
  const int AF = a.out_dim, OD = a.cond_dim;
  float* abc = a_bc_out ? a_bc_out : W.a_bc;
  float* arl = a_rl_out ? a_rl_out : W.a_rl;
  // both actors read one image of the observation rows
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, OD, B, W.A[0].in, LA.Kp0, s);
  W.A[1].in = W.A[0].in;
  cfg_bc.deterministic = 1;                       // sigma 1e-4, and the draw all the same
  const float* prm[2] = {bcp, rlp};
  const char* pk[2] = {bck, rlk};
  const dppo_gaussian_cfg* cfg[2] = {&cfg_bc, &cfg_rl};
  const dppo_dropout* drop[2] = {drop_bc, drop_rl};
  const float* noise[2] = {noise_bc, noise_rl};
  float* out[2] = {abc, arl};
  hipStream_t st = fork_side(s, 0);  // the BC actor beside the online one, then one member beside the other (ibrl.h: measured at B = 1)
  for (int i = 0; i < 2; ++i) {
    hipStream_t si = i == 0 ? st : s;
    mlp_forward<P>(a, prm[i], pk[i], LA, B, W.A[i], false, si, nullptr, false, drop[i]);
    GaussArgs g;
    memset(&g, 0, sizeof(g));
    g.cfg = *cfg[i], g.mean_pre = W.A[i].out, g.ldm = W.A[i].ldout, g.N = B, g.AF = AF;
    g.noise = noise[i], g.out_actions = out[i];
    launch_gauss_sample(g, si);
  }
  join_side(s, st, 0);
  IbrlRows r;
  memset(&r, 0, sizeof(r));
  r.ring.next_obs = obs, r.ring.obs_mod = B, r.ring.N = B, r.ring.OD = OD, r.ring.AD = AF;
  r.a_bc = abc, r.a_rl = arl, r.tin = W.Q[0].in, r.Kp = LQ.Kp0;
  launch_ibrl_rows<P>(r, s);
  W.Q[1].in = W.Q[0].in;
  st = fork_side(s, 0);
  mlp_forward<P>(q, qp1, qk1, LQ, 2 * B, W.Q[1], false, st);
  mlp_forward<P>(q, qp0, qk0, LQ, 2 * B, W.Q[0], false, s);
  join_side(s, st, 0);
  IbrlSelect sel = sel_in;
  sel.q1 = W.Q[0].out, sel.q2 = W.Q[1].out, sel.ldq = W.Q[0].ldout, sel.N = B, sel.AF = AF, sel.a_bc = abc, sel.a_rl = arl;
  sel.q_bc = q_bc_out ? q_bc_out : W.q_bc, sel.q_rl = q_rl_out ? q_rl_out : W.q_rl, sel.took_bc = took_out ? took_out : W.took;
  launch_ibrl_select(sel, s);
  return check_launch();
}
int dppo_ibrl_act(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, int E, const float* bc_params, const void* bc_packed,
                  const float* rl_params, const void* rl_packed, const dppo_gaussian_cfg* cfg_bc, const dppo_gaussian_cfg* cfg_rl,
                  const dppo_dropout* drop_bc, const dppo_dropout* drop_rl, const float* q_params, const void* const* q_packed,
                  int pair0, int pair1, const float* obs, const float* noise_bc, const float* noise_rl, int64_t B, int soft,
                  double beta, const float* u, uint32_t seed_lo, uint32_t seed_hi, float* actions, float* a_bc_out, float* a_rl_out,
                  float* q_bc_out, float* q_rl_out, uint8_t* took_bc_out, void* workspace, int64_t workspace_bytes,
                  dppo_stream_t stream) {
  if (int e = check_ibrl_act_nets(actor, q, E)) return e;
  if (int e = check_prec(prec)) return e;
  if (int e = check_gauss(actor, cfg_bc, nullptr)) return e;
  if (int e = check_gauss(actor, cfg_rl, nullptr)) return e;
  if (cfg_bc->std_mode != 0 || cfg_rl->std_mode != 0) return fail(-1, "IBRL's actors have a fixed std (std_mode 0)");
  if (drop_bc)
    if (int e = check_dropout(drop_bc)) return e;
  if (drop_rl)
    if (int e = check_dropout(drop_rl)) return e;
  if (!bc_params || !bc_packed || !rl_params || !rl_packed || !q_params || !q_packed || !obs || !actions || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_member_pair(pair0, pair1, E)) return e;
  if (!q_packed[pair0] || !q_packed[pair1]) return fail(-1, "null pointer: kernel image of a member of the pair");
  if (B < 1 || B > 0x3fffffff) return fail(-1, "B out of range");
  if (!(beta == beta)) return fail(-1, "soft_action_sample_beta is NaN");
  IbrlSelect sel;
  memset(&sel, 0, sizeof(sel));
  sel.soft = soft != 0, sel.beta = (float)beta, sel.u = u, sel.k0 = seed_lo, sel.k1 = seed_hi, sel.action = actions;
  const int64_t nq = param_layout(*q).total;
#define CALL(P)                                                                                                                     \
  ibrl_act_impl<P>(*actor, *q, bc_params, (const char*)bc_packed, rl_params, (const char*)rl_packed, *cfg_bc, *cfg_rl, drop_bc,     \
                   drop_rl, q_params + pair0 * nq, (const char*)q_packed[pair0], q_params + pair1 * nq,                             \
                   (const char*)q_packed[pair1], obs, noise_bc, noise_rl, B, sel, a_bc_out, a_rl_out, q_bc_out, q_rl_out,           \
                   took_bc_out, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// The TD loss with the better of the two proposals as bootstrap: ensemble_td_impl (further up, beside RLPD's)
int dppo_ibrl_q_loss_fwd_bwd(const dppo_net_desc* q, int prec, int E, const float* q_params, const void* const* q_packed,
                             const float* target_q_params, const void* const* target_q_packed, int pair0, int pair1,
                             const dppo_idql_batch* batch, int obs_dim, const float* next_actions_bc, const float* next_actions_rl,
                             int64_t N, double gamma, float* q_grad, double* stats, float* y_out, double* bc_share, void* workspace,
                             int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_rlpd_q(q, obs_dim, E)) return e;
  if (int e = check_prec(prec)) return e;
  if (!q_params || !q_packed || !target_q_params || !target_q_packed || !next_actions_bc || !next_actions_rl || !q_grad || !stats ||
      !workspace)
    return fail(-1, "null pointer");
  if (int e = check_ensemble_td(q_packed, target_q_packed, pair0, pair1, E, batch, N, 0x3fffffff, gamma)) return e;
  EnsembleBootstrap bs;
  memset(&bs, 0, sizeof(bs));
  bs.next_bc = next_actions_bc, bs.next_rl = next_actions_rl, bs.y_out = y_out, bs.bc_share = bc_share;
#define CALL(P)                                                                                                                   \
  ensemble_td_impl<P>(*q, E, q_params, q_packed, target_q_params, target_q_packed, pair0, pair1, *batch, obs_dim, bs, N, gamma, q_grad, \
                      stats, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// The actor's loss through the ensemble's mean (rlpd.h).  The actor and its head are SAC's (checked further down).
static int check_sac_actor(const dppo_net_desc* a);
static int check_sac_cfg(const dppo_net_desc* a, const dppo_sac_cfg* cfg);
static SacHead sac_head_of(const dppo_sac_cfg& cfg, const float* out, int ldo, int AF, const float* noise, int64_t N);
// SAC's actor ([mean | raw logvar], out_dim = 2 Ta*Da) against a Q trunk over [obs | a]; both descriptors already checked
static int check_sac_actor_q(const dppo_net_desc* a, const dppo_net_desc* q, int obs_dim) {
  if (a->cond_dim != obs_dim || q->in_dim - obs_dim != a->out_dim / 2)
    return fail(-1, "actor / Q descriptors do not pair: actor cond_dim=%d, Ta*Da=%d against obs_dim=%d, Q in_dim=%d", a->cond_dim,
                a->out_dim / 2, obs_dim, q->in_dim);
  return 0;
}
static int check_rlpd_pair(const dppo_net_desc* a, const dppo_net_desc* q, int obs_dim, int E) {
  if (int e = check_sac_actor(a)) return e;
  if (int e = check_rlpd_q(q, obs_dim, E)) return e;
  return check_sac_actor_q(a, q, obs_dim);
}
// An actor loss through M Q trunks (RLPD: the E LayerNorm members; twin: SAC's plain pair and Cal-QL's LayerNorm pair, with their
// choice per row): the chains' buffers, the actor's, and the head's rows
template <class P>
struct QActorWs : QChainWs<P> {
  MlpBufs<P> A;
  float *actions, *logp, *sig;
  float* qsel;    // twin only, as sel
  float* dout32;  // bf16 only: [N][2 AF] the head's gradient before its rounding to elem (SacTail::d_out32)
  uint8_t* sel;
};
template <class P>
static size_t carve_q_actor(Carver& c, const dppo_net_desc& a, const dppo_net_desc& q, int64_t N, int M, bool twin, QActorWs<P>& W) {
  const int AF = a.out_dim / 2;
  carve_mlp<P>(c, a, N, true, true, W.A);
  carve_q_chains<P>(c, q, AF, N, M, W);
  W.actions = (float*)c.take((size_t)N * AF * 4);
  W.logp = (float*)c.take((size_t)N * 4);
  W.sig = (float*)c.take((size_t)N * 4);
  W.qsel = twin ? (float*)c.take((size_t)N * 4) : nullptr;
  W.dout32 = P::ESIZE == 4 ? nullptr : (float*)c.take((size_t)N * 2 * AF * 4);
  W.sel = twin ? (uint8_t*)c.take((size_t)N) : nullptr;
  return al256(c.off);
}
int64_t dppo_rlpd_actor_workspace_bytes(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, int obs_dim, int64_t N, int E) {
  if (check_rlpd_pair(actor, q, obs_dim, E) || check_prec(prec)) return -1;
  if (int e = check_rows(N)) return e;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    QActorWs<decltype(p)> W;
    return carve_q_actor<decltype(p)>(c, *actor, *q, N, E, false, W);
  });
}
// The front of such a loss, on s: the actor's rows [obs | 0], the W0 action columns of the M trunks as [AF][M H], the actor's forward
// with the activations kept, and the head: sample, log-probability and ONE image of the critic's rows [obs | a | 0] that every trunk
// reads (no forward writes its input rows).  -> the head, which the tail runs backwards.
template <class P>
static SacHead q_actor_front(const dppo_net_desc& a, const dppo_net_desc& q, int M, const float* ap, const char* ak, const float* qp,
                             const dppo_sac_cfg& cfg, const dppo_idql_batch& b, int OD, int64_t N, const float* noise,
                             QActorWs<P>& W, float* actions, float* logp, hipStream_t s) {
  const PackLayout LA = pack_layout<P>(a, 0), LQ = pack_layout<P>(q, 0);
  const ParamLayout plq = param_layout(q);
  const int AF = a.out_dim / 2;
  IdqlRows r = idql_rows_of(b, N, OD, AF);
  r.vin = W.A.in, r.KpV = LA.Kp0;
  launch_idql_rows<P>(r, s);
  launch_pack_w0a<P>(qp, plq.total, plq.W0, q.in_dim, OD, AF, q.hidden, M, W.w0a, s);
  mlp_forward<P>(a, ap, ak, LA, N, W.A, true, s);
  SacHead h = sac_head_of(cfg, W.A.out, W.A.ldout, AF, noise, N);
  h.ring = idql_rows_of(b, N, OD, AF);
  h.actions = actions, h.logp = logp, h.sig_row = W.sig, h.q1in = h.q2in = W.Q[0].in, h.KpQ = LQ.Kp0;
  launch_sac_head<P>(h, s);
  for (int i = 1; i < M; ++i) W.Q[i].in = W.Q[0].in;
  return h;
}
// The back, on s: one tail over the M trunks' dh_0 whose epilogue is the head's backward, the caller's statistics, the actor's
// backward.  The tail is the one choice.  E >= 1: rlpd_tail_kernel, K = M H over a 16-lane butterfly, the sum divided by E (E members
// averaged; 1: the seeds carry the weights).  E = 0: sac_tail_kernel, K = 2H in index order from LDS rows.  The two add in different
// orders, so neither stands in for the other.
static void launch_actor_stats(const RlpdActorStats& a, hipStream_t s) { launch_rlpd_actor_stats(a, s); }
static void launch_actor_stats(const SacStats& a, hipStream_t s) { launch_sac_stats(a, s); }
template <class P, class Stats>
static void q_actor_back(const dppo_net_desc& a, const dppo_net_desc& q, int M, int E, const float* ap, const char* ak,
                         const SacHead& h, const double* alpha, const Stats& stats, int64_t N, QActorWs<P>& W, float* grad, float* d_a,
                         hipStream_t s) {
  const PackLayout LA = pack_layout<P>(a, 0);
  const int AF = a.out_dim / 2;
  if (E > 0) {
    RlpdTail tl;
    memset(&tl, 0, sizeof(tl));
    tl.head = h, tl.dh = W.dhcat, tl.wa = W.w0a, tl.K = M * q.hidden, tl.E = E, tl.alpha = alpha;
    tl.d_out = W.A.d_out, tl.ldd = LA.Kpo, tl.d_out32 = W.dout32, tl.d_a = d_a;
    launch_rlpd_tail<P>(tl, s);
  } else {
    SacTail tl;
    memset(&tl, 0, sizeof(tl));
    tl.head = h, tl.dh = W.dhcat, tl.wa = W.w0a, tl.H2 = M * q.hidden, tl.rows = qsm_tail_rows(M * q.hidden), tl.alpha = alpha;
    tl.d_out = W.A.d_out, tl.ldd = LA.Kpo, tl.d_out32 = W.dout32, tl.d_a = d_a;
    launch_sac_tail<P>(tl, s);
  }
  launch_actor_stats(stats, s);
  mlp_backward<P>(a, ap, ak, LA, N, W.A, grad, nullptr, nullptr, 0, s);
  if (W.dout32 != nullptr)  // the two heads' bias gradient again, from the unrounded rows
    launch_colsum<F32>(W.dout32, (int)N, 2 * AF, 2 * AF, W.A.part, REDUCE_BLOCKS, grad + param_layout(a).bout, 1.f, s);
}
template <class P>
static int rlpd_actor_impl(const dppo_net_desc& a, const dppo_net_desc& q, int E, const float* ap, const char* ak, const float* qp,
                           const void* const* qk, const dppo_sac_cfg& cfg, const dppo_idql_batch& b, int OD, int64_t N,
                           const float* noise, const double* alpha, float* grad, double* stats, float* d_a, float* logp_out,
                           float* actions_out, void* ws, int64_t wsb, hipStream_t s) {
  QActorWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_q_actor<P>(c, a, q, N, E, false, W); })) return e;
  const int64_t q_stride = W.Q[1].out - W.Q[0].out;
  for (int e = 1; e < E; ++e)
    if (W.Q[e].out - W.Q[0].out != e * q_stride) return fail(-1, "members' workspaces are not evenly spaced");
  const PackLayout LQ = pack_layout<P>(q, 0);
  const ParamLayout plq = param_layout(q);
  const int AF = a.out_dim / 2, H = q.hidden;
  float* logp = logp_out != nullptr ? logp_out : W.logp;
  const SacHead h = q_actor_front<P>(a, q, E, ap, ak, qp, cfg, b, OD, N, noise, W, actions_out != nullptr ? actions_out : W.actions, logp, s);
  // the members take turns on the caller's stream and the three side streams: each runs its forward and its chain back to back
  hipStream_t st[4] = {s, fork_side(s, 0), fork_side(s, 1), fork_side(s, 2)};
  for (int e = 0; e < E; ++e) {
    const float* prm = qp + e * plq.total;
    mlp_forward<P>(q, prm, (const char*)qk[e], LQ, N, W.Q[e], true, st[e & 3]);
    q_seeded_chain<P>(q, prm, (const char*)qk[e], LQ, N, W.Q[e], W.dza[e], W.dzb[e], (char*)W.dhcat + (size_t)e * H * P::ESIZE,
                      E * H, st[e & 3]);
  }
  for (int i = 1; i < 4; ++i) join_side(s, st[i], i - 1);
  RlpdActorStats sa;
  memset(&sa, 0, sizeof(sa));
  sa.q = W.Q[0].out, sa.q_stride = q_stride, sa.ldq = W.Q[0].ldout, sa.E = E, sa.logp = logp, sa.sig_row = W.sig, sa.alpha = alpha;
  sa.N = N, sa.AF = AF, sa.stats = stats;
  q_actor_back<P>(a, q, E, E, ap, ak, h, alpha, sa, N, W, grad, d_a, s);
  return check_launch();
}
int dppo_rlpd_actor_fwd_bwd(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, int E, const float* actor_params,
                            const void* actor_packed, const float* q_params, const void* const* q_packed, const dppo_sac_cfg* cfg,
                            const dppo_idql_batch* batch, int obs_dim, int64_t N, const float* noise, const double* alpha,
                            float* actor_grad, double* stats, float* d_a, float* logp_out, float* actions_out, void* workspace,
                            int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_rlpd_pair(actor, q, obs_dim, E)) return e;
  if (int e = check_prec(prec)) return e;
  if (int e = check_sac_cfg(actor, cfg)) return e;
  if (cfg->deterministic) return fail(-1, "the actor loss samples: deterministic must be 0");
  if (!actor_params || !actor_packed || !q_params || !q_packed || !alpha || !actor_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_member_images(q_packed, E)) return e;
  if (int e = check_rows(N)) return e;
  if (int e = check_idql_batch(batch, N, RING_OBS)) return e;
#define CALL(P)                                                                                                                    \
  rlpd_actor_impl<P>(*actor, *q, E, actor_params, (const char*)actor_packed, q_params, q_packed, *cfg, *batch, obs_dim, N, noise,   \
                     alpha, actor_grad, stats, d_a, logp_out, actions_out, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// IBRL's actor loss through the ensemble's min (ibrl.h).  The actor is the plain fixed-std trunk with dropout; the members, their
// forwards and their chains are RLPD's.  What differs from rlpd_actor_impl: the head (no log-probability, no second output half),
// the choice per row between the forwards and the chains, the tail without 1/E, and the dropout steps of the actor's backward.
template <class P>
struct IbrlActorWs : QChainWs<P> {
  MlpBufs<P> A;
  float *actions, *mu, *qmin;
  float* dout32;  // bf16 only: [N][AF] the head's gradient before its rounding to elem
  uint8_t* sel;
  uint8_t* mask;  // [LA][N][H]: the dropout mask the forward used
};
template <class P>
static size_t carve_ibrl_actor(Carver& c, const dppo_net_desc& a, const dppo_net_desc& q, int64_t N, int E, IbrlActorWs<P>& W) {
  const int AF = a.out_dim;
  carve_mlp<P>(c, a, N, true, true, W.A);
  carve_q_chains<P>(c, q, AF, N, E, W);
  W.actions = (float*)c.take((size_t)N * AF * 4);
  W.mu = (float*)c.take((size_t)N * AF * 4);
  W.qmin = (float*)c.take((size_t)N * 4);
  W.dout32 = P::ESIZE == 4 ? nullptr : (float*)c.take((size_t)N * AF * 4);
  W.sel = (uint8_t*)c.take((size_t)N);
  W.mask = (uint8_t*)c.take((size_t)(a.n_blocks + 1) * N * a.hidden);
  return al256(c.off);
}
static int check_ibrl_actor_nets(const dppo_net_desc* actor, const dppo_net_desc* q, int obs_dim, int E) {
  if (!actor || !q) return fail(-1, "null pointer: descriptor");
  if (int e = check_ibrl_act_nets(actor, q, E)) return e;
  if (actor->cond_dim != obs_dim)
    return fail(-1, "actor / Q descriptors do not pair: actor cond_dim=%d against obs_dim=%d", actor->cond_dim, obs_dim);
  return 0;
}
int64_t dppo_ibrl_actor_workspace_bytes(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, int obs_dim, int64_t N, int E) {
  if (check_ibrl_actor_nets(actor, q, obs_dim, E) || check_prec(prec)) return -1;
  if (int e = check_rows(N)) return e;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    IbrlActorWs<decltype(p)> W;
    return carve_ibrl_actor<decltype(p)>(c, *actor, *q, N, E, W);
  });
}
template <class P>
static int ibrl_actor_impl(const dppo_net_desc& a, const dppo_net_desc& q, int E, const float* ap, const char* ak, const float* qp,
                           const void* const* qk, const dppo_gaussian_cfg& cfg, const dppo_dropout* drop, const dppo_idql_batch& b,
                           int OD, int64_t N, const float* noise, float* grad, double* stats, float* d_a, float* actions_out,
                           float* qmin_out, uint8_t* sel_out, void* ws, int64_t wsb, hipStream_t s) {
  IbrlActorWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_ibrl_actor<P>(c, a, q, N, E, W); })) return e;
  const int64_t q_stride = W.Q[1].out - W.Q[0].out;
  for (int e = 1; e < E; ++e)
    if (W.Q[e].out - W.Q[0].out != e * q_stride) return fail(-1, "members' workspaces are not evenly spaced");
  const PackLayout LA = pack_layout<P>(a, 0), LQ = pack_layout<P>(q, 0);
  const ParamLayout plq = param_layout(q);
  const int AF = a.out_dim, H = q.hidden;
  // the actor's rows [obs | 0], the members' W0 action columns, the actor's forward with dropout: the mask it used is kept
  IdqlRows r = idql_rows_of(b, N, OD, AF);
  r.vin = W.A.in, r.KpV = LA.Kp0;
  launch_idql_rows<P>(r, s);
  launch_pack_w0a<P>(qp, plq.total, plq.W0, q.in_dim, OD, AF, H, E, W.w0a, s);
  const bool dropping = drop != nullptr && (drop->p > 0.f || drop->mask != nullptr);
  dppo_dropout dl;
  memset(&dl, 0, sizeof(dl));
  if (dropping) {
    dl = *drop;
    if (dl.mask_out == nullptr) dl.mask_out = W.mask;
  }
  mlp_forward<P>(a, ap, ak, LA, N, W.A, true, s, nullptr, false, dropping ? &dl : nullptr);
  IbrlHead h;
  memset(&h, 0, sizeof(h));
  h.cfg = cfg, h.ring = idql_rows_of(b, N, OD, AF), h.out = W.A.out, h.ldo = W.A.ldout, h.noise = noise;
  h.actions = actions_out != nullptr ? actions_out : W.actions, h.mu = W.mu, h.qin = W.Q[0].in, h.Kp = LQ.Kp0;
  launch_ibrl_head<P>(h, s);
  for (int e = 1; e < E; ++e) W.Q[e].in = W.Q[0].in;
  // the members' forwards on the caller's stream and the three side streams; the choice needs all of them
  hipStream_t st[4] = {s, fork_side(s, 0), fork_side(s, 1), fork_side(s, 2)};
  for (int e = 0; e < E; ++e) mlp_forward<P>(q, qp + e * plq.total, (const char*)qk[e], LQ, N, W.Q[e], true, st[e & 3]);
  for (int i = 1; i < 4; ++i) join_side(s, st[i], i - 1);
  IbrlMin mn;
  memset(&mn, 0, sizeof(mn));
  mn.q = W.Q[0].out, mn.q_stride = q_stride, mn.ldq = W.Q[0].ldout, mn.E = E, mn.N = N, mn.H = H, mn.act = q.act;
  for (int e = 0; e < E; ++e)
    mn.wout[e] = (const char*)qk[e] + LQ.Wout, mn.z[e] = W.Q[e].z1[q.n_blocks - 1], mn.dz[e] = W.dza[e];
  mn.qmin = qmin_out != nullptr ? qmin_out : W.qmin, mn.sel = sel_out != nullptr ? sel_out : W.sel;
  launch_ibrl_min<P>(mn, s);
  // every member's chain from its seed (zero on the rows it did not win), on the same streams
  for (int i = 1; i < 4; ++i) st[i] = fork_side(s, i - 1);
  for (int e = 0; e < E; ++e)
    q_chain_from_seed<P>(q, qp + e * plq.total, (const char*)qk[e], LQ, N, W.Q[e], W.dza[e], W.dzb[e],
                         (char*)W.dhcat + (size_t)e * H * P::ESIZE, E * H, st[e & 3]);
  for (int i = 1; i < 4; ++i) join_side(s, st[i], i - 1);
  IbrlTail tl;
  memset(&tl, 0, sizeof(tl));
  tl.dh = W.dhcat, tl.wa = W.w0a, tl.K = E * H, tl.AF = AF, tl.tanh_mean = cfg.tanh_mean, tl.N = N, tl.mu = W.mu;
  tl.d_out = W.A.d_out, tl.ldd = LA.Kpo, tl.d_out32 = W.dout32, tl.d_a = d_a;
  launch_ibrl_tail<P>(tl, s);
  IbrlActorStats sa;
  memset(&sa, 0, sizeof(sa));
  sa.qmin = mn.qmin, sa.q = W.Q[0].out, sa.q_stride = q_stride, sa.ldq = W.Q[0].ldout, sa.E = E, sa.N = N, sa.stats = stats;
  launch_ibrl_actor_stats(sa, s);
  DropBwd db;
  memset(&db, 0, sizeof(db));
  if (dropping) db.mask = dl.mask_out, db.scale = 1.f / (1.f - dl.p);
  mlp_backward<P>(a, ap, ak, LA, N, W.A, grad, nullptr, nullptr, 0, s, nullptr, dropping ? &db : nullptr);
  if (W.dout32 != nullptr)  // the out bias again, from the unrounded rows
    launch_colsum<F32>(W.dout32, (int)N, AF, AF, W.A.part, REDUCE_BLOCKS, grad + param_layout(a).bout, 1.f, s);
  return check_launch();
}
int dppo_ibrl_actor_fwd_bwd(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, int E, const float* actor_params,
                            const void* actor_packed, const float* q_params, const void* const* q_packed,
                            const dppo_gaussian_cfg* cfg, const dppo_dropout* drop, const dppo_idql_batch* batch, int obs_dim,
                            int64_t N, const float* noise, float* actor_grad, double* stats, float* d_a, float* actions_out,
                            float* qmin_out, uint8_t* sel_out, void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_ibrl_actor_nets(actor, q, obs_dim, E)) return e;
  if (int e = check_prec(prec)) return e;
  if (int e = check_gauss(actor, cfg, nullptr)) return e;
  if (cfg->std_mode != 0) return fail(-1, "IBRL's actor has a fixed std (std_mode 0): a learned std is not built here");
  if (cfg->deterministic) return fail(-1, "the actor loss samples: deterministic must be 0");
  if (drop)
    if (int e = check_dropout(drop)) return e;
  if (!actor_params || !actor_packed || !q_params || !q_packed || !actor_grad || !stats || !workspace) return fail(-1, "null pointer");
  if (int e = check_member_images(q_packed, E)) return e;
  if (int e = check_rows(N)) return e;
  if (int e = check_idql_batch(batch, N, RING_OBS)) return e;
#define CALL(P)                                                                                                                       \
  ibrl_actor_impl<P>(*actor, *q, E, actor_params, (const char*)actor_packed, q_params, q_packed, *cfg, drop, *batch, obs_dim, N, noise, \
                     actor_grad, stats, d_a, actions_out, qmin_out, sel_out, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- Cal-QL (calql.hip): the conservative critic loss on a twin of LayerNorm Q trunks --------------------------------------------
static int check_calql_q(const dppo_net_desc* q, int obs_dim, int64_t N, int R, int S) {
  if (int e = check_ln_q(q, obs_dim, "Cal-QL's twin is two plain trunks with LayerNorm (plain = 1, use_layernorm = 1); a twin without LayerNorm trains through dppo_sac_q_loss_fwd_bwd"))
    return e;
  if (R < 1 || R > CALQL_MAX_SAMPLES) return fail(-1, "n_random=%d random actions per row out of [1, %d]", R, CALQL_MAX_SAMPLES);
  if (S < 1 || S > CALQL_MAX_SAMPLES) return fail(-1, "n_next=%d policy samples per next observation out of [1, %d]", S, CALQL_MAX_SAMPLES);
  if (N < 1 || N * (R + 3) > 0x7fffffff || N * S > 0x7fffffff) return fail(-1, "N out of range");
  return 0;
}
template <class P>
struct CalqlWs {
  MlpBufs<P> Q[2], T[2];
  double *partial, *partial_d;
  float *r, *term, *y, *lse;
};
template <class P>
static size_t carve_calql(Carver& c, const dppo_net_desc& q, int64_t N, int R, int S, CalqlWs<P>& W) {
  W.partial = (double*)c.take((size_t)2 * rlpd_blocks(N) * 4 * sizeof(double));
  W.partial_d = (double*)c.take((size_t)2 * rlpd_blocks(N) * sizeof(double));
  W.r = (float*)c.take((size_t)N * 4);
  W.term = (float*)c.take((size_t)N * 4);
  W.y = (float*)c.take((size_t)N * 4);
  W.lse = (float*)c.take(2 * 4);
  for (int i = 0; i < 2; ++i) carve_mlp<P>(c, q, N * (R + 3), true, true, W.Q[i]);
  for (int i = 0; i < 2; ++i) carve_mlp<P>(c, q, N * S, false, false, W.T[i]);
  return al256(c.off);
}
int64_t dppo_calql_q_loss_workspace_bytes(const dppo_net_desc* q, int prec, int obs_dim, int64_t N, int n_random, int n_next) {
  if (check_calql_q(q, obs_dim, N, n_random, n_next) || check_prec(prec)) return -1;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    CalqlWs<decltype(p)> W;
    return carve_calql<decltype(p)>(c, *q, N, n_random, n_next, W);
  });
}
template <class P>
static int calql_impl(const dppo_net_desc& q, const float* qp, const char* qk1, const char* qk2, const float* tp, const char* tk1,
                      const char* tk2, const dppo_calql_cfg& cfg, const dppo_idql_batch& b, int OD, const float* returns,
                      const float* next_actions, const float* pi_actions, const float* log_pi, const float* pi_next_actions,
                      const float* log_pi_next, const float* random_actions, int64_t N, double gamma, float* qgrad, double* stats,
                      float* y_out, float* random_out, void* ws, int64_t wsb, hipStream_t s) {
  CalqlWs<P> W;
  const int R = cfg.n_random, S = cfg.n_next;
  const int64_t M = N * (R + 3), MT = N * S;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_calql<P>(c, q, N, R, S, W); })) return e;
  const PackLayout L = pack_layout<P>(q, 0);
  const int64_t nq = param_layout(q).total;
  // both trunks read the same M rows, both targets the same N S rows: one image each
  CalqlRows r;
  memset(&r, 0, sizeof(r));
  r.ring = idql_rows_of(b, N, OD, q.in_dim - OD);
  r.random_actions = random_actions, r.pi_actions = pi_actions, r.pi_next_actions = pi_next_actions, r.next_actions = next_actions;
  r.R = R, r.S = S, r.seed_lo = cfg.seed_lo, r.seed_hi = cfg.seed_hi, r.qin = W.Q[0].in, r.tin = W.T[0].in, r.KpQ = L.Kp0;
  r.r_out = W.r, r.term_out = W.term, r.random_out = random_out;
  launch_calql_rows<P>(r, s);
  W.Q[1].in = W.Q[0].in, W.T[1].in = W.T[0].in;
  // Q2 and the two target trunks on the three side streams beside Q1 (and the L, L' reduction in front of it)
  hipStream_t s2 = fork_side(s, 0), s3 = fork_side(s, 1), s4 = fork_side(s, 2);
  mlp_forward<P>(q, tp, tk1, L, MT, W.T[0], false, s3);
  mlp_forward<P>(q, tp + nq, tk2, L, MT, W.T[1], false, s4);
  mlp_forward<P>(q, qp + nq, qk2, L, M, W.Q[1], true, s2);
  if (!cfg.per_row_logpi) launch_calql_lse(log_pi, log_pi_next, N, W.lse, s);
  mlp_forward<P>(q, qp, qk1, L, M, W.Q[0], true, s);
  if (s2 != s) join_side(s, s2, 0);
  if (s3 != s) join_side(s, s3, 1);
  if (s4 != s) join_side(s, s4, 2);
  launch_calql_target(W.T[0].out, W.T[1].out, W.T[0].ldout, W.r, W.term, (float)gamma, N, S, W.y, y_out, s);
  CalqlLoss l;
  memset(&l, 0, sizeof(l));
  l.q = W.Q[0].out, l.q_stride = W.Q[1].out - W.Q[0].out, l.ldq = W.Q[0].ldout, l.y = W.y, l.returns = returns;
  l.log_pi = log_pi, l.log_pi_next = log_pi_next, l.lse = W.lse, l.per_row = cfg.per_row_logpi ? 1 : 0;
  l.w = cfg.min_q_weight, l.clip_min = cfg.clip_diff_min, l.clip_max = cfg.clip_diff_max, l.c = cfg.log_rand_pi, l.N = N, l.R = R;
  l.d_out = W.Q[0].d_out, l.d_stride = (char*)W.Q[1].d_out - (char*)W.Q[0].d_out, l.ldd = L.Kpo;
  l.partial = W.partial, l.partial_d = W.partial_d, l.stats = stats;
  launch_calql_loss<P>(l, s);
  s2 = fork_side(s, 0);
  mlp_backward<P>(q, qp + nq, qk2, L, M, W.Q[1], qgrad + nq, nullptr, nullptr, 0, s2);
  mlp_backward<P>(q, qp, qk1, L, M, W.Q[0], qgrad, nullptr, nullptr, 0, s);
  if (s2 != s) join_side(s, s2, 0);
  // (rlpd.h has the reason: the column sum of the elem rows loses the bias gradient in bf16; partial's fourth sum is unrounded)
  launch_rlpd_out_bias(W.partial, N, 2, qgrad, nq, param_layout(q).bout, s);
  return check_launch();
}
int dppo_calql_q_loss_fwd_bwd(const dppo_net_desc* q, int prec, const float* q_params, const void* q1_packed, const void* q2_packed,
                              const float* target_q_params, const void* target_q1_packed, const void* target_q2_packed,
                              const dppo_calql_cfg* cfg, const dppo_idql_batch* batch, int obs_dim, const float* returns,
                              const float* next_actions, const float* pi_actions, const float* log_pi, const float* pi_next_actions,
                              const float* log_pi_next, const float* random_actions, int64_t N, double gamma, float* q_grad,
                              double* stats, float* y_out, float* random_out, void* workspace, int64_t workspace_bytes,
                              dppo_stream_t stream) {
  if (!cfg) return fail(-1, "null pointer: cfg");
  if (int e = check_calql_q(q, obs_dim, N, cfg->n_random, cfg->n_next)) return e;
  if (int e = check_prec(prec)) return e;
  if (!(cfg->clip_diff_min <= cfg->clip_diff_max))
    return fail(-1, "clip_diff_min=%g must not exceed clip_diff_max=%g", (double)cfg->clip_diff_min, (double)cfg->clip_diff_max);
  if (!(cfg->min_q_weight >= 0.f && cfg->min_q_weight <= 3.0e38f)) return fail(-1, "min_q_weight=%g must be finite and >= 0", (double)cfg->min_q_weight);
  if (!q_params || !q1_packed || !q2_packed || !target_q_params || !target_q1_packed || !target_q2_packed || !returns ||
      !next_actions || !pi_actions || !log_pi || !pi_next_actions || !log_pi_next || !q_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_idql_batch(batch, N, RING_TRANSITION)) return e;
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(-1, "discount gamma=%g outside [0, 1]", gamma);
#define CALL(P)                                                                                                                     \
  calql_impl<P>(*q, q_params, (const char*)q1_packed, (const char*)q2_packed, target_q_params, (const char*)target_q1_packed,       \
                (const char*)target_q2_packed, *cfg, *batch, obs_dim, returns, next_actions, pi_actions, log_pi, pi_next_actions,   \
                log_pi_next, random_actions, N, gamma, q_grad, stats, y_out, random_out, workspace, workspace_bytes,               \
                (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// The actor's loss through the minimum of the LayerNorm twin (calql.h).  The actor and its head are SAC's.
static int check_calql_pair(const dppo_net_desc* a, const dppo_net_desc* q, int obs_dim, int64_t N) {
  if (int e = check_sac_actor(a)) return e;
  if (int e = check_calql_q(q, obs_dim, N, 1, 1)) return e;
  return check_sac_actor_q(a, q, obs_dim);
}
static int64_t twin_actor_ws_bytes(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, int64_t N) {
  return ws_bytes(prec, [&](Carver& c, auto p) {
    QActorWs<decltype(p)> W;
    return carve_q_actor<decltype(p)>(c, *actor, *q, N, 2, true, W);
  });
}
int64_t dppo_calql_actor_workspace_bytes(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, int obs_dim, int64_t N) {
  if (check_calql_pair(actor, q, obs_dim, N) || check_prec(prec)) return -1;
  return twin_actor_ws_bytes(actor, q, prec, N);
}
// The actor's loss through the smaller Q of a twin, per row: SAC's (plain trunks) and Cal-QL's (LayerNorm trunks).  Between the shared
// front and back, both forwards side by side, the choice per row, which seeds both chains, and the two chains side by side.  The
// descriptor decides the three things that differ: the select kernel (SAC: a tie goes to Q1, the other trunk's seed is 0, sel_out is
// a copy; Cal-QL: a tie's seeds are halves), the LayerNorm steps of the chain, and the tail (q_actor_back).
template <class P>
static int twin_actor_impl(const dppo_net_desc& a, const dppo_net_desc& q, const float* ap, const char* ak, const float* qp,
                           const char* qk1, const char* qk2, const dppo_sac_cfg& cfg, const dppo_idql_batch& b, int OD, int64_t N,
                           const float* noise, const double* alpha, float* grad, double* stats, float* d_a, float* logp_out,
                           uint8_t* sel_out, float* actions_out, void* ws, int64_t wsb, hipStream_t s) {
  QActorWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_q_actor<P>(c, a, q, N, 2, true, W); })) return e;
  const PackLayout LQ = pack_layout<P>(q, 0);
  const int AF = a.out_dim / 2, H = q.hidden;
  float* logp = logp_out != nullptr ? logp_out : W.logp;
  const SacHead h = q_actor_front<P>(a, q, 2, ap, ak, qp, cfg, b, OD, N, noise, W, actions_out != nullptr ? actions_out : W.actions, logp, s);
  const float* prm[2] = {qp, qp + param_layout(q).total};
  const char* qk[2] = {qk1, qk2};
  hipStream_t s2 = fork_side(s, 0);
  mlp_forward<P>(q, prm[1], qk[1], LQ, N, W.Q[1], true, s2);
  mlp_forward<P>(q, prm[0], qk[0], LQ, N, W.Q[0], true, s);
  if (s2 != s) join_side(s, s2, 0);
  auto twin_of = [&](auto& sl) {  // what both select kernels read, and the two seeds they write
    memset(&sl, 0, sizeof(sl));
    sl.q1 = W.Q[0].out, sl.q2 = W.Q[1].out, sl.ldq = W.Q[0].ldout, sl.wout1 = qk[0] + LQ.Wout, sl.wout2 = qk[1] + LQ.Wout;
    sl.z1 = W.Q[0].z1[q.n_blocks - 1], sl.z2 = W.Q[1].z1[q.n_blocks - 1], sl.N = N, sl.H = H, sl.act = q.act;
    sl.dz1 = W.dza[0], sl.dz2 = W.dza[1], sl.qsel = W.qsel;
  };
  if (q.use_layernorm) {
    CalqlSelect sl;
    twin_of(sl);
    sl.sel = sel_out != nullptr ? sel_out : W.sel;
    launch_calql_select<P>(sl, s);
  } else {
    SacSelect sl;
    twin_of(sl);
    sl.sel = W.sel, sl.sel_out = sel_out;
    launch_sac_select<P>(sl, s);
  }
  s2 = fork_side(s, 0);
  q_chain_from_seed<P>(q, prm[1], qk[1], LQ, N, W.Q[1], W.dza[1], W.dzb[1], (char*)W.dhcat + (size_t)H * P::ESIZE, 2 * H, s2);
  q_chain_from_seed<P>(q, prm[0], qk[0], LQ, N, W.Q[0], W.dza[0], W.dzb[0], W.dhcat, 2 * H, s);
  if (s2 != s) join_side(s, s2, 0);
  SacStats st;
  memset(&st, 0, sizeof(st));
  st.qsel = W.qsel, st.logp = logp, st.sig_row = W.sig, st.alpha = alpha, st.N = N, st.AF = AF, st.stats = stats;
  q_actor_back<P>(a, q, 2, q.use_layernorm ? 1 : 0, ap, ak, h, alpha, st, N, W, grad, d_a, s);  // (E = 1: the seeds carry the weights)
  return check_launch();
}
int dppo_calql_actor_fwd_bwd(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, const float* actor_params,
                             const void* actor_packed, const float* q_params, const void* q1_packed, const void* q2_packed,
                             const dppo_sac_cfg* cfg, const dppo_idql_batch* batch, int obs_dim, int64_t N, const float* noise,
                             const double* alpha, float* actor_grad, double* stats, float* d_a, float* logp_out, uint8_t* sel_out,
                             float* actions_out, void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_calql_pair(actor, q, obs_dim, N)) return e;
  if (int e = check_prec(prec)) return e;
  if (int e = check_sac_cfg(actor, cfg)) return e;
  if (cfg->deterministic) return fail(-1, "the actor loss samples: deterministic must be 0");
  if (!actor_params || !actor_packed || !q_params || !q1_packed || !q2_packed || !alpha || !actor_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_idql_batch(batch, N, RING_OBS)) return e;
#define CALL(P)                                                                                                                      \
  twin_actor_impl<P>(*actor, *q, actor_params, (const char*)actor_packed, q_params, (const char*)q1_packed, (const char*)q2_packed, \
                     *cfg, *batch, obs_dim, N, noise, alpha, actor_grad, stats, d_a, logp_out, sel_out, actions_out, workspace,      \
                      workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- DQL (dql.hip): the actor loss whose gradient flows through the K-step sampling chain ----------------------------------------
static int check_dql(const dppo_net_desc* a, const dppo_net_desc* q, int obs_dim) {
  if (int e = check_net(a)) return e;
  if (a->kind != 0) return fail(-1, "dppo_dql_actor_fwd_bwd needs an actor descriptor");
  if (a->plain)
    return fail(-1, "the gradient through the sampling chain is built for residual actors (a plain actor, residual_style=False, is not; no shipped cfg has one)");
  if (a->use_layernorm) return fail(-1, "the gradient through the sampling chain runs on the layered GEMM path: LayerNorm blocks (fused kernels only) are not built");
  if (int e = check_qsm_q(q, obs_dim)) return e;
  if (int e = check_qsm_plain(q)) return e;
  if (a->cond_dim != obs_dim || q->in_dim - obs_dim != a->act_flat)
    return fail(-1, "actor / Q descriptors do not pair: actor cond_dim=%d, Ta*Da=%d against obs_dim=%d, Q in_dim=%d", a->cond_dim,
                a->act_flat, obs_dim, q->in_dim);
  if (qsm_tail_rows(a->hidden) < 1) return fail(-1, "hidden=%d too wide for the chain's link", a->hidden);
  return 0;
}
static int check_dql_sizes(const dppo_net_desc* a, int64_t N, int K) {
  if (int e = check_rows(N)) return e;
  if (K < 1 || K > 1024) return fail(-1, "K=%d denoising steps outside [1, 1024]", K);
  if ((int64_t)(K + 1) * N > 0x7fffffff) return fail(-1, "(K + 1) * N out of range");
  if ((int64_t)K * a->time_dim > 65536 || time_backward_lds_bytes(K, a->time_dim) > 156 * 1024)
    return fail(-1, "K * time_dim = %d too large for the time-embedding backward (LDS)", K * a->time_dim);
  return 0;
}
template <class P>
struct DqlWs {
  MlpBufs<P> A, Q1, Q2;
  int32_t* krow;
  void *dza, *dzb, *dhcat;  // the chosen Q trunk's data-gradient chain (q_seeded_chain)
  void *w0x, *w0q;          // [AF][H] / [AF][Hq] elem: the x columns of the actor's W0, the action columns of the chosen trunk's
  float *dx, *scale;
  double* rowsum;
  uint8_t* mask;
  char* wimg;  // the actor's row-major GEMM operands (W and W^T), which dppo_pack_net leaves out where the fused kernels cover the shape
};
template <class P>
static size_t carve_dql(Carver& c, const dppo_net_desc& a, const dppo_net_desc& q, int64_t N, int K, DqlWs<P>& W) {
  const size_t ES = P::ESIZE;
  const int64_t M = (int64_t)(K + 1) * N;
  carve_mlp<P>(c, a, M, true, true, W.A);
  carve_mlp<P>(c, q, N, true, false, W.Q1);
  carve_mlp<P>(c, q, N, true, false, W.Q2);
  W.krow = (int32_t*)c.take((size_t)M * 4);
  W.dza = c.take((size_t)N * q.hidden * ES);
  W.dzb = c.take((size_t)N * q.hidden * ES);
  W.dhcat = c.take((size_t)N * 2 * q.hidden * ES);
  W.w0x = c.take((size_t)a.act_flat * a.hidden * ES);
  W.w0q = c.take((size_t)a.act_flat * q.hidden * ES);
  W.dx = (float*)c.take((size_t)N * a.act_flat * 4);
  W.scale = (float*)c.take(256);
  W.rowsum = (double*)c.take((size_t)N * 8);
  W.mask = (uint8_t*)c.take((size_t)N * K * a.act_flat);
  W.wimg = (char*)c.take(pack_layout<P>(a, 0).total);
  return al256(c.off);
}
int64_t dppo_dql_actor_workspace_bytes(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, int obs_dim, int64_t N, int K) {
  if (check_dql(actor, q, obs_dim) || check_prec(prec) || check_dql_sizes(actor, N, K)) return -1;
  return ws_bytes(prec, [&](Carver& c, auto p) {
    DqlWs<decltype(p)> W;
    return carve_dql<decltype(p)>(c, *actor, *q, N, K, W);
  });
}
// Data gradients of the residual trunk for rows [r0, r0 + N): d_out -> dh_all[nb] .. dh_all[0] and dz1_all[..], each kept at the
// rows' own place (backward_layered's steps without their weight gradients; the derivative sources are the layered forward's)
template <class P>
static void dql_actor_chain(const dppo_net_desc& d, const char* pk, const PackLayout& L, int64_t N, int64_t r0, MlpBufs<P>& B,
                            hipStream_t s) {
  const size_t ES = P::ESIZE;
  const int H = d.hidden, nb = d.n_blocks;
  auto at = [&](const void* p, int ld, size_t es) { return (void*)((char*)p + (size_t)r0 * ld * es); };
  GemmNT g;
  memset(&g, 0, sizeof(g));
  g.M = (int)N, g.N = H, g.Kp = L.Kpo, g.ldx = L.Kpo, g.ldw = L.Kpo, g.ldo = H;
  g.X = at(B.d_out, L.Kpo, ES), g.W = pk + L.WoutT, g.out_pre = at(B.dh_all[nb], H, ES);
  launch_gemm_nt<P>(g, s);
  for (int b = nb - 1; b >= 0; --b) {
    memset(&g, 0, sizeof(g));  // dz1 = (dh . W2) * act'(z1)
    g.M = (int)N, g.N = H, g.Kp = H, g.ldx = H, g.ldw = H, g.ldo = H;
    g.X = at(B.dh_all[b + 1], H, ES), g.W = pk + L.W2T[b], g.dsrc = at(B.z1[b], H, ES), g.dsrc_kind = 2, g.dsrc_ld = H, g.dact = d.act;
    g.out_pre = at(B.dz1_all[b], H, ES);
    launch_gemm_nt<P>(g, s);
    memset(&g, 0, sizeof(g));  // dh_b = dh_{b+1} + (dz1 . W1) * act'(h_b)
    g.M = (int)N, g.N = H, g.Kp = H, g.ldx = H, g.ldw = H, g.ldo = H;
    g.X = at(B.dz1_all[b], H, ES), g.W = pk + L.W1T[b], g.dsrc = at(B.h[b], H, 4), g.dsrc_kind = 1, g.dsrc_ld = H, g.dact = d.act;
    g.add = at(B.dh_all[b + 1], H, ES), g.ldadd = H, g.out_pre = at(B.dh_all[b], H, ES);
    launch_gemm_nt<P>(g, s);
  }
}
// Every parameter gradient from the stored per-row data gradients, once over all M rows
template <class P>
static void dql_weight_grads(const dppo_net_desc& d, const float* prm, const char* pk, const PackLayout& L, int64_t M, MlpBufs<P>& B,
                             float* grad, const int32_t* krow, const dppo_step* tsteps, int K, hipStream_t s) {
  const ParamLayout pl = param_layout(d);
  const int H = d.hidden, nb = d.n_blocks;
  weight_grad<P>(B.d_out, L.Kpo, d.out_dim, B.hE, H, H, M, B, grad + pl.Wout, H, s);
  launch_colsum<P>(B.d_out, (int)M, d.out_dim, L.Kpo, B.part, REDUCE_BLOCKS, grad + pl.bout, 1.f, s);
  for (int b = nb - 1; b >= 0; --b) {
    weight_grad<P>(B.dh_all[b + 1], H, H, B.a2[b], H, H, M, B, grad + pl.l2w[b], H, s);
    launch_colsum<P>(B.dh_all[b + 1], (int)M, H, H, B.part, REDUCE_BLOCKS, grad + pl.l2b[b], 1.f, s);
    weight_grad<P>(B.dz1_all[b], H, H, B.a1[b], H, H, M, B, grad + pl.l1w[b], H, s);
    launch_colsum<P>(B.dz1_all[b], (int)M, H, H, B.part, REDUCE_BLOCKS, grad + pl.l1b[b], 1.f, s);
  }
  weight_grad<P>(B.dh_all[0], H, H, B.in, L.Kp0, d.in_dim, M, B, grad + pl.W0, d.in_dim, s);
  launch_colsum<P>(B.dh_all[0], (int)M, H, H, B.part, REDUCE_BLOCKS, grad + pl.b0, 1.f, s);
  time_embedding_grad<P>(d, prm, pk, L, M, B, B.dh_all[0], grad, krow, tsteps, K, s);
  if (d.cond_hidden > 0) cond_backward<P>(d, prm, pk, L, M, B, B.dh_all[0], B.cin, grad, s);
}
template <class P>
static int dql_impl(const dppo_net_desc& a, const dppo_net_desc& q, const float* ap, const char* ak, const float* qp, const char* qk1,
                    const char* qk2, const dppo_diffusion_cfg& cfg, const dppo_step* tsteps, int K, const dppo_idql_batch& b,
                    int OD, int64_t N, const float* chains, const float* noise_bc, const int64_t* t_bc, const float* sa,
                    const float* sb, double eta, int which, float* grad, double* stats, uint8_t* masks, float* d_a, void* ws,
                    int64_t wsb, hipStream_t s) {
  DqlWs<P> W;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_dql<P>(c, a, q, N, K, W); })) return e;
  const size_t ES = P::ESIZE;
  const PackLayout LA = pack_layout<P>(a, 0), LQ = pack_layout<P>(q, 0);
  const ParamLayout pla = param_layout(a), plq = param_layout(q);
  const int64_t M = (int64_t)(K + 1) * N;
  const int H = a.hidden, Hq = q.hidden, AF = a.act_flat;
  uint8_t* mask = masks != nullptr ? masks : W.mask;
  // d_out's padding columns are the K padding of the chain's first GEMM: zero; its data columns are written slab by slab below
  if (hipMemsetAsync(W.A.d_out, 0, (size_t)M * LA.Kpo * ES, s) != hipSuccess) return fail(-2, "hipMemsetAsync failed");
  DqlRows r;
  memset(&r, 0, sizeof(r));
  r.ring = idql_rows_of(b, N, OD, AF);
  r.chains = chains, r.noise_bc = noise_bc, r.t_bc = t_bc, r.sa = sa, r.sb = sb, r.temb = (const float*)(ak + LA.temb);
  r.K = K, r.AF = AF, r.td = a.time_dim, r.obs_in_a = a.cond_hidden > 0 ? 0 : 1, r.inA = W.A.in, r.KpA = LA.Kp0;
  r.inC = a.cond_hidden > 0 ? W.A.cin : nullptr, r.KpC = LA.Kpc, r.krow = W.krow, r.q1in = W.Q1.in, r.q2in = W.Q2.in, r.KpQ = LQ.Kp0;
  launch_dql_rows<P>(r, s);
  // the twin's forwards and the chosen trunk's data-gradient chain on side stream 0 beside the actor's forward over all rows
  hipStream_t sq = fork_side(s, 0);
  mlp_forward<P>(q, qp, qk1, LQ, N, W.Q1, true, sq);
  mlp_forward<P>(q, qp + plq.total, qk2, LQ, N, W.Q2, true, sq);
  q_seeded_chain<P>(q, qp + (which ? plq.total : 0), which ? qk2 : qk1, LQ, N, which ? W.Q2 : W.Q1, W.dza, W.dzb, W.dhcat, 2 * Hq, sq);
  launch_dql_pack_cols<P>(qp + (which ? plq.total : 0) + plq.W0, q.in_dim, OD, AF, Hq, W.w0q, sq);
  launch_dql_pack_cols<P>(ap + pla.W0, a.in_dim, 0, AF, H, W.w0x, s);
  // The layered path's operands: part of the packed image only where the fused kernels do NOT cover the shape (pack_impl);
  // otherwise cast / transposed here, into an image of the same layout (a dozen small launches, whatever K)
  const char* wk = ak;
  if (fused_ok<P>(a)) {
    char* w = W.wimg;
    launch_cast_pad<P>(ap + pla.W0, H, a.in_dim, a.in_dim, w + LA.W0, LA.Kp0, s);
    for (int b = 0; b < a.n_blocks; ++b) {
      launch_cast_pad<P>(ap + pla.l1w[b], H, H, H, w + LA.W1[b], H, s);
      launch_cast_pad<P>(ap + pla.l2w[b], H, H, H, w + LA.W2[b], H, s);
      launch_transpose_cast<P>(ap + pla.l1w[b], H, H, H, 0, w + LA.W1T[b], H, s);
      launch_transpose_cast<P>(ap + pla.l2w[b], H, H, H, 0, w + LA.W2T[b], H, s);
    }
    launch_cast_pad<P>(ap + pla.Wout, a.out_dim, H, H, w + LA.Wout, H, s);
    launch_transpose_cast<P>(ap + pla.Wout, a.out_dim, H, H, 0, w + LA.WoutT, LA.Kpo, s);
    wk = w;
  }
  if (a.cond_hidden > 0) cond_encode<P>(a, ap, ak, LA, M, W.A.cin, W.A, W.A.in, nullptr, 0, true, s);
  mlp_forward<P>(a, ap, wk, LA, M, W.A, true, s, nullptr, true);
  DqlPost po;
  memset(&po, 0, sizeof(po));
  po.chains = chains, po.eps = W.A.out, po.lde = W.A.ldout, po.tsteps = tsteps, po.N = N, po.K = K, po.AF = AF;
  po.has_clip = cfg.has_denoised_clip, po.clip = cfg.denoised_clip, po.mask = mask;
  launch_dql_post(po, s);
  DqlBc bc;
  memset(&bc, 0, sizeof(bc));
  bc.eps = W.A.out + (size_t)K * N * W.A.ldout, bc.lde = W.A.ldout, bc.noise = noise_bc, bc.N = N, bc.AF = AF;
  bc.d_out = (char*)W.A.d_out + (size_t)K * N * LA.Kpo * ES, bc.ldd = LA.Kpo, bc.rowsum = W.rowsum;
  launch_dql_bc<P>(bc, s);
  dql_actor_chain<P>(a, wk, LA, N, (int64_t)K * N, W.A, s);
  if (sq != s) join_side(s, sq, 0);
  DqlStats st;
  memset(&st, 0, sizeof(st));
  st.q1 = W.Q1.out, st.q2 = W.Q2.out, st.ldq = W.Q1.ldout, st.rowsum = W.rowsum, st.N = N, st.AF = AF, st.which = which;
  st.eta = eta, st.stats = stats, st.scale = W.scale;
  launch_dql_stats(st, s);
  // the seed: d a = scale * dQ_which/da + sa[t_bc] * (dh_0 of the BC slab . W0[:, :AF]), then through the final clamp
  DqlLink lk;
  memset(&lk, 0, sizeof(lk));
  lk.N = N, lk.AF = AF, lk.dx = W.dx, lk.scale = W.scale, lk.t_bc = t_bc, lk.sa = sa, lk.a = chains + (size_t)K * AF, lk.K = K;
  lk.final_clip = cfg.has_final_clip, lk.tsteps = tsteps, lk.mask = mask, lk.ldd = LA.Kpo;
  lk.dh = W.dhcat, lk.ldh = 2 * Hq, lk.wa = W.w0q, lk.H = Hq, lk.rows = qsm_tail_rows(Hq), lk.mode = 0;
  launch_dql_link<P>(lk, s);
  auto slab = [&](const void* p, int ld, size_t es, int i) { return (void*)((char*)p + (size_t)i * N * ld * es); };
  lk.wa = W.w0x, lk.H = H, lk.ldh = H, lk.rows = qsm_tail_rows(H);
  lk.dh = slab(W.A.dh_all[0], H, ES, K), lk.mode = 1, lk.p = K, lk.d_a = d_a, lk.d_out_prev = slab(W.A.d_out, LA.Kpo, ES, K - 1);
  launch_dql_link<P>(lk, s);
  lk.mode = 2, lk.d_a = nullptr;
  for (int p = K - 1; p >= 0; --p) {  // the only sequential part: one slab's data gradients, then the link to the slab before
    dql_actor_chain<P>(a, wk, LA, N, (int64_t)p * N, W.A, s);
    lk.dh = slab(W.A.dh_all[0], H, ES, p), lk.p = p, lk.d_out_prev = p > 0 ? slab(W.A.d_out, LA.Kpo, ES, p - 1) : nullptr;
    launch_dql_link<P>(lk, s);
  }
  dql_weight_grads<P>(a, ap, ak, LA, M, W.A, grad, W.krow, tsteps, K, s);
  return check_launch();
}
int dppo_dql_actor_fwd_bwd(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, const float* actor_params,
                           const void* actor_packed, const float* q_params, const void* q1_packed, const void* q2_packed,
                           const dppo_diffusion_cfg* cfg, const dppo_step* tsteps, int K, const dppo_idql_batch* batch, int obs_dim,
                           int64_t N, const float* chains, const float* noise_bc, const int64_t* t_bc,
                           const float* sqrt_alphas_cumprod, const float* sqrt_one_minus_alphas_cumprod, double eta, int which,
                           float* actor_grad, double* stats, uint8_t* masks, float* d_a, void* workspace, int64_t workspace_bytes,
                           dppo_stream_t stream) {
  if (int e = check_dql(actor, q, obs_dim)) return e;
  if (int e = check_prec(prec)) return e;
  if (!actor_params || !actor_packed || !q_params || !q1_packed || !q2_packed || !cfg || !tsteps || !chains || !noise_bc || !t_bc ||
      !sqrt_alphas_cumprod || !sqrt_one_minus_alphas_cumprod || !actor_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_dql_sizes(actor, N, K)) return e;
  if (int e = check_idql_batch(batch, N, RING_OBS)) return e;
  if (which != 0 && which != 1) return fail(-1, "which=%d must be 0 (-mean q1 / mean|q2|) or 1 (-mean q2 / mean|q1|)", which);
  if (!(eta >= -3.0e38 && eta <= 3.0e38)) return fail(-1, "eta=%g must be finite", eta);
  if (cfg->use_ddim) return fail(-1, "DQL does not support DDIM");
#define CALL(P)                                                                                                                  \
  dql_impl<P>(*actor, *q, actor_params, (const char*)actor_packed, q_params, (const char*)q1_packed, (const char*)q2_packed, *cfg, \
              tsteps, K, *batch, obs_dim, N, chains, noise_bc, t_bc, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, eta,     \
              which, actor_grad, stats, masks, d_a, workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

// ---- SAC (sac.hip): tanh-Gaussian actor with a state-dependent std, entropy-regularised twin-Q, temperature --------------------
static int check_sac_actor(const dppo_net_desc* a) {
  if (int e = check_net(a)) return e;
  if (a->kind != 1 || !a->plain)
    return fail(-1, "the SAC actor is a kind-1 plain trunk (Gaussian_MLP with fixed_std=None, residual_style=False); a residual actor is not built");
  if (a->out_dim % 2) return fail(-1, "the SAC actor's out_dim=%d must be 2 * Ta*Da ([mean | raw logvar])", a->out_dim);
  return 0;
}
static int check_sac_cfg(const dppo_net_desc* a, const dppo_sac_cfg* cfg) {
  if (!cfg) return fail(-1, "null cfg");
  if (cfg->horizon_steps < 1 || cfg->action_dim < 1 || 2 * cfg->horizon_steps * cfg->action_dim != a->out_dim)
    return fail(-1, "2 * Ta*Da != actor out_dim");
  if (!(cfg->logvar_min <= cfg->logvar_max)) return fail(-1, "logvar_min must not exceed logvar_max");
  if (!(cfg->randn_clip >= 0.f)) return fail(-1, "randn_clip must be >= 0");
  if ((cfg->deterministic != 0 && cfg->deterministic != 1) || (cfg->squash != 0 && cfg->squash != 1))
    return fail(-1, "deterministic and squash must be 0 or 1");
  return 0;
}
static SacHead sac_head_of(const dppo_sac_cfg& cfg, const float* out, int ldo, int AF, const float* noise, int64_t N) {
  SacHead h;
  memset(&h, 0, sizeof(h));
  h.cfg = cfg, h.half_span = 0.5f * (cfg.logvar_max - cfg.logvar_min), h.out = out, h.ldo = ldo, h.AF = AF, h.noise = noise;
  h.ring.N = N, h.ring.AD = AF;
  return h;
}
template <class P>
static size_t carve_sac_sample(Carver& c, const dppo_net_desc& a, int64_t B, MlpBufs<P>& A) {
  carve_mlp<P>(c, a, B, false, false, A);
  return al256(c.off);
}
int64_t dppo_sac_sample_workspace_bytes(const dppo_net_desc* actor, int prec, int64_t B) {
  if (check_sac_actor(actor) || check_prec(prec)) return -1;
  if (B < 1 || B > 0x7fffffff) return fail(-1, "B out of range");
  return ws_bytes(prec, [&](Carver& c, auto p) {
    MlpBufs<decltype(p)> A;
    return carve_sac_sample<decltype(p)>(c, *actor, B, A);
  });
}
template <class P>
static int sac_sample_impl(const dppo_net_desc& d, const float* prm, const char* pk, const dppo_sac_cfg& cfg, const float* obs,
                           const float* noise, int64_t B, float* actions, float* logp, float* u_out, void* ws, int64_t wsb,
                           hipStream_t s) {
  MlpBufs<P> A;
  if (int e = carve_ws(ws, wsb, [&](Carver& c) { return carve_sac_sample<P>(c, d, B, A); })) return e;
  const PackLayout L = pack_layout<P>(d, 0);
  launch_build_direct<P>(nullptr, nullptr, obs, nullptr, 0, 0, d.cond_dim, B, A.in, L.Kp0, s);
  mlp_forward<P>(d, prm, pk, L, B, A, false, s);
  SacHead h = sac_head_of(cfg, A.out, A.ldout, d.out_dim / 2, noise, B);
  h.actions = actions, h.logp = logp, h.u_out = u_out;
  launch_sac_head<P>(h, s);
  return check_launch();
}
int dppo_sac_sample(const dppo_net_desc* actor, int prec, const float* params, const void* packed, const dppo_sac_cfg* cfg,
                    const float* obs, const float* noise, int64_t B, float* actions, float* logp, float* u_out, void* workspace,
                    int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_sac_actor(actor)) return e;
  if (int e = check_prec(prec)) return e;
  if (int e = check_sac_cfg(actor, cfg)) return e;
  if (!params || !packed || !obs || !actions || !workspace) return fail(-1, "null pointer");
  if (B < 1 || B > 0x7fffffff) return fail(-1, "B out of range");
#define CALL(P)                                                                                                             \
  sac_sample_impl<P>(*actor, params, (const char*)packed, *cfg, obs, noise, B, actions, logp, u_out, workspace, workspace_bytes, \
                     (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

int64_t dppo_sac_q_loss_workspace_bytes(const dppo_net_desc* q, int prec, int obs_dim, int64_t N) {
  return dppo_qsm_q_loss_workspace_bytes(q, prec, obs_dim, N);  // the same four trunks, partials and gathered rows
}
int dppo_sac_q_loss_fwd_bwd(const dppo_net_desc* q, int prec, const float* q_params, const void* q1_packed, const void* q2_packed,
                            const float* target_q_params, const void* target_q1_packed, const void* target_q2_packed,
                            const dppo_idql_batch* batch, int obs_dim, const float* next_actions, const float* next_logp,
                            const double* alpha, int64_t N, double gamma, float* q_grad, double* stats, void* workspace,
                            int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_qsm_q(q, obs_dim)) return e;
  if (int e = check_prec(prec)) return e;
  if (!q_params || !q1_packed || !q2_packed || !target_q_params || !target_q1_packed || !target_q2_packed || !next_actions ||
      !next_logp || !alpha || !q_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_rows(N)) return e;
  if (int e = check_idql_batch(batch, N, RING_TRANSITION)) return e;
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(-1, "discount gamma=%g outside [0, 1]", gamma);
#define CALL(P)                                                                                                                \
  twin_td_impl<P>(*q, q_params, (const char*)q1_packed, (const char*)q2_packed, target_q_params, (const char*)target_q1_packed, \
                  (const char*)target_q2_packed, *batch, obs_dim, next_actions, next_logp, alpha, N, gamma, q_grad, stats,      \
                  workspace, workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

static int check_sac_pair(const dppo_net_desc* a, const dppo_net_desc* q, int obs_dim) {
  if (int e = check_sac_actor(a)) return e;
  if (int e = check_qsm_q(q, obs_dim)) return e;
  if (int e = check_qsm_plain(q)) return e;
  return check_sac_actor_q(a, q, obs_dim);
}
int64_t dppo_sac_actor_workspace_bytes(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, int obs_dim, int64_t N) {
  if (check_sac_pair(actor, q, obs_dim) || check_prec(prec)) return -1;
  if (int e = check_rows(N)) return e;
  return twin_actor_ws_bytes(actor, q, prec, N);  // twin_actor_impl, beside Cal-QL's
}
int dppo_sac_actor_fwd_bwd(const dppo_net_desc* actor, const dppo_net_desc* q, int prec, const float* actor_params,
                           const void* actor_packed, const float* q_params, const void* q1_packed, const void* q2_packed,
                           const dppo_sac_cfg* cfg, const dppo_idql_batch* batch, int obs_dim, int64_t N, const float* noise,
                           const double* alpha, float* actor_grad, double* stats, float* d_a, float* logp_out, uint8_t* sel_out,
                           float* actions_out, void* workspace, int64_t workspace_bytes, dppo_stream_t stream) {
  if (int e = check_sac_pair(actor, q, obs_dim)) return e;
  if (int e = check_prec(prec)) return e;
  if (int e = check_sac_cfg(actor, cfg)) return e;
  if (cfg->deterministic) return fail(-1, "the actor loss samples: deterministic must be 0");
  if (!actor_params || !actor_packed || !q_params || !q1_packed || !q2_packed || !alpha || !actor_grad || !stats || !workspace)
    return fail(-1, "null pointer");
  if (int e = check_rows(N)) return e;
  if (int e = check_idql_batch(batch, N, RING_OBS)) return e;
#define CALL(P)                                                                                                                   \
  twin_actor_impl<P>(*actor, *q, actor_params, (const char*)actor_packed, q_params, (const char*)q1_packed, (const char*)q2_packed, \
                     *cfg, *batch, obs_dim, N, noise, alpha, actor_grad, stats, d_a, logp_out, sel_out, actions_out, workspace,      \
                    workspace_bytes, (hipStream_t)stream)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}
int dppo_sac_alpha_loss(const float* logp, int64_t N, const double* log_alpha, double target_entropy, double* out,
                        dppo_stream_t stream) {
  if (!logp || !log_alpha || !out) return fail(-1, "null pointer");
  if (int e = check_rows(N)) return e;
  if (!(target_entropy >= -3.0e38 && target_entropy <= 3.0e38)) return fail(-1, "target_entropy=%g must be finite", target_entropy);
  launch_sac_alpha_loss(logp, N, log_alpha, target_entropy, out, (hipStream_t)stream);
  return check_launch();
}

// ---- optimiser ----------------------------------------------------------------------------------------
int dppo_grad_sq_norm(const float* grad, int64_t n, double* scratch, double* out, dppo_stream_t stream) {
  if (!grad || !scratch || !out || n < 1) return fail(-1, "bad argument");
  launch_sq_norm(grad, n, scratch, out, (hipStream_t)stream);
  return check_launch();
}

int dppo_adamw_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step, double lr,
                    double beta1, double beta2, double eps, double weight_decay, const double* sq_norm, double max_norm,
                    dppo_stream_t stream) {
  if (!params || !grad || !exp_avg || !exp_avg_sq || n < 1 || step < 1) return fail(-1, "bad argument");
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  launch_adamw(params, grad, exp_avg, exp_avg_sq, n, (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2,
               (float)(1.0 - beta2), (float)(lr / bc1), (float)sqrt(bc2), (float)eps, sq_norm, (float)max_norm,
               (hipStream_t)stream);
  return check_launch();
}


int dppo_adamw_step_dev(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t* step_dev,
                        const float* lr_dev, double beta1, double beta2, double eps, double weight_decay,
                        const double* sq_norm, double max_norm, dppo_stream_t stream) {
  if (!params || !grad || !exp_avg || !exp_avg_sq || !step_dev || !lr_dev || n < 1) return fail(-1, "bad argument");
  launch_adamw_dev(params, grad, exp_avg, exp_avg_sq, n, step_dev, lr_dev, beta1, beta2, (float)eps, weight_decay, sq_norm,
                   (float)max_norm, (hipStream_t)stream);
  return check_launch();
}

int dppo_adamw_step_multi(const dppo_adamw_slot* slots, int n_slots, dppo_stream_t stream) {
  if (!slots || n_slots < 1 || n_slots > 4) return fail(-1, "1..4 slots");
  AdamwSlots a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n_slots; ++i) {
    const dppo_adamw_slot& q = slots[i];
    if (!q.params || !q.grad || !q.exp_avg || !q.exp_avg_sq || !q.step_dev || !q.lr_dev || q.n < 1)
      return fail(-1, "bad argument in slot %d", i);
    AdamwSlot& t = a.s[i];
    t.p = q.params, t.g = q.grad, t.m = q.exp_avg, t.v = q.exp_avg_sq, t.n = q.n, t.step_dev = q.step_dev;
    t.lr_dev = q.lr_dev, t.beta1 = q.beta1, t.beta2 = q.beta2, t.weight_decay = q.weight_decay, t.eps = (float)q.eps;
    t.max_norm = (float)q.max_norm, t.sq_norm = q.sq_norm;
  }
  a.n = n_slots;
  launch_adamw_multi(a, (hipStream_t)stream);
  return check_launch();
}

int dppo_stats_split(const double* stats, float* hi_lo, dppo_stream_t stream) {
  if (!stats || !hi_lo) return fail(-1, "null pointer");
  launch_stats_split(stats, hi_lo, DPPO_STAT_COUNT, (hipStream_t)stream);
  return check_launch();
}
int dppo_stats_merge(const float* hi_lo, double* stats, int world, dppo_stream_t stream) {
  return dppo_stats_merge_n(hi_lo, stats, world, 2, stream);
}
int dppo_stats_merge_n(const float* hi_lo, double* stats, int world, int n_avg, dppo_stream_t stream) {
  if (!stats || !hi_lo || world < 1 || n_avg < 0 || DPPO_STAT_ADV_MEAN + n_avg > DPPO_STAT_COUNT) return fail(-1, "bad argument");
  launch_stats_merge(hi_lo, stats, DPPO_STAT_COUNT, DPPO_STAT_ADV_MEAN, n_avg, 1.0 / world, (hipStream_t)stream);
  return check_launch();
}

// ---- measurement hook ----------------------------------------------------------------------------------
int dppo_probe_arm(int kernel_id, int max_launches) {
  if (probe_arm(kernel_id, max_launches)) return fail(-1, "probe already armed or bad size");
  return 0;
}
int dppo_probe_collect(double* total_ms_host, int* launches_host, double* flops_host) {
  if (!total_ms_host || !launches_host || !flops_host) return fail(-1, "null pointer");
  if (probe_collect(total_ms_host, launches_host, flops_host)) return fail(-1, "probe not armed / event error");
  return 0;
}
int dppo_probe_collect_bytes(double* total_ms_host, int* launches_host, double* flops_host, double* bytes_host) {
  if (!total_ms_host || !launches_host || !flops_host || !bytes_host) return fail(-1, "null pointer");
  if (probe_collect(total_ms_host, launches_host, flops_host, bytes_host)) return fail(-1, "probe not armed / event error");
  return 0;
}

// ---- tuning / micro-benchmark hooks -------------------------------------------------------------------
// experiments that were measured, lost and removed with their code: setting one is an error, not a no-op
static int retired_knob(int knob) {
  return fail(-1, "tuning knob %d is retired: the code it selected was removed (DESIGN.md section 13)", knob);
}
int dppo_tune_set(int knob, int value) {
  switch (knob) {
    case 0: set_gemm_nt_variant(value); return 0;   // gemm_nt operand staging: LDS-DMA where legal (1, default) or through registers (0)
    case 1: g_use_fused = value; return 0;          // big-batch MLP path: fused row-tile kernels (1, default) or the layered gemm_nt chain (0)
    case 2: g_overlap = value; return 0;            // side streams: all (1, default), none (0), else a bit mask over them shifted by one
    case 3:                                         // weight-gradient GEMMs: workgroups aimed for (default 256)
      if (value < 1) break;
      g_tn_target = value;
      return 0;
    case 4:                                         // ... and the cap on their row splits (default 128)
      if (value < 1) break;
      g_tn_max_splits = value;
      return 0;
    case 5: set_gemm_tn_variant(value); return 0;   // ungrouped gemm_tn: register-staged (0, default), an LDS-DMA ring (1..8), by shape (-1)
    case 6: set_gemm_tn_thin(value); return 0;      // ungrouped gemm_tn: the 512 x 64 tile for thin outputs (1, default) or not (0)
    case 7: set_fused_short_tiles(value); return 0; // fused kernels: bit mask of short-tile variants (default 0: none)
    case 8: g_dbg = value; return 0;                // timing experiments, results are wrong while set (default 0)
    case 9: case 10: return retired_knob(knob);
    case 11: g_temb_onehot = value; return 0;       // time-embedding gradient through one-hot step columns of the input rows (1, default) or a pass of its own (0)
    case 12: g_tn_group = value; return 0;          // weight-gradient GEMMs of a backward pass in one grouped launch (1, default) or one launch each (0)
    case 13: g_pack_one = value; return 0;          // dppo_pack_net: one launch per network (1, default) or per image (0)
    case 14: g_early_join = value; return 0;        // side streams joined right behind the weight-gradient launch (1, default) or at the call's end (0)
    case 15: set_sampler_l0_lds(value); return 0;   // sampler: layer-0 weight fragments resident in LDS when they fit (1, default) or not (0)
    case 16: g_lowrank_top = value; return 0;       // top block's dW2 from the rank-out_dim factorisation (1, default) or an H x H GEMM (0)
    case 17: g_merge_top = value; return 0;         // sampler: top block's second layer merged into the out layer (1, default) or run (0)
    case 18: g_post_one = value; return 0;          // what follows the slab reduction of a backward pass in one launch (1, default) or several (0)
    case 20: dppo::set_vis_mfma_attn(value); return 0;  // visual encoder: attention on the matrix cores (1, default) or the scalar kernels (0)
    case 21: set_gemm_nt_small(value); return 0;    // gemm_nt: small tiles for small problems (1, default) or the 128 x 128 / 64 x 128 / 16 x 256 shapes only (0)
    case 22: set_fused_merge_fwd(value); return 0;  // fused forward of one-block networks: second layer merged into the out layer (1, default), not (0),
                                                    // heads of up to 16 outputs only (3); takes effect at the next pack (both forms are always packed)
    case 23: set_fused_bwd_one(value); return 0;    // fused backward of one-block networks: the specialised kernel (1, default) or the general one (0)
    case 25: set_fused_compact(value); return 0;    // one-block kernels: short layers walked without their padding k-steps (1, default) or padded (0)
    case 26: set_gemm_tn_nbuf(value); return 0;     // grouped weight-gradient GEMM, LDS stages: by the group's size (0, default), 1 or 2
    case 27: set_sampler_split(value); return 0;    // sampler: one 16-row tile over eight workgroups for small env batches (1, default) or one (0)
    case 28: set_sampler_split_pre_sweep(value); return 0;  // split sampler: 64-cycle sleep periods between a member's exchange store and its first sweep (default 4)
    case 29: set_sampler_split_spin_limit(value); return 0;  // split sampler: sweeps a member waits before giving up (default 2^20; <= 0 restores it)
    case 30:                                        // low-rank dW2 (knob 16) and the one-block backward: on for M >= value x out_dim (default 100)
      if (value < 1) break;
      g_lowrank_ratio = value;
      return 0;
    case 31: case 32: case 33: case 34: case 35: return retired_knob(knob);
    case 36: g_mom_rider = value; return 0;         // advantage moments as riders of the row builder: up to 16,384 samples (0, default), always (1), never (2)
    case 37: g_dw0 = value; return 0;               // in-kernel first-layer weight gradient of the one-block backward (1, default) or dh_0 stored and a GEMM (0)
    case 38: g_side_tail = value; return 0;         // with knob 37: what the backward kernel alone feeds runs on a side stream under the GEMMs (1, default) or behind them (0)
    case 39: case 40: return retired_knob(knob);
    case 41: g_tail_post = value; return 0;         // with knob 38: the GEMMs' slab reductions and the post-reduce parts behind them in one launch (1, default) or two (0)
    case 42: g_fuse_loss = value; return 0;         // policy half of the PPO loss in the epilogue of the actor's fused forward where it qualifies (1, default) or always a launch (0)
    default: break;
  }
  return fail(-1, "unknown tuning knob %d", knob);
}

template <class P>
static int route_mask(const dppo_net_desc& d, int64_t M, int Kft, int flags, int* mask_out) {
  Carver c{nullptr, 0, 0};
  MlpBufs<P> B;
  carve_mlp<P>(c, d, M, true, true, B);
  if (int e = plan_route<P>(d, M, Kft, flags, B)) return e;
  const BwdRoute& R = B.route;
  const bool bit[12] = {R.fused,   R.one_block,    R.lowrank,   R.merged,   R.onehot_col >= 0, R.dw0,
                        R.dw0_nhot > 0, R.dw0_round, R.need_aux, R.side_tail, R.tail_post, R.post_one};
  *mask_out = 0;
  for (int i = 0; i < 12; ++i) *mask_out |= bit[i] ? 1 << i : 0;
  return 0;
}
int dppo_backward_route(const dppo_net_desc* net, int prec, int64_t M, int Kft, int flags, int* mask_out) {
  if (int e = check_net(net)) return e;
  if (int e = check_prec(prec)) return e;
  if (!mask_out || M < 1 || M > 0x7fffffff || Kft < 0 || Kft > 1024 || (flags & ~7)) return fail(-1, "bad argument");
#define CALL(P) route_mask<P>(*net, M, Kft, flags, mask_out)
  return DPPO_DISPATCH(prec, CALL);
#undef CALL
}

int dppo_ppo_loss_route(const dppo_net_desc* actor, const dppo_net_desc* critic, int prec, int64_t N, int has_global_moments) {
  if (int e = check_net(actor)) return e;
  if (int e = check_net(critic)) return e;
  if (int e = check_prec(prec)) return e;
  if (N < 2 || N > 0x7fffffff) return fail(-1, "N out of range");
  // (the value half runs on the critic's stream whenever side stream 0 is on: ppo_impl's two_streams)
  if (prec == DPPO_PREC_F32) return fuse_loss_ok<F32>(*actor, N, has_global_moments != 0, side_stream_on(0), 0) ? 1 : 0;
  return fuse_loss_ok<BF16>(*actor, N, has_global_moments != 0, side_stream_on(0), 0) ? 1 : 0;
}

int dppo_gemm_nt_raw(int prec, const void* X, const void* W, const float* bias, int64_t M, int N, int Kp, float* out_f32,
                     void* out_elem, int ldo, int act, dppo_stream_t stream) {
  if (int e = check_prec(prec)) return e;
  if (!X || !W || M < 1 || M > 0x7fffffff || N < 1) return fail(-1, "bad argument");
  const int es = prec == DPPO_PREC_F32 ? 4 : 2;
  if (Kp < 1 || (Kp * es) % 128) return fail(-1, "Kp must be a multiple of %d", 128 / es);
  if (ldo < ((N + 15) & ~15)) return fail(-1, "ldo too small");
  GemmNT g;
  memset(&g, 0, sizeof(g));
  g.X = X, g.W = W, g.bias = bias, g.M = (int)M, g.N = N, g.Kp = Kp, g.ldx = Kp, g.ldw = Kp;
  g.out_f32 = out_f32, g.ldo32 = ldo, g.out_act = out_elem, g.ldo = ldo, g.act = act;
  if (prec == DPPO_PREC_F32)
    launch_gemm_nt<F32>(g, (hipStream_t)stream);
  else
    launch_gemm_nt<BF16>(g, (hipStream_t)stream);
  return check_launch();
}

int dppo_gemm_tn_raw(int prec, const void* A, int lda, int N1, const void* B, int ldb, int N2, int64_t M,
                     int rows_per_split, float* slab, float* C, dppo_stream_t stream) {
  if (int e = check_prec(prec)) return e;
  if (!A || !B || !slab || !C || M < 1 || M > 0x7fffffff || N1 < 1 || N2 < 1) return fail(-1, "bad argument");
  if (rows_per_split < 64 || rows_per_split % 64) return fail(-1, "rows_per_split must be a multiple of 64");
  const int es = prec == DPPO_PREC_F32 ? 4 : 2;
  if (lda < N1 || ldb < N2) return fail(-1, "lda / ldb smaller than N1 / N2");
  if ((lda * es) % 16 || (ldb * es) % 16) return fail(-1, "lda and ldb must be multiples of %d", 16 / es);
  GemmTN t;
  memset(&t, 0, sizeof(t));
  t.A = A, t.B = B, t.M = (int)M, t.N1 = N1, t.N2 = N2, t.lda = lda, t.ldb = ldb, t.slab = slab, t.ldc = N2;
  t.rows_per_split = rows_per_split, t.splits = (int)((M + rows_per_split - 1) / rows_per_split);
  if (prec == DPPO_PREC_F32)
    launch_gemm_tn<F32>(t, (hipStream_t)stream);
  else
    launch_gemm_tn<BF16>(t, (hipStream_t)stream);
  launch_slab_reduce_2d(slab, t.splits, N1, N2, N2, C, N2, 1.f, (hipStream_t)stream);
  return check_launch();
}

int dppo_gemm_nt_desc_raw(int prec, const dppo_gemm_nt_desc* d, dppo_stream_t stream) {
  if (int e = check_prec(prec)) return e;
  if (!d || !d->X || !d->W) return fail(-1, "null pointer");
  if (!d->out_f32 && !d->out_pre && !d->out_act) return fail(-1, "null pointer: no output");
  if (d->M < 1 || d->M > 0x7fffffff || d->N < 1) return fail(-1, "bad argument: M / N");
  const int es = prec == DPPO_PREC_F32 ? 4 : 2;
  if (d->Kp < 1 || (d->Kp * es) % 128) return fail(-1, "Kp must be a multiple of %d", 128 / es);
  if (d->ldx < d->Kp || d->ldw < d->Kp) return fail(-1, "ldx / ldw smaller than Kp");
  if ((d->ldx * es) % 16 || (d->ldw * es) % 16) return fail(-1, "ldx and ldw must be multiples of %d", 16 / es);
  const int nst = (d->N + 15) & ~15;  // columns of every epilogue operand the kernel touches
  if (d->dsrc_kind < 0 || d->dsrc_kind > 2) return fail(-1, "dsrc_kind must be 0, 1 or 2");
  if (d->dsrc_kind != 0 && !d->dsrc) return fail(-1, "null pointer: dsrc");
  if (d->dsrc_kind != 0 && (d->dsrc_ld < nst || d->dsrc_ld % 4)) return fail(-1, "dsrc_ld too small or not a multiple of 4");
  if (d->res && (d->ldres < nst || d->ldres % 4)) return fail(-1, "ldres too small or not a multiple of 4");
  if (d->add && (d->ldadd < nst || d->ldadd % 4)) return fail(-1, "ldadd too small or not a multiple of 4");
  if (d->out_f32 && (d->ldo32 < nst || d->ldo32 % 4)) return fail(-1, "ldo32 too small or not a multiple of 4");
  if ((d->out_pre || d->out_act) && (d->ldo < nst || d->ldo % 4)) return fail(-1, "ldo too small or not a multiple of 4");
  if (d->act < 0 || d->act > ACT_NONE || d->dact < 0 || d->dact > ACT_NONE) return fail(-1, "act / dact must be 0, 1 or 2");
  GemmNT g;
  memset(&g, 0, sizeof(g));
  g.X = d->X, g.W = d->W, g.bias = d->bias, g.M = (int)d->M, g.N = d->N, g.Kp = d->Kp, g.ldx = d->ldx, g.ldw = d->ldw;
  g.dsrc = d->dsrc_kind ? d->dsrc : nullptr, g.dsrc_kind = d->dsrc_kind, g.dsrc_ld = d->dsrc_ld, g.dact = d->dact;
  g.res = d->res, g.ldres = d->ldres, g.add = d->add, g.ldadd = d->ldadd;
  g.out_f32 = d->out_f32, g.ldo32 = d->ldo32, g.out_pre = d->out_pre, g.out_act = d->out_act, g.ldo = d->ldo, g.act = d->act;
  if (prec == DPPO_PREC_F32)
    launch_gemm_nt<F32>(g, (hipStream_t)stream);
  else
    launch_gemm_nt<BF16>(g, (hipStream_t)stream);
  return check_launch();
}

// 0 and t filled, or -1 with the reason in dppo_last_error()
static int tn_job_checked(const dppo_gemm_tn_job& j, int es, GemmTN& t) {
  if (!j.A || !j.B || !j.slab) return fail(-1, "null pointer");
  if (j.M < 1 || j.M > 0x7fffffff || j.N1 < 1 || j.N2 < 1) return fail(-1, "bad argument: M / N1 / N2");
  if (j.rows_per_split < 64 || j.rows_per_split % 64) return fail(-1, "rows_per_split must be a multiple of 64");
  if (j.lda < 1 || j.ldb < 1 || (j.lda * es) % 16 || (j.ldb * es) % 16)
    return fail(-1, "lda and ldb must be multiples of %d", 16 / es);
  if (j.ncol_a < 0 || j.ncol_b < 0 || (j.ncol_a * es) % 16 || (j.ncol_b * es) % 16)
    return fail(-1, "ncol_a and ncol_b must be multiples of %d", 16 / es);
  if ((j.ncol_a > 0 ? j.ncol_a : j.lda) < j.N1 || (j.ncol_b > 0 ? j.ncol_b : j.ldb) < j.N2)
    return fail(-1, "lda / ldb (ncol_a / ncol_b) smaller than N1 / N2");
  memset(&t, 0, sizeof(t));
  t.A = j.A, t.B = j.B, t.M = (int)j.M, t.N1 = j.N1, t.N2 = j.N2, t.lda = j.lda, t.ldb = j.ldb, t.slab = j.slab, t.ldc = j.N2;
  t.rows_per_split = j.rows_per_split, t.splits = (int)((j.M + j.rows_per_split - 1) / j.rows_per_split);
  t.ncol_a = j.ncol_a, t.ncol_b = j.ncol_b;
  return 0;
}

int dppo_gemm_tn_group_raw(int prec, const dppo_gemm_tn_job* jobs, int n, float* const* C_out, dppo_stream_t stream) {
  if (int e = check_prec(prec)) return e;
  if (!jobs || !C_out) return fail(-1, "null pointer");
  if (n < 1 || n > MAX_TN_JOBS) return fail(-1, "n must be 1..%d", MAX_TN_JOBS);
  const int es = prec == DPPO_PREC_F32 ? 4 : 2;
  GemmTNGroup gr;
  memset(&gr, 0, sizeof(gr));
  for (int i = 0; i < n; ++i) {
    if (!C_out[i]) return fail(-1, "null pointer: C_out[%d]", i);
    if (int e = tn_job_checked(jobs[i], es, gr.j[i])) return e;
  }
  gr.n = n;
  gemm_tn_group_order(gr);
  if (prec == DPPO_PREC_F32)
    launch_gemm_tn_group<F32>(gr, (hipStream_t)stream);
  else
    launch_gemm_tn_group<BF16>(gr, (hipStream_t)stream);
  for (int i = 0; i < n; ++i) {  // the caller's order: a job's slab does not move with the sort
    const dppo_gemm_tn_job& j = jobs[i];
    const int splits = (int)((j.M + j.rows_per_split - 1) / j.rows_per_split);
    launch_slab_reduce_2d(j.slab, splits, j.N1, j.N2, j.N2, C_out[i], j.N2, 1.f, (hipStream_t)stream);
  }
  return check_launch();
}

int dppo_gemm_tn_job_raw(int prec, const dppo_gemm_tn_job* job, float* C, dppo_stream_t stream) {
  if (int e = check_prec(prec)) return e;
  if (!job || !C) return fail(-1, "null pointer");
  GemmTN t;
  if (int e = tn_job_checked(*job, prec == DPPO_PREC_F32 ? 4 : 2, t)) return e;
  if (prec == DPPO_PREC_F32)
    launch_gemm_tn<F32>(t, (hipStream_t)stream);
  else
    launch_gemm_tn<BF16>(t, (hipStream_t)stream);
  launch_slab_reduce_2d(t.slab, t.splits, t.N1, t.N2, t.N2, C, t.N2, 1.f, (hipStream_t)stream);
  return check_launch();
}
