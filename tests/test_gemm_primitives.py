"""GPU: the two MFMA GEMM families of csrc/gemm.hip called directly, every dispatch path, against exact references.

Exact data: operands are random integers in [-4, 4] (exact in bf16 and fp32), every partial sum is an integer below 2^24
(worst case 16 x 50,001), so fp32 accumulation is exact in ANY order and the result must EQUAL a float64 torch.matmul --
no tolerance.  Integer bias / res / add and ReLU / identity activations keep the gemm_nt epilogue exact; bf16 outputs
must equal the reference rounded to nearest-even.  One-hot probes name the element that was read in the wrong place.
Every output, slab and result is allocated with spare rows / columns / floats filled with a sentinel that must survive.

Where bit-identity is promised by the code (gemm.hip: smaller gemm_nt tiles, LDS-DMA staging, the grouped kernel against
the ungrouped one, NBUF 1 against 2) it is asserted on random normal data; where it is not (LDS-DMA rings of knob 5, the
512 x 64 tile) the result is held to the worst-case summation bound |got - ref| <= 2 L 2^-24 (|A|^T |B|) + one rounding
of the stored type, L the contraction length, computed from the float64 reference of the same inputs.

`nt_branch`, `tn_branch` and `group_nbuf` are pure-Python copies of the dispatch predicates of launch_gemm_nt,
launch_gemm_tn and launch_gemm_tn_group: every case states the instantiation it is meant to hit and asserts it, and
`test_every_instantiation_is_named` asserts that the case tables cover all of them (DESIGN.md section 4 has the table).
"""
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch

from dppo_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -0.375  # exact in bf16, never an integer result
PRECS = {"fp32": (hip.PREC_F32, torch.float32, 4), "bf16": (hip.PREC_BF16, torch.bfloat16, 2)}
ACT_RELU, ACT_MISH, ACT_NONE = 0, 1, 2
KNOB_DEFAULTS = {0: 1, 5: 0, 6: 1, 21: 1, 26: 0}
SPARE = 64  # rows of data behind the M rows of every gemm_tn operand (one LDS stage): a kernel that reads past M gets them


@pytest.fixture(autouse=True)
def _gemm_knobs():
    """Each test starts from the library's default GEMM knobs whatever DPPO_TUNE says (the suite is also run with the
    default-on optimisations off) and the environment's choice is put back afterwards."""
    lib = hip.load()
    for k, v in KNOB_DEFAULTS.items():
        assert lib.dppo_tune_set(k, v) == 0
    yield
    env = dict(kv.split("=") for kv in filter(None, os.environ.get("DPPO_TUNE", "").split(",")))
    for k, v in KNOB_DEFAULTS.items():
        lib.dppo_tune_set(k, int(env.get(str(k), v)))


def tune(knob, value):
    assert hip.load().dppo_tune_set(knob, value) == 0


def cdiv(a, b):
    return (a + b - 1) // b


def rup(a, b):
    return cdiv(a, b) * b


def ints(gen, shape, dt, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=DEV).to(dt)


def gen_for(*key):
    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def mm64(a, b):
    """float64 a @ b: on the CPU for small shapes, on the device for large ones (exact for integer data either way)."""
    if a.shape[0] * a.shape[1] * b.shape[1] <= 1 << 24:
        return (a.double().cpu() @ b.double().cpu()).to(DEV)
    return a.double() @ b.double()


def assert_exact(got, ref, what):
    """got == ref element for element (numpy's assert_array_equal does the reporting)."""
    assert got.shape == ref.shape, what
    g, r = got.float(), ref.float()
    if torch.equal(g, r):
        return
    bad = (g != r).nonzero()
    first = ", ".join(f"{tuple(i.tolist())}: got {g[tuple(i)].item()} ref {r[tuple(i)].item()}" for i in bad[:6])
    np.testing.assert_array_equal(g.cpu().numpy(), r.cpu().numpy(), err_msg=f"{what}: {bad.shape[0]} wrong, first {first}")


def assert_bits_equal(a, b, what):
    ia = a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32)
    assert torch.equal(ia, ib), f"{what}: {(ia != ib).sum().item()} elements differ in their bits"


class Guarded:
    """rows x width window of a (rows + 3) x ld buffer filled with the sentinel."""

    def __init__(self, rows, width, ld, dt):
        assert ld > width
        self.rows, self.width, self.ld = rows, width, ld
        self.buf = torch.full((rows + 3, ld), SENT, device=DEV, dtype=dt)

    def ptr(self):
        return self.buf.data_ptr()

    def view(self):
        return self.buf[:self.rows, :self.width]

    def check(self, what):
        assert bool((self.buf[self.rows:] == SENT).all()), f"{what}: wrote below row {self.rows}"
        assert bool((self.buf[:self.rows, self.width:] == SENT).all()), f"{what}: wrote right of column {self.width}"


# ------------------------------------------------------------------------------------------------------------ gemm_nt
NT_INSTANCES = {("16x256", 0), ("64x128", 0), ("64x64", 0), ("64x64", 1), ("64x32", 0), ("64x32", 1),
                ("128x128sq", 0), ("128x128sq", 1), ("128x128", 0), ("128x128", 1)}


def nt_branch(M, N, Kp, knob0, knob21):
    """launch_gemm_nt's choice: (tile, LDS-DMA staging)."""
    dma = int(knob0 == 1 and N % 128 == 0)
    wg128 = cdiv(M, 128) * cdiv(N, 128)
    if knob21 and N > 16 and wg128 < 192:
        dma64 = int(knob0 == 1 and N % 64 == 0)
        return ("64x64" if cdiv(M, 64) * cdiv(N, 64) >= 192 else "64x32"), dma64
    if N <= 16:
        return "16x256", 0
    if N <= 64:
        return "64x128", 0
    if N == Kp:
        return "128x128sq", dma
    return "128x128", dma


def kp_of(k, es):
    """k > 0: elements; k < 0: -k k-tiles of 128 bytes (32 fp32 / 64 bf16 elements)."""
    return k if k > 0 else -k * (128 // es)


# (M, N, K, tile with knob 21 = 1, tile with knob 21 = 0); K as in kp_of
NT_CASES = []
for _n in (1, 7, 12, 16):  # 16 x 256 tile (N <= 16 never takes a small tile); M around BM = 256 and the flagship batch
    for _m, _k in ((1, -1), (255, -2), (256, -3), (257, -9), (50000, -2)):
        NT_CASES.append((_m, _n, _k, "16x256", "16x256"))
for _n in (40, 64):  # 64 x 128 tile: 391 row tiles >= 192 workgroups
    NT_CASES.append((50000, _n, -3, "64x128", "64x128"))
# 64 x 64 tile: fewer than 192 workgroups of 128 x 128 and at least 192 of 64 x 64.  At M = 4,000 that holds for N = 256 only
# (N = 192 needs M > 4,032; N = 40, 64 need M > 12,224); the others run at 4,000 too, where the 64 x 32 tile takes them
NT_CASES += [(4000, 256, -2, "64x64", "128x128"), (4100, 192, -2, "64x64", "128x128"),
             (16000, 40, -1, "64x64", "64x128"), (16000, 64, -2, "64x64", "64x128"),
             (4000, 40, -2, "64x32", "64x128"), (4000, 64, -9, "64x32", "64x128"), (4000, 192, 192, "64x32", "128x128sq")]
for _n, _k in ((40, -1), (64, -3), (192, -2), (256, -9)):  # 64 x 32 tile
    NT_CASES.append((500, _n, _k, "64x32", "64x128" if _n <= 64 else "128x128"))
# 128 x 128 tile at the flagship batch: square hidden layers (their own instantiation) and the others
NT_CASES += [(50000, 256, 256, "128x128sq", "128x128sq"), (50000, 512, 512, "128x128sq", "128x128sq"),
             (50000, 512, 64, "128x128", "128x128"), (50000, 256, 512, "128x128", "128x128"),
             (50000, 200, 256, "128x128", "128x128"), (50000, 384, 1024, "128x128", "128x128")]
# M in {BM - 1, BM, BM + 1} for every tile shape (16 x 256 above) and K of one, two, three and many k-tiles
for _d, _k in ((-1, -1), (0, -2), (1, -3)):
    NT_CASES += [(128 + _d, 40, _k, "64x32", "64x128"),        # 64 x 128 (knob 21 = 0)
                 (64 + _d, 12288, _k, "64x64", "128x128"),     # 64 x 64: one or two row tiles x 192 feature tiles
                 (64 + _d, 12280, -1, "64x64", "128x128"),     # ... with a ragged last feature tile (register staging)
                 (32 + _d, 40, _k, "64x32", "64x128"),         # 64 x 32
                 (32 + _d, 64, -9, "64x32", "64x128"),
                 (128 + _d, 200, _k, "64x32", "128x128"),      # 128 x 128 (knob 21 = 0)
                 (128 + _d, 256, 256, "64x32", "128x128sq"),   # 128 x 128 square
                 (128 + _d, 128, 128, "64x32", "128x128sq")]
NT_CASES += [(300, 192, 192, "64x32", "128x128sq"), (300, 200, -9, "64x32", "128x128"), (300, 40, -9, "64x32", "64x128"),
             (300, 64, -1, "64x32", "64x128"), (70, 12288, -9, "64x64", "128x128"), (300, 384, -1, "64x32", "128x128")]
NT_CASES_FP32_ONLY = [(300, 96, 96, "64x32", "128x128sq")]  # three k-tiles on the square instantiation (fp32: 32 per tile)


def nt_cases(prec):
    return NT_CASES + (NT_CASES_FP32_ONLY if prec == "fp32" else [])


def run_nt(prec, M, N, Kp, X, ldx, W, ldw, bias=None, dsrc=None, dsrc_kind=0, dact=ACT_RELU, res=None, add=None,
           out_f32=None, out_pre=None, out_act=None, act=ACT_RELU):
    d = hip.GemmNTDesc(X=X.data_ptr(), W=W.data_ptr(), bias=None if bias is None else bias.data_ptr(), M=M, N=N, Kp=Kp,
                       ldx=ldx, ldw=ldw, dsrc=None if dsrc is None else dsrc.data_ptr(), dsrc_kind=dsrc_kind,
                       dsrc_ld=0 if dsrc is None else dsrc.shape[1], dact=dact,
                       res=None if res is None else res.data_ptr(), ldres=0 if res is None else res.shape[1],
                       add=None if add is None else add.data_ptr(), ldadd=0 if add is None else add.shape[1],
                       out_f32=None if out_f32 is None else out_f32.ptr(), ldo32=0 if out_f32 is None else out_f32.ld,
                       out_pre=None if out_pre is None else out_pre.ptr(), out_act=None if out_act is None else out_act.ptr(),
                       ldo=max([o.ld for o in (out_pre, out_act) if o is not None], default=0), act=act)
    hip.check(hip.load().dppo_gemm_nt_desc_raw(PRECS[prec][0], C.byref(d), hip.stream()), "gemm_nt_desc_raw")


def nt_operands(gen, M, N, Kp, dt, es, fill=ints):
    """X (M, ldx) and W (N, ldw) with leading dimensions larger than Kp (a multiple of 16 bytes), all of it data."""
    ldx, ldw = Kp + 16 // es, Kp + 32 // es
    return fill(gen, (M, ldx), dt), ldx, fill(gen, (N, ldw), dt), ldw


@pytest.mark.parametrize("prec,case", [(p, i) for p in ("fp32", "bf16") for i in range(len(nt_cases(p)))])
def test_gemm_nt_exact(prec, case):
    """Every tile / staging configuration of launch_gemm_nt: X . W^T + bias, fp32 and elem outputs, exact."""
    M, N, K, tile_on, tile_off = nt_cases(prec)[case]
    _, dt, es = PRECS[prec]
    Kp, nst = kp_of(K, es), rup(N, 16)
    gen = gen_for("nt", case, prec)
    X, ldx, W, ldw = nt_operands(gen, M, N, Kp, dt, es)
    bias = ints(gen, (N,), torch.float32, -64, 64)
    ref = mm64(X[:, :Kp], W[:, :Kp].t()) + bias.double()
    ref = torch.cat([ref, torch.zeros(M, nst - N, device=DEV, dtype=torch.float64)], 1)  # zero accumulators, no bias
    assert ref.abs().max().item() < 2 ** 24
    first = None
    for knob21 in (1, 0):
        for knob0 in (1, 0):
            tile, dma = nt_branch(M, N, Kp, knob0, knob21)
            assert tile == (tile_on if knob21 else tile_off), (tile, dma)
            assert (tile, dma) in NT_INSTANCES
            tune(0, knob0), tune(21, knob21)
            o32 = Guarded(M, nst, nst + 20, torch.float32)
            oact = Guarded(M, nst, nst + 16, dt)
            run_nt(prec, M, N, Kp, X, ldx, W, ldw, bias=bias, out_f32=o32, out_act=oact, act=ACT_RELU)
            torch.cuda.synchronize()
            what = f"gemm_nt {prec} M={M} N={N} Kp={Kp} {tile} dma={dma}"
            assert_exact(o32.view(), ref.float(), what + " out_f32")
            assert_exact(oact.view(), torch.relu(ref).to(dt), what + " out_act")
            o32.check(what), oact.check(what)
            if first is None:
                first = (o32.view().clone(), oact.view().clone())
            else:
                assert_bits_equal(o32.view(), first[0], what), assert_bits_equal(oact.view(), first[1], what)


def test_every_instantiation_is_named():
    """The case tables reach every launch_nt_cfg / launch_tn_cfg / launch_tn_dma_cfg instantiation and both grouped ones."""
    hit = set()
    for prec in PRECS:
        for M, N, K, _, _ in nt_cases(prec):
            for knob21 in (0, 1):
                for knob0 in (0, 1):
                    hit.add(nt_branch(M, N, kp_of(K, PRECS[prec][2]), knob0, knob21))
    assert hit == NT_INSTANCES
    tn = set()
    for N1, _, N2, _ in TN_SQUARE + TN_THIN:
        for knob6 in (0, 1):
            tn.add(tn_branch(N1, N2, 0, knob6, False))
    for N1, _, N2, _ in TN_DMA_SHAPES:
        for knob5 in TN_DMA_VARIANTS:
            tn.add(tn_branch(N1, N2, knob5, 1, False))
    tn.add(tn_branch(48, 64, 3, 1, True))
    assert tn == {"reg128", "thin"} | {f"dma{v}" for v in range(1, 9)}
    assert {group_nbuf(k, g, m) for k, g, m in ((1, 1, 1), (2, 1, 1), (0, 769, 32768), (0, 768, 50000), (0, 1244, 32767))} == {1, 2}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("coded", ["W", "X"])
def test_gemm_nt_one_hot_probe(prec, coded):
    """One operand one-hot, the other index-coded: the output IS the element the kernel read, so a failure names it.
    bf16 codes are (flat index) mod 257 (<= 256, exact); fp32 codes are row * Kp + col."""
    _, dt, es = PRECS[prec]
    for M, N, K in ((257, 12, -3), (300, 40, -3), (300, 200, -3), (129, 256, 256), (4000, 256, -2), (3000, 64, -3)):
        Kp = kp_of(K, es)
        ldx, ldw = Kp + 16 // es, Kp + 32 // es
        rows_c, rows_h = (N, M) if coded == "W" else (M, N)
        code = torch.arange(rows_c * Kp, device=DEV).reshape(rows_c, Kp)
        code = code if prec == "fp32" else code % 257
        hot_col = (torch.arange(rows_h, device=DEV) * 7 + 3) % Kp
        hot = torch.zeros(rows_h, Kp, device=DEV)
        hot[torch.arange(rows_h, device=DEV), hot_col] = 1
        cmat, hmat = torch.full((rows_c, max(ldx, ldw)), 5.0, device=DEV), torch.full((rows_h, max(ldx, ldw)), 5.0, device=DEV)
        cmat[:, :Kp], hmat[:, :Kp] = code.float(), hot
        Wm, Xm = (cmat, hmat) if coded == "W" else (hmat, cmat)
        X, W = Xm[:, :ldx].to(dt).contiguous(), Wm[:, :ldw].to(dt).contiguous()
        ref = code[:, hot_col].t() if coded == "W" else code[:, hot_col]  # (M, N): out[m][n] = the coded element read
        for knob21 in (1, 0):
            for knob0 in (1, 0):
                tune(0, knob0), tune(21, knob21)
                o32 = Guarded(M, rup(N, 16), rup(N, 16) + 4, torch.float32)
                run_nt(prec, M, N, Kp, X, ldx, W, ldw, out_f32=o32)
                torch.cuda.synchronize()
                got = o32.view()[:, :N]
                if not torch.equal(got, ref.float()):
                    i = tuple((got != ref.float()).nonzero()[0].tolist())
                    g = int(got[i].item())
                    where = f"row {g // Kp} col {g % Kp}" if prec == "fp32" else f"code {g}"
                    raise AssertionError(f"gemm_nt {prec} M={M} N={N} Kp={Kp} {nt_branch(M, N, Kp, knob0, knob21)}: out{i} read "
                                         f"{coded} {where}, expected row {i[1] if coded == 'W' else i[0]} col "
                                         f"{int(hot_col[i[0] if coded == 'W' else i[1]])}")
                o32.check("one-hot")


def mish64(x):
    return x * torch.tanh(torch.nn.functional.softplus(x))


def mish_grad64(x):
    x = x.clone().requires_grad_(True)
    mish64(x).sum().backward()
    return x.grad


EPI_SHAPES = [(257, 12, -3), (300, 40, -2), (300, 64, -1), (300, 200, -3), (129, 256, 256), (200, 384, -2), (70, 12288, -1)]
EPI_PARTS = [("dsrc1",), ("dsrc2",), ("res",), ("add",), ("f32",), ("pre",), ("act",),
             ("dsrc1", "res", "add", "f32", "pre", "act"), ("dsrc2", "res", "add", "f32", "pre", "act")]


def epilogue_case(prec, M, N, K, parts, exact, seed, ident=False):
    """One gemm_nt launch per knob 0 x knob 21 with the epilogue operands named in `parts`; every leading dimension is
    larger than its width.  exact: integer data, ReLU (ident: identity) derivative and activation; else random normal data
    and Mish."""
    _, dt, es = PRECS[prec]
    Kp, nst = kp_of(K, es), rup(N, 16)
    gen = gen_for("epi", M, N, K, parts, prec, seed)
    if exact:
        fill, a = ints, (ACT_NONE if ident else ACT_RELU)
    else:
        def fill(g, shape, d, *_):
            return torch.randn(shape, generator=g, device=DEV).to(d)
        a = ACT_MISH
    X, ldx, W, ldw = nt_operands(gen, M, N, Kp, dt, es, fill)
    if not exact:
        W = (W.float() / Kp ** 0.5).to(dt)
    bias = fill(gen, (N,), torch.float32)
    kind = 1 if "dsrc1" in parts else (2 if "dsrc2" in parts else 0)
    dsrc = fill(gen, (M + 1, nst + 4), torch.float32 if kind == 1 else dt) if kind else None
    res = fill(gen, (M + 1, nst + 8), torch.float32) if "res" in parts else None
    add = fill(gen, (M + 1, nst + 12), dt) if "add" in parts else None
    v = mm64(X[:, :Kp], W[:, :Kp].t()) + bias.double()
    v = torch.cat([v, torch.zeros(M, nst - N, device=DEV, dtype=torch.float64)], 1)
    if kind:
        z = dsrc[:M, :nst].double()
        v = v * ((torch.ones_like(z) if ident else (z > 0).double()) if exact else mish_grad64(z))
    if res is not None:
        v = v + res[:M, :nst].double()
    if add is not None:
        v = v + add[:M, :nst].double()
    va = (v if ident else torch.relu(v)) if exact else mish64(v)
    outs = [p for p in parts if p in ("f32", "pre", "act")] or ["f32"]
    first = None
    for knob21 in (1, 0):
        for knob0 in (1, 0):
            tune(0, knob0), tune(21, knob21)
            o32 = Guarded(M, nst, nst + 20, torch.float32) if "f32" in outs else None
            opre = Guarded(M, nst, nst + 16, dt) if "pre" in outs else None
            oact = Guarded(M, nst, nst + 16, dt) if "act" in outs else None
            run_nt(prec, M, N, Kp, X, ldx, W, ldw, bias=bias, dsrc=dsrc, dsrc_kind=kind, dact=a, res=res, add=add,
                   out_f32=o32, out_pre=opre, out_act=oact, act=a)
            torch.cuda.synchronize()
            what = f"gemm_nt epilogue {prec} M={M} N={N} Kp={Kp} {parts} {nt_branch(M, N, Kp, knob0, knob21)}"
            got = []
            for o, r, name in ((o32, v, "out_f32"), (opre, v, "out_pre"), (oact, va, "out_act")):
                if o is None:
                    continue
                o.check(what + " " + name)
                if exact:
                    assert_exact(o.view(), r.float().to(o.buf.dtype), what + " " + name)
                else:  # the project's forward tolerances (tests/test_hip_parity.py), relative to the largest magnitude
                    tol = 2e-5 if prec == "fp32" else 3e-2
                    err = (o.view()[:, :N].double() - r[:, :N]).abs().max().item()
                    print(f"{what} {name}: max err {err:.3e} of max |ref| {r[:, :N].abs().max().item():.3e}")
                    assert err <= tol * r[:, :N].abs().max().item(), what + " " + name
                got.append(o.view().clone())
            if first is None:
                first = got
            else:  # smaller tiles and the other staging do not change the accumulation order
                for g, f in zip(got, first):
                    assert_bits_equal(g, f, what)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("parts", EPI_PARTS, ids=["+".join(p) for p in EPI_PARTS])
def test_gemm_nt_epilogue_exact(parts, prec):
    for M, N, K in EPI_SHAPES:
        epilogue_case(prec, M, N, K, parts, True, 0)
        if len(parts) > 1:  # the same with identity for both activations
            epilogue_case(prec, M, N, K, parts, True, 2, ident=True)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["dsrc1", "dsrc2"])
def test_gemm_nt_epilogue_mish(kind, prec):
    for M, N, K in EPI_SHAPES[:6]:
        epilogue_case(prec, M, N, K, (kind, "res", "add", "f32", "pre", "act"), False, 1)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_gemm_nt_bit_identical_across_staging_and_tile_size(prec):
    """gemm.hip's claim: the small tiles and LDS-DMA staging keep each output's accumulation order -- random normal data."""
    _, dt, es = PRECS[prec]
    for M, N, K in ((4000, 256, -9), (500, 192, 192), (16000, 64, -3), (300, 384, -3), (129, 512, 512), (50000, 512, 512)):
        Kp = kp_of(K, es)
        gen = gen_for("ntbits", M, N, K, prec)
        X = torch.randn((M, Kp), generator=gen, device=DEV).to(dt)
        W = (torch.randn((N, Kp), generator=gen, device=DEV) / Kp ** 0.5).to(dt)
        first, seen = None, set()
        for knob21 in (1, 0):
            for knob0 in (1, 0):
                tune(0, knob0), tune(21, knob21)
                seen.add(nt_branch(M, N, Kp, knob0, knob21))
                o32 = Guarded(M, N, N + 4, torch.float32)
                run_nt(prec, M, N, Kp, X, Kp, W, Kp, out_f32=o32)
                torch.cuda.synchronize()
                if first is None:
                    first = o32.view().clone()
                    ref = mm64(X, W.t())
                    assert bool(((first.double() - ref).abs() <= summation_bound(X.t(), W.t(), ref, Kp)).all())
                else:
                    assert_bits_equal(o32.view(), first, f"gemm_nt {prec} M={M} N={N} Kp={Kp} {sorted(seen)}")
        assert len(seen) >= 2


# ------------------------------------------------------------------------------------------------------------ gemm_tn
def tn_branch(N1, N2, knob5, knob6, overlapping):
    """launch_gemm_tn's choice."""
    if overlapping:
        return "reg128"
    if knob6 and N2 <= 64 and N1 > 64:
        return "thin"
    v = knob5 if knob5 >= 0 else (2 if N1 * N2 >= 512 * 512 else 0)
    return f"dma{v}" if 1 <= v <= 8 else "reg128"


def group_nbuf(knob26, grid, m_first):
    """launch_gemm_tn_group's choice of LDS stages."""
    return knob26 if knob26 else (2 if grid > 768 and m_first >= 32768 else 1)


# (N1, lda, N2, ldb)
TN_SQUARE = [(512, 512, 512, 512), (256, 256, 256, 264), (128, 136, 128, 128), (200, 200, 136, 136), (129, 136, 16, 16),
             (16, 16, 16, 24)]  # (129, 16) is thin with knob 6 = 1
TN_THIN = [(512, 512, 12, 16), (512, 520, 64, 64), (256, 256, 39, 48), (65, 72, 64, 72)]
TN_DMA_SHAPES = [(512, 512, 512, 512), (256, 256, 256, 256), (128, 128, 128, 128), (200, 200, 136, 136), (200, 208, 136, 144)]
TN_DMA_VARIANTS = (1, 2, 3, 4, 5, 6, 7, 8, -1)
# (M, rows_per_split): stage boundaries of both element types (32 / 64 rows), rps - 1 / rps / rps + 1, 1 / 8 / 128 splits,
# a last split of one row
TN_ROWS = [(1, 64), (31, 64), (32, 64), (33, 64), (63, 64), (64, 64), (65, 64), (127, 128), (128, 128), (129, 128),
           (449, 64), (50000, 50048), (50000, 6272), (50000, 448), (48769, 384)]
assert [cdiv(m, r) for m, r in TN_ROWS[-5:]] == [8, 1, 8, 112, 128] and 448 + 1 == 449 and 127 * 384 + 1 == 48769


class TnOut:
    """Slab and result of one product, each followed by spare floats holding the sentinel."""

    def __init__(self, N1, N2, M, rps):
        self.N1, self.N2, self.splits = N1, N2, cdiv(M, rps)
        self.slab = torch.full((self.splits * N1 * N2 + 4096,), SENT, device=DEV)
        self.C = torch.full((N1 * N2 + 1024,), SENT, device=DEV)

    def result(self):
        return self.C[:self.N1 * self.N2].view(self.N1, self.N2)

    def check(self, what):
        assert bool((self.slab[self.splits * self.N1 * self.N2:] == SENT).all()), what + ": wrote past the slab"
        assert bool((self.C[self.N1 * self.N2:] == SENT).all()), what + ": wrote past the result"
        assert not bool((self.slab[:self.splits * self.N1 * self.N2] == SENT).any()), what + ": slab element not written"


def tn_job(A, lda, N1, B, ldb, N2, M, rps, out, ncol_a=0, ncol_b=0):
    return hip.GemmTNJob(A=A.data_ptr(), B=B.data_ptr(), slab=out.slab.data_ptr(), M=M, lda=lda, N1=N1, ldb=ldb, N2=N2,
                         rows_per_split=rps, ncol_a=ncol_a, ncol_b=ncol_b, pad=0)


def run_tn(prec, A, lda, N1, B, ldb, N2, M, rps, how, ncol_a=0, ncol_b=0):
    """how: 'raw' (dppo_gemm_tn_raw), 'job' (dppo_gemm_tn_job_raw: the same dispatch, takes ncol) or 'group' (one job)."""
    lib, out = hip.load(), TnOut(N1, N2, M, rps)
    if how == "raw":
        assert ncol_a == 0 and ncol_b == 0
        hip.check(lib.dppo_gemm_tn_raw(PRECS[prec][0], A.data_ptr(), lda, N1, B.data_ptr(), ldb, N2, M, rps, out.slab.data_ptr(),
                                       out.C.data_ptr(), hip.stream()), "gemm_tn_raw")
    elif how == "job":
        j = tn_job(A, lda, N1, B, ldb, N2, M, rps, out, ncol_a, ncol_b)
        hip.check(lib.dppo_gemm_tn_job_raw(PRECS[prec][0], C.byref(j), out.C.data_ptr(), hip.stream()), "gemm_tn_job_raw")
    else:
        run_group(prec, [(A, lda, N1, B, ldb, N2, M, rps, ncol_a, ncol_b)], [out])
    torch.cuda.synchronize()
    return out


def run_group(prec, jobs, outs=None):
    """jobs: (A, lda, N1, B, ldb, N2, M, rps[, ncol_a, ncol_b]) in the caller's order."""
    n = len(jobs)
    outs = outs or [TnOut(j[2], j[5], j[6], j[7]) for j in jobs]
    arr = (hip.GemmTNJob * n)(*[tn_job(*j[:8], o, *(j[8:] or (0, 0))) for j, o in zip(jobs, outs)])
    cptr = (C.c_void_p * n)(*[o.C.data_ptr() for o in outs])
    hip.check(hip.load().dppo_gemm_tn_group_raw(PRECS[prec][0], arr, n, cptr, hip.stream()), "gemm_tn_group_raw")
    torch.cuda.synchronize()
    return outs


def tn_exact_sweep(prec, shape, rows, how, tag):
    N1, lda, N2, ldb = shape
    _, dt, _ = PRECS[prec]
    gen = gen_for("tn", shape, prec)
    mmax = max(m for m, _ in rows)
    # columns N1..lda and N2..ldb and the rows behind M hold data that must not count
    A, B = ints(gen, (mmax + SPARE, lda), dt), ints(gen, (mmax + SPARE, ldb), dt)
    by_m = {}
    for M, rps in rows:
        if M not in by_m:
            by_m[M] = (mm64(A[:M, :N1].t().contiguous(), B[:M, :N2]).float(), [])
        out = run_tn(prec, A, lda, N1, B, ldb, N2, M, rps, how)
        what = f"gemm_tn {tag} {prec} {N1}x{N2} lda={lda} ldb={ldb} M={M} rps={rps} splits={out.splits}"
        assert_exact(out.result(), by_m[M][0], what)
        out.check(what)
        by_m[M][1].append(out.result().clone())
    for M, (_, results) in by_m.items():  # integer data: any split count gives the same bits
        for r in results[1:]:
            assert_bits_equal(r, results[0], f"gemm_tn {tag} {prec} {N1}x{N2} M={M} across split counts")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", TN_SQUARE, ids=lambda s: f"{s[0]}x{s[2]}")
def test_gemm_tn_register_staged_exact(shape, prec):
    """gemm_tn_kernel<2,2,4,4> (knob 5 = 0; knob 6 = 0 keeps (129, 16) off the thin tile)."""
    tune(6, 0)
    assert tn_branch(shape[0], shape[2], 0, 0, False) == "reg128"
    tn_exact_sweep(prec, shape, TN_ROWS, "raw", "reg128")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("knob6", [1, 0])
@pytest.mark.parametrize("shape", TN_THIN, ids=lambda s: f"{s[0]}x{s[2]}")
def test_gemm_tn_thin_outputs_exact(shape, knob6, prec):
    """gemm_tn_kernel<4,1,8,4> (512 x 64 tile, knob 6 = 1) and the same shapes forced onto the square tile (knob 6 = 0)."""
    tune(6, knob6)
    assert tn_branch(shape[0], shape[2], 0, knob6, False) == ("thin" if knob6 else "reg128")
    tn_exact_sweep(prec, shape, TN_ROWS, "raw", "thin" if knob6 else "reg128")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("knob5", TN_DMA_VARIANTS)
def test_gemm_tn_dma_rings_exact(knob5, prec):
    """gemm_tn_dma_kernel, every ring configuration of knob 5, aligned and ragged shapes (a DMA cannot zero-fill: lanes
    without a row or column read the zero page)."""
    tune(5, knob5)
    for shape in TN_DMA_SHAPES:
        want = f"dma{knob5}" if knob5 > 0 else ("dma2" if shape[0] * shape[2] >= 512 * 512 else "reg128")
        assert tn_branch(shape[0], shape[2], knob5, 1, False) == want
        rows = [(50001, 3136), (50000, 6272), (1, 64), (65, 64), (129, 128), (449, 64)]
        tn_exact_sweep(prec, shape, rows, "raw", want)


def summation_bound(A, B, ref, L):
    """2 L 2^-24 (|A|^T |B|) + one fp32 rounding of the result."""
    return 2.0 * L * 2.0 ** -24 * (A.double().abs().t() @ B.double().abs()) + 2.0 ** -24 * ref.abs()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_gemm_tn_random_data_within_the_summation_bound(prec):
    """The LDS-DMA rings and the thin tile on random normal data (no bit-identity promised there)."""
    _, dt, _ = PRECS[prec]
    todo = [(s, 5, v) for s in [TN_DMA_SHAPES[0], TN_DMA_SHAPES[3]] for v in TN_DMA_VARIANTS] + [(s, 6, 1) for s in TN_THIN]
    for (N1, lda, N2, ldb), knob, value in todo:
        for M, rps in ((50001, 3136), (449, 64)):
            gen = gen_for("tnrand", N1, N2, prec, M)
            A = torch.randn((M + SPARE, lda), generator=gen, device=DEV).to(dt)
            B = torch.randn((M + SPARE, ldb), generator=gen, device=DEV).to(dt)
            ref = A[:M, :N1].double().t() @ B[:M, :N2].double()
            bound = summation_bound(A[:M, :N1], B[:M, :N2], ref, M)
            tune(5, 0), tune(6, 1), tune(knob, value)
            out = run_tn(prec, A, lda, N1, B, ldb, N2, M, rps, "raw")
            what = f"gemm_tn {tn_branch(N1, N2, value if knob == 5 else 0, 1, False)} {prec} {N1}x{N2} M={M}"
            err = (out.result().double() - ref).abs()
            print(f"{what}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3e}")
            assert bool((err <= bound).all()), what
            out.check(what)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_gemm_tn_one_hot_probe(prec):
    """A one-hot per batch row, B index-coded: C[n1][n2] = sum of the B codes of the rows whose hot column is n1 -- with
    one row per n1 (M <= N1) the output IS the element read.  Register-staged, thin, grouped and ring kernels."""
    _, dt, _ = PRECS[prec]
    for (N1, N2, M, how, knob5, knob6) in ((200, 136, 200, "raw", 0, 1), (512, 64, 300, "raw", 0, 1), (200, 136, 150, "group", 0, 1),
                                           (200, 136, 200, "raw", 1, 1), (256, 256, 256, "raw", 7, 1), (512, 40, 64, "raw", 0, 0)):
        tune(5, knob5), tune(6, knob6)
        lda, ldb = rup(N1, 8) + 8, rup(N2, 8) + 8
        hot_col = (torch.arange(M, device=DEV) * 3 + 1) % N1 if M < N1 else torch.arange(M, device=DEV)
        assert hot_col.unique().numel() == M
        A = torch.ones(M + SPARE, lda, device=DEV)
        A[:M] = 0
        A[torch.arange(M, device=DEV), hot_col] = 1
        code = torch.arange(M * N2, device=DEV).reshape(M, N2)
        code = code if prec == "fp32" else code % 257
        B = torch.full((M + SPARE, ldb), 5.0, device=DEV)
        B[:M, :N2] = code.float()
        ref = torch.zeros(N1, N2, device=DEV)
        ref[hot_col] = code.float()
        out = run_tn(prec, A.to(dt), lda, N1, B.to(dt), ldb, N2, M, 64, how)
        got = out.result()
        if not torch.equal(got, ref):
            i = tuple((got != ref).nonzero()[0].tolist())
            g = int(got[i].item())
            where = f"row {g // N2} col {g % N2}" if prec == "fp32" else f"code {g}"
            raise AssertionError(f"gemm_tn {how} knob5={knob5} knob6={knob6} {prec} {N1}x{N2} M={M}: C{i} holds B {where}, "
                                 f"expected {ref[i].item()}")
        out.check("one-hot")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("how", ["job", "group"])
def test_gemm_tn_overlapping_rows(how, prec):
    """An operand that is a window of width 3 C at stride C over a channel-last buffer (ncol_a / ncol_b: the conv
    denoiser's im2col); the reference reads the same buffer through as_strided."""
    _, dt, _ = PRECS[prec]
    for Cc, N2, M, rps in ((16, 40, 1000, 256), (64, 136, 4099, 1024), (8, 16, 65, 64), (72, 24, 300, 64)):
        gen = gen_for("overlap", Cc, N2, M, prec)
        buf = ints(gen, ((M + SPARE + 2) * Cc,), dt)  # M (+ SPARE) windows of 3 C elements, one every C
        other = ints(gen, (M + SPARE, N2 + 8), dt)
        win = buf.as_strided((M, 3 * Cc), (Cc, 1))
        for side in ("a", "b"):
            if side == "a":
                assert tn_branch(3 * Cc, N2, 3, 1, True) == "reg128"
                tune(5, 3)  # overlapping rows stay on the register-staged kernel whatever knob 5 says
                ref = mm64(win.t().contiguous(), other[:M, :N2])
                out = run_tn(prec, buf, Cc, 3 * Cc, other, N2 + 8, N2, M, rps, how, ncol_a=3 * Cc)
            else:
                ref = mm64(other[:M, :N2].t().contiguous(), win)
                out = run_tn(prec, other, N2 + 8, N2, buf, Cc, 3 * Cc, M, rps, how, ncol_b=3 * Cc)
            what = f"gemm_tn {how} overlapping {side} {prec} C={Cc} N2={N2} M={M}"
            assert_exact(out.result(), ref.float(), what)
            out.check(what)


# ------------------------------------------------------------------------------------------------------ grouped kernel
def hopper_jobs(gen, dt, M):
    """The weight-gradient products of the hopper actor's backward (hidden 512, in 39 -> 64 padded, out 12), in the order
    a backward pass queues them, with the row splits weight_grad() gives them at 50,000 samples: rows_per_split ascends."""
    jobs = []
    for N1, lda, N2, ldb, rps in ((512, 512, 12, 16, 832), (512, 512, 39, 48, 832), (512, 512, 64, 64, 832),
                                  (512, 512, 512, 512, 3136), (512, 520, 512, 512, 3136)):
        jobs.append((ints(gen, (M + SPARE, lda), dt), lda, N1, ints(gen, (M + SPARE, ldb), dt), ldb, N2, M, rps))
    return jobs


def group_grid(jobs):
    return sum(cdiv(j[6], j[7]) * cdiv(j[2], 128) * cdiv(j[5], 128) for j in jobs)


def check_group(prec, jobs, what):
    outs = run_group(prec, jobs)
    for i, (j, o) in enumerate(zip(jobs, outs)):
        A, lda, N1, B, ldb, N2, M, rps = j[:8]
        ref = mm64(A[:M, :N1].t().contiguous(), B[:M, :N2]).float()
        assert_exact(o.result(), ref, f"{what} job {i} ({N1}x{N2} M={M} rps={rps})")
        o.check(f"{what} job {i}")
    return outs


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("knob26", [1, 2, 0])
def test_gemm_tn_group_exact(knob26, prec):
    """gemm_tn_group_kernel<NBUF = 1 / 2>: groups of 1, 3 and 8 jobs handed over with rows_per_split NOT descending (the
    sort and base[] matter), the hopper actor's real set, unequal M per job; knob 26 = 0 picks NBUF by size."""
    _, dt, _ = PRECS[prec]
    tune(26, knob26)
    gen = gen_for("group", prec)
    # hopper at 50,000 samples: 1,244 workgroups over >= 32,768 rows -> two stages; at 30,000: one
    for M, nbuf0 in ((50000, 2), (30000, 1)):
        jobs = hopper_jobs(gen, dt, M)
        assert [j[7] for j in jobs] == sorted(j[7] for j in jobs) and jobs[0][7] < jobs[-1][7]
        assert group_nbuf(knob26, group_grid(jobs), M) == (knob26 or nbuf0)
        check_group(prec, jobs, f"group hopper M={M} {prec} knob26={knob26}")
    # 1 job; 3 jobs; 8 jobs of unequal M and shape (ragged tiles, a last split of one row)
    shapes = [(200, 200, 136, 136, 449, 64), (16, 16, 16, 24, 1, 64), (129, 136, 16, 16, 5000, 128), (256, 256, 256, 264, 33000, 4160),
              (65, 72, 64, 72, 65, 64), (128, 136, 128, 128, 48769, 384), (512, 512, 12, 16, 127, 128), (40, 40, 300, 304, 2049, 1024)]
    for n in (1, 3, 8):
        jobs = [(ints(gen, (M + SPARE, lda), dt), lda, N1, ints(gen, (M + SPARE, ldb), dt), ldb, N2, M, rps)
                for N1, lda, N2, ldb, M, rps in shapes[:n]]
        if n > 1:
            assert [j[7] for j in jobs] != sorted((j[7] for j in jobs), reverse=True)
        first_m = sorted(jobs, key=lambda j: -j[7])[0][6]  # (stable, as the library's insertion sort)
        assert group_nbuf(knob26, group_grid(jobs), first_m) == (knob26 or 1)
        check_group(prec, jobs, f"group of {n} {prec} knob26={knob26}")
    # knob 26 = 0 on the far side of the switch by size alone: one big job
    M = 40000
    jobs = [(ints(gen, (M + SPARE, 512), dt), 512, 512, ints(gen, (M + SPARE, 512), dt), 512, 512, M, 640)]
    assert group_grid(jobs) == 63 * 16 and group_nbuf(knob26, group_grid(jobs), M) == (knob26 or 2)
    check_group(prec, jobs, f"group of one large job {prec} knob26={knob26}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_gemm_tn_grouped_equals_ungrouped_bit_for_bit(prec):
    """The grouped kernel runs the same tn_tile as gemm_tn_kernel<2,2,4,4>, with one LDS stage or two: random normal data,
    identical bits (jobs the ungrouped path also runs on the 128 x 128 tile: knob 5 = 0, knob 6 = 0)."""
    _, dt, _ = PRECS[prec]
    gen = gen_for("groupbits", prec)
    specs = [(512, 512, 12, 16, 832), (200, 200, 136, 136, 1088), (512, 512, 512, 512, 3136), (256, 264, 256, 256, 3136)]
    M = 50000
    jobs = [(torch.randn((M + SPARE, lda), generator=gen, device=DEV).to(dt), lda, N1,
             torch.randn((M + SPARE, ldb), generator=gen, device=DEV).to(dt), ldb, N2, M, rps) for N1, lda, N2, ldb, rps in specs]
    tune(5, 0), tune(6, 0)
    res = {}
    for nbuf in (1, 2):
        tune(26, nbuf)
        res[nbuf] = [o.result().clone() for o in run_group(prec, jobs)]
    for i, j in enumerate(jobs):
        A, lda, N1, B, ldb, N2, M, rps = j
        assert tn_branch(N1, N2, 0, 0, False) == "reg128"
        alone = run_tn(prec, A, lda, N1, B, ldb, N2, M, rps, "raw").result()
        what = f"{prec} job {i} ({N1}x{N2})"
        assert_bits_equal(res[1][i], res[2][i], "NBUF 1 vs 2 " + what)
        assert_bits_equal(res[1][i], alone, "grouped vs ungrouped " + what)
        ref = A[:M, :N1].double().t() @ B[:M, :N2].double()
        assert bool(((alone.double() - ref).abs() <= summation_bound(A[:M, :N1], B[:M, :N2], ref, M)).all()), what
