#!/usr/bin/env python3
"""Micro-benchmark + correctness check of the bare MFMA GEMMs (dppo_gemm_nt_raw / dppo_gemm_tn_raw) at the PPO
update's shapes.  Variants are timed interleaved in ONE process on random data (cdna_hip_programming.md rule 24/25).
Every result is ASSERTED against a float64 reference of the same (rounded) operands: per element
|got - ref| <= 2 L 2^-24 (|A|^T |B|) + one rounding of the stored type, L the contraction length (the worst-case
summation bound of tests/test_gemm_primitives.py).

    python tools/gemm_bench.py [--M 50000] [--rounds 5]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dppo_amd import hip  # noqa: E402


def time_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def bound(absA, absB, ref, L, out_eps):
    """absA (L, n1), absB (L, n2) float64 magnitudes of the operands, ref (n1, n2) float64."""
    return 2.0 * L * 2.0 ** -24 * (absA.t() @ absB) + out_eps * ref.abs()


def check(got, ref, bnd, what):
    err = (got.double() - ref).abs()
    worst = (err / bnd.clamp_min(1e-300)).max().item()
    assert worst <= 1.0, f"{what}: max |err| {err.max().item():.3e} is {worst:.2f} x the summation bound"
    return err.max().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=50000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tn-only", action="store_true")
    ap.add_argument("--variants", default="", help="comma list of gemm_tn variants (tuning knob 5); default all")
    ap.add_argument("--prec", default="", help="bf16 or fp32 only")
    ap.add_argument("--shapes", default="512,256", help="comma list of square gemm_tn output sizes")
    args = ap.parse_args()
    lib = hip.load()
    dev = "cuda:0"
    M = args.M
    for prec, name, dt in ((hip.PREC_BF16, "bf16", torch.bfloat16), (hip.PREC_F32, "fp32", torch.float32)):
        if args.prec and args.prec != name:
            continue
        for (N, K) in (() if args.tn_only else ((512, 512), (256, 256), (512, 64))):
            X = torch.randn(M, K, device=dev).to(dt).contiguous()
            W = (torch.randn(N, K, device=dev) / K ** 0.5).to(dt).contiguous()
            b = torch.randn(N, device=dev)
            out = torch.empty(M, N, device=dev)
            oe = torch.empty(M, N, device=dev, dtype=dt)
            ref = X.double() @ W.double().t() + b.double()
            bnd = bound(X.double().abs().t(), W.double().abs().t(), ref, K, 2.0 ** -24) + 2.0 ** -24 * b.double().abs()
            bnd_e = bnd + (2.0 ** -24 if dt == torch.float32 else 2.0 ** -8) * (ref.abs() + bnd)  # + rounding to elem

            def run():
                hip.check(lib.dppo_gemm_nt_raw(prec, X.data_ptr(), W.data_ptr(), b.data_ptr(), M, N, K, out.data_ptr(),
                                               oe.data_ptr(), N, hip.ACT_RELU, hip.stream()), "gemm_nt_raw")
            res = {}
            for variant in (0, 1):
                lib.dppo_tune_set(0, variant)
                run()
                torch.cuda.synchronize()
                what = f"gemm_nt {name} M={M} N={N} K={K} staging={'dma' if variant else 'reg'}"
                err = check(out, ref, bnd, what + " f32-out")
                err_e = check(oe, torch.relu(ref), bnd_e, what + " elem-out")
                res[variant] = [err, err_e, []]
            for _ in range(args.rounds):
                for variant in (0, 1):
                    lib.dppo_tune_set(0, variant)
                    res[variant][2].append(time_ms(run, args.iters))
            for variant in (0, 1):
                err, err_e, ts = res[variant]
                ts = sorted(ts)
                tf = 2.0 * M * N * K / (ts[len(ts) // 2] * 1e-3) / 1e12
                print(f"gemm_nt {name} M={M} N={N} K={K} staging={'dma' if variant else 'reg'}: median {ts[len(ts)//2]*1e3:8.1f} us "
                      f"min {ts[0]*1e3:8.1f} us  {tf:7.1f} TFLOP/s  max|err| f32-out {err:.2e} elem-out {err_e:.2e}", flush=True)
            lib.dppo_tune_set(0, 1)
        # weight-gradient GEMM
        for (N1, N2) in [(int(x), int(x)) for x in args.shapes.split(",")]:
            A = torch.randn(M, N1, device=dev).to(dt).contiguous()
            B = torch.randn(M, N2, device=dev).to(dt).contiguous()
            rps = (M // 32 + 63) // 64 * 64
            splits = (M + rps - 1) // rps
            slab = torch.empty(splits * N1 * N2, device=dev)
            Cc = torch.empty(N1, N2, device=dev)
            ref = A.double().t() @ B.double()
            bnd = bound(A.double().abs(), B.double().abs(), ref, M, 2.0 ** -24)

            def run_tn():
                hip.check(lib.dppo_gemm_tn_raw(prec, A.data_ptr(), N1, N1, B.data_ptr(), N2, N2, M, rps, slab.data_ptr(),
                                               Cc.data_ptr(), hip.stream()), "gemm_tn_raw")
            names = {0: "reg-staged 128x128", 1: "dma 128x128 x3", 2: "dma 128x128 x2", 3: "dma 256x128 x3", 4: "dma 128x128 x4",
                     5: "dma 256x128 w128x64 x2k1", 6: "dma 256x128 w128x64 x3k1", 7: "dma 256x256 8w x2",
                     8: "dma 256x128 w128x64 x2"}
            for variant in (sorted(names) if not args.variants else [int(v) for v in args.variants.split(",")]):
                lib.dppo_tune_set(5, variant)
                Cc.zero_()
                run_tn()
                torch.cuda.synchronize()
                check(Cc, ref, bnd, f"gemm_tn {name} M={M} N1={N1} N2={N2} {names[variant]}")
                err = ((Cc.double() - ref).abs().max() / ref.abs().max()).item()
                ts = sorted(time_ms(run_tn, args.iters) for _ in range(args.rounds))
                tf = 2.0 * M * N1 * N2 / (ts[len(ts) // 2] * 1e-3) / 1e12
                print(f"gemm_tn {name} M={M} N1={N1} N2={N2} splits={splits} {names[variant]:26s}: median "
                      f"{ts[len(ts)//2]*1e3:8.1f} us  {tf:7.1f} TFLOP/s (incl. slab reduce)  rel err {err:.2e}", flush=True)
            lib.dppo_tune_set(5, 0)


if __name__ == "__main__":
    main()
