#!/usr/bin/env python
"""Record aon_gemm_workspace_bytes / aon_gemm_batch_workspace_bytes for a table of argument sets
(tests/golden/gemm_workspace.json, pinned by tests/test_capi.py).  Both are pure host functions
of the split policy: no GPU is needed and no pointer is dereferenced.

    python tools/gemm_workspace_table.py [--lib PATH] [--commit HASH] > tests/golden/gemm_workspace.json

A case lists only the aon_gemm_args fields that differ from DEFAULTS (below, recorded as the
table's "defaults"); lda / ldb / ldc default to the operand widths (M, N, N)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "articulated-object-nerf_amd"))

ALIGNED, MISALIGNED = 1 << 20, (1 << 20) + 2  # fake operand addresses
DEFAULTS = dict(A=ALIGNED, B=ALIGNED, C=ALIGNED, b_rdiv=1, a_scale=1.0, b_scale=1.0)
KS = (4096, 8192 + 40, 266240)  # no split; ragged last tile; the coarse level's rows


def gemm_args(L, case):
    f = dict(DEFAULTS, lda=case["M"], ldb=case["N"], ldc=case["N"])
    f.update(case)
    return L.AonGemmArgs(**f)


BF = dict(mma_bf16=1, a_bf16=1, b_bf16=1)
F1 = dict(f16_single=1, a_tiled=1, b_tiled=1)
KC = dict(a_kc=1, b_kc=1)


def single_cases():
    """(name, fields) for every route at every K of KS (k_splits 0, and 3 at the middle K), and
    both sides of each routing condition."""
    base = [
        # small exact-fp32: M N at 65,536 and above it, K at and above 1,024
        ("exact_16x16", dict(M=16, N=16, exact_fp32=1, **KC)),
        ("exact_256x256", dict(M=256, N=256, exact_fp32=1, **KC)),
        ("exact_256x257", dict(M=256, N=257, exact_fp32=1, **KC)),
        # segment-sum: b_rdiv at 40 and at 1, bf16 and exact fp32, misaligned A, lda % 8 != 0
        ("segsum_bf16_rdiv40", dict(M=256, N=64, b_rdiv=40, **BF)),
        ("segsum_bf16_rdiv1", dict(M=256, N=64, b_rdiv=1, **BF)),
        ("segsum_f32_rdiv40", dict(M=8, N=24, b_rdiv=40)),
        ("segsum_bf16_misaligned", dict(M=256, N=64, b_rdiv=40, A=MISALIGNED, **BF)),
        ("segsum_bf16_lda260", dict(M=256, N=64, b_rdiv=40, lda=260, **BF)),
        ("segsum_bf16_m264", dict(M=264, N=64, b_rdiv=40, **BF)),
        # skinny: M at 4 and 5, N at 256 and 264, c_trans, exact fp32
        ("skinny_bf16_m1", dict(M=1, N=256, mma_bf16=1, b_bf16=1)),
        ("skinny_bf16_m4", dict(M=4, N=256, mma_bf16=1, b_bf16=1)),
        ("skinny_bf16_m5", dict(M=5, N=256, mma_bf16=1, b_bf16=1)),
        ("skinny_bf16_m4_n264", dict(M=4, N=264, mma_bf16=1, b_bf16=1)),
        ("skinny_bf16_m3_ctrans", dict(M=3, N=128, ldc=3, c_trans=1, mma_bf16=1, b_bf16=1)),
        ("skinny_f32_m3", dict(M=3, N=128)),
        ("skinny_f32_m3_bias", dict(M=3, N=128, bias=ALIGNED)),
        # f1: f16_single set and clear at its three shapes and at 256 x 128
        ("f1_256x256", dict(M=256, N=256, **F1)),
        ("f1_128x256", dict(M=128, N=256, **F1)),
        ("f1_256x64", dict(M=256, N=64, **F1)),
        ("f1_256x128", dict(M=256, N=128, **F1)),
        ("nof1_256x256", dict(M=256, N=256, a_tiled=1, b_tiled=1)),
        ("nof1_128x256", dict(M=128, N=256, a_tiled=1, b_tiled=1)),
        ("nof1_256x64", dict(M=256, N=64, a_tiled=1, b_tiled=1)),
        ("nof1_256x128", dict(M=256, N=128, a_tiled=1, b_tiled=1)),
        # bf16 LDS-DMA 256-tile: aligned and misaligned pairs, lda % 8 != 0, several tiles
        ("dma256_256x256", dict(M=256, N=256, **BF)),
        ("dma256_misaligned_a", dict(M=256, N=256, A=MISALIGNED, **BF)),
        ("dma256_misaligned_b", dict(M=256, N=256, B=MISALIGNED, **BF)),
        ("dma256_lda260", dict(M=256, N=256, lda=260, **BF)),
        ("dma256_512x256", dict(M=512, N=256, **BF)),
        ("dma256_4096x4096", dict(M=4096, N=4096, **BF)),
        # bf16 LDS-DMA 128-tile, n_store < N
        ("dma128_128x256", dict(M=128, N=256, **BF)),
        ("dma128_384x128", dict(M=384, N=128, **BF)),
        ("dma128_nstore", dict(M=256, N=128, n_store=100, **BF)),
        ("dma128_3072x3072", dict(M=3072, N=3072 + 128, **BF)),
        # bf16 register-staged: ragged shapes, fp32 operands
        ("bf16km_100x60", dict(M=100, N=60, **BF)),
        ("bf16km_f32_256x256", dict(M=256, N=256, mma_bf16=1)),
        ("bf16km_rdiv40_m260", dict(M=260, N=64, b_rdiv=40, **BF)),
        # generic fp16x3: a layer product, a weight gradient, A2, n_store < N
        ("generic_layer", dict(M=4096, N=256, lda=0, ldb=0, **KC)),
        ("generic_dw_256x256", dict(M=256, N=256)),
        ("generic_dw_300x70", dict(M=300, N=70)),
        ("generic_nstore", dict(M=256, N=128, n_store=100)),
        ("generic_a2", dict(M=512, N=256, lda=0, ldb=0, A2=ALIGNED, lda2=64, K1=-64, a2_rdiv=64,
                            **KC)),
        ("generic_tiles512", dict(M=4096, N=2048)),
    ]
    out = []
    for name, f in base:
        for K in KS:
            for ks in ((0, 3) if K == KS[1] else (0,)):
                c = dict(f, K=K)
                if ks:
                    c["k_splits"] = ks
                # k-contiguous operands: leading dimension K (A2: its columns start at K - 64)
                for ld in ("lda", "ldb"):
                    if c.get(ld) == 0:
                        c[ld] = K
                if c.get("K1", 0) < 0:
                    c["K1"] += K
                out.append((f"{name}_k{K}_s{ks}", c))
    # small path: K at its limit and past it
    for K in (8, 1024, 1025):
        out.append((f"small_16x16_k{K}", dict(M=16, N=16, K=K, lda=K, ldb=K, exact_fp32=1, **KC)))
    return out


def batch_cases():
    f1 = dict(M=256, N=256, **F1)
    d256 = dict(M=256, N=256, **BF)
    d128a, d128b = dict(M=128, N=256, **BF), dict(M=256, N=128, **BF)
    f16 = dict(M=256, N=256)
    f16b = dict(M=128, N=128)
    skinny = dict(M=3, N=128, mma_bf16=1, b_bf16=1)
    segsum = dict(M=256, N=64, b_rdiv=40, **BF)
    out = []
    for K in KS:
        k = lambda *cs: [dict(c, K=K) for c in cs]  # noqa: E731
        out += [
            (f"f1_x8_k{K}", k(*[f1] * 8)),
            (f"f1_x8_and_other_shapes_k{K}", k(*[f1] * 8, dict(M=128, N=256, **F1),
                                               dict(M=256, N=64, **F1))),
            (f"bf16_mix_k{K}", k(d256, d128a, d256, d128b, d256)),
            (f"bf16_mix_heads_k{K}", k(d256, d128a, d256, d128b, skinny, segsum)),
            (f"f16_x4_k{K}", k(f16, f16, f16b, f16)),
            (f"f16_ksplits_k{K}", k(f16, dict(f16, k_splits=3), f16)),
            (f"one_f1_k{K}", k(f1)),
            (f"one_dma256_k{K}", k(d256)),
            (f"one_dma128_k{K}", k(d128a)),
            (f"one_f16_k{K}", k(f16)),
            (f"other_k_k{K}", k(d256, d256) + [dict(d256, K=K + 32)] + k(d256)),
            (f"other_k_f1_k{K}", [dict(f1, K=70003)] + k(f1, f1)),
            (f"all_classes_k{K}", k(f1, f1, f16, f16b, d256, d256, d128a, d128b, skinny, segsum)),
            (f"max_count_k{K}", k(*[d128a] * 12)),
        ]
    return out


def measure(L, singles, batches):
    import ctypes

    lib = L.lib()
    table = {"single": [], "batch": []}
    for name, c in singles:
        a = gemm_args(L, c)
        table["single"].append({"name": name, "args": c,
                                "bytes": int(lib.aon_gemm_workspace_bytes(ctypes.byref(a)))})
    for name, cs in batches:
        arr = (L.AonGemmArgs * len(cs))(*[gemm_args(L, c) for c in cs])
        table["batch"].append({"name": name, "args": cs,
                               "bytes": int(lib.aon_gemm_batch_workspace_bytes(arr, len(cs)))})
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="library to record from (default: the release library)")
    ap.add_argument("--commit", default="", help="commit the library was built from (recorded)")
    o = ap.parse_args()
    from aonerf import _lib as L

    if o.lib:
        L.use_library(o.lib)
    table = {"recorded_from": o.commit}
    table.update(measure(L, single_cases(), batch_cases()))
    out = ["{", f' "recorded_from": {json.dumps(o.commit)},',
           f' "defaults": {json.dumps(DEFAULTS)},']
    for key in ("single", "batch"):
        out.append(f' "{key}": [')
        rows = [json.dumps(r, separators=(",", ":")) for r in table[key]]
        out.append(",\n".join("  " + r for r in rows))
        out.append(" ]," if key == "single" else " ]")
    out.append("}")
    print("\n".join(out))


if __name__ == "__main__":
    main()
