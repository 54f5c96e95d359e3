#!/usr/bin/env python3
"""Decode-time expert GEMMs: the weight-streaming kernel (csmoe_grouped_gemm_skinny, gather folded into the first product) against
the same two products through csmoe_grouped_gemm(kernel=AUTO) behind a dispatch_tokens copy -- what a layer call does without
the decode switch.  usage: python tools/decode_bench.py [--reps 30] [--out table.md]

Grid: T in {1 .. 256} tokens, K = 2, at the headline dimensions (D 4096, F 11008, 64 experts) and at the SigLIP layer's (1152 / 4304,
4 experts), both weight layouts (B_NK with GELU as the LLaVA stack runs it, B_KN with ReLU as the pretrain stack does).  Both paths
are timed by device events around their launches, alternating in one process, `--reps` repetitions after 5 warm-ups; the median
is reported.  "cold": the routing changes every repetition and the weights rotate over enough copies that the set a repetition
reads was last touched more than 256 MiB (the Infinity Cache) of other weights ago, so the active experts' weights come from HBM.
"warm": the same routing and the same copy every repetition (Infinity-Cache-resident where the active weights fit).

The calls are bound by bandwidth: `GB` is the algorithmic weight traffic of a repetition (the two matrices of every expert that
received a row, bf16, read once), `% HBM` that traffic per second of the new path over the 8.0 TB/s HBM3E peak of the MI355X
(6.3 TB/s is what a copy kernel reaches)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from competesmoe_amd import ops, _lib as L  # noqa: E402

DEV = "cuda"
HBM_PEAK = 8.0e12
TS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
DIMS = {"headline": (4096, 11008, 64), "siglip": (1152, 4304, 4)}
K = 2


def weight_sets(D, F, E):
    """Copies of the two weight stacks: enough that one pass over the others evicts a copy from the 256 MiB Infinity Cache."""
    one = 2 * E * D * F * 2
    n = max(2, min(12, -(-(3 * 256 << 20) // one)))        # at least 2: the two paths of a repetition never share a copy
    mk = lambda: (torch.randn(E, F * D, device=DEV, dtype=torch.bfloat16) * 0.02)
    return [(mk(), mk()) for _ in range(n)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def bench_case(sets, D, F, E, layout, T, reps, warm):
    act = L.ACT_GELU if layout == L.B_NK else L.ACT_RELU
    ld1, ld2 = (D, F) if layout == L.B_NK else (F, D)
    g = torch.Generator().manual_seed(1000 * T + layout)
    x = torch.randn(T, D, generator=g).bfloat16().to(DEV)
    total = reps + 5
    routes = []
    for r in range(total):
        idx = torch.rand(T, E, generator=g).topk(K, -1).indices.int()
        if warm and routes:
            idx = routes[0][0].cpu()
        active = int(idx.unique().numel())
        idx = idx.to(DEV)
        routes.append((idx, ops.bin_tokens(idx, E), active))
    tabs = [(ops.ptr_table(w1, E, D * F * 2), ops.ptr_table(w2, E, D * F * 2)) for w1, w2 in sets]

    def new(bins, t):
        _, h = ops.grouped_gemm_skinny(x, t[0], layout, ld1, F, bins.offsets, E, epilogue=L.EPI_BIAS_ACT, act=act, want_c2=True,
                                       want_c=False, src_rows=bins.perm, src_div=K)
        ops.grouped_gemm_skinny(h, t[1], layout, ld2, D, bins.offsets, E)

    def old(bins, t):
        xs = ops.dispatch_tokens(x, bins)
        _, h = ops.grouped_gemm(xs, t[0], layout, ld1, F, bins.offsets, E, epilogue=L.EPI_BIAS_ACT, act=act, want_c2=True,
                                want_c=act != L.ACT_RELU)
        ops.grouped_gemm(h, t[1], layout, ld2, D, bins.offsets, E)

    ev = {"new": [], "old": []}
    for r, (idx, bins, active) in enumerate(routes):
        order = (("new", new), ("old", old)) if r % 2 == 0 else (("old", old), ("new", new))
        for j, (name, fn) in enumerate(order):
            # cold: every launch pair reads a copy that the other copies' traffic has pushed out since its last use
            t = tabs[0] if warm else tabs[(2 * r + j) % len(tabs)]
            e = timed(lambda: fn(bins, t))
            if r >= 5:
                ev[name].append(e)
    torch.cuda.synchronize()
    ms = {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}
    act_med = statistics.median(a for _, _, a in routes[5:])
    return ms["new"], ms["old"], act_med * 2 * D * F * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dims", default="headline,siglip")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}; reps {a.reps}, median; K = {K}", "",
             "| dims | layout | T | rows | cold new ms | cold old ms | old/new | GB (active weights) | cold new GB/s | % of 8.0 TB/s | warm new ms | warm old ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in a.dims.split(","):
        D, F, E = DIMS[name]
        sets = weight_sets(D, F, E)
        for layout in (L.B_NK, L.B_KN):
            for T in TS:
                cn, co, nbytes = bench_case(sets, D, F, E, layout, T, a.reps, warm=False)
                wn, wo, _ = bench_case(sets, D, F, E, layout, T, a.reps, warm=True)
                bw = nbytes / (cn * 1e-3)
                lines.append(f"| {name} | {'B_NK' if layout == L.B_NK else 'B_KN'} | {T} | {T * K} | {cn:.4f} | {co:.4f} | {co / cn:.2f} | "
                             f"{nbytes / 1e9:.3f} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} | {wn:.4f} | {wo:.4f} |")
                print(lines[-1], flush=True)
        del sets
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
