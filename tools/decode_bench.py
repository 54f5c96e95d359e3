#!/usr/bin/env python3
"""Decode-time expert GEMMs: the weight-streaming kernel (csmoe_grouped_gemm_skinny, gather folded into the first product) against
the same two products through csmoe_grouped_gemm(kernel=AUTO) behind a dispatch_tokens copy -- what a layer call does without
the decode switch.  usage: python tools/decode_bench.py [--reps 30] [--out table.md] [--dtype bf16|fp8|fp4]

Grid: T in {1 .. 256} tokens, K = 2, at the headline dimensions (D 4096, F 11008, 64 experts) and at the SigLIP layer's (1152 / 4304,
4 experts), both weight layouts (B_NK with GELU as the LLaVA stack runs it, B_KN with ReLU as the pretrain stack does).  Both paths
are timed by device events around their launches, alternating in one process, `--reps` repetitions after 5 warm-ups; the median
is reported.  "cold": the routing changes every repetition and the weights rotate over enough copies that the set a repetition
reads was last touched more than 256 MiB (the Infinity Cache) of other weights ago, so the active experts' weights come from HBM.
"warm": the same routing and the same copy every repetition (Infinity-Cache-resident where the active weights fit).

The calls are bound by bandwidth: `GB` is the algorithmic weight traffic of a repetition (the two matrices of every expert that
received a row, bf16, read once), `% HBM` that traffic per second of the new path over the 8.0 TB/s HBM3E peak of the MI355X
(6.3 TB/s is what a copy kernel reaches).

--dtype fp8 (the fp8 layers, `args.fp8_experts`): at the headline dimensions and at BASELINE config 5's (128 experts) three chains
are timed the same way, each in its own series of one process: the fp8 decode chain (quantize_mxfp8 of the T rows + two
csmoe_grouped_gemm_skinny_mxfp8 launches, the first gathering and writing the MXFP8 hidden activations), the tiled fp8 chain the
layer runs without the switch (dispatch_tokens_mxfp8 + grouped_gemm_mxfp8 + quantize_mxfp8 + grouped_gemm_mxfp8), and the bf16
decode chain at the same dimensions (B_KN, ReLU: the pretrain stack).  `+-` is half the interquartile range of the repetitions;
the fp8 weight traffic counts one byte per element plus the scale bytes (1 / 32).

--dtype fp4 (`args.fp4_decode_weights`): the W4A8 decode chain (quantize_mxfp8 of the T rows + two csmoe_grouped_gemm_skinny_mxfp4w
launches on MXFP4 weight tables) beside the fp8 decode chain above, in the same process and rotation (the order of the two
alternates with the repetition; cold, each chain reads its own copies, at least three of them).  The fp4 weight traffic counts
half a byte per element plus the scale bytes: 0.516 of the fp8 table, the bound of the ratio.  The last columns are the bytes the
two weight caches of a layer of these dimensions hold (both tables of all E experts, forward orientation).

--layer [--dtype bf16|fp8|fp4]: the WHOLE layer forward (router, binning, quantiser, expert GEMMs, combine) under torch.no_grad() with
decode_rows on, the decode front end (competesmoe_amd.decode_front: csmoe_decode_route) off and on, alternating in one process; T in
{1 .. 64}.  Layers: pretrain `smoe` at the headline dimensions (64 experts) and `deepseekv2` at BASELINE config 5's (128 routed + 2
shared); bf16 modules, with `fp8_experts` + `fp8_weight_cache` (and `fp4_decode_weights`) for --dtype fp8 (fp4).  Cold: the
repetitions rotate over copies of the layer and over inputs (so the routing changes).  Per cell: device time (events around the
call) and host wall time per call (a batch of calls ended by one synchronise, divided by the batch size: the enqueue side is what
the launch count buys), median +- half the interquartile range over `--reps` repetitions after 5 warm-ups, and the number of
launching csmoe_* C calls per layer call in each arm (csmoe_bin_tokens_hist is two kernels, csmoe_bin_tokens three,
csmoe_decode_route one kernel behind a memset node; torch's own kernels are not counted).  The "off" arm is the path without the
switch, which tests/test_decode_front_path_gpu.py pins bit for bit against the "on" arm."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from competesmoe_amd import ops, _lib as L  # noqa: E402

DEV = "cuda"
HBM_PEAK = 8.0e12
TS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
DIMS = {"headline": (4096, 11008, 64), "siglip": (1152, 4304, 4), "config5": (4096, 11008, 128)}
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


def weight_sets_fp8(D, F, E):
    """Copies of the two MXFP8 forward tables ([E, F, D] / [E, D, F] e4m3 with scales along the last dim): finite random bytes."""
    one = 2 * E * D * F
    n = max(3, min(12, -(-(3 * 256 << 20) // one)))        # at least 3: two chains read these, and never the same copy in a repetition

    def mk(rows, cols):
        q = torch.randint(0, 120, (E, rows, cols), device=DEV, dtype=torch.uint8)
        q += torch.randint(0, 2, (E, rows, cols), device=DEV, dtype=torch.uint8) * 128
        return q, torch.randint(112, 118, (E, rows, cols // 32), device=DEV, dtype=torch.uint8)
    return [(mk(F, D), mk(D, F)) for _ in range(n)]


def _med_spread(events):
    ms = sorted(a.elapsed_time(b) for a, b in events)
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), (q[2] - q[0]) / 2


def bench_case_fp8(sets8, sets16, D, F, E, T, reps, warm):
    """(median ms, spread) of the fp8 decode chain, the tiled fp8 chain and the bf16 decode chain, and the active experts."""
    g = torch.Generator().manual_seed(1000 * T + 8)
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
    tabs16 = [(ops.ptr_table(w1, E, D * F * 2), ops.ptr_table(w2, E, D * F * 2)) for w1, w2 in sets16]

    def new8(bins, t):
        (kq, ks), (vq, vs) = t
        xq, xs = ops.quantize_mxfp8(x)
        _, _, hq, hs = ops.grouped_gemm_skinny_mxfp8(xq, xs, kq, ks, bins.offsets, epilogue=L.EPI_BIAS_ACT, act=L.ACT_RELU, want_c=False,
                                                     want_q=True, src_rows=bins.perm, src_div=K)
        ops.grouped_gemm_skinny_mxfp8(hq, hs, vq, vs, bins.offsets)

    def old8(bins, t):
        (kq, ks), (vq, vs) = t
        _, xq, xs = ops.dispatch_tokens_mxfp8(x, bins)
        _, h = ops.grouped_gemm_mxfp8(xq, xs, kq, ks, bins.offsets, epilogue=L.EPI_BIAS_ACT, act=L.ACT_RELU, want_c2=True, want_c=False)
        hq, hs = ops.quantize_mxfp8(h)
        ops.grouped_gemm_mxfp8(hq, hs, vq, vs, bins.offsets)

    def new16(bins, t):
        _, h = ops.grouped_gemm_skinny(x, t[0], L.B_KN, F, F, bins.offsets, E, epilogue=L.EPI_BIAS_ACT, act=L.ACT_RELU, want_c2=True,
                                       want_c=False, src_rows=bins.perm, src_div=K)
        ops.grouped_gemm_skinny(h, t[1], L.B_KN, D, D, bins.offsets, E)

    # (name, chain, its weight copies, copies a repetition advances by, offset of this chain): cold, the two fp8 chains of
    # repetition r read fp8 copies 2 r and 2 r + 1 (mod n >= 3: never the same one, and a copy's next use comes after the other
    # copies' traffic), the bf16 chain its own copy r
    chains = (("new8", new8, sets8, 2, 0), ("old8", old8, sets8, 2, 1), ("new16", new16, tabs16, 1, 0))
    ev = {c[0]: [] for c in chains}
    for r, (idx, bins, active) in enumerate(routes):
        for j in range(3):
            name, fn, pool, step, own = chains[(r + j) % 3]
            t = pool[0] if warm else pool[(step * r + own) % len(pool)]
            e = timed(lambda: fn(bins, t))
            if r >= 5:
                ev[name].append(e)
    torch.cuda.synchronize()
    return {k: _med_spread(v) for k, v in ev.items()}, statistics.median(a for _, _, a in routes[5:])


def main_fp8(a):
    lines = [f"device: {torch.cuda.get_device_name(0)}; reps {a.reps}, median +- half the interquartile range; K = {K}; ReLU", "",
             "| dims | T | rows | cold fp8 decode ms | cold fp8 tiled ms | tiled/decode | cold bf16 decode ms | bf16/fp8 decode | fp8 GB | "
             "fp8 decode GB/s | % of 8.0 TB/s | bf16 decode GB/s | % of 8.0 TB/s | warm fp8 decode ms | warm fp8 tiled ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in a.dims.split(","):
        D, F, E = DIMS[name]
        sets8 = weight_sets_fp8(D, F, E)
        sets16 = [(torch.randn(E, D * F, device=DEV, dtype=torch.bfloat16) * 0.02, torch.randn(E, D * F, device=DEV, dtype=torch.bfloat16) * 0.02)
                  for _ in range(2)]
        for T in TS:
            cold, active = bench_case_fp8(sets8, sets16, D, F, E, T, a.reps, warm=False)
            warm, _ = bench_case_fp8(sets8, sets16, D, F, E, T, a.reps, warm=True)
            b8, b16 = active * 2 * D * F * (1 + 1 / 32), active * 2 * D * F * 2
            (n8, sn8), (o8, so8), (n16, sn16) = cold["new8"], cold["old8"], cold["new16"]
            bw8, bw16 = b8 / (n8 * 1e-3), b16 / (n16 * 1e-3)
            lines.append(f"| {name} | {T} | {T * K} | {n8:.4f} +- {sn8:.4f} | {o8:.4f} +- {so8:.4f} | {o8 / n8:.2f} | {n16:.4f} +- {sn16:.4f} | "
                         f"{n16 / n8:.2f} | {b8 / 1e9:.3f} | {bw8 / 1e9:.0f} | {100 * bw8 / HBM_PEAK:.1f} | {bw16 / 1e9:.0f} | "
                         f"{100 * bw16 / HBM_PEAK:.1f} | {warm['new8'][0]:.4f} | {warm['old8'][0]:.4f} |")
            print(lines[-1], flush=True)
        del sets8, sets16
        torch.cuda.empty_cache()
    return lines


def weight_sets_fp4(D, F, E):
    """Copies of the two MXFP4 forward tables ([E, F, D / 2] / [E, D, F / 2] packed e2m1, scales [.., / 32]): every byte is two
    finite elements."""
    one = E * D * F
    n = max(3, min(12, -(-(3 * 256 << 20) // one)))

    def mk(rows, cols):
        return (torch.randint(0, 256, (E, rows, cols // 2), device=DEV, dtype=torch.uint8),
                torch.randint(112, 118, (E, rows, cols // 32), device=DEV, dtype=torch.uint8))
    return [(mk(F, D), mk(D, F)) for _ in range(n)]


def bench_case_fp4(sets4, sets8, D, F, E, T, reps, warm):
    """(median ms, spread) of the fp4 (W4A8) decode chain and the fp8 decode chain, and the active experts."""
    g = torch.Generator().manual_seed(1000 * T + 4)
    x = torch.randn(T, D, generator=g).bfloat16().to(DEV)
    routes = []
    for r in range(reps + 5):
        idx = torch.rand(T, E, generator=g).topk(K, -1).indices.int()
        if warm and routes:
            idx = routes[0][0].cpu()
        active = int(idx.unique().numel())
        idx = idx.to(DEV)
        routes.append((idx, ops.bin_tokens(idx, E), active))

    def chain(gemm):
        def run(bins, t):
            (kq, ks), (vq, vs) = t
            xq, xs = ops.quantize_mxfp8(x)
            _, _, hq, hs = gemm(xq, xs, kq, ks, bins.offsets, epilogue=L.EPI_BIAS_ACT, act=L.ACT_RELU, want_c=False, want_q=True,
                                src_rows=bins.perm, src_div=K)
            gemm(hq, hs, vq, vs, bins.offsets)
        return run

    chains = (("fp4", chain(ops.grouped_gemm_skinny_mxfp4w), sets4), ("fp8", chain(ops.grouped_gemm_skinny_mxfp8), sets8))
    ev = {c[0]: [] for c in chains}
    for r, (idx, bins, active) in enumerate(routes):
        for j in range(2):
            name, fn, pool = chains[(r + j) % 2]
            t = pool[0] if warm else pool[r % len(pool)]     # cold: a copy's next use comes after the other copies' and chain's traffic
            e = timed(lambda: fn(bins, t))
            if r >= 5:
                ev[name].append(e)
    torch.cuda.synchronize()
    return {k: _med_spread(v) for k, v in ev.items()}, statistics.median(a for _, _, a in routes[5:])


def main_fp4(a):
    lines = [f"device: {torch.cuda.get_device_name(0)}; reps {a.reps}, median +- half the interquartile range; K = {K}; ReLU", "",
             "| dims | T | rows | cold fp4 decode ms | cold fp8 decode ms | fp8/fp4 | wins by more than both spreads | fp4 GB | fp4 GB/s | "
             "% of 8.0 TB/s | fp8 GB | fp8 GB/s | % of 8.0 TB/s | warm fp4 ms | warm fp8 ms | warm fp8/fp4 | fp4 cache GB | fp8 cache GB |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in a.dims.split(","):
        D, F, E = DIMS[name]
        sets4, sets8 = weight_sets_fp4(D, F, E), weight_sets_fp8(D, F, E)
        c4, c8 = E * 2 * D * F * (0.5 + 1 / 32), E * 2 * D * F * (1 + 1 / 32)
        for T in TS:
            cold, active = bench_case_fp4(sets4, sets8, D, F, E, T, a.reps, warm=False)
            warm, _ = bench_case_fp4(sets4, sets8, D, F, E, T, a.reps, warm=True)
            b4, b8 = active * 2 * D * F * (0.5 + 1 / 32), active * 2 * D * F * (1 + 1 / 32)
            (n4, s4), (n8, s8) = cold["fp4"], cold["fp8"]
            (w4, ws4), (w8, ws8) = warm["fp4"], warm["fp8"]
            bw4, bw8 = b4 / (n4 * 1e-3), b8 / (n8 * 1e-3)
            verdict = "fp4" if n8 - n4 > s4 + s8 else ("fp8" if n4 - n8 > s4 + s8 else "neither")
            lines.append(f"| {name} | {T} | {T * K} | {n4:.4f} +- {s4:.4f} | {n8:.4f} +- {s8:.4f} | {n8 / n4:.2f} | {verdict} | {b4 / 1e9:.3f} | "
                         f"{bw4 / 1e9:.0f} | {100 * bw4 / HBM_PEAK:.1f} | {b8 / 1e9:.3f} | {bw8 / 1e9:.0f} | {100 * bw8 / HBM_PEAK:.1f} | "
                         f"{w4:.4f} +- {ws4:.4f} | {w8:.4f} +- {ws8:.4f} | {w8 / w4:.2f} | {c4 / 1e9:.2f} | {c8 / 1e9:.2f} |")
            print(lines[-1], flush=True)
        del sets4, sets8
        torch.cuda.empty_cache()
    return lines


LAYER_TS = (1, 2, 4, 8, 16, 32, 64)
LAYERS = {"smoe": ("smoe", "headline", {}), "deepseekv2": ("deepseekv2", "config5", {"n_shared_experts": 2})}
_HOST_QUERIES = ("_ok", "_bytes", "_rows", "_ints", "_floats", "_parts", "_cols", "_blocks", "_bound", "_ranges", "_error", "_version",
                 "_info")


class _CountingLib:
    """ops.lib with every launching csmoe_* call counted by name."""

    def __init__(self, lib):
        self._lib, self.counts = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("csmoe_") or name.endswith(_HOST_QUERIES):
            return fn

        def counted(*a):
            self.counts[name] = self.counts.get(name, 0) + 1
            return fn(*a)
        return counted


def _count_launches(call):
    real = ops.lib
    ops.lib = proxy = _CountingLib(real)
    try:
        call()
    finally:
        ops.lib = real
    return proxy.counts


def _stats(v):
    v = sorted(v)
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), (q[2] - q[0]) / 2


HOST_BATCH = 10      # calls per host-time batch


def bench_layer(layers, D, Kl, T, reps, batch=HOST_BATCH):
    """{arm: ((device ms, spread), (host ms per call, spread), launches)} of layer(x) with the front end off / on."""
    import competesmoe_amd
    g = torch.Generator().manual_seed(77 * T)
    xs = [torch.randn(1, T, D, generator=g).bfloat16().to(DEV) for _ in range(8)]
    dev = {False: [], True: []}
    host = {False: [], True: []}
    launches = {}
    with torch.no_grad():
        competesmoe_amd.decode_rows(max(64, T * Kl))
        try:
            for arm in (False, True):                             # also the warm-up of every copy's weight cache
                competesmoe_amd.decode_front(arm)
                for layer in layers:
                    layer(xs[0])
                launches[arm] = _count_launches(lambda: layers[0](xs[0]))
            for r in range(reps + 5):
                for j in range(2):
                    arm = bool((r + j) % 2)
                    competesmoe_amd.decode_front(arm)
                    layer, x = layers[(2 * r + j) % len(layers)], xs[(2 * r + j) % len(xs)]
                    e = timed(lambda: layer(x))
                    if r >= 5:
                        dev[arm].append(e)
            torch.cuda.synchronize()
            for r in range(reps + 2):
                for j in range(2):
                    arm = bool((r + j) % 2)
                    competesmoe_amd.decode_front(arm)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for b in range(batch):
                        layers[(r + b) % len(layers)](xs[(r + b) % len(xs)])
                    torch.cuda.synchronize()
                    if r >= 2:
                        host[arm].append((time.perf_counter() - t0) * 1e3 / batch)
        finally:
            competesmoe_amd.decode_front(False)
            competesmoe_amd.decode_rows(0)
    return {arm: (_stats([a.elapsed_time(b) for a, b in dev[arm]]), _stats(host[arm]), launches[arm]) for arm in (False, True)}


def main_layer(a):
    import types
    import torch.nn.functional as F
    from competesmoe_amd.pretrain import get_moe
    base = dict(stop_after=10, warm_up=0.0, rate_flip=1.0, max_compete_in_iter=8, balance_loss_coef=0.01, balance_loss_coef_comp=0.02,
                router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False, tribrid=False, balance_affinity=False,
                is_cosine=False, is_norm_weight=False, norm_sigmoid=False, scale_weight=1.0, test_only=False)
    if a.dtype != "bf16":
        base.update(fp8_experts=True, fp8_weight_cache=True, fp4_decode_weights=a.dtype == "fp4")
    lines = [f"device: {torch.cuda.get_device_name(0)}; whole layer forward, no_grad, decode_rows on; {a.dtype} experts; reps {a.reps}, "
             f"host batches of {HOST_BATCH} calls; median +- half the interquartile range; K = {K}; ReLU", "",
             "| layer | T | device ms off | device ms on | host ms/call off | host ms/call on | ahead by more than both spreads (device / host) | "
             "csmoe calls off | csmoe calls on |", "|---|---|---|---|---|---|---|---|---|"]
    for lname in a.layers.split(","):
        name, dims, extra = LAYERS[lname]
        D, FH, E = DIMS[dims]
        n = 3 if E <= 64 else 2            # copies of the layer to rotate over
        layers = []
        for c in range(n):
            torch.manual_seed(100 + c)
            with torch.device(DEV):
                layer = get_moe(name)(D, E, FH, n_heads=K, activation=F.relu, bias=False, log_interval=None,
                                      args=types.SimpleNamespace(**base, **extra))
            layers.append(layer.to(torch.bfloat16).eval())
        for T in LAYER_TS:
            res = bench_layer(layers, D, K, T, a.reps)
            (d0, sd0), (h0, sh0), l0 = res[False]
            (d1, sd1), (h1, sh1), l1 = res[True]
            verdict = lambda x0, s0, x1, s1: "on" if x0 - x1 > s0 + s1 else ("off" if x1 - x0 > s0 + s1 else "neither")
            fmt = lambda l: f"{sum(l.values())} (" + ", ".join(f"{k[6:]} {v}" for k, v in sorted(l.items())) + ")"
            lines.append(f"| {lname} {a.dtype} | {T} | {d0:.4f} +- {sd0:.4f} | {d1:.4f} +- {sd1:.4f} | {h0:.4f} +- {sh0:.4f} | "
                         f"{h1:.4f} +- {sh1:.4f} | {verdict(d0, sd0, d1, sd1)} / {verdict(h0, sh0, h1, sh1)} | {fmt(l0)} | {fmt(l1)} |")
            print(lines[-1], flush=True)
        del layers
        if a.dtype != "bf16":
            from competesmoe_amd import functional as Fn
            Fn.fp8_weight_cache_clear()
            Fn.fp4_weight_cache_clear()
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layer", action="store_true", help="whole-layer forward, decode front end off against on")
    ap.add_argument("--layers", default="smoe,deepseekv2", help="--layer: which of " + ", ".join(LAYERS))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dims", default=None, help="default: headline,siglip (bf16) / headline,config5 (fp8, fp4)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "fp4"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.layer:
        if a.reps < 30:
            ap.error("--layer: at least 30 repetitions")
        for name in a.layers.split(","):
            if name not in LAYERS:
                ap.error(f"unknown layer '{name}'; choose from {', '.join(LAYERS)}")
        text = "\n".join(main_layer(a)) + "\n"
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        print(text)
        return
    a.dims = a.dims or ("headline,config5" if a.dtype != "bf16" else "headline,siglip")
    for name in a.dims.split(","):
        if name not in DIMS:
            ap.error(f"unknown dims '{name}'; choose from {', '.join(DIMS)}")
        D, F, _ = DIMS[name]
        if a.dtype != "bf16" and (D % 128 or F % 128):
            ap.error(f"--dtype {a.dtype}: dims '{name}' (D = {D}, F = {F}) are no multiples of 128, which the MXFP8 kernels need for both "
                     "reduction dims; choose from headline, config5")
    lines = {"fp8": main_fp8, "fp4": main_fp4, "bf16": main_bf16}[a.dtype](a)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


def main_bf16(a):
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
    return lines


if __name__ == "__main__":
    main()
