#!/usr/bin/env python3
"""One-pass router (csmoe_gate_select) against gate GEMM + router_select + counting pass at the headline token count, and the
one-pass XMoE cosine router (csmoe_cosine_select) against the torch-op form of the same gate and against csmoe_gate_select at the
same T and D (it streams the same bytes); `perturbed`: the same kernel in its CSMOE_COS_NORM_THETA mode (`smoe_perturbed`) against
the XMoE mode of the same build and the torch-op gate; `sigmoid`: csmoe_gate_select with the rule CSMOE_SEL_SIGMOID_NORM
(`smoe_sigmoidgating` / `smoe_sigmoid`) beside its softmax rule at the same shape, in the run-time and the specialised instantiation.
usage (GPU box): python tools/router_bench.py [linear|cosine|perturbed|sigmoid|all] [rounds [iters]]   (rounds / iters: not `linear`)

What the event times are: every candidate is called through its Python entry, which allocates its outputs (five to seven
torch.empty) and launches; the torch-op gate is about a dozen eager launches per call.  The figures are therefore the cost of a
call as a layer pays it -- GPU time plus whatever of the host's dispatch the GPU cannot hide -- not kernel durations.  For those,
run the same command under a kernel trace with statistics, in a run of its own, and read the per-kernel averages."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from competesmoe_amd import ops, _lib as L  # noqa: E402


def timed(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def cosine(rounds=3, iters=500):
    """T = 32 768, D = 4096, E = 64, K = 2, bf16, the flags of the pretrain stack under bf16 autocast.  The candidates alternate
    inside every round, so that a drift of the machine shows up as spread between rounds rather than as a difference."""
    from competesmoe_amd.functional import cosine_route_unfused
    dev = "cuda"
    T, D, E, K = 32768, 4096, 64, 2
    flags = L.COS_OPER_BF16
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(T, D, device=dev, generator=g).to(torch.bfloat16)
    wr = (torch.randn(E // 2, D, device=dev, generator=g) * D ** -0.5).to(torch.bfloat16)
    wg = (torch.randn(E, D, device=dev, generator=g) * D ** -0.5).to(torch.bfloat16)
    emb = torch.randn(E, E // 2, device=dev, generator=g)
    emb = (emb * (1.5 / emb.norm(dim=-1, keepdim=True))).contiguous()
    red, lg, p, idx, w, _ = ops.cosine_select(x, wr, emb, K, flags)
    dw, dp = torch.randn(T, K, device=dev, generator=g), torch.randn(T, E, device=dev, generator=g)
    dl = torch.randn(T, E, device=dev, generator=g).to(torch.bfloat16)
    cands = {
        "cosine_select (one pass + patch launch)": lambda: ops.cosine_select(x, wr, emb, K, flags),
        "torch-op gate (GateLogits + normalize + matmul + make_finite + router_select)":
            lambda: cosine_route_unfused(x, wr, None, emb, K, flags),
        "gate_select (linear router, same T and D)": lambda: ops.gate_select(x, wg, K, L.SEL_SOFTMAX, True),
        "cosine_select_bwd (row kernel + d_emb sum)": lambda: ops.cosine_select_bwd(red, emb, lg, idx, w, dw, dp, dl, K, flags),
    }
    gb = T * D * 2 / 1e9
    times = {k: [] for k in cands}
    with torch.no_grad():
        for _ in range(rounds):
            for k, fn in cands.items():
                times[k].append(timed(fn, iters))
    for k, v in times.items():
        rate = f" ({gb / min(v) * 1e6:.0f} GB/s of x at the best round)" if "bwd" not in k else ""
        print(f"T={T} D={D} E={E} K={K} {k}: " + " / ".join(f"{t:.1f}" for t in v) + f" us{rate}", flush=True)


def perturbed(rounds=3, iters=500):
    """The shape and the method of `cosine`.  Flag sets 27 (the LLaVA bf16 module) and 12 (the pretrain stack under bf16 autocast)
    of the perturbed normalisation, theta = 0.1; the XMoE launch of the same build (flags 4) reads the same bytes and is the
    yardstick inside the run."""
    from competesmoe_amd.functional import cosine_route_unfused
    dev = "cuda"
    T, D, E, K = 32768, 4096, 64, 2
    theta = 0.1
    f_llava = L.TEMP_P_BF16 | L.TEMP_W_BF16 | L.COS_NORM_THETA | L.COS_NORM_BF16
    f_pre = L.COS_OPER_BF16 | L.COS_NORM_THETA
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(T, D, device=dev, generator=g).to(torch.bfloat16)
    wr = (torch.randn(E // 2, D, device=dev, generator=g) * D ** -0.5).to(torch.bfloat16)
    emb = torch.randn(E, E // 2, device=dev, generator=g)
    emb = (emb * (1.5 / (emb.norm(dim=-1, keepdim=True) + theta))).contiguous()
    dw, dp = torch.randn(T, K, device=dev, generator=g), torch.randn(T, E, device=dev, generator=g)
    dl = torch.randn(T, E, device=dev, generator=g).to(torch.bfloat16)
    saved = {f: ops.cosine_select(x, wr, emb, K, f, 0.3, theta if f & L.COS_NORM_THETA else 1e-4) for f in (f_llava, f_pre, L.COS_OPER_BF16)}

    def bwd(f, eps):
        red, lg, _, idx, w, _ = saved[f]
        return lambda: ops.cosine_select_bwd(red, emb, lg, idx, w, dw, dp, dl, K, f, 0.3, eps)
    cands = {
        f"cosine_select NORM_THETA flags {f_llava} (LLaVA bf16 module)": lambda: ops.cosine_select(x, wr, emb, K, f_llava, 0.3, theta),
        f"cosine_select NORM_THETA flags {f_pre} (pretrain, bf16 autocast)": lambda: ops.cosine_select(x, wr, emb, K, f_pre, 0.3, theta),
        "cosine_select xmoe flags 4 (same build)": lambda: ops.cosine_select(x, wr, emb, K, L.COS_OPER_BF16),
        f"torch-op gate NORM_THETA flags {f_pre} (GateLogits + norm + div + matmul + make_finite + router_select)":
            lambda: cosine_route_unfused(x, wr, None, emb, K, f_pre, 0.3, theta),
        f"cosine_select_bwd NORM_THETA flags {f_llava}": bwd(f_llava, theta),
        f"cosine_select_bwd NORM_THETA flags {f_pre}": bwd(f_pre, theta),
        "cosine_select_bwd xmoe flags 4 (same build)": bwd(L.COS_OPER_BF16, 1e-4),
    }
    gb = T * D * 2 / 1e9
    times = {k: [] for k in cands}
    with torch.no_grad():
        for _ in range(rounds):
            for k, fn in cands.items():
                times[k].append(timed(fn, iters))
    for k, v in times.items():
        rate = f" ({gb / min(v) * 1e6:.0f} GB/s of x at the best round)" if "bwd" not in k else ""
        print(f"T={T} D={D} E={E} K={K} {k}: " + " / ".join(f"{t:.1f}" for t in v) + f" us{rate}", flush=True)


def sigmoid(rounds=3, iters=500):
    """The shape and the method of `cosine`.  csmoe_gate_select with SEL_SIGMOID_NORM, `round_sum_bf16` 1 (a bf16 module: bf16
    quotient) and 0 (bf16 autocast on an fp32 stream), beside SEL_SOFTMAX in the same run-time instantiation (`round_sum_bf16` 0 keeps
    K = 2 out of the specialised kernel) and in the specialised one: all four read the same bytes.  The spread between the rounds of
    the run-time softmax line is the yardstick for the two sigmoid lines.  Then the selection backward of both rules."""
    dev = "cuda"
    T, D, E, K = 32768, 4096, 64, 2
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(T, D, device=dev, generator=g).to(torch.bfloat16)
    wg = (torch.randn(E, D, device=dev, generator=g) * D ** -0.5).to(torch.bfloat16)
    dw, dsm = torch.randn(T, K, device=dev, generator=g), torch.randn(T, E, device=dev, generator=g)
    saved = {m: ops.gate_select(x, wg, K, m, True) for m in (L.SEL_SIGMOID_NORM, L.SEL_SOFTMAX)}

    def bwd(m):
        lg, sm, idx, w = saved[m]
        return lambda: ops.router_select_bwd(lg, K, m, True, sm, idx, w, dw, dsm)
    cands = {
        "gate_select SEL_SIGMOID_NORM round_sum_bf16=1 (run-time instantiation)": lambda: ops.gate_select(x, wg, K, L.SEL_SIGMOID_NORM, True),
        "gate_select SEL_SIGMOID_NORM round_sum_bf16=0 (run-time instantiation)": lambda: ops.gate_select(x, wg, K, L.SEL_SIGMOID_NORM, False),
        "gate_select SEL_SOFTMAX round_sum_bf16=0 (run-time instantiation)": lambda: ops.gate_select(x, wg, K, L.SEL_SOFTMAX, False),
        "gate_select SEL_SOFTMAX round_sum_bf16=1 (specialised kernel)": lambda: ops.gate_select(x, wg, K, L.SEL_SOFTMAX, True),
        "router_select_bwd SEL_SIGMOID_NORM": bwd(L.SEL_SIGMOID_NORM),
        "router_select_bwd SEL_SOFTMAX": bwd(L.SEL_SOFTMAX),
    }
    gb = T * D * 2 / 1e9
    times = {k: [] for k in cands}
    with torch.no_grad():
        for _ in range(rounds):
            for k, fn in cands.items():
                times[k].append(timed(fn, iters))
    for k, v in times.items():
        rate = f" ({gb / min(v) * 1e6:.0f} GB/s of x at the best round)" if "bwd" not in k else ""
        print(f"T={T} D={D} E={E} K={K} {k}: " + " / ".join(f"{t:.1f}" for t in v) + f" us{rate}", flush=True)


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("cosine", "all"):
        cosine(*(int(a) for a in sys.argv[2:4]))
    if which in ("perturbed", "all"):
        perturbed(*(int(a) for a in sys.argv[2:4]))
    if which in ("sigmoid", "all"):
        sigmoid(*(int(a) for a in sys.argv[2:4]))
    if which in ("cosine", "perturbed", "sigmoid"):
        return
    dev = "cuda"
    for T, D, E, K in ((32768, 4096, 64, 2), (32768, 4096, 64, 8), (32768, 1024, 64, 2), (32768, 4096, 16, 2), (12800, 1152, 4, 2)):
        x = torch.randn(T, D, device=dev).to(torch.bfloat16)
        wg = (torch.randn(E, D, device=dev) * D ** -0.5).to(torch.bfloat16)
        t_f = timed(lambda: ops.gate_select(x, wg, K, L.SEL_SOFTMAX, True))
        t_g = timed(lambda: ops.gate_logits(x, wg))
        lg = ops.gate_logits(x, wg)
        t_s = timed(lambda: ops.router_select(lg, K, L.SEL_SOFTMAX, True))
        _, idx, _ = ops.router_select(lg, K, L.SEL_SOFTMAX, True)
        t_b = timed(lambda: ops.bin_tokens(idx.clone(), E))
        _, _, idx2, _ = ops.gate_select(x, wg, K, L.SEL_SOFTMAX, True)
        t_bh = timed(lambda: ops.bin_tokens(idx2, E))
        gb = T * D * 2 / 1e9
        print(f"T={T} D={D} E={E} K={K}: fused {t_f:.1f} us ({gb / t_f * 1e6:.0f} GB/s) + bins-from-hist {t_bh:.1f} us | "
              f"gate {t_g:.1f} us ({gb / t_g * 1e6:.0f} GB/s) + select {t_s:.1f} us + bins (incl. a 256 KB clone) {t_b:.1f} us", flush=True)


if __name__ == "__main__":
    main()
