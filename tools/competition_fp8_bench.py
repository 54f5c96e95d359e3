#!/usr/bin/env python3
"""Time one pretrain `competesmoe` layer, forward + backward, on a COMPETITION step in three forms:

    bf16_lean    bf16 experts, the lean form (CSMOE_COMPETITION_LEAN=1: CompetitionAffinityPacked + MoEFFNPackedSlots)
    fp8_stored   args.fp8_experts with args.fp8_competition off: E dense bf16 FFNs, their [T, E, D] outputs kept
    fp8_lean     args.fp8_experts + args.fp8_competition: CompetitionAffinityPackedFP8 + MoEFFNPackedFP8Slots

    tools/competition_fp8_bench.py [--sizes 8x8192,64x32768] [--d 4096] [--f 11008] [--k 2] [--warmup 1] [--repeats 5]

The three layers share one set of parameters and one input; after the warm-up they alternate in one process (a round runs each
form once), every step is timed with device events, and the median / min / max over the rounds and the peak allocated memory of
a step are printed per form, then one JSON line.  A size given as ExT! (a trailing `!`) leaves out fp8_stored, whose stored
activations do not fit at 64 experts x 32 768 tokens.  It needs a GPU: without one it fails."""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARGS = dict(moe_name="competesmoe", stop_after=10, warm_up=0.0, rate_flip=1.0, max_compete_in_iter=8, balance_loss_coef=0.01,
            balance_loss_coef_comp=0.02, router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False, tribrid=False,
            balance_affinity=False, is_cosine=False, is_norm_weight=False, norm_sigmoid=False, scale_weight=1.0, test_only=False)
FORMS = {"bf16_lean": dict(), "fp8_stored": dict(fp8_experts=True), "fp8_lean": dict(fp8_experts=True, fp8_competition=True)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="8x8192,64x32768!", help="experts x tokens, comma separated; a trailing ! leaves out fp8_stored")
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--f", type=int, default=11008)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        sys.exit("competition_fp8_bench: no GPU visible -- this tool measures on the device and has no fallback")
    from competesmoe_amd.pretrain import get_moe
    dev = "cuda"
    results = []
    for size in a.sizes.split(","):
        lean_only = size.endswith("!")
        E, T = (int(v) for v in size.rstrip("!").split("x"))
        forms = [f for f in FORMS if not (lean_only and f == "fp8_stored")]
        torch.manual_seed(0)
        layers = {}
        for name in forms:
            with torch.device(dev):
                lay = get_moe("competesmoe")(a.d, E, a.f, n_heads=a.k, activation=F.relu, log_interval=None,
                                             args=types.SimpleNamespace(**ARGS, **FORMS[name]))
            if layers:                                     # one set of parameters for all forms
                first = next(iter(layers.values()))
                lay.keys, lay.values, lay.w_gate = first.keys, first.values, first.w_gate
            lay.train()
            lay.regularization_present = True
            lay.step_warm, lay.flip_steps = 0, 10
            lay.prob_flips_final = {0: torch.ones(10, dtype=torch.bool, device=dev)}     # every step competes
            lay.set_current_steps(3)
            layers[name] = lay
        B = 8
        x = torch.randn(B, T // B, a.d, device=dev).requires_grad_(True)
        dy = torch.randn(B, T // B, a.d, device=dev).to(torch.bfloat16)
        one = torch.ones((), device=dev)
        base = torch.cuda.memory_allocated()

        def step(name):
            lay = layers[name]
            os.environ["CSMOE_COMPETITION_LEAN"] = "1" if name == "bf16_lean" else "auto"
            x.grad = None
            for p in lay.parameters():
                p.grad = None
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0.record()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = lay(x, id_layer=0)
                reg = sum(v.float() for v in lay.get_reg_loss().values())
            torch.autograd.backward([out, reg], [dy.view(out.shape), one])
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1), torch.cuda.max_memory_allocated()

        for _ in range(a.warmup):
            for name in forms:
                step(name)
        ms = {n: [] for n in forms}
        peak = {n: 0 for n in forms}
        for _ in range(a.repeats):
            for name in forms:
                t, m = step(name)
                ms[name].append(t)
                peak[name] = max(peak[name], m)
        print(f"# competition step, fwd + bwd: E={E} T={T} D={a.d} F={a.f} K={a.k}; {a.repeats} rounds after {a.warmup} warm-up; "
              f"parameters + inputs {base / 2 ** 30:.1f} GiB")
        row = {"E": E, "T": T, "D": a.d, "F": a.f, "K": a.k, "repeats": a.repeats, "base_gib": round(base / 2 ** 30, 2), "forms": {}}
        for name in forms:
            v = ms[name]
            med = statistics.median(v)
            print(f"{name:11s} median {med:9.2f} ms   min {min(v):9.2f}   max {max(v):9.2f}   spread {(max(v) - min(v)) / med:6.1%}   "
                  f"peak {peak[name] / 2 ** 30:7.1f} GiB")
            row["forms"][name] = {"median_ms": round(med, 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                                  "peak_gib": round(peak[name] / 2 ** 30, 2)}
        if "bf16_lean" in ms and "fp8_lean" in ms:
            print(f"fp8_lean / bf16_lean = {statistics.median(ms['fp8_lean']) / statistics.median(ms['bf16_lean']):.3f} (median over median)")
        results.append(row)
        del layers, x, dy
        from competesmoe_amd import functional as Fn
        Fn.fp8_weight_cache_clear()
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "competition_fp8_bench", "results": results}))


if __name__ == "__main__":
    main()
