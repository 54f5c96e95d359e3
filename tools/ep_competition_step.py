#!/usr/bin/env python3
"""Router and competition steps of the pretrain CompeteSMoE layer, `competesmoe_ep` at world 1 over RCCL against the single-GPU
`competesmoe` (CSMOE_COMPETITION_LEAN=1), and the dX chain of the expert-parallel competition backward with the EPI_ACCUM epilogue
against GEMM + add_ (CSMOE_COMP_DX_ACCUM=1 / 0; the tool flips the module-level switch between runs).

A step = forward + backward of one layer under bf16 autocast over fp32 masters (the stack's training configuration), timed with
events on the current stream, median of --steps after --warmup.  bench.py refuses pretrain competition steps, hence this tool.
`--experts 8 --tokens 32768` is one rank's share of an 8-rank run of 64 experts at 4096 tokens per rank (8 local experts over the
gathered rows) -- without the exchanges, which a one-GPU box cannot time.  Larger shares stop at the fp32-master GEMMs' 2 GiB operand
bound (`csmoe_grouped_gemm_f32w`: T * K * F * 2 bytes of activations) on the router step, in both layers.

    python tools/ep_competition_step.py [--tokens 32768] [--dmodel 4096] [--dff 11008] [--experts 64] [--steps 5] [--warmup 2]
Prints one JSON line per configuration."""
import argparse
import json
import os
import socket
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["CSMOE_COMPETITION_LEAN"] = "1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--dmodel", type=int, default=4096)
    ap.add_argument("--dff", type=int, default=11008)
    ap.add_argument("--experts", type=int, default=64)
    ap.add_argument("--topk", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", default="competesmoe,competesmoe_ep")
    a = ap.parse_args()

    import torch
    import torch.distributed as dist
    import torch.nn.functional as F
    from competesmoe_amd import ep
    from competesmoe_amd.pretrain import get_moe

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(s.getsockname()[1]))
    s.close()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        args = types.SimpleNamespace(stop_after=10, warm_up=0.0, rate_flip=1.0, max_compete_in_iter=8, balance_loss_coef=0.01,
                                     balance_loss_coef_comp=0.02, router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False,
                                     tribrid=False, balance_affinity=False)
        T, D = a.tokens, a.dmodel
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(T // 2048 if T >= 2048 else 1, min(T, 2048), D, device=dev, generator=g)
        dy = torch.randn(x.shape, device=dev, generator=g)

        def run(name, comp, accum=None):
            torch.manual_seed(1)
            lay = get_moe(name)(D, a.experts, a.dff, n_heads=a.topk, activation=F.relu, log_interval=None, args=args).to(dev).train()
            lay.regularization_present = True
            lay.step_warm, lay.flip_steps = 0, 2
            lay.prob_flips_final = {0: torch.tensor([False, True], device=dev)}
            lay.set_current_steps(1 if comp else 0)
            if accum is not None:
                ep._COMP_DX_ACCUM = accum
            xin = x.clone().requires_grad_(True)
            times = []
            for i in range(a.warmup + a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    out = lay(xin, id_layer=0)
                    reg = sum(lay.get_reg_loss().values())
                torch.autograd.backward([out, reg.float()], [dy.to(out.dtype), torch.ones((), device=dev)])
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times.append(e0.elapsed_time(e1))
                lay.zero_grad(set_to_none=True)
                xin.grad = None
            times.sort()
            print(json.dumps({"layer": name, "step": "competition" if comp else "router", "comp_dx_accum": accum, "tokens": T,
                              "dmodel": D, "dff": a.dff, "experts": a.experts, "ms_median": round(times[len(times) // 2], 3),
                              "ms_min": round(times[0], 3), "steps": a.steps}), flush=True)
            del lay
            torch.cuda.empty_cache()

        for name in a.layers.split(","):
            run(name, False)
            if name == "competesmoe_ep":
                run(name, True, accum=False)
                run(name, True, accum=True)
            else:
                run(name, True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
