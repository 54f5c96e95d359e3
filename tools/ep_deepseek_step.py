#!/usr/bin/env python3
"""One layer forward + backward of the pretrain shared-expert layer, `deepseekv2_ep` at world 1 over RCCL against the single-GPU
`deepseekv2`, with bf16 experts (64 routed + 1 shared) and with fp8 experts (BASELINE config 5: 128 routed + 2 shared), at
T = 32 768, D = 4096, F = 11008 under bf16 autocast over fp32 masters.

A step is timed with events on the current stream; the median and the minimum of --steps after --warmup are printed, one JSON line
per (configuration, layer).  bench.py cannot run these layers, hence this tool.  At world 1 the exchange is a device copy: what the
shared expert hides of a real all-to-all cannot be seen here, only what the expert-parallel plumbing costs (self-copies, the regroup
passes, the host read of the plan).  A kernel trace of this tool (`rocprofv3 --kernel-trace -- python tools/ep_deepseek_step.py
--configs bf16 --layers deepseekv2_ep --chunks 2 ...`) shows that the shared expert's GEMMs are issued between the sends and the
first wait.

    python tools/ep_deepseek_step.py [--configs bf16,fp8] [--layers deepseekv2,deepseekv2_ep] [--tokens 32768] [--dmodel 4096]
                                     [--dff 11008] [--steps 5] [--warmup 2] [--chunks 1]"""
import argparse
import json
import os
import socket
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"bf16": dict(experts=64, shared=1, fp8=False), "fp8": dict(experts=128, shared=2, fp8=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="bf16,fp8")
    ap.add_argument("--layers", default="deepseekv2,deepseekv2_ep")
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--dmodel", type=int, default=4096)
    ap.add_argument("--dff", type=int, default=11008)
    ap.add_argument("--topk", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunks", type=int, default=1)
    ap.add_argument("--experts", type=int, default=0, help="override the configuration's routed expert count")
    a = ap.parse_args()

    import torch
    import torch.distributed as dist
    import torch.nn.functional as F
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
        T, D = a.tokens, a.dmodel
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(T // 2048 if T >= 2048 else 1, min(T, 2048), D, device=dev, generator=g)
        dy = torch.randn(x.shape, device=dev, generator=g)

        def run(cname, name):
            c = CONFIGS[cname]
            E = a.experts or c["experts"]
            args = types.SimpleNamespace(balance_loss_coef=0.01, n_shared_experts=c["shared"], test_only=False, fp8_experts=c["fp8"])
            kw = dict(chunks=a.chunks) if name.endswith("_ep") else {}
            torch.manual_seed(1)
            with torch.device(dev):
                lay = get_moe(name)(D, E, a.dff, n_heads=a.topk, activation=F.relu, log_interval=None, args=args, **kw).train()
            lay.regularization_present = True
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
            print(json.dumps({"config": cname, "layer": name, "tokens": T, "dmodel": D, "dff": a.dff, "experts": E,
                              "shared": c["shared"], "fp8": c["fp8"], "chunks": a.chunks if kw else None,
                              "ms_median": round(times[len(times) // 2], 3), "ms_min": round(times[0], 3), "steps": a.steps}),
                  flush=True)
            del lay, xin
            torch.cuda.empty_cache()

        for cname in a.configs.split(","):
            for name in a.layers.split(","):
                run(cname, name)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
