#!/usr/bin/env python3
"""Does a row's result in the single-GPU fp8 `deepseekv2` depend on where the row stands in its expert's range (a full 256-row tile of
`gg8f_kernel` or the thin remainder loop)?  Runs one fwd + bwd on T tokens and again on the same tokens in a permuted order, un-permutes,
and prints whether output and dx agree bit for bit, with the largest relative difference.  The expert-parallel fp8 layers
(`deepseekv2_ep` / `deepseekv3_ep`) deliver an expert's rows in another order than the single-GPU layer, so their bit-for-bit dx
contract rests on this.

    python tools/fp8_row_order_probe.py"""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.nn.functional as F
    from competesmoe_amd.pretrain import get_moe
    dev = torch.device("cuda", 0)
    for (B, N, D, Fh, E, K, ns, bias) in ((2, 1024, 256, 512, 8, 2, 2, False), (2, 1024, 256, 512, 8, 2, 1, True),
                                          (2, 96, 128, 256, 8, 2, 1, False)):
        torch.manual_seed(11)
        args = types.SimpleNamespace(balance_loss_coef=0.01, n_shared_experts=ns, test_only=False, fp8_experts=True)
        lay = get_moe("deepseekv2")(D, E, Fh, n_heads=K, activation=F.relu, bias=bias, log_interval=None, args=args).to(dev).train()
        lay.regularization_present = True
        g = torch.Generator().manual_seed(70)
        x = torch.randn(B, N, D, generator=g).to(dev)
        dy = torch.randn(B, N, D, generator=g).to(dev)
        perm = torch.randperm(B * N, generator=g).to(dev)

        def run(xin, dyin):
            xin = xin.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = lay(xin, id_layer=0)
            lay.get_reg_loss()
            out.backward(dyin.to(out.dtype))
            return out.detach(), xin.grad.detach()

        oa, ga = run(x, dy)
        ob, gb = run(x.view(-1, D)[perm].view(B, N, D), dy.view(-1, D)[perm].view(B, N, D))
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(B * N, device=dev)
        ob, gb = ob.view(-1, D)[inv].view(B, N, D), gb.view(-1, D)[inv].view(B, N, D)
        worst = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max())
        print(f"T={B * N} D={D} F={Fh} E={E} K={K} shared={ns} bias={bias}: out bit for bit {torch.equal(oa, ob)} (largest relative "
              f"difference {worst(ob, oa):.3e}), dx bit for bit {torch.equal(ga, gb)} ({worst(gb, ga):.3e})", flush=True)


if __name__ == "__main__":
    main()
