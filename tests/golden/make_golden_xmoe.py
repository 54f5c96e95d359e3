#!/usr/bin/env python3
"""Generate golden vectors for the XMoE cosine-router layers of BOTH stacks by RUNNING THE REFERENCE classes.

Build-container only (needs /root/reference).  The LLaVA class is imported as make_golden_llava.py does, the pretrain class through
tests/golden/ref_env.py (unmodified: its Triton interpreter, its CUDA-autocast-on-CPU policy), plus `layers.moe.xmoe`, which that
module's import list does not name.  Nothing of the reference is restated: every stage is recorded by wrapping the reference's own
methods (`inp_reduction`, `_make_finite`, `_keepTopk`) while its forward runs.

Every fixture holds: meta, the state BEFORE the forward, x, dy, the stages (`reduced`, `gate_logits`, `gate_softmax`,
`selected_experts`, `weights`), `expert_embeddings` AFTER the forward (the layer renormalises the parameter in place), the output,
losses / regularisers, x.grad and every parameter gradient.

torch.topk's pick among equal keys is unspecified, so a fixture is only written for a seed at which NO row of the reference's own
run has its K-th and (K+1)-th key equal (`meta["tie_share"] == 0`, asserted); seeds are tried in ascending order.

Usage:  python tests/golden/make_golden_xmoe.py   (writes tests/golden/{llava,pretrain}_xmoe_*.pt)
"""
import contextlib
import importlib
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_env  # noqa: E402  (sets TRITON_INTERPRET=1 before triton is imported)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import make_golden_llava as GL  # noqa: E402
import make_golden_pretrain as GP  # noqa: E402

MAX_SEEDS = 16


class Stages:
    """Records what the reference's own router methods see and return during one forward."""

    def __init__(self, layer):
        self.rec = {}
        make_finite, keep_topk = layer._make_finite, layer._keepTopk

        def spy_finite(scores):
            out = make_finite(scores)
            self.rec["gate_logits"] = out.detach().clone()
            return out

        def spy_topk(p):
            w, idx = keep_topk(p)
            self.rec["gate_softmax"] = p.detach().clone()
            self.rec["weights"], self.rec["selected_experts"] = w.detach().clone(), idx.detach().clone()
            return w, idx
        layer._make_finite, layer._keepTopk = spy_finite, spy_topk
        red = layer.inp_reduction
        if isinstance(red, nn.Module):
            red.register_forward_hook(lambda m, a, out: self.rec.__setitem__("reduced", out.detach().clone()))
        else:
            def spy_red(x):
                out = red(x)
                self.rec["reduced"] = out.detach().clone()
                return out
            layer.inp_reduction = spy_red

    def tie_share(self, K):
        p = self.rec["gate_softmax"].float()
        top = p.topk(K + 1, dim=-1).values
        return float((top[..., K - 1] == top[..., K]).float().mean())


def _llava_once(dtype, seed, B, N, D, Fh, E, K):
    get_moe, SiglipMLP = GL._import_reference()
    importlib.import_module("moe_model.model.moe.xmoe")
    args = GL.make_args(moe_name="xmoe")
    experts = GL.build_experts("seq_gelu", E, D, Fh, D, seed + 1, SiglipMLP)
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        layer = get_moe("xmoe")(D, D, E, K, experts, args)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():      # the class leaves these two at nn.Linear's default draw from the global generator: pin them
        layer.inp_reduction.weight.copy_(torch.randn(layer.inp_reduction.weight.shape, generator=g) * D ** -0.5)
        layer.gate.weight.copy_(torch.randn(layer.gate.weight.shape, generator=g) * 0.02)
        layer.gate.bias.zero_()
    layer = layer.to(dtype)
    layer.train()
    x = torch.randn(B, N, D, generator=g).to(dtype)
    dy = torch.randn(B, N, D, generator=g).to(dtype)
    fx = {"meta": dict(name="xmoe", moe_name="xmoe", dtype=str(dtype).replace("torch.", ""), B=B, N=N, D=D, F=Fh, Dout=D, E=E, K=K,
                       expert_kind="seq_gelu", seed=seed, args=vars(args)),
          "state": {k: v.clone() for k, v in layer.state_dict().items()}, "x": x.clone(), "dy": dy.clone()}
    st = Stages(layer)
    xg = x.clone().requires_grad_(True)
    out, aux, _none, infor = layer(xg)
    fx.update(st.rec)
    fx["expert_embeddings_after"] = layer.expert_embeddings.detach().clone()
    fx["output"], fx["aux_loss"] = out.detach().clone(), aux.detach().clone()
    fx["infor_aux"] = {k: v.detach().clone() for k, v in infor.items()}
    ((out.float() * dy.float()).sum() + aux.float()).backward()
    fx["x_grad"] = xg.grad.clone()
    fx["grads"] = {k: (p.grad.clone() if p.grad is not None else None) for k, p in layer.named_parameters()}
    return fx, st.tie_share(K)


def _pretrain_once(bf16, sel_bias, seed, B, N, D, Fh, E, K):
    get_moe = GP._import_reference()
    importlib.import_module("layers.moe.xmoe")
    args = GP.make_args(moe_name="xmoe")
    torch.manual_seed(seed)
    layer = get_moe("xmoe")(D, E, Fh, n_heads=K, activation=F.relu, sel_bias=sel_bias, log_interval=None, args=args)
    layer.train()
    g = torch.Generator().manual_seed(seed + 1)
    if sel_bias:
        with torch.no_grad():
            layer.sel_bias.copy_(torch.randn(layer.sel_bias.shape, generator=g) * 0.1)
    x = torch.randn(B, N, D, generator=g)
    dy = torch.randn(B, N, D, generator=g)
    upcasts = {}
    fx = {"meta": dict(name="xmoe", moe_name="xmoe", bf16=bf16, B=B, N=N, D=D, E=E, F=Fh, K=K, bias=False, sel_bias=sel_bias,
                       competition=False, seed=seed, args=vars(args), cvmm=ref_env.CVMM_META),
          "state": {k: v.clone() for k, v in layer.state_dict().items()}, "x": x.clone(), "dy": dy.clone()}
    st = Stages(layer)
    xg = x.clone().requires_grad_(True)
    layer.regularization_present = True
    with GP.amp(bf16, upcasts):
        out = layer(xg)
        reg = layer.get_reg_loss()
    fx.update(st.rec)
    fx["expert_embeddings_after"] = layer.expert_embeddings.detach().clone()
    fx["output"] = out.detach().clone()
    fx["reg_loss"] = {k: v.detach().clone() for k, v in reg.items()}
    ((out.float() * dy).sum() + sum(v.float() for v in reg.values())).backward()
    fx["x_grad"] = xg.grad.clone()
    fx["grads"] = {k: (p.grad.clone() if p.grad is not None else None) for k, p in layer.named_parameters()}
    fx["meta"]["autocast_fp32_upcasts"] = dict(upcasts)
    return fx, st.tie_share(K)


def write(path, once):
    for seed in range(MAX_SEEDS):
        fx, share = once(seed)
        if share == 0.0:
            break
    assert share == 0.0, f"{path}: no seed below {MAX_SEEDS} without a tie between the K-th and (K+1)-th key"
    fx["meta"]["tie_share"] = share
    torch.save(fx, path)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB | seed", fx["meta"]["seed"], "| tie share", share)


def main():
    torch.set_num_threads(4)
    cwd = os.getcwd()
    shape = dict(B=2, N=64, D=64, E=8, K=2)
    for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        write(os.path.join(HERE, f"llava_xmoe_{tag}.pt"), lambda s: _llava_once(dt, s, Fh=64, **shape))
    for bf16, tag in ((False, "fp32"), (True, "bf16")):
        write(os.path.join(HERE, f"pretrain_xmoe_{tag}.pt"), lambda s: _pretrain_once(bf16, False, s, Fh=32, **shape))
    write(os.path.join(HERE, "pretrain_xmoe_selbias_fp32.pt"), lambda s: _pretrain_once(False, True, s, Fh=32, **shape))
    os.chdir(cwd)


if __name__ == "__main__":
    main()
