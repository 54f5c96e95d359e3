#!/usr/bin/env python3
"""Generate golden vectors for the perturbed-cosine router layers (`smoe_perturbed`) of BOTH stacks by RUNNING THE REFERENCE classes.

Build-container only (needs /root/reference).  Patterned on make_golden_xmoe.py, whose `Stages` recorder, reference importers
(make_golden_llava.py, make_golden_pretrain.py) and environment (ref_env.py) it uses.  Nothing of the reference is restated: every
stage is recorded by wrapping the reference's own methods (`inp_reduction`, `_make_finite`, `_keepTopk`) while its forward runs.

Every fixture holds: meta, the state BEFORE the forward, x, dy, the stages (`reduced`, `gate_logits`, `gate_softmax`,
`selected_experts`, `weights`), `expert_embeddings` AFTER the forward (the layer rescales the parameter in place), the output,
losses / regularisers, x.grad and every parameter gradient.  A fixture is only written for a seed (0..15, ascending) at which no row of
the reference's own run ties its K-th with its (K+1)-th key (`meta["tie_share"] == 0`).

The parameters the classes leave to the global generator or uninitialised are pinned from the fixture's generator: `inp_reduction.weight`
and `gate.weight` (LLaVA), `expert_embeddings` (pretrain: torch.empty upstream, as make_golden_pretrain.py pins it).

The older pretrain_smoe_perturbed_{fp32,bf16}.pt (make_golden_pretrain.py: tie rows, no stages) are other files and stay.

Usage:  python tests/golden/make_golden_perturbed.py [out_dir]   (writes {llava,pretrain}_smoe_perturbed_*.pt, default tests/golden)
"""
import contextlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_env  # noqa: E402  (sets TRITON_INTERPRET=1 before triton is imported)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import make_golden_llava as GL  # noqa: E402
import make_golden_pretrain as GP  # noqa: E402
from make_golden_xmoe import MAX_SEEDS, Stages  # noqa: E402

NAME = "smoe_perturbed"


def _llava_once(dtype, seed, B, N, D, Fh, E, K):
    get_moe, SiglipMLP = GL._import_reference()
    args = GL.make_args(moe_name=NAME)
    experts = GL.build_experts("seq_gelu", E, D, Fh, D, seed + 1, SiglipMLP)
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        layer = get_moe(NAME)(D, D, E, K, experts, args)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():      # the class leaves these two at nn.Linear's default draw from the global generator: pin them
        layer.inp_reduction.weight.copy_(torch.randn(layer.inp_reduction.weight.shape, generator=g) * D ** -0.5)
        layer.gate.weight.copy_(torch.randn(layer.gate.weight.shape, generator=g) * 0.02)
    layer = layer.to(dtype)
    layer.train()
    x = torch.randn(B, N, D, generator=g).to(dtype)
    dy = torch.randn(B, N, D, generator=g).to(dtype)
    fx = {"meta": dict(name=NAME, moe_name=NAME, dtype=str(dtype).replace("torch.", ""), B=B, N=N, D=D, F=Fh, Dout=D, E=E, K=K,
                       expert_kind="seq_gelu", seed=seed, theta=float(layer.theta), args=vars(args)),
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


def _pretrain_once(bf16, seed, B, N, D, Fh, E, K):
    get_moe = GP._import_reference()
    args = GP.make_args(moe_name=NAME)
    torch.manual_seed(seed)
    layer = get_moe(NAME)(D, E, Fh, n_heads=K, activation=F.relu, sel_bias=False, log_interval=None, args=args)
    layer.train()
    with torch.no_grad():       # torch.empty upstream (smoe_perturbed.py:100-104): pinned as make_golden_pretrain.py:58 pins it
        layer.expert_embeddings.copy_(torch.randn(layer.expert_embeddings.shape, generator=torch.Generator().manual_seed(seed + 9)))
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, N, D, generator=g)
    dy = torch.randn(B, N, D, generator=g)
    upcasts = {}
    fx = {"meta": dict(name=NAME, moe_name=NAME, bf16=bf16, B=B, N=N, D=D, E=E, F=Fh, K=K, bias=False, sel_bias=False,
                       competition=False, seed=seed, theta=float(layer.theta), args=vars(args), cvmm=ref_env.CVMM_META),
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
    out_dir = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE
    cwd = os.getcwd()
    shape = dict(B=2, N=64, D=64)
    for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        write(os.path.join(out_dir, f"llava_{NAME}_{tag}.pt"), lambda s: _llava_once(dt, s, Fh=64, E=8, K=2, **shape))
    write(os.path.join(out_dir, f"llava_{NAME}_e16_bf16.pt"), lambda s: _llava_once(torch.bfloat16, s, Fh=64, E=16, K=4, **shape))
    for bf16, tag in ((False, "fp32"), (True, "bf16")):
        write(os.path.join(out_dir, f"pretrain_{NAME}_stages_{tag}.pt"), lambda s: _pretrain_once(bf16, s, Fh=32, E=8, K=2, **shape))
    os.chdir(cwd)


if __name__ == "__main__":
    main()
