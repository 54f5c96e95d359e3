#!/usr/bin/env python3
"""Generate golden vectors for the sigmoid-router layers (LLaVA `smoe_sigmoidgating`, pretrain `smoe_sigmoid`: MoEUT's sigmoid gate)
by RUNNING THE REFERENCE classes.

Build-container only (needs /root/reference).  Patterned on make_golden_perturbed.py: the reference importers (make_golden_llava.py,
make_golden_pretrain.py), the environment (ref_env.py; `layers.moe.smoeut_norm` is imported after it has built its stubs) and the
`Stages` recorder of make_golden_xmoe.py, here with the hooks these two classes offer.  Nothing of the reference is restated: every
stage is recorded by wrapping the reference's own modules and methods (`gate` / `compute_gate`, `sigmoid`, `topk_expert`,
`compute_moe`, the module's `cvmm`) while its forward runs.

Every fixture holds: meta, the state BEFORE the forward, x, dy, the stages (`gate_logits`, the keys `gate_sigmoid`, `gate_softmax`
(LLaVA), `selected_experts`, the renormalised `weights`), the output, losses / regularisers, x.grad and every parameter gradient.

A sigmoid in [0.5, 1) has 128 bf16 values, so bf16 keys tie at the top-K boundary in every draw and torch.topk has no tie rule:
meta["tie_rows"] records the share of rows with ANY equal pair among the reference's top K + 1 keys.  Seed policy: fp32 -- the first
seed of 0..15 with tie_rows == 0; bf16 with E = 8 -- the first with tie_rows <= 0.25; bf16 with E = 16, K = 4 -- seed 0 whatever its
share (it serves the value checks and the teacher-forced stages, not id equality).

Usage:  python tests/golden/make_golden_sigmoid.py [out_dir]   (writes llava_smoe_sigmoidgating_*.pt, pretrain_smoe_sigmoid_*.pt)
"""
import contextlib
import importlib
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

LLAVA, PRETRAIN = "smoe_sigmoidgating", "smoe_sigmoid"


class SigmoidStages(Stages):
    """The recorder for the two sigmoid-router classes: what their own gate, sigmoid, top-K and expert step see and return."""

    def __init__(self, layer, module=None):
        self.rec = {}
        rec = self.rec
        topk = layer.topk_expert

        def spy_topk(gate_logits):
            w, idx, third = topk(gate_logits=gate_logits)
            rec["gate_logits"] = gate_logits.detach().clone()
            rec["selected_experts"] = idx.detach().clone()
            if module is None:                     # LLaVA: (top-K keys, ids, fp32 softmax); the keys come from the nn.Sigmoid hook
                rec["gate_softmax"] = third.detach().clone()
            else:                                  # pretrain: (top-K keys, ids, keys)
                rec["gate_sigmoid"] = third.detach().clone()
            return w, idx, third
        layer.topk_expert = spy_topk
        if module is None:
            layer.sigmoid.register_forward_hook(lambda m, a, out: rec.__setitem__("gate_sigmoid", out.detach().clone()))
            compute_moe = layer.compute_moe

            def spy_moe(selected_experts, weights, *a, **k):
                rec["weights"] = weights.detach().clone()
                return compute_moe(selected_experts, weights, *a, **k)
            layer.compute_moe = spy_moe
        else:
            cvmm = module.cvmm

            def spy_cvmm(x, sel, w):
                if getattr(sel, "reduction_weight", None) is not None:
                    rec["weights"] = sel.reduction_weight.detach().clone()
                return cvmm(x, sel, w)
            module.cvmm = spy_cvmm
            self._restore = lambda: setattr(module, "cvmm", cvmm)

    def close(self):
        getattr(self, "_restore", lambda: None)()

    def tie_rows(self, K):
        keys = self.rec["gate_sigmoid"].float()
        top = keys.topk(K + 1, dim=-1).values
        return float((top[..., :-1] == top[..., 1:]).any(-1).float().mean())


def _llava_once(dtype, seed, B, N, D, Fh, E, K):
    get_moe, SiglipMLP = GL._import_reference()
    importlib.import_module("moe_model.model.moe.smoe_sigmoidgating")
    args = GL.make_args(moe_name=LLAVA)
    experts = GL.build_experts("seq_gelu", E, D, Fh, D, seed + 1, SiglipMLP)
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        layer = get_moe(LLAVA)(D, D, E, K, experts, args)       # the gate is drawn by init_gate_weights (generator seed 42)
    layer = layer.to(dtype)
    layer.train()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, D, generator=g).to(dtype)
    dy = torch.randn(B, N, D, generator=g).to(dtype)
    fx = {"meta": dict(name=LLAVA, moe_name=LLAVA, dtype=str(dtype).replace("torch.", ""), B=B, N=N, D=D, F=Fh, Dout=D, E=E, K=K,
                       expert_kind="seq_gelu", seed=seed, args=vars(args)),
          "state": {k: v.clone() for k, v in layer.state_dict().items()}, "x": x.clone(), "dy": dy.clone()}
    st = SigmoidStages(layer)
    xg = x.clone().requires_grad_(True)
    out, aux, _none, infor = layer(xg)
    fx.update(st.rec)
    fx["output"], fx["aux_loss"] = out.detach().clone(), aux.detach().clone()
    fx["infor_aux"] = {k: v.detach().clone() for k, v in infor.items()}
    ((out.float() * dy.float()).sum() + aux.float()).backward()
    fx["x_grad"] = xg.grad.clone()
    fx["grads"] = {k: (p.grad.clone() if p.grad is not None else None) for k, p in layer.named_parameters()}
    return fx, st.tie_rows(K)


def _pretrain_once(bf16, seed, B, N, D, Fh, E, K):
    get_moe = GP._import_reference()
    mod = importlib.import_module("layers.moe.smoeut_norm")
    args = GP.make_args(moe_name=PRETRAIN)
    torch.manual_seed(seed)
    layer = get_moe(PRETRAIN)(D, E, Fh, n_heads=K, activation=F.relu, sel_bias=False, log_interval=None, args=args)
    layer.train()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, N, D, generator=g)
    dy = torch.randn(B, N, D, generator=g)
    upcasts = {}
    fx = {"meta": dict(name=PRETRAIN, moe_name=PRETRAIN, bf16=bf16, B=B, N=N, D=D, E=E, F=Fh, K=K, bias=False, sel_bias=False,
                       competition=False, seed=seed, args=vars(args), cvmm=ref_env.CVMM_META),
          "state": {k: v.clone() for k, v in layer.state_dict().items()}, "x": x.clone(), "dy": dy.clone()}
    st = SigmoidStages(layer, mod)
    xg = x.clone().requires_grad_(True)
    layer.regularization_present = True
    try:
        with GP.amp(bf16, upcasts):
            out = layer(xg)
            reg = layer.get_reg_loss()
    finally:
        st.close()
    fx.update(st.rec)
    fx["output"] = out.detach().clone()
    fx["reg_loss"] = {k: v.detach().clone() for k, v in reg.items()}
    ((out.float() * dy).sum() + sum(v.float() for v in reg.values())).backward()
    fx["x_grad"] = xg.grad.clone()
    fx["grads"] = {k: (p.grad.clone() if p.grad is not None else None) for k, p in layer.named_parameters()}
    fx["meta"]["autocast_fp32_upcasts"] = dict(upcasts)
    return fx, st.tie_rows(K)


def write(path, once, limit, seeds=MAX_SEEDS):
    """The first seed below `seeds` whose share of tie rows is at most `limit` (None: the first seed, whatever its share)."""
    for seed in range(seeds):
        fx, share = once(seed)
        if limit is None or share <= limit:
            break
    assert limit is None or share <= limit, f"{path}: no seed below {seeds} with at most {limit} tie rows"
    fx["meta"]["tie_rows"] = share
    torch.save(fx, path)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB | seed", fx["meta"]["seed"], "| tie rows", share)


def main():
    torch.set_num_threads(4)
    out_dir = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE
    cwd = os.getcwd()
    shape = dict(B=2, N=64, D=64)
    for dt, tag, limit in ((torch.float32, "fp32", 0.0), (torch.bfloat16, "bf16", 0.25)):
        write(os.path.join(out_dir, f"llava_{LLAVA}_{tag}.pt"), lambda s: _llava_once(dt, s, Fh=64, E=8, K=2, **shape), limit)
    write(os.path.join(out_dir, f"llava_{LLAVA}_e16_bf16.pt"), lambda s: _llava_once(torch.bfloat16, s, Fh=64, E=16, K=4, **shape), None)
    for bf16, tag, limit in ((False, "fp32", 0.0), (True, "bf16", 0.25)):
        write(os.path.join(out_dir, f"pretrain_{PRETRAIN}_{tag}.pt"), lambda s: _pretrain_once(bf16, s, Fh=32, E=8, K=2, **shape), limit)
    os.chdir(cwd)


if __name__ == "__main__":
    main()
