"""Test-side restatement of the XMoE cosine router in plain torch ops (CPU or GPU tensors), pinned to the reference by
tests/test_xmoe_cpu.py: fed a fixture's inputs it reproduces every recorded stage (fp32 to 1e-6, bf16 bit for bit).

The rounding points are flags, as in the kernels (include/csmoe.h): P_BF16 -- p is cast to bf16 before the top-K; W_BF16 -- the softmax
over the K values is a bf16 tensor op; OPER_BF16 -- the cosine product runs on bf16 operands (matmul under bf16 autocast).
Selection: K rounds of arg-max, lowest index on ties (the project's tie rule); `forced_idx` evaluates the weights (and with them the
gradients) for given indices.  The expert FFNs and the losses come from the pinned oracle (oracle/moe_oracle.py)."""
import torch
import torch.nn.functional as F

from oracle import moe_oracle as O

P_BF16, W_BF16, OPER_BF16 = 1, 2, 4
TEMPERATURE, EPS = 0.3, 1e-4


def renorm(emb):
    """The in-place rescale of the parameter to row norm 1.5, in the parameter's dtype."""
    return emb * (1.5 / emb.norm(p=2.0, dim=-1, keepdim=True))


def make_finite(scores):
    ok = scores.isfinite()
    low = torch.where(ok, scores, torch.full_like(scores, float("inf"))).min()
    return torch.where(ok, scores, low.detach())       # the assigned entries carry no gradient in this restatement


def cosine(reduced, emb, flags, eps=EPS):
    v = reduced.float()
    m = v / v.norm(2.0, -1, keepdim=True).clamp_min(eps).expand_as(v)
    if flags & OPER_BF16:
        return torch.matmul(m.to(torch.bfloat16), emb.float().transpose(0, 1).to(torch.bfloat16))
    return torch.matmul(m, emb.float().transpose(0, 1)).type_as(reduced)


def select(cos, K, flags, temperature=TEMPERATURE, forced_idx=None):
    """(p, idx, w): p in bf16 under P_BF16 else fp32; w in p's dtype (bf16 only under W_BF16)."""
    p = F.softmax((cos / temperature).float(), dim=-1)
    if flags & P_BF16:
        p = p.to(torch.bfloat16)
    idx = O.topk_lowest_index(p.detach(), K)[1] if forced_idx is None else forced_idx.long()
    vals = torch.gather(p, -1, idx)
    if not flags & W_BF16:
        vals = vals.float()
    return p, idx, torch.softmax(vals, dim=-1)


def row_half(reduced, emb, K, flags, forced_idx=None):
    """reduced [.., R] -> (cos, p, idx, w): everything the row half of the one-pass kernel computes."""
    cos = make_finite(cosine(reduced, emb, flags))
    p, idx, w = select(cos, K, flags, forced_idx=forced_idx)
    return cos, p, idx, w


def router(x_op, sel_w, sel_bias, emb, K, flags, forced_idx=None):
    """x in the operand dtype, reduction matrix / bias, RENORMALISED embeddings -> (reduced, cos, p, idx, w)."""
    reduced = F.linear(x_op, sel_w.to(x_op.dtype), None if sel_bias is None else sel_bias.to(x_op.dtype))
    return (reduced,) + row_half(reduced, emb, K, flags, forced_idx)


def llava_flags(dtype):
    return (P_BF16 | W_BF16) if dtype == torch.bfloat16 else 0


def pretrain_flags(bf16_autocast):
    return OPER_BF16 if bf16_autocast else 0


def llava_forward(x, params, meta, forced_idx=None):
    """The LLaVA layer: `params` name -> tensor (state-dict names, `expert_embeddings` already renormalised).
    Returns (out, aux, stages dict)."""
    E, K = meta["E"], meta["K"]
    flags = llava_flags(x.dtype)
    reduced, cos, p, idx, w = router(x, params["inp_reduction.weight"], None, params["expert_embeddings"], K, flags, forced_idx)
    experts = [tuple(params[f"experts.{i}.{j}"] for j in ("0.weight", "0.bias", "2.weight", "2.bias")) for i in range(E)]
    out = O.compute_moe(x, idx, w, experts, "gelu", meta["Dout"])
    a = meta["args"]
    aux, bal, z = O.combine_loss(idx, p, cos, E, a["balance_loss_coef"], a["router_z_loss_coef"])
    return out, aux, dict(reduced=reduced, gate_logits=cos, gate_softmax=p, selected_experts=idx, weights=w, balance_loss=bal,
                          router_z_loss=z)


def pretrain_forward(x, params, meta, forced_idx=None):
    """The pretrain layer (fp32 stream; bf16 operands under autocast when meta["bf16"]).  Returns (out, reg, stages dict)."""
    K = meta["K"]
    op = torch.bfloat16 if meta["bf16"] else torch.float32
    flags = pretrain_flags(meta["bf16"])
    reduced, cos, p, idx, w = router(x.to(op), params["expert_sel"], params.get("sel_bias"), params["expert_embeddings"], K, flags,
                                     forced_idx)
    out = O.pretrain_ffn(x, idx, w, params["keys"], params["values"], "relu", op)
    reg = O.entropy_balance(cos) * meta["args"]["balance_loss_coef"]
    return out, reg, dict(reduced=reduced, gate_logits=cos, gate_softmax=p, selected_experts=idx, weights=w)
