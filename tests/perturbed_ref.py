"""Test-side restatement of the perturbed-cosine router (`smoe_perturbed`) in plain torch ops (CPU or GPU tensors), pinned to the
reference by tests/test_perturbed_cpu.py: fed a fixture's inputs it reproduces every recorded stage (fp32 to 1e-6, bf16 bit for bit).

It is tests/xmoe_ref.py's router (`select`, `make_finite`, the expert FFNs and losses of the pinned oracle) with another cosine
stage: the row is divided by norm + theta, no clamp.  Two more rounding points are flags, as in the kernels (include/csmoe.h):
NORM_THETA -- this normalisation; NORM_BF16 -- the norm and `norm + theta` are tensors of the row's own dtype (a bf16 module without
autocast), else the norm is taken in fp32 (under bf16 autocast `norm` is an fp32-policy op).  The ops are the reference's (`norm`,
`+ theta`, an fp32 division), so autograd rounds where the reference's does: `reduced` is used twice -- the `.float()` cast and
the norm -- and receives the sum of two gradients in its own dtype."""
import torch
import torch.nn.functional as F

from oracle import moe_oracle as O
from tests.xmoe_ref import OPER_BF16, P_BF16, W_BF16, TEMPERATURE, make_finite, select  # noqa: F401

NORM_THETA, NORM_BF16 = 8, 16
THETA = 0.1


def renorm(emb, theta=THETA):
    """The in-place rescale of the parameter by 1.5 / (row norm + theta), in the parameter's dtype."""
    return emb * (1.5 / (emb.norm(p=2.0, dim=-1, keepdim=True) + theta))


def cosine(reduced, emb, flags, theta=THETA):
    assert flags & NORM_THETA
    nrm = (reduced if flags & NORM_BF16 else reduced.float()).norm(p=2, dim=-1, keepdim=True)
    m = reduced.float() / (nrm + theta)
    if flags & OPER_BF16:
        return torch.matmul(m.to(torch.bfloat16), emb.float().transpose(0, 1).to(torch.bfloat16)).type_as(reduced)
    return torch.matmul(m, emb.float().transpose(0, 1)).type_as(reduced)


def row_half(reduced, emb, K, flags, theta=THETA, forced_idx=None):
    """reduced [.., R] -> (cos, p, idx, w): everything the row half of the one-pass kernel computes."""
    cos = make_finite(cosine(reduced, emb, flags, theta))
    p, idx, w = select(cos, K, flags, forced_idx=forced_idx)
    return cos, p, idx, w


def router(x_op, sel_w, sel_bias, emb, K, flags, theta=THETA, forced_idx=None):
    """x in the operand dtype, reduction matrix / bias, RENORMALISED embeddings -> (reduced, cos, p, idx, w)."""
    reduced = F.linear(x_op, sel_w.to(x_op.dtype), None if sel_bias is None else sel_bias.to(x_op.dtype))
    return (reduced,) + row_half(reduced, emb, K, flags, theta, forced_idx)


def llava_flags(dtype):
    return (P_BF16 | W_BF16 | NORM_THETA | NORM_BF16) if dtype == torch.bfloat16 else NORM_THETA


def pretrain_flags(bf16_autocast):
    return (OPER_BF16 | NORM_THETA) if bf16_autocast else NORM_THETA


def llava_forward(x, params, meta, forced_idx=None):
    """The LLaVA layer: `params` name -> tensor (state-dict names, `expert_embeddings` already renormalised).
    Returns (out, aux, stages dict)."""
    E, K = meta["E"], meta["K"]
    reduced, cos, p, idx, w = router(x, params["inp_reduction.weight"], None, params["expert_embeddings"], K, llava_flags(x.dtype),
                                     meta.get("theta", THETA), forced_idx)
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
    reduced, cos, p, idx, w = router(x.to(op), params["expert_sel"], params.get("sel_bias"), params["expert_embeddings"], K,
                                     pretrain_flags(meta["bf16"]), meta.get("theta", THETA), forced_idx)
    out = O.pretrain_ffn(x, idx, w, params["keys"], params["values"], "relu", op)
    reg = O.entropy_balance(cos) * meta["args"]["balance_loss_coef"]
    return out, reg, dict(reduced=reduced, gate_logits=cos, gate_softmax=p, selected_experts=idx, weights=w)
