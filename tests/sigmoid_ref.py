"""Test-side restatement of the sigmoid router (MoEUT's sigmoid gate: LLaVA `smoe_sigmoidgating`, pretrain `smoe_sigmoid`) in plain
torch ops (CPU or GPU tensors), stage by stage: logits, keys, selection with the project's tie rule, weights, output, losses, and
gradients through autograd.  Pinned to the fixtures captured from the reference classes by tests/test_sigmoid_cpu.py.

The reference's lines (moe_model/model/moe/smoe_sigmoidgating.py:33-42; moe_pretrain_model/layers/moe/smoeut_norm.py:112-125):
    keys = sigmoid(logits);  vals, idx = topk(keys, K);  w = vals / sum(vals, -1, keepdim=True).to(x.dtype)
`sum` is a tensor op of vals' dtype outside autocast and an fp32-policy op under CUDA autocast (`sum_fp32`), which is all that
separates the four ways the reference reaches the rule (include/csmoe.h, CSMOE_SEL_SIGMOID_NORM).  Selection: K rounds of arg-max,
lowest index on ties (the project's tie rule; torch.topk has none); `idx=` replaces it (teacher forcing), and every later stage --
weights, output, losses, gradients -- is then evaluated for those ids.  The expert FFNs and the losses come from the pinned oracle
(oracle/moe_oracle.py).

`select_bwd_emulation` restates the lines of router_select_bwd_kernel's SEL_SIGMOID_NORM branch (competesmoe_amd/csrc/
moe_kernels.hip) with torch ops, rounding where the kernel rounds."""
import torch
import torch.nn.functional as F

from oracle import moe_oracle as O

SEL_SIGMOID_NORM = 6


def select(logits, K, x_dtype, sum_fp32=False, idx=None):
    """logits [.., E] -> (keys, softmax fp32, idx, w).  `x_dtype`: what `.to(x.dtype)` casts the K-sum to; `sum_fp32`: the sum runs
    under CUDA autocast (input cast to fp32 first)."""
    sm = F.softmax(logits, dim=-1, dtype=torch.float32)
    keys = torch.sigmoid(logits)
    idx = O.topk_lowest_index(keys.detach(), K)[1] if idx is None else idx.long()
    vals = torch.gather(keys, -1, idx)
    s = torch.sum(vals.float() if sum_fp32 else vals, dim=-1, keepdim=True)
    return keys, sm, idx, vals / s.to(x_dtype)


def select_flags(scores_dtype, round_sum_bf16):
    """(x_dtype, sum_fp32) of the reference call that csmoe_router_select(scores, SEL_SIGMOID_NORM, round_sum_bf16) stands for."""
    if scores_dtype == torch.float32:
        return (torch.bfloat16 if round_sum_bf16 else torch.float32), False
    return (torch.bfloat16, False) if round_sum_bf16 else (torch.float32, True)


def llava_forward(x, params, meta, idx=None):
    """The LLaVA layer: `params` name -> tensor (state-dict names).  Returns (out, aux, stages dict)."""
    E, K = meta["E"], meta["K"]
    logits = F.linear(x, params["gate.weight"])
    keys, sm, idx, w = select(logits, K, x.dtype, idx=idx)
    experts = [tuple(params[f"experts.{i}.{j}"] for j in ("0.weight", "0.bias", "2.weight", "2.bias")) for i in range(E)]
    out = O.compute_moe(x, idx, w, experts, "gelu", meta["Dout"])
    a = meta["args"]
    aux, bal, z = O.combine_loss(idx, sm, logits, E, a["balance_loss_coef"], a["router_z_loss_coef"])
    return out, aux, dict(gate_logits=logits, gate_sigmoid=keys, gate_softmax=sm, selected_experts=idx, weights=w, balance_loss=bal,
                          router_z_loss=z)


def pretrain_forward(x, params, meta, idx=None, stream_bf16=False):
    """The pretrain layer: fp32 stream, bf16 operands under autocast when meta["bf16"]; `stream_bf16`: the layer is called with a
    bf16 x under that autocast (`.to(x.dtype)` then rounds the fp32 sum).  Returns (out, reg, stages dict)."""
    K = meta["K"]
    op = torch.bfloat16 if meta["bf16"] else torch.float32
    logits = F.linear(x.to(op), params["w_gate"].to(op))
    keys, _sm, idx, w = select(logits, K, torch.bfloat16 if stream_bf16 else x.dtype, sum_fp32=meta["bf16"], idx=idx)
    out = O.pretrain_ffn(x, idx, w, params["keys"], params["values"], "relu", op)
    reg = O.entropy_balance(logits) * meta["args"]["balance_loss_coef"]
    return out, reg, dict(gate_logits=logits, gate_sigmoid=keys, selected_experts=idx, weights=w)


def _r(t, dt):
    return t.to(dt).float()


def _wave_sum(t):
    """Row sums of t [T, E] in the order of the kernel's wave: lane l adds its elements l, l + 64, ... in turn, then the xor
    butterfly over 64 lanes (partners 32, 16, 8, 4, 2, 1)."""
    T, E = t.shape
    vpl = (E + 63) // 64
    pad = torch.zeros(T, vpl * 64, dtype=t.dtype, device=t.device)
    pad[:, :E] = t
    pad = pad.view(T, vpl, 64)
    s = torch.zeros(T, 64, dtype=t.dtype, device=t.device)
    for v in range(vpl):
        s = s + pad[:, v]
    lanes = torch.arange(64, device=t.device)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, :1]


def select_bwd_emulation(logits, sm, idx, dw, dsm, round_sum_bf16, wave_tree=False):
    """router_select_bwd_kernel, SEL_SIGMOID_NORM branch, line by line: logits [T, E] (fp32 or bf16), sm fp32 [T, E] or None,
    idx [T, K], dw fp32 [T, K], dsm fp32 [T, E] or None -> d logits [T, E] in logits.dtype.  fp32 arithmetic between the roundings,
    sums over K in slot order.  `wave_tree`: the row sum of the softmax path in the wave's own order (comparisons with the kernel;
    E <= 64) instead of torch's (comparisons with autograd)."""
    dt = logits.dtype
    bq = bool(round_sum_bf16) and dt == torch.bfloat16
    idx = idx.long()
    K = idx.shape[-1]
    v = torch.gather(torch.sigmoid(logits), -1, idx).float()          # the keys in the scores' dtype, widened

    def ksum(t):
        acc = torch.zeros_like(t[..., :1])
        for k in range(K):
            acc = acc + t[..., k:k + 1]
        return acc
    den = ksum(v)
    if round_sum_bf16:
        den = _r(den, torch.bfloat16)
    dw = dw.float()
    if bq:
        dwr = _r(dw, dt)
        q = _r(_r(v / den, dt) / den, dt)
        dd = _r(ksum(_r(-dwr * q, dt)), dt)
        dv = _r(_r(dwr / den, dt) + dd, dt)
    else:
        dd = ksum(-dw * ((v / den) / den))
        if round_sum_bf16:
            dd = _r(dd, torch.bfloat16)
        dv = _r(_r(dw / den, dt) + _r(dd, dt), dt)
    dz = _r((dv * (1.0 - v)) * v, dt)
    direct = torch.zeros(logits.shape, dtype=torch.float32, device=logits.device).scatter(-1, idx, dz)
    sp = torch.zeros_like(direct)
    if dsm is not None:
        g = dsm.float()
        sp = sm * (g - (_wave_sum(g * sm) if wave_tree else (g * sm).sum(-1, keepdim=True)))
    return (_r(sp, dt) + direct).to(dt)
