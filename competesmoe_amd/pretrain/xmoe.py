"""Pretrain `xmoe` (moe_pretrain_model/layers/moe/xmoe.py:37-188): the XMoE cosine router over the two-cvmm FFN.

reduced = F.linear(x, expert_sel, sel_bias) in E / 2 dimensions, normalised and scored by its cosine against `expert_embeddings`
(orthogonal init, gain 0.32; rescaled IN PLACE to norm 1.5 on every forward), p = softmax(cos / 0.3) cast to x.dtype, top-K of p, weights
= softmax over the K values; regulariser `<name>_ebalance` = entropy_balance(cos).  FFN form only (upstream's att_forward is commented
out).  The router is one launch that reads x once (functional.CosineSelect) where its kernel takes the shape (bf16 operands, E even
and <= 64, D % 8 == 0, no `sel_bias`), else the gate kernel + torch-op cosine + the router kernel (functional.cosine_route_unfused)."""
import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..functional import CosineSelect, cosine_route_unfused
from .moe import MoE
from .register import register_moe


@register_moe("xmoe")
class XMOE(MoE):

    def __init__(self, *a, std=1, **kw):
        sel_bias = kw.get("sel_bias", False)
        super().__init__(*a, **kw)
        self.reduction_dim = int(self.n_experts / 2)
        emb = torch.empty(self.num_of_experts, self.reduction_dim)
        nn.init.orthogonal_(emb, gain=0.32)
        self.register_parameter("expert_embeddings", nn.Parameter(emb))
        self.temperature = 0.3
        self.bias = None
        self.expert_sel = nn.Parameter(torch.empty(self.reduction_dim, self.k_vec_dim))
        self.sel_bias = nn.Parameter(torch.zeros(self.reduction_dim)) if sel_bias else None
        nn.init.normal_(self.expert_sel, std=self.k_vec_dim ** -0.5 * self.sel_weight_scale)

    def _plain_gate(self) -> bool:
        return False

    def renorm_embeddings(self):
        with torch.no_grad():               # xmoe.py:145-149
            nrm = self.expert_embeddings.norm(p=2.0, dim=-1, keepdim=True)
            self.expert_embeddings.mul_(1.5 / nrm)

    def _flags(self, x) -> int:
        """The reference's rounding points: under bf16 autocast over an fp32 stream `matmul` runs on bf16 operands while p and the
        K-softmax stay fp32 (x.dtype); a bf16 module without autocast multiplies in fp32 and casts p / the weights to bf16."""
        xd = self._stream_dtype if self._stream_dtype is not None else x.dtype
        flags = (L.TEMP_P_BF16 | L.TEMP_W_BF16) if xd == torch.bfloat16 else 0
        if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16:
            flags |= L.COS_OPER_BF16
        return flags

    def route(self, x):
        """(gate_logits [..., E] op dtype, gate_softmax [..., E] fp32 holding x.dtype values, selected_experts [..., K] int32,
        weights [..., K] fp32)."""
        shp = x.shape
        K, E = self.num_selected, self.num_of_experts
        x2 = self.operand(x)
        self.renorm_embeddings()
        flags = self._flags(x)
        if self.sel_bias is None and ops.cosine_select_ok(x2, self.expert_sel, E, K):
            logits, p, idx, w = CosineSelect.apply(x2, self.expert_sel, self.expert_embeddings, K, flags, self.temperature, 1e-4)
        else:
            logits, p, idx, w = cosine_route_unfused(x2, self.expert_sel, self.sel_bias, self.expert_embeddings, K, flags,
                                                     self.temperature, 1e-4)
        return logits.view(*shp[:-1], E), p.view(*shp[:-1], E), idx.view(*shp[:-1], K), w.view(*shp[:-1], K)

    def forward(self, x, return_id_experts=False, return_full=True, *args, **kwargs):
        gate_logits, gate_softmax, selected_experts, weights = self.route(x)
        out = self.ffn(x, selected_experts, weights)
        bal = self.entropy_balance(gate_logits) * (self.args.balance_loss_coef / self.div)
        self.add_reg(lambda: bal, f"{self.name_moe}_ebalance")
        self._test_stats(selected_experts, weights, gate_softmax)
        return self._finish(out, x)
