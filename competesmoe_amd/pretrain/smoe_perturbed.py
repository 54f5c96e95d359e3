"""Pretrain `smoe_perturbed` (moe_pretrain_model/layers/moe/smoe_perturbed.py:38-226): cosine gating against learned expert
embeddings in a reduced space, and -- the reason it is built here -- the only upstream layer that implements the MoE ATTENTION
projections (`att_forward` / `compute_moe`, :199-226) which `FullMoeRelativeAttentionCore` calls for its q / k / v / o maps
(layers/transformer/full_moe_relative_attention.py:267-300, 355-388): per head, a top-K mixture of expert projection matrices
`experts[h * E + e]` of shape [inp_expert, out_expert], evaluated by ONE `cvmm` with reduction weights [B, N, heads, K].

The FFN form routes in one launch that reads x once (functional.CosineSelect with COS_NORM_THETA: reduction, perturbed cosine,
temperature softmax, top-K, softmax over the K) where its kernel takes the shape (bf16 operands, E even and <= 64, D % 8 == 0, no
`sel_bias`; with CSMOE_FUSED_ROUTER=0 the same router as separate launches, functional.cosine_route_unfused).  Everywhere else -- and in the attention form always, whose softmax runs per head over heads x E logits -- the gate
math ([T, E/2]- and [T, E]-sized) stays torch ops like upstream and the selection is the router kernel (RouterSelect,
SEL_TOPK_SOFTMAX: top-K of the softmax values, softmax over the K); the expert products are the grouped GEMM behind
`pretrain.cvmm`."""
import os
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib as L
from .. import ops
from ..functional import CosineSelect, RouterSelect, cosine_route_unfused
from .cvmm import cvmm, cvmm_prepare_sel2
from .moe import MoE, op_dtype
from .register import register_moe

Selection = namedtuple("Selection", ["raw_sel", "sel_val", "raw_sel_index", "sel_index"])


@register_moe("smoe_perturbed")
class MoEPerturbedCosingGating(MoE):
    _fuses_residual = True

    def __init__(self, *a, std=1, **kw):
        sel_bias = kw.get("sel_bias", False)
        super().__init__(*a, **kw)
        self.reduction_dim = int(self.n_experts / 2)
        # upstream leaves `expert_embeddings` uninitialised (torch.empty, :100-104) and renormalises it in every forward
        self.expert_embeddings = nn.Parameter(torch.empty(self.num_of_experts, self.reduction_dim))
        self.temperature = 0.3
        self.bias = None
        self.expert_sel = nn.Parameter(torch.empty(self.reduction_dim, self.k_vec_dim))
        self.sel_bias = nn.Parameter(torch.zeros(self.reduction_dim)) if sel_bias else None
        nn.init.normal_(self.expert_sel, std=self.k_vec_dim ** -0.5 * self.sel_weight_scale)
        self.theta = 0.1
        self.total_selections, self.total_gate_softmax, self.total_gate_logits = [], [], []

    def _plain_gate(self) -> bool:
        return False

    # ------------------------------------------------------------------ gate (:148-160)
    def inp_reduction(self, x):
        return F.linear(x, self.expert_sel, self.sel_bias)

    def _cosine(self, mat1, mat2):
        m1 = mat1.float() / (mat1.norm(p=2, dim=-1, keepdim=True) + self.theta)
        return torch.matmul(m1, mat2.float().transpose(0, 1)).type_as(mat1)

    def _make_finite(self, scores):
        ok = scores.isfinite()          # upstream branches on ok.all() (a host sync) and assigns in place; same values
        low = torch.where(ok, scores, torch.full_like(scores, float("inf"))).min()
        return torch.where(ok, scores, low)

    def compute_gate(self, x):
        reduced = self.inp_reduction(x)
        with torch.no_grad():           # the parameter is renormalised IN PLACE on every call, as upstream
            nrm = self.expert_embeddings.norm(p=2.0, dim=-1, keepdim=True)
            self.expert_embeddings.mul_(1.5 / (nrm + self.theta))
        return self._make_finite(self._cosine(reduced, self.expert_embeddings))

    def _top_softmax(self, gate_softmax):
        """top-K of the softmax values, softmax over the K (`_keepTopk`, :119-122; att_forward :209-214)."""
        shp = gate_softmax.shape
        _, idx, w = RouterSelect.apply(gate_softmax.reshape(-1, shp[-1]), self.num_selected, L.SEL_TOPK_SOFTMAX, False)
        K = self.num_selected
        return w.view(*shp[:-1], K), idx.view(*shp[:-1], K)

    # ------------------------------------------------------------------ FFN form (:162-197)
    def renorm_embeddings(self):
        with torch.no_grad():           # the parameter is renormalised IN PLACE on every call, as upstream (:151-155)
            nrm = self.expert_embeddings.norm(p=2.0, dim=-1, keepdim=True)
            self.expert_embeddings.mul_(1.5 / (nrm + self.theta))

    def _flags(self, x, op) -> int:
        """The reference's rounding points, as pretrain/xmoe.py::_flags, plus the perturbed normalisation: under bf16 autocast
        `norm` is an fp32-policy op (the norm and `norm + theta` stay fp32); a bf16 stream without autocast takes them in bf16."""
        xd = self._stream_dtype if self._stream_dtype is not None else x.dtype
        flags = L.COS_NORM_THETA | ((L.TEMP_P_BF16 | L.TEMP_W_BF16) if xd == torch.bfloat16 else 0)
        if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16:
            flags |= L.COS_OPER_BF16
        elif op == torch.bfloat16:
            flags |= L.COS_NORM_BF16
        return flags

    def _route_one_pass(self, x):
        """(gate_logits, weights, selected_experts) from the one-pass kernel (under CSMOE_FUSED_ROUTER=0 from its unfused twin), or None
        where it does not take the call."""
        K, E = self.num_selected, self.num_of_experts
        op = op_dtype(x)
        if (self.sel_bias is not None or not x.is_cuda or op != torch.bfloat16
                or not L.lib.csmoe_cosine_select_ok(x.numel() // x.shape[-1], x.shape[-1], E, K, L.BF16)):
            return None
        x2 = self.operand(x)
        if ops.cosine_select_ok(x2, self.expert_sel, E, K):
            route = CosineSelect.apply
        elif os.environ.get("CSMOE_FUSED_ROUTER", "1") == "0":
            # the A/B switch: the SAME router as separate launches (gate kernel, torch-op cosine, router kernel), as in xmoe.  The older
            # torch-op gate below is not its twin: on the GPU `gate_logits / temperature` of a bf16 tensor multiplies by the reciprocal,
            # which moves some bf16 quotients by an ulp and the weights by up to 2e-3; both kernels divide, as the CPU reference does.
            def route(x2_, sel, emb, *cfg):
                return cosine_route_unfused(x2_, sel, None, emb, *cfg)
        else:
            return None
        self.renorm_embeddings()
        logits, _p, idx, w = route(x2, self.expert_sel, self.expert_embeddings, K, self._flags(x, op), self.temperature, float(self.theta))
        shp = x.shape[:-1]
        return logits.view(*shp, E), w.view(*shp, K), idx.view(*shp, K)

    def forward(self, x, return_id_experts=False, return_full=True, *args, **kwargs):
        routed = self._route_one_pass(x)
        if routed is not None:
            gate_logits, weights, selected_experts = routed
            out = self.ffn(x, selected_experts, weights)
            bal = self.entropy_balance(gate_logits) * (self.args.balance_loss_coef / self.div)
            self.add_reg(lambda: bal, f"{self.name_moe}_ebalance")
            return self._finish(out, x)
        gate_logits = self.compute_gate(x)
        gate_softmax = F.softmax(gate_logits / self.temperature, dim=-1, dtype=torch.float).to(x.dtype)
        weights, selected_experts = self._top_softmax(gate_softmax)
        out = self.ffn(x, selected_experts, weights)
        bal = self.entropy_balance(gate_logits) * (self.args.balance_loss_coef / self.div)
        self.add_reg(lambda: bal, f"{self.name_moe}_ebalance")
        return self._finish(out, x)

    # ------------------------------------------------------------------ attention projections (:199-226)
    def pre_train_forward(self):
        self.total_selections, self.total_gate_softmax, self.total_gate_logits = [], [], []

    def update_aux_statistics(self, gate_logits, gate_softmax, selected_experts):
        self.total_selections.append(selected_experts)
        self.total_gate_logits.append(gate_logits)
        self.total_gate_softmax.append(gate_softmax)

    def before_loss(self):
        self.pre_train_forward()        # add_perplexity_reg upstream only resets the history (moe.py:340-358)
        if self.training:
            self.iter += 1

    def att_forward(self, x, n_experts, n_copies, return_full=True, *args, **kwargs):
        """x [B, N, dmodel] -> Selection: per head (n_copies) the top-K of softmax(gate / T) over that head's `n_experts`, the K
        values re-normalised by a softmax, and the cvmm selection over the GLOBAL expert ids h * n_experts + e."""
        if self.selection_dropout > 0 and self.training:
            x = F.dropout(x, self.selection_dropout)
        gate_logits = self.compute_gate(x)
        gate_logits = gate_logits.view(*gate_logits.shape[:-1], n_copies, -1)
        gate_softmax = F.softmax(gate_logits / self.temperature, dim=-1, dtype=torch.float).to(x.dtype)
        val, index = self._top_softmax(gate_softmax)                              # [B, N, heads, K]
        shift = (torch.arange(n_copies, device=index.device, dtype=index.dtype) * n_experts).unsqueeze(-1)
        sel_pp = cvmm_prepare_sel2((shift + index).flatten(-2, -1).int(), val, n_experts=self.n_experts)
        if self.training:
            self.update_aux_statistics(gate_logits=gate_logits, gate_softmax=gate_softmax, selected_experts=index)
        return Selection(gate_logits, val, index, sel_pp)

    def compute_moe(self, x, sel: Selection):
        """[B, N, inp_expert] -> [B, N, heads, out_expert]: sum_k val[b,n,h,k] * x[b,n] @ experts[h * E + index[b,n,h,k]]."""
        return cvmm(x, sel.sel_index, self.experts)
