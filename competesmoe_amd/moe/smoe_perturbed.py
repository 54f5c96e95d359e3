"""`smoe_perturbed`: the perturbed-cosine router (https://arxiv.org/abs/2405.14131) + sparse FFN
(moe_model/model/moe/smoe_perturbed.py:10-145).

XMoE's router (moe/xmoe.py) with a perturbed normalisation: the projected token is divided by ||v|| + theta (no clamp) and the expert
embeddings are rescaled IN PLACE by 1.5 / (||e|| + theta) on every forward; theta = 0.1.  p = softmax(cos / 0.3) cast to x.dtype,
top-K of p, weights = softmax over the K values.  On the HIP path the whole router is one launch that reads x once
(functional.CosineSelect with COS_NORM_THETA) where its kernel takes the shape (bf16, E even and <= 64, D % 8 == 0), else the gate
kernel + torch-op cosine + the router kernel (functional.cosine_route_unfused).  State-dict names are the reference's: gate.weight
(the base class's plain gate: kept, never used, no gradient), inp_reduction.weight, expert_embeddings, experts.*.  The reference
class's `competition_policy` is never called by its forward and is not built."""
import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..functional import CosineSelect, cosine_route_unfused
from .moe import MoeLayer
from .register import register_moe


@register_moe("smoe_perturbed")
class MoEPerturbedCosingGating(MoeLayer):

    def __init__(self, in_embed_dim=768, out_embed_dim=768, num_of_experts=4, num_selected=2, expert=None, args=None, theta=0.1):
        super().__init__(in_embed_dim, out_embed_dim, num_of_experts, num_selected, expert, args)
        self.theta = theta
        self.register_parameter("expert_embeddings", nn.Parameter(torch.empty(self.num_of_experts, int(num_of_experts / 2))))
        self.inp_reduction = nn.Linear(in_embed_dim, int(num_of_experts / 2), bias=False)
        self.temperature = 0.3
        self.init_gate_weights()

    def init_gate_weights(self):
        """smoe_perturbed.py:29-50: only `expert_embeddings` is drawn, from the seed-42 generator; `gate` stays as the base class
        left it."""
        if getattr(self.args, "init_weight", True) is False:
            return
        dev = self.expert_embeddings.device
        gen = torch.Generator(device=dev if dev != torch.device("meta") else torch.device("cpu"))
        gen.manual_seed(42)
        nn.init.normal_(self.expert_embeddings, mean=0.0, std=0.02, generator=gen)

    @staticmethod
    def _fusable(selected_experts, gate_softmax, gate_logits=None) -> bool:
        """Never, as in xmoe: `gate_softmax` is the TEMPERATURE softmax cast to x.dtype, not the fp32 softmax of `gate_logits` the
        loss kernels take, so the losses run in their torch form on exactly the tensors upstream hands them."""
        return False

    def _flags(self, x) -> int:
        # module dtype, no autocast: p, the K-softmax, the norm and `norm + theta` are x.dtype tensors; the division and the cosine
        # product are fp32
        if x.dtype == torch.bfloat16:
            return L.TEMP_P_BF16 | L.TEMP_W_BF16 | L.COS_NORM_THETA | L.COS_NORM_BF16
        return L.COS_NORM_THETA

    def renorm_embeddings(self):
        with torch.no_grad():               # smoe_perturbed.py:120-124: the PARAMETER is rescaled, in its own dtype
            nrm = self.expert_embeddings.norm(p=2.0, dim=-1, keepdim=True)
            self.expert_embeddings.mul_(1.5 / (nrm + self.theta))

    def route(self, x):
        """(gate_logits [B,N,E] x.dtype, gate_softmax [B,N,E] x.dtype, selected_experts [B,N,K] int32, weights [B,N,K] fp32 holding
        x.dtype values)."""
        B, N, D = x.shape
        K, E = self.num_selected, self.num_of_experts
        x2 = x.reshape(B * N, D)
        self.renorm_embeddings()
        wr = self.inp_reduction.weight
        theta = float(self.theta)
        if ops.cosine_select_ok(x2, wr, E, K):
            logits, p, idx, w = CosineSelect.apply(x2, wr, self.expert_embeddings, K, self._flags(x), self.temperature, theta)
        else:
            logits, p, idx, w = cosine_route_unfused(x2, wr, None, self.expert_embeddings, K, self._flags(x), self.temperature, theta)
        return logits.view(B, N, E), p.to(x.dtype).view(B, N, E), idx.view(B, N, K), w.view(B, N, K)

    def forward(self, x, return_id_experts=False, is_vision=False):
        """(output, auxiliary_loss, None, infor_aux) -- smoe_perturbed.py:116-145."""
        gate_logits, gate_softmax, selected_experts, weights = self.route(x)
        # `weights` is an x.dtype tensor upstream (a softmax of x.dtype values): the combine multiplies in that dtype
        output = self.compute_moe(selected_experts, weights, None, x, weights_rounded=x.dtype == torch.bfloat16)
        auxiliary_loss = x.new_zeros(())
        infor_aux = {}
        if x.requires_grad:
            auxiliary_loss, balance_loss, router_z_loss = self.combine_loss(selected_experts, gate_softmax, gate_logits)
            infor_aux = {"balance_loss": balance_loss.clone().detach(), "router_z_loss": router_z_loss.clone().detach()}
        return output, auxiliary_loss, None, infor_aux
