"""`xmoe`: the XMoE cosine router (https://arxiv.org/abs/2204.09179) + sparse FFN (moe_model/model/moe/xmoe.py:11-105).

The token is projected to E / 2 dimensions (`inp_reduction`), normalised, and scored by its cosine against learned expert embeddings
that are rescaled IN PLACE to norm 1.5 on every forward; p = softmax(cos / 0.3) cast to x.dtype, top-K of p, weights = softmax over the K
values.  On the HIP path the whole router is one launch that reads x once (functional.CosineSelect) where its kernel takes the shape
(bf16, E even and <= 64, D % 8 == 0), else the gate kernel + torch-op cosine + the router kernel (functional.cosine_route_unfused).
State-dict names are the reference's: gate.weight / gate.bias (built and initialised, never used), inp_reduction.weight,
expert_embeddings, experts.*."""
import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..functional import CosineSelect, cosine_route_unfused
from .moe import MoeLayer
from .register import register_moe


@register_moe("xmoe")
class XMOE(MoeLayer):

    def __init__(self, in_embed_dim=768, out_embed_dim=768, num_of_experts=4, num_selected=2, expert=None, args=None):
        super().__init__(in_embed_dim, out_embed_dim, num_of_experts, num_selected, expert, args)
        self.gate = nn.Linear(in_embed_dim, num_of_experts, bias=True)
        self.register_parameter("expert_embeddings", nn.Parameter(torch.empty(self.num_of_experts, int(num_of_experts / 2))))
        self.inp_reduction = nn.Linear(in_embed_dim, int(num_of_experts / 2), bias=False)
        self.temperature = 0.3
        self.bias = None
        self.init_gate_weights()

    def init_gate_weights(self):
        """xmoe.py:30-47: only `expert_embeddings` is drawn from the seed-42 generator; `gate` keeps nn.Linear's default."""
        if getattr(self.args, "init_weight", True) is False:
            return
        dev = self.expert_embeddings.device
        gen = torch.Generator(device=dev if dev != torch.device("meta") else torch.device("cpu"))
        gen.manual_seed(42)
        nn.init.normal_(self.expert_embeddings, mean=0.0, std=0.02, generator=gen)

    @staticmethod
    def _fusable(selected_experts, gate_softmax, gate_logits=None) -> bool:
        """Never: the loss kernels (functional.RouterAux) take `gate_softmax` for the fp32 softmax of `gate_logits`; here it is the
        TEMPERATURE softmax cast to x.dtype, so the losses run in their torch form on exactly the tensors upstream hands them."""
        return False

    def _flags(self, x) -> int:
        # module dtype, no autocast: p and the K-softmax are x.dtype tensors; the cosine product is a true fp32 product
        return (L.TEMP_P_BF16 | L.TEMP_W_BF16) if x.dtype == torch.bfloat16 else 0

    def renorm_embeddings(self):
        with torch.no_grad():               # xmoe.py:81-85: the PARAMETER is rescaled, in its own dtype
            nrm = self.expert_embeddings.norm(p=2.0, dim=-1, keepdim=True)
            self.expert_embeddings.mul_(1.5 / nrm)

    def route(self, x):
        """(gate_logits [B,N,E] x.dtype, gate_softmax [B,N,E] x.dtype, selected_experts [B,N,K] int32, weights [B,N,K] fp32 holding
        x.dtype values)."""
        B, N, D = x.shape
        K, E = self.num_selected, self.num_of_experts
        x2 = x.reshape(B * N, D)
        self.renorm_embeddings()
        wr = self.inp_reduction.weight
        if ops.cosine_select_ok(x2, wr, E, K):
            logits, p, idx, w = CosineSelect.apply(x2, wr, self.expert_embeddings, K, self._flags(x), self.temperature, 1e-4)
        else:
            logits, p, idx, w = cosine_route_unfused(x2, wr, None, self.expert_embeddings, K, self._flags(x), self.temperature, 1e-4)
        return logits.view(B, N, E), p.to(x.dtype).view(B, N, E), idx.view(B, N, K), w.view(B, N, K)

    def forward(self, x, return_id_experts=False, is_vision=False):
        """(output, auxiliary_loss, None, infor_aux) -- xmoe.py:78-105."""
        gate_logits, gate_softmax, selected_experts, weights = self.route(x)
        # `weights` is an x.dtype tensor upstream (a softmax of x.dtype values): the combine multiplies in that dtype
        output = self.compute_moe(selected_experts, weights, None, x, weights_rounded=x.dtype == torch.bfloat16)
        auxiliary_loss = x.new_zeros(())
        infor_aux = {}
        if x.requires_grad:
            auxiliary_loss, balance_loss, router_z_loss = self.combine_loss(selected_experts, gate_softmax, gate_logits)
            infor_aux = {"balance_loss": balance_loss.clone().detach(), "router_z_loss": router_z_loss.clone().detach()}
        return output, auxiliary_loss, None, infor_aux
