"""`smoe_sigmoidgating`: MoEUT's sigmoid gate (arXiv 2405.16039) on the LLaVA stack -- sigmoid of the gate logits, top-K of the
sigmoids, the K values divided by their sum cast to x.dtype, sparse FFN (moe_model/model/moe/smoe_sigmoidgating.py:8-58).

The gate is the plain `self.gate(x)`, so the router is the one-pass kernel (csmoe_gate_select, CSMOE_SEL_SIGMOID_NORM) where it
takes the shape and GateLogits + RouterSelect with the same rule elsewhere.  The reference has no epsilon in the denominator and
casts the sum with `.to(x.dtype)`: in a bf16 module the sum, the quotient and the weights are bf16 tensors, so the rule rounds the
quotient and the combine multiplies bf16 weights (COMBINE_SEQ_RW).  The balance loss reads the fp32 softmax of the logits and the
selected ids, the z-loss the logits; both only when x requires a gradient (:46-56)."""
import torch.nn as nn

from .. import _lib as L
from .moe import MoeLayer
from .register import register_moe


@register_moe("smoe_sigmoidgating")
class SMoESigmoidGating(MoeLayer):
    SEL = L.SEL_SIGMOID_NORM
    WEIGHTS_XDTYPE = True         # `weights / sum(...).to(x.dtype)`: a tensor of x.dtype
    _fuses_residual = True        # output = one combine: a block around the layer may add its residual there (moe/block.py)

    def __init__(self, in_embed_dim=768, out_embed_dim=768, num_of_experts=4, num_selected=2, expert=None, args=None):
        super().__init__(in_embed_dim, out_embed_dim, num_of_experts, num_selected, expert, args)
        self.sigmoid = nn.Sigmoid()
        self.init_gate_weights()

    def forward(self, x, return_id_experts=False, is_vision=False):
        """(output, auxiliary_loss, None, infor_aux) -- smoe_sigmoidgating.py:38-58."""
        route, output = self._route_and_compute(x)
        aux, infor_aux = self._router_aux(route, x.requires_grad, x)
        return output, aux, None, infor_aux
