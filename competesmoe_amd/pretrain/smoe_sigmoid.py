"""Pretrain `smoe_sigmoid`: MoEUT's sigmoid gate -- sigmoid of F.linear(x, w_gate), top-K of the sigmoids, the K values divided by
their sum cast to x.dtype, the two cvmm products (moe_pretrain_model/layers/moe/smoeut_norm.py:36-149).

The router is the one-pass kernel (csmoe_gate_select, CSMOE_SEL_SIGMOID_NORM) for bf16 operands, E <= 64, D % 8 == 0, and GateLogits
+ RouterSelect with the same rule elsewhere (fp32, E > 64, CSMOE_FUSED_ROUTER=0, logits handed over by the block).  Under bf16
autocast on an fp32 stream `sum` is an fp32-policy op and the quotient stays fp32; a bf16 stream rounds the sum and the quotient
(include/csmoe.h).  `std_gate` / `std_expert` default to the TYPE `float` upstream, a slip every caller overrides; 1.0 here.  The
regulariser is the entropy balance of the logits under the reference's name `<name_moe>_balance`."""
import torch

from .. import _lib as L
from .moe import MoE
from .register import register_moe


@register_moe("smoe_sigmoid")
class SMoEUTNorm(MoE):
    _fuses_residual = True

    def __init__(self, dmodel, n_experts, expert_size, n_heads, std_gate=1.0, std_expert=1.0, topk=2, dropout=0,
                 weight_scale=1.0, selection_mode="sigmoid", perplexity_reg=0.0, perplexity_reg_mode="step",
                 activation_after_topk=False, activation=lambda x: torch.nn.functional.relu(x, inplace=True), sel_bias=False,
                 bias=False, v_dim=None, expert_dropout=0.0, sync_distributed=False, selection_dropout=0.0, log_interval=100,
                 args=None, std=1, out_dmodel=None, is_att=False, inp_expert=None, out_expert=None):
        super().__init__(dmodel=dmodel, n_experts=n_experts, expert_size=expert_size, n_heads=n_heads, topk=topk, dropout=dropout,
                         weight_scale=weight_scale, selection_mode=selection_mode, perplexity_reg=perplexity_reg,
                         perplexity_reg_mode=perplexity_reg_mode, activation_after_topk=activation_after_topk, activation=activation,
                         sel_bias=sel_bias, bias=bias, v_dim=v_dim, expert_dropout=expert_dropout, sync_distributed=sync_distributed,
                         selection_dropout=selection_dropout, log_interval=log_interval, args=args, out_dmodel=out_dmodel, is_att=is_att,
                         out_expert=out_expert, inp_expert=inp_expert, std_gate=std_gate, std_expert=std_expert)

    def topk_expert(self, gate_logits, x_dtype=torch.float32):
        """(renormalised weights fp32, ids int32, fp32 softmax of the logits) by the sigmoid rule."""
        return self.select(gate_logits, L.SEL_SIGMOID_NORM, x_dtype)

    def forward(self, x, return_id_experts=False, return_full=True, *args, **kwargs):
        gate_logits, weights, selected_experts, _softmax = self.gate_and_select(x, L.SEL_SIGMOID_NORM, x.dtype)
        out = self.ffn(x, selected_experts, weights)
        bal = self.entropy_balance(gate_logits) * (self.args.balance_loss_coef / self.div)
        self.add_reg(lambda: bal, f"{self.name_moe}_balance")
        if getattr(self.args, "test_only", False):       # eval-time statistics over sigmoid(logits).softmax(-1) (smoeut_norm.py:145-148)
            self._test_stats(selected_experts, weights, torch.sigmoid(gate_logits).softmax(dim=-1))
        return self._finish(out, x)
