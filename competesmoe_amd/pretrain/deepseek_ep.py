"""Pretrain `deepseekv2` / `deepseekv3` with expert-parallel routed experts (`deepseekv2_ep`, `deepseekv3_ep`).

The reference trains data-parallel only (moe_pretrain_model/layers/moe/deepseekv2.py:135-181, deepseekv3.py:142-190); these are its
shared-expert layers with the packed routed experts sharded over the group, under the contract every expert-parallel layer here has:
the numbers of the single-GPU layer on the same tokens.

* Routed experts: `keys` [E/P, D, F], `values` [E/P, F, Dout] (and `bias` [E/P, F]) are this rank's slice (global experts rank*E/P
  ...); `n_experts` is the GLOBAL count.  bf16 / fp32 experts take ep.EPFFNPacked, `args.fp8_experts` takes ep.EPFFNPackedFP8
  (`args.fp8_weight_cache` as on one GPU).  `args.fp8_wgrad` is refused: its token-dim blocks hold 32 consecutive binned rows of one
  expert, and under expert parallelism an expert's rows stand in another order (by source rank), so the blocks -- and the numbers --
  would differ from the single-GPU layer's.
* Replicated: `w_gate`, `o_bias`, `keys_shared`, `values_shared`, `bias_shared` (and v3's unused `e_score_correction_bias`).  Every
  rank runs the shared expert on its own tokens, inside the exchange: its launches go between the sends and the first wait of the
  routed step, forward and backward, and its output enters the combine epilogue in the residual slot (the bits of
  `out + out_shared`).  Gradients of the replicated tensors are summed over the group once per backward pass.
* The entropy-balance regulariser is per rank on local tokens, as data-parallel training of the reference computes it.

State-dict contract: a single-GPU `deepseekv2` / `deepseekv3` state dict with `keys` / `values` / `bias` sliced loads with
strict=True.  Init as `competesmoe_ep`: the replicated tensors are broadcast from the group's first rank, the routed shard is drawn
from a generator offset by the rank."""
import torch
import torch.distributed as dist

from .. import _lib as L
from ..ep import EPFFNPacked, EPFFNPackedFP8, _direct_default, reduce_grad_on_backward
from .deepseek import DeepSeekV2, DeepSeekV3
from .moe import op_dtype
from .register import register_moe
from .smoe_ep import EPPackedExperts, _broadcast


class _EPSharedExperts(EPPackedExperts):
    _fp8_experts_ok = True

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.fp8_wgrad:
            raise ValueError(f"{self._ep_name}: args.fp8_wgrad (or CSMOE_FP8_WGRAD=1) is a single-GPU path -- its token-dim blocks "
                             "follow the order of an expert's rows, which differs under expert parallelism")
        assert not self._fuses_residual         # the shared output takes the residual slot of the combine
        rank = dist.get_rank(self.group)
        replicated = [self.w_gate, self.o_bias, self.keys_shared, self.values_shared, self.bias_shared,
                      getattr(self, "e_score_correction_bias", None)]
        with torch.no_grad():
            for p in replicated:
                if p is not None:
                    _broadcast(p.data, self.group)
            # one base draw of the default generator (equal on ranks seeded alike, different per layer), offset by the rank
            base = int(torch.randint(0, 2 ** 62, ()))
            g = torch.Generator(device=self.keys.device).manual_seed(base + rank)
            self.keys.normal_(0.0, self.k_dim ** -0.5 * self.weight_scale, generator=g)
            self.values.normal_(0.0, self.size ** -0.5 * self.weight_scale, generator=g)
        for p in (self.keys_shared, self.values_shared, self.bias_shared):      # w_gate / o_bias: EPPackedExperts
            if p is not None:
                reduce_grad_on_backward(p, self.group)

    def _routed_and_shared(self, x, selected_experts, weights):
        """ffn(x) + shared_ffn(x) of the single-GPU layer as ONE function over the exchange.  operand(x) is called for the routed step,
        then for the shared expert -- after the gate's call: the order in which OperandFork hands out its twins on one GPU."""
        shp = x.shape
        op = op_dtype(x)
        x2 = self.operand(x)
        x_sh = self.operand(x)
        K = selected_experts.shape[-1]
        assert self._residual is None, f"{self._ep_name}: a block residual arrived in the slot of the shared expert's output"
        wk = weights.reshape(-1, K).float().contiguous()
        ik = selected_experts.reshape(-1, K).int().contiguous()
        b_sh = None if self.bias_shared is None else self.bias_shared[0]
        direct = _direct_default() if self.direct is None else bool(self.direct)
        if self.fp8_experts:
            if op != torch.bfloat16:
                raise ValueError("competesmoe_amd: args.fp8_experts needs bf16 activations (bf16 autocast or a bf16 layer)")
            out = EPFFNPackedFP8.apply(x2, wk, ik, self.keys, self.values, self.bias, self.act_code, L.COMBINE_DOT, self.n_experts,
                                       self.group, self._n_chunks(), direct, self.fp8_weight_cache, x_sh, self.keys_shared[0],
                                       self.values_shared[0], b_sh)
            return out.view(*shp[:-1], -1)
        stats = {} if (self.log_interval is not None and self.iter % self.log_interval == 0) else None
        out = EPFFNPacked.apply(x2, wk, ik, self.keys, self.values, self.bias, None, self.act_code, L.COMBINE_DOT, self.n_experts,
                                self.group, self._n_chunks(), direct, None, stats, x_sh, self.keys_shared[0], self.values_shared[0], b_sh)
        if stats:
            with torch.no_grad():
                h = stats["hact"]
                if h.numel():
                    self.log("relu_pass_rate", (h > 0).float().sum() / h.numel())
        return out.view(*shp[:-1], -1)

    def forward(self, x, return_id_experts=False, return_full=True, *args, **kwargs):
        """_SharedBase.forward with the routed step and the shared expert in one function."""
        gate_logits, weights, selected_experts, gate_softmax = self.gate_and_select(x, self.SEL, x.dtype)
        out = self._routed_and_shared(x, selected_experts, weights)
        bal = self.entropy_balance(gate_logits) * (self.args.balance_loss_coef / self.div)
        self.add_reg(lambda: bal, f"{self.name_moe}_ebalance")
        self._test_stats(selected_experts, weights, gate_softmax)
        return self._finish(out, x)


@register_moe("deepseekv2_ep")
class EPDeepSeekV2(_EPSharedExperts, DeepSeekV2):
    _ep_name = "deepseekv2_ep"


@register_moe("deepseekv3_ep")
class EPDeepSeekV3(_EPSharedExperts, DeepSeekV3):
    _ep_name = "deepseekv3_ep"
