"""Pretrain `competesmoe` with expert-parallel experts (`competesmoe_ep`).

The reference trains data-parallel only; this is the pretrain stack's CompeteSMoE layer
(moe_pretrain_model/layers/moe/competesmoe.py:37-616) with its packed experts sharded over the group, under one contract: the
numbers of the single-GPU `competesmoe` (with CSMOE_COMPETITION_LEAN=1) on the same tokens.

* Router steps: the sparse exchange of `smoe_ep` (ep.EPFFNPacked, COMBINE_DOT, the block's residual in the combine epilogue).
* Competition steps (`competition_policy_mlp_faster`): every rank gathers all ranks' tokens (ep.AllGatherRows), runs ITS experts
  densely over them (ep.local_competition_affinity: the lean pass, its backward chaining the local dX products with EPI_ACCUM),
  sends every token's affinities to the token's owner (ep.ScatterAffinities), which then selects as the single-GPU layer does; the
  K winners' outputs for the diversity loss come back from the sparse step (ep.EPFFNPackedSlots).
* forward() and every router-loss variant (plain, in_topk, hybrid, tribrid, balance_affinity, is_cosine, is_norm_weight) are the
  single-GPU class's; regularisers are per rank on local tokens, as data-parallel training of the reference computes them.
* Before its first collective every forward checks that the ranks agree on the competing decision (and, on competition steps, on
  the token count the all-gather needs): a disagreement raises the same error on every rank instead of hanging a collective.

State-dict contract: `n_experts` is the GLOBAL expert count; `keys` [E/P, D, F], `values` [E/P, F, Dout] (and `bias` [E/P, F]) are
this rank's slice of the packed tensors (global experts rank*E/P ...), `w_gate` / `o_bias` are replicated.  The slices of a
single-GPU `competesmoe` state dict load into the ranks' layers with strict=True.  Init: `w_gate` (and `o_bias`) are broadcast from
the group's first rank; each rank draws its expert shard from a generator offset by its rank, so the shards differ even when every
rank was seeded alike."""
from typing import List

import torch
import torch.distributed as dist

from .. import _lib as L
from ..ep import AllGatherRows, ScatterAffinities, local_competition_affinity
from ..functional import RouterSelect
from .competesmoe import CompeteSMoE
from .moe import op_dtype
from .register import register_moe
from .smoe_ep import EPPackedExperts, _broadcast


@register_moe("competesmoe_ep")
class EPCompeteSMoE(EPPackedExperts, CompeteSMoE):
    _ep_name = "competesmoe_ep"
    _fp8_competition_ok = False

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.fp8_competition:
            raise ValueError("competesmoe_ep: args.fp8_competition is a single-GPU path (it needs args.fp8_experts, which this layer "
                             "refuses)")
        rank = dist.get_rank(self.group)
        with torch.no_grad():
            _broadcast(self.w_gate.data, self.group)
            if self.o_bias is not None:
                _broadcast(self.o_bias.data, self.group)
            # one base draw of the default generator (equal on ranks seeded alike, different per layer), offset by the rank
            base = int(torch.randint(0, 2 ** 62, ()))
            g = torch.Generator(device=self.keys.device).manual_seed(base + rank)
            self.keys.normal_(0.0, self.k_dim ** -0.5 * self.weight_scale, generator=g)
            self.values.normal_(0.0, self.size ** -0.5 * self.weight_scale, generator=g)

    # ------------------------------------------------------------------ schedule
    def _share_schedule(self, draw, n: int, device) -> torch.Tensor:
        """Drawn on the group's first rank, broadcast within the group."""
        if dist.get_rank(self.group) == 0:
            t = torch.tensor(draw(), dtype=torch.bool, device=device)
        else:
            t = torch.empty(n, dtype=torch.bool, device=device)
        _broadcast(t, self.group)
        return t

    # ------------------------------------------------------------------ rank agreement
    def _competing(self, x, id_layer) -> bool:
        comp = super()._competing(x, id_layer)
        T = x.numel() // x.shape[-1]
        P = dist.get_world_size(self.group)
        if P > 1:
            dev = x.device if dist.get_backend(self.group) == "nccl" else torch.device("cpu")
            mine = torch.tensor([int(comp), T], dtype=torch.int64, device=dev)
            got = [torch.empty_like(mine) for _ in range(P)]
            dist.all_gather(got, mine, group=self.group)
            seen: List[List[int]] = torch.stack(got).cpu().tolist()
            decisions = {c for c, _ in seen}
            if len(decisions) > 1 or (comp and len({t for _, t in seen}) > 1):
                raise RuntimeError("competesmoe_ep: the ranks disagree on this step -- (competing, tokens) per rank: "
                                   f"{[tuple(v) for v in seen]}; the competing decision must agree, and a competition step needs "
                                   "the same token count on every rank")
        return comp

    # ------------------------------------------------------------------ steps
    def competition_policy_mlp_faster(self, x):
        """Affinities of this rank's tokens to ALL experts through the gather / local dense pass / scatter, then the single-GPU
        selection on the raw affinities; topk = None: forward() takes the winners' outputs from the sparse step (ffn_slots)."""
        B, N, D = x.shape
        op = op_dtype(x)
        x2 = self.operand(x)
        fp32_aff = op == torch.bfloat16 and torch.is_autocast_enabled("cuda")
        xa = AllGatherRows.apply(x2, self.group)                                                     # [P*T, D]
        aff_local = local_competition_affinity(xa, self.keys, self.values, self.act_code, fp32_aff)   # [P*T, E/P]
        aff = ScatterAffinities.apply(aff_local, self.group)                                          # [T, E], global expert order
        asm, idx, w = RouterSelect.apply(aff, self.num_selected, L.SEL_RAW, False)
        return w.view(B, N, -1), idx.view(B, N, -1), asm.view(B, N, -1), aff.view(B, N, -1), None

    def ffn_slots(self, x, selected_experts, weights):
        return self._ep_ffn(x, selected_experts, weights, True)
