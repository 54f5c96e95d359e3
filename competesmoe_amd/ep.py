"""Expert parallelism for the sparse-MoE layer: experts sharded over the ranks of one node, tokens exchanged with RCCL
all-to-all over xGMI.

The reference has NO expert parallelism (data parallel only); this is the multi-GPU form BASELINE.json's
north_star asks for, with one correctness contract: the same numbers as the single-GPU layer on the same tokens.

Layout: rank r owns the contiguous experts [r*E/P, (r+1)*E/P).  Because the binned row space is sorted by GLOBAL expert id,
the rows a rank must send to peer p are one contiguous slice -> `all_to_all_single` with per-peer split sizes, no packing
pass.  On the full xGMI mesh every peer pair has its own link, so an all-to-all uses all 7 links at once (ring collectives
would be bound by one).  Per forward: one tiny all-to-all of per-expert counts (+ one D2H read of 2*P*E/P ints: torch's
collective API wants host split sizes), then rows out, rows back; backward mirrors with the same splits.

Received rows arrive grouped by source rank; a second (local, K=1) binning pass regroups them by local expert for the
grouped GEMM and is undone before the return trip.

Overlap (`chunks` > 1): the local experts are cut into `chunks` groups.  A group's rows are P contiguous sub-slices of the binned
row space (one per peer), exchanged as one asynchronous all-to-all that torch's RCCL process group runs on its own HIP stream:
all outbound exchanges are queued at once, the grouped GEMMs of group c start as soon as ITS rows are in, and its results travel
back while group c+1 is in the GEMMs.  Exposed communication drops from 2 (4 in the backward) full exchanges to about 1/chunks of
them.  chunks = 1 is the plain path (one blocking all_to_all_single each way).

One exchange lane, one local step: a group of local experts is a `_Lane` (send / arrived / give_back; per-peer messages + a regroup
pass, or `direct`: one message per (peer, local expert) that lands expert-major) under every overlapped function -- EPFFNChunked
for the LLaVA stack's module experts, EPFFNPacked / EPFFNPackedFP8 / EPFFNPackedSlots for the packed experts of the pretrain stack
-- and under EPFFN's direct road.  Between the trips EPFFN and EPFFNChunked call the same helpers (`_local_ffn`, `_local_dh`,
`_local_dxs`, `_local_wgrads`); the packed functions take their preludes (operand tables, fp8 input checks, the second-backward
error) from functional.py, where the single-GPU functions they mirror row for row take them too.

Everything that touches `torch.distributed` is in the small functions at the top so the plumbing is testable with `gloo`
on CPU (tests/test_ep_gloo.py); the compute between the exchanges is the same HIP kernels as the single-GPU path.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib as L
from . import functional as Fn
from . import ops
from .functional import (CompetitionAffinityPacked, DenseFFN, ExpertTable, RouterSelect, SoftplusMean, _SlotMap, _grouped_colsum,
                         _module_grads, _take_saved)
from .moe.moe import MoeLayer
from .moe.register import register_moe


# ------------------------------------------------------------------------------------------------ plumbing (gloo-testable)
@dataclass
class EPPlan:
    P: int
    E_local: int
    send_splits: List[int]        # rows this rank sends to each peer
    recv_splits: List[int]        # rows this rank receives from each peer
    recv_counts: torch.Tensor     # [P, E_local] int32 (device): rows from peer s for local expert e
    R: int                        # total rows received
    send_host: Optional[torch.Tensor] = None     # [P, E_local] int64 (host) rows sent to peer p for ITS local expert e
    recv_host: Optional[torch.Tensor] = None     # [P, E_local] int64 (host) copy of recv_counts


def make_plan(counts: torch.Tensor, group=None, per_expert: bool = False) -> EPPlan:
    """counts[E] (int32, device) = rows per GLOBAL expert on this rank -> exchange plan.  One small all-to-all + one host read
    (2*P ints, or the two [P, E/P] count matrices when the chunked exchange needs per-expert sizes)."""
    P = dist.get_world_size(group)
    E = counts.numel()
    assert E % P == 0, "experts must divide evenly over the expert-parallel ranks"
    El = E // P
    send = counts.view(P, El).contiguous()
    recv = torch.empty_like(send)
    dist.all_to_all_single(recv, send, group=group)
    if per_expert:
        both = torch.stack([send, recv]).cpu().long()         # the one device->host sync of the exchange
        sh, rh = both[0], both[1]
        return EPPlan(P, El, sh.sum(1).tolist(), rh.sum(1).tolist(), recv, int(rh.sum()), sh, rh)
    both = torch.stack([send.sum(1), recv.sum(1)]).cpu()       # the one device->host sync of the exchange
    send_splits = [int(v) for v in both[0]]
    recv_splits = [int(v) for v in both[1]]
    return EPPlan(P, El, send_splits, recv_splits, recv, sum(recv_splits))


def a2a_rows(rows: torch.Tensor, in_splits: List[int], out_splits: List[int], group=None) -> torch.Tensor:
    """Variable-size row exchange: peer p gets rows[sum(in[:p]) : sum(in[:p+1])]."""
    out = torch.empty(sum(out_splits), rows.shape[1], dtype=rows.dtype, device=rows.device)
    with ops._timed("ep_all_to_all", (rows.shape[0] + out.shape[0]) * rows.shape[1] * rows.element_size()):
        dist.all_to_all_single(out, rows.contiguous(), output_split_sizes=out_splits, input_split_sizes=in_splits, group=group)
    return out


class _Done:
    def wait(self):
        return True


def exchange_views(outs: List[torch.Tensor], ins: List[torch.Tensor], group=None):
    """Asynchronous all-to-all over per-peer row VIEWS (peer p gets ins[p], outs[p] is filled by peer p); returns a handle whose
    wait() orders the current stream after the exchange.  RCCL: `dist.all_to_all(async_op=True)` -- grouped send/recv on the
    process group's own HIP stream, started once the work already queued on the current stream is done.  Other backends (gloo in
    the CPU tests) have no list all-to-all: the views are packed and exchanged with all_to_all_single, synchronously."""
    if dist.get_backend(group) == "nccl":
        return dist.all_to_all(outs, ins, group=group, async_op=True)
    packed = torch.cat(ins) if len(ins) > 1 else ins[0].contiguous()
    got = torch.empty(sum(o.shape[0] for o in outs), packed.shape[1], dtype=packed.dtype, device=packed.device)
    dist.all_to_all_single(got, packed, output_split_sizes=[o.shape[0] for o in outs], input_split_sizes=[i.shape[0] for i in ins],
                           group=group)
    r = 0
    for o in outs:
        o.copy_(got[r:r + o.shape[0]])
        r += o.shape[0]
    return _Done()


@dataclass
class EPChunk:
    """One group of local experts [e0, e1) of the chunked exchange."""
    e0: int
    e1: int
    send_lo: List[int]            # per peer p: first row, in the binned row space, of the rows for p's local experts [e0, e1)
    send_n: List[int]             # per peer p: their number
    recv_n: List[int]             # per source s: rows arriving for my local experts [e0, e1)
    R: int                        # sum(recv_n)


def chunk_plan(plan: EPPlan, chunks: int) -> List[EPChunk]:
    """Cut the local experts into `chunks` nearly equal groups and derive every group's send sub-slices / receive sizes (host)."""
    P, El = plan.P, plan.E_local
    C = max(1, min(chunks, El))
    sh, rh = plan.send_host, plan.recv_host
    goff = torch.zeros(P * El + 1, dtype=torch.int64)
    goff[1:] = sh.flatten().cumsum(0)                         # offsets of the GLOBAL experts in the binned row space
    out = []
    for c in range(C):
        e0, e1 = c * El // C, (c + 1) * El // C
        lo = [int(goff[p * El + e0]) for p in range(P)]
        n = [int(goff[p * El + e1]) - lo[p] for p in range(P)]
        rn = [int(v) for v in rh[:, e0:e1].sum(1)]
        out.append(EPChunk(e0, e1, lo, n, rn, sum(rn)))
    return out


def _views(buf: torch.Tensor, lo: List[int], n: List[int]) -> List[torch.Tensor]:
    return [buf[a:a + k] for a, k in zip(lo, n)]


def _packed_views(buf: torch.Tensor, n: List[int]) -> List[torch.Tensor]:
    out, r = [], 0
    for k in n:
        out.append(buf[r:r + k])
        r += k
    return out


def local_expert_ids(plan: EPPlan, e0: int = 0, e1: Optional[int] = None) -> torch.Tensor:
    """Local expert id (relative to e0) of every received row of the experts [e0, e1) (rows arrive grouped by source rank, sorted
    by expert inside a group)."""
    dev = plan.recv_counts.device
    e1 = plan.E_local if e1 is None else e1
    pattern = torch.arange(e1 - e0, device=dev, dtype=torch.int32).repeat(plan.P)
    cnt = plan.recv_counts[:, e0:e1]
    R = plan.R if (e0 == 0 and e1 == plan.E_local) else int(plan.recv_host[:, e0:e1].sum())
    return torch.repeat_interleave(pattern, cnt.flatten().long(), output_size=R)


# ---- direct exchange: one message per (peer, local expert), delivered where the grouped GEMM wants it (no regroup passes) ----------
def _direct_default() -> bool:
    return os.environ.get("CSMOE_EP_DIRECT", "0") == "1"


def direct_views(buf: torch.Tensor, plan: EPPlan, e0: int, e1: int, local: bool):
    """Row views of `buf` for the experts [e0, e1) of every peer, as [(peer, view)] in the canonical message order (peer-major,
    expert ascending -- the order both ends of a pair issue their sends / receives in).
    local = False: `buf` is this rank's BINNED row space (rows sorted by global expert id): the rows of peer p's local expert e.
    local = True:  `buf` holds ONLY the rows received for my experts [e0, e1), expert-major (expert e's rows contiguous, ordered
    by source rank inside): the rows that came from peer p for my expert e."""
    P, El = plan.P, plan.E_local
    out = []
    if not local:
        goff = torch.zeros(P * El + 1, dtype=torch.int64)
        goff[1:] = plan.send_host.flatten().cumsum(0)
        for pr in range(P):
            for e in range(e0, e1):
                a = int(goff[pr * El + e])
                out.append((pr, buf[a:a + int(plan.send_host[pr, e])]))
        return out
    rh = plan.recv_host[:, e0:e1]                                  # [P, e1 - e0]
    ebase = torch.zeros(e1 - e0 + 1, dtype=torch.int64)
    ebase[1:] = rh.sum(0).cumsum(0)
    within = torch.zeros_like(rh)
    within[1:] = rh.cumsum(0)[:-1]                                # rows of expert e that came from lower ranks
    for pr in range(P):
        for j in range(e1 - e0):
            a = int(ebase[j] + within[pr, j])
            out.append((pr, buf[a:a + int(rh[pr, j])]))
    return out


def local_bins(plan: EPPlan, e0: int, e1: int) -> "ops.Bins":
    """The binned row space of an expert-major receive buffer: offsets from the received counts, on the device (no host read)."""
    cnt = plan.recv_counts[:, e0:e1].sum(0).int()
    off = torch.zeros(e1 - e0 + 1, dtype=torch.int32, device=cnt.device)
    off[1:] = cnt.cumsum(0)
    n = int(plan.recv_host[:, e0:e1].sum())
    return ops.Bins(cnt, off, None, None, n, e1 - e0, 1)


class _Works:
    def __init__(self, works):
        self.works = works

    def wait(self):
        for w in self.works:
            w.wait()
        return True


def exchange_direct(dst, src, group=None):
    """dst / src: [(peer, view)] lists of equal length in the canonical order: view i of `src` goes to its peer, view i of `dst` is
    filled by its peer (matching is by order per pair, as RCCL matches grouped send / recv).  Empty views are skipped on both ends
    (the counts agree: my send count to p for e IS p's receive count from me for e); the self pair is a device copy.  One grouped
    launch (`batch_isend_irecv`) on the process group's stream; returns a handle whose wait() orders the current stream after it."""
    me = dist.get_rank(group)
    p2p = []
    for (ps, vs), (pd, vd) in zip(src, dst):
        assert ps == pd
        if ps == me:
            if vd.shape[0]:
                vd.copy_(vs)
            continue
        peer = ps if group is None else dist.get_global_rank(group, ps)
        if vs.shape[0]:
            p2p.append(dist.P2POp(dist.isend, vs, peer, group))
        if vd.shape[0]:
            p2p.append(dist.P2POp(dist.irecv, vd, peer, group))
    return _Works(dist.batch_isend_irecv(p2p) if p2p else [])


# ------------------------------------------------------------------------------------------------ the EP FFN
class _Unsort:
    """Adapter so ops.dispatch_rows can apply the inverse of a K=1 binning (out[m] = sorted[slot_of[m]])."""
    def __init__(self, bins):
        self.perm, self.K, self.n = bins.slot_of, 1, bins.n


class _Lane:
    """One group [e0, e1) of local experts of an exchange: carries rows of the token side's binned row space to their owners, where
    they stand expert-major, and rows back (per-peer messages + a regroup pass, or `direct`).  Narrow fp32 columns ([n, 1]: routing
    weights out, dot products back) take the same road with torch indexing as their regroup."""

    def __init__(self, plan: EPPlan, cp: EPChunk, direct: bool, group):
        self.plan, self.cp, self.direct, self.group = plan, cp, direct, group
        self.as_is = direct or cp.e1 - cp.e0 == 1      # received rows are expert-major as they land (one expert: trivially)
        self._lb = None

    @property
    def lb(self) -> "ops.Bins":
        if self._lb is None:
            cp = self.cp
            self._lb = (local_bins(self.plan, cp.e0, cp.e1) if self.as_is else
                        ops.bin_tokens(local_expert_ids(self.plan, cp.e0, cp.e1).view(-1, 1), cp.e1 - cp.e0))
        return self._lb

    def send(self, src: torch.Tensor):
        """token side -> owners, asynchronously: (receive buffer, handle)."""
        cp = self.cp
        r = torch.empty(cp.R, src.shape[1], dtype=src.dtype, device=src.device)
        if self.direct:
            wk = exchange_direct(direct_views(r, self.plan, cp.e0, cp.e1, True), direct_views(src, self.plan, cp.e0, cp.e1, False), self.group)
        else:
            wk = exchange_views(_packed_views(r, cp.recv_n), _views(src, cp.send_lo, cp.send_n), self.group)
        return r, wk

    def arrived(self, r: torch.Tensor) -> torch.Tensor:
        """A waited-for receive buffer as expert-major rows."""
        if self.as_is or r.shape[0] == 0:
            return r
        return r[self.lb.perm.long()] if r.shape[1] == 1 else ops.dispatch_rows(r, self.lb)

    def arrived_mxfp8(self, r: torch.Tensor):
        """A waited-for receive buffer of bf16 rows as (expert-major rows, their MXFP8 elements, scales): the regroup pass quantises
        the rows it moves (ops.dispatch_rows_mxfp8); rows that landed expert-major are quantised where they are."""
        if r.shape[0] == 0:
            return r, r.new_empty(0, r.shape[1], dtype=torch.uint8), r.new_empty(0, r.shape[1] // 32, dtype=torch.uint8)
        if self.as_is:
            return (r,) + ops.quantize_mxfp8(r)
        return ops.dispatch_rows_mxfp8(r, self.lb)

    def give_back(self, rows: torch.Tensor, dst: torch.Tensor):
        """owners -> token side, asynchronously, into the binned row space `dst`: (handle, buffer to keep alive until waited for)."""
        cp = self.cp
        if self.direct:
            return exchange_direct(direct_views(dst, self.plan, cp.e0, cp.e1, False), direct_views(rows, self.plan, cp.e0, cp.e1, True),
                                   self.group), rows
        if rows.shape[0] and not self.as_is:
            rows = rows[self.lb.slot_of.long()] if rows.shape[1] == 1 else ops.dispatch_rows(rows, _Unsort(self.lb))
        return exchange_views(_views(dst, cp.send_lo, cp.send_n), _packed_views(rows, cp.recv_n), self.group), rows


def _wait_all(back) -> None:
    """Wait for every return trip queued with _Lane.give_back."""
    with ops._timed("ep_wait_exposed"):
        for wk, _ in back:
            wk.wait()


# ---- the owners' arithmetic of the LLaVA-stack functions: module experts [e0, e1) of `tab` on their expert-major rows
def _local_ffn(tab: ExpertTable, e0: int, e1: int, rs: torch.Tensor, lb):
    """GEMM 1 (+ b1, activation) and GEMM 2 (+ b2): (hpre, hact, ys)."""
    hpre, hact = ops.grouped_gemm(rs, tab.w1_ptrs[e0:e1], tab.layout, tab.D, tab.F, lb.offsets, e1 - e0,
                                  bias_ptrs=None if tab.b1_ptrs is None else tab.b1_ptrs[e0:e1],
                                  epilogue=L.EPI_BIAS_ACT, act=tab.act, want_c2=True, want_c=tab.act != L.ACT_RELU)
    ys = ops.grouped_gemm(hact, tab.w2_ptrs[e0:e1], tab.layout, tab.F, tab.Dout, lb.offsets, e1 - e0,
                          bias_ptrs=None if tab.b2_ptrs is None else tab.b2_ptrs[e0:e1],
                          epilogue=L.EPI_BIAS if tab.b2_ptrs is not None else L.EPI_PLAIN)
    return hpre, hact, ys


def _local_dh(tab: ExpertTable, e0: int, e1: int, dys, lb, hpre, hact):
    """dH = dYs @ W2 through the activation gradient."""
    return ops.grouped_gemm(dys, tab.w2_ptrs[e0:e1], L.B_KN, tab.F, tab.F, lb.offsets, e1 - e0, epilogue=L.EPI_ACTGRAD, act=tab.act,
                            aux=hpre if hpre is not None else hact)


def _local_dxs(tab: ExpertTable, e0: int, e1: int, dh, lb):
    """dXs = dH @ W1.  Its own call: EPFFNChunked sends it home before the weight gradients, EPFFN forms them first."""
    return ops.grouped_gemm(dh, tab.w1_ptrs[e0:e1], L.B_KN, tab.D, tab.D, lb.offsets, e1 - e0)


def _wgrad_buffers(tab: ExpertTable, dev):
    """(gW1 [E, F, D], its pointer table, gW2 [E, Dout, F], its pointer table) for all local experts."""
    E, pd = tab.E, tab.param_dtype
    es = torch.tensor([], dtype=pd).element_size()
    gW2 = torch.empty(E, tab.Dout, tab.F, dtype=pd, device=dev)
    gW1 = torch.empty(E, tab.F, tab.D, dtype=pd, device=dev)
    tW2, tW1 = ops.ptr_table(gW2, E, gW2[0].numel() * es), ops.ptr_table(gW1, E, gW1[0].numel() * es)
    return gW1, tW1, gW2, tW2


def _local_wgrads(tab: ExpertTable, e0: int, e1: int, lb, rs, hact, dys, dh, bufs):
    """Weight gradients of the experts [e0, e1) into their slices of `bufs` (_wgrad_buffers); returns their bias column sums
    (gb1 [e1 - e0, F] | None, gb2 [e1 - e0, Dout] | None) -- _grouped_colsum cuts a few experts' rows into chunks to fill the chip."""
    gW1, tW1, gW2, tW2 = bufs
    Ec, pd = e1 - e0, tab.param_dtype
    ops.grouped_wgrad(dys, hact, lb.offsets, Ec, gW2, tW2[e0:e1], xcd_order=lb.xcd_order)
    ops.grouped_wgrad(dh, rs, lb.offsets, Ec, gW1, tW1[e0:e1], xcd_order=lb.xcd_order)
    gb1 = _grouped_colsum(dh, lb.offsets, Ec, pd) if tab.b1_ptrs is not None else None
    gb2 = _grouped_colsum(dys, lb.offsets, Ec, pd) if tab.b2_ptrs is not None else None
    return gb1, gb2


def _return_trip(rows, n: int, plan: EPPlan, lane, lb, group):
    """EPFFN's blocking return trip of expert-major `rows` into a fresh [n, C] tensor in the token side's binned order."""
    if lane is None:
        return a2a_rows(ops.dispatch_rows(rows, _Unsort(lb)), plan.recv_splits, plan.send_splits, group)
    dst = torch.empty(n, rows.shape[1], dtype=rows.dtype, device=rows.device)
    lane.give_back(rows, dst)[0].wait()
    return dst


class EPFFN(torch.autograd.Function):
    """dispatch -> all-to-all -> local grouped FFN -> all-to-all -> combine, and the mirrored backward."""

    @staticmethod
    def forward(ctx, x2, w, idx, tab: ExpertTable, E_global: int, group, combine_mode: int, want_slots: bool, direct: bool, *params):
        """Returns (out [T, Dout], y_tk): the combined output and, with `want_slots`, the expert outputs per (token, k) slot in flat
        order [T*K, Dout] -- what `torch.gather(expert_outputs, idx)` gives the single-GPU competition step for its diversity
        loss (an empty tensor otherwise); gradients of both are accepted.
        `direct`: one message per (peer, local expert) straight into an expert-major buffer -- ONE lane of all local experts, waited
        for at once -- instead of one blocking all_to_all_single per trip followed by a regroup pass (and its inverse before the
        return trip); same rows through the same kernels."""
        x2 = x2.contiguous()
        T = x2.shape[0]
        bins = ops.bin_tokens(idx, E_global)
        xs = ops.dispatch_tokens(x2, bins)
        plan = make_plan(bins.counts, group, per_expert=direct)
        lane = _Lane(plan, chunk_plan(plan, 1)[0], True, group) if direct else None
        if direct:
            r, wk = lane.send(xs)
            wk.wait()
            rs, lb = lane.arrived(r), lane.lb
        else:
            recv = a2a_rows(xs, plan.send_splits, plan.recv_splits, group)
            lb = ops.bin_tokens(local_expert_ids(plan).view(-1, 1), tab.E)
            rs = ops.dispatch_rows(recv, lb)
        hpre, hact, ys = _local_ffn(tab, 0, tab.E, rs, lb)
        y = _return_trip(ys, bins.n, plan, lane, lb, group)
        out = ops.combine(y, bins, idx, w, combine_mode, T)
        ctx.saved = (bins, lb, plan, lane, rs, hpre, hact, y)
        ctx.tab, ctx.w, ctx.group, ctx.n_params = tab, w, group, len(params)
        ctx.want_slots = want_slots
        ctx.round_dw = combine_mode == L.COMBINE_SEQ_RW        # bf16 affinity weights: d w as autograd forms it (functional._ffn_backward)
        y_tk = ops.dispatch_rows(y, _Unsort(bins)) if want_slots else y.new_empty(0)      # y_tk[t*K+k] = y[slot_of[t*K+k]]
        return out, y_tk

    @staticmethod
    def backward(ctx, dout, dy_tk=None):
        bins, lb, plan, lane, rs, hpre, hact, y = _take_saved(ctx)
        tab, group = ctx.tab, ctx.group
        assert tab.layout == L.B_NK
        E, dev = tab.E, dout.device
        T = dout.shape[0]
        dy, dw = ops.combine_bwd(dout.contiguous(), y, bins, ctx.w, want_dw=ctx.needs_input_grad[1], round_products=ctx.round_dw)
        if dy_tk is not None and ctx.want_slots:               # gradient of the per-slot outputs (diversity loss), binned order
            dy = dy + ops.dispatch_rows(dy_tk.contiguous(), ops.Bins(None, None, bins.perm, None, bins.n, bins.E, 1))
        if lane is None:
            dys = ops.dispatch_rows(a2a_rows(dy, plan.send_splits, plan.recv_splits, group), lb)
        else:
            r, wk = lane.send(dy)
            wk.wait()
            dys = lane.arrived(r)
        dh = _local_dh(tab, 0, E, dys, lb, hpre, hact)
        grads = None
        if any(ctx.needs_input_grad[9:]):
            bufs = _wgrad_buffers(tab, dev)
            gb1, gb2 = _local_wgrads(tab, 0, E, lb, rs, hact, dys, dh, bufs)
            grads = (bufs[0], gb1, bufs[2], gb2)
        dx2 = None
        if ctx.needs_input_grad[0]:
            dx2 = ops.dispatch_rows_bwd(_return_trip(_local_dxs(tab, 0, E, dh, lb), bins.n, plan, lane, lb, group), bins, T)
        return (dx2, dw, None, None, None, None, None, None, None, *_module_grads(grads, E, ctx.n_params))


class EPFFNChunked(torch.autograd.Function):
    """EPFFN with the exchanges cut into groups of local experts -- one _Lane each -- and overlapped with the grouped GEMMs (module
    docstring).  Same numbers as EPFFN: every row goes through the same kernels with the same operands, only the launch grouping
    differs."""

    @staticmethod
    def forward(ctx, x2, w, idx, tab: ExpertTable, E_global: int, group, combine_mode: int, chunks: int, direct: bool, *params):
        x2 = x2.contiguous()
        T = x2.shape[0]
        bins = ops.bin_tokens(idx, E_global)
        xs = ops.dispatch_tokens(x2, bins)
        plan = make_plan(bins.counts, group, per_expert=True)
        lanes = [_Lane(plan, cp, direct, group) for cp in chunk_plan(plan, chunks)]
        sent = [ln.send(xs) for ln in lanes]               # every outbound exchange is queued now, on the process group's stream
        y = torch.empty(bins.n, tab.Dout, dtype=xs.dtype, device=xs.device)
        back, saved = [], []
        for ln, (r, wk) in zip(lanes, sent):
            with ops._timed("ep_wait_exposed"):
                wk.wait()
            rs = ln.arrived(r)
            hpre, hact, ys = _local_ffn(tab, ln.cp.e0, ln.cp.e1, rs, ln.lb)
            back.append(ln.give_back(ys, y))
            saved.append((rs, hpre, hact))
        _wait_all(back)
        del back, sent
        out = ops.combine(y, bins, idx, w, combine_mode, T)
        ctx.saved = (bins, lanes, saved, y)
        ctx.tab, ctx.w, ctx.n_params = tab, w, len(params)
        return out

    @staticmethod
    def backward(ctx, dout):
        bins, lanes, saved, y = _take_saved(ctx)
        tab = ctx.tab
        assert tab.layout == L.B_NK
        E, dev, pd = tab.E, dout.device, tab.param_dtype
        T = dout.shape[0]
        need_params = any(ctx.needs_input_grad[9:])
        need_dx = ctx.needs_input_grad[0]
        dy, dw = ops.combine_bwd(dout.contiguous(), y, bins, ctx.w, want_dw=ctx.needs_input_grad[1])
        sent = [ln.send(dy) for ln in lanes]
        grads = None
        if need_params:
            bufs = _wgrad_buffers(tab, dev)
            gb1 = torch.empty(E, tab.F, dtype=pd, device=dev) if tab.b1_ptrs is not None else None
            gb2 = torch.empty(E, tab.Dout, dtype=pd, device=dev) if tab.b2_ptrs is not None else None
            grads = (bufs[0], gb1, bufs[2], gb2)
        dxs = torch.empty(bins.n, tab.D, dtype=dy.dtype, device=dev) if need_dx else None
        back = []
        for ln, (r, wk), (rs, hpre, hact) in zip(lanes, sent, saved):
            with ops._timed("ep_wait_exposed"):
                wk.wait()
            e0, e1, lb = ln.cp.e0, ln.cp.e1, ln.lb
            dys = ln.arrived(r)
            dh = _local_dh(tab, e0, e1, dys, lb, hpre, hact)
            if need_dx:                                  # input gradient first: its return trip overlaps this group's weight gradients
                back.append(ln.give_back(_local_dxs(tab, e0, e1, dh, lb), dxs))
            if need_params:
                for buf, part in zip((gb1, gb2), _local_wgrads(tab, e0, e1, lb, rs, hact, dys, dh, bufs)):
                    if buf is not None:
                        buf[e0:e1] = part
        dx2 = None
        if need_dx:
            _wait_all(back)
            del back
            dx2 = ops.dispatch_rows_bwd(dxs, bins, T)
        return (dx2, dw, None, None, None, None, None, None, None, *_module_grads(grads, E, ctx.n_params))


# ------------------------------------------------------------------------------------------------ packed experts (pretrain stack)
def _packed_grad_buffers(El: int, D: int, F: int, Dout: int, pd, gb_dtype, dev):
    """(gk [El, D, F], gv [El, F, Dout], their pointer tables, gb [El, F] in `gb_dtype` | None) of this rank's packed experts."""
    es = torch.tensor([], dtype=pd).element_size()
    gk = torch.empty(El, D, F, dtype=pd, device=dev)
    gv = torch.empty(El, F, Dout, dtype=pd, device=dev)
    tk, tv = ops.ptr_table(gk, El, D * F * es), ops.ptr_table(gv, El, F * Dout * es)
    gb = None if gb_dtype is None else torch.empty(El, F, dtype=gb_dtype, device=dev)
    return gk, gv, tk, tv, gb


class EPFFNPacked(torch.autograd.Function):
    """functional.MoEFFNPacked (the pretrain stack's two `cvmm` calls, moe_pretrain_model/layers/moe/moe.py:397-435 + cvmm.py:490-551)
    with the packed experts sharded over the group: `keys` [E/P, D, F], `values` [E/P, F, Dout] (+ `bias` [E/P, F]) are THIS rank's
    experts, `idx` holds global expert ids.  Rows travel to their experts' owners in `chunks` groups of local experts whose exchanges
    overlap the grouped GEMMs, as in EPFFNChunked.  The arithmetic is the single-GPU function's, row for row:
    * forward: combine with the bf16-valued routing weights (`reduction_weight.type_as`), o_bias / residual in its epilogue;
    * backward of the weighted product in the reference's order (cvmm.py:527-543): the UNSCALED upstream rows and their routing
      weights go to the owners, where dH's epilogue scales the rounded product; the owners form dy = round(w * row) for d values
      themselves; with ReLU experts d w is the dot <unscaled rounded product, activated input> (cvmm.py:544) out of the same launch
      and returns with the dXs rows as one fp32 column."""

    @staticmethod
    def forward(ctx, x2, w, idx, keys, values, bias, o_bias, act: int, combine_mode: int, E_global: int, group, chunks: int,
                direct: bool, residual=None, stats=None, x_shared=None, keys_shared=None, values_shared=None, bias_shared=None):
        """`x_shared`, `keys_shared` [D, Fs], `values_shared` [Fs, Dout], `bias_shared` [Fs] or None: the always-on shared expert of
        the deepseek layers (functional.DenseFFN's body), launched after every lane's send is queued and before the first wait, in the
        forward and in the backward; its output enters the combine epilogue as the residual (the bits of `out + out_shared`), its dx
        is returned as the gradient of `x_shared`, a separate input."""
        x2 = x2.contiguous()
        op = x2.dtype
        if op == torch.bfloat16:
            w = w.to(op).float()
        _, D, F = keys.shape
        has_shared = x_shared is not None
        # the shared output takes the residual slot of the combine: no block residual may arrive with it (_fuses_residual = False)
        assert not (has_shared and residual is not None), "EPFFNPacked: a shared expert and a block residual share one combine slot"
        Dout = values.shape[2]
        dev = x2.device
        T = x2.shape[0]

        def operand(t):
            if t.dtype == op:
                return t.contiguous()
            if Fn._WEIGHT_CACHE_ON:
                c, hit = Fn._cached_copy(t, op)
                if hit:
                    return c
            c = t.to(op)
            if Fn._WEIGHT_CACHE_ON:
                Fn._remember(t, op, c)
            return c

        # fp32 masters under bf16 rows: converted inside the forward GEMMs' tile fill, the bf16 copies the backward reads being a side
        # output (functional.MoEFFNPacked; groups too small for that kernel cast their slice first)
        in_fill = (Fn._F32W_ON and not Fn._WEIGHT_CACHE_ON and op == torch.bfloat16 and keys.dtype == torch.float32
                   and values.dtype == torch.float32 and keys.is_contiguous() and values.is_contiguous())
        if in_fill:
            k_op = torch.empty(keys.shape, dtype=op, device=dev)
            v_op = torch.empty(values.shape, dtype=op, device=dev)
        else:
            k_op, v_op = operand(keys), operand(values)
        tab, b_op, ob = Fn._packed_table(k_op, v_op, bias, o_bias, act, combine_mode, keys.dtype)
        b1, epi1 = tab.b1_ptrs, tab.epi1
        bins = ops.bin_tokens(idx, E_global)
        xs = ops.dispatch_tokens(x2, bins)
        plan = make_plan(bins.counts, group, per_expert=True)
        lanes = [_Lane(plan, cp, direct, group) for cp in chunk_plan(plan, chunks)]
        sent = [ln.send(xs) for ln in lanes]               # every outbound exchange is queued now, on the process group's stream
        ctx.shared = None
        if has_shared:                                     # no communication: its GEMMs cover the exchange
            residual, sh_saved, sh_cfg = Fn.dense_ffn_forward(x_shared, keys_shared, bias_shared, values_shared, None, act, L.B_KN)
            ctx.shared = (sh_saved, sh_cfg)
        y = torch.empty(bins.n, Dout, dtype=op, device=dev)
        back, saved = [], []
        for ln, (r, wk) in zip(lanes, sent):
            with ops._timed("ep_wait_exposed"):
                wk.wait()
            e0, e1 = ln.cp.e0, ln.cp.e1
            rs, lb = ln.arrived(r), ln.lb
            b1c = None if b1 is None else b1[e0:e1]
            # the converting launch covers ONE row tile per expert (ceil(N / 256) workgroups each): with fewer than 4 experts it leaves
            # most of the chip idle while it streams their fp32 weights (tools/ep_groups_ab.sh 8 --stack pretrain: 0.80 against 0.62 ms
            # per single-expert GEMM) -- such groups cast their slice and take the plain kernels
            if in_fill and e1 - e0 >= 4 and ops.f32w_ok(rs.shape[0], F, D) and ops.f32w_ok(rs.shape[0], Dout, F):
                hpre, hact = ops.grouped_gemm_f32w(rs, keys[e0:e1], lb.offsets, copy=k_op[e0:e1], bias_ptrs=b1c, epilogue=epi1, act=act,
                                                   want_c2=True, want_c=act != L.ACT_RELU)
                ys = ops.grouped_gemm_f32w(hact, values[e0:e1], lb.offsets, copy=v_op[e0:e1])
            else:
                if in_fill:
                    k_op[e0:e1].copy_(keys[e0:e1])
                    v_op[e0:e1].copy_(values[e0:e1])
                hpre, hact = ops.grouped_gemm(rs, tab.w1_ptrs[e0:e1], L.B_KN, F, F, lb.offsets, e1 - e0, bias_ptrs=b1c, epilogue=epi1,
                                              act=act, want_c2=True, want_c=act != L.ACT_RELU)
                ys = ops.grouped_gemm(hact, tab.w2_ptrs[e0:e1], L.B_KN, Dout, Dout, lb.offsets, e1 - e0)
            back.append(ln.give_back(ys, y))
            saved.append((rs, hpre, hact))
        _wait_all(back)
        del back, sent
        out = ops.combine(y, bins, idx, w, combine_mode, T, obias=ob, residual=None if residual is None else residual.contiguous())
        if stats is not None:               # `relu_pass_rate` over the rows this rank's experts processed
            stats["hact"] = torch.cat([sv[2] for sv in saved]) if len(saved) > 1 else saved[0][2]
        ctx.tab, ctx.w, ctx.group, ctx.op = tab, w, group, op
        ctx.saved = (bins, lanes, saved, y)
        ctx.keep = (k_op, v_op, b_op)
        ctx.has = (bias is not None, o_bias is not None, residual is not None and not has_shared)
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.ob_dtype = None if o_bias is None else o_bias.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        return EPFFNPacked._backward(ctx, _take_saved(ctx), dout)

    @staticmethod
    def _backward(ctx, taken, dout, dy_extra=None):
        """`dy_extra`: gradient of the per-slot outputs (EPFFNPackedSlots) in binned order, operand dtype.  It travels to the owners as
        one more message per lane and enters there as functional._ffn_backward's `dy_extra` does: its own dH product (W2^T and the
        activation gradient, no routing weight) added to dH, and added to dy for d values; it carries no d w."""
        bins, lanes, saved, y = taken
        tab, op = ctx.tab, ctx.op
        El, D, F, Dout, pd = tab.E, tab.D, tab.F, tab.Dout, tab.param_dtype
        dev = dout.device
        T = dout.shape[0]
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_params = ctx.needs_input_grad[3] or ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
        dout = dout.contiguous()
        scale_after = tab.scale_after_gemm and Fn._SCALE_AFTER_ON
        relu = tab.act == L.ACT_RELU
        # every rank must take the same road (the dot column is an exchange): decided from the shapes, not from this rank's row count
        use_dot = bool(scale_after and need_dw and relu and ops.rowdot_cols(256, F, Dout, Dout, Dout, F, op) > 0)
        dy, dw = ops.combine_bwd(dout, y if (need_dw and not use_dot) else None, bins, ctx.w, want_dw=need_dw and not use_dot, act_dtype=op)
        del y
        if scale_after:
            rows_out = ops.dispatch_tokens(dout.to(op), bins)
            w_out = ctx.w.reshape(-1)[bins.perm.long()].float().view(-1, 1).contiguous()
            sent = [(ln.send(rows_out), ln.send(w_out)) for ln in lanes]
        else:
            sent = [(ln.send(dy), None) for ln in lanes]
        extra_sent = [ln.send(dy_extra) for ln in lanes] if dy_extra is not None else [None] * len(lanes)
        sh = (None,) * 4
        if ctx.shared is not None:                       # the shared expert's backward, between the sends and the first wait
            sh_saved, sh_cfg = ctx.shared
            ctx.shared = None
            need = ctx.needs_input_grad
            dx_s, gks, gbs, gvs, _ = Fn.dense_ffn_backward(sh_saved, sh_cfg, dout, (need[15], need[16], need[18], need[17], False))
            sh = (dx_s, gks, gvs, gbs)
        gk = gv = gb = None
        if need_params:
            gk, gv, tk, tv, gb = _packed_grad_buffers(El, D, F, Dout, pd, pd if tab.b1_ptrs is not None else None, dev)
        dxs = torch.empty(bins.n, D, dtype=op, device=dev) if need_dx else None
        dots = torch.empty(bins.n, 1, dtype=torch.float32, device=dev) if use_dot else None
        back = []
        for ln, (rows_s, w_s), ex_s, (rs, hpre, hact) in zip(lanes, sent, extra_sent, saved):
            with ops._timed("ep_wait_exposed"):
                rows_s[1].wait()
                if w_s is not None:
                    w_s[1].wait()
                if ex_s is not None:
                    ex_s[1].wait()
            e0, e1 = ln.cp.e0, ln.cp.e1
            Ec, lb = e1 - e0, ln.lb
            dys = ln.arrived(rows_s[0])
            ex = None if ex_s is None else ln.arrived(ex_s[0])
            aux = hpre if hpre is not None else hact
            if scale_after:
                wr = ln.arrived(w_s[0]).view(-1)
                dot = col = None
                if use_dot and dys.shape[0]:
                    dc = ops.rowdot_cols(dys.shape[0], F, Dout, Dout, Dout, F, op)
                    if dc:
                        dot = torch.empty(dys.shape[0], dc, dtype=torch.float32, device=dev)
                    else:
                        # this lane's dH launch writes no dot table (its rows push A past the fast kernel's 2 GiB limit) while the
                        # group's launches do: the column in three steps, as _CVMM.backward's fallback forms it; same exchange shape
                        prod = ops.grouped_gemm(dys, tab.w2_ptrs[e0:e1], L.B_NK, Dout, F, lb.offsets, Ec)
                        col = (prod.float() * hact.float()).sum(-1).view(-1, 1)
                        del prod
                dh = ops.grouped_gemm(dys, tab.w2_ptrs[e0:e1], L.B_NK, Dout, F, lb.offsets, Ec, epilogue=L.EPI_ACTGRAD_ROWSCALE, act=tab.act,
                                      aux=aux, row_scale=wr, row_dot=dot)
                if use_dot:
                    if dot is not None:
                        col = ops.finish_row_dot(dot).view(-1, 1)
                    elif col is None:
                        col = torch.empty(0, 1, dtype=torch.float32, device=dev)
                    back.append(ln.give_back(col, dots))
                if ex is not None:                       # the unweighted per-slot rows: their own product, added to dH
                    dh = dh + ops.grouped_gemm(ex.contiguous(), tab.w2_ptrs[e0:e1], L.B_NK, Dout, F, lb.offsets, Ec, epilogue=L.EPI_ACTGRAD,
                                               act=tab.act, aux=aux)
                if need_params:                          # dy = round(w * upstream row), what combine_bwd hands the single-GPU d values
                    dys = ops.scale_rows(dys, wr)
                    if ex is not None:
                        dys = dys + ex
            else:
                if ex is not None:                       # dy + extra through one dH product, as the single-GPU backward forms it
                    dys = dys + ex
                dh = ops.grouped_gemm(dys, tab.w2_ptrs[e0:e1], L.B_NK, Dout, F, lb.offsets, Ec, epilogue=L.EPI_ACTGRAD, act=tab.act, aux=aux)
            if need_dx:                                  # input gradient first: its return trip overlaps this group's weight gradients
                back.append(ln.give_back(ops.grouped_gemm(dh, tab.w1_ptrs[e0:e1], L.B_NK, F, D, lb.offsets, Ec), dxs))
            if need_params:
                ops.grouped_wgrad(hact, dys, lb.offsets, Ec, gv, tv[e0:e1], xcd_order=lb.xcd_order)
                ops.grouped_wgrad(rs, dh, lb.offsets, Ec, gk, tk[e0:e1], xcd_order=lb.xcd_order)
                if gb is not None:
                    gb[e0:e1] = _grouped_colsum(dh, lb.offsets, Ec, pd)
        _wait_all(back)
        del back, sent
        if use_dot:
            dw = dots.view(-1)[bins.slot_of.long()].view(T, bins.K)
        dx2 = ops.dispatch_rows_bwd(dxs, bins, T) if need_dx else None
        if gb is not None and gb.dtype != ctx.bias_dtype:
            gb = gb.to(ctx.bias_dtype)
        gob = None
        if ctx.has[1] and ctx.needs_input_grad[6]:
            gob = Fn._chunked_dense_colsum(dout, ctx.ob_dtype)
        return (dx2, dw, None, gk, gv, gb, gob, None, None, None, None, None, None,
                dout if (ctx.has[2] and ctx.needs_input_grad[13]) else None, None, *sh)


class EPFFNPackedFP8(torch.autograd.Function):
    """functional.MoEFFNPackedFP8 (the four row-space expert GEMMs of a step on the block-scaled fp8 pipe, BASELINE config 5) with the
    packed experts sharded over the group, row for row, on the lanes of EPFFNPacked.  bf16 rows travel (the owners need them for the
    bf16 weight gradients); the owners' regroup pass quantises them as it moves them (_Lane.arrived_mxfp8).  The master weights of
    the local shard are quantised once per forward (or per parameter version with `cache`) and sliced per lane; the backward pair is
    kept.  Backward: combine_bwd on the token side as on one GPU -- dy = round(w * dout row) travels, one message per lane, and d w
    comes from the returned y; there is no weight or dot column (the fp8 layer scales before the product).  Every rank takes the same
    road through every collective: nothing here branches on a row count in a way that changes the messages.
    `x_shared` ...: the shared expert (functional.DenseFFNFP8's body) between the sends and the first wait, as in EPFFNPacked."""

    @staticmethod
    def forward(ctx, x2, w, idx, keys, values, bias, act: int, combine_mode: int, E_global: int, group, chunks: int, direct: bool,
                cache: bool = False, x_shared=None, keys_shared=None, values_shared=None, bias_shared=None):
        x2, w = Fn._fp8_rows_and_weights(x2, w)
        El, D, F = keys.shape
        Dout = values.shape[2]
        T = x2.shape[0]
        dev = x2.device
        bins = ops.bin_tokens(idx, E_global)
        xs = ops.dispatch_tokens(x2, bins)
        plan = make_plan(bins.counts, group, per_expert=True)
        lanes = [_Lane(plan, cp, direct, group) for cp in chunk_plan(plan, chunks)]
        sent = [ln.send(xs) for ln in lanes]               # every outbound exchange is queued now, on the process group's stream
        y_shared = None
        ctx.shared = None
        if x_shared is not None:                           # no communication: its GEMMs cover the exchange
            y_shared, sh_saved, sh_cfg = Fn.dense_ffn_fp8_forward(x_shared, keys_shared, bias_shared, values_shared, act, cache)
            ctx.shared = (sh_saved, sh_cfg)
        (kq_b, ks_b), (kq, ks) = Fn._quantize_weight_both(keys, cache)        # backward pair [El, D, F]; forward pair [El, F, D]
        (vq_b, vs_b), (vq, vs) = Fn._quantize_weight_both(values, cache)      # backward pair [El, F, Dout]; forward pair [El, Dout, F]
        b_op, b1 = Fn._fp8_bias_table(bias)
        y = torch.empty(bins.n, Dout, dtype=torch.bfloat16, device=dev)
        back, saved = [], []
        for ln, (r, wk) in zip(lanes, sent):
            with ops._timed("ep_wait_exposed"):
                wk.wait()
            e0, e1 = ln.cp.e0, ln.cp.e1
            rs, rq, rsc = ln.arrived_mxfp8(r)              # the bf16 rows are kept for the `keys` gradient
            lb = ln.lb
            hpre, hact = ops.grouped_gemm_mxfp8(rq, rsc, kq[e0:e1], ks[e0:e1], lb.offsets, bias_ptrs=None if b1 is None else b1[e0:e1],
                                                epilogue=L.EPI_BIAS_ACT, act=act, want_c2=True, want_c=act != L.ACT_RELU)
            del rq, rsc
            hq, hs = _quantize_rows(hact)
            ys = ops.grouped_gemm_mxfp8(hq, hs, vq[e0:e1], vs[e0:e1], lb.offsets)
            back.append(ln.give_back(ys, y))
            saved.append((rs, hpre, hact))
        _wait_all(back)
        del back, sent
        out = ops.combine(y, bins, idx, w, combine_mode, T, residual=y_shared)
        ctx.saved = (bins, lanes, saved, y, b_op)
        ctx.wq = (kq_b, ks_b, vq_b, vs_b)
        ctx.w, ctx.shape, ctx.pd = w, (El, D, F, Dout), keys.dtype
        ctx.cfg = (act, None if bias is None else bias.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        bins, lanes, saved, y, _ = _take_saved(ctx)
        act, bias_dtype = ctx.cfg
        El, D, F, Dout = ctx.shape
        dev = dout.device
        T = dout.shape[0]
        need = ctx.needs_input_grad
        need_dx, need_dw = need[0], need[1]
        need_params = need[3] or need[4] or need[5]
        dout = dout.contiguous()
        dy, dw = ops.combine_bwd(dout, y if need_dw else None, bins, ctx.w, want_dw=need_dw, act_dtype=torch.bfloat16)
        del y
        sent = [ln.send(dy) for ln in lanes]
        sh = (None,) * 4
        if ctx.shared is not None:                       # the shared expert's backward, between the sends and the first wait
            sh_saved, sh_cfg = ctx.shared
            ctx.shared = None
            dx_s, gks, gbs, gvs = Fn.dense_ffn_fp8_backward(sh_saved, sh_cfg, dout, (need[13], need[14], need[16], need[15]))
            sh = (dx_s, gks, gvs, gbs)
        kq, ks, vq, vs = ctx.wq
        ctx.wq = None
        gk = gv = gb = None
        if need_params:
            gk, gv, tk, tv, gb = _packed_grad_buffers(El, D, F, Dout, ctx.pd, bias_dtype, dev)
        dxs = torch.empty(bins.n, D, dtype=torch.bfloat16, device=dev) if need_dx else None
        back = []
        for ln, (r, wk), (rs, hpre, hact) in zip(lanes, sent, saved):
            with ops._timed("ep_wait_exposed"):
                wk.wait()
            e0, e1 = ln.cp.e0, ln.cp.e1
            Ec, lb = e1 - e0, ln.lb
            dys, dyq, dysc = ln.arrived_mxfp8(r)           # the bf16 dy is kept for the `values` gradient
            dh = ops.grouped_gemm_mxfp8(dyq, dysc, vq[e0:e1], vs[e0:e1], lb.offsets, epilogue=L.EPI_ACTGRAD, act=act,     # values as stored
                                        aux=hpre if hpre is not None else hact)
            del dyq, dysc
            if need_dx:                                  # input gradient first: its return trip overlaps this group's weight gradients
                dhq, dhs = _quantize_rows(dh)
                back.append(ln.give_back(ops.grouped_gemm_mxfp8(dhq, dhs, kq[e0:e1], ks[e0:e1], lb.offsets), dxs))   # dxs = dh @ keys[e]^T
                del dhq, dhs
            if need_params:
                ops.grouped_wgrad(hact, dys, lb.offsets, Ec, gv, tv[e0:e1], xcd_order=lb.xcd_order)
                ops.grouped_wgrad(rs, dh, lb.offsets, Ec, gk, tk[e0:e1], xcd_order=lb.xcd_order)
                if gb is not None:
                    gb[e0:e1] = _grouped_colsum(dh, lb.offsets, Ec, bias_dtype)
        _wait_all(back)
        del back, sent
        dx2 = ops.dispatch_rows_bwd(dxs, bins, T) if need_dx else None
        return (dx2, dw, None, gk, gv, gb, None, None, None, None, None, None, None, *sh)


def _quantize_rows(t: torch.Tensor):
    """ops.quantize_mxfp8 of [n, C] rows; a lane that holds no rows launches nothing."""
    if t.shape[0] == 0:
        return t.new_empty(0, t.shape[1], dtype=torch.uint8), t.new_empty(0, t.shape[1] // 32, dtype=torch.uint8)
    return ops.quantize_mxfp8(t)


class EPFFNPackedSlots(torch.autograd.Function):
    """EPFFNPacked that also returns the expert outputs per (token, k) slot, [T, K, Dout] -- functional.MoEFFNPackedSlots under expert
    parallelism: the `topk` outputs of the pretrain competition step's diversity loss (moe_pretrain_model/layers/moe/competesmoe.py:
    403-410), taken from the rows the owners sent back.  Same arguments as EPFFNPacked."""

    @staticmethod
    def forward(ctx, x2, w, idx, keys, values, bias, o_bias, act: int, combine_mode: int, E_global: int, group, chunks: int,
                direct: bool, residual=None, stats=None):
        out = EPFFNPacked.forward(ctx, x2, w, idx, keys, values, bias, o_bias, act, combine_mode, E_global, group, chunks, direct,
                                  residual, stats)
        bins, y = ctx.saved[0], ctx.saved[3]
        y_tk = ops.dispatch_rows(y, _SlotMap(bins.slot_of, bins.n))        # y_tk[t*K+k] = y[slot_of[t*K+k]]
        return out, y_tk.view(x2.shape[0], idx.shape[-1], y.shape[-1])

    @staticmethod
    def backward(ctx, dout, dy_tk):
        taken = _take_saved(ctx)
        bins = taken[0]
        extra = None
        if dy_tk is not None:                             # binned order, in the operand dtype: one more message per lane
            extra = ops.dispatch_rows(dy_tk.reshape(bins.n, -1).to(ctx.op).contiguous(), _SlotMap(bins.perm, bins.n))
        if dout is None:
            dout = torch.zeros(ctx.w.shape[0], ctx.tab.Dout, dtype=ctx.op, device=ctx.w.device)
        return EPFFNPacked._backward(ctx, taken, dout, extra)[:15]     # this function takes no shared expert


# default of the local competition pass's dX chain, read once per process: 1 = every expert after the first adds its dX product into the
# running sum in the GEMM epilogue (EPI_ACCUM); 0 = GEMM + torch add_ (the single-GPU chain; same bits)
_COMP_DX_ACCUM = os.environ.get("CSMOE_COMP_DX_ACCUM", "1") != "0"


class LocalCompetitionAffinity(torch.autograd.Function):
    """The competition pass of THIS rank's packed experts over the gathered rows of all ranks: xa [P*T, D] -> [P*T, El].  Forward and
    recompute backward are functional.CompetitionAffinityPacked's; the dX products of the local experts are chained into one buffer
    with EPI_ACCUM (the first expert writes, the rest add, ascending expert order -- at world 1 the single-GPU chain bit for bit)."""

    @staticmethod
    def forward(ctx, xa, keys, values, act: int, fp32_affinity: bool):
        return CompetitionAffinityPacked.forward(ctx, xa, keys, values, act, fp32_affinity)

    @staticmethod
    def backward(ctx, daff):
        return CompetitionAffinityPacked._backward(ctx, daff, _COMP_DX_ACCUM)


def local_competition_affinity(xa: torch.Tensor, keys: torch.Tensor, values: torch.Tensor, act: int, fp32_affinity: bool) -> torch.Tensor:
    """Affinities [P*T, El] of the gathered rows to this rank's experts.  Where the affinity epilogues cannot run (ops.affinity_ok:
    fp32 operands, odd sizes) each local expert is a DenseFFN over the gathered rows followed by SoftplusMean -- the stored form of
    the single-GPU pass; only the affinities are kept, the selected outputs come from the sparse step either way."""
    if ops.affinity_ok(xa, keys.shape[2], values.shape[2]):
        return LocalCompetitionAffinity.apply(xa, keys, values, act, fp32_affinity)
    return torch.stack([SoftplusMean.apply(DenseFFN.apply(xa, keys[e], None, values[e], None, act, L.B_KN), fp32_affinity)
                        for e in range(keys.shape[0])], dim=-1)


def reduce_grad_on_backward(param: torch.Tensor, group=None):
    """Sum the gradient of a REPLICATED parameter over the expert-parallel group, once per backward pass, BEFORE it is
    accumulated into `param.grad`: with gradient accumulation (several micro-batches per optimizer step -- the pretrain loop,
    simple_task.py:286-320, and LLaVA's gradient_accumulation_steps) `param.grad` ends up as sum_r sum_mb g.  A
    post-accumulate hook that reduces `param.grad` itself would re-reduce the earlier micro-batches' sum on every pass."""
    def hook(g):
        if dist.is_initialized() and dist.get_world_size(group) > 1:
            g = g.clone()
            dist.all_reduce(g, group=group)
        return g
    return param.register_hook(hook)


# ------------------------------------------------------------------------------------------------ module
@register_moe("smoe_ep")
class EPSMoeLayer(MoeLayer):
    """`smoe` with expert-parallel experts.  `num_of_experts` is the GLOBAL expert count; `expert` is an nn.ModuleList
    with this rank's E/P local experts (global ids rank*E/P ...).  The gate is replicated: its gradient is summed over the
    group after backward (tokens are data-parallel); expert gradients are local by construction."""
    _decode_front_ok = False          # routing stays on the launches the exchange was built around

    def __init__(self, in_embed_dim=768, out_embed_dim=768, num_of_experts=4, num_selected=2, expert=None, args=None, group=None,
                 chunks: Optional[int] = None, direct: Optional[bool] = None):
        if not isinstance(expert, nn.ModuleList):
            raise ValueError("EPSMoeLayer: pass this rank's local experts as an nn.ModuleList")
        super().__init__(in_embed_dim, out_embed_dim, num_of_experts, num_selected, expert, args)
        self.group = group
        self.chunks = chunks        # groups of local experts whose exchanges overlap the GEMMs; None: CSMOE_EP_CHUNKS, else 2 (1 at P=1)
        # one message per (peer, local expert) instead of one per peer + regroup passes (exchange_direct); None: CSMOE_EP_DIRECT, else
        # off -- the per-peer all-to-all is the pattern collective libraries are tuned for; this one has not run between two GPUs yet
        # 
        self.direct = direct
        self.init_gate_weights()
        reduce_grad_on_backward(self.gate.weight, group)

    def _n_chunks(self) -> int:
        c = self.chunks
        if c is None:
            env = os.environ.get("CSMOE_EP_CHUNKS")
            c = int(env) if env else (2 if dist.get_world_size(self.group) > 1 else 1)
        return max(1, min(int(c), len(self.experts)))

    def forward(self, x, return_id_experts=False, is_vision=False):
        B, N, D = x.shape
        route = self._route(x)            # one-pass router where the shapes allow (its histogram feeds the GLOBAL binning below)
        gate_logits, weights, selected_experts, gate_softmax = route.logits, route.w, route.idx, route.softmax
        tab, params = self._expert_table(len(self.experts), x.dtype, x.device)
        chunks = self._n_chunks()
        w2 = weights.reshape(B * N, weights.shape[-1]).contiguous()
        i2 = selected_experts.reshape(B * N, selected_experts.shape[-1]).contiguous()
        direct = _direct_default() if self.direct is None else bool(self.direct)
        if chunks > 1:
            out = EPFFNChunked.apply(x.reshape(B * N, D), w2, i2, tab, self.num_of_experts, self.group, L.COMBINE_SEQ, chunks, direct,
                                     *params)
        else:
            out, _ = EPFFN.apply(x.reshape(B * N, D), w2, i2, tab, self.num_of_experts, self.group, L.COMBINE_SEQ, False, direct, *params)
        output = out.view(B, N, out.shape[-1])
        auxiliary_loss = x.new_zeros(())        # a fill kernel: torch.tensor(0.0, device=...) is a blocking H2D copy
        infor_aux = {}
        if x.requires_grad or return_id_experts:
            # per-rank losses on local tokens, as data-parallel training of the reference computes them
            auxiliary_loss, balance_loss, router_z_loss = self.combine_loss(selected_experts, gate_softmax, gate_logits)
            infor_aux = {"balance_loss": balance_loss.clone().detach(), "router_z_loss": router_z_loss.clone().detach()}
        return output, auxiliary_loss, None, infor_aux


# ------------------------------------------------------------------------------------------------ competition step under EP
def _a2a_equal(t: torch.Tensor, group) -> torch.Tensor:
    """all_to_all_single with equal splits along dim 0 (t [P * n, ...] -> [P * n, ...]: block p goes to rank p)."""
    out = torch.empty_like(t)
    dist.all_to_all_single(out, t.contiguous(), group=group)
    return out


class AllGatherRows(torch.autograd.Function):
    """x [T, D] (same T on every rank) -> [P * T, D], rank-major.  Backward: every rank holds a partial gradient of ALL tokens (the
    contribution of its local experts); block p goes to rank p and the P partial blocks are summed (an all-to-all + one add pass:
    the bytes of a reduce-scatter, and it also runs on gloo)."""

    @staticmethod
    def forward(ctx, x, group):
        P = dist.get_world_size(group)
        ctx.group, ctx.P = group, P
        if P == 1:
            return x.contiguous().clone()
        outs = list(torch.empty(P, *x.shape, dtype=x.dtype, device=x.device).unbind(0))
        dist.all_gather(outs, x.contiguous(), group=group)
        return torch.cat(outs, 0)

    @staticmethod
    def backward(ctx, g):
        if ctx.P == 1:
            return g, None
        parts = _a2a_equal(g.contiguous(), ctx.group)                     # [P * T, D]: block s = rank s's partial gradient of MY tokens
        return parts.view(ctx.P, -1, *g.shape[1:]).sum(0), None


class ScatterAffinities(torch.autograd.Function):
    """aff_local [P * T, El] -- the affinities of ALL tokens to MY experts -- -> [T, P * El]: the affinities of MY tokens to ALL
    experts, columns in global expert order (rank p owns experts p * El ...).  Backward is the mirror exchange."""

    @staticmethod
    def forward(ctx, aff_local, group):
        P = dist.get_world_size(group)
        ctx.group, ctx.P = group, P
        if P == 1:
            return aff_local.contiguous().clone()
        T, El = aff_local.shape[0] // P, aff_local.shape[1]
        got = _a2a_equal(aff_local.contiguous(), group)                   # block s = rank s's experts' affinities of MY tokens
        return got.view(P, T, El).permute(1, 0, 2).reshape(T, P * El).contiguous()

    @staticmethod
    def backward(ctx, g):
        if ctx.P == 1:
            return g, None
        P = ctx.P
        T, E = g.shape
        send = g.view(T, P, E // P).permute(1, 0, 2).reshape(P * T, E // P).contiguous()
        return _a2a_equal(send, ctx.group), None


@register_moe("competesmoe_ep")
class EPCompeteSMoE(MoeLayer):
    """`competesmoe` (moe_model/model/moe/competesmoe.py:8-415) with expert-parallel experts.  Router steps are the sparse exchange
    of `smoe_ep`.  Competition steps: every rank gathers ALL ranks' tokens, runs ITS experts densely over them (DenseFFN kernels),
    reduces each output row to its mean-softplus affinity (SoftplusMean) and sends every token's affinities back to the token's
    owner, which then holds [T, E] affinities exactly as the single-GPU layer does; selection, losses and the sparse recompute of
    the K winners (through the exchange) follow the single-GPU code.  The diversity loss takes the winners' outputs from the
    sparse pass (they live on other ranks; same values as the dense outputs the single-GPU layer gathers from).
    The reference has no expert parallelism: the contract is "the single-GPU layer's numbers on the same tokens"."""
    _decode_front_ok = False          # routing stays on the launches the exchange was built around

    def __init__(self, in_embed_dim=768, out_embed_dim=768, num_of_experts=4, num_selected=2, expert=None, args=None, group=None):
        if not isinstance(expert, nn.ModuleList):
            raise ValueError("EPCompeteSMoE: pass this rank's local experts as an nn.ModuleList")
        super().__init__(in_embed_dim, out_embed_dim, num_of_experts, num_selected, expert, args)
        from .moe.competesmoe import CompeteSMoE
        self._single = CompeteSMoE                       # schedule + branch test are the single-GPU layer's, unbound
        if args is None or not hasattr(args, "rate_flip") or not hasattr(args, "warm_up"):
            raise ValueError("The 'args' parameter must have the attributes 'rate_flip' and 'warm_up'.")
        self.group = group
        self.warm_up, self.rate_flip = args.warm_up, args.rate_flip
        self.total_steps, self.current_steps, self.step_warm, self.is_prob_flips = None, 0, None, True
        self.register_buffer("prob_flips", torch.zeros(15801))
        self._flips_host = self._flips_key = None
        self.init_gate_weights()
        reduce_grad_on_backward(self.gate.weight, group)

    def set_total_steps(self, total_steps, id_layer, prob_flips_final):
        return self._single.set_total_steps(self, total_steps, id_layer, prob_flips_final)      # rank 0 draws, broadcast

    def set_current_steps(self, step):
        self.current_steps = step

    def _sparse(self, x, idx, w, mode, want_slots=False):
        B, N, D = x.shape
        tab, params = self._expert_table(len(self.experts), x.dtype, x.device)
        K = idx.shape[-1]
        out, y_tk = EPFFN.apply(x.reshape(B * N, D), w.reshape(B * N, K).float().contiguous(), idx.reshape(B * N, K).int().contiguous(),
                                tab, self.num_of_experts, self.group, mode, want_slots, _direct_default(), *params)
        return out.view(B, N, -1), (y_tk.view(B, N, K, -1) if want_slots else None)

    def competition_policy(self, x):
        """[T, E] affinities of the local tokens to ALL experts, then the single-GPU selection (competesmoe.py:219-259)."""
        B, N, D = x.shape
        xa = AllGatherRows.apply(x.reshape(B * N, D), self.group)                   # [P*T, D]
        outs = [self.dense_expert(i, xa.view(1, -1, D)) for i in range(len(self.experts))]
        aff_local = torch.stack([SoftplusMean.apply(o.reshape(-1, o.shape[-1])) for o in outs], dim=-1)      # [P*T, El]
        aff = ScatterAffinities.apply(aff_local, self.group)                        # [T, E]
        scores = torch.sigmoid(aff) if getattr(self.args, "norm_sigmoid", False) else aff
        if getattr(self.args, "norm_sigmoid", False):
            asm = torch.softmax(aff, dim=-1, dtype=torch.float32)
            _, idx, w = RouterSelect.apply(scores, self.num_selected, L.SEL_RAW, False)
        else:
            asm, idx, w = RouterSelect.apply(scores, self.num_selected, L.SEL_RAW, False)
        E, K = self.num_of_experts, self.num_selected
        return w.view(B, N, K), idx.view(B, N, K), asm.view(B, N, E), aff.view(B, N, E)

    def forward(self, x, return_id_experts=False, is_vision=False):
        import torch.nn.functional as F
        route = self._route(x)
        gate_logits, gate_w, gate_idx, gate_softmax = route.logits, route.w, route.idx, route.softmax
        auxiliary_loss, infor_aux = x.new_zeros(()), {}
        if self._single._competing(self, x):
            aff_w, aff_idx, aff_softmax, _ = self.competition_policy(x)
            routerloss = F.mse_loss(gate_softmax, aff_softmax.detach())
            if getattr(self.args, "hybrid", False):
                il = aff_idx.long()
                routerloss = routerloss + F.mse_loss(torch.gather(gate_softmax, -1, il), torch.gather(aff_softmax, -1, il).detach()) \
                    * self.args.router_theta
            output, topk_out = self._sparse(x, aff_idx, aff_w, L.COMBINE_SEQ_RW, want_slots=True)
            diversity_loss = self.experts_diversity_loss(expert_outputs=topk_out)
            balance_loss = self.balanceloss(selected_experts=aff_idx, gate_softmax=aff_softmax)
            auxiliary_loss = (routerloss * self.args.router_loss_coef + diversity_loss * self.args.diversity_loss_coef
                              + balance_loss * self.args.bal_comp_loss_coef)
            infor_aux = {"balance_loss": balance_loss.clone().detach(), "diversity_loss": diversity_loss.clone().detach(),
                         "routerloss": routerloss.clone().detach()}
        else:
            output, _ = self._sparse(x, gate_idx, gate_w, L.COMBINE_SEQ)
            if x.requires_grad or return_id_experts:
                auxiliary_loss, balance_loss, router_z_loss = self.combine_loss(gate_idx, gate_softmax, gate_logits)
                infor_aux = {"balance_loss": balance_loss.clone().detach(), "router_z_loss": router_z_loss.clone().detach()}
        return output, auxiliary_loss, None, infor_aux
