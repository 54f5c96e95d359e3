"""MXFP8 weight gradients: the token-dim quantiser (csmoe_quantize_mxfp8_tokens), the fp8 weight-gradient GEMM
(csmoe_grouped_wgrad_mxfp8) and the `wgrad_fp8` switch of the fp8 FFN functions and the pretrain layer.

Blocking contract (include/csmoe.h): a block is 32 consecutive BINNED rows of one expert, binned order being the order
`(idx == e).nonzero()` lists; expert e's rows sit at padded positions poff[e] .. with poff[e] = sum_{j<e} roundup(count_j, 128) and
zeros up to poff[e+1].  The emulation below applies oracle/mxfp8.py's quantize to every expert's zero-padded transposed rows."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

if torch.cuda.is_available():
    from competesmoe_amd import ops, _lib as L

from oracle import mxfp8 as MX
from tests.golden_util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MX_GRAD, LOOSE = 4e-3, 3e-2


def _poff(off):
    cnt = (off[1:] - off[:-1]).long()
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum((cnt + 127) // 128 * 128, 0)])


def emulate_tokens(a, off):
    """(qt [C, poff[E]], st [C, poff[E]/32], poff) of binned rows a [n, C] with expert row ranges off [E+1] (CPU)."""
    po = _poff(off)
    qs, ss = [], []
    for e in range(len(off) - 1):
        r0, r1 = int(off[e]), int(off[e + 1])
        P = int(po[e + 1] - po[e])
        if P == 0:
            continue
        pad = torch.zeros(P, a.shape[1], dtype=torch.float32)
        pad[: r1 - r0] = a[r0:r1].float()
        nan = torch.isnan(pad)                                       # the kernel's amax skips a NaN; the NaN itself stays NaN (0x7F)
        q, s = MX.quantize(torch.where(nan, torch.zeros_like(pad), pad).t().contiguous())
        q[nan.t()] = 0x7F
        qs.append(q)
        ss.append(s)
    C = a.shape[1]
    qt = torch.cat(qs, 1) if qs else torch.zeros(C, 0, dtype=torch.uint8)
    st = torch.cat(ss, 1) if ss else torch.zeros(C, 0, dtype=torch.uint8)
    return qt, st, po


def _offsets(counts):
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.tensor(counts), 0)]).int()


def _skewed_counts(E, n, seed, hot=8):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(E, generator=g) + 0.05
    w[:hot] *= 12                                                    # consecutive hot experts (BASELINE's skewed regime)
    c = (w / w.sum() * n).long()
    c[-1] += n - int(c.sum())
    return c.tolist()


@pytest.mark.parametrize("counts,C", [([37, 0, 200, 129, 31, 64, 1], 160),        # ragged, an empty expert, C not a multiple of 128
                                      ([32768], 64),                               # E = 1, n = 32768
                                      (None, 96)])                                 # E = 128
def test_token_quantiser_matches_the_emulation(counts, C):
    if counts is None:
        counts = _skewed_counts(128, 128 * 37, 5)
    off = _offsets(counts)
    n, E = int(off[-1]), len(counts)
    g = torch.Generator().manual_seed(n + C)
    a = (torch.randn(n, C, generator=g) * torch.exp2(torch.randint(-6, 6, (n, 1), generator=g).float())).bfloat16()
    if n > 300:
        a[3, 5], a[250, 7], a[251, 9] = float("nan"), float("inf"), float("-inf")
    (qt, st, poff), (q, s) = ops.quantize_mxfp8_tokens(a.to(DEV), off.to(DEV), E, rows=True)
    eq, es, ep = emulate_tokens(a, off)
    P = int(ep[-1])
    assert qt.shape == (C, ops.token_pad_bound(n, E)) and st.shape == (C, qt.shape[1] // 32)
    assert torch.equal(poff.cpu().long(), ep)
    got = qt[:, :P].cpu().clone()
    got[(eq == 0x7F) & ((got & 0x7F) == 0x7F)] = 0x7F                # NaN of either sign
    assert torch.equal(got, eq)
    assert torch.equal(st[:, :P // 32].cpu(), es)
    rq, rs = ops.quantize_mxfp8(a.to(DEV))
    assert torch.equal(q, rq) and torch.equal(s, rs)
    # the transposed-only form writes the same bytes
    qt2, st2, _ = ops.quantize_mxfp8_tokens(a.to(DEV), off.to(DEV), E)
    assert torch.equal(qt2[:, :P], qt[:, :P]) and torch.equal(st2[:, :P // 32], st[:, :P // 32])


def _emu_wgrad(At, As, Bt, Bs, po):
    A, B = MX.dequantize(At, As), MX.dequantize(Bt, Bs)
    E = len(po) - 1
    out = torch.zeros(E, At.shape[0], Bt.shape[0], dtype=torch.float64)
    for e in range(E):
        k0, k1 = int(po[e]), int(po[e + 1])
        if k1 > k0:
            out[e] = A[:, k0:k1] @ B[:, k0:k1].t()
    return out


@pytest.mark.parametrize("counts,Na,Nb", [([300, 0, 77, 513], 264, 520), ([1000], 128, 256), ([5, 130, 260, 40, 0, 999, 64, 128], 512, 384)])
def test_wgrad_is_exact_on_exact_data(counts, Na, Nb):
    """Small integers and power-of-two block scales that differ per row and per k-block: every partial sum is exact in fp32."""
    off = _offsets(counts)
    E, n = len(counts), int(off[-1])
    po = _poff(off)
    n_pad = ops.token_pad_bound(n, E)
    g = torch.Generator().manual_seed(Na + Nb + E)
    At = MX.to_e4m3_bytes(torch.randint(-2, 3, (Na, n_pad), generator=g).float())
    Bt = MX.to_e4m3_bytes(torch.randint(-1, 3, (Nb, n_pad), generator=g).float())
    As = torch.randint(124, 130, (Na, n_pad // 32), generator=g, dtype=torch.uint8)
    Bs = torch.randint(125, 129, (Nb, n_pad // 32), generator=g, dtype=torch.uint8)
    ref = _emu_wgrad(At, As, Bt, Bs, po).float()
    out = torch.full((E, Na, Nb), float("nan"), device=DEV)
    ops.grouped_wgrad_mxfp8(At.to(DEV), As.to(DEV), Bt.to(DEV), Bs.to(DEV), po.int().to(DEV), E, out, ops.ptr_table(out, E, Na * Nb * 4))
    assert torch.equal(out.cpu(), ref), float((out.cpu() - ref).abs().max())
    if E == 1:
        d = ops.dense_wgrad_mxfp8(At.to(DEV), As.to(DEV), Bt.to(DEV), Bs.to(DEV), po.int().to(DEV))
        assert torch.equal(d.cpu(), ref[0])


def _random_case(counts, Na, Nb, seed):
    off = _offsets(counts)
    n, E = int(off[-1]), len(counts)
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, Na, generator=g).bfloat16()
    b = torch.randn(n, Nb, generator=g).bfloat16()
    at, ats, poff = ops.quantize_mxfp8_tokens(a.to(DEV), off.to(DEV), E)
    bt, bts, _ = ops.quantize_mxfp8_tokens(b.to(DEV), off.to(DEV), E)
    emu = _emu_wgrad(at.cpu(), ats.cpu(), bt.cpu(), bts.cpu(), poff.cpu())
    full = torch.zeros(E, Na, Nb, dtype=torch.float64)
    for e in range(E):
        r0, r1 = int(off[e]), int(off[e + 1])
        full[e] = a[r0:r1].double().t() @ b[r0:r1].double()
    return off, (at, ats, bt, bts, poff), emu, full


def test_wgrad_on_random_data_outputs_accumulate_and_split_k():
    counts = [700, 0, 129, 2000, 31, 512]
    E, Na, Nb = len(counts), 256, 384
    off, ops_in, emu, full = _random_case(counts, Na, Nb, 7)
    at, ats, bt, bts, poff = ops_in
    out = torch.empty(E, Na, Nb, device=DEV)
    ptrs = ops.ptr_table(out, E, Na * Nb * 4)
    ops.grouped_wgrad_mxfp8(at, ats, bt, bts, poff, E, out, ptrs)
    assert rel_l2(out.cpu(), emu) <= 2e-3, rel_l2(out.cpu(), emu)
    assert rel_l2(out.cpu(), full) <= 6e-2, rel_l2(out.cpu(), full)
    assert float(out[1].abs().max()) == 0.0                                       # the empty expert
    # accumulate into fp32
    base = torch.randn(E, Na, Nb, device=DEV)
    acc = base.clone()
    ops.grouped_wgrad_mxfp8(at, ats, bt, bts, poff, E, acc, ops.ptr_table(acc, E, Na * Nb * 4), accumulate=True)
    assert torch.equal(acc, base + out)
    # bf16 output (and accumulate into it)
    ob = torch.empty(E, Na, Nb, dtype=torch.bfloat16, device=DEV)
    ops.grouped_wgrad_mxfp8(at, ats, bt, bts, poff, E, ob, ops.ptr_table(ob, E, Na * Nb * 2))
    assert torch.equal(ob, out.bfloat16())
    bb = base.bfloat16()
    ob2 = bb.clone()
    ops.grouped_wgrad_mxfp8(at, ats, bt, bts, poff, E, ob2, ops.ptr_table(ob2, E, Na * Nb * 2), accumulate=True)
    assert torch.equal(ob2, (bb.float() + out).bfloat16())
    # split-K: every padded range cut into P chunks of whole K-tiles, fp32 partials, one sum
    P = 3
    co = ops.chunk_offsets(poff, E, P, 128)
    part = torch.empty(E * P, Na, Nb, device=DEV)
    ops.grouped_wgrad_mxfp8(at, ats, bt, bts, co, E * P, part, ops.ptr_table(part, E * P, Na * Nb * 4))
    summed = ops.sum_partials(part.view(E * P, Na * Nb), E, P, torch.float32).view(E, Na, Nb)
    assert rel_l2(summed.cpu(), emu) <= 2e-3
    assert rel_l2(summed.cpu(), out.cpu()) <= 1e-6


def test_wgrad_dealt_to_the_xcds_under_skewed_routing():
    """64 experts with 8 hot ones, more tiles than CUs: the persistent kernel walks the experts dealt by csmoe_expert_order."""
    E, Na, Nb = 64, 512, 768
    counts = _skewed_counts(E, 64 * 200, 11)
    off, (at, ats, bt, bts, poff), emu, _ = _random_case(counts, Na, Nb, 3)
    order = ops.expert_order(off.to(DEV), E)
    out = torch.empty(E, Na, Nb, device=DEV)
    ops.grouped_wgrad_mxfp8(at, ats, bt, bts, poff, E, out, ops.ptr_table(out, E, Na * Nb * 4), xcd_order=order)
    plain = torch.empty_like(out)
    ops.grouped_wgrad_mxfp8(at, ats, bt, bts, poff, E, plain, ops.ptr_table(plain, E, Na * Nb * 4))
    assert torch.equal(out, plain)
    assert rel_l2(out.cpu(), emu) <= 2e-3


# ---------------------------------------------------------------------------------------------------------------- functions
def _tok_mx_product(a, b):
    """fp64 a^T b of one expert's binned rows, both quantised along the tokens (zero-padded to 128)."""
    off = torch.tensor([0, a.shape[0]], dtype=torch.int32)
    qa, sa, _ = emulate_tokens(a, off)
    qb, sb, _ = emulate_tokens(b, off)
    return MX.dequantize(qa, sa) @ MX.dequantize(qb, sb).t()


def _emu_routed_wgrads(x2, idx, w, keys, values, act, dout, bias):
    """gk, gv of MoEFFNPackedFP8 with wgrad_fp8: the oracle's forward / dH (oracle/mxfp8.py ffn_forward_backward), weight gradients
    of token-dim quantised operands in binned order."""
    f, fgrad = MX._ACT[act]
    E, D, Fh = keys.shape
    wb = MX._bf(w).double()
    kf, vf = keys.float(), values.float()
    k_fwd, v_bwd = MX._mx(kf.transpose(1, 2)), MX._mx(vf)
    xq = MX._mx(x2)
    gk = torch.zeros(E, D, Fh, dtype=torch.float64)
    gv = torch.zeros(E, Fh, values.shape[-1], dtype=torch.float64)
    for e in range(E):
        t, k = (idx == e).nonzero(as_tuple=True)
        if t.numel() == 0:
            continue
        h = xq[t] @ k_fwd[e].t()
        if bias is not None:
            h = h + MX._bf(bias[e]).double()
        h = MX._bf(h)
        a = MX._bf(f(h.float()))
        dy = MX._bf(wb[t, k].unsqueeze(-1) * dout[t].double())
        dh = MX._bf(MX._bf(MX._mx(dy) @ v_bwd[e].t()).double() * fgrad(h))
        gv[e] = _tok_mx_product(a, dy)
        gk[e] = _tok_mx_product(x2[t], dh)
    return gk, gv


def _masked(g, r, col):
    keep = (~col).unsqueeze(-2).expand_as(r) if col is not None else torch.ones_like(r, dtype=torch.bool)
    return rel_l2(g * keep, r * keep)


@pytest.mark.parametrize("actname", ["relu", "gelu"])
def test_ffn_functions_with_fp8_weight_gradients(actname):
    from competesmoe_amd.functional import MoEFFNPackedFP8, DenseFFNFP8
    T, D, Fh, E, K = 384, 256, 384, 8, 2
    g = torch.Generator().manual_seed(21)
    x2 = torch.randn(T, D, generator=g).bfloat16()
    idx = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(T)])
    idx[idx == 5] = 4                                                  # an expert without rows
    w = torch.rand(T, K, generator=g)
    keys, values = torch.randn(E, D, Fh, generator=g) * 0.06, torch.randn(E, Fh, D, generator=g) * 0.05
    bias = torch.randn(E, Fh, generator=g) * 0.1
    dout = torch.randn(T, D, generator=g).bfloat16()
    act = {"relu": L.ACT_RELU, "gelu": L.ACT_GELU}[actname]
    runs = []
    for f8w in (False, True):
        xd, wd, kd, vd, bd = (t.to(DEV).requires_grad_(True) for t in (x2, w, keys, values, bias))
        out = MoEFFNPackedFP8.apply(xd, wd, idx.int().to(DEV), kd, vd, bd, act, L.COMBINE_DOT, False, f8w)
        out.backward(dout.to(DEV))
        runs.append((out.detach(), xd.grad, wd.grad, bd.grad, kd.grad.cpu(), vd.grad.cpu()))
    (o0, dx0, dw0, gb0, gk0, gv0), (o1, dx1, dw1, gb1, gk1, gv1) = runs
    assert torch.equal(o0, o1) and torch.equal(dx0, dx1) and torch.equal(dw0, dw1) and torch.equal(gb0, gb1)
    ref = MX.ffn_forward_backward(x2, idx, w, keys, values, actname, dout, bias=bias)
    col = None
    if actname == "relu":
        col = torch.zeros(E, Fh, dtype=torch.bool)
        for e, (_, f) in ref["near"].items():
            col[e, f] = True
    ek, ev = _emu_routed_wgrads(x2, idx, w, keys, values, actname, dout, bias)
    errs = {"gk": _masked(gk1, ek, col), "gv": rel_l2(gv1, ev), "gk@near": rel_l2(gk1, ek)}
    apart = {"gk": _masked(gk1, gk0.double(), col), "gv": rel_l2(gv1, gv0.double())}
    print("routed", actname, errs, "vs bf16 products", apart)
    assert errs["gk"] <= MX_GRAD and errs["gv"] <= MX_GRAD and errs["gk@near"] <= LOOSE, errs
    assert apart["gk"] > MX_GRAD and apart["gv"] > MX_GRAD, apart                  # the test tells the two paths apart
    assert float(gk1[5].abs().max()) == 0.0 and float(gv1[5].abs().max()) == 0.0
    # the shared expert (dense form, E = 1), width 2F
    w1, w2 = torch.randn(D, 2 * Fh, generator=g) * 0.06, torch.randn(2 * Fh, D, generator=g) * 0.04
    runs = []
    for f8w in (False, True):
        xs, w1d, w2d = (t.to(DEV).requires_grad_(True) for t in (x2, w1, w2))
        y = DenseFFNFP8.apply(xs, w1d, None, w2d, act, False, f8w)
        y.backward(dout.to(DEV))
        runs.append((y.detach(), xs.grad, w1d.grad.cpu(), w2d.grad.cpu()))
    (y0, dxs0, gw10, gw20), (y1, dxs1, gw11, gw21) = runs
    assert torch.equal(y0, y1) and torch.equal(dxs0, dxs1)
    rd = MX.dense_ffn_forward_backward(x2, w1, w2, actname, dout)
    col = None
    if actname == "relu":
        col = torch.zeros(1, 2 * Fh, dtype=torch.bool)
        for e, (_, f) in rd["near"].items():
            col[0, f] = True
        col = col[0]
    ek, ev = _emu_routed_wgrads(x2, torch.zeros(T, 1, dtype=torch.long), torch.ones(T, 1), w1[None], w2[None], actname, dout, None)
    errs = {"gw1": _masked(gw11, ek[0], col), "gw2": rel_l2(gw21, ev[0])}
    apart = {"gw1": _masked(gw11, gw10.double(), col), "gw2": rel_l2(gw21, gw20.double())}
    print("shared", actname, errs, "vs bf16 products", apart)
    assert errs["gw1"] <= MX_GRAD and errs["gw2"] <= MX_GRAD, errs
    assert apart["gw1"] > MX_GRAD and apart["gw2"] > MX_GRAD, apart


# ---------------------------------------------------------------------------------------------------------------- layer
_LAYER_SNIPPET = r"""
import sys, types, torch, torch.nn.functional as F
sys.path.insert(0, {root!r})
from competesmoe_amd.pretrain import get_moe

def run(name, fp8_wgrad, pass_flag):
    D, Fh, E, K, B, N = 256, 384, 16, 3, 2, 192
    args = types.SimpleNamespace(balance_loss_coef=0.01, fp8_experts=True, n_shared_experts=2, test_only=False)
    if pass_flag:
        args.fp8_wgrad = fp8_wgrad
    torch.manual_seed(4)
    lay = get_moe(name)(D, E, Fh, n_heads=K, activation=F.relu, log_interval=None, args=args).to("cuda").train()
    lay.regularization_present = True
    g = torch.Generator().manual_seed(10)
    x = torch.randn(B, N, D, generator=g)
    dy = torch.randn(B, N, D, generator=g)
    xg = x.to("cuda").requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = lay(xg)
        reg = sum(lay.get_reg_loss().values())
    ((out.float() * dy.to("cuda")).sum() + reg.float()).backward()
    res = {{"out": out.detach().float().cpu(), "dx": xg.grad.cpu(), "fp8_wgrad": lay.fp8_wgrad}}
    for k, p in lay.named_parameters():
        res["p." + k] = None if p.grad is None else p.grad.cpu()
    return res
"""


def _layer_ns():
    ns = {}
    exec(_LAYER_SNIPPET.format(root=ROOT), ns)
    return ns


@pytest.mark.parametrize("name", ["deepseekv2", "deepseekv3"])
def test_layer_with_fp8_weight_gradients(name, tmp_path):
    ns = _layer_ns()
    base = ns["run"](name, False, True)
    f8 = ns["run"](name, True, True)
    assert f8["fp8_wgrad"] and not base["fp8_wgrad"]
    assert torch.equal(base["out"], f8["out"]) and torch.equal(base["dx"], f8["dx"])
    expert = ("p.keys", "p.values", "p.keys_shared", "p.values_shared")
    for k, v in base.items():
        if not k.startswith("p.") or v is None:
            continue
        assert torch.isfinite(f8[k]).all(), k
        if k in expert:
            # the format's own error against the bf16 products (tests/test_fp8_gpu.py: <= 6e-2 against unquantised operands)
            err = rel_l2(f8[k], v.double())
            print(name, k, f"fp8 vs bf16 weight gradient {err:.2e}")
            assert MX_GRAD < err <= 6e-2, (k, err)
        else:
            assert torch.equal(f8[k], v), k
    if name == "deepseekv2":
        # the environment default, read once per process: a fresh child with CSMOE_FP8_WGRAD=1 and no args.fp8_wgrad
        out = tmp_path / "child.pt"
        code = _LAYER_SNIPPET.format(root=ROOT) + f"\ntorch.save(run({name!r}, None, False), {str(out)!r})\n"
        env = dict(os.environ, CSMOE_FP8_WGRAD="1")
        subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=600, cwd=ROOT)
        child = torch.load(str(out))
        assert child["fp8_wgrad"]
        for k in expert + ("out", "dx"):
            assert torch.equal(child[k], f8[k]), k
