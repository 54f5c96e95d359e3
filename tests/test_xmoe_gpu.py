"""GPU tests of the XMoE cosine router: the one-pass kernel (csmoe_cosine_select), its backward (csmoe_cosine_select_bwd), the
selection rule CSMOE_SEL_TEMP_SOFTMAX_TOPK, and both `xmoe` layers against the fixtures captured from the reference classes
(tests/golden/make_golden_xmoe.py) and the test-side restatement pinned to them (tests/xmoe_ref.py, tests/test_xmoe_cpu.py).

Bounds.  (a) is exact.  (b) is derived: half an ulp of bf16 at the value's magnitude plus R * 2^-23 * sum|terms| for the fp32 chain.
(c) uses the bounds the two stacks' module tests already use (tests/test_llava_modules_gpu.py:3-5, tests/test_pretrain_modules_gpu.py
:5-8): LLaVA fp32 <= 1e-5 of max|ref|, bf16 <= 1e-3 relative L2 and <= 2 bf16 ulp of max|ref|; pretrain fp32 outputs <= 1e-5,
gradients <= 4e-5 relative L2, bf16 outputs of same-routed rows <= 2e-4, gradients <= 2e-3; rows routed unlike the fixture: 0 for
fp32, <= 1 % for bf16.  (d) compares two bf16 computations that round at the same points: 2e-3 relative L2, the bf16 gradient
bound of (c).  (e) holds the two forms of each layer to that layer's bf16 bounds of (c), the LLaVA stack's elementwise one included."""
import os
import subprocess
import sys
import tempfile
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import xmoe_ref as X
from tests.golden_util import load, rel_l2, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from competesmoe_amd import _lib as L, ops
    from competesmoe_amd.functional import CosineSelect
    from competesmoe_amd.moe import get_moe as llava_get
    from competesmoe_amd.pretrain import get_moe as pretrain_get

FLAG_SETS = [3, 4]          # the LLaVA bf16 module (p and the K-softmax in bf16), the pretrain stack under bf16 autocast (bf16 operands)
BF16_BAD_ROWS = 0.01


def _inputs(T, D, E, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(T, D, generator=g, device=DEV).to(torch.bfloat16)
    wr = (torch.randn(E // 2, D, generator=g, device=DEV) * D ** -0.5).to(torch.bfloat16)
    emb = X.renorm(torch.randn(E, E // 2, generator=g, device=DEV))
    return x, wr, emb.contiguous()


# ------------------------------------------------------------------------------------------------ (a) exact anchors
@pytest.mark.parametrize("D", [64, 264, 4096])
@pytest.mark.parametrize("T", [1, 63, 64, 1000, 32768])
def test_a_exact_anchors(T, D):
    """`reduced` carries the bits of csmoe_gate_logits(x, expert_sel); (p, idx, w) the bits of csmoe_router_select (rule 5) on the
    kernel's own logits; block_hist is the histogram of idx.  E in {4, 8, 16, 64}, K in {1, 2, 4}, both flag sets."""
    rows = int(L.lib.csmoe_gate_select_rows())
    wrong = []
    for E in (4, 8, 16, 64):
        x, wr, emb = _inputs(T, D, E, seed=E)
        want_red = ops.gate_logits(x, wr)
        for K in (1, 2, 4):
            for flags in FLAG_SETS:
                red, lg, p, idx, w, status = ops.cosine_select(x, wr, emb, K, flags)
                p2, idx2, w2 = ops.router_select(lg, K, L.SEL_TEMP_SOFTMAX_TOPK, flags & 3, param=0.3)
                hist = ops._ROUTE_HIST[2]
                blk = torch.arange(T, device=DEV).div(rows, rounding_mode="floor").unsqueeze(1) * E + idx.long()
                want = torch.bincount(blk.flatten(), minlength=hist.numel()).view_as(hist)
                got = dict(reduced=torch.equal(red, want_red), idx=torch.equal(idx, idx2), p=torch.equal(p, p2), w=torch.equal(w, w2),
                           hist=torch.equal(hist.long(), want), status=int(status) == 0)
                wrong += [(E, K, flags, k) for k, ok in got.items() if not ok]
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------ (b) cosine stage
def _m32_like_kernel(red):
    """The normalised row in fp32 exactly as the kernel forms it: squares of elements l and l + 16 added inside the lane, then the
    16-lane tree (partners 8, 4, 2, 1), IEEE sqrt and division."""
    T, R = red.shape
    v = torch.zeros(T, 32, device=red.device)
    v[:, :R] = red.float()
    s = v[:, :16] * v[:, :16] + v[:, 16:] * v[:, 16:]
    for sh in (8, 4, 2, 1):
        s = s + s.roll(-sh, -1)
    den = s[:, :1].sqrt().clamp_min(1e-4)
    return v[:, :R] / den


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("E", [4, 8, 16, 64])
def test_b_cosine_stage_against_fp64(E, flags):
    """|logit - fp64 value| <= half a bf16 ulp at the value's magnitude + R * 2^-23 * sum|terms|, the fp64 value evaluated from the
    kernel's own `reduced` (and, under the bf16-operand flag, from the operands rounded as the kernel rounds them)."""
    T, D, R = 1000, 264, E // 2
    x, wr, emb = _inputs(T, D, E, seed=3)
    red, lg, *_ = ops.cosine_select(x, wr, emb, 2, flags)
    m = _m32_like_kernel(red)
    e = emb
    if flags & L.COS_OPER_BF16:
        m, e = m.to(torch.bfloat16).float(), e.to(torch.bfloat16).float()
    terms = m.double().unsqueeze(1) * e.double().unsqueeze(0)              # [T, E, R]
    exact = terms.sum(-1)
    mag = torch.maximum(exact.abs(), lg.double().abs()).clamp_min(2.0 ** -126)
    half_ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7) / 2            # bf16: 8 significant bits
    bound = half_ulp + R * 2.0 ** -23 * terms.abs().sum(-1)
    err = (lg.double() - exact).abs()
    print(f"E={E} flags={flags}: max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------------------------------------ (c) layers against the fixtures
def _llava_layer(fx):
    m = fx["meta"]
    ex = nn.ModuleList([nn.Sequential(nn.Linear(m["D"], m["F"]), nn.GELU(), nn.Linear(m["F"], m["Dout"])) for _ in range(m["E"])])
    layer = llava_get("xmoe")(m["D"], m["Dout"], m["E"], m["K"], ex, types.SimpleNamespace(**m["args"]))
    layer.load_state_dict(fx["state"], strict=True)
    dt = torch.float32 if m["dtype"] == "float32" else torch.bfloat16
    return layer.to(DEV).to(dt).train(), dt


def _pretrain_layer(fx):
    m = fx["meta"]
    layer = pretrain_get("xmoe")(m["D"], m["E"], m["F"], n_heads=m["K"], activation=F.relu, bias=m["bias"], sel_bias=m["sel_bias"],
                                 log_interval=None, args=types.SimpleNamespace(**m["args"]))
    layer.load_state_dict(fx["state"], strict=True)
    layer = layer.to(DEV).train()
    layer.regularization_present = True
    return layer


def _spy(layer, name, pos):
    seen = []
    fn = getattr(layer, name)

    def spy(*a, **k):
        seen.append(a[pos].detach().clone())
        return fn(*a, **k)
    setattr(layer, name, spy)
    return seen


def _llava_step(layer, fx):
    x = fx["x"].to(DEV).requires_grad_(True)
    out, aux, none, infor = layer(x)
    assert none is None
    ((out.float() * fx["dy"].to(DEV).float()).sum() + aux.float()).backward()
    return x, out, aux, infor


def _pretrain_step(layer, fx):
    x = fx["x"].to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=fx["meta"]["bf16"]):
        out = layer(x)
        reg = layer.get_reg_loss()
    ((out.float() * fx["dy"].to(DEV)).sum() + sum(v.float() for v in reg.values())).backward()
    return x, out, reg


def _restated_grads(fx, idx, stack):
    ps = {k: v.clone() for k, v in fx["state"].items()}
    ps["expert_embeddings"] = X.renorm(ps["expert_embeddings"])
    ps = {k: v.requires_grad_(True) for k, v in ps.items()}
    x = fx["x"].clone().requires_grad_(True)
    idx = idx.cpu().long().view(*x.shape[:-1], -1)
    if stack == "llava":
        out, aux, _ = X.llava_forward(x, ps, fx["meta"], forced_idx=idx)
        ((out.float() * fx["dy"].float()).sum() + aux.float()).backward()
    else:
        out, reg, _ = X.pretrain_forward(x, ps, fx["meta"], forced_idx=idx)
        ((out.float() * fx["dy"]).sum() + reg.float()).backward()
    return out.detach(), x.grad, {k: p.grad for k, p in ps.items()}


def _emb_after_ok(layer, fx):
    a, b = layer.expert_embeddings.detach().cpu(), fx["expert_embeddings_after"]
    assert a.dtype == b.dtype
    if a.dtype == torch.float32:
        assert max_rel(a, b) <= 1e-6, max_rel(a, b)
    else:       # the norm of a bf16 row is an fp32 sum rounded once: the device's summation order may move it by one bf16 ulp
        assert float(((a.float() - b.float()).abs() / b.float().abs()).max()) <= 2.0 ** -7


@pytest.mark.parametrize("tag", ["fp32", "bf16"])
def test_c_llava_layer_matches_fixture(tag):
    """Observed on the MI355X (the prints below): no row routed unlike the fixture; fp32 outputs 3.4e-7 of max|ref|, gradients
    <= 4.3e-7; bf16 outputs and the gradients of `expert_embeddings`, `inp_reduction` and all but three expert matrices the
    reference's bits, d x 3.9e-5 relative L2 / 7.1e-4 of max|ref|, the other three <= 1.1e-5 / 1.4e-4."""
    fx = load(f"llava_xmoe_{tag}")
    layer, dt = _llava_layer(fx)
    seen = _spy(layer, "compute_moe", 0)
    x, out, aux, infor = _llava_step(layer, fx)
    assert out.dtype == dt and out.shape == fx["output"].shape
    _emb_after_ok(layer, fx)
    K = fx["meta"]["K"]
    idx = seen[0].reshape(-1, K)
    same = (idx.long().sort(-1).values.cpu() == fx["selected_experts"].reshape(-1, K).sort(-1).values).all(-1)
    bad = float((~same).float().mean())
    print(f"llava {tag}: rows routed unlike the fixture {bad:.4f}")
    assert bad <= (0.0 if dt == torch.float32 else BF16_BAD_ROWS), bad
    ref_out, ref_xg, ref_g = fx["output"], fx["x_grad"], fx["grads"]
    if bad > 0:
        # a row routed unlike the fixture: the restatement under the KERNEL's indices (its autograd is pinned to the fixtures'
        # recorded gradients by tests/test_xmoe_cpu.py).  Otherwise the reference is the fixture itself.
        ref_out, ref_xg, ref_g = _restated_grads(fx, idx, "llava")
    rl, mr = (1e-5, 1e-5) if dt == torch.float32 else (1e-3, 2 * 2 ** -8)
    o = out.detach().cpu().reshape(-1, out.shape[-1])[same]
    g = fx["output"].reshape(-1, out.shape[-1])[same]
    print(f"llava {tag}: out rel-L2 {rel_l2(o, g):.2e} max-rel {max_rel(o, g):.2e}")
    assert max_rel(o, g) <= mr and (dt == torch.float32 or rel_l2(o, g) <= rl)
    assert abs(float(aux) - float(fx["aux_loss"])) <= (2e-5 if dt == torch.float32 else 2e-3) * max(1.0, abs(float(fx["aux_loss"])))
    assert set(infor) == set(fx["infor_aux"])

    def check(name, a, b):
        print(f"llava {tag}: d {name} rel-L2 {rel_l2(a, b):.2e} max-rel {max_rel(a, b):.2e}")
        assert max_rel(a, b) <= mr, (name, max_rel(a, b))
        assert dt == torch.float32 or rel_l2(a, b) <= rl, (name, rel_l2(a, b))
    check("x", x.grad.cpu(), ref_xg)
    for name, p in layer.named_parameters():
        g = ref_g.get(name)
        if g is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        check(name, p.grad.cpu(), g)


@pytest.mark.parametrize("name", ["xmoe_fp32", "xmoe_bf16", "xmoe_selbias_fp32"])
def test_c_pretrain_layer_matches_fixture(name):
    """Observed on the MI355X (the prints below): no row routed unlike the fixture; fp32 (with and without `sel_bias`) outputs
    <= 3.2e-7 of max|ref|, gradients <= 7.2e-7 relative L2; bf16 autocast outputs, d x, d `expert_sel` and d `expert_embeddings`
    the reference's bits, d keys / d values 2.2e-8 relative L2 (bound 2e-3: what the torch-op gate of `smoe_perturbed` needs)."""
    fx = load(f"pretrain_{name}")
    bf16 = fx["meta"]["bf16"]
    layer = _pretrain_layer(fx)
    seen = _spy(layer, "ffn", 1)
    x, out, reg = _pretrain_step(layer, fx)
    assert out.dtype == fx["output"].dtype and set(reg) == set(fx["reg_loss"])
    _emb_after_ok(layer, fx)
    K = fx["meta"]["K"]
    idx = seen[0].reshape(-1, K)
    same = (idx.long().sort(-1).values.cpu() == fx["selected_experts"].reshape(-1, K).sort(-1).values).all(-1)
    bad = float((~same).float().mean())
    print(f"pretrain {name}: rows routed unlike the fixture {bad:.4f}")
    assert bad <= (BF16_BAD_ROWS if bf16 else 0.0), bad
    o = out.detach().cpu().reshape(-1, out.shape[-1])[same]
    g = fx["output"].reshape(-1, out.shape[-1])[same]
    print(f"pretrain {name}: out rel-L2 {rel_l2(o, g):.2e} max-rel {max_rel(o, g):.2e}")
    if bf16:
        assert rel_l2(o, g) <= 2e-4, rel_l2(o, g)
    else:
        assert max_rel(o, g) <= 1e-5, max_rel(o, g)
    for k, v in fx["reg_loss"].items():
        assert abs(float(reg[k]) - float(v)) <= (2e-6 if not bf16 else 2e-5 * (1 + 20 * (bad > 0))) + 1e-4 * abs(float(v)), k
    ref_xg, ref_g = fx["x_grad"], fx["grads"]
    if bad > 0:
        _, ref_xg, ref_g = _restated_grads(fx, idx, "pretrain")
    tol = 2e-3 if bf16 else 4e-5
    print(f"pretrain {name}: d x rel-L2 {rel_l2(x.grad.cpu(), ref_xg):.2e}")
    assert rel_l2(x.grad.cpu(), ref_xg) <= tol, rel_l2(x.grad.cpu(), ref_xg)
    for pname, p in layer.named_parameters():
        g = ref_g.get(pname)
        if g is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, pname
            continue
        print(f"pretrain {name}: d {pname} rel-L2 {rel_l2(p.grad.cpu(), g):.2e}")
        assert rel_l2(p.grad.cpu(), g) <= tol, (pname, rel_l2(p.grad.cpu(), g))


# ------------------------------------------------------------------------------------------------ (d) backward kernel
@pytest.mark.parametrize("nulls", ["all", "no_dp", "no_dlogits", "only_dlogits", "only_dp"])
@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("E,K", [(8, 2), (64, 4), (4, 1)])
def test_d_backward_kernel_against_autograd_of_the_restatement(E, K, flags, nulls):
    T, R = 777, E // 2
    g = torch.Generator().manual_seed(11)                                     # the restatement runs where it is pinned: on the CPU
    red = torch.randn(T, R, generator=g).to(torch.bfloat16)
    red[5] = 0                                                                # clamped norm: the gradient is d m / eps there
    emb = X.renorm(torch.randn(E, R, generator=g)).contiguous()
    red_l, emb_l = red.clone().requires_grad_(True), emb.clone().requires_grad_(True)
    cos, p, idx, w = X.row_half(red_l, emb_l, K, flags)
    dw = torch.randn(T, K, generator=g) if nulls in ("all", "no_dp", "no_dlogits") else None
    dp = torch.randn(T, E, generator=g) if nulls in ("all", "no_dlogits", "only_dp") else None
    dl = (torch.randn(T, E, generator=g) * 0.1).to(torch.bfloat16) if nulls in ("all", "no_dp", "only_dlogits") else None
    if flags & X.P_BF16 and dp is not None:
        dp = dp.to(torch.bfloat16).float()          # the gradient of a bf16 tensor is a bf16 tensor
    if flags & X.W_BF16 and dw is not None:
        dw = dw.to(torch.bfloat16).float()
    loss = 0
    if dw is not None:
        loss = loss + (w.float() * dw).sum()
    if dp is not None:
        loss = loss + (p.float() * dp).sum()
    if dl is not None:
        loss = loss + (cos.float() * dl.float()).sum()
    loss.backward()
    dev = lambda t: None if t is None else t.detach().to(DEV).contiguous()
    red, emb, cos, dw, dp, dl = dev(red), dev(emb), dev(cos), dev(dw), dev(dp), dev(dl)
    idx, w = dev(idx), dev(w)
    g_red, g_emb = red_l.grad.to(DEV), emb_l.grad.to(DEV)
    d_red, d_emb = ops.cosine_select_bwd(red, emb, cos.detach().contiguous(), idx.int().contiguous(), w.detach().float().contiguous(),
                                         dw, dp, dl, K, flags)
    if flags & L.COS_OPER_BF16:
        d_emb = d_emb.to(torch.bfloat16).float()
    keep = torch.arange(T, device=DEV) != 5            # row 5's gradient is 1 / eps times larger: compared on its own below
    e1, e2 = rel_l2(d_red[keep], g_red[keep]), rel_l2(d_emb, g_emb)
    print(f"E={E} K={K} flags={flags} {nulls}: d_reduced {e1:.2e} d_emb {e2:.2e}")
    assert e1 <= 2e-3 and e2 <= 2e-3, (e1, e2)
    assert bool(d_red[5].isfinite().all()) and rel_l2(d_red[5], g_red[5]) <= 2e-3


# ------------------------------------------------------------------------------------------------ (e) fused against unfused
def _run_both_layers():
    res = {}
    for stack, name in (("llava", "llava_xmoe_bf16"), ("pretrain", "pretrain_xmoe_bf16")):
        fx = load(name)
        if stack == "llava":
            layer, _ = _llava_layer(fx)
            seen = _spy(layer, "compute_moe", 0)
            x, out, *_ = _llava_step(layer, fx)
        else:
            layer = _pretrain_layer(fx)
            seen = _spy(layer, "ffn", 1)
            x, out, _ = _pretrain_step(layer, fx)
        res[stack] = dict(idx=seen[0].cpu(), out=out.detach().float().cpu(), dx=x.grad.float().cpu(),
                          grads={k: p.grad.float().cpu() for k, p in layer.named_parameters() if p.grad is not None})
    return res


def _child(path):
    assert os.environ.get("CSMOE_FUSED_ROUTER") == "0"
    torch.save(_run_both_layers(), path)


def test_e_fused_against_unfused():
    """CSMOE_FUSED_ROUTER is read per call but belongs to the process: the torch-op form runs in a fresh child process."""
    fused = _run_both_layers()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "unfused.pt")
        env = dict(os.environ, CSMOE_FUSED_ROUTER="0")
        subprocess.run([sys.executable, "-c", f"import tests.test_xmoe_gpu as t; t._child({path!r})"], cwd=ROOT, env=env, check=True,
                       timeout=600)
        unfused = torch.load(path, weights_only=True)
    ulp2 = 2 * 2.0 ** -8                 # the LLaVA stack's second bf16 bound of (c): 2 bf16 ulp of max|ref|, elementwise
    for stack in ("llava", "pretrain"):
        a, b = fused[stack], unfused[stack]
        assert torch.equal(a["idx"], b["idx"]), f"{stack}: the two forms route differently"

        def check(name, u, v, tol):
            e, m = rel_l2(u, v), max_rel(u, v)
            print(f"{stack}: fused vs unfused {name} rel-L2 {e:.2e} max-rel {m:.2e}")
            assert e <= tol, (stack, name, e)
            assert stack != "llava" or m <= ulp2, (stack, name, m)
        check("out", a["out"], b["out"], 1e-3 if stack == "llava" else 2e-4)
        tol = 1e-3 if stack == "llava" else 2e-3
        check("d x", a["dx"], b["dx"], tol)
        assert set(a["grads"]) == set(b["grads"])
        for k in a["grads"]:
            check(f"d {k}", a["grads"][k], b["grads"][k], tol)


# ------------------------------------------------------------------------------------------------ (f) a non-finite input row
def test_f_non_finite_row_routes_like_the_restatement():
    """One x row holds inf: its logits become the smallest finite logit of the tensor, it routes to experts 0..K-1 with weights
    1/K -- a numeric case handled without a host synchronisation; a finite run leaves the counter at zero."""
    fx = load("llava_xmoe_bf16")
    m = fx["meta"]
    B, N, E, K = m["B"], m["N"], m["E"], m["K"]
    x = fx["x"].clone()
    layer, dt = _llava_layer(fx)
    with torch.no_grad():
        layer(x.to(DEV))
    assert int(CosineSelect.last_status) == 0
    x[1, 7, 3] = float("inf")
    layer, dt = _llava_layer(fx)        # a fresh layer: every forward rescales the embeddings again
    routed = []
    route0 = layer.route

    def route_spy(x_):
        routed.append(route0(x_))
        return routed[-1]
    layer.route = route_spy
    with torch.no_grad():
        out = layer(x.to(DEV))[0]
    logits, p, idx, w = routed[0]
    assert int(CosineSelect.last_status) == 1
    ps = dict(fx["state"])
    ps["expert_embeddings"] = X.renorm(ps["expert_embeddings"])
    with torch.no_grad():
        ref_out, _, st = X.llava_forward(x, ps, m)
    row = 1 * N + 7
    lg, rl_ = logits.reshape(-1, E).cpu(), st["gate_logits"].reshape(-1, E)
    assert bool(lg.isfinite().all())
    # the row's logits: E copies of the tensor's smallest finite logit (of THIS run's logits)
    others = torch.cat([lg[:row], lg[row + 1:]])
    assert torch.equal(lg[row], others.min().expand(E))
    # Every logit against the restatement's: one bf16 ulp at |cos| <= 1.5 (the embeddings' row norm), not equality.  The restatement
    # runs on the CPU, whose matmul adds the R fp32 terms in an order of its own; the kernel adds them over ascending r (bounded
    # against fp64 in (b)).  Two fp32 sums that differ in the last bits can fall on either side of a bf16 rounding boundary.
    assert float((lg.float() - rl_.float()).abs().max()) <= 2.0 ** -7 * 1.5
    assert idx.reshape(-1, K)[row].tolist() == st["selected_experts"].reshape(-1, K)[row].tolist() == list(range(K))
    assert torch.equal(w.reshape(-1, K)[row].cpu(), st["weights"].reshape(-1, K)[row].float())
    assert torch.equal(p.reshape(-1, E)[row].cpu(), st["gate_softmax"].reshape(-1, E)[row])
    same = (idx.reshape(-1, K).long().sort(-1).values.cpu() == st["selected_experts"].reshape(-1, K).sort(-1).values).all(-1)
    assert float((~same).float().mean()) <= BF16_BAD_ROWS
    same[row] = False
    o, g = out.reshape(-1, out.shape[-1]).cpu(), ref_out.reshape(-1, out.shape[-1])
    assert bool(o[same].isfinite().all()) and rel_l2(o[same], g[same]) <= 1e-3
    assert not bool(o[row].isfinite().all()) and not bool(g[row].isfinite().all())      # the experts see the inf, here as there


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("K", [2, 4])
def test_f_non_finite_rows_in_the_mfma_kernel(K, flags):
    """E = 64 (the MFMA kernel), three rows with an inf: two in one 64-row block, one ten blocks further, so the patch launch walks
    its block loop past clean blocks and rewrites two rows of one block.  The flagged rows hold E copies of the smallest finite
    logit, route to experts 0..K-1 with weights 1/K and p = 1/E (all exact in bf16 and fp32) as the restatement routes them; every
    other row carries the bits of the same call on finite input; the counter holds 3."""
    T, D, E = 1000, 264, 64
    bad_rows = [5, 6, 700]
    x, wr, emb = _inputs(T, D, E, seed=9)
    clean = [t.clone() for t in ops.cosine_select(x, wr, emb, K, flags)]
    assert int(clean[5]) == 0
    xb = x.clone()
    for n, t in enumerate(bad_rows):
        xb[t, 17 * n + 3] = float("inf") if n != 1 else float("-inf")
    red, lg, p, idx, w, status = ops.cosine_select(xb, wr, emb, K, flags)
    hist = ops._ROUTE_HIST[2].clone()
    assert int(status) == len(bad_rows)
    keep = torch.ones(T, dtype=torch.bool, device=DEV)
    keep[bad_rows] = False
    for name, a, b in zip(("reduced", "logits", "p", "idx", "w"), (red, lg, p, idx, w), clean):
        assert torch.equal(a[keep], b[keep]), name
    assert not bool(red[bad_rows].isfinite().any()) and bool(lg.isfinite().all())
    assert torch.equal(lg[bad_rows], lg[keep].min().expand(len(bad_rows), E))
    _, rp, ridx, rw = X.row_half(red, emb, K, flags)                        # the restatement on the kernel's own `reduced`
    assert torch.equal(idx[bad_rows].long(), ridx[bad_rows]) and idx[bad_rows[0]].tolist() == list(range(K))
    assert torch.equal(w[bad_rows], rw[bad_rows].float()) and float(w[bad_rows[0], 0]) == 1.0 / K
    assert torch.equal(p[bad_rows], rp[bad_rows].float()) and float(p[bad_rows[0], 0]) == 1.0 / E
    rows = int(L.lib.csmoe_gate_select_rows())
    blk = torch.arange(T, device=DEV).div(rows, rounding_mode="floor").unsqueeze(1) * E + idx.long()
    assert torch.equal(hist.long(), torch.bincount(blk.flatten(), minlength=hist.numel()).view_as(hist))


# ------------------------------------------------------------------------------------------------ (g) determinism
def test_g_two_identical_steps_are_bit_identical():
    a, b = _run_both_layers(), _run_both_layers()
    for stack in a:
        assert torch.equal(a[stack]["idx"], b[stack]["idx"]) and torch.equal(a[stack]["out"], b[stack]["out"])
        assert torch.equal(a[stack]["dx"], b[stack]["dx"])
        for k in a[stack]["grads"]:
            assert torch.equal(a[stack]["grads"][k], b[stack]["grads"][k]), (stack, k)
    # the backward kernel at a size where many workgroups contribute partial tables of d emb
    T, E, K = 20000, 64, 2
    g = torch.Generator(device=DEV).manual_seed(5)
    red = torch.randn(T, E // 2, generator=g, device=DEV).to(torch.bfloat16)
    emb = X.renorm(torch.randn(E, E // 2, generator=g, device=DEV)).contiguous()
    with torch.no_grad():
        cos, p, idx, w = X.row_half(red, emb, K, 3)
    dw, dp = torch.randn(T, K, generator=g, device=DEV), torch.randn(T, E, generator=g, device=DEV)
    runs = [ops.cosine_select_bwd(red, emb, cos.contiguous(), idx.int().contiguous(), w.float().contiguous(), dw, dp, None, K, 3)
            for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])


# ------------------------------------------------------------------------------------------------ (h) no host synchronisation
@pytest.mark.parametrize("stack", ["llava", "pretrain"])
def test_h_step_has_no_host_synchronisation(stack):
    fx = load(f"{stack}_xmoe_bf16")
    if stack == "llava":
        layer, _ = _llava_layer(fx)
        step = lambda x: _llava_fwd_bwd(layer, x, dy)
    else:
        layer = _pretrain_layer(fx)
        step = lambda x: _pretrain_fwd_bwd(layer, x, dy, fx["meta"]["bf16"])
    dy = fx["dy"].to(DEV)
    dy = dy.float() if stack == "llava" else dy
    x0 = fx["x"].to(DEV)
    step(x0.clone().requires_grad_(True))             # the first step builds the per-expert pointer tables (host-to-device copies)
    torch.cuda.synchronize()
    x1 = x0.clone().requires_grad_(True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        step(x1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(x1.grad.isfinite().all())


def _llava_fwd_bwd(layer, x, dy):
    out, aux, _, _ = layer(x)
    ((out.float() * dy).sum() + aux.float()).backward()


def _pretrain_fwd_bwd(layer, x, dy, bf16):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        out = layer(x)
        reg = layer.get_reg_loss()
    ((out.float() * dy).sum() + sum(v.float() for v in reg.values())).backward()
