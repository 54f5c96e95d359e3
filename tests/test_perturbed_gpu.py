"""GPU tests of the perturbed-cosine router (`smoe_perturbed`): the second normalisation mode of the one-pass kernel
(csmoe_cosine_select with CSMOE_COS_NORM_THETA / CSMOE_COS_NORM_BF16), its backward (csmoe_cosine_select_bwd), and both layers
against the fixtures captured from the reference classes (tests/golden/make_golden_perturbed.py) and the test-side restatement pinned
to them (tests/perturbed_ref.py, tests/test_perturbed_cpu.py).

Flag sets: 27 = P_BF16 | W_BF16 | NORM_THETA | NORM_BF16, the LLaVA bf16 module; 12 = OPER_BF16 | NORM_THETA, the pretrain stack under
bf16 autocast.

Bounds.  (a) is exact.  (b) is derived: half an ulp of bf16 at the value's magnitude plus R * 2^-23 * sum|terms| for the fp32 chain.
(c) uses the bounds of tests/test_xmoe_gpu.py (c): LLaVA fp32 <= 1e-5 of max|ref|, bf16 <= 1e-3 relative L2 and <= 2 bf16 ulp of
max|ref|; pretrain fp32 outputs <= 1e-5, gradients <= 4e-5 relative L2, bf16 outputs of same-routed rows <= 2e-4, gradients <= 2e-3;
rows routed unlike the fixture: 0 for fp32, <= 1 % for bf16.  (d) compares two bf16 computations that round at the same points: 2e-3
relative L2, the project's bf16 gradient bound.  (e) holds the two forms of each layer to that layer's bf16 bounds of (c).

theta of the LLaVA bf16 fixtures.  The fixtures are runs on the CPU, where torch's kernel for `bf16 tensor + Python scalar` rounds
the scalar to bf16 first (0.1 -> 0.10009765625); the GPU's kernel keeps 0.1f.  The two sums can differ by one bf16 ulp of `norm +
theta` in rare rows (most often at R = 2).  Tests that compare a bf16 LLaVA layer, or the kernel under NORM_BF16, with a CPU run hand
theta = bf16(0.1) to both sides, where the two agree exactly; the layer's default stays 0.1, and (e) runs that value too."""
import os
import subprocess
import sys
import tempfile
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import perturbed_ref as P
from tests.golden_util import load, rel_l2, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from competesmoe_amd import _lib as L, ops
    from competesmoe_amd.functional import CosineSelect, cosine_route_unfused
    from competesmoe_amd.moe import get_moe as llava_get
    from competesmoe_amd.pretrain import get_moe as pretrain_get

FLAG_SETS = [27, 12]
BF16_BAD_ROWS = 0.01
THETA = 0.1
THETA_BF16 = float(torch.tensor(0.1).bfloat16())        # 0.10009765625: see the module docstring


def _inputs(T, D, E, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(T, D, generator=g, device=DEV).to(torch.bfloat16)
    wr = (torch.randn(E // 2, D, generator=g, device=DEV) * D ** -0.5).to(torch.bfloat16)
    emb = P.renorm(torch.randn(E, E // 2, generator=g, device=DEV))
    return x, wr, emb.contiguous()


# ------------------------------------------------------------------------------------------------ (a) exact anchors
@pytest.mark.parametrize("D", [64, 264, 4096])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 1000])
def test_a_exact_anchors(T, D):
    """`reduced` carries the bits of csmoe_gate_logits(x, expert_sel); (p, idx, w) the bits of csmoe_router_select (rule 5) on the
    kernel's own logits; block_hist is the histogram of idx; the status is 0.  E in {4, 8, 16, 64}, K in {1, 2, 4}, both flag sets."""
    rows = int(L.lib.csmoe_gate_select_rows())
    wrong = []
    for E in (4, 8, 16, 64):
        x, wr, emb = _inputs(T, D, E, seed=E)
        want_red = ops.gate_logits(x, wr)
        for K in (1, 2, 4):
            for flags in FLAG_SETS:
                red, lg, p, idx, w, status = ops.cosine_select(x, wr, emb, K, flags, 0.3, THETA)
                hist = ops._ROUTE_HIST[2]
                p2, idx2, w2 = ops.router_select(lg, K, L.SEL_TEMP_SOFTMAX_TOPK, flags & 3, param=0.3)
                blk = torch.arange(T, device=DEV).div(rows, rounding_mode="floor").unsqueeze(1) * E + idx.long()
                want = torch.bincount(blk.flatten(), minlength=hist.numel()).view_as(hist)
                got = dict(reduced=torch.equal(red, want_red), idx=torch.equal(idx, idx2), p=torch.equal(p, p2), w=torch.equal(w, w2),
                           hist=torch.equal(hist.long(), want), status=int(status) == 0, finite=bool(lg.isfinite().all()))
                wrong += [(E, K, flags, k) for k, ok in got.items() if not ok]
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------ (b) cosine stage
def _m32_like_kernel(red, flags, theta):
    """The normalised row in fp32 exactly as the kernel forms it: squares of elements l and l + 16 added inside the lane, then the
    16-lane tree (partners 8, 4, 2, 1), IEEE sqrt, `+ theta` (norm and sum rounded to bf16 under NORM_BF16), IEEE division."""
    T, R = red.shape
    v = torch.zeros(T, 32, device=red.device)
    v[:, :R] = red.float()
    s = v[:, :16] * v[:, :16] + v[:, 16:] * v[:, 16:]
    for sh in (8, 4, 2, 1):
        s = s + s.roll(-sh, -1)
    n = s[:, :1].sqrt()
    th = torch.tensor(theta, dtype=torch.float32, device=red.device)
    if flags & L.COS_NORM_BF16:
        den = (n.to(torch.bfloat16).float() + th).to(torch.bfloat16).float()
    else:
        den = n + th
    return v[:, :R] / den


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("E", [4, 8, 16, 64])
def test_b_cosine_stage_against_fp64(E, flags):
    """|logit - fp64 value| <= half a bf16 ulp at the value's magnitude + R * 2^-23 * sum|terms|, the fp64 value evaluated from the
    kernel's own `reduced` with the denominator formed as the kernel forms it (and, under the bf16-operand flag, from the operands
    rounded as the kernel rounds them).  Row 7 of x is zero: `reduced` is zero there and the logits must be exactly 0."""
    T, D, R = 1000, 264, E // 2
    x, wr, emb = _inputs(T, D, E, seed=3)
    x[7] = 0
    red, lg, p, idx, w, status = ops.cosine_select(x, wr, emb, 2, flags, 0.3, THETA)
    assert int(status) == 0 and float(red[7].abs().max()) == 0.0
    assert float(lg[7].abs().max()) == 0.0 and idx[7].tolist() == [0, 1] and w[7].tolist() == [0.5, 0.5]
    m = _m32_like_kernel(red, flags, THETA)
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
def _llava_layer(fx, theta=None):
    m = fx["meta"]
    ex = nn.ModuleList([nn.Sequential(nn.Linear(m["D"], m["F"]), nn.GELU(), nn.Linear(m["F"], m["Dout"])) for _ in range(m["E"])])
    layer = llava_get("smoe_perturbed")(m["D"], m["Dout"], m["E"], m["K"], ex, types.SimpleNamespace(**m["args"]))
    layer.load_state_dict(fx["state"], strict=True)
    dt = torch.float32 if m["dtype"] == "float32" else torch.bfloat16
    if dt == torch.bfloat16:
        # The fixture is a CPU run: there `bf16 tensor + 0.1` rounds the scalar to bf16 first, the GPU keeps 0.1f (module docstring).
        # theta = bf16(0.1) makes the two sums the same on both; the layer's default stays 0.1.
        layer.theta = THETA_BF16 if theta is None else theta
    return layer.to(DEV).to(dt).train(), dt


def _pretrain_layer(fx):
    m = fx["meta"]
    layer = pretrain_get("smoe_perturbed")(m["D"], m["E"], m["F"], n_heads=m["K"], activation=F.relu, bias=m["bias"],
                                           sel_bias=m["sel_bias"], log_interval=None, args=types.SimpleNamespace(**m["args"]))
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
    ps["expert_embeddings"] = P.renorm(ps["expert_embeddings"], fx["meta"]["theta"])
    ps = {k: v.requires_grad_(True) for k, v in ps.items()}
    x = fx["x"].clone().requires_grad_(True)
    idx = idx.cpu().long().view(*x.shape[:-1], -1)
    if stack == "llava":
        out, aux, _ = P.llava_forward(x, ps, fx["meta"], forced_idx=idx)
        ((out.float() * fx["dy"].float()).sum() + aux.float()).backward()
    else:
        out, reg, _ = P.pretrain_forward(x, ps, fx["meta"], forced_idx=idx)
        ((out.float() * fx["dy"]).sum() + reg.float()).backward()
    return out.detach(), x.grad, {k: p.grad for k, p in ps.items()}


def _emb_after_ok(layer, fx):
    a, b = layer.expert_embeddings.detach().cpu(), fx["expert_embeddings_after"]
    assert a.dtype == b.dtype
    if a.dtype == torch.float32:
        assert max_rel(a, b) <= 1e-6, max_rel(a, b)
    else:       # the norm of a bf16 row is an fp32 sum rounded once: the device's summation order may move it by one bf16 ulp
        assert float(((a.float() - b.float()).abs() / b.float().abs()).max()) <= 2.0 ** -7


@pytest.mark.parametrize("tag", ["fp32", "bf16", "e16_bf16"])
def test_c_llava_layer_matches_fixture(tag):
    """Against the reference's recorded run; `e16_bf16` (E = 16, K = 4, R = 8) goes through the MFMA kernel.  The prints below are
    the observed figures."""
    fx = load(f"llava_smoe_perturbed_{tag}")
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
    ref_xg, ref_g = fx["x_grad"], fx["grads"]
    if bad > 0:
        # a row routed unlike the fixture: the restatement under the KERNEL's indices (its autograd is pinned to the fixtures'
        # recorded gradients by tests/test_perturbed_cpu.py).  Otherwise the reference is the fixture itself.
        _, ref_xg, ref_g = _restated_grads(fx, idx, "llava")
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
    assert layer.gate.weight.grad is None or float(layer.gate.weight.grad.abs().max()) == 0.0


@pytest.mark.parametrize("name", ["stages_fp32", "stages_bf16"])
def test_c_pretrain_layer_matches_fixture(name):
    """Against the reference's recorded run; the bf16 case runs the one-pass kernel under autocast (flags 12), the fp32 case the
    torch-op path.  The prints below are the observed figures; `bit-equal` reports whether the bf16
    d expert_sel reproduces the reference's bits (reported, not a pass condition)."""
    fx = load(f"pretrain_smoe_perturbed_{name}")
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
        print(f"pretrain {name}: d {pname} rel-L2 {rel_l2(p.grad.cpu(), g):.2e} bit-equal {torch.equal(p.grad.cpu(), g)}")
        assert rel_l2(p.grad.cpu(), g) <= tol, (pname, rel_l2(p.grad.cpu(), g))


# ------------------------------------------------------------------------------------------------ (d) backward kernel
@pytest.mark.parametrize("nulls", ["all", "no_dp", "no_dlogits", "only_dlogits", "only_dp"])
@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("E,K", [(8, 2), (64, 4), (4, 1)])
def test_d_backward_kernel_against_autograd_of_the_restatement(E, K, flags, nulls):
    """The restatement runs where it is pinned, on the CPU; under NORM_BF16 both sides get theta = bf16(0.1) (module docstring)."""
    T, R = 777, E // 2
    theta = THETA_BF16 if flags & L.COS_NORM_BF16 else THETA
    g = torch.Generator().manual_seed(11)
    red = torch.randn(T, R, generator=g).to(torch.bfloat16)
    red[5] = 0                                                                # norm 0: the norm's branch is masked, d reduced = d m / theta
    emb = P.renorm(torch.randn(E, R, generator=g)).contiguous()
    red_l, emb_l = red.clone().requires_grad_(True), emb.clone().requires_grad_(True)
    cos, p, idx, w = P.row_half(red_l, emb_l, K, flags, theta)
    dw = torch.randn(T, K, generator=g) if nulls in ("all", "no_dp", "no_dlogits") else None
    dp = torch.randn(T, E, generator=g) if nulls in ("all", "no_dlogits", "only_dp") else None
    dl = (torch.randn(T, E, generator=g) * 0.1).to(torch.bfloat16) if nulls in ("all", "no_dp", "only_dlogits") else None
    if flags & P.P_BF16 and dp is not None:
        dp = dp.to(torch.bfloat16).float()          # the gradient of a bf16 tensor is a bf16 tensor
    if flags & P.W_BF16 and dw is not None:
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
                                         dw, dp, dl, K, flags, 0.3, theta)
    if flags & L.COS_OPER_BF16:
        d_emb = d_emb.to(torch.bfloat16).float()
    keep = torch.arange(T, device=DEV) != 5            # row 5's gradient is d m / theta, no norm branch: compared on its own below
    e1, e2 = rel_l2(d_red[keep], g_red[keep]), rel_l2(d_emb, g_emb)
    e5 = rel_l2(d_red[5], g_red[5])
    print(f"E={E} K={K} flags={flags} {nulls}: d_reduced {e1:.2e} d_emb {e2:.2e} zero row {e5:.2e}")
    assert e1 <= 2e-3 and e2 <= 2e-3, (e1, e2)
    assert bool(d_red[5].isfinite().all()) and float(g_red[5].abs().max()) > 0 and e5 <= 2e-3, e5


# ------------------------------------------------------------------------------------------------ (e) fused against unfused
def _run_layers():
    res = {}
    cases = (("llava", "llava_smoe_perturbed_bf16", None), ("llava_theta_default", "llava_smoe_perturbed_bf16", THETA),
             ("llava_e16", "llava_smoe_perturbed_e16_bf16", None), ("pretrain", "pretrain_smoe_perturbed_stages_bf16", None))
    for key, name, theta in cases:
        fx = load(name)
        if key.startswith("llava"):
            layer, _ = _llava_layer(fx, theta)
            seen = _spy(layer, "compute_moe", 0)
            x, out, *_ = _llava_step(layer, fx)
        else:
            layer = _pretrain_layer(fx)
            seen = _spy(layer, "ffn", 1)
            x, out, _ = _pretrain_step(layer, fx)
        res[key] = dict(idx=seen[0].cpu(), out=out.detach().float().cpu(), dx=x.grad.float().cpu(),
                        grads={k: p.grad.float().cpu() for k, p in layer.named_parameters() if p.grad is not None})
    return res


def _child(path):
    assert os.environ.get("CSMOE_FUSED_ROUTER") == "0"
    torch.save(_run_layers(), path)


def test_e_fused_against_unfused():
    """CSMOE_FUSED_ROUTER is read per call but belongs to the process: the torch-op form runs in a fresh child process.  The LLaVA
    bf16 layer runs with theta = bf16(0.1) and with its default 0.1."""
    fused = _run_layers()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "unfused.pt")
        env = dict(os.environ, CSMOE_FUSED_ROUTER="0")
        subprocess.run([sys.executable, "-c", f"import tests.test_perturbed_gpu as t; t._child({path!r})"], cwd=ROOT, env=env,
                       check=True, timeout=600)
        unfused = torch.load(path, weights_only=True)
    ulp2 = 2 * 2.0 ** -8                 # the LLaVA stack's second bf16 bound of (c): 2 bf16 ulp of max|ref|, elementwise
    for stack in fused:
        a, b = fused[stack], unfused[stack]
        llava = stack.startswith("llava")
        assert torch.equal(a["idx"], b["idx"]), f"{stack}: the two forms route differently"

        def check(name, u, v, tol):
            e, m = rel_l2(u, v), max_rel(u, v)
            print(f"{stack}: fused vs unfused {name} rel-L2 {e:.2e} max-rel {m:.2e}")
            assert e <= tol, (stack, name, e)
            assert not llava or m <= ulp2, (stack, name, m)
        check("out", a["out"], b["out"], 1e-3 if llava else 2e-4)
        tol = 1e-3 if llava else 2e-3
        check("d x", a["dx"], b["dx"], tol)
        assert set(a["grads"]) == set(b["grads"])
        for k in a["grads"]:
            check(f"d {k}", a["grads"][k], b["grads"][k], tol)


# ------------------------------------------------------------------------------------------------ (f) a non-finite input row
@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("E,K", [(8, 2), (16, 4), (64, 2)])
def test_f_non_finite_row(E, K, flags):
    """One x row holds inf (E = 8: the small kernel; 16, 64: the MFMA kernel): it routes to experts 0..K-1 with weights 1/K and
    p = 1/E, its stored logits are the smallest finite logit of the tensor, the status is 1, the histogram counts it; every other
    row carries the bits of the same call on finite input."""
    T, D, row = 1000, 264, 700
    x, wr, emb = _inputs(T, D, E, seed=9)
    clean = [t.clone() for t in ops.cosine_select(x, wr, emb, K, flags, 0.3, THETA)]
    assert int(clean[5]) == 0
    xb = x.clone()
    xb[row, 20] = float("inf")
    red, lg, p, idx, w, status = ops.cosine_select(xb, wr, emb, K, flags, 0.3, THETA)
    hist = ops._ROUTE_HIST[2].clone()
    assert int(status) == 1
    keep = torch.ones(T, dtype=torch.bool, device=DEV)
    keep[row] = False
    for name, a, b in zip(("reduced", "logits", "p", "idx", "w"), (red, lg, p, idx, w), clean):
        assert torch.equal(a[keep], b[keep]), name
    assert not bool(red[row].isfinite().all()) and bool(lg.isfinite().all())
    assert torch.equal(lg[row], lg[keep].min().expand(E))
    _, rp, ridx, rw = P.row_half(red, emb, K, flags, THETA)                 # the restatement on the kernel's own `reduced`
    assert idx[row].tolist() == ridx[row].tolist() == list(range(K))
    assert torch.equal(w[row], rw[row].float()) and w[row].tolist() == [1.0 / K] * K
    assert torch.equal(p[row], rp[row].float()) and float(p[row, 0]) == 1.0 / E
    rows = int(L.lib.csmoe_gate_select_rows())
    blk = torch.arange(T, device=DEV).div(rows, rounding_mode="floor").unsqueeze(1) * E + idx.long()
    assert torch.equal(hist.long(), torch.bincount(blk.flatten(), minlength=hist.numel()).view_as(hist))


# ------------------------------------------------------------------------------------------------ (g) determinism
def test_g_two_identical_steps_are_bit_identical():
    a, b = _run_layers(), _run_layers()
    for stack in a:
        assert torch.equal(a[stack]["idx"], b[stack]["idx"]) and torch.equal(a[stack]["out"], b[stack]["out"])
        assert torch.equal(a[stack]["dx"], b[stack]["dx"])
        for k in a[stack]["grads"]:
            assert torch.equal(a[stack]["grads"][k], b[stack]["grads"][k]), (stack, k)
    # the backward kernel where several workgroups contribute partial tables of d emb
    T, E, K = 1000, 64, 2
    g = torch.Generator(device=DEV).manual_seed(5)
    red = torch.randn(T, E // 2, generator=g, device=DEV).to(torch.bfloat16)
    emb = P.renorm(torch.randn(E, E // 2, generator=g, device=DEV)).contiguous()
    dw, dp = torch.randn(T, K, generator=g, device=DEV), torch.randn(T, E, generator=g, device=DEV)
    for flags in FLAG_SETS:
        with torch.no_grad():
            cos, p, idx, w = P.row_half(red, emb, K, flags)
        runs = [ops.cosine_select_bwd(red, emb, cos.contiguous(), idx.int().contiguous(), w.float().contiguous(), dw, dp, None, K, flags,
                                      0.3, THETA) for _ in range(3)]
        for r in runs[1:]:
            assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])


# ------------------------------------------------------------------------------------------------ (h) no host synchronisation
@pytest.mark.parametrize("stack", ["llava", "pretrain"])
def test_h_step_has_no_host_synchronisation(stack):
    if stack == "llava":
        fx = load("llava_smoe_perturbed_bf16")
        layer, _ = _llava_layer(fx)
        step = lambda x: _llava_fwd_bwd(layer, x, dy)
    else:
        fx = load("pretrain_smoe_perturbed_stages_bf16")
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


# ------------------------------------------------------------------------------------------------ (i) the default mode is xmoe's
@pytest.mark.parametrize("flags", [3, 4])
@pytest.mark.parametrize("E", [8, 16])
def test_i_default_flags_still_give_xmoe_results(E, flags):
    """Neither new flag set: the XMoE normalisation (clamp at eps), as before.  A cheap guard beside tests/test_xmoe_gpu.py: the
    routing of the one-pass kernel equals the torch-op form's, `reduced` is still csmoe_gate_logits' bits, and the result differs
    from the perturbed mode's (the flag is read)."""
    T, D, K = 257, 264, 2
    x, wr, emb = _inputs(T, D, E, seed=21)
    red, lg, p, idx, w, status = ops.cosine_select(x, wr, emb, K, flags)
    with torch.no_grad():
        lg2, p2, idx2, w2 = cosine_route_unfused(x, wr, None, emb, K, flags)
    assert int(status) == 0 and torch.equal(red, ops.gate_logits(x, wr))
    assert torch.equal(idx, idx2)
    assert float((lg.float() - lg2.float()).abs().max()) <= 2.0 ** -7 * 1.5          # one bf16 ulp at |cos| <= 1.5, as test_xmoe_gpu (f)
    n = red.float().norm(dim=-1, keepdim=True)
    assert float(n.min()) > 1e-4                                                      # no clamped row: |logit| is |cos| * 1.5
    lg_t = ops.cosine_select(x, wr, emb, K, flags | L.COS_NORM_THETA, 0.3, THETA)[1]
    assert not torch.equal(lg, lg_t)
