"""GPU tests of the sigmoid router (CSMOE_SEL_SIGMOID_NORM; LLaVA `smoe_sigmoidgating`, pretrain `smoe_sigmoid`): the rule in
csmoe_router_select / csmoe_router_select_bwd / csmoe_gate_select, and both layers against the fixtures captured from the reference
classes (tests/golden/make_golden_sigmoid.py) and the test-side restatement pinned to them (tests/sigmoid_ref.py,
tests/test_sigmoid_cpu.py).

Bounds.  Selection: ids equal; weights rtol 1e-5 where the quotient is fp32, 2^-7 where it is bf16-rounded (tests/test_ops_gpu.py's
figures for rules 3 and 1).  Backward: fp32 against CPU autograd rtol 1e-4, atol 1e-6 (test_router_select_bwd_fp32); bf16 against the
torch-op emulation of the kernel's lines bit for bit (the emulation is pinned to autograd on the CPU).  One-pass router: the bits of
csmoe_router_select on its own logits.  Layers: the bounds tests/test_perturbed_gpu.py (c) uses for the same quantities -- LLaVA fp32
<= 1e-5 of max|ref|, bf16 <= 1e-3 relative L2 and <= 2 bf16 ulp of max|ref|; pretrain fp32 outputs <= 1e-5, gradients <= 4e-5
relative L2, bf16 outputs <= 2e-4, gradients <= 2e-3.  bf16 sigmoid keys tie at the top-K boundary in every draw, so the reference
for ids is the restatement with the project's tie rule on the same inputs, and the fixture is compared through the sorted selected
keys, on every row."""
import os
import subprocess
import sys
import tempfile
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import sigmoid_ref as S
from tests.golden_util import load, rel_l2, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from competesmoe_amd import _lib as L, ops
    from competesmoe_amd.moe import get_moe as llava_get, MoEBlock as LlavaBlock
    from competesmoe_amd.pretrain import get_moe as pretrain_get, MoEBlock as PretrainBlock

LLAVA = ["llava_smoe_sigmoidgating_fp32", "llava_smoe_sigmoidgating_bf16", "llava_smoe_sigmoidgating_e16_bf16"]
PRETRAIN = ["pretrain_smoe_sigmoid_fp32", "pretrain_smoe_sigmoid_bf16"]
MODE = 6
SHAPES = [(1, 4, 1), (77, 8, 2), (300, 63, 7), (512, 64, 2), (256, 128, 8), (64, 300, 4), (40, 8, 8)]
CASES = [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, 1)]      # (scores, round_sum_bf16) as the reference reaches the rule


# ------------------------------------------------------------------------------------------------ csmoe_router_select
@pytest.mark.parametrize("dtype,rs", CASES)
@pytest.mark.parametrize("T,E,K", SHAPES)
def test_router_select_sigmoid_norm(T, E, K, dtype, rs):
    g = torch.Generator().manual_seed(E * 7 + K)
    scores = (torch.randn(T, E, generator=g) * 2).to(dtype)
    if dtype == torch.bfloat16:
        scores = torch.cat([scores, torch.zeros(1, E, dtype=dtype)])        # an all-zero row: E equal keys of 0.5
    sm, idx, w = ops.router_select(scores.to(DEV), K, MODE, round_sum_bf16=bool(rs))
    x_dtype, sum_fp32 = S.select_flags(dtype, rs)
    _keys, rsm, ridx, rw = S.select(scores, K, x_dtype, sum_fp32=sum_fp32)
    assert torch.allclose(sm.cpu(), rsm, rtol=2e-6, atol=1e-8)
    assert torch.equal(idx.cpu().long(), ridx)
    bq = dtype == torch.bfloat16 and rs
    assert rw.dtype == (torch.bfloat16 if bq else torch.float32)
    assert torch.allclose(w.cpu(), rw.float(), rtol=2 ** -7 if bq else 1e-5, atol=1e-7)
    if dtype == torch.bfloat16:
        half = torch.tensor(0.5)
        den = (half * K).bfloat16().float() if rs else half * K
        one = (half / den).bfloat16().float() if bq else half / den
        assert idx[-1].tolist() == list(range(K)) and w[-1].tolist() == [float(one)] * K


# ------------------------------------------------------------------------------------------------ csmoe_router_select_bwd
def test_router_select_bwd_sigmoid_norm_fp32():
    T, E, K = 200, 16, 3
    g = torch.Generator().manual_seed(5)
    scores, dw, dsm = torch.randn(T, E, generator=g), torch.randn(T, K, generator=g), torch.randn(T, E, generator=g)
    sd = scores.to(DEV)
    sm, idx, w = ops.router_select(sd, K, MODE, False)
    ds = ops.router_select_bwd(sd, K, MODE, False, sm, idx, w, dw.to(DEV), dsm.to(DEV))
    s = scores.clone().requires_grad_(True)
    _, smr, _, wr = S.select(s, K, torch.float32, idx=idx.cpu())
    ((wr * dw).sum() + (smr * dsm).sum()).backward()
    assert torch.allclose(ds.cpu(), s.grad, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("with_softmax", [False, True])
@pytest.mark.parametrize("rs", [0, 1])
@pytest.mark.parametrize("T,E,K", [(200, 16, 3), (130, 64, 2)])
def test_router_select_bwd_sigmoid_norm_bf16_is_the_emulation(T, E, K, rs, with_softmax):
    """The kernel against the torch-op restatement of its own lines (run on the device, the row sum of the softmax path in the
    wave's butterfly order): bit for bit, both rounding cases, with and without a gradient on the softmax."""
    g = torch.Generator().manual_seed(T + K)
    scores = (torch.randn(T, E, generator=g) * 2).bfloat16().to(DEV)
    dw = torch.randn(T, K, generator=g).to(DEV)
    if rs:
        dw = dw.bfloat16().float()            # the gradient of a bf16 tensor is a bf16 tensor
    dsm = torch.randn(T, E, generator=g).to(DEV) if with_softmax else None
    sm, idx, w = ops.router_select(scores, K, MODE, bool(rs))
    ds = ops.router_select_bwd(scores, K, MODE, bool(rs), sm, idx, w, dw, dsm)
    want = S.select_bwd_emulation(scores, sm, idx, dw, dsm, rs, wave_tree=True)
    diff = (ds.float() - want.float()).abs()
    print(f"T={T} E={E} K={K} rs={rs} softmax={with_softmax}: differing {int((ds != want).sum())} of {ds.numel()}, max {float(diff.max()):.2e}")
    assert ds.dtype == want.dtype and torch.equal(ds, want)


# ------------------------------------------------------------------------------------------------ csmoe_gate_select
@pytest.mark.parametrize("rs", [0, 1])
@pytest.mark.parametrize("T,D,E,K", [(1, 64, 4, 2), (63, 256, 8, 2), (65, 1152, 4, 2), (300, 264, 40, 4), (1000, 4096, 64, 2),
                                     (257, 520, 16, 1), (128, 1024, 48, 8)])
def test_gate_select_sigmoid_norm_equals_gate_then_select(T, D, E, K, rs):
    g = torch.Generator(device=DEV).manual_seed(T * 7 + E)
    x = torch.randn(T, D, device=DEV, generator=g).to(torch.bfloat16)
    wg = (torch.randn(E, D, device=DEV, generator=g) * D ** -0.5).to(torch.bfloat16)
    assert ops.gate_select_ok(x, wg, K)
    logits, sm, idx, w = ops.gate_select(x, wg, K, MODE, bool(rs))
    ref_logits = ops.gate_logits(x, wg)
    d = (logits.float() - ref_logits.float()).abs()
    assert (d <= 2.0 ** -7 * ref_logits.float().abs().clamp_min(2.0 ** -6)).all(), d.max()
    sm2, idx2, w2 = ops.router_select(logits, K, MODE, bool(rs))
    assert torch.equal(idx, idx2) and torch.equal(w, w2) and torch.equal(sm, sm2)
    b_hist = ops.bin_tokens(idx, E)                 # picks the histogram of this routing up
    assert ops._route_hist_for(idx, E) is not None
    idx_copy = idx.clone()
    b_plain = ops.bin_tokens(idx_copy, E)
    assert ops._route_hist_for(idx_copy, E) is None
    for a, b in ((b_hist.counts, b_plain.counts), (b_hist.offsets, b_plain.offsets), (b_hist.perm, b_plain.perm),
                 (b_hist.slot_of, b_plain.slot_of)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the layers
def _experts(D, Fh, Dout, E):
    return nn.ModuleList([nn.Sequential(nn.Linear(D, Fh), nn.GELU(), nn.Linear(Fh, Dout)) for _ in range(E)])


def _llava_layer(fx):
    m = fx["meta"]
    layer = llava_get("smoe_sigmoidgating")(m["D"], m["Dout"], m["E"], m["K"], _experts(m["D"], m["F"], m["Dout"], m["E"]),
                                            types.SimpleNamespace(**m["args"]))
    layer.load_state_dict(fx["state"], strict=True)
    return layer.to(DEV).to(fx["x"].dtype).train()


def _pretrain_layer(fx):
    m = fx["meta"]
    layer = pretrain_get("smoe_sigmoid")(m["D"], m["E"], m["F"], n_heads=m["K"], activation=F.relu, bias=m["bias"],
                                         sel_bias=m["sel_bias"], log_interval=None, args=types.SimpleNamespace(**m["args"]))
    layer.load_state_dict(fx["state"], strict=True)
    layer = layer.to(DEV).train()
    layer.regularization_present = True
    return layer


def _spy(layer, name, take):
    seen = []
    fn = getattr(layer, name)

    def spy(*a, **k):
        seen.append(take(a))
        return fn(*a, **k)
    setattr(layer, name, spy)
    return seen


def _step(fx, layer=None):
    """One forward + backward of the fixture's layer on the device -> dict(idx, w, out, loss, dx, grads, infor)."""
    llava = fx["meta"]["name"] == "smoe_sigmoidgating"
    x = fx["x"].to(DEV).requires_grad_(True)
    dy = fx["dy"].to(DEV)
    if llava:
        layer = layer or _llava_layer(fx)
        seen = _spy(layer, "_router_aux", lambda a: (a[0].idx.detach().clone(), a[0].w.detach().clone()))
        out, loss, none, infor = layer(x)
        assert none is None
        ((out.float() * dy.float()).sum() + loss.float()).backward()
    else:
        layer = layer or _pretrain_layer(fx)
        seen = _spy(layer, "ffn", lambda a: (a[1].detach().clone(), a[2].detach().clone()))
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=fx["meta"]["bf16"]):
            out = layer(x)
            reg = layer.get_reg_loss()
        (name, loss), = reg.items()
        assert name == "mlp_balance"
        infor = {}
        ((out.float() * dy).sum() + loss.float()).backward()
    idx, w = seen[0]
    return dict(idx=idx.cpu(), w=w.float().cpu(), out=out.detach().cpu(), loss=loss.detach().float().cpu(), dx=x.grad.cpu(),
                grads={k: p.grad.cpu() for k, p in layer.named_parameters() if p.grad is not None},
                infor={k: v.float().cpu() for k, v in infor.items()})


def _restated(fx, idx=None):
    llava = fx["meta"]["name"] == "smoe_sigmoidgating"
    ps = {k: v.clone().requires_grad_(True) for k, v in fx["state"].items()}
    x = fx["x"].clone().requires_grad_(True)
    out, loss, st = (S.llava_forward if llava else S.pretrain_forward)(x, ps, fx["meta"], idx=idx)
    ((out.float() * fx["dy"].float()).sum() + loss.float()).backward()
    return dict(idx=st["selected_experts"], w=st["weights"].detach().float(), out=out.detach(), loss=loss.detach().float(), dx=x.grad,
                grads={k: p.grad for k, p in ps.items()}, keys=st["gate_sigmoid"].detach())


def _bounds(fx):
    """(output check, gradient check, loss bound) of tests/test_perturbed_gpu.py (c) for this stack and dtype."""
    llava = fx["meta"]["name"] == "smoe_sigmoidgating"
    bf16 = fx["gate_logits"].dtype == torch.bfloat16
    if llava:
        rl, mr = (1e-3, 2 * 2.0 ** -8) if bf16 else (None, 1e-5)
        out_ok = grad_ok = lambda a, b: max_rel(a, b) <= mr and (rl is None or rel_l2(a, b) <= rl)
        loss_tol = lambda v: (2e-3 if bf16 else 2e-5) * max(1.0, abs(v))
    else:
        out_ok = (lambda a, b: rel_l2(a, b) <= 2e-4) if bf16 else (lambda a, b: max_rel(a, b) <= 1e-5)
        grad_ok = lambda a, b: rel_l2(a, b) <= (2e-3 if bf16 else 4e-5)
        loss_tol = lambda v: (2e-5 if bf16 else 2e-6) + 1e-4 * abs(v)
    return out_ok, grad_ok, loss_tol


@pytest.mark.parametrize("name", LLAVA + PRETRAIN)
def test_layer_against_restatement_and_fixture(name):
    """(a) the layer against the restatement with the project's tie rule on the same inputs, all rows; (b) against the fixture, all
    rows, through the sorted selected keys."""
    fx = load(name)
    K = fx["meta"]["K"]
    got, ref = _step(fx), _restated(fx)
    bf16 = fx["gate_logits"].dtype == torch.bfloat16
    out_ok, grad_ok, loss_tol = _bounds(fx)
    assert got["out"].dtype == fx["output"].dtype and got["out"].shape == fx["output"].shape
    assert torch.equal(got["idx"].long().reshape(-1, K), ref["idx"].reshape(-1, K))                          # (a) every row
    dw = (got["w"].reshape(-1, K) - ref["w"].reshape(-1, K)).abs()
    print(f"{name}: weights max |diff| {float(dw.max()):.2e}; out rel-L2 {rel_l2(got['out'], ref['out']):.2e} "
          f"max-rel {max_rel(got['out'], ref['out']):.2e}")
    assert torch.allclose(got["w"].reshape(-1, K), ref["w"].reshape(-1, K), rtol=2 ** -7 if bf16 else 1e-5, atol=1e-7)
    assert out_ok(got["out"], ref["out"])
    assert abs(float(got["loss"]) - float(ref["loss"])) <= loss_tol(float(ref["loss"]))
    for k, g in dict(ref["grads"], x=ref["dx"]).items():
        a = got["dx"] if k == "x" else got["grads"][k]
        print(f"{name}: d {k} rel-L2 {rel_l2(a, g):.2e} max-rel {max_rel(a, g):.2e}")
        assert a.dtype == g.dtype and grad_ok(a, g), k
    mine = torch.gather(fx["gate_sigmoid"], -1, got["idx"].long().view(fx["selected_experts"].shape)).sort(-1).values
    theirs = torch.gather(fx["gate_sigmoid"], -1, fx["selected_experts"].long()).sort(-1).values
    assert torch.equal(mine, theirs)                                                                          # (b) every row, bitwise
    if fx["meta"]["name"] == "smoe_sigmoidgating":
        assert set(got["infor"]) == set(fx["infor_aux"])
        assert abs(float(got["loss"]) - float(fx["aux_loss"])) <= loss_tol(float(fx["aux_loss"]))


def _run_layers():
    return {name: _step(load(name)) for name in LLAVA + PRETRAIN}


def _child(path):
    torch.save(_run_layers(), path)


@pytest.mark.parametrize("switch", ["CSMOE_FUSED_ROUTER", "CSMOE_FUSED_STEP"])
def test_one_pass_and_separate_launch_paths_give_the_same_bits(switch):
    """(c) The switches are read per call but belong to the process: the separate-launch form runs in a fresh child process."""
    fused = _run_layers()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "other.pt")
        subprocess.run([sys.executable, "-c", f"import tests.test_sigmoid_gpu as t; t._child({path!r})"], cwd=ROOT,
                       env=dict(os.environ, **{switch: "0"}), check=True, timeout=600)
        other = torch.load(path, weights_only=True)
    wrong = []
    for name in fused:
        a, b = fused[name], other[name]
        for k in ("idx", "w", "out", "loss", "dx"):
            if not torch.equal(a[k], b[k]):
                wrong.append((name, k, float((a[k].float() - b[k].float()).abs().max())))
        assert set(a["grads"]) == set(b["grads"])
        wrong += [(name, k, float((a["grads"][k].float() - b["grads"][k].float()).abs().max())) for k in a["grads"]
                  if not torch.equal(a["grads"][k], b["grads"][k])]
    assert not wrong, wrong


@pytest.mark.parametrize("stack", ["llava", "pretrain"])
@pytest.mark.parametrize("why,D,E", [("fp32", 64, 8), ("E80", 64, 80), ("D60", 60, 8)])
def test_refused_shapes_take_the_fallback(stack, why, D, E):
    """(d) fp32, E = 80 and D = 60 are shapes csmoe_gate_select refuses: GateLogits + RouterSelect with the same rule, against the
    restatement."""
    K, Fh, B, N = 2, 32, 2, 40
    bf16 = why != "fp32"
    g = torch.Generator().manual_seed(E + D)
    args = dict(balance_loss_coef=0.01, router_z_loss_coef=0.001, init_weight=True, test_only=False)
    if stack == "llava":
        dt = torch.bfloat16 if bf16 else torch.float32
        layer = llava_get("smoe_sigmoidgating")(D, D, E, K, _experts(D, Fh, D, E), types.SimpleNamespace(**args))
        with torch.no_grad():
            for p in layer.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (p.shape[-1] ** -0.5 if p.dim() == 2 else 0.1))
        layer = layer.to(dt)
        meta = dict(name="smoe_sigmoidgating", E=E, K=K, D=D, F=Fh, Dout=D, args=args)
        x = torch.randn(B, N, D, generator=g).to(dt)
        assert not ops.gate_select_ok(x.reshape(-1, D).to(DEV), layer.gate.weight.to(DEV), K)
        layer = layer.to(DEV).train()
    else:
        layer = pretrain_get("smoe_sigmoid")(D, E, Fh, n_heads=K, activation=F.relu, log_interval=None, args=types.SimpleNamespace(**args))
        meta = dict(name="smoe_sigmoid", E=E, K=K, D=D, F=Fh, bf16=bf16, args=args)
        x = torch.randn(B, N, D, generator=g)
        xo = x.reshape(-1, D).to(DEV)
        assert not ops.gate_select_ok(xo.bfloat16() if bf16 else xo, layer.w_gate.to(DEV), K)
        layer = layer.to(DEV).train()
        layer.regularization_present = True
    state = {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}
    dy = torch.randn(B, N, D, generator=g).to(x.dtype)
    logits = F.linear(x.to(torch.bfloat16 if bf16 else torch.float32), state["gate.weight" if stack == "llava" else "w_gate"].to(
        torch.bfloat16 if bf16 else torch.float32))
    fx = dict(meta=meta, state=state, x=x, dy=dy, gate_logits=logits)
    got, ref = _step(fx, layer), _restated(fx)
    out_ok, grad_ok, loss_tol = _bounds(fx)
    assert torch.equal(got["idx"].long().reshape(-1, K), ref["idx"].reshape(-1, K))
    assert torch.allclose(got["w"].reshape(-1, K), ref["w"].reshape(-1, K), rtol=2 ** -7 if bf16 else 1e-5, atol=1e-7)
    assert out_ok(got["out"], ref["out"])
    assert abs(float(got["loss"]) - float(ref["loss"])) <= loss_tol(float(ref["loss"]))
    for k, gr in dict(ref["grads"], x=ref["dx"]).items():
        a = got["dx"] if k == "x" else got["grads"][k]
        assert grad_ok(a, gr), (k, rel_l2(a, gr), max_rel(a, gr))


@pytest.mark.parametrize("name", ["llava_smoe_sigmoidgating_fp32", "llava_smoe_sigmoidgating_bf16", "pretrain_smoe_sigmoid_fp32",
                                  "pretrain_smoe_sigmoid_bf16"])
def test_layer_inside_its_block_equals_layer_plus_residual(name):
    """(e) moe/block.py and pretrain/block.py around the layer at the fixture shape -- LayerNorm + gate in one launch, the logits and
    the residual handed to the layer -- against x + layer(LayerNorm(x)) from the separate pieces (LLaVA: the block's own normalised
    rows, as tests/test_block_gpu.py composes it; pretrain: torch's LayerNorm under the same autocast, as tests/
    test_pretrain_block_gpu.py does).  fp32: 1e-6 (LLaVA, the bound of that test) / 1e-5 (pretrain: two LayerNorm kernels); bf16: 2e-3
    relative L2, the project's bf16 bound (the block rounds moe + residual once, the composition twice)."""
    fx = load(name)
    llava = name.startswith("llava")
    D = fx["meta"]["D"]
    bf16 = fx["gate_logits"].dtype == torch.bfloat16
    x = fx["x"].to(DEV)
    if llava:
        layer = _llava_layer(fx)
        ln = nn.LayerNorm(D).to(DEV).to(x.dtype)
        blk = LlavaBlock(ln, layer)
        with torch.no_grad():
            a = blk(x)[0]
            xn = ops.layernorm_gate(x.reshape(-1, D), ln.weight, ln.bias, ln.eps, None)[0].view_as(x)
            b = x + layer(xn)[0]
    else:
        layer = _pretrain_layer(fx)
        ln = nn.LayerNorm(D).to(DEV)
        blk = PretrainBlock(ln, layer, 0.0).train()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            a = blk(x)
            b = x + layer(ln(x))
    assert a.dtype == b.dtype and a.shape == b.shape
    print(f"{name}: block vs layer + residual rel-L2 {rel_l2(a, b):.2e}")
    assert rel_l2(a, b) <= (2e-3 if bf16 else (1e-6 if llava else 1e-5)), rel_l2(a, b)


@pytest.mark.parametrize("name", ["llava_smoe_sigmoidgating_fp32", "llava_smoe_sigmoidgating_bf16"])
def test_llava_layer_without_grad_returns_zero_aux(name):
    """(f) x.requires_grad == False: a zero of x.dtype and {} (smoe_sigmoidgating.py:46-56)."""
    fx = load(name)
    layer = _llava_layer(fx)
    x = fx["x"].to(DEV)
    out, aux, none, infor = layer(x)
    assert none is None and infor == {} and aux.dtype == x.dtype and aux.shape == () and float(aux) == 0.0
    assert out.shape == fx["output"].shape and bool(out.isfinite().all())
