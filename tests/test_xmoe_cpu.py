"""CPU checks of the XMoE cosine-router layers: registration, initialisation, state-dict names, the C ABI of the new kernels, and
the pin of the test-side restatement (tests/xmoe_ref.py) to the fixtures captured from the reference classes
(tests/golden/make_golden_xmoe.py): every recorded stage, fp32 to 1e-6 and bf16 bit for bit (the fixtures hold no tie rows)."""
import ctypes
import os
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import xmoe_ref as X
from tests.golden_util import load

LLAVA = ["llava_xmoe_fp32", "llava_xmoe_bf16"]
PRETRAIN = ["pretrain_xmoe_fp32", "pretrain_xmoe_bf16", "pretrain_xmoe_selbias_fp32"]
STAGES = ["reduced", "gate_logits", "gate_softmax", "weights"]


def llava_layer(fx):
    from competesmoe_amd.moe import get_moe
    m = fx["meta"]
    ex = nn.ModuleList([nn.Sequential(nn.Linear(m["D"], m["F"]), nn.GELU(), nn.Linear(m["F"], m["Dout"])) for _ in range(m["E"])])
    return get_moe("xmoe")(m["D"], m["Dout"], m["E"], m["K"], ex, types.SimpleNamespace(**m["args"]))


def pretrain_layer(fx):
    from competesmoe_amd.pretrain import get_moe
    m = fx["meta"]
    return get_moe("xmoe")(m["D"], m["E"], m["F"], n_heads=m["K"], activation=F.relu, bias=m["bias"], sel_bias=m["sel_bias"],
                           log_interval=None, args=types.SimpleNamespace(**m["args"]))


def test_both_registries_know_xmoe():
    from competesmoe_amd.moe import get_moe as llava_get, XMOE as LX
    from competesmoe_amd.pretrain import get_moe as pre_get, XMOE as PX
    assert llava_get("xmoe") is LX and pre_get("xmoe") is PX


def test_llava_expert_embeddings_initial_draw_is_the_references():
    fx = load("llava_xmoe_fp32")
    layer = llava_layer(fx)
    assert torch.equal(layer.expert_embeddings.detach(), fx["state"]["expert_embeddings"])
    assert layer.gate.bias is not None and layer.inp_reduction.bias is None


@pytest.mark.parametrize("name", LLAVA + PRETRAIN)
def test_state_dict_loads_strictly_by_name(name):
    fx = load(name)
    layer = llava_layer(fx) if name.startswith("llava") else pretrain_layer(fx)
    layer = layer.to(next(iter(fx["state"].values())).dtype) if name.startswith("llava") else layer
    assert set(layer.state_dict()) == set(fx["state"])
    layer.load_state_dict(fx["state"], strict=True)
    for k, v in layer.state_dict().items():
        assert v.shape == fx["state"][k].shape and v.dtype == fx["state"][k].dtype, k


def test_pretrain_init_follows_the_reference():
    fx = load("pretrain_xmoe_fp32")
    layer = pretrain_layer(fx)
    e = layer.expert_embeddings.detach()
    # orthogonal_(gain = 0.32) on [E, E/2]: orthogonal columns of norm 0.32
    assert torch.allclose(e.t() @ e, 0.32 ** 2 * torch.eye(e.shape[1]), atol=1e-6)
    D = fx["meta"]["D"]
    assert abs(float(layer.expert_sel.detach().std()) - D ** -0.5) < 0.2 * D ** -0.5
    assert layer.sel_bias is None and pretrain_layer(load("pretrain_xmoe_selbias_fp32")).sel_bias is not None


def test_new_cabi_symbols_resolve():
    from competesmoe_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("csmoe_cosine_select_ok", "csmoe_cosine_select_work_ints", "csmoe_cosine_select", "csmoe_cosine_select_bwd_parts",
                 "csmoe_cosine_select_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "csmoe.h")).read()
    assert "CSMOE_SEL_TEMP_SOFTMAX_TOPK = 5" in header and _lib.SEL_TEMP_SOFTMAX_TOPK == 5
    ok = _lib.lib.csmoe_cosine_select_ok
    assert ok(1000, 4096, 64, 2, _lib.BF16) == 1 and ok(1, 64, 4, 1, _lib.BF16) == 1
    assert ok(1000, 4096, 64, 2, _lib.F32) == 0          # fp32
    assert ok(1000, 4096, 66, 2, _lib.BF16) == 0         # E > 64
    assert ok(1000, 4096, 7, 2, _lib.BF16) == 0          # odd E
    assert ok(1000, 4100, 8, 2, _lib.BF16) == 0          # D % 8
    assert _lib.lib.csmoe_cosine_select_work_ints(129) == 2 + 2 * 3
    assert 1 <= _lib.lib.csmoe_cosine_select_bwd_parts(32768) <= 256


def _check_stages(fx, st, bf16):
    # no row ties its K-th with its (K+1)-th key, so the selected SET is defined; two equal keys inside the top-K may come in either
    # order (equal keys, equal weights)
    assert torch.equal(st["selected_experts"].sort(-1).values, fx["selected_experts"].long().sort(-1).values)
    for k in STAGES:
        a, b = st[k].detach(), fx[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype)
        if bf16:
            assert torch.equal(a, b), (k, float((a.float() - b.float()).abs().max()))
        else:
            assert float((a - b).abs().max()) <= 1e-6 * max(1.0, float(b.abs().max())), (k, float((a - b).abs().max()))


@pytest.mark.parametrize("name", LLAVA)
def test_restatement_reproduces_llava_fixture(name):
    fx = load(name)
    assert fx["meta"]["tie_share"] == 0.0
    ps = dict(fx["state"])
    ps["expert_embeddings"] = X.renorm(ps["expert_embeddings"])
    assert torch.equal(ps["expert_embeddings"], fx["expert_embeddings_after"])
    bf16 = fx["x"].dtype == torch.bfloat16
    out, aux, st = X.llava_forward(fx["x"], ps, fx["meta"])
    _check_stages(fx, st, bf16)
    # the balance loss reads the top-1 COLUMN: under the reference's own order of two equal keys (one row of the bf16 fixture)
    out, aux, st = X.llava_forward(fx["x"], ps, fx["meta"], forced_idx=fx["selected_experts"])
    tol = 0.0 if bf16 else 1e-6
    assert float((out.float() - fx["output"].float()).abs().max()) <= tol * float(fx["output"].abs().max())
    assert abs(float(aux) - float(fx["aux_loss"])) <= (0.0 if bf16 else 1e-6)


@pytest.mark.parametrize("name", LLAVA + PRETRAIN)
def test_restatement_autograd_reproduces_recorded_gradients(name):
    """tests/test_xmoe_gpu.py takes autograd of the restatement as the gradient reference wherever a row routes unlike the fixture;
    this pins that autograd to the gradients the reference recorded (x.grad and every parameter's), under the fixture's own
    indices.  Bounds: the ones the two stacks' GPU tests hold the layers to, so the substitute is no looser a reference than the
    fixture: LLaVA fp32 1e-5 of max|ref|, bf16 1e-3 relative L2 and 2 bf16 ulp of max|ref|; pretrain fp32 4e-5, bf16 2e-3 relative
    L2.  Printed below: bit-equal for both LLaVA fixtures and for d x, d expert_sel, d expert_embeddings of the bf16 pretrain one (d keys,
    d values 2.3e-8), relative L2 <= 4.1e-7 for the fp32 pretrain ones."""
    from tests.golden_util import rel_l2, max_rel
    fx = load(name)
    llava = name.startswith("llava")
    ps = {k: v.clone() for k, v in fx["state"].items()}
    ps["expert_embeddings"] = X.renorm(ps["expert_embeddings"])
    ps = {k: v.requires_grad_(True) for k, v in ps.items()}
    x = fx["x"].clone().requires_grad_(True)
    if llava:
        out, aux, _ = X.llava_forward(x, ps, fx["meta"], forced_idx=fx["selected_experts"])
        ((out.float() * fx["dy"].float()).sum() + aux.float()).backward()
        bf16 = fx["x"].dtype == torch.bfloat16
        rl, mr = (1e-3, 2 * 2.0 ** -8) if bf16 else (1e-5, 1e-5)
    else:
        out, reg, _ = X.pretrain_forward(x, ps, fx["meta"], forced_idx=fx["selected_experts"])
        ((out.float() * fx["dy"]).sum() + reg.float()).backward()
        rl, mr = (2e-3 if fx["meta"]["bf16"] else 4e-5), None
    got = dict({k: p.grad for k, p in ps.items()}, x=x.grad)
    want = dict(fx["grads"], x=fx["x_grad"])
    for k, g in want.items():
        if g is None:                           # a parameter the router does not use (the plain gate): the reference left no gradient
            assert got[k] is None or float(got[k].abs().max()) == 0.0, k
            continue
        assert got[k] is not None and got[k].dtype == g.dtype and got[k].shape == g.shape, k
        print(f"{name}: d {k} rel-L2 {rel_l2(got[k], g):.2e} max-rel {max_rel(got[k], g):.2e}")
        assert rel_l2(got[k], g) <= rl, (k, rel_l2(got[k], g))
        assert mr is None or max_rel(got[k], g) <= mr, (k, max_rel(got[k], g))
    for k, p in ps.items():
        assert k in want or p.grad is None or float(p.grad.abs().max()) == 0.0, k


@pytest.mark.parametrize("name", PRETRAIN)
def test_restatement_reproduces_pretrain_fixture(name):
    fx = load(name)
    assert fx["meta"]["tie_share"] == 0.0
    ps = dict(fx["state"])
    ps["expert_embeddings"] = X.renorm(ps["expert_embeddings"])
    assert torch.equal(ps["expert_embeddings"], fx["expert_embeddings_after"])
    bf16 = fx["meta"]["bf16"]
    out, reg, st = X.pretrain_forward(fx["x"], ps, fx["meta"])
    _check_stages(fx, st, bf16)
    assert out.dtype == fx["output"].dtype
    err = float((out.float() - fx["output"].float()).norm() / fx["output"].float().norm())
    assert err <= (2e-4 if bf16 else 1e-6), err       # the oracle's cvmm restatement, at its own pinned bound
    (k, v), = fx["reg_loss"].items()
    assert k.endswith("_ebalance") and abs(float(reg) - float(v)) <= (2e-6 if bf16 else 1e-6)
