"""CPU checks of the perturbed-cosine router layers (`smoe_perturbed`): registration, initialisation, state-dict names, the two new
flag values, and the pin of the test-side restatement (tests/perturbed_ref.py) to the fixtures captured from the reference classes
(tests/golden/make_golden_perturbed.py): every recorded stage, fp32 to 1e-6 and bf16 bit for bit (the fixtures hold no tie rows),
and its autograd against the recorded gradients at the bounds tests/test_xmoe_cpu.py uses."""
import os
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import perturbed_ref as P
from tests.golden_util import load, rel_l2, max_rel

LLAVA = ["llava_smoe_perturbed_fp32", "llava_smoe_perturbed_bf16", "llava_smoe_perturbed_e16_bf16"]
PRETRAIN = ["pretrain_smoe_perturbed_stages_fp32", "pretrain_smoe_perturbed_stages_bf16"]
STAGES = ["reduced", "gate_logits", "gate_softmax", "weights"]


def llava_layer(fx):
    from competesmoe_amd.moe import get_moe
    m = fx["meta"]
    ex = nn.ModuleList([nn.Sequential(nn.Linear(m["D"], m["F"]), nn.GELU(), nn.Linear(m["F"], m["Dout"])) for _ in range(m["E"])])
    return get_moe("smoe_perturbed")(m["D"], m["Dout"], m["E"], m["K"], ex, types.SimpleNamespace(**m["args"]))


def pretrain_layer(fx):
    from competesmoe_amd.pretrain import get_moe
    m = fx["meta"]
    return get_moe("smoe_perturbed")(m["D"], m["E"], m["F"], n_heads=m["K"], activation=F.relu, bias=m["bias"], sel_bias=m["sel_bias"],
                                     log_interval=None, args=types.SimpleNamespace(**m["args"]))


def test_both_registries_know_smoe_perturbed():
    from competesmoe_amd.moe import get_moe as llava_get, MoEPerturbedCosingGating as LP
    from competesmoe_amd.pretrain import get_moe as pre_get, MoEPerturbedCosingGating as PP
    assert llava_get("smoe_perturbed") is LP and pre_get("smoe_perturbed") is PP and LP is not PP


def test_llava_expert_embeddings_initial_draw_is_the_references():
    fx = load("llava_smoe_perturbed_fp32")
    layer = llava_layer(fx)
    assert torch.equal(layer.expert_embeddings.detach(), fx["state"]["expert_embeddings"])
    assert layer.gate.bias is None and layer.inp_reduction.bias is None
    assert layer.theta == 0.1 == fx["meta"]["theta"] and layer.temperature == 0.3


@pytest.mark.parametrize("name", LLAVA + PRETRAIN)
def test_state_dict_loads_strictly_by_name(name):
    fx = load(name)
    layer = llava_layer(fx) if name.startswith("llava") else pretrain_layer(fx)
    layer = layer.to(next(iter(fx["state"].values())).dtype) if name.startswith("llava") else layer
    assert set(layer.state_dict()) == set(fx["state"])
    if name.startswith("llava"):
        assert {"gate.weight", "inp_reduction.weight", "expert_embeddings"} <= set(fx["state"]) and "gate.bias" not in fx["state"]
    layer.load_state_dict(fx["state"], strict=True)
    for k, v in layer.state_dict().items():
        assert v.shape == fx["state"][k].shape and v.dtype == fx["state"][k].dtype, k


def test_header_and_lib_agree_on_the_new_flags():
    from competesmoe_amd import _lib
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "csmoe.h")).read()
    assert "CSMOE_COS_NORM_THETA = 8" in header and _lib.COS_NORM_THETA == 8 == P.NORM_THETA
    assert "CSMOE_COS_NORM_BF16 = 16" in header and _lib.COS_NORM_BF16 == 16 == P.NORM_BF16
    assert "CSMOE_COS_OPER_BF16 = 4" in header and _lib.COS_OPER_BF16 == 4


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


def _params(fx):
    ps = dict(fx["state"])
    ps["expert_embeddings"] = P.renorm(ps["expert_embeddings"], fx["meta"]["theta"])
    assert torch.equal(ps["expert_embeddings"], fx["expert_embeddings_after"])
    return ps


@pytest.mark.parametrize("name", LLAVA)
def test_restatement_reproduces_llava_fixture(name):
    fx = load(name)
    assert fx["meta"]["tie_share"] == 0.0
    ps = _params(fx)
    bf16 = fx["x"].dtype == torch.bfloat16
    out, aux, st = P.llava_forward(fx["x"], ps, fx["meta"])
    _check_stages(fx, st, bf16)
    # the balance loss reads the top-1 COLUMN: under the reference's own order of two equal keys
    out, aux, st = P.llava_forward(fx["x"], ps, fx["meta"], forced_idx=fx["selected_experts"])
    tol = 0.0 if bf16 else 1e-6
    assert float((out.float() - fx["output"].float()).abs().max()) <= tol * float(fx["output"].abs().max())
    assert abs(float(aux) - float(fx["aux_loss"])) <= (0.0 if bf16 else 1e-6)


@pytest.mark.parametrize("name", PRETRAIN)
def test_restatement_reproduces_pretrain_fixture(name):
    fx = load(name)
    assert fx["meta"]["tie_share"] == 0.0
    ps = _params(fx)
    bf16 = fx["meta"]["bf16"]
    if bf16:        # the reference's run took the norm in fp32: the upcast the restatement's missing NORM_BF16 flag stands for
        assert fx["meta"]["autocast_fp32_upcasts"].get("norm", 0) >= 1
    out, reg, st = P.pretrain_forward(fx["x"], ps, fx["meta"])
    _check_stages(fx, st, bf16)
    assert out.dtype == fx["output"].dtype
    err = float((out.float() - fx["output"].float()).norm() / fx["output"].float().norm())
    assert err <= (2e-4 if bf16 else 1e-6), err       # the oracle's cvmm restatement, at its own pinned bound
    (k, v), = fx["reg_loss"].items()
    assert k.endswith("_ebalance") and abs(float(reg) - float(v)) <= (2e-6 if bf16 else 1e-6)


@pytest.mark.parametrize("name", LLAVA + PRETRAIN)
def test_restatement_autograd_reproduces_recorded_gradients(name):
    """tests/test_perturbed_gpu.py takes autograd of the restatement as the gradient reference (the backward kernel; a layer whose
    rows route unlike the fixture); this pins that autograd to the gradients the reference recorded (x.grad and every parameter's),
    under the fixture's own indices.  Bounds: those of tests/test_xmoe_cpu.py -- LLaVA fp32 1e-5 of max|ref|, bf16 1e-3 relative L2
    and 2 bf16 ulp of max|ref|; pretrain fp32 4e-5, bf16 2e-3 relative L2.  The observed figures are printed."""
    fx = load(name)
    llava = name.startswith("llava")
    ps = {k: v.clone() for k, v in fx["state"].items()}
    ps["expert_embeddings"] = P.renorm(ps["expert_embeddings"], fx["meta"]["theta"])
    ps = {k: v.requires_grad_(True) for k, v in ps.items()}
    x = fx["x"].clone().requires_grad_(True)
    if llava:
        out, aux, _ = P.llava_forward(x, ps, fx["meta"], forced_idx=fx["selected_experts"])
        ((out.float() * fx["dy"].float()).sum() + aux.float()).backward()
        bf16 = fx["x"].dtype == torch.bfloat16
        rl, mr = (1e-3, 2 * 2.0 ** -8) if bf16 else (1e-5, 1e-5)
    else:
        out, reg, _ = P.pretrain_forward(x, ps, fx["meta"], forced_idx=fx["selected_experts"])
        ((out.float() * fx["dy"]).sum() + reg.float()).backward()
        rl, mr = (2e-3 if fx["meta"]["bf16"] else 4e-5), None
    got = dict({k: p.grad for k, p in ps.items()}, x=x.grad)
    want = dict(fx["grads"], x=fx["x_grad"])
    for k, g in want.items():
        if g is None:                           # `gate.weight`: the router does not use the plain gate, the reference left no gradient
            assert got[k] is None or float(got[k].abs().max()) == 0.0, k
            continue
        assert got[k] is not None and got[k].dtype == g.dtype and got[k].shape == g.shape, k
        print(f"{name}: d {k} rel-L2 {rel_l2(got[k], g):.2e} max-rel {max_rel(got[k], g):.2e}")
        assert rel_l2(got[k], g) <= rl, (k, rel_l2(got[k], g))
        assert mr is None or max_rel(got[k], g) <= mr, (k, max_rel(got[k], g))
    for k, p in ps.items():
        assert k in want or p.grad is None or float(p.grad.abs().max()) == 0.0, k
    if llava:
        assert want["gate.weight"] is None
